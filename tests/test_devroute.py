"""devroute.run_blocks, the block pipeline the per-line drivers share, driven by a fake device that records its calls: the order
"submit k+1, then collect k", the host route, carry, the \\r rule, the cut hook, an early end, spans.  No library, no GPU."""
import threading

import pytest

from genomics_general_amd import devroute

T = [b"a\t1\tx\nb\t2\ty\n", b"c\t3\tz\n", b"d\t4\tw\ne\t5\tv\n", b"f\t6\tu\n", b"g\t7\tt\n"]


class Span:
    """what devroute.is_span takes for a genoio.BgzfSpan: .tab and a length; nothing may look at its text"""

    def __init__(self, n):
        self.tab, self.n = (), n

    def __len__(self):
        return self.n


class Fake:
    """records (call, block) in .log; a ticket is ("ticket", block), a result ("result", block)"""

    def __init__(self, bad=None, code=3, exc=None):
        self.log, self.bad, self.code, self.exc = [], bad, code, exc

    def submit(self, block):
        self.log.append(("submit", block))
        return ("ticket", block)

    def collect(self, ticket):
        assert ticket[0] == "ticket"
        self.log.append(("collect", ticket[1]))
        return ("result", ticket[1])

    def finish(self, result):
        assert result[0] == "result"
        self.log.append(("finish", result[1]))
        if result[1] == self.bad:
            if self.exc:
                raise self.exc
            return self.code
        return None

    def host(self, text, n_lines):
        self.log.append(("host", text, n_lines))
        return None

    def of(self, call):
        return [e[1] for e in self.log if e[0] == call]


def run(blocks, dev, fake=None, ahead=False, **kw):
    fake = fake or dev
    info = dict(blocks=0, blocks_inflated_on_device=0)
    it = iter(list(blocks) + [b""])
    if ahead:
        it = devroute.read_ahead(it, "pg-test-read")
    rc = devroute.run_blocks(it, dev, info, fake.finish, fake.host, **kw)
    return rc, info


def test_a_block_is_submitted_before_the_one_before_it_is_collected():
    d = Fake()
    rc, info = run(T[:4], d)
    assert rc == 0 and info == dict(blocks=4, blocks_inflated_on_device=0)
    assert d.log == [("submit", T[0]),
                     ("submit", T[1]), ("collect", T[0]), ("finish", T[0]),
                     ("submit", T[2]), ("collect", T[1]), ("finish", T[1]),
                     ("submit", T[3]), ("collect", T[2]), ("finish", T[2]),
                     ("collect", T[3]), ("finish", T[3])]          # the last one when the input has ended


def test_closures_stand_in_for_the_devices_own_submit_and_collect():
    d, mine = Fake(), Fake()
    rc, _ = run(T[:3], d, submit=mine.submit, collect=mine.collect)
    assert rc == 0 and d.of("submit") == [] and d.of("collect") == [] and d.of("finish") == T[:3]
    assert mine.log == [("submit", T[0]), ("submit", T[1]), ("collect", T[0]), ("submit", T[2]), ("collect", T[1]), ("collect", T[2])]


def test_without_a_device_every_block_is_the_hosts():
    f = Fake()
    rc, info = run(T[:4], None, f)
    assert rc == 0 and info["blocks"] == 4
    assert f.log == [("host", T[0], 2), ("host", T[1], 1), ("host", T[2], 2), ("host", T[3], 1)]
    f = Fake()
    run([b"a\t1\tx\nb\t2\ty"], None, f)                            # a last line without its line feed counts
    assert f.log == [("host", b"a\t1\tx\nb\t2\ty", 2)]


def test_a_non_zero_code_from_the_host_route_ends_the_run():
    f = Fake()
    f.host = lambda text, n: f.log.append(("host", text, n)) or (2 if text == T[1] else None)
    rc, info = run(T[:4], None, f)
    assert rc == 2 and info["blocks"] == 2 and [e[1] for e in f.log] == T[:2]


def test_carry_stands_in_front_of_the_first_block_only():
    d = Fake()
    rc, info = run(T[:3], d, carry=b"h\t0\t")
    assert rc == 0 and info["blocks"] == 3
    assert d.of("submit") == [b"h\t0\t" + T[0], T[1], T[2]] == d.of("finish")


@pytest.mark.parametrize("with_dev", [True, False])
def test_carry_before_an_immediate_end_is_still_finished(with_dev):
    d = Fake()
    rc, info = run([], d if with_dev else None, d, carry=b"h\t0\tq\n")
    assert rc == 0 and info["blocks"] == 1
    assert d.log == ([("submit", b"h\t0\tq\n"), ("collect", b"h\t0\tq\n"), ("finish", b"h\t0\tq\n")] if with_dev else [("host", b"h\t0\tq\n", 1)])


def test_no_input_and_no_carry_is_no_block():
    d = Fake()
    rc, info = run([], d)
    assert rc == 0 and info["blocks"] == 0 and d.log == []


def test_from_a_carriage_return_on_the_rest_is_the_hosts_in_one_piece():
    blocks = [T[0], b"c\t3\tz\r\n", T[2], T[3]]
    d = Fake()
    rc, info = run(blocks, d, universal=True)
    rest = b"".join(blocks[1:])
    assert rc == 0 and info["blocks"] == 2
    assert d.log == [("submit", T[0]), ("collect", T[0]), ("finish", T[0]), ("host", rest, rest.count(b"\n"))]
    d = Fake()
    rc, info = run(blocks, d, universal=False)                     # (a driver that takes \r elsewhere)
    assert rc == 0 and info["blocks"] == 4 and d.of("submit") == blocks == d.of("finish") and d.of("host") == []


def test_a_carriage_return_in_the_carry_counts():
    d = Fake()
    rc, info = run(T[:2], d, universal=True, carry=b"h\r")
    assert rc == 0 and info["blocks"] == 1 and d.log == [("host", b"h\r" + T[0] + T[1], 3)]


def hold_last_line(seen):
    def cut(data, lines_before, eof):
        seen.append((data, lines_before, eof))
        if eof:
            return data, b""
        at = data.rfind(b"\n", 0, len(data) - 1) + 1
        return data[:at], data[at:]
    return cut


def test_cut_holds_the_tail_of_a_block_back_for_the_next():
    d, seen = Fake(), []
    rc, info = run(T[:4], d, cut=hold_last_line(seen))
    # T[0] gives its first line; its second joins T[1], which as two lines gives one; ...; the end hands the last line on
    want = [b"a\t1\tx\n", b"b\t2\ty\n", b"c\t3\tz\nd\t4\tw\n", b"e\t5\tv\n", b"f\t6\tu\n"]
    assert rc == 0 and d.of("submit") == want == d.of("finish") and info["blocks"] == 5
    assert b"".join(want) == b"".join(T[:4])
    assert [(s[1], s[2]) for s in seen] == [(0, False), (1, False), (2, False), (4, False), (5, True)]
    assert seen[1][0] == b"b\t2\ty\n" + T[1] and seen[-1][0] == b"f\t6\tu\n"      # the held text in front; at the end only it


def test_cut_counts_the_hosts_lines_too():
    f, seen = Fake(), []
    run(T[:3], None, f, cut=hold_last_line(seen))
    assert [s[1] for s in seen] == [0, 1, 2, 4] and [e[2] for e in f.log] == [1, 1, 2, 1]


def test_a_cut_that_holds_a_whole_block_back_submits_nothing_for_it():
    d = Fake()
    cut = lambda data, before, eof: (data, b"") if eof or data.count(b"\n") >= 3 else (b"", data)     # noqa: E731
    rc, info = run(T[:4], d, cut=cut)
    assert rc == 0 and d.of("submit") == [T[0] + T[1], T[2] + T[3]] == d.of("finish") and info["blocks"] == 2
    assert b"" not in d.of("submit")


@pytest.mark.parametrize("exc", [None, SystemExit(1)])
def test_a_non_zero_finish_ends_the_run_and_the_reader(exc):
    d = Fake(bad=T[1], code=3, exc=exc)
    before = set(threading.enumerate())
    if exc:
        with pytest.raises(SystemExit):
            run(T, d, ahead=True)
    else:
        rc, info = run(T, d, ahead=True)
        assert rc == 3 and info["blocks"] == 3
    assert d.of("submit") == T[:3]                                 # block 3 was in flight when block 2 was finished; none behind it
    assert d.of("finish") == T[:2] and d.of("collect") == T[:2]
    assert not [t for t in set(threading.enumerate()) - before if t.name == "pg-test-read"]


def test_the_reader_has_ended_after_a_whole_run_too():
    before = set(threading.enumerate())
    rc, _ = run(T, Fake(), ahead=True)
    assert rc == 0 and not [t for t in set(threading.enumerate()) - before if t.name == "pg-test-read"]


def test_a_non_zero_finish_of_the_last_block_is_returned():
    d = Fake(bad=T[2], code=2)
    rc, _ = run(T[:3], d)
    assert rc == 2 and d.of("finish") == T[:3]


def test_spans_are_submitted_unopened_and_counted():
    spans = [Span(10), Span(20), Span(30)]
    d = Fake()
    rc, info = run(spans + [Span(0), Span(40)], d, universal=True, carry=b"")      # an empty span is the end
    assert rc == 0 and info == dict(blocks=3, blocks_inflated_on_device=3)
    assert d.log == [("submit", spans[0]),
                     ("submit", spans[1]), ("collect", spans[0]), ("finish", spans[0]),
                     ("submit", spans[2]), ("collect", spans[1]), ("finish", spans[1]),
                     ("collect", spans[2]), ("finish", spans[2])]


def test_an_empty_text_block_ends_a_run_of_spans():
    spans = [Span(10), Span(20)]
    d = Fake()
    rc, info = run(spans, d)                                       # (run appends b"")
    assert rc == 0 and info["blocks"] == 2 and d.of("finish") == spans


def test_field_at_reads_in_growing_pieces():
    text = b"x" * 700 + b"\tafter\n"
    asked = []

    def text_at(a, k):
        asked.append(k)
        return text[a:a + k]
    assert devroute.field_at(text_at, 100) == b"x" * 600 and asked == [64, 256, 1024]
    assert devroute.field_at(lambda a, k: b"scaf\t12\tA/A\n"[a:a + k], 0) == b"scaf"


def test_exits_write_one_line_and_carry_their_status(capsys):
    class U(devroute.Usage):
        prog = "tool.py"

    class S(devroute.Stop):
        prog = "tool.py"
    assert U("no -f").code == 2 and S("line 3: bad").code == 1
    assert capsys.readouterr().err == "tool.py: no -f\ntool.py: line 3: bad\n"
    assert not issubclass(S, devroute.Usage) and issubclass(U, SystemExit)


def test_report_publishes_and_writes_the_timing_line(capsys, monkeypatch):
    last = {"stale": 1}
    monkeypatch.delenv("PG_TIMING", raising=False)
    devroute.report(last, {"b": 2, "a": 1.5}, "x")
    assert last == {"b": 2, "a": 1.5} and capsys.readouterr().err == ""
    monkeypatch.setenv("PG_TIMING", "1")
    devroute.report(last, {"b": 2, "a": 1.5}, "x")
    assert capsys.readouterr().err == "PG_TIMING x a=1.5 b=2\n"
