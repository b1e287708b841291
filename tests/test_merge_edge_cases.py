"""The cases of tests/merge_edge_cases.py contain what they are built for -- shown without a GPU.  The Python port of pgm_hash and of
the .fai table build is held against the project's own function (pgm_emul_hash of tests/merge_emul.cpp); every case goes through the
emulator in the device's place inside the driver and through the host route, both against the model byte for byte, and no round is
handed back but in the SEAMS defects and under the --missing of 65 bytes: that entitles tests/test_gpu_merge_edges.py to demand the same
of the device.  The rest are conditions on the cases, from what the generator knows and the model alone: a case that loses its edge
fails here and does not pass quietly on the GPU.  A test here walks all the cases of a set (130 cases in 23 tests) and names every
case that fails in its message."""
import ctypes as C

import numpy as np
import pytest

import merge_edge_cases as MC
from merge_common import run_main
from test_merge_emul import emul, on_emul  # noqa: F401  (fixtures)

from genomics_general_amd import mergegeno

IDS = [name for _, name, _ in MC.ALL]


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    return MC.Store(tmp_path_factory.mktemp("merge_edges"))


def difference(got, want):
    k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    return "first difference in line %d, at byte %d of %d / %d: %r != %r" % (want.count(b"\n", 0, k), k, len(got), len(want),
                                                                            got[max(k - 40, 0):k + 40], want[max(k - 40, 0):k + 40])


def each(names, check, *args):
    """check(name, *args) for every case; the failures of all of them in one message, each under its case's name"""
    failed = []
    assert len(names) >= 1
    for name in names:
        try:
            check(name, *args)
        except AssertionError as exc:
            failed.append("%s: %s" % (name, str(exc)[:800]))
    assert not failed, "%d of %d cases:\n%s" % (len(failed), len(names), "\n".join(failed))


def names_of(cases):
    return [name for name, _ in cases]


def c_hash(emul):                                                 # noqa: F811
    fn = emul.pgm_emul_hash
    fn.restype, fn.argtypes = C.c_uint32, [C.c_char_p, C.c_int64]
    return lambda name: fn(name, len(name))


# ---- the port ----------------------------------------------------------------------------------------------------------------------
def test_the_hash_port_is_pgm_hash(emul):                         # noqa: F811
    h = c_hash(emul)
    rng = np.random.default_rng(20261021)
    names = [b"", b"a", b"\x00", b"\xff" * 200] + [bytes(rng.integers(0, 256, size=int(rng.integers(0, 201)), dtype=np.uint8)) for _ in range(400)]
    for name in names:
        assert MC.name_hash(name) == h(name), name


def test_the_table_port_places_the_twins_names_as_pgm_hash_does(emul, store):   # noqa: F811
    each(["twins_%s_union" % kind for kind in "abcd"], _the_table_is_pgm_hashs, c_hash(emul), store)


def _the_table_is_pgm_hashs(name, h, store):
    _, facts, _ = store.get(name)
    names = [n.encode() for n in facts["fai"]]
    assert MC.build_table(names, h) == facts["table"] == MC.build_table(names)
    assert len(facts["table"]) == MC.table_size(len(names)) and sorted(e for e in facts["table"] if e >= 0) == list(range(len(names)))
    name = (facts["ghost"] or facts["wanted"]).encode()
    assert MC.chain(facts["table"], names, name, h) == (facts["chain"], facts["found"])


# ---- every case through the emulator and the host route ----------------------------------------------------------------------------
def _run(argv, want, monkeypatch, stream, device="1"):
    monkeypatch.setenv("PG_MERGE_DEVICE", device)
    if stream:
        monkeypatch.setenv("PG_STREAM_BYTES", str(stream))
    else:
        monkeypatch.delenv("PG_STREAM_BYTES", raising=False)
    rc, out, err = run_main(argv)
    assert rc == 0, err
    assert out == want, difference(out, want)
    return dict(mergegeno.last_info)


@pytest.mark.parametrize("set_name", list(MC.SETS))
def test_the_emulated_device_and_the_host_route_give_the_models_bytes(set_name, store, on_emul, monkeypatch):   # noqa: F811
    each(names_of(MC.SETS[set_name]), _both_routes_give_the_models_bytes, store, on_emul, monkeypatch)


def _both_routes_give_the_models_bytes(name, store, on_emul, monkeypatch):   # noqa: F811
    argv, facts, want = store.get(name)
    on_emul.devices = on_emul.not_taken = 0
    info = _run(argv, want, monkeypatch, facts["stream"])
    assert on_emul.devices == 1 and info["rounds"] >= 1
    if not facts["device_takes"]:
        assert on_emul.not_taken == 1 and info["rounds_on_device"] == 0
    elif facts["handed_back"]:
        assert info["rounds_on_host"] >= 1 and info["rounds_on_device"] >= 1, info
    else:
        assert on_emul.not_taken == 0 and info["rounds_on_host"] == 0 and info["rounds_on_device"] == info["rounds"], info
    assert info["stopped_files"] == facts["stopped_files"]
    assert info["rounds"] >= facts.get("rounds_at_least", 1), info
    info = _run(argv, want, monkeypatch, facts["stream"], device="0")
    assert info["rounds_on_device"] == 0 and info["stopped_files"] == facts["stopped_files"]


@pytest.mark.parametrize("set_name", MC.STREAMED_SETS)
def test_a_few_lines_a_file_and_round_are_many_rounds_of_the_same_bytes(set_name, store, on_emul, monkeypatch):   # noqa: F811
    each([n for s, n, _ in MC.streamed() if s == set_name], _many_rounds_give_the_same_bytes, store, monkeypatch)


def _many_rounds_give_the_same_bytes(name, store, monkeypatch):
    argv, facts, want = store.get(name)
    info = _run(argv, want, monkeypatch, facts["few_lines_stream"])
    assert info["rounds_on_host"] == 0 and info["rounds_on_device"] == info["rounds"] > 3, info


# ---- conditions on the cases -------------------------------------------------------------------------------------------------------
def test_every_case_writes_more_than_the_header_line(store):
    each(IDS, _writes_more_than_the_header_line, store)


def _writes_more_than_the_header_line(name, store):
    argv, facts, want = store.get(name)
    assert want.count(b"\n") > 1 and want.endswith(b"\n")
    for geo in facts["lines"]:                                    # the steps are the 64-byte steps of the line's length
        assert all(g["steps"] == -(-g["n"] // 64) for g in geo)
    if facts["parts_known"]:                                      # what the generator knows of the files makes up every written line
        for _, head, parts, n in MC.written_parts(facts, want):
            assert head + sum(p[1] for p in parts) == n


def test_names_the_tabs_stand_where_the_case_says(store):
    each([n for n, _ in MC.NAMES], _names_tabs, store)


def _names_tabs(name, store):
    argv, facts, want = store.get(name)
    length = facts["want_t0"]
    mine = [g for geo in facts["lines"] for g in geo if g["t0"] == length]
    assert len(mine) >= 10
    assert {g["steps"] for g in mine} == facts["want_steps"]
    assert facts["want_t1"] <= {g["t1"] for g in mine}
    if facts["want_t1"]:                                          # the second tab in the first byte of a step, in front of and behind it
        assert {g["t1"] % 64 for g in mine} >= {63, 0, 1}
    if length in (60, 62, 63, 124, 127):
        assert any(g["t1"] // 64 == g["t0"] // 64 + 1 for g in mine)                    # the second tab found a step behind the first
    # both names of that length are used, and they differ in their last byte only
    a, b = [n for n in facts["fai"] if len(n) == length and n != "mid"]
    assert a[:-1] == b[:-1] and a != b
    names = [n.encode() for n in facts["fai"]]
    slots, found = MC.chain(MC.build_table(names), names, b.encode())               # ... which a look-up of the second meets on its way
    assert found == facts["fai"].index(b) and a.encode() in [names[MC.build_table(names)[s]] for s in slots[:-1]]
    held = set(k[0] for mine_f in facts["held"] for k in mine_f)
    assert {a, b} <= held
    rows = [r for r in MC.written_parts(facts, want) if r[0] in (a, b)]
    if "_all" in name:                                            # sites no file holds: their heads are rendered from the .fai
        assert sum(all(p[2] for p in parts) for _, _, parts, _ in rows) >= 2
    assert sum(not all(p[2] for p in parts) for _, _, parts, _ in rows) >= 2              # ... and heads copied from the text


def test_width_the_lines_have_the_stated_lengths_and_tabs_on_both_sides_of_every_seam(store):
    each([n for n, _ in MC.WIDTH], _width_lengths_and_tabs, store)


def _width_lengths_and_tabs(name, store):
    argv, facts, want = store.get(name)
    geo = facts["lines"][facts["wide_file"]]
    assert {g["n"] for g in geo} == facts["want_n"] and {g["steps"] for g in geo} == facts["want_steps"] and len(geo) >= 12
    n_cols = facts["n_cells"][facts["wide_file"]] + 2
    assert 32 <= n_cols <= 92 and all(g["ntab"] == n_cols - 1 for g in geo)
    path = argv[1 + 2 * facts["wide_file"]]
    with open(path) as f:
        lines = f.read().split("\n")[1:-1]
    for ln, g in zip(lines, geo):                                 # a tab within two bytes of either side of every seam among the cells
        seams = [seam for seam in range(64, len(ln), 64) if seam > g["t1"] + 2]
        assert name == "width_turn" or len(seams) == (len(ln) - 1) // 64        # (width_turn's long names reach over the first seams)
        for seam in seams:
            assert "\t" in ln[seam - 2:seam] and ("\t" in ln[seam:seam + 2] or len(ln) - seam < 2), (len(ln), seam)
    if name == "width_turn":                                      # all the lengths in turn, twice
        order = [g["n"] for g in geo]
        assert order == 2 * [n for w in (63, 127, 191) for n in (w, w, w + 1, w + 1, w + 2, w + 2)]
    if name == "width_bare":
        bare = 1 - facts["wide_file"]
        assert facts["n_cells"][bare] == 0 and all(g["ntab"] == 1 and g["t1"] is None for g in facts["lines"][bare])


def test_twins_the_table_holds_the_stated_chain(store):
    each([n for n, _ in MC.TWINS], _twins_chain, store)


def _twins_chain(name, store):
    argv, facts, want = store.get(name)
    kind, table, slots = facts["kind"], facts["table"], facts["chain"]
    names = facts["fai"]
    target = facts["ghost"] or facts["wanted"]
    passed = [names[table[s]] for s in slots[:-1]]                # the entries the look-up passes
    assert all(table[s] >= 0 for s in slots[:-1])
    if kind in "ab":
        twin = passed[0]
        at = [k for k in range(len(target)) if twin[k] != target[k]]
        assert len(slots) >= 2 and len(twin) == len(target) >= 66 and len(at) == 1
        assert at[0] >= 64 if kind == "a" else at[0] == 0
        assert MC.name_hash(twin.encode()) & (len(table) - 1) == MC.name_hash(target.encode()) & (len(table) - 1) == slots[0]
        assert names.index(twin) < names.index(target) and facts["found"] == names.index(target)
    elif kind == "c":
        assert slots[0] == len(table) - 1 and slots[1] == 0 and facts["found"] == names.index(target)
        assert len(passed[0]) == len(target)
    else:
        same = [n for n in passed if len(n) == len(target)]
        assert same and facts["found"] == -1 and table[slots[-1]] == -1 and target not in names
        at = [k for k in range(len(target)) if same[0][k] != target[k]]
        assert len(at) == 1 and at[0] >= 64
        with open(argv[1]) as f:
            text = f.read().split("\n")[1:-1]
        where = [k for k, ln in enumerate(text) if ln.startswith(target + "\t")]
        assert len(where) == 1 and where[0] >= len(text) // 2 and facts["lines"][0][where[0]]["t0"] == len(target)
        assert len(facts["held"][0]) == where[0]                  # the file gives its lines in front of it, and no other
    if kind != "d":                                               # the files' sites use the name behind the chain
        assert sum(k[0] == target for mine in facts["held"] for k in mine) >= 20
    assert facts["stopped_files"] == (1 if kind == "d" else 0)


def test_dummy_a_line_holds_the_stated_run_off_the_64_byte_grid(store):
    each([n for n, _ in MC.DUMMY], _dummy_run, store)


def _dummy_run(name, store):
    argv, facts, want = store.get(name)
    g, run = facts["dummy_file"], facts["dummy_run"]
    rows = MC.written_parts(facts, want)
    mine = [parts for _, _, parts, _ in rows if parts[g][2]]
    assert mine and all(p[g][1] == run for p in mine)
    assert any(p[g][0] % 64 != 0 for p in mine)
    assert any(p[g][0] % 64 != 0 and not p[0][2] for p in mine)   # ... behind the held cells of the file in front
    if "_all" in name:                                            # every file a dummy
        assert any(all(x[2] for x in p) and p[g][0] % 64 != 0 for p in mine)
    per = 1 + facts["missing_len"]
    assert run == facts["n_cells"][g] * per and (facts["n_cells"][g], facts["missing_len"]) in MC.DUMMY_RUNS + ((2, 65),)
    # the run itself, in the model's bytes
    missing = argv[argv.index("--missing") + 1] if "--missing" in argv else "N"
    assert (("\t" + missing) * facts["n_cells"][g] + "\n").encode() in want


def test_cells_a_line_holds_the_stated_part_in_its_file_position(store):
    each([n for n, _ in MC.CELLS], _cells_part, store)


def _cells_part(name, store):
    argv, facts, want = store.get(name)
    g, part = facts["part_file"], facts["part"]
    rows = MC.written_parts(facts, want)
    mine = [parts for _, _, parts, _ in rows if not parts[g][2]]
    assert len(mine) >= 5 and all(p[g][1] == part for p in mine)
    assert any(p[g][2] for _, _, p, _ in rows)                     # ... and lines the file does not hold
    assert b"\t" not in want and want.count(b",") > want.count(b"\n")


def test_digits_every_digit_count_is_rendered_from_the_fai(store):
    each([n for n, _ in MC.DIGITS], _digits_rendered, store)


def _digits_rendered(name, store):
    argv, facts, want = store.get(name)
    rows = want.decode().split("\n")[1:-1]
    assert len(rows) == MC.DIGITS_LEN
    held = set(k[1] for mine in facts["held"] for k in mine)
    for nd in range(1, 7):
        free = [p for p in range(10 ** (nd - 1), min(10 ** nd, MC.DIGITS_LEN + 1)) if p not in held]
        assert len(free) >= 4, nd                                     # (the first and the last of them stand next to the changes)
        assert all(rows[p - 1] == "chr\t%d\tN\tN\tN" % p for p in free)
    assert sum(len(str(p)) != len(str(p - 1)) or len(str(p)) != len(str(p + 1)) for p in held) >= 4     # files hold sites at the changes
    assert held & {MC.DIGITS_LEN - 1, MC.DIGITS_LEN}
    if facts["stream"]:                                           # rounds of 1000 positions: the last of a round the first of a digit count
        assert facts["stream"] // 29 == MC.DIGITS_ROUND and all(p % MC.DIGITS_ROUND == 0 for p in (1000, 10000, 100000))


def test_seams_the_defect_stands_on_its_byte_and_the_twin_is_regular(store):
    each([n for n, _ in MC.SEAMS if n.endswith("defect")], _seams_defect, store)


def _seams_defect(name, store):
    argv, facts, _ = store.get(name)
    _, twin_facts, _ = store.get(name.replace("defect", "twin"))
    kind, d = facts["seam"]
    line, twin = facts["special_line"], twin_facts["special_line"]
    assert len(line) == len(twin) and [k for k in range(len(line)) if line[k] != twin[k]] == [d]
    if kind == "dtab":
        assert line[d - 1:d + 1] == "\t\t" and line[d - 2] != "\t" and line[d + 1] != "\t" and d % 64 == 0
    elif kind == "trail":
        assert line[-1] == "\t" and len(line) - 1 == d and line[-2] != "\t"
    else:
        assert line[d] == " " and "\t" not in line[d - 1:d + 2]
    assert sum(c == " " or (c == "\t" and (k == len(line) - 1 or line[k + 1] == "\t")) for k, c in enumerate(line)) == 1   # one defect
    n_cols = twin_facts["n_cells"][1] + 2
    assert twin.count("\t") == n_cols - 1 and "\t\t" not in twin and " " not in twin and not twin.endswith("\t")
    f, at = facts["special"]                                      # in the second half of its file, several rounds in
    geo = facts["lines"][f]
    assert at >= len(geo) // 2 and geo[at]["n"] == len(line)
    before = sum(g["n"] + 1 for g in geo[:at])
    assert before > 3 * facts["stream"] // 2 and facts["stream"] == twin_facts["stream"]
    for x, (a, b) in enumerate(zip(argv[1:4:2], store.get(name.replace("defect", "twin"))[0][1:4:2])):
        with open(a) as fa, open(b) as fb:
            ta, tb = fa.read(), fb.read()
        assert len(ta) == len(tb) and sum(p != q for p, q in zip(ta, tb)) == (1 if x == f else 0)


def test_lines_both_files_hold_exactly_the_stated_lines(store):
    each([n for n, _ in MC.LINES], _lines_count, store)


def _lines_count(name, store):
    argv, facts, want = store.get(name)
    assert [len(geo) for geo in facts["lines"]] == [facts["n_lines"]] * 2 and want.count(b"\n") == facts["n_lines"] + 1
