"""-m gpu: the device tokenizer's kernels (csrc/pg_tokenize.hip) against the case table of tests/tok_cases.py -- texts drawn cell by
cell together with the rows, positions and scaffold runs they must give, no parser involved -- at every route of pg_plan_tok
(csrc/pg_tok_plan.h; tests/test_host.py shows which case takes which kernel): k_tok_cells3<DIPLO | PHASED | PAIRS, 0 .. 4> with column
counts on both sides of every multiple of 64 and line counts on both sides of a wavefront's 16 and a block's 64 lines, k_tok_cells
with wide cells, k_tok_parse at the sizes that are its own, k_tok_heads across its 256-line seam and with heads of 63, 64 and 65
bytes, lines shorter than a head load, every byte 33 .. 255 as an allele.  Everything is an integer: every comparison is exact."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from genomics_general_amd import genoio, synth
from genomics_general_amd.engine import Engine
from genomics_general_amd.samples import HapLayout, SampleData

import tok_cases as TC

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def run_cases(specs):
    e = Engine(0)
    try:
        for sp in specs:
            TC.check_on_device(e, TC.build(sp))
    finally:
        e.close()
    return len(specs)


@pytest.mark.parametrize("layout", TC.LAYOUTS)
@pytest.mark.parametrize("family", TC.FAMILIES)
def test_every_column_and_line_count(family, layout):
    """1 .. 600 columns x 1 .. 65 lines: k_tok_cells3 with NIT 1, 2, 3, 4 and 0, its clamp where the columns are no multiple of
    64, its row-clear and row-store loops with one trip and with several"""
    assert run_cases(TC.grid(families=(family,), layouts=(layout,))) == len(TC.COLS) * len(TC.LINES)


def test_scaffold_runs_across_the_seam_of_k_tok_heads():
    """255, 256, 257 and 513 lines: a scaffold change right at, before and behind the seam of two 256-line blocks, none across it,
    names that begin with each other in both orders"""
    assert run_cases(TC.seam()) == 48


def test_heads_of_63_64_65_bytes_positions_and_lines_shorter_than_a_head():
    assert run_cases(TC.heads()) == 8


def test_wide_cells_take_the_general_kernel():
    """phased ploidy 3 and 26, pairs ploidy 4 and 5, an unwanted column of seven characters beside narrow wanted cells"""
    assert run_cases(TC.general()) == 80


def test_layouts_that_change_the_route_by_their_size():
    """haplo columns on both sides of k_tok_cells3's LDS limit (k_tok_cells behind it), diploid phased columns on both sides of
    k_tok_cells' (k_tok_parse + k_nib_pack behind it)"""
    assert run_cases(TC.by_size()) == 5


@pytest.mark.parametrize("base", range(8))
def test_defective_twins_are_refused_and_the_engine_stays_right(base):
    """a base per route (tok_cases.refusal_bases) and its twins with one defect each -- a short cell, a doubled tab, a blank inside a
    cell, a letter for a separator, at columns 0, 63, 64 and the last in rows 0, 15, 16 and the last; a 19-digit position, a `#`
    line --: tokenize_text returns None, and the regular text tokenized right afterwards on the same engine gives its rows"""
    c = TC.build(TC.refusal_bases()[base])
    e = Engine(0)
    e.set_layout(c.lay)
    e.reserve(37 + c.n_lines + 11)
    TC.check_on_device(e, c, set_layout=False)
    n = 0
    for label, kind, col, text in TC.twins(c):
        got = e.tokenize_text(text, row_offset=37, n_rows=text.count(b"\n"), at_most=True)
        assert got is None, (c.name, label)
        TC.check_on_device(e, c, set_layout=False)
        n += 1
    e.close()
    assert n >= 30


FORCED = r"""
import os, sys
sys.path.insert(0, os.getcwd())
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import tok_cases as TC
from genomics_general_amd.engine import Engine
import time
t0 = time.time()
e = Engine(0)
specs = TC.reduced() + TC.heads()
cases = [TC.build(sp) for sp in specs]
t1 = time.time()
for c in cases:
    TC.check_on_device(e, c)
e.close()
print("ok %d (cases drawn in %.2f s, tokenized and compared in %.2f s)" % (len(specs), t1 - t0, time.time() - t1))
"""


@pytest.mark.parametrize("switch", ["PG_TOK_PARSE=1", "PG_TOK_PARSE=2", "PG_TOK_CELLS_REGS=0"])
def test_forced_forms_in_processes_of_their_own(switch):
    """the switches are read once per process: a fresh one per switch (started before this process touches the device in this
    test) takes the reduced table -- all column counts and formats, 1, 17 and 65 lines -- and the heads through k_tok_parse +
    k_nib_pack, k_tok_cells and k_tok_cells3<FMT, 0>"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PG_TOK_")}
    name, _, val = switch.partition("=")
    env[name] = val
    r = subprocess.run([sys.executable, "-c", FORCED], cwd=ROOT, env=env, capture_output=True, text=True, timeout=600)
    print(switch, r.stdout.strip())
    assert r.returncode == 0 and "ok %d " % (len(TC.reduced()) + 8) in r.stdout, r.stdout[-2000:] + r.stderr[-3000:]


def test_three_steps_with_alternating_slots_and_a_change_of_layout():
    """tokenize_submit / _parse / _collect the way the drivers run them (parse(k) -> submit(k + 1) -> collect(k), slots alternating):
    four blocks of different lengths at 200 columns, then the same slots with a 65-column layout (the column tables are kept per
    slot)"""
    e = Engine(0)
    for n_cols, lengths in ((200, (65, 1, 300, 17)), (65, (16, 130))):
        blocks = [TC.build(TC.grid_spec("phased2", "all", n_cols, n, "-step%d" % k)) for k, n in enumerate(lengths)]
        lay = blocks[0].lay
        assert all(np.array_equal(b.lay.col_slot, lay.col_slot) for b in blocks)
        e.set_layout(lay)
        total = sum(lengths)
        e.reserve(5 + total + 7)
        e.upload(np.full((5 + total + 7, lay.n_hap), TC.SENTINEL, dtype=np.int8), 0)
        at = [5 + sum(lengths[:k]) for k in range(len(lengths))]
        got = [None] * len(blocks)
        assert e.tokenize_submit(blocks[0].text, 0)
        for k, b in enumerate(blocks):
            assert e.tokenize_parse(k % 2, at[k], b.n_lines) == b.n_lines
            if k + 1 < len(blocks):
                assert e.tokenize_submit(blocks[k + 1].text, (k + 1) % 2)
            got[k] = e.tokenize_collect(k % 2, b.text, b.n_lines)
        rows = e.download(0, 5 + total + 7)
        for k, b in enumerate(blocks):
            assert got[k] is not None, b.name
            n, pos, run_starts, run_names = got[k]
            assert n == b.n_lines and np.array_equal(pos, b.pos) and np.array_equal(run_starts, b.run_starts) and list(run_names) == b.run_names, b.name
            assert np.array_equal(rows[at[k]:at[k] + b.n_lines], b.rows), b.name
        assert (rows[:5] == TC.SENTINEL).all() and (rows[5 + total:] == TC.SENTINEL).all()
    e.close()


def test_pair_counts_read_the_tokenized_rows_as_they_read_uploaded_ones():
    """a layout of 97 slots (n_hap % 16 != 0: the last dword of a row holds pad nibbles the pair kernels read): pairCounts on the
    tokenized rows == pairCounts on the same rows uploaded as int8"""
    c = TC.build(TC.grid_spec("phased12", "shuf", 97, 300, "-pairs"))
    order = c.lay.ind_order
    half = len(order) // 2
    sd = SampleData(indNames=list(order), popNames=["p0", "p1"], popInds=[order[:half], order[half:]], ploidyDict=dict(c.lay.sampleData.ploidy))
    lay = HapLayout(sd, ["s%d" % k for k in range(c.n_cols)], "phased")
    assert np.array_equal(lay.col_slot, c.lay.col_slot) and lay.n_hap % 16 != 0
    c.lay = lay
    e = Engine(0)
    TC.check_on_device(e, c)
    wins = [(37, 37 + 300), (40, 37 + 257)]
    D, C = e.batch([w[0] for w in wins], [w[1] for w in wins]).pairCounts(reference_order=True)
    e.close()
    e2 = Engine(0)
    e2.set_layout(lay)
    e2.load_sites(c.rows)
    D2, C2 = e2.batch([w[0] - 37 for w in wins], [w[1] - 37 for w in wins]).pairCounts(reference_order=True)
    e2.close()
    assert np.array_equal(D, D2) and np.array_equal(C, C2) and C.max() > 0 and D.max() > 0


def test_a_200_column_bgzf_file_through_the_driver(tmp_path, monkeypatch, capfd):
    """popgenWindows.py on a bgzipped file of 200 diploid columns (k_tok_cells3<PHASED, 4>, the members inflated on the device),
    2400 sites on two scaffolds, in several blocks: the oracle's output, every block tokenized on the device"""
    import oracle_cli
    import test_gpu_golden as G
    from golden_util import align_columns
    n_dip, n_pops, per_scaf = 200, 4, 1200
    names = ["s%d" % d for d in range(n_dip)]
    plain = str(tmp_path / "wide.geno")
    with open(plain, "wb") as f:
        for k in range(2):
            codes = synth.gen_codes(777, np.full(per_scaf, k, dtype=np.int64), np.arange(1, per_scaf + 1), n_dip, n_pops, var_thr=6500, miss_thr=2000)
            part = plain + ".part"
            synth.write_geno_fast(part, codes, names, "scaf%d" % (k + 1), 1)
            with open(part, "rb") as g:
                if k:
                    g.readline()
                f.write(g.read())
            os.remove(part)
    with open(plain, "rb") as f:
        text = f.read()
    packed = str(tmp_path / "wide.geno.gz")
    with genoio.BgzfWriter(packed) as w:
        w.write(text)
    per = n_dip // n_pops
    argv = ["-f", "phased", "-w", "300", "-m", "40", "--roundTo", "6", "--analysis", "popDist", "popPairDist"]
    for k in range(n_pops):
        argv += ["-p", "p%d" % k, ",".join(names[k * per:(k + 1) * per])]
    want = oracle_cli.run("popgenWindows.py", ["-g", plain] + argv)
    monkeypatch.setenv("PG_TIMING", "1")
    monkeypatch.setenv("PG_STREAM_BYTES", str(400000))
    out = str(tmp_path / "out.csv")
    G.MAINS["popgenWindows.py"](["-g", packed] + argv + ["-o", out])
    with open(out) as f:
        got = f.read()
    assert len(want.splitlines()) >= 8
    assert G.compare_text(align_columns(got, want), want, 6) == 0
    tm = [json.loads(ln[len("PG_TIMING "):]) for ln in capfd.readouterr().err.splitlines() if ln.startswith("PG_TIMING ")]
    assert tm and tm[-1].get("device_tokenizer") == 1 and tm[-1]["host_tokenized_blocks"] == 0, tm
