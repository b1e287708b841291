"""The windowStats.py drop-in's device route (pg_ws_dev.hip: k_ws_lines, k_ws_stats) on an MI355X.

Every golden of the unmodified reference, byte for byte, from plain, gzip and BGZF input (members inflated on the device), in one block
and in small blocks, with PG_TIMING's counters showing who parsed the blocks -- k_ws_lines those of the regular spelling, the host route
the blocks handed back (the HOST_BLOCKS goldens: the same bytes) -- and that the device computed the cells.  Then device against host
route (PG_WS_DEVICE=0: pg_ws_text, std::sort and the same core arithmetic, held to NumPy bit for bit by tests/test_wstats_cpu.py),
bytes equal, on seeded tables at the smallest shapes where either kernel can go wrong.  Parse: 1, 63, 64, 65 and 129 value columns (the
lanes' stride); a cell of 15 against 16 digits and an exponent of 22 against 23, each flipping the one block to the host; runs of blanks
as separators; positions across 2^31; '#' lines, scaffold changes and runs that go on across block seams; a short line, a long line, a
position and a cell of another spelling and a carriage return, each handing exactly its block back.  Statistics: non-nan counts per
window on both sides of the sum's 8 and 128 and of the 256 sites a workgroup reads at a time; with PG_WS_LDS_VALS=256 counts of 255,
256, 257 and 1000 (the sort in LDS, the radix select, and their boundary) and one window of the default capacity + 1, which is also
one value past the 8192 of a summation piece; equal values, two distinct values, mixed signs, subnormals, inf, neighbours that differ
in the last bit, nan in the first and last place, ranks where q (n - 1) is an integer and interpolation weights on both sides of 0.5,
overlapping windows, 3000 windows of one site, a -0.0 among the cells of a `sum`-only run.  The jobs of a test run in one process of
their own under a time limit (tests/wstats_runner.py)."""
import gzip
import json
import os
import random
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from wstats_cases import ALL, CASES, DEVICE, HOST_BLOCKS, NOTHING, fixture_path, golden  # noqa: E402

pytestmark = pytest.mark.gpu

BY_NAME = {c[0]: c for c in CASES}
LDS_DEFAULT = 8192


def run_jobs(jobs, tmp_path, timeout=120):
    """jobs: [(argv without -o, env)] -> [(output bytes, exit status, counters, stderr)], all in one process"""
    spec = []
    for k, (argv, env) in enumerate(jobs):
        spec.append({"argv": list(argv) + ["-o", str(tmp_path / ("out%d.csv" % k))], "env": dict(env)})
    jp, rp = str(tmp_path / "jobs.json"), str(tmp_path / "results.json")
    with open(jp, "w") as f:
        json.dump(spec, f)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "wstats_runner.py"), jp, rp], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    with open(rp) as f:
        results = json.load(f)
    out = []
    for k, res in enumerate(results):
        path = str(tmp_path / ("out%d.csv" % k))
        data = b""
        if os.path.exists(path):
            with open(path, "rb") as f:
                data = f.read()
        out.append((data, res["status"], res["info"], res["stderr"]))
    return out


def _source(fixture, source, tmp_path):
    """the fixture as plain text, as one gzip stream, or as bgzip's BGZF members"""
    from genomics_general_amd import genoio
    inp = fixture_path(fixture)
    if source == "plain":
        return inp
    with open(inp, "rb") as f:
        text = f.read()
    p = str(tmp_path / ("%s_%s.tsv.gz" % (fixture, source)))
    if not os.path.exists(p):
        with open(p, "wb") as g:
            g.write(bytes(genoio.bgzf_compress(text, block=700)) if source == "bgzf" else gzip.compress(text))
    return p


DEV = {"PG_WS_DEVICE": "1"}
HOST = {"PG_WS_DEVICE": "0"}


@pytest.mark.parametrize("source,block", [("plain", None), ("plain", 300), ("gz", None), ("gz", 300), ("bgzf", None), ("bgzf", 300)])
def test_device_route_reproduces_the_reference(source, block, tmp_path):
    env = dict(DEV, **({"PG_STREAM_BYTES": str(block)} if block else {}))
    names = [n for n, _, _, _ in CASES]
    jobs = []
    for name in names:
        _, fixture, argv, _ = BY_NAME[name]
        jobs.append(([a.replace("@G", GOLD) for a in argv] + ["-i", _source(fixture, source, tmp_path)], env))
    for name, (data, status, info, err) in zip(names, run_jobs(jobs, tmp_path)):
        assert status == 0, (name, err)
        assert data == golden(name), name
        if name in DEVICE or name in HOST_BLOCKS:
            assert info["device_cells"] >= 1 and info["host_cells"] == 0, (name, info)
            assert info["device_lds_cells"] + info["device_big_cells"] <= info["device_cells"], (name, info)
            assert (info["cells_through_float"] > 0) == (name in HOST_BLOCKS), (name, info)
        else:
            assert name in NOTHING and info["device_cells"] == 0, (name, info)
        # who parsed the lines: k_ws_lines every block of the regular spelling, the host route the blocks it hands back
        if BY_NAME[name][1] != "header_only":
            assert info["device_blocks"] >= 1, (name, info)
            assert (info["device_host_blocks"] > 0) == (name in HOST_BLOCKS), (name, info)
            assert info["device_host_blocks"] <= info["device_blocks"], (name, info)
        if source == "bgzf" and BY_NAME[name][1] in ("main", "headerless"):
            assert info["blocks_inflated_on_device"] >= 1, (name, info)
        if block and source != "bgzf" and BY_NAME[name][1] == "main":       # (a span of members is not cut below the reader's own unit)
            assert info["blocks"] > 3, (name, info)


def _both(inp, argv, tmp_path, env=None, timeout=120):
    """host route, then device route, in one process: equal bytes, equal exit status; the device's counters"""
    (want, ws, _, _), (got, gs, info, err) = run_jobs([(argv + ["-i", inp], HOST), (argv + ["-i", inp], dict(DEV, **(env or {})))], tmp_path,
                                                     timeout=timeout)
    assert gs == ws, err
    assert got == want
    assert len(want) > len("scaffold,start,end,mid,sites")
    return got, gs, info, err


def _number(R):
    kind = R.random()
    if kind < 0.3:
        return str(R.randint(-1000, 1000))
    if kind < 0.8:
        return "%.*f" % (R.randint(1, 9), R.uniform(-100, 100))
    return "%.5e" % R.uniform(-1e8, 1e8)


def _table(path, windows, n_cols=1, seed=1, width=100000, cell=None):
    """coordinate windows of `width` bases on one scaffold; windows[k] = the cells of window k's sites: a list of strings per site (one
    per column), or a count c, which stands for c numbers between a nan in the first and in the last place"""
    R = random.Random(seed)
    cell = cell or _number
    rows = ["\t".join(["scaffold", "position"] + ["v%d" % k for k in range(n_cols)])]
    for k, w in enumerate(windows):
        if isinstance(w, int):
            w = [["nan"] * n_cols] + [[cell(R) for _ in range(n_cols)] for _ in range(w)] + [["nan"] * n_cols]
        for j, cells in enumerate(w):
            rows.append("\t".join(["s1", str(k * width + 1 + j)] + list(cells)))
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return path


NO_MINMAX = [s for s in ALL if s not in ("min", "max")]


@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 129])
def test_columns_at_the_edges_of_a_wave(n_cols, tmp_path):
    inp = _table(str(tmp_path / "t.tsv"), [5, 9, 130, 1, 40], n_cols=n_cols, seed=n_cols)
    _, _, info, _ = _both(inp, ["-w", "100000", "--stats"] + ALL, tmp_path)
    assert info["device_cells"] == 5 * n_cols and info["device_lds_cells"] == 5 * n_cols, info
    assert info["device_blocks"] == 1 and info["device_host_blocks"] == 0, info           # (the lanes' stride over the columns)


def test_counts_around_the_sums_eight_and_128(tmp_path):
    counts = [1, 2, 3, 7, 8, 9, 127, 128, 129, 253, 254, 255, 256, 257]       # (+ 2 nan: 256 sites a step of the workgroup's walk)
    inp = _table(str(tmp_path / "t.tsv"), counts, n_cols=2, seed=7)
    got, _, info, _ = _both(inp, ["-w", "100000", "--stats"] + ALL, tmp_path)
    assert got.count(b"\n") == len(counts) + 1 and info["device_big_cells"] == 0, info


def test_a_column_without_a_value(tmp_path):
    inp = _table(str(tmp_path / "t.tsv"), [3, 0, 4], n_cols=2, seed=3)
    got, status, _, _ = _both(inp, ["-w", "100000", "--stats"] + NO_MINMAX, tmp_path)
    assert status == 0 and b",nan,nan,nan,0.0," in got.split(b"\n")[2]
    got, status, _, err = _both(inp, ["-w", "100000", "--stats"] + ALL, tmp_path)          # min / max of nothing: both stop at window 2
    assert status == 1 and got.count(b"\n") == 2 and "window 2" in err and "min / max" in err


def test_both_tiers_and_their_boundary_on_small_windows(tmp_path):
    counts = [255, 256, 257, 1000, 3]
    inp = _table(str(tmp_path / "t.tsv"), counts, n_cols=2, seed=11)
    _, _, info, _ = _both(inp, ["-w", "100000", "--stats"] + ALL, tmp_path, env={"PG_WS_LDS_VALS": "256"})
    assert info["device_lds_cells"] == 3 * 2 and info["device_big_cells"] == 2 * 2, info
    _, _, info, _ = _both(inp, ["-w", "100000", "--stats", "mean", "sd", "sum", "min", "max"], tmp_path, env={"PG_WS_LDS_VALS": "256"})
    assert info["device_lds_cells"] == 0 and info["device_big_cells"] == 0, info            # (no order statistic: no tier)


def test_one_value_past_the_default_capacity(tmp_path):
    inp = _table(str(tmp_path / "t.tsv"), [LDS_DEFAULT + 1, LDS_DEFAULT, 20], n_cols=1, seed=13)
    _, _, info, _ = _both(inp, ["-w", "100000", "--stats"] + ALL, tmp_path)
    assert info["device_big_cells"] == 1 and info["device_lds_cells"] == 2, info


def _special(path):
    import numpy as np
    tiny = 5e-324
    x = 1.0 + 2.0 ** -30
    near = [repr(float(v)) for v in (x, np.nextafter(x, 2.0), np.nextafter(x, 0.0), np.nextafter(np.nextafter(x, 2.0), 2.0))]
    windows = [
        [["2.5"]] * 9,                                                       # all values equal
        [["1"], ["7"], ["1"], ["7"], ["7"], ["1"], ["1"]],                   # two distinct values
        [["-3.5"], ["4"], ["-1e-3"], ["2e5"], ["0"], ["-77"], ["12.25"], ["-0.125"]],      # mixed signs
        [[repr(tiny)], [repr(3 * tiny)], ["2.2250738585072014e-308"], [repr(-tiny)], ["1e-310"], ["0"]],     # subnormals
        [["inf"], ["1"], ["2"], ["3"], ["4"]], [["-inf"], ["inf"], ["5"]], [["inf"], ["inf"], ["inf"]],    # inf
        [[v] for v in near * 3],                                             # neighbours that differ in the last bit
        [["nan"], ["1.5"], ["nan"], ["2.5"], ["nan"]],                       # nan in the first and last place
        [["1"], ["2"], ["4"], ["8"], ["16"]],                                # n = 5: 0.25 * 4 and 0.75 * 4 are integers
        [["1"], ["2"], ["4"], ["8"]],                                        # n = 4: weights 0.75 and 0.25, and the median's mean
        [[str(v)] for v in range(21)],                                       # n = 21: 0.05 * 20 .. 0.95 * 20
        [["3"]], [["3"], ["9"]],
    ]
    return _table(path, windows)


def test_values_where_the_arithmetic_turns(tmp_path):
    inp = _special(str(tmp_path / "t.tsv"))
    got, status, info, _ = _both(inp, ["-w", "100000", "--stats"] + ALL, tmp_path)
    assert status == 0 and got.count(b"\n") == 15, got
    # the same windows through the radix select
    _, _, info, _ = _both(inp, ["-w", "100000", "--stats"] + ALL, tmp_path, env={"PG_WS_LDS_VALS": "1"})
    assert info["device_big_cells"] >= 12, info


def test_overlapping_windows(tmp_path):
    R = random.Random(5)
    rows = ["scaffold\tposition\ta\tb"]
    for scaf in ("s1", "s2"):
        for p in sorted(R.sample(range(1, 3000), 700)):
            rows.append("%s\t%d\t%s\t%s" % (scaf, p, _number(R), _number(R) if R.random() < 0.9 else "nan"))
    inp = str(tmp_path / "t.tsv")
    with open(inp, "w") as f:
        f.write("\n".join(rows) + "\n")
    _both(inp, ["-w", "500", "-s", "100", "-m", "3", "--stats"] + ALL, tmp_path)
    _both(inp, ["--windType", "sites", "-w", "300", "-O", "290", "--stats"] + ALL, tmp_path, env={"PG_WS_LDS_VALS": "256"})


def test_3000_windows_of_one_site(tmp_path):
    R = random.Random(9)
    rows = ["scaffold\tposition\ta"] + ["s1\t%d\t%s" % (p, _number(R)) for p in range(1, 3001)]
    inp = str(tmp_path / "t.tsv")
    with open(inp, "w") as f:
        f.write("\n".join(rows) + "\n")
    got, _, info, _ = _both(inp, ["-w", "1", "--stats"] + ALL, tmp_path)
    assert got.count(b"\n") == 3001 and info["device_cells"] == 3000, info


def test_negative_zero_in_a_sum(tmp_path):
    inp = _table(str(tmp_path / "t.tsv"), [[["-0.0"]], [["-0.0"], ["0"]], [["-0.0"]] * 9, [["-0.0"], ["-1"], ["1"]]])
    _both(inp, ["-w", "100000", "--stats", "sum"], tmp_path)


@pytest.mark.parametrize("cell,through_float", [("123456789012345", 0), ("1234567890123456", 1), ("1e22", 0), ("1e23", 1),
                                                ("1.5e-22", 1), ("15e-23", 1), ("15e-22", 0)])
def test_a_cell_on_either_side_of_the_regular_spelling(cell, through_float, tmp_path):
    inp = _table(str(tmp_path / "t.tsv"), [[["1"], [cell], ["3.5"]], 4])
    _, _, info, _ = _both(inp, ["-w", "100000", "--stats"] + ALL, tmp_path)
    assert info["cells_through_float"] == through_float, info
    assert info["device_blocks"] == 1 and info["device_host_blocks"] == through_float, info     # the one block flips to the host


def test_runs_of_blanks_and_positions_across_2_31(tmp_path):
    R = random.Random(21)
    rows = ["scaffold  position \t a\tb"]
    base = (1 << 31) - 40
    for k in range(80):
        rows.append("s1 \t %d  %s\t\t%s " % (base + k, _number(R), _number(R)))
    inp = str(tmp_path / "t.tsv")
    with open(inp, "w") as f:
        f.write("\n".join(rows) + "\n")
    got, _, info, _ = _both(inp, ["--windType", "sites", "-w", "16", "--stats"] + ALL, tmp_path)
    assert b"s1,2147483608,2147483623,2147483616,16," in got
    assert info["device_blocks"] == 1 and info["device_host_blocks"] == 0, info


def test_comment_lines_scaffold_changes_and_block_seams_on_the_device(tmp_path):
    R = random.Random(31)
    rows = ["scaffold\tposition\ta\tb"]
    for k in range(400):
        if k % 37 == 5:
            rows.append("# a comment %d 1 2" % k)
        rows.append("%s\t%d\t%s\t%s" % ("s%d" % (k // 90), k % 90 * 3 + 1, _number(R), _number(R) if k % 11 else "nan"))
    inp = str(tmp_path / "t.tsv")
    with open(inp, "w") as f:
        f.write("\n".join(rows) + "\n")
    argv = ["-w", "50", "-s", "20", "--stats"] + ALL
    _, _, info, _ = _both(inp, argv, tmp_path)
    assert info["device_blocks"] == 1 and info["device_host_blocks"] == 0 and info["sites"] == 400, info
    _, _, info, _ = _both(inp, argv, tmp_path, env={"PG_STREAM_BYTES": "500"})       # runs that go on across the blocks' seams
    assert info["device_blocks"] > 10 and info["device_host_blocks"] == 0 and info["sites"] == 400, info


@pytest.mark.parametrize("line", ["s9\t5\t1", "s9\t5\t1\t2\t3", "s9\t5x\t1\t2", "s9\t5\t1\tinf", "s9\t5\t1\t2\r"])
def test_a_line_of_another_shape_hands_its_block_to_the_host(line, tmp_path):
    R = random.Random(41)
    rows = ["scaffold\tposition\ta\tb"] + ["s1\t%d\t%s\t%s" % (k + 1, _number(R), _number(R)) for k in range(120)]
    rows.insert(100, line)
    inp = str(tmp_path / "t.tsv")
    with open(inp, "wb") as f:
        f.write(("\n".join(rows) + "\n").encode())
    (want, ws, _, _), (got, gs, info, err) = run_jobs([(["-w", "30", "-i", inp], HOST), (["-w", "30", "-i", inp],
                                                                                        dict(DEV, PG_STREAM_BYTES="600"))], tmp_path)
    assert gs == ws and got == want, err
    assert info["device_host_blocks"] == 1 and info["device_blocks"] >= 3, info
