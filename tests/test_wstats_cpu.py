"""The windowStats.py drop-in without a GPU (PG_WS_DEVICE=0: pg_ws_text, pg_ws_stats_host): every golden of the unmodified reference byte
for byte; each rejection (exit status 2, nothing written) and each stop (exit status 1 behind the rows that were whole); --include /
--exclude, -o, -o x.gz and gzipped input, which the reference's Python-2 lines do not survive; pg_ws_core.h's cell rule, built with g++
alone, against float() on a seeded corpus; pg_ws_stats_host against NumPy itself to the last bit; and k_ws_stats' steps -- the walk in
chunks of 256, the pieces of 8192, the summation tree's leaves, the bitonic network, the radix select -- emulated serially by
tests/ws_core_main.cpp, against NumPy as well."""
import gzip
import os
import random
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from wstats_cases import ALL, CASES, NOTHING, NUMPY_VERSION, fixture_path, golden  # noqa: E402

HEAD = b"scaffold,start,end,mid,sites"
COUNTS = [0, 1, 2, 3, 7, 8, 9, 127, 128, 129, 255, 256, 257, 8191, 8192, 8193, 20000]
needs_recorded_numpy = pytest.mark.skipif(np.__version__ != NUMPY_VERSION, reason="the statistics are NumPy %s's to the last bit" % NUMPY_VERSION)


def run(argv, inp=None, stdin=None, env=None, timeout=120):
    e = dict(os.environ, PG_WS_DEVICE="0", PG_TIMING="1", **(env or {}))
    cmd = [sys.executable, os.path.join(ROOT, "windowStats.py")] + [a.replace("@G", GOLD) for a in argv] + (["-i", inp] if inp else [])
    return subprocess.run(cmd, input=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout, cwd=ROOT)


def info_of(r):
    line = [ln for ln in r.stderr.decode().splitlines() if ln.startswith("PG_TIMING wstats ")][0]
    return dict(kv.split("=", 1) for kv in line.split()[2:])


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_host_route_reproduces_the_reference(case):
    name, fixture, argv, through_stdin = case
    if through_stdin:
        with open(fixture_path(fixture), "rb") as f:
            r = run(argv, stdin=f.read())
    else:
        r = run(argv, inp=fixture_path(fixture))
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    assert r.stdout == golden(name)
    info = info_of(r)
    assert info["device_cells"] == "0" and (int(info["host_cells"]) == 0) == (name in NOTHING), info


def test_small_blocks_and_progress_lines(tmp_path):
    R = random.Random(3)
    rows = ["scaffold\tposition\ta"] + ["s%d\t%d\t%s" % (k // 200, k % 200 + 1, R.randint(0, 99)) for k in range(450)]
    inp = str(tmp_path / "t.tsv")
    with open(inp, "w") as f:
        f.write("\n".join(rows) + "\n")
    one = run(["-w", "1"], inp=inp)
    many = run(["-w", "1"], inp=inp, env={"PG_STREAM_BYTES": "64", "PG_HOST_THREADS": "3"})
    assert one.returncode == 0 and many.returncode == 0 and one.stdout == many.stdout and one.stdout.count(b"\n") == 451
    assert int(info_of(many)["blocks"]) > 50
    assert [ln for ln in one.stderr.decode().splitlines() if ln.endswith("windows analysed...")] == ["%d windows analysed..." % n
                                                                                                    for n in (100, 200, 300, 400)]


MAIN = fixture_path("main")


@pytest.mark.parametrize("argv,said", [
    ([], "Window size must be provided."),
    (["-w", "0"], "Window size must be provided."),
    (["-w", "10", "-O", "2"], "Overlap does not apply to coordinate windows"),
    (["-w", "10", "-D", "5"], "Maximum distance only applies to sites windows."),
    (["--windType", "sites"], "Window size (number of sites) must be provided."),
    (["--windType", "sites", "-w", "5", "-s", "2"], "Step size only applies to coordinate windows"),
    (["--windType", "predefined"], "Please provide a file of window coordinates."),
    (["--windType", "predefined", "--windCoords", "@G/wstats/coords.txt", "-O", "1"], "Overlap does not apply for predefined windows."),
    (["--windType", "predefined", "--windCoords", "@G/wstats/coords.txt", "-D", "1"], "Maximum does not apply for predefined windows."),
    (["--windType", "predefined", "--windCoords", "@G/wstats/coords.txt", "-s", "1"], "Step size does not apply for predefined windows."),
    (["--windType", "predefined", "--windCoords", "@G/wstats/coords.txt", "--include", "@G/wstats/coords.txt"], "You cannot only include"),
    (["--windType", "predefined", "--windCoords", "@G/wstats/coords.txt", "--exclude", "@G/wstats/coords.txt"], "You cannot exclude"),
    (["--windType", "predefined", "--windCoords", "@G/wstats/coords.txt", "-m", "0"], "predefined -m 0"),
    (["-w", "100", "--columns", "a", "nobody"], "nobody is not in the header"),
])
def test_command_lines_that_are_rejected(argv, said):
    r = run(argv, inp=MAIN)
    assert r.returncode == 2 and r.stdout == b"" and said in r.stderr.decode(), r.stderr.decode()
    assert len(r.stderr.decode().strip().splitlines()) == 1


def _file(tmp_path, text, name="t.tsv"):
    p = str(tmp_path / name)
    with open(p, "wb") as f:
        f.write(text if isinstance(text, bytes) else text.encode())
    return p


@pytest.mark.parametrize("text,argv,said", [
    ("scaffold position\nc1 1\n", ["-w", "10"], "names no value column"),
    (b"scaffold position a\nc1 1 2\nc1 2 \xc3\xa9\n", ["-w", "10"], "line 3: text that is not ASCII"),
    (b"scaffold position \xc3\xa9\nc1 1 2\n", ["-w", "10"], "not ASCII"),
    ("scaffold position a\nc1 1 2\nc1 1234567890123456789 3\n", ["-w", "10"], "line 3: a position of more than 18 digits"),
    ("scaffold position a\n" + "".join("c1 %d 1\n" % k for k in range(1, 200)), ["-w", "10"], "PG_SCRATCH_GIB"),
])
def test_inputs_that_are_rejected(text, argv, said, tmp_path):
    r = run(argv, inp=_file(tmp_path, text), env={"PG_SCRATCH_GIB": "0.000001"} if said == "PG_SCRATCH_GIB" else None)
    assert r.returncode == 2 and r.stdout == b"" and said in r.stderr.decode(), r.stderr.decode()


def test_a_bad_cell_stops_at_the_first_window_that_converts_it():
    r = run(["-w", "100"], inp=fixture_path("bad"))
    want = golden("bad_in_failed_window").split(b"\n")
    assert r.returncode == 1 and r.stdout.split(b"\n")[0] == want[0]
    assert r.stdout.count(b"\n") == 2 and r.stdout.split(b"\n")[1].startswith(b"c1,1,100,26,4,")
    err = r.stderr.decode()
    assert "window 2 (c1 101-200), column a: the cell 'x' is not a number" in err
    # b's bad cell stands in the same window; -m 4 fails that window and the reference runs through (the golden)
    r = run(["-w", "100", "--columns", "b"], inp=fixture_path("bad"))
    assert r.returncode == 1 and "column b: the cell 'oops'" in r.stderr.decode() and r.stdout.count(b"\n") == 2


def test_min_of_a_column_without_a_value_stops_there():
    r = run(["-w", "100", "--stats", "mean", "min"], inp=fixture_path("allnan"))
    assert r.returncode == 1 and r.stdout == HEAD + b",a_mean,a_min,b_mean,b_min\n"
    assert "window 1 (c1 1-100), column b: min / max of a column without a value" in r.stderr.decode()
    r = run(["-w", "100", "--stats", "mean", "max", "--columns", "a"], inp=fixture_path("allnan"))
    assert r.returncode == 0 and r.stdout.count(b"\n") == 3


LINES = "scaffold position a b\n" + "".join("c1 %d %d %d.5\n" % (p, p, p) for p in (5, 15, 25, 105, 115, 205, 215, 305))


@pytest.mark.parametrize("bad_line,said,rows", [
    ("c1 2x6 1 2\n", "line 8: the position '2x6' is not an integer", 2),
    ("c1 206 1\n", "line 8: fewer fields than the selected columns need", 2),
    ("\n", "line 8: fewer fields", 2),
    ("c1 206 1 2 3\n", "line 8: more value fields than the header names", 2),
])
def test_a_line_the_reference_dies_on_stops_behind_the_whole_rows(bad_line, said, rows, tmp_path):
    lines = LINES.splitlines(True)
    text = "".join(lines[:7] + [bad_line] + lines[7:])
    r = run(["-w", "100"], inp=_file(tmp_path, text))
    whole = run(["-w", "100"], inp=_file(tmp_path, LINES, "whole.tsv"))
    assert r.returncode == 1 and said in r.stderr.decode(), r.stderr.decode()
    # windows 1-100 and 101-200 had been yielded when the line was read (the site at 205, in front of the line, closed the second)
    assert r.stdout == b"".join(whole.stdout.splitlines(True)[:1 + rows])


def test_position_spellings_int_takes(tmp_path):
    plain = "scaffold position a\nc1 7 1\nc1 10 2\nc1 12 4\n"
    spelled = "scaffold position a\nc1 007 1\nc1 1_0 2\nc1 +12 4\n"
    a, b = run(["-w", "100"], inp=_file(tmp_path, plain, "a.tsv")), run(["-w", "100"], inp=_file(tmp_path, spelled, "b.tsv"))
    assert a.returncode == 0 and b.returncode == 0 and a.stdout == b.stdout and b",10,3," in a.stdout


def test_include_and_exclude(tmp_path):
    with open(MAIN) as f:
        lines = f.read().splitlines(True)
    c1 = _file(tmp_path, "".join(ln for k, ln in enumerate(lines) if k == 0 or ln.startswith("c1\t")), "c1.tsv")
    c2 = _file(tmp_path, "".join(ln for k, ln in enumerate(lines) if k == 0 or ln.startswith("c2\t")), "c2.tsv")
    only = _file(tmp_path, "c1\n", "only.txt")
    for argv in (["-w", "100"], ["--windType", "sites", "-w", "10", "-O", "3"]):
        want1, want2 = run(argv, inp=c1), run(argv, inp=c2)
        inc = run(argv + ["--include", only], inp=MAIN)
        exc = run(argv + ["--exclude", only], inp=MAIN)
        assert inc.returncode == 0 and inc.stdout == want1.stdout and "1 scaffolds will be analysed.\n" in inc.stderr.decode()
        assert exc.returncode == 0 and exc.stdout == want2.stdout and "1 scaffolds will be excluded.\n" in exc.stderr.decode()


def test_output_file_gzipped_output_and_gzipped_input(tmp_path):
    argv = ["-w", "100", "--stats"] + ALL
    want = golden("stats_all")
    out = str(tmp_path / "o.csv")
    r = run(argv + ["-o", out], inp=MAIN)
    assert r.returncode == 0 and r.stdout == b"" and open(out, "rb").read() == want
    r = run(argv + ["-o", out + ".gz"], inp=MAIN)
    assert r.returncode == 0 and gzip.open(out + ".gz", "rb").read() == want
    from genomics_general_amd import genoio
    with open(MAIN, "rb") as f:
        text = f.read()
    for name, data in (("plain.tsv.gz", gzip.compress(text)), ("members.tsv.gz", bytes(genoio.bgzf_compress(text, block=500)))):
        r = run(argv, inp=_file(tmp_path, data, name), env={"PG_STREAM_BYTES": "700"})
        assert r.returncode == 0 and r.stdout == want, name
    crlf = run(argv, inp=_file(tmp_path, text.replace(b"\n", b"\r\n"), "crlf.tsv"))
    assert crlf.returncode == 0 and crlf.stdout == want


# ---- pg_ws_core.h as a program of its own ------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def core_main(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("ws_core") / "ws_core_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "ws_core_main.cpp"),
                           "-o", exe])
    return exe


def _corpus():
    R = random.Random(77)
    cells = ["nan", "NaN", "NAN", "nAn", "0", "-0", "+0", "0.0", "-0.0", "00", "007", "1.", ".5", "-.5", "+.5e-3", "1e3", "1E3", "1e+3", "1e-3",
             "0e400", "0.000e-999", "1e22", "1e-22", "1e23", "1e-23", "123456789012345e22", "123456789012345e23", "1.5e23", "15e22", "1.5e-22",
             "0.15e24", "0.15e25", "0.001e25", "0.001e26", "1000e22", "1000e23", "999999999999999", "1000000000000000", "0999999999999999",
             "9007199254740992", "9007199254740993", "900719925474099", "9.00719925474099e15", "0.000000000000000000001", "1" + "0" * 14,
             "1" + "0" * 15, "0." + "0" * 30 + "123456789012345", "0." + "0" * 7 + "123456789012345", "0." + "0" * 8 + "123456789012345"]
    irregular = ["", "+", "-", ".", "e5", "1e", "1e+", "-nan", "+nan", "inf", "-inf", "infinity", "Infinity", "1_0", "0x10", "1d5", "nan(1)", "1 ",
                 " 1", "1e400", "1e-400", "--1", "1..2", "1.2.3", "1e5e5", "١", "nana", "na"]
    for _ in range(3000):
        digits = R.randint(1, 17)
        m = "".join(R.choice("0123456789") for _ in range(digits))
        point = R.randint(0, digits) if R.random() < 0.7 else None
        s = m if point is None else m[:point] + "." + m[point:]
        if R.random() < 0.6:
            s += R.choice("eE") + R.choice(["", "+", "-"]) + str(R.choice([0, 1, 5, 9, 21, 22, 23, 24, R.randint(0, 40)]))
        cells.append(R.choice(["", "", "+", "-"]) + s)
    for base in (10 ** 15, 2 ** 53):
        for d in range(-3, 4):
            cells += [str(base + d), "%de-7" % (base + d), "%d.0e7" % (base + d)]
    return cells, irregular


def test_the_cell_rule_against_float(core_main, tmp_path):
    cells, irregular = _corpus()
    src, dst = str(tmp_path / "cells.txt"), str(tmp_path / "out.txt")
    with open(src, "w", encoding="utf-8") as f:
        f.write("".join(c + "\n" for c in cells + irregular))
    r = subprocess.run([core_main, "cells", src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout.decode().strip() == "%d cells" % (len(cells) + len(irregular)), r.stderr.decode()[-2000:]
    with open(dst) as f:
        got = f.read().split()
    regular = 0
    for c, g in zip(cells + irregular, got):
        if g == "I":
            continue
        regular += 1
        assert c not in irregular, c
        want = float(c)
        assert int(g, 16) == struct.unpack("=Q", struct.pack("=d", want))[0] or (want != want and int(g, 16) == 0x7FF8000000000000), (c, g, want)
    by = dict(zip(cells + irregular, got))
    assert all(by[c] == "I" for c in irregular)
    # the edges of the rule: 15 against 16 significant digits, an effective exponent of 22 against 23 -- the latter irregular
    for c, reg in (("999999999999999", 1), ("1000000000000000", 0), ("0999999999999999", 1), ("1e22", 1), ("1e23", 0), ("1e-22", 1), ("1e-23", 0),
                   ("123456789012345e22", 1), ("123456789012345e23", 0), ("1.5e23", 1), ("15e22", 1), ("1.5e-22", 0), ("0.15e24", 1),
                   ("0.15e25", 0), ("0.001e25", 1), ("0.001e26", 0), ("1000e22", 1), ("1000e23", 0), ("0e400", 1), ("1.", 1), (".5", 1),
                   ("0." + "0" * 7 + "123456789012345", 1), ("0." + "0" * 8 + "123456789012345", 0)):
        assert (by[c] != "I") == bool(reg), c
    assert regular > 1500


def _arrays(rng):
    """per count: spread magnitudes with nan sprinkled in (first and last place among them), ties, and small integers"""
    arrays = []
    for n in COUNTS:
        for kind in range(3):
            if kind == 0:
                a = rng.choice([-1.0, 1.0], size=n) * 10.0 ** rng.uniform(-8.0, 8.0, size=n)
            elif kind == 1:
                a = rng.integers(-3, 4, size=n).astype(np.float64) / 8.0 + 0.1
            else:
                a = rng.standard_normal(n) * 50.0
            out = []
            for value, hole in zip(a, rng.random(n) < 0.1):
                if hole:
                    out.append(np.nan)
                out.append(value)
            arrays.append(np.asarray([np.nan] + out + [np.nan], dtype=np.float64))
    return arrays


def _numpy_stats(x):
    """windowStats.py:163-180 on one column, before round(sd, 6): the 12 statistics' bit patterns (nan: any)"""
    v = x[~np.isnan(x)]
    out = []
    with np.errstate(all="ignore"):
        import warnings
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for s in ALL:
                if s == "mean":
                    r = v.mean()
                elif s == "median":
                    r = np.median(v)
                elif s in ("min", "max"):
                    r = (np.min(v) if s == "min" else np.max(v)) if len(v) else np.nan
                elif s == "sd":
                    r = np.std(v)
                elif s == "sum":
                    r = np.sum(v)
                else:
                    try:
                        r = np.quantile(v, {"q5": 0.05, "q10": 0.1, "q25": 0.25, "q75": 0.75, "q90": 0.9, "q95": 0.95}[s])
                    except IndexError:
                        r = np.nan
                out.append(np.float64(r))
    return out, len(v)


def _same(got_bits, want):
    if np.isnan(want):
        return bool(np.isnan(np.uint64(got_bits).view(np.float64)))
    return int(got_bits) == int(np.float64(want).view(np.uint64))


@needs_recorded_numpy
def test_host_statistics_against_numpy_bit_for_bit():
    from genomics_general_amd import wstats
    rng = np.random.default_rng(4242)
    arrays = _arrays(rng)
    pitch = max(len(a) for a in arrays)
    for a in arrays:
        vals = np.full((2, pitch), np.nan)
        vals[1, :len(a)] = a                                 # (the second column; the first holds no value)
        out, cnt, flag = wstats.host_stats(vals, np.array([0, 0]), np.array([len(a), 0]), (1 << 12) - 1, n_threads=2)
        want, n = _numpy_stats(a)
        assert cnt[0, 1] == n and cnt[0, 0] == 0 and flag[0, 1] == (n == 0) and flag[0, 0] == 1
        for s, (g, w) in enumerate(zip(out[0, 1].view(np.uint64), want)):
            assert _same(g, w), (len(a), n, ALL[s], float(np.uint64(g).view(np.float64)), float(w))
        assert out[1, 1, 5] == 0.0 and np.isnan(out[1, 1, 0])
        # few statistics: the ranks are selected one after another (std::nth_element) instead of sorted
        for stats in (("q10", "q25"), ("median",), ("q95", "q5")):
            mask = sum(1 << ALL.index(s) for s in stats)
            out, _, _ = wstats.host_stats(vals, np.array([0]), np.array([len(a)]), mask, n_threads=1)
            for s in stats:
                assert _same(out[0, 1].view(np.uint64)[ALL.index(s)], want[ALL.index(s)]), (len(a), n, stats, s)


@needs_recorded_numpy
@pytest.mark.parametrize("lds", [256, 8192])
def test_the_kernels_steps_emulated_against_numpy(core_main, lds, tmp_path):
    rng = np.random.default_rng(99 + lds)
    arrays = _arrays(rng)
    src, dst = str(tmp_path / "arrays.bin"), str(tmp_path / "stats.txt")
    with open(src, "wb") as f:
        f.write(struct.pack("=q", len(arrays)))
        for a in arrays:
            f.write(struct.pack("=q", len(a)) + a.tobytes())
    r = subprocess.run([core_main, "emul", str(lds), src, dst], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0 and r.stdout.decode().strip() == "%d arrays" % len(arrays), r.stderr.decode()[-3000:]
    with open(dst) as f:
        rows = [line.split() for line in f]
    assert len(rows) == 2 * len(arrays)
    for k, a in enumerate(arrays):
        want, n = _numpy_stats(a)
        for tier in (0, 1):
            got = rows[2 * k + tier]
            assert int(got[-1]) == n
            for s, w in enumerate(want):
                if n == 0 and ALL[s] in ("min", "max"):
                    continue
                assert _same(int(got[s], 16), w), (len(a), n, ("lds", "big")[tier], ALL[s])
