"""The filterGenotypes.py drop-in against oracle/filter_oracle.py, an independent plain-Python restatement of the reference (pinned to
the reference's goldens by tests/test_filter_oracle_golden.py), on the CPU: the host route (PG_FILTER_DEVICE=0) and the device's
per-line functions walked by tests/filter_emul.cpp, on tests/golden/filter_cases.edge_case files (ties, polyploid cells, odd
characters, prefix contig names, shared and empty populations, thresholds equal to attainable ratios) and on random_case files; every
tie pattern of 2, 3 and 4 present alleles through the outputs that depend on the allele order; named cases of the rules the oracle
settled."""
import os
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
sys.path.insert(0, ROOT)
from filter_cases import edge_case, edge_files, random_case  # noqa: E402

from genomics_general_amd import filtergeno  # noqa: E402
from oracle.filter_oracle import filter_reference  # noqa: E402
from test_filter_emul import _emul_device, _Stats, emul  # noqa: E402,F401  (the emulator's fixture)


def _write(tmp_path, text, argv, files=None):
    inp = str(tmp_path / "in.geno")
    with open(inp, "w") as f:
        f.write(text)
    d = str(tmp_path)
    return inp, edge_files(argv, files or {}, d), files


def _oracle(text, argv, files):
    return filter_reference(argv, text)          # (the extra files are read where edge_files wrote them)


def _host(inp, argv, out, monkeypatch, capsys, block=None):
    monkeypatch.setenv("PG_FILTER_DEVICE", "0")
    if block:
        monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    capsys.readouterr()
    rc = filtergeno.filter_main(["-i", inp, "-o", out] + argv)
    return rc, open(out, "rb").read(), capsys.readouterr().err


def _emulated(emul, inp, argv, out, monkeypatch, capsys, block):
    monkeypatch.setattr(filtergeno, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_FILTER_DEVICE", "1")
    monkeypatch.setenv("PG_BGZF_DEVICE", "0")
    monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    _Stats.blocks = _Stats.handed_back = 0
    capsys.readouterr()
    rc = filtergeno.filter_main(["-i", inp, "-o", out, "--device", "0"] + argv)
    return rc, open(out, "rb").read(), capsys.readouterr().err


def check(res, rc, got, err):
    """a drop-in run (exit code, output bytes, stderr) against the oracle's Result"""
    if res.setup_error:
        assert rc != 0, res.setup_error
    elif res.error:
        assert rc != 0 and ("line %d:" % res.error[0]) in err, (res.error, err[-500:])
    else:
        assert rc == 0, err[-2000:]
        if not res.matches(got):
            want = res.data() if not res.random else b""
            g, w = got.split(b"\n"), want.split(b"\n")
            first = next((k for k in range(min(len(g), len(w))) if g[k] != w[k]), None)
            raise AssertionError("differs from the oracle at output line %s: got %r want %r (%d / %d lines)" % (
                first, g[first] if first is not None else None, w[first] if first is not None else None, len(g), len(w)))


EDGE_SEEDS = range(200)
RANDOM_SEEDS = range(60)


@pytest.mark.parametrize("seed", EDGE_SEEDS)
def test_host_route_equals_the_oracle_on_edge_files(seed, tmp_path, monkeypatch, capsys):
    text, argv, files = edge_case(seed + 11000)
    inp, argv, files = _write(tmp_path, text, argv, files)
    res = _oracle(text, argv, files)
    check(res, *_host(inp, argv, str(tmp_path / "h.geno"), monkeypatch, capsys, block=1500 + 211 * (seed % 7)))


@pytest.mark.parametrize("seed", EDGE_SEEDS)
def test_device_functions_equal_the_oracle_on_edge_files(seed, emul, tmp_path, monkeypatch, capsys):  # noqa: F811
    text, argv, files = edge_case(seed + 11000)
    inp, argv, files = _write(tmp_path, text, argv, files)
    res = _oracle(text, argv, files)
    check(res, *_emulated(emul, inp, argv, str(tmp_path / "d.geno"), monkeypatch, capsys, 1200 + 97 * (seed % 11)))
    assert _Stats.handed_back == 0


@pytest.mark.parametrize("seed", RANDOM_SEEDS)
def test_both_routes_equal_the_oracle_on_random_files(seed, emul, tmp_path, monkeypatch, capsys):  # noqa: F811
    text, argv = random_case(seed)
    inp, argv, files = _write(tmp_path, text, argv)
    res = _oracle(text, argv, files)
    check(res, *_host(inp, argv, str(tmp_path / "h.geno"), monkeypatch, capsys))
    check(res, *_emulated(emul, inp, argv, str(tmp_path / "d.geno"), monkeypatch, capsys, 2000))


def _tie_file():
    """one line per count pattern (values 1..m over m present alleles, every ordering, tied or not) on every m-subset of ACGT: the
    alleles dealt in order into 8 diploid cells (so hets show the within-genotype order), N filling the rest"""
    import itertools
    names = ["d%d" % k for k in range(8)]
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    pos = 0
    for m in (2, 3, 4):
        for bases in itertools.combinations("ACGT", m):
            for pat in itertools.product(range(1, m + 1), repeat=m):
                if m == 4 and len(set(pat)) == m:
                    continue                      # (no ties: 4! orderings of 1..4 need 10 alleles; covered by the m = 4 ties and m < 4)
                slots = [b for b, c in zip(bases, pat) for _ in range(c)]
                slots += ["N"] * (16 - len(slots))
                cells = [slots[2 * k] + "/|"[k % 2] + slots[2 * k + 1] for k in range(8)]
                pos += 1
                rows.append("\t".join(["t%d" % m, str(pos)] + cells))
    return "\n".join(rows) + "\n"


@pytest.mark.parametrize("argv", [["-of", "coded"], ["-of", "count"], ["-of", "alleles", "--alleleOrder", "freq"],
                                  ["-of", "bases", "--alleleOrder", "freq", "--ploidy", "2"]], ids=["coded", "count", "alleles", "bases"])
def test_every_tie_pattern_orders_the_alleles_as_numpy(argv, emul, tmp_path, monkeypatch, capsys):  # noqa: F811
    text = _tie_file()
    inp, argv, files = _write(tmp_path, text, argv)
    res = _oracle(text, argv, files)
    assert res.error is None and len(res.rows) == text.count("\n") - 1
    check(res, *_host(inp, argv, str(tmp_path / "h.geno"), monkeypatch, capsys))
    check(res, *_emulated(emul, inp, argv, str(tmp_path / "d.geno"), monkeypatch, capsys, 1 << 20))


def test_thresholds_equal_to_a_ratio_pass(emul, tmp_path, monkeypatch, capsys):  # noqa: F811
    """--minFreq / --maxFreq at k/n, --maxHet at h/c and --nearlyFixedDiff at an attainable difference: the reference's <= / >= pass"""
    text = ("#CHROM\tPOS\ta\tb\tc\td\n"
            "c\t1\tA/T\tA/A\tA/A\tA/A\n"        # minor 1/8, 1 het of 4
            "c\t2\tA/T\tT/T\tA/A\tA/A\n"        # minor 3/8
            "c\t3\tA/A\tA/A\tT/T\tA/T\n")       # P0 = a,b all A; P1 = c,d T 3/4: difference 3/4 (line 2: 3/4 too)
    for argv in (["--minFreq", repr(1 / 8)], ["--maxFreq", repr(3 / 8)], ["--maxHet", "0.25"],
                 ["-p", "P0", "a,b", "-p", "P1", "c,d", "--nearlyFixedDiff", "0.75"]):
        inp, av, files = _write(tmp_path, text, argv)
        res = _oracle(text, av, files)
        check(res, *_host(inp, av, str(tmp_path / "h.geno"), monkeypatch, capsys))
        check(res, *_emulated(emul, inp, av, str(tmp_path / "d.geno"), monkeypatch, capsys, 1 << 20))
    assert [r[1] for r in filter_reference(["--minFreq", repr(1 / 8)], text).rows] == ["1", "2", "3"]
    assert [r[1] for r in filter_reference(["--maxHet", "0.25"], text).rows] == ["1", "2", "3"]
    assert [r[1] for r in filter_reference(["-p", "P0", "a,b", "-p", "P1", "c,d", "--nearlyFixedDiff", "0.75"], text).rows] == ["2", "3"]


@pytest.mark.parametrize("route", ["host", "emul"])
def test_a_cell_of_17_alleles_stops_the_run_at_its_line(route, emul, tmp_path, monkeypatch, capsys):  # noqa: F811
    """16 alleles (31 bytes phased) are taken; 17 are past the drop-in's limit: the run stops and names the line"""
    text, argv, files = edge_case(4242, n_samples=6, n_lines=400, ploidy="none", over_limit=300, fmt="phased")
    inp, argv, files = _write(tmp_path, text, argv, files)
    out = str(tmp_path / "o.geno")
    rc, _, err = (_host(inp, argv, out, monkeypatch, capsys, block=2000) if route == "host"
                  else _emulated(emul, inp, argv, out, monkeypatch, capsys, 2000))
    assert rc != 0 and "line 300:" in err, err[-500:]


@pytest.mark.parametrize("route", ["host", "emul"])
def test_leading_zeros_do_not_count_towards_the_18_digits_of_a_position(route, emul, tmp_path, monkeypatch, capsys):  # noqa: F811
    """int() takes '0' + 18 digits; the drop-in used to stop the run at such a line under --thinDist (a position of 19 characters)"""
    text = ("#CHROM\tPOS\ta\tb\n"
            "c\t0123456789012345678\tA/T\tA/A\n"
            "c\t000123456789012345680\tA/T\tT/T\n"
            "c\t123456789012345681\tA/T\tT/T\n"
            "c\t0000000000000000000000123456789012345690\tA/A\tT/T\n")
    argv = ["--thinDist", "2"]
    inp, argv, files = _write(tmp_path, text, argv)
    res = _oracle(text, argv, files)
    assert [r[1] for r in res.rows] == ["000123456789012345680", "0000000000000000000000123456789012345690"]
    out = str(tmp_path / "o.geno")
    check(res, *(_host(inp, argv, out, monkeypatch, capsys) if route == "host" else
                 _emulated(emul, inp, argv, out, monkeypatch, capsys, 1 << 20)))


HWE_NN = ("#CHROM\tPOS\ta\tb\tc\td\n"
          "c\t1\tN/N\tN|N\tA/T\tT/T\n"            # a, b (the populations) N/N; c, d vary: inHWE drops the N diplotypes -> True
          "c\t2\tN/N\tN/N\tA/A\tA/A\n"
          "c\t3\tN/N\tN/N\tC/T\tC/C\n"
          "c\t4\tA/A\tN/N\tA/T\tT/T\n")           # a called genotype in P0: the reference reaches its undefined `unique`


@pytest.mark.parametrize("route", ["host", "emul"])
@pytest.mark.parametrize("argv,rows,line", [
    (["--HWE", "0.05", "both", "-p", "P0", "a", "-p", "P1", "b", "--keepAllSamples"], ["1", "2", "3"], 5),
    (["--HWE", "0.05", "both", "-p", "P0", "a,b", "-s", "d,c,b,a"], ["1", "2", "3"], 5),
    (["--HWE", "0.05", "both", "-p", "P0", "a", "-p", "E", "--keepAllSamples"], [], 2),         # E is empty: all samples
], ids=["two_pops", "samples", "empty_pop"])
def test_hwe_with_populations_of_n_genotypes_passes_as_in_the_reference(argv, rows, line, route, emul, tmp_path, monkeypatch,  # noqa: F811
                                                                         capsys):
    """--HWE with populations: the reference's inHWE drops "N" diplotypes and returns True when none are left, so a variable site whose
    populations are all N/N passes; a population with a called genotype (an empty one stands for all samples) raises"""
    inp, av, files = _write(tmp_path, HWE_NN, argv)
    res = _oracle(HWE_NN, av, files)
    assert [r[1] for r in res.rows] == rows and res.error[0] == line
    out = str(tmp_path / "o.geno")
    rc, got, err = (_host(inp, av, out, monkeypatch, capsys) if route == "host" else
                    _emulated(emul, inp, av, out, monkeypatch, capsys, 1 << 20))
    check(res, rc, got, err)
    assert got == res.data()                     # the rows before the line that raises
