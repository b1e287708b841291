"""-m gpu: distPaint.py on the device.  The goldens of the unmodified reference through cli.distpaint_main, byte for byte (also from
bgzip-compressed input and in blocks of 3 kB); engine.WindowBatch.paint (the pack and pair kernels, k_hap_called for the individuals'
own called counts, k_paint, the host's table of critical rank sums and its finish of the delta cells with a nan mean) against the
NumPy model of tests/paint_model.py with ==, on rows chosen for where the kernel can go wrong:

  case A  70 haploid individuals (more than a wavefront) under names that are not in sorted order; reference populations of 1, 2, 7,
          8, 9 and 33 individuals (around the 8-way unrolled loop of NumPy's sum); windows of 0, 3, 8, 12, 16, 40, 257 and 600 sites
          (one empty, one below minSites; short ones make tied quotients common); 30 % missing calls and minSites 6, so that nan
          pairs (in the windows of 12 and 16 sites: some pairs of a list, not all), an all-nan population and a nan in the best
          population occur;
  case B  200 individuals, populations of 130 (past the 128-value run of NumPy's pairwise sum) and 64;
  case C  260 individuals, reference lists of 1024, 1000 and 24: 2048 reference individuals, PAINT_MAX_REFS, which take the whole 64 KiB
          of LDS a launch may ask for, and lists past the second halving of the sum;
  case D  130 individuals, 64 populations of 1, 2 and 3: PAINT_MAX_POPS, every lane of the wavefront with a population;
  case S  600 individuals under 27 short windows: three batches under the smallest scratch limit, cells left to the host from every one;
  case F  rows with four alleles at nearly every site: the first pass of a fresh engine starts over.
What the library refuses (65 populations, 2049 reference individuals, a population without individuals, the delta mode with one
population) is refused on the host before any launch, and the engine goes on answering.

The cases are built in tests/finisher_cases.py (tests/test_finisher_cases.py shows without a GPU what they contain); the model's inputs
D and C are counted there with NumPy from the rows, once per case."""
import gzip
import os

import numpy as np
import pytest

import finisher_cases as FC
from paint_cases import PAINT_CASES
from genomics_general_amd import cli
from genomics_general_amd.engine import Engine

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
IDS = [c["name"] for c in PAINT_CASES]


def golden_text(case):
    with open(os.path.join(GOLD, "paint", case["name"] + ".out")) as f:
        return f.read()


def run_driver(case, tmp_path, geno=None):
    geno = geno or os.path.join(GOLD, case["fixture"] + ".geno.gz")
    out = str(tmp_path / (case["name"] + (".out.gz" if case.get("gz") else ".out")))
    assert cli.distpaint_main([a.format(geno=geno, dir=GOLD) for a in case["argv"]] + ["-o", out]) in (0, None)
    with (gzip.open(out, "rt") if case.get("gz") else open(out)) as f:
        return f.read()


@pytest.mark.parametrize("case", PAINT_CASES, ids=IDS)
def test_driver_reproduces_the_reference(case, tmp_path):
    assert run_driver(case, tmp_path) == golden_text(case)


TWO = [c for c in PAINT_CASES if c["name"] in ("mosaic_nan_delta", "unsorted_test")]


@pytest.mark.parametrize("case", TWO, ids=lambda c: c["name"])
def test_driver_in_small_blocks(case, tmp_path, monkeypatch):
    monkeypatch.setenv("PG_STREAM_BYTES", "3000")
    assert run_driver(case, tmp_path) == golden_text(case)


@pytest.mark.parametrize("case", TWO, ids=lambda c: c["name"])
def test_driver_on_bgzf_input(case, tmp_path, monkeypatch):
    from genomics_general_amd import genoio
    with gzip.open(os.path.join(GOLD, case["fixture"] + ".geno.gz"), "rb") as f:
        text = f.read()
    geno = str(tmp_path / (case["fixture"] + ".geno.gz"))
    with open(geno, "wb") as f:
        f.write(genoio.bgzf_compress(text, block=5000).tobytes())       # members of 5000 bytes of text: they end anywhere in a line
    monkeypatch.setenv("PG_STREAM_BYTES", "20000")
    assert run_driver(case, tmp_path, geno=geno) == golden_text(case)


# ---- WindowBatch.paint against the model ---------------------------------------------------------------------------------------
# (the cases and the model's answers: tests/finisher_cases.py, shared with tests/test_finisher_cases.py)
CASES = FC.PAINT_SHAPES
case_data = FC.paint_case
model = FC.paint_expect


def device(name, p_threshold, delta_threshold, noresult, scratch_limit=None, calls=1):
    """(decisions, cells the host finished, entries of the device's list of such cells, pack launches of every call)"""
    from genomics_general_amd import _lib
    lay, gt, lo, hi, ref_lists, _, _ = case_data(name)
    e = Engine(0)
    try:
        e.set_layout(lay)
        e.load_sites(gt)
        if scratch_limit:
            e.set_scratch_limit(scratch_limit)
        e.kernel_time_select(None)
        launches = []
        for _ in range(calls):
            e.kernel_time_reset()
            wb = e.batch(lo, hi)
            out = wb.paint(ref_lists, CASES[name]["min_sites"], p_threshold=p_threshold, delta_threshold=delta_threshold, noresult=noresult)
            launches.append(e.kernel_time(_lib.K_PACK)[1])
        return out, wb.paint_host_cells, wb.paint_host_count, launches
    finally:
        e.close()


def test_case_a_contains_what_it_is_built_for():
    _, _, info = model("A", 0.05, None, 7)
    assert info["tied_values"] > 0 and info["nan_pairs"] > 0 and info["all_nan_means"] > 0 and info["nan_in_best"] > 0, info
    assert info["partly_nan_lists"] > 0 and info["nan_in_best"] > info["nan_mean_cells"], info       # (a nan in the best list whose mean is a number)
    out, nan_mean, info = model("A", 0.05, 0.05, 7)
    assert 0 < nan_mean.sum() < nan_mean.size and info["nan_mean_cells"] == nan_mean.sum(), info
    assert len(set(out.ravel().tolist())) >= 4                # several populations and noresult are decided
    _, _, infob = model("B", 0.05, None, 7)
    assert infob["tied_values"] > 0, infob


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
@pytest.mark.parametrize("p_threshold", [0.05, 0.5])
def test_paint_test_mode_equals_the_model(name, p_threshold):
    want, _, _ = model(name, p_threshold, None, 7)
    got, host_cells, _, _ = device(name, p_threshold, None, 7)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert (got == want).all(), np.argwhere(got != want)[:10]
    assert not host_cells.any()
    assert (want == 7).any() and (want != 7).any()


@pytest.mark.parametrize("name", ["A", "B", "C", "D"])
@pytest.mark.parametrize("delta", [0.0, 0.05])
def test_paint_delta_mode_equals_the_model(name, delta):
    want, nan_mean, _ = model(name, 0.05, delta, 7)
    got, host_cells, host_count, _ = device(name, 0.05, delta, 7)
    assert (got == want).all(), np.argwhere(got != want)[:10]
    # the host finishes exactly the cells with a nan among their means, each listed once
    assert (host_cells == nan_mean).all() and host_count == nan_mean.sum()
    if name != "B":
        assert nan_mean.any()


def test_paint_with_the_popcount_pair_kernels(monkeypatch):
    monkeypatch.setenv("PG_PAIR_VALU", "1")
    for delta in (None, 0.05):
        want, nan_mean, _ = model("A", 0.05, delta, 7)
        got, host_cells, _, _ = device("A", 0.05, delta, 7)
        assert (got == want).all() and (host_cells == (nan_mean if delta is not None else False)).all()


# ---- the limits the library states, and what it refuses --------------------------------------------------------------------------
def paint_limits():
    """PAINT_MAX_POPS and PAINT_MAX_REFS, read where the library defines them"""
    import re
    with open(os.path.join(os.path.dirname(GOLD), os.pardir, "genomics_general_amd", "csrc", "pg_paint.hip")) as f:
        text = f.read()
    return tuple(int(re.search(r"#define %s (\d+)" % name, text).group(1)) for name in ("PAINT_MAX_POPS", "PAINT_MAX_REFS"))


def test_the_cases_at_the_limits_are_at_the_limits():
    max_pops, max_refs = paint_limits()
    assert sum(CASES["C"]["sizes"]) == max_refs and len(CASES["D"]["sizes"]) == max_pops


def test_paint_refuses_what_is_beyond_its_limits_and_goes_on():
    from genomics_general_amd._lib import PopgenError
    max_pops, max_refs = paint_limits()
    lay, gt, lo, hi, ref_lists, _, _ = case_data("A")
    n = lay.n_hap
    e = Engine(0)
    try:
        e.set_layout(lay)
        e.load_sites(gt)
        wb = e.batch(lo, hi)
        refused = [
            ([[k % n] for k in range(max_pops + 1)], None, "%d reference populations (1 .. %d)" % (max_pops + 1, max_pops)),
            ([[k % n for k in range(max_refs - 7)], list(range(8))], None, "%d reference individuals (at most %d)" % (max_refs + 1, max_refs)),
            ([[1, 2], [], [3]], None, "reference population 1 has no individuals"),
            ([[1, 2], [], [3]], 0.05, "reference population 1 has no individuals"),
            ([[1, 2, 3]], 0.05, "the delta mode needs two populations"),
        ]
        for lists, delta, message in refused:
            with pytest.raises(PopgenError) as err:
                wb.paint(lists, 6, delta_threshold=delta, noresult=7)
            assert message in str(err.value), (message, str(err.value))
            for d in (None, 0.05):                        # the engine still answers, in both modes
                want, nan_mean, _ = model("A", 0.05, d, 7)
                got = wb.paint(ref_lists, CASES["A"]["min_sites"], p_threshold=0.05, delta_threshold=d, noresult=7)
                assert (got == want).all() and wb.paint_host_count == (nan_mean.sum() if d is not None else 0)
    finally:
        e.close()


@pytest.mark.parametrize("delta", [None, 0.05])
def test_paint_in_sub_batches_under_a_scratch_limit(delta):
    """case S under 64 MiB of scratch, the smallest limit: the matrices of 27 windows of 600 individuals take 78 MB, so the pass is cut
    into three batches and k_paint's cell0 and its list of cells for the host (cleared at the first batch only) run past zero"""
    want, nan_mean, _ = model("S", 0.05, delta, 7)
    got, host_cells, host_count, launches = device("S", 0.05, delta, 7, scratch_limit=64 << 20)
    print("pack launches:", launches)
    assert launches[0] >= 3, launches
    assert (got == want).all(), np.argwhere(got != want)[:10]
    if delta is None:
        assert host_count == 0 and not host_cells.any()
    else:
        assert (host_cells == nan_mean).all() and host_count == nan_mean.sum()
        tenth = len(want) // 10
        assert host_cells[:tenth].any() and host_cells[-tenth:].any()


@pytest.mark.parametrize("delta", [None, 0.05])
def test_paint_across_a_pass_that_starts_over(delta):
    """case F on a fresh engine: the long windows' virtual sites overflow the default reservation, the pass runs again with the worst-case
    one -- and the list of cells for the host starts again with it.  A second call on the same engine packs half as often: the
    evidence that the first was repeated"""
    want, nan_mean, _ = model("F", 0.05, delta, 7)
    got, host_cells, host_count, launches = device("F", 0.05, delta, 7, calls=2)
    print("pack launches:", launches)
    assert launches[1] >= 1 and launches[0] == 2 * launches[1], launches
    assert (got == want).all(), np.argwhere(got != want)[:10]
    if delta is not None:
        assert nan_mean.any() and (host_cells == nan_mean).all() and host_count == nan_mean.sum()
