"""-m gpu: distPaint.py on the device.  The goldens of the unmodified reference through cli.distpaint_main, byte for byte (also from
bgzip-compressed input and in blocks of 3 kB); engine.WindowBatch.paint (the pack and pair kernels, k_hap_called for the individuals'
own called counts, k_paint, the host's table of critical rank sums and its finish of the delta cells with a nan mean) against the
NumPy model of tests/paint_model.py with ==, on rows chosen for where the kernel can go wrong:

  case A  70 haploid individuals (more than a wavefront) under names that are not in sorted order; reference populations of 1, 2, 7,
          8, 9 and 33 individuals (around the 8-way unrolled loop of NumPy's sum); windows of 0, 3, 8, 12, 16, 40, 257 and 600 sites
          (one empty, one below minSites; short ones make tied quotients common); 30 % missing calls and minSites 6, so that nan
          pairs (in the windows of 12 and 16 sites: some pairs of a list, not all), an all-nan population and a nan in the best
          population occur;
  case B  200 individuals, populations of 130 (past the 128-value run of NumPy's pairwise sum) and 64.

The model's inputs D and C are counted here with NumPy from the rows, once per case."""
import functools
import gzip
import os

import numpy as np
import pytest

import paint_model
from paint_cases import PAINT_CASES
from genomics_general_amd import cli
from genomics_general_amd.engine import Engine
from genomics_general_amd.samples import HapLayout, SampleData

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
CASES = {
    "A": dict(seed=4101, n=70, sizes=[1, 2, 7, 8, 9, 33], wins=[0, 3, 8, 12, 16, 40, 257, 600], miss=0.30, min_sites=6, n_src=6),
    "B": dict(seed=4102, n=200, sizes=[130, 64], wins=[50, 300, 1000], miss=0.10, min_sites=20, n_src=2),
}


@functools.lru_cache(maxsize=None)
def case_data(name):
    """(layout, rows in slot order, window bounds, reference lists, D, C in the alignment's order with the called counts on C's
    diagonal); individuals are named h0, h1, ... so that the sorted order (h0, h1, h10, ...) is not the file's"""
    p = CASES[name]
    rng = np.random.default_rng(p["seed"])
    n = p["n"]
    names = ["h%d" % k for k in range(n)]
    lay = HapLayout(SampleData(indNames=list(names), ploidyDict={nm: 1 for nm in names}), names, "haplo")
    assert list(lay.ref_order) != list(range(n))
    L = sum(p["wins"])
    # reference individuals: a random choice of the alignment's rows, a population drawing its alleles from its own source; one
    # individual is in two populations and one twice in the same
    perm = rng.permutation(n)
    ref_lists, at = [], 0
    for s in p["sizes"]:
        ref_lists.append([int(v) for v in perm[at:at + s]])
        at += s
    ref_lists[-1][-1] = ref_lists[-1][0]
    ref_lists[0][0] = ref_lists[-1][1]
    src = rng.integers(0, p["n_src"], size=n)                 # by alignment row
    for k, r in enumerate(ref_lists):
        src[r] = k % p["n_src"]
    freq = rng.choice([0.05, 0.3, 0.7, 0.95], size=(L, p["n_src"]))
    # a fifth of the individuals draw every site from a source of its own: near no population in particular (noresult cells)
    src_site = np.where(rng.random(n) < 0.2, rng.integers(0, p["n_src"], size=(L, n)), src[None, :])
    alt = rng.random((L, n)) < np.take_along_axis(freq, src_site, axis=1)
    base = rng.integers(0, 4, size=L)
    allele = np.where(alt, (base[:, None] + 1 + rng.integers(0, 2, size=(L, 1))) % 4, base[:, None])
    rows = (1 << allele).astype(np.int8)                      # allele codes 1, 2, 4, 8; 0 = missing
    rows[rng.random((L, n)) < p["miss"]] = 0
    hi = np.cumsum(p["wins"]).astype(np.int64)
    lo = hi - np.array(p["wins"], dtype=np.int64)
    D = np.zeros((len(lo), n, n), dtype=np.int64)
    C = np.zeros_like(D)
    for w, (a, b) in enumerate(zip(lo, hi)):
        g = rows[a:b].astype(np.int64)
        called = (g != 0).astype(np.int64)
        C[w] = called.T @ called
        D[w] = C[w] - sum((g == code).astype(np.int64).T @ (g == code).astype(np.int64) for code in (1, 2, 4, 8))
    gt = np.zeros((L, n), dtype=np.int8)
    gt[:, lay.ref_order] = rows                               # slot (= file) order: alignment row k is slot ref_order[k]
    return lay, gt, lo, hi, ref_lists, D, C


@functools.lru_cache(maxsize=None)
def model(name, p_threshold, delta_threshold, noresult):
    _, _, _, _, ref_lists, D, C = case_data(name)
    info = {}
    out, nan_mean = paint_model.paint_windows(D, C, ref_lists, CASES[name]["min_sites"], p_threshold=p_threshold,
                                              delta_threshold=delta_threshold, noresult=noresult, info=info)
    return out, nan_mean, info


def device(name, p_threshold, delta_threshold, noresult):
    lay, gt, lo, hi, ref_lists, _, _ = case_data(name)
    e = Engine(0)
    try:
        e.set_layout(lay)
        e.load_sites(gt)
        wb = e.batch(lo, hi)
        out = wb.paint(ref_lists, CASES[name]["min_sites"], p_threshold=p_threshold, delta_threshold=delta_threshold, noresult=noresult)
        return out, wb.paint_host_cells
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


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("p_threshold", [0.05, 0.5])
def test_paint_test_mode_equals_the_model(name, p_threshold):
    want, _, _ = model(name, p_threshold, None, 7)
    got, host_cells = device(name, p_threshold, None, 7)
    assert got.dtype == np.int32 and got.shape == want.shape
    assert (got == want).all(), np.argwhere(got != want)[:10]
    assert not host_cells.any()
    assert (want == 7).any() and (want != 7).any()


@pytest.mark.parametrize("name", ["A", "B"])
@pytest.mark.parametrize("delta", [0.0, 0.05])
def test_paint_delta_mode_equals_the_model(name, delta):
    want, nan_mean, _ = model(name, 0.05, delta, 7)
    got, host_cells = device(name, 0.05, delta, 7)
    assert (got == want).all(), np.argwhere(got != want)[:10]
    # the host finishes exactly the cells with a nan among their means
    assert (host_cells == nan_mean).all()
    if name == "A":
        assert nan_mean.any()


def test_paint_with_the_popcount_pair_kernels(monkeypatch):
    monkeypatch.setenv("PG_PAIR_VALU", "1")
    for delta in (None, 0.05):
        want, nan_mean, _ = model("A", 0.05, delta, 7)
        got, host_cells = device("A", 0.05, delta, 7)
        assert (got == want).all() and (host_cells == (nan_mean if delta is not None else False)).all()
