"""-m gpu: the fused form of k_pack3 (csrc/pg_pair2.hip: the called counts C formed inside the pack kernel, no called plane).
Everything is an integer, so every comparison is array_equal: pairCounts() against the oracle and against the same call under
PG_PACK_FUSE=0 (the two kernels the fused form replaces), over the unit counts around its tile edges, the window lengths around its
word, K-step and 8-word iteration edges, parts with atomics, the `mismatch` redo and the XV overflow redo.  The library takes the
fused form by itself from 1024 windows a call and more than 128 units on; PG_PACK_FUSE=1 takes it anywhere in its domain, which is
how the small shapes here reach it."""
import numpy as np
import pytest

from genomics_general_amd import synth
from genomics_general_amd.engine import Engine
from genomics_general_amd.samples import HapLayout, SampleData
from oracle import popgen_oracle as orc

import gpu_util as G

pytestmark = pytest.mark.gpu

PG_K_PAIRWISE = 1               # include/popgen_hip.h: the called-count kernel's timing family


def ploidy_layout(ploidies, n_pops):
    names = ["s%d" % i for i in range(len(ploidies))]
    per = max(1, len(names) // n_pops)
    pops = [names[k * per:(k + 1) * per] for k in range(n_pops)]
    pops[-1] += names[n_pops * per:]
    pops = [p for p in pops if p]
    sd = SampleData(indNames=list(names), popNames=["p%d" % k for k in range(len(pops))], popInds=pops,
                    ploidyDict=dict(zip(names, ploidies)))
    return names, HapLayout(sd, names, "phased")


def oracle_counts(lay, codes, lo, hi):
    aln, _ = orc.aln_from_codes(codes[lo:hi], lay.hap_names, lay.hap_sample_name,
                                [g if g is not None else "~none" for g in lay.hap_group])
    return orc.pair_counts_gemm(aln)


def mostly_biallelic(rng, L, n_hap, p_miss=0.1):
    """random genotypes, 10 % missing, most sites pulled towards one allele (as real data), some with three and four alleles left"""
    codes = (1 << rng.integers(0, 4, size=(L, n_hap))).astype(np.int8)
    codes[rng.random((L, n_hap)) < p_miss] = 0
    ref = (1 << rng.integers(0, 4, size=(L, 1))).astype(np.int8)
    keep = rng.random((L, n_hap)) < 0.7
    return np.where(keep & (codes != 0), ref, codes).astype(np.int8)


def diploid_called(rng, codes):
    """missing genotypes per individual (both slots), so that the diploid shortcut holds"""
    miss = np.repeat(rng.random((codes.shape[0], codes.shape[1] // 2)) < 0.1, 2, axis=1)
    out = np.where(codes == 0, np.int8(1), codes)
    out[miss] = 0
    return out


def counts_both_ways(e, wins, monkeypatch, fused_expected, force=True):
    """(D, C) of the call under PG_PACK_FUSE=1 (the fused form whatever the number of windows, inside its domain; force=False: the
    library's own choice), checked against the same call under PG_PACK_FUSE=0; and which path the first call took: the called-count
    family records a launch only when its kernel runs"""
    lo, hi = [w[0] for w in wins], [w[1] for w in wins]
    e.kernel_time_select(None)
    e.kernel_time_reset()
    if force:
        monkeypatch.setenv("PG_PACK_FUSE", "1")
    D, C = e.batch(lo, hi).pairCounts(reference_order=True)
    launches = e.kernel_time(PG_K_PAIRWISE)[1]
    assert (launches == 0) == fused_expected, "called-count launches: %d" % launches
    monkeypatch.setenv("PG_PACK_FUSE", "0")
    e.kernel_time_reset()
    D0, C0 = e.batch(lo, hi).pairCounts(reference_order=True)
    assert e.kernel_time(PG_K_PAIRWISE)[1] > 0 or not wins
    monkeypatch.delenv("PG_PACK_FUSE")
    assert np.array_equal(C, C0), "C differs from the PG_PACK_FUSE=0 call"
    assert np.array_equal(D, D0), "D differs from the PG_PACK_FUSE=0 call"
    return D, C


def check_oracle(lay, codes, wins, D, C):
    for k, (a, b) in enumerate(wins):
        Do, Co = oracle_counts(lay, codes, a, b)
        assert np.array_equal(C[k], Co), "C differs from the oracle in window %d = [%d, %d)" % (k, a, b)
        assert np.array_equal(D[k], Do), "D differs from the oracle in window %d = [%d, %d)" % (k, a, b)


# units of the called counts: individuals of a diploid layout, haplotypes otherwise; 224 = 7 tiles of 32 is the last fused count
@pytest.mark.parametrize("name,ploidies,fused", [
    ("dip1", [2] * 1, True), ("dip31", [2] * 31, True), ("dip32", [2] * 32, True), ("dip33", [2] * 33, True),
    ("dip100", [2] * 100, True), ("dip200", [2] * 200, True), ("dip224", [2] * 224, True), ("dip225", [2] * 225, False),
    ("hap1", [1] * 1, True), ("hap33", [1] * 33, True), ("hap100", [1] * 100, True), ("hap224", [1] * 224, True),
    ("hap225", [1] * 225, False),
    ("mixed48", [2, 1, 2, 2, 1, 1, 2, 1] * 4, True), ("mixed223", [2, 1] * 74 + [1], True), ("mixed225", [2, 1] * 75, False),
])
def test_unit_counts_and_ploidies(name, ploidies, fused, monkeypatch):
    names, lay = ploidy_layout(ploidies, min(4, len(ploidies)))
    rng = np.random.default_rng(1000 + lay.n_hap)
    L = 2100
    codes = mostly_biallelic(rng, L, lay.n_hap)
    if all(p == 2 for p in ploidies):
        codes = diploid_called(rng, codes)
    e = Engine(0)
    e.set_layout(lay)
    e.load_sites(codes)
    wins = [(0, L), (3, 1027), (777, 778), (50, 50)]
    D, C = counts_both_ways(e, wins, monkeypatch, fused)
    check_oracle(lay, codes, wins, D, C)
    e.close()


# word (32 sites), K step (64) and iteration (8 words = 256 sites) edges, an empty window, 50 000 sites; few windows: parts + atomics
@pytest.mark.parametrize("n_dip", [200, 20])
def test_window_lengths(n_dip, monkeypatch):
    names, lay = G.make_layout(n_dip, 4)
    rng = np.random.default_rng(n_dip)
    L = 51000
    codes = diploid_called(rng, mostly_biallelic(rng, L, lay.n_hap))
    e = Engine(0)
    e.set_layout(lay)
    e.load_sites(codes)
    wins = [(7, 7), (9, 10), (100, 131), (200, 232), (300, 333), (1001, 1256), (2000, 2256), (3003, 3260), (777, 50777)]
    D, C = counts_both_ways(e, wins, monkeypatch, True)
    check_oracle(lay, codes, wins, D, C)
    # one long window alone: cut into many parts, every count arrives through atomics
    wins = [(13, 50013)]
    D, C = counts_both_ways(e, wins, monkeypatch, True)
    check_oracle(lay, codes, wins, D, C)
    e.close()


# by itself the library takes the fused form from 1024 windows a call and more than 128 units on
@pytest.mark.parametrize("n_dip,own_choice", [(40, False), (130, True)])
def test_thousands_of_tiny_windows(n_dip, own_choice, monkeypatch):
    names, lay = G.make_layout(n_dip, 4)
    rng = np.random.default_rng(5)
    n_win = 3000
    L = 17 * n_win + 40
    codes = diploid_called(rng, mostly_biallelic(rng, L, lay.n_hap))
    e = Engine(0)
    e.set_layout(lay)
    e.load_sites(codes)
    wins = [(17 * k + (k % 5), 17 * k + (k % 5) + 1 + (k * 7) % 40) for k in range(n_win)]
    D, C = counts_both_ways(e, wins, monkeypatch, True)
    check_oracle(lay, codes, wins, D, C)
    D1, C1 = counts_both_ways(e, wins, monkeypatch, own_choice, force=False)
    assert np.array_equal(D1, D) and np.array_equal(C1, C)
    counts_both_ways(e, wins[:1000], monkeypatch, False, force=False)        # fewer than 1024 windows: the two kernels
    e.close()


@pytest.mark.parametrize("fill", ["all_called", "all_missing"])
def test_all_called_and_all_missing_rows(fill, monkeypatch):
    names, lay = G.make_layout(100, 4)
    rng = np.random.default_rng(11)
    L = 3000
    codes = (1 << rng.integers(0, 2, size=(L, lay.n_hap))).astype(np.int8) if fill == "all_called" else np.zeros((L, lay.n_hap), np.int8)
    e = Engine(0)
    e.set_layout(lay)
    e.load_sites(codes)
    wins = [(0, L), (1, 258), (100, 1900)]
    D, C = counts_both_ways(e, wins, monkeypatch, True)
    check_oracle(lay, codes, wins, D, C)
    if fill == "all_called":
        assert all(C[k][0, 1] == b - a for k, (a, b) in enumerate(wins))
    else:
        assert not C.any() and not D.any()
    e.close()


# one allele of one individual missing: the diploid shortcut is withdrawn (flag bit 0) and the call runs again with haploid units --
# 200 of them are still fused, 400 take the two kernels
@pytest.mark.parametrize("n_dip,fused_after_redo", [(100, True), (200, False)])
def test_one_allele_missing_redoes_with_haploid_units(n_dip, fused_after_redo, monkeypatch):
    names, lay = G.make_layout(n_dip, 4)
    rng = np.random.default_rng(21 + n_dip)
    L = 2600
    codes = diploid_called(rng, mostly_biallelic(rng, L, lay.n_hap))
    codes[1999, 2 * (n_dip - 1) + 1] = 0
    codes[1999, 2 * (n_dip - 1)] = 4
    e = Engine(0)
    e.set_layout(lay)
    e.load_sites(codes)
    wins = [(0, L), (1500, 2100), (0, 1999)]
    D, C = counts_both_ways(e, wins, monkeypatch, fused_after_redo)
    check_oracle(lay, codes, wins, D, C)
    e.close()


def test_xv_overflow_redoes_with_the_worst_case_reservation(monkeypatch):
    """every site with four alleles: three virtual sites per site, more than the default reservation of one (flag bit 1)"""
    names, lay = G.make_layout(100, 4)
    rng = np.random.default_rng(31)
    L = 4200
    codes = diploid_called(rng, (1 << rng.integers(0, 4, size=(L, lay.n_hap))).astype(np.int8))
    e = Engine(0)
    e.set_layout(lay)
    e.load_sites(codes)
    wins = [(0, L), (100, 4000), (5, 300)]
    D, C = counts_both_ways(e, wins, monkeypatch, True)
    check_oracle(lay, codes, wins, D, C)
    e.close()


def test_parts_stay_below_the_exact_range_of_f32(monkeypatch):
    """a window of 9 * 10^6 sites, every genotype called: the counts pass 2^23, no part may (an accumulator holds count / 4)"""
    names, lay = G.make_layout(8, 2)
    L = 9_000_000
    rng = np.random.default_rng(41)
    codes = (1 << rng.integers(0, 2, size=(L, lay.n_hap))).astype(np.int8)
    codes[::1000, 0:2] = 0
    e = Engine(0)
    e.set_layout(lay)
    e.load_sites(codes)
    e.kernel_time_select(None)
    e.kernel_time_reset()
    monkeypatch.setenv("PG_PACK_FUSE", "1")
    D, C = e.batch([0], [L]).pairCounts(reference_order=False)
    assert e.kernel_time(PG_K_PAIRWISE)[1] == 0
    called = (codes != 0).astype(np.float64)
    Co = np.zeros((lay.n_hap, lay.n_hap))
    Do = np.zeros((lay.n_hap, lay.n_hap))
    for a in range(0, L, 1_000_000):
        v = called[a:a + 1_000_000]
        Co += v.T @ v
        same = sum(((codes[a:a + 1_000_000] == al).astype(np.float64)).T @ (codes[a:a + 1_000_000] == al).astype(np.float64) for al in (1, 2))
        Do += v.T @ v - same
    np.fill_diagonal(Co, 0)
    np.fill_diagonal(Do, 0)
    assert C[0].max() > (1 << 23)
    assert np.array_equal(C[0], Co.astype(np.int64)) and np.array_equal(D[0], Do.astype(np.int64))
    e.close()


def test_group_dist_table_on_the_c2_shape_bit_for_bit(monkeypatch):
    """10^7 sites x 100 diploids, 4 populations, 200 windows of 50 kb (BASELINE.json configs[1], generated on the device)"""
    n_dip, n_pops, n_sites, wind = 100, 4, 10_000_000, 50_000
    names, lay = G.make_layout(n_dip, n_pops)
    e = Engine(0)
    e.set_layout(lay)
    e.reserve(n_sites)
    e.synth_fill(0, n_sites, 0, synth.SEED_DEFAULT, n_sites // 4, n_dip, n_pops, G.slot_gen_hap(names, lay), synth.VAR_THR, synth.MISS_THR)
    lo = np.arange(0, n_sites, wind, dtype=np.int64)
    hi = lo + wind
    e.kernel_time_select(None)
    e.kernel_time_reset()
    monkeypatch.setenv("PG_PACK_FUSE", "1")
    tab, cols = e.batch(lo, hi).groupDistTable(True, 100, 0.01)
    fused = e.kernel_time(PG_K_PAIRWISE)[1] == 0
    monkeypatch.setenv("PG_PACK_FUSE", "0")
    tab0, cols0 = e.batch(lo, hi).groupDistTable(True, 100, 0.01)
    monkeypatch.delenv("PG_PACK_FUSE")
    e.kernel_time_reset()
    tab1, cols1 = e.batch(lo, hi).groupDistTable(True, 100, 0.01)
    assert fused, "the c2 shape is inside the fused form's domain"
    assert e.kernel_time(PG_K_PAIRWISE)[1] > 0, "200 windows x 100 units: the library's own choice is the two kernels (measured faster)"
    assert cols == cols0 and tab.shape == tab0.shape and tab.tobytes() == tab0.tobytes() and tab1.tobytes() == tab0.tobytes()
    assert np.isfinite(tab).any()
    e.close()
