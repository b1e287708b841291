"""-m gpu: the site-statistics kernels -- k_abba_q, k_abba_reduce, k_quartet_np (WindowBatch.ABBABABA, fourPop) and k_popfreq_q,
k_popfreq, k_popfreq_ordered (groupFreqStats) -- against the oracle on the cases of tests/quartet_cases.py: quartets out of slot order
with populations and unassigned individuals left out (third alleles among them), rows on both sides of every dispatch border of the
row width (256 | 257, 512 | 513, 1024 | 1025 slots: all four NPASS forms of k_abba_q with six and with fourteen sums, k_popfreq_q<1, 2, 4>
and k_popfreq), windows across the 4096-site block, minData of exactly k / N, 13 and 16 populations, and more than 65535 windows.
tests/test_quartet_cases.py shows without a GPU that the cases contain all this.  The expectations are the oracle's alone: bit for
bit (gpu_util.same) in NumPy's order; in the fixed trees within the bound that the oracle's own sums give (quartet_cases.order_bound)."""
import numpy as np
import pytest

import gpu_util as G
import quartet_cases as QC
from genomics_general_amd._lib import PopgenError
from oracle import popgen_oracle as orc

pytestmark = pytest.mark.gpu

ABBA_STATS = ("D", "fd", "fdM", "ABBA", "BABA")
PLAIN_SUMS = ("ABBA", "BABA", "ABAA", "BAAA")


def engine_of(c):
    e = G.Engine(0)
    e.set_layout(c["lay"])
    e.load_sites(c["gt"])
    return e


def run_mode(wb, quartet, min_data, mode):
    if mode == "abba":
        return wb.ABBABABA(*quartet, min_data)
    return wb.fourPop(*quartet, min_data, polarize=mode == "polarize", fixed=mode == "fixed")


def assert_used(mode, got, want, where):
    if mode == "abba":
        assert G.same(got, want), where + (got, want)                  # nan without a good site (genomics.py:1693-1695)
    else:
        assert got == want, where + (got, want)


def assert_bit_for_bit(name, qi, min_data, mode, got, windows=None):
    """every statistic of every window (or of `windows`: (index in got, index in the case)) == the oracle's"""
    expect = QC.expect(name, qi, min_data, mode)
    for k, w in (windows if windows is not None else [(w, w) for w in range(len(expect))]):
        want, sums = expect[w]
        where = (name, qi, min_data, mode, QC.case(name)["wins"][w])
        assert_used(mode, got["sitesUsed"][k], want["sitesUsed"], where)
        for key in (ABBA_STATS if mode == "abba" else orc.FOURPOP_STATS):
            if mode != "abba" and not sums:
                # fourPop without a good site: the reference answers nan for everything; WindowBatch.fourPop leaves the empty sums
                # of such a window (0.0, and 0 / 0 for the ratios) to its caller, who prints nan below minSites used sites
                g = got[key][k]
                assert (G.same(g, 0.0) if key in PLAIN_SUMS else np.isnan(g)), where + (key, g)
            else:
                assert G.same(got[key][k], want[key]), where + (key, got[key][k], want[key])


@pytest.mark.parametrize("name", QC.QUARTET_CASES)
def test_quartet_statistics_in_numpy_order_equal_the_oracle_bit_for_bit(name):
    c = QC.case(name)
    e = engine_of(c)
    try:
        e.set_sum_order(1)                   # NumPy's order for every window (k_quartet_np over the flags of k_abba_q)
        wb = e.batch([w[0] for w in c["wins"]], [w[1] for w in c["wins"]])
        for qi, quartet in enumerate(c["quartets"]):
            for md in QC.min_datas(name):
                for mode in QC.MODES:
                    assert_bit_for_bit(name, qi, md, mode, run_mode(wb, quartet, md, mode))
    finally:
        e.close()


@pytest.mark.parametrize("name", QC.QUARTET_CASES)
def test_quartet_statistics_in_the_fixed_trees_lie_within_the_bound_of_their_sums(name):
    """set_sum_order(2): the partial sums of k_abba_q's blocks, added up by k_abba_reduce -- the order fourPopWindows.py and
    ABBABABAwindows.py get for every window above 256 sites.  The per-site terms are those of the NumPy order (quartet_values), so
    the difference is the order of the additions alone: quartet_cases.order_bound, from the oracle's own sums"""
    c = QC.case(name)
    e = engine_of(c)
    compared = left_out = 0
    worst = 0.0
    try:
        e.set_sum_order(2)
        wb = e.batch([w[0] for w in c["wins"]], [w[1] for w in c["wins"]])
        for qi, quartet in enumerate(c["quartets"]):
            for md in QC.min_datas(name):
                for mode in QC.MODES:
                    got = run_mode(wb, quartet, md, mode)
                    for k, (want, sums) in enumerate(QC.expect(name, qi, md, mode)):
                        where = (name, qi, md, mode, c["wins"][k])
                        assert_used(mode, got["sitesUsed"][k], want["sitesUsed"], where)
                        for key, entry in sums.items():
                            g = got[key][k]
                            bound = QC.order_bound(entry, want[key])
                            if bound is None:
                                left_out += 1
                                if np.isnan(entry[0]) or (entry[2] is not None and np.isnan(entry[2])):
                                    assert np.isnan(g), where + (key, g)             # a nan term makes the sum nan in any order
                                continue
                            compared += 1
                            worst = max(worst, abs(g - want[key]) / bound)
                            assert abs(g - want[key]) <= bound, where + (key, g, want[key], bound)
    finally:
        e.close()
    print(name, "compared %d pairs, left out %d; largest difference / bound: %.3f" % (compared, left_out, worst))
    assert compared >= 1000


@pytest.mark.parametrize("name", QC.QUARTET_CASES)
def test_a_window_alone_gives_the_numbers_it_gives_inside_the_batch(name):
    """the default order, chosen window by window (NumPy's up to 256 sites): the short windows equal the oracle, and every window is
    bit for bit what it is in a batch of its own (k_quartet_np skips the long windows, k_abba_reduce wrote them)"""
    c = QC.case(name)
    mode = ("minor", "polarize", "fixed")[QC.QUARTET_CASES.index(name) % 3]
    qi, md = QC.QUARTET_CASES.index(name) % 2, 0 if name == "N50" else 0.3
    quartet = c["quartets"][qi]
    e = engine_of(c)
    try:
        full = run_mode(e.batch([w[0] for w in c["wins"]], [w[1] for w in c["wins"]]), quartet, md, mode)
        short = [(k, k) for k, (a, b) in enumerate(c["wins"]) if b - a <= 256]
        assert len(short) >= 6
        assert_bit_for_bit(name, qi, md, mode, full, short)
        for k, (a, b) in enumerate(c["wins"]):
            one = run_mode(e.batch([a], [b]), quartet, md, mode)
            for key in full:
                assert G.same(full[key][k], one[key][0]), (name, mode, (a, b), key, full[key][k], one[key][0])
    finally:
        e.close()


def all_same(col, want):
    """every entry of the array is bit for bit the value (or nan with it)"""
    col = np.ascontiguousarray(col, dtype=np.float64)
    if np.isnan(want):
        return bool(np.isnan(col).all())
    return bool((col.view(np.uint64) == np.float64(want).view(np.uint64)).all())


def test_more_than_65535_windows_take_a_second_launch_with_its_own_flags():
    """65535 + 65 short windows of case N in the default order: quartet_stats, pg_popfreq and pg_hap_called cut the batch at 65535
    windows, stage the windows again, and the first two clear the flag words and take another `base` (the first launch lies below
    site 4000, the second from site 8000 on).  One oracle value per distinct window, every copy compared with it"""
    c = QC.case("N")
    lo, hi, which, distinct = QC.turn_windows()
    quartet, md = c["quartets"][0], 0.3
    pops = QC.freq_pops("N")
    e = engine_of(c)
    try:
        wb = e.batch(lo, hi)
        ab, fp, fr, called = wb.ABBABABA(*quartet, md), wb.fourPop(*quartet, md), wb.groupFreqStats(), wb.hapCalled()
    finally:
        e.close()
    assert called.shape == (len(lo), c["lay"].n_hap)
    for d, (a, b) in enumerate(distinct):
        idx = np.flatnonzero(which == d)
        assert len(idx) >= 6
        where = ("window", a, b)
        want, _ = QC.oracle_quartet("N", quartet, md, "abba", a, b)
        for key in ABBA_STATS + ("sitesUsed",):
            assert all_same(ab[key][idx], want[key]), where + (key, ab[key][idx[:3]], want[key])
        want, sums = QC.oracle_quartet("N", quartet, md, "minor", a, b)
        assert (fp["sitesUsed"][idx] == want["sitesUsed"]).all(), where
        for key in orc.FOURPOP_STATS:
            if not sums:                                                # (see assert_bit_for_bit)
                assert (all_same(fp[key][idx], 0.0) if key in PLAIN_SUMS else np.isnan(fp[key][idx]).all()), where + (key,)
            else:
                assert all_same(fp[key][idx], want[key]), where + (key, fp[key][idx[:3]], want[key])
        want = orc.group_freq_stats(QC.window_aln("N", a, b, True))
        for p in pops:
            assert (fr["l_" + p][idx] == want["l_" + p]).all(), where + (p,)
            for st in ("S_", "thetaPi_", "thetaW_", "TajD_"):
                assert all_same(fr[st + p][idx], want[st + p]), where + (st + p, fr[st + p][idx[:3]], want[st + p])
        assert (called[idx] == (c["gt"][a:b] != 0).sum(axis=0)[None, :]).all(), where


@pytest.mark.parametrize("name", QC.FREQ_CASES)
def test_group_freq_stats_with_up_to_sixteen_populations_and_on_every_row_width(name):
    """l, S, thetaPi, thetaW and Tajima's D of every population against the oracle, with the equality of
    test_group_freq_stats_exact_integers; the individuals in no population void sites (their missing calls count, genomics.py:1010)"""
    c = QC.case(name)
    e = engine_of(c)
    try:
        got = e.batch([w[0] for w in c["wins"]], [w[1] for w in c["wins"]]).groupFreqStats()
    finally:
        e.close()
    for k, want in enumerate(QC.freq_expect(name)):
        for p in QC.freq_pops(name):
            for st in ("l_", "S_", "thetaPi_", "thetaW_", "TajD_"):
                g, v = got[st + p][k], want[st + p]
                if st not in ("l_", "S_"):
                    g = float(g)
                assert (g == v) or (g != g and v != v), (name, c["wins"][k], st + p, g, v)


def test_seventeen_populations_are_refused_and_the_engine_goes_on():
    c = QC.case("F17")
    e = engine_of(c)
    try:
        lo, hi = [w[0] for w in c["wins"]], [w[1] for w in c["wins"]]
        with pytest.raises(PopgenError):
            e.batch(lo, hi).groupFreqStats()
        called = e.batch(lo, hi).hapCalled()
        for k, (a, b) in enumerate(c["wins"]):
            assert np.array_equal(called[k], (c["gt"][a:b] != 0).sum(axis=0))
    finally:
        e.close()
