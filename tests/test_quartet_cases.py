"""Without a GPU: the cases of tests/quartet_cases.py contain what they are built for -- shown from the oracle (oracle/popgen_oracle.py)
and NumPy alone, so that a device test that passes on them has met the things it is meant to meet.

Shares measured with NumPy 2.2.6 (each is asserted below with the bound given in its test; the tests print them again):
  missing calls        N 6.8 %, N50 50.4 %, the wide cases 7.2 .. 7.7 %
  outside alleles      sites biallelic in the quartet with a third allele in a slot outside it: N 1654 and 1547 of 5350 and 5286
                       (the two quartets), N50 1354 / 1198, E256 672 / 719, E257 606 / 625, E512 378 / 356, E513 374 / 335,
                       E1024 387 / 343, E1025 401 / 315; at least 300 of them are good sites under minData 0.3 in every case
                       sites biallelic in the row and monomorphic in the quartet: 136 (E1024) .. 1196 (N50)
  50:50 sites          N, whole range, minData 0.3: 40 .. 65 per pair of bases in the quartet of 18 haplotypes, 9 .. 14 in the one of 46
  used under `fixed`   whole range: N 1756 / 1601, N50 (minData 0) 1154 / 914, the wide cases 194 (E512) .. 361 (E256)
  used sites per wave  of the first 4096-site block of the whole-range window: 262 .. 607 under ABBABABA, 481 .. 613 under `minor`
                       (`fixed`: 38 .. 212: there the candidate ring wraps and the ring of usable sites does not in the wide cases)
  0 / 0 frequencies    N50, minData 0: 378 and 2028 used sites with a population without a call under ABBABABA / `polarize`, 2837 under
                       `minor`, none under `fixed`; every sum of the whole-range window is nan but under `fixed`
  minData == k / N     N: 1/3 of p5 kept with n == 1 at 124 and 136 sites, dropped with n == 0 at 1 and 1; 3/5 of p4: 67 kept, 19
                       dropped; 5/9 of p1: 53 and 45 kept, 25 and 23 dropped
  left out of the tree-order comparison (window, statistic): N 58 of 6560 (0.9 %), N50 25 of 1394 (1.8 %, minData 0.3), E256 1.4 %,
                       E257 3.7 %, E512 0.1 %, E513 3.3 %, E1024 1.1 %, E1025 2.0 %
  groupFreqStats       complete sites of the whole range 2503 .. 2719; S of a population 300 .. 879; without the individuals in no
                       population 16 (F13) and 8 (F16) more sites would be complete"""
import numpy as np
import pytest

import quartet_cases as QC
from oracle import popgen_oracle as orc


def _alleles_of(gt, cols):
    """bit mask of the alleles called among the slots `cols` at every site"""
    return np.bitwise_or.reduce(gt[:, cols].astype(np.uint8), axis=1) if len(cols) else np.zeros(len(gt), dtype=np.uint8)


def _popcount4(m):
    return (m & 1) + ((m >> 1) & 1) + ((m >> 2) & 1) + ((m >> 3) & 1)


def _quartet_slots(c, quartet):
    inside = np.zeros(c["lay"].n_hap, dtype=bool)
    for pop in quartet:
        s, e = QC.pop_range(c, pop)
        inside[s:e] = True
    return inside


@pytest.mark.parametrize("name", QC.QUARTET_CASES)
def test_sites_counted_with_numpy_are_the_oracles_used_sites(name):
    """quartet_cases.site_flags (what the conditions below are read from) gives the oracle's sitesUsed in every window, quartet,
    minData and mode: nan (ABBABABA) or 0 (fourPop) without a good site"""
    c = QC.case(name)
    for qi in range(len(c["quartets"])):
        for md in QC.min_datas(name):
            for mode in QC.MODES:
                good, used = QC.site_flags(name, qi, md, mode)
                for (a, b), (want, _) in zip(c["wins"], QC.expect(name, qi, md, mode)):
                    if good[a:b].sum() == 0:
                        assert (np.isnan(want["sitesUsed"]) if mode == "abba" else want["sitesUsed"] == 0), (qi, md, mode, a, b)
                    else:
                        assert want["sitesUsed"] == used[a:b].sum(), (qi, md, mode, a, b, want["sitesUsed"], used[a:b].sum())


@pytest.mark.parametrize("name", QC.QUARTET_CASES)
def test_third_alleles_outside_the_quartet_and_sites_monomorphic_in_it(name):
    c = QC.case(name)
    gt = c["gt"]
    every = _alleles_of(gt, np.arange(c["lay"].n_hap))
    for qi, quartet in enumerate(c["quartets"]):
        inside = _quartet_slots(c, quartet)
        assert inside.sum() < c["lay"].n_hap
        a_in, a_out = _alleles_of(gt, np.flatnonzero(inside)), _alleles_of(gt, np.flatnonzero(~inside))
        biallelic = _popcount4(a_in) == 2
        outside_third = biallelic & ((a_out & ~a_in) != 0)
        mono = (_popcount4(a_in) == 1) & (_popcount4(every) == 2)
        good, used = QC.site_flags(name, qi, 0.3, "minor")
        print(name, quartet, "biallelic in the quartet: %d, of them with another allele outside it: %d (good under minData 0.3: %d); "
              "biallelic in the row and monomorphic in the quartet: %d" % (biallelic.sum(), outside_third.sum(), (outside_third & good).sum(), mono.sum()))
        assert outside_third.sum() >= 200 and (outside_third & good).sum() >= 100 and mono.sum() >= 20
        # the windows without a good site: no call in the quartet
        for a, b in c["wins"][8:10]:
            assert b - a == QC.BLANK and not gt[a:b][:, inside].any()


@pytest.mark.parametrize("name", QC.QUARTET_CASES)
def test_slot_ranges_of_the_chosen_populations_start_and_end_at_every_kind_of_nibble(name):
    c = QC.case(name)
    chosen = sorted({pop for quartet in c["quartets"] for pop in quartet})
    ranges = [QC.pop_range(c, pop) for pop in chosen]
    starts, ends = {s % 8 for s, _ in ranges}, {e % 8 for _, e in ranges}
    assert {0, 1, 7} <= starts and {0, 1, 7} <= ends, (ranges, starts, ends)
    assert any(s >> 3 == (e - 1) >> 3 for s, e in ranges)                  # inside one dword of eight slots
    assert any(e - s > 32 and s % 32 != 0 for s, e in ranges)              # several 16-byte loads, the first from inside its piece
    names = c["lay"].sampleData.popNames
    for quartet in c["quartets"]:
        ids = [names.index(p) for p in quartet]
        assert ids != sorted(ids) and len(set(ids)) == 4
        assert set(range(len(names))) - set(ids)                           # somebody is left out
    # one quartet has the outgroup first of the four in the row and P1 last
    assert any(names.index(q[3]) == min(names.index(p) for p in q) and names.index(q[0]) == max(names.index(p) for p in q) for q in c["quartets"])
    left_out = [set(range(len(names))) - {names.index(p) for p in q} for q in c["quartets"]]
    lows, highs = [min(names.index(p) for p in q) for q in c["quartets"]], [max(names.index(p) for p in q) for q in c["quartets"]]
    before = any(x < lo for s, lo in zip(left_out, lows) for x in s)
    between = any(lo < x < hi for s, lo, hi in zip(left_out, lows, highs) for x in s)
    behind = any(x > hi for s, hi in zip(left_out, highs) for x in s) or c["lay"].n_hap > c["start"][-1]
    assert before and between, (name, left_out)
    if len(names) >= 6:
        assert behind and all(len(s) >= 2 for s in left_out)
    if name in ("N", "N50"):
        solo = names[c["lay"].pop_sizes.index(1)]
        assert [q[1] for q in c["quartets"]].count(solo) == 1 and c["lay"].n_hap - c["start"][-1] == 4
        assert all(any(x < lo for x in s) and any(lo < x < hi for x in s) and any(x > hi for x in s)
                   for s, lo, hi in zip(left_out, lows, highs))


def test_widths_stand_on_both_sides_of_every_dispatch_border():
    want = {"E256": 256, "E257": 257, "E512": 512, "E513": 513, "E1024": 1024, "E1025": 1025}
    for name, slots in want.items():
        assert QC.case(name)["lay"].n_hap == slots
    assert QC.case("N")["lay"].n_hap == 73 and sorted(QC.case("N")["lay"].pop_sizes) == [1, 3, 5, 7, 9, 11, 33]
    assert np.array_equal(QC.case("N")["lay"].hap_pop, QC.case("N50")["lay"].hap_pop)
    for name in QC.QUARTET_CASES:
        lay = QC.case(name)["lay"]
        assert sorted(set(len(lay.ind_slots[nm]) for nm in lay.ind_order)) == [1, 2]
        miss = (QC.case(name)["gt"] == 0).mean()
        print(name, "missing calls: %.3f" % miss)
        assert (0.45 < miss < 0.55) if name == "N50" else (0.05 < miss < 0.08)


def test_windows_are_the_ones_the_device_tests_need():
    for L in (QC.L_NARROW, QC.L_WIDE):
        w = QC.windows(L)
        assert w[0] == (0, L) and (1, 4100) in w
        assert any(b - a == 4096 and b == a + 4096 for a, b in w) and any(b - a == 4097 for a, b in w)
        assert any(a == b for a, b in w) and any(b - a == 1 for a, b in w)
        assert sum(1 for a, b in w if 0 < b - a <= 256 and a % 128 and b - a > QC.BLANK) >= 2
        assert all(0 <= a <= b <= L for a, b in w)
        assert sum(1 for a, b in w if 256 < b - a < 4096) >= 10                      # fixed trees without a chunk seam
    lo, hi, which, distinct = QC.turn_windows()
    assert len(lo) == 65535 + 65 and lo[:65535].max() < 4000 and lo[65535:].min() >= 8000 and (hi - lo).max() <= 256 and hi.max() <= QC.L_NARROW
    assert 35 <= len(distinct) <= 45 and set(which[:65535]) | set(which[65535:]) == set(range(len(distinct)))
    assert (hi[:65535] == lo[:65535]).any()
    good, _ = QC.site_flags("N", 0, 0.3, "minor")
    for part in (slice(0, 65535), slice(65535, None)):
        n_good = [int(good[a:b].sum()) for a, b in zip(lo[part][:64], hi[part][:64])]
        assert 0 in [g for g, a, b in zip(n_good, lo[part], hi[part]) if b > a] and max(n_good) > 20       # a window without a good site in each launch


def test_minor_allele_ties_of_every_pair_of_bases():
    c = QC.case("N")
    for qi in range(len(c["quartets"])):
        cnt, _ = QC.quartet_counts("N", qi)
        good, _ = QC.site_flags("N", qi, 0.3, "minor")
        tot = cnt.sum(axis=0)[good]
        ties = {}
        for row in tot:
            i, j = np.flatnonzero(row > 0)
            if row[i] == row[j]:
                ties[(int(i), int(j))] = ties.get((int(i), int(j)), 0) + 1
        print("N", c["quartets"][qi], "50:50 sites by pair of bases:", dict(sorted(ties.items())))
        assert set(ties) == set(orc.MINOR_TIE) and min(ties.values()) >= 5, ties


@pytest.mark.parametrize("name", QC.QUARTET_CASES)
def test_fixed_keeps_sites_and_every_wave_fills_its_rings_more_than_once(name):
    """a wave of k_abba_q (a quarter of a 4096-site block) has more than 128 used sites in the whole-range window: PG_ABBA_RING and
    PG_ABBA_CAND (128 entries each; every used site was a candidate first) wrap"""
    c = QC.case(name)
    md = 0 if name == "N50" else 0.3
    for qi in range(len(c["quartets"])):
        _, used = QC.site_flags(name, qi, md, "fixed")
        share = {mode: QC.wave_share(name, qi, md, mode) for mode in ("abba", "minor", "fixed")}
        print(name, c["quartets"][qi], "minData", md, "used under fixed:", int(used.sum()), "used per wave of the first block:", share)
        assert used.sum() >= 100
        assert min(share["abba"]) > 128 and min(share["minor"]) > 128


def test_half_missing_rows_have_zero_by_zero_frequencies_among_the_used_sites():
    c = QC.case("N50")
    for qi in range(len(c["quartets"])):
        _, n = QC.quartet_counts("N50", qi)
        for mode in QC.MODES:
            _, used = QC.site_flags("N50", qi, 0, mode)
            empty = used & (n == 0).any(axis=0)
            want = QC.expect("N50", qi, 0, mode)[0][0]
            nan_sums = [k for k, v in want.items() if k != "sitesUsed" and np.isnan(v)]
            print("N50", c["quartets"][qi], mode, "used sites with a population without a call:", int(empty.sum()), "nan:", nan_sums)
            if mode == "fixed":
                assert empty.sum() == 0                    # (0 / 0 is neither 0 nor 1: genomics.py:1611-1614)
            else:
                assert empty.sum() >= 1 and nan_sums


def test_min_data_of_exactly_k_of_n_has_sites_on_both_sides():
    c = QC.case("N")
    for md, pop, k in QC.GRID:
        s, e = QC.pop_range(c, pop)
        assert k * 1. / (e - s) == md and (k - 1) * 1. / (e - s) < md
        found = 0
        for qi, quartet in enumerate(c["quartets"]):
            if pop not in quartet:
                continue
            z = quartet.index(pop)
            _, n = QC.quartet_counts("N", qi)
            good, _ = QC.site_flags("N", qi, md, "minor")
            # what the site would be if this population's count were of no concern: good under minData 0 and enough data elsewhere
            loose, _ = QC.site_flags("N", qi, 0, "minor")
            others = np.ones(c["L"], dtype=bool)
            for y, other in enumerate(quartet):
                if y != z:
                    so, eo = QC.pop_range(c, other)
                    others &= n[y] * 1. / (eo - so) >= md
            kept, dropped = int((good & (n[z] == k)).sum()), int((loose & others & ~good & (n[z] == k - 1)).sum())
            print("N minData %r = %d/%d of %s in %s: kept with n == k: %d, dropped with n == k - 1: %d" % (md, k, e - s, pop, quartet, kept, dropped))
            assert kept >= 1 and dropped >= 1
            found += 1
        assert found >= 1


@pytest.mark.parametrize("name", QC.QUARTET_CASES)
def test_tree_order_comparison_leaves_few_pairs_out(name):
    """quartet_cases.order_bound leaves at most 5 % of the (window, statistic) pairs of a case out (N50: under minData 0.3; under
    minData 0 nearly every sum of its windows is nan, which is what it is there for)"""
    c = QC.case(name)
    out = total = 0
    for qi in range(len(c["quartets"])):
        for md in QC.min_datas(name):
            if name == "N50" and md == 0:
                continue
            for mode in QC.MODES:
                for want, sums in QC.expect(name, qi, md, mode):
                    for key, entry in sums.items():
                        total += 1
                        out += QC.order_bound(entry, want[key]) is None
    print(name, "left out of the tree-order comparison: %d of %d pairs (%.1f %%)" % (out, total, 100.0 * out / total))
    assert total >= 1000 and 20 * out <= total, (out, total)


@pytest.mark.parametrize("name", QC.FREQ_CASES)
def test_group_freq_cases_have_complete_sites_and_every_population_polymorphic(name):
    c = QC.case(name)
    lay = c["lay"]
    exp = QC.freq_expect(name)
    pops = QC.freq_pops(name)
    whole = exp[0]
    print(name, "slots", lay.n_hap, "populations", lay.n_pops, "complete sites", whole["l_" + pops[0]], "S", [whole["S_" + p] for p in pops])
    assert whole["l_" + pops[0]] > 1000 and all(whole["S_" + p] > 50 for p in pops)
    assert sum(1 for w in exp if w["l_" + pops[0]] >= 1) >= len(exp) - 4              # all but the empty and the blank windows
    if name.startswith("F"):
        assert lay.n_pops == {"F13": 13, "F16": 16, "F16w": 16, "F16x": 16}[name] and min(lay.pop_sizes) >= 2
        assert {"F13": 85 < lay.n_hap < 100, "F16": 85 < lay.n_hap < 100, "F16w": 650 < lay.n_hap <= 1024, "F16x": lay.n_hap > 1024}[name]
    if name in ("F13", "F16"):
        # the individuals in no population void sites: without their rows more sites are complete
        full = QC.full_aln(name, True)
        keep = np.array([g != "~none" for g in full.groups])
        assert 0 < (~keep).sum() <= 4
        without = int(np.all(full.mask[keep], axis=0).sum())
        print(name, "complete sites without the individuals in no population:", without)
        assert whole["l_" + pops[0]] < without


def test_seventeen_populations_are_one_more_than_the_kernels_take():
    assert QC.case("F17")["lay"].n_pops == 17 and QC.case("F16")["lay"].n_pops == 16
