"""Without a GPU: the cases of tests/finisher_cases.py contain what they are built for -- shown from the oracle (oracle/popgen_oracle.py)
and the NumPy model (tests/paint_model.py) alone, so that a device test that passes on them has met the things it is meant to meet.

Shares measured with NumPy 2.2.6 (each is asserted below with the bound given in its test; the tests print them again):
  hapStats  2367 cells (case, state, maxDist, window, population) over Hs, Hd, Dd, DdN and X4
            clusters per cell: 317 below 8, 1513 in 8 .. 128, 381 in 129 .. 256, 87 in 257 .. 512, 69 above 512
            the left-to-right sum of f^2 differs from the oracle's H1 in 1169 of the 1970 cells with 16 clusters or more (59 %;
            43 % of all cells are all singletons -- maxDist -1, empty windows --, where every addend is the same)
            steps of the greedy loop with tied rows of different alive matches: 18 542; with such rows more than 256 apart: 3622
            (Hd); with matches that differ from column 32 on only: 11 521; taking the last tied row instead of the first changes
            H1, H12 or H2 in 52 cells
            H2 != 0 and H12 != H1 in 2238 cells; all singletons 1029; one cluster 129
  indHet    357 diploid cells: bit 1 of the jointly called count set in 151, clear in 206; the minSites mask removes 125 of the 151
            values (sub-batch windows: 5105 / 15 295, the mask removes 1254)
  paint C   the left-to-right mean of the 1024- and 1000-value lists differs from np.nanmean in 1014 of 1047 cells without a nan"""
import numpy as np
import pytest

import finisher_cases as FC
import paint_model


def bits(v):
    return int(np.float64(v).view(np.uint64))


def left_to_right(values):
    s = 0.0
    for x in values:
        s += x
    return s


@pytest.fixture(scope="module")
def hap_survey():
    """every (case, state, maxDist, window, population) cell: the oracle's H values, the cluster sizes of the traced loop (which must
    give the oracle's values to the last bit), its tie steps, and whether the last-row rule would have given other values"""
    cells = []
    for name in FC.HAP_CASES:
        c = FC.hap_case(name)
        counts = FC.hap_counts(name)
        for state in FC.HAP_STATES:
            dms = [FC.cached_dist(aln, D, C, state) for aln, D, C in counts]
            for md in FC.HAP_MAX_DISTS:
                exp = FC.hap_expect(name, state, md)
                for w, (aln, _, _) in enumerate(counts):
                    g = np.array(aln.groups, dtype=object)
                    for p in c["lay"].sampleData.popNames:
                        idx = np.where(g == p)[0]
                        with np.errstate(invalid="ignore"):
                            match = dms[w][np.ix_(idx, idx)] <= md
                        sizes, ties = FC.greedy_trace(match)
                        want = (exp[w]["H1_" + p], exp[w]["H12_" + p], exp[w]["H2_" + p])
                        got = FC.h_of_sizes(sizes)
                        assert all(bits(a) == bits(b) for a, b in zip(got, want)), (name, state, md, w, p)
                        other = False
                        if ties:
                            other = any(bits(a) != bits(b) for a, b in zip(FC.h_of_sizes(FC.greedy_trace(match, "last")[0]), want))
                        cells.append(dict(case=name, n=len(idx), sizes=sizes, ties=ties, H=want, last_rule_differs=other))
    return cells


def test_hapstats_cases_reach_every_class_of_cluster_counts(hap_survey):
    classes = {"<8": 0, "8..128": 0, "129..256": 0, "257..512": 0, ">512": 0}
    for cell in hap_survey:
        k = len(cell["sizes"])
        classes["<8" if k < 8 else "8..128" if k <= 128 else "129..256" if k <= 256 else "257..512" if k <= 512 else ">512"] += 1
    print(len(hap_survey), "cells; clusters per cell:", classes)
    assert all(v > 0 for v in classes.values()), classes
    # populations on both sides of every mask word and of the 256 threads
    assert {1, 2, 31, 32, 33, 64, 65, 255, 256, 257, 513, 600, 128, 130, 34} <= {cell["n"] for cell in hap_survey}


def test_hapstats_sums_show_the_order_of_their_additions(hap_survey):
    differ = counted = 0
    for cell in hap_survey:
        if len(cell["sizes"]) >= 16:
            f = np.array(cell["sizes"]) / sum(cell["sizes"])
            counted += 1
            differ += bits(left_to_right((f ** 2).tolist())) != bits(cell["H"][0])
    print("left-to-right sum of f^2 differs from H1 in %d of %d cells with 16 clusters or more" % (differ, counted))
    assert counted >= 1000 and 2 * differ >= counted, (differ, counted)


def test_hapstats_ties_are_decided_by_the_first_row_rule(hap_survey):
    steps = sum(len(cell["ties"]) for cell in hap_survey)
    far = sum(1 for cell in hap_survey for d, _ in cell["ties"] if d > 256)
    later_word = sum(1 for cell in hap_survey for _, b in cell["ties"] if b)
    decided = sum(cell["last_rule_differs"] for cell in hap_survey)
    print("tie steps with different matches: %d; rows more than 256 apart: %d; differing from column 32 on only: %d; "
          "cells another rule changes: %d" % (steps, far, later_word, decided))
    assert steps > 0 and far > 0 and later_word > 0
    # ... and the rule shows in the printed values: taking the last tied row gives another H1, H12 or H2, also in the layout whose
    # tied rows lie in different trips of the row loop
    assert decided >= 10 and any(cell["last_rule_differs"] for cell in hap_survey if cell["case"] == "Hd")


def test_hapstats_cells_are_mostly_neither_all_singletons_nor_one_cluster(hap_survey):
    n = len(hap_survey)
    informative = sum(1 for cell in hap_survey if cell["H"][2] != 0 and cell["H"][1] != cell["H"][0])
    singletons = sum(1 for cell in hap_survey if len(cell["sizes"]) > 1 and max(cell["sizes"]) == 1)
    one = sum(1 for cell in hap_survey if len(cell["sizes"]) == 1)
    print("%d cells: H2 != 0 and H12 != H1 in %d, all singletons %d, one cluster %d" % (n, informative, singletons, one))
    assert 4 * informative >= 3 * n and 0 < singletons < n // 2 and 0 < one < n // 2


def test_hapstats_windows_and_layouts_are_the_ones_the_device_tests_need():
    for name in ("Hs", "Hd", "Dd"):
        assert {0, 1, 40, 300, 1200} <= {w[0] for w in FC.hap_case(name)["wins"]}
    hs = FC.hap_case("Hs")
    # the empty and the one-site window are not in the first batch of four windows that 64 MiB of scratch allow (8 MB of matrices each)
    assert min(k for k, w in enumerate(hs["wins"]) if w[0] == 1) >= 4 and 8 * hs["lay"].n_hap ** 2 * len(hs["wins"]) > 3 * (32 << 20)
    assert FC.hap_case("Hd")["lay"].n_hap > 1024
    # DdN: the same rows as Dd but for genotypes with one haplotype called; Dd itself has none
    dd, ddn = FC.hap_case("Dd"), FC.hap_case("DdN")
    pairs = np.array([dd["lay"].ind_slots[nm] for nm in dd["lay"].ind_order])
    half = lambda gt: int(((gt[:, pairs[:, 0]] != 0) != (gt[:, pairs[:, 1]] != 0)).sum())      # noqa: E731
    assert half(dd["gt"]) == 0 and half(ddn["gt"]) > 100 and (dd["gt"] == 0).any()
    # X4: nearly every site of the long windows carries four alleles
    x4 = FC.hap_case("X4")
    four = [(np.bitwise_or.reduce(x4["gt"][a:b].astype(np.uint8), axis=1) == 15).mean() for a, b in zip(x4["lo"], x4["hi"]) if b - a >= 500]
    assert len(four) == 3 and min(four) > 0.9, four


def test_indhet_case_has_the_bit_set_and_clear_and_a_mask_that_removes_some_cells():
    c = FC.het_case()
    lay = c["lay"]
    assert sorted(set(len(lay.ind_slots[nm]) for nm in lay.ind_order)) == [1, 2, 3, 4] and lay.n_samp == 90 and len(c["lo"]) == 7
    assert lay.n_samp * len(c["lo"]) > 512                                     # a third block of 256 threads
    for sub in (False, True):
        plain, masked = FC.het_expect(sub, False), FC.het_expect(sub, True)
        bit = clear = removed = kept = 0
        for (hp, called), (hm, _) in zip(plain, masked):
            for s in lay.ind_order:
                v, m = hp["het_" + s], hm["het_" + s]
                if s not in called:
                    assert np.isnan(v) and np.isnan(m)                          # (ploidy 1, 3, 4: no value)
                    continue
                bit += bool(called[s] & 2)
                clear += not called[s] & 2
                assert np.isnan(v) == (not called[s] & 2)
                removed += bool(not np.isnan(v) and np.isnan(m))
                kept += bool(not np.isnan(m))
        print("sub-batch windows" if sub else "the 7 windows", "bit set", bit, "clear", clear, "removed by the mask", removed, "kept", kept)
        assert bit > 20 and clear > 20 and removed > 20 and kept > 20
    assert len(c["sub_lo"]) * 4 * lay.n_hap ** 2 > 2 * (32 << 20)               # the D matrices alone exceed two batches
    assert {0, 1} <= set((c["sub_hi"] - c["sub_lo"])[160:320].tolist())         # empty and one-site windows behind the first batch


@pytest.mark.parametrize("name", ["C", "D", "S", "F"])
def test_paint_cases_contain_what_they_are_built_for(name):
    p = FC.PAINT_SHAPES[name]
    _, _, lo, hi, ref_lists, D, C = FC.paint_case(name)
    tested, _, info = FC.paint_expect(name, 0.05, None, 7)
    assert info["tied_values"] > 0 and info["nan_pairs"] > 0 and info["partly_nan_lists"] > 0 and info["nan_mean_cells"] > 0, info
    out, nan_mean, _ = FC.paint_expect(name, 0.05, 0.05, 7)
    assert 0 < nan_mean.sum() < nan_mean.size and info["nan_mean_cells"] == nan_mean.sum()
    decisions = set(out.ravel().tolist()) | set(tested.ravel().tolist())
    assert len(decisions) >= 4 and 7 in decisions, decisions
    if name == "C":
        assert [len(r) for r in ref_lists] == [1024, 1000, 24] and len(set(ref_lists[0])) < 1024 and D.shape[1] == 260
        differ = counted = 0
        for w in range(len(D)):
            d = paint_model.pair_dist(D[w], C[w], p["min_sites"])
            for i in range(len(d)):
                for r in ref_lists[:2]:
                    a = d[i, np.asarray(r)]
                    if not np.isnan(a).any():
                        counted += 1
                        differ += bits(left_to_right(a.tolist()) / len(a)) != bits(np.nanmean(a))
        print("left-to-right mean differs from np.nanmean in %d of %d cells without a nan" % (differ, counted))
        assert counted >= 500 and 2 * differ >= counted
    if name == "D":
        assert len(ref_lists) == 64 and sorted(set(len(r) for r in ref_lists)) == [1, 2, 3] and D.shape[1] == 130
    if name == "S":
        # flagged cells from batches behind the first: nan-mean cells in the first and in the last tenth of the windows, and matrices
        # (D and C of 600 individuals) of more than twice the 32 MiB a batch may take
        tenth = max(1, len(lo) // 10)
        assert nan_mean[:tenth].any() and nan_mean[-tenth:].any() and len(lo) >= 20
        assert len(lo) * 8 * 600 * 600 > 2 * (32 << 20) and {0, 1} <= set((hi - lo)[11:].tolist())
    if name == "F":
        lay, gt, _, _, _, _, _ = FC.paint_case(name)
        four = [(np.bitwise_or.reduce(gt[a:b].astype(np.uint8), axis=1) == 15).mean() for a, b in zip(lo, hi) if b - a >= 500]
        assert len(four) == 2 and min(four) > 0.9, four
