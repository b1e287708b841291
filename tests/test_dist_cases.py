"""The cases of tests/dist_cases.py contain what they are built for -- shown from the oracle, NumPy and the layouts alone, without a
GPU and without the library's results (pg_np_tree, the host's layout of a summation tree, is the one call into it).  These are
conditions on the cases, not on the code: tests/test_gpu_dist_finishers.py runs the device over the same cases."""
import ctypes as C

import numpy as np
import pytest

import dist_cases as DC
from oracle import popgen_oracle as orc

F_CASES = ["F1", "F2h", "F0", "M", "M1"]
N_CASES = ["N361", "N362", "N363"]


def half_called(c):
    """per window: genotypes of a diploid layout with exactly one haplotype called"""
    gt = c["gt"]
    return [int(((gt[a:b, 0::2] != 0) != (gt[a:b, 1::2] != 0)).sum()) for a, b in zip(c["lo"], c["hi"])]


def test_the_form_of_the_fixed_tree_finisher_follows_from_the_layout():
    f1, f2h, f0 = DC.case("F1"), DC.case("F2h"), DC.case("F0")
    assert DC.form_of(f1["lay"]) == 1 and DC.form_of(f1["lay"], no_dip=True) == 2
    assert half_called(f1) == [0] * 5                                   # nothing withdraws the called counts per individual
    assert half_called(f2h) == [1, 0, 1, 1, 1] and DC.form_of(f2h["lay"], half_called=True) == 2
    assert np.array_equal(f1["gt"] != f2h["gt"], (f1["gt"] != 0) & (f2h["gt"] == 0)) and (f1["gt"] != f2h["gt"]).sum() == 4
    assert DC.form_of(f0["lay"]) == 0
    ploidy = sorted({len(s) for s in f0["lay"].ind_slots.values()})
    assert ploidy == [1, 2, 3]
    assert DC.form_of(DC.case("M")["lay"]) == 1 and DC.form_of(DC.case("M1")["lay"]) == 1
    for name in N_CASES:
        assert DC.form_of(DC.case(name)["lay"]) == 0                    # (a haploid sample gives the odd count)
    assert DC.form_of(DC.S_case()["lay"]) == 1
    assert DC.form_of(DC.P_case()["lay"]) == 0 and DC.form_of(DC.G_case()["lay"]) == 0


def test_rectangles_lie_on_both_sides_of_every_stride():
    lay = DC.case("F1")["lay"]
    assert [n // 2 for n in lay.pop_sizes] == [1, 2, 16, 17, 23, 257] and lay.n_samp == 319
    rect = DC.rectangles(lay, 1)
    sizes = set(rect.values())
    assert {1, 2, 256, 272, 391, 529, 257 * 257} <= sizes and {257 * k for k in (1, 2, 16, 17, 23)} <= sizes
    tri = {rect[(x, x)] for x in range(lay.n_pops)}
    assert {256, 289, 529} <= tri                                       # 16 x 16 = one pair a thread, 17 x 17 a second one, 23 x 23 a second trip
    for stride in (256, 512):
        assert any(v < stride for v in sizes) and any(v > stride for v in sizes) and any(v < stride for v in tri) and any(v > stride for v in tri)
    assert 256 in sizes and 514 in sizes
    # 257 individuals are the columns of five rectangles: 256 / 257 = 0 rows a stride; 16, 17 and 23 give 16, 15 and 11
    cols = {lay.pop_sizes[y] // 2 for (x, y) in rect if x < y}
    assert cols == {2, 16, 17, 23, 257}

    lay = DC.case("F0")["lay"]
    assert lay.pop_sizes == [1, 3, 31, 32, 33, 255, 256, 257]
    rect = DC.rectangles(lay, 0)
    assert rect[(2, 4)] == 1023 and rect[(3, 3)] == 1024 and rect[(3, 4)] == 1056
    sizes = set(rect.values())
    for stride in (256, 512, 1024):
        assert any(v < stride for v in sizes) and any(v > stride for v in sizes)
    cols = {lay.pop_sizes[y] for (x, y) in rect if x < y}
    assert {255, 256, 257} <= cols and min(cols) < 256
    lone = [nm for nm in lay.ind_order if lay.hap_group[lay.ind_slots[nm][0]] == "p0"]
    assert len(lone) == 1 and len(lay.ind_slots[lone[0]]) == 1           # one population is a single haploid

    lay = DC.case("M")["lay"]
    assert lay.n_pops == 12 and set(n // 2 for n in lay.pop_sizes) == {1, 2, 3, 4, 5}
    assert sorted(lay.sampleData.popNames) != list(lay.sampleData.popNames)
    assert DC.case("M1")["lay"].n_pops == 1


def test_361_haplotypes_fill_the_numpy_order_tree_and_362_do_not():
    from genomics_general_amd import _lib
    L = _lib.lib()

    def runs_of_the_host(n):
        blob = np.zeros(4 * n // 64 + 64, dtype=np.int32)
        ln = C.c_int64(0)
        _lib.check(L.pg_np_tree(n, blob, len(blob), C.byref(ln)))
        return int(blob[0])
    assert DC.np_runs(361 * 361) == 1024 == runs_of_the_host(361 * 361)
    assert DC.np_runs(362 * 362) == 1025 == runs_of_the_host(362 * 362) and 362 * 362 <= 131072
    assert 363 * 363 > 131072
    assert DC.np_runs(347 * 347) == 960
    for n in (1, 7, 8, 128, 129, 8192, 8193, 21316):
        assert DC.np_runs(n) == runs_of_the_host(n), n
    for name, sizes in (("N361", [180, 181]), ("N362", [181, 181]), ("N363", [181, 182])):
        c = DC.case(name)
        assert c["lay"].pop_sizes == sizes and c["wins"] == [37, 200]
        assert list(c["lay"].ref_order) != list(range(c["lay"].n_hap))


@pytest.mark.parametrize("name", F_CASES + N_CASES + ["P"])
def test_min_sites_is_a_called_count_of_the_case_and_so_is_the_count_below(name):
    thr = DC.min_sites_of(name)
    w = 0 if name.startswith("N") else 1 if name == "P" else DC.WIN_SHORT
    aln, _, Cm = DC.counts(name)[w]
    in_pop = np.array([g != DC.NONE for g in aln.groups])
    c = Cm[np.ix_(in_pop, in_pop)][np.triu_indices(int(in_pop.sum()), 1)]
    assert (c == thr).sum() >= 1 and (c == thr - 1).sum() >= 1 and thr > 1
    assert 0.02 < (c < thr).mean() < 0.4                                # the mask removes some pairs of the short window, not most


@pytest.mark.parametrize("name", F_CASES)
def test_the_missing_individual_leaves_exactly_the_share_the_formula_gives(name):
    c = DC.case(name)
    lay, k = c["lay"], c["hole_k"]
    names = lay.sampleData.popNames
    n = lay.pop_sizes[c["hole_pop"]]
    assert 1 <= k and n - k >= 2
    shares = DC.hole_shares(name)
    for key, (nv, size, share) in shares.items():
        if key.startswith("pi_"):
            assert (nv, size) == ((n - k) * (n - k - 1), n * n)
        else:
            other = [p for p in key.split("_")[1:] if p != names[c["hole_pop"]]][0]
            m = lay.pop_sizes[names.index(other)]
            assert (nv, size) == (((n - k) * m, n * m) if key.startswith("dxy_") else ((n + m - k) * (n + m - k - 1), (n + m) ** 2))
        assert 0 < share < 1
        at, _ = DC.expect(name, DC.WIN_HOLE, 1, share)
        above, _ = DC.expect(name, DC.WIN_HOLE, 1, float(np.nextafter(share, 1)))
        if key.startswith("Fst_"):
            # pi_t's share is the largest of the three: where it decides, pi of the population is nan already and Fst with it.  The
            # pass at this minData still puts `1 - (1.*n_nan/size) >= minData` of the pi_t block to the test at equality
            assert share > shares["pi_" + names[c["hole_pop"]]][2] and np.isnan(at[key]) and np.isnan(above[key])
            assert np.isfinite(DC.expect(name, DC.WIN_HOLE, 1)[0][key])
        else:
            assert np.isfinite(at[key]) and np.isnan(above[key]), (key, share, at[key], above[key])
    assert len(shares) == (3 if lay.n_pops > 1 else 1)


def cells(name):
    """(compared cells, nan among them, nan by construction) of a case's two passes: minSites 1 and the case's own"""
    c = DC.case(name)
    lay = c["lay"]
    total = nan = built = 0
    for ms in (1, DC.min_sites_of(name)):
        for w, L in enumerate(c["wins"]):
            out, _ = DC.expect(name, w, ms)
            for key, kind, pops in DC.stat_keys(lay):
                lone = any(lay.pop_sizes[lay.sampleData.popNames.index(p)] == 1 for p in pops) and kind != "dxy"
                total += 1
                nan += bool(np.isnan(out[key]))
                built += bool(np.isnan(out[key]) and (L == 0 or lone))
    return total, nan, built


@pytest.mark.parametrize("name", F_CASES + N_CASES)
def test_at_most_a_quarter_of_the_compared_cells_is_nan(name):
    total, nan, built = cells(name)
    print(name, "cells", total, "nan", nan, "by construction", built)
    assert total - built > 0 and (nan - built) <= 0.25 * (total - built), (name, total, nan, built)
    if name == "F0":
        assert built > total // 5                                        # pi of the lone haploid and its Fst, in every window


def test_at_most_a_quarter_of_the_cells_of_p_g_and_s_is_nan():
    """the cap for the cases of the individual-pair table, nothing counted as nan by construction.  P: the four passes the device test
    compares (plain and masked, with and without includeSameWithSame), 3 windows x 1711 pairs each: 3653 of 20 532 cells.  Under
    the mask the one-site window is nan in every cell (no pair shares minSites sites of one), a third of a masked pass: the cap holds
    for the case, and for the windows of 40 and 300 sites of every pass alone.  G: every cell of the tables from the supplied
    counts and from the window of real rows.  S: the six windows compared with the oracle, both tables"""
    total = nan = 0
    for masked in (False, True):
        for include_same in (False, True):
            want = DC.P_expect(masked, include_same)
            names = DC.P_case()["lay"].ind_order
            per_window = [np.array([w[a][b] for a in names for b in names if a <= b]) for w in want]
            assert all(len(v) == 1711 for v in per_window)
            total += sum(len(v) for v in per_window)
            nan += sum(int(np.isnan(v).sum()) for v in per_window)
            longer = np.concatenate(per_window[1:])
            assert 4 * np.isnan(longer).sum() <= len(longer), (masked, include_same)
            if masked:
                assert np.isnan(per_window[0]).all()
    print("P cells", total, "nan", nan)
    assert total == 4 * 3 * 1711 and 4 * nan <= total, (total, nan)

    g = DC.G_case()
    total = nan = 0
    D, Cm = DC.slot_counts(g["gt"])
    for include_same in (False, True):
        tabs = [DC.pair_table_np(g["D"][w], g["C"][w], g["lay"], DC.G_MIN_SITES, include_same) for w in range(2)]
        tabs += [DC.pair_table_np(D, Cm, g["lay"], ms, include_same) for ms in (None, DC.G_ROW_MIN_SITES)]
        for t in tabs:
            assert 4 * np.isnan(t).sum() <= len(t), (include_same, int(np.isnan(t).sum()), len(t))
            total, nan = total + len(t), nan + int(np.isnan(t).sum())
    print("G cells", total, "nan", nan)
    hap = Cm[np.triu_indices(len(Cm), 1)]
    assert (hap == DC.G_ROW_MIN_SITES).any() and (hap == DC.G_ROW_MIN_SITES - 1).any()

    c = DC.S_case()
    total = nan = 0
    for w in DC.S_CHECKED:
        out, _, D, Cm = DC.S_expect(w)
        vals = np.array([out[key] for key, _, _ in DC.stat_keys(c["lay"])] + DC.pair_table_np(D, Cm, c["lay"], DC.S_MIN_SITES, False).tolist())
        total, nan = total + len(vals), nan + int(np.isnan(vals).sum())
    print("S cells", total, "nan", nan)
    assert total == 6 * (16 + 20100) and 4 * nan <= total, (total, nan)


@pytest.mark.parametrize("name", ["F1", "F0", "N362"])
def test_numpy_s_own_order_lies_within_the_bound_derived_for_any_fixed_order(name):
    """the oracle's values (np.nanmean: one of the fixed orders) against the exact sums: the bound's own code is checked here"""
    c = DC.case(name)
    worst = 0.0
    for w, L in enumerate(c["wins"]):
        out, sums = DC.expect(name, w, DC.min_sites_of(name))
        for key, kind, pops in DC.stat_keys(c["lay"]):
            if not np.isfinite(out[key]):
                continue
            ref, bound = DC.fixed_tree_bound(kind, pops, sums)
            assert abs(out[key] - ref) <= bound, (name, w, key, out[key], ref, bound)
            if bound > 0:
                worst = max(worst, abs(out[key] - ref) / bound)
    print(name, "largest share of the bound:", worst)
    assert worst < 1


def test_with_sums_leaves_the_default_return_value_as_it_was():
    aln, D, Cm = DC.counts("M")[0]
    plain = orc.group_dist_stats(aln, D, Cm, True, 5, 0.01)
    more = orc.group_dist_stats(aln, D, Cm, True, 5, 0.01, with_sums=True)
    assert len(plain) == 2 and len(more) == 3 and plain[0].keys() == more[0].keys()
    assert all(np.array_equal(plain[0][k], more[0][k], equal_nan=True) for k in plain[0])
    assert np.array_equal(plain[1], more[1], equal_nan=True)
    nv, size, fs = more[2]["pi_p0"]
    blk = plain[1][np.ix_(np.array(aln.groups) == "p0", np.array(aln.groups) == "p0")]
    assert size == blk.size == 36 and nv == (~np.isnan(blk)).sum() and abs(fs / nv - np.nanmean(blk)) < 1e-15
    assert set(more[2]) >= {"pi_p0", "dxy_p0_p1", "pit_p0_p1", "dxy_p10_p2"} and "dxy_p2_p10" not in more[2]
    one = orc.group_dist_stats(*DC.counts("M1")[0], True, 5, 0.01, with_sums=True)
    assert set(one[2]) == {"pi_p0", "pi_" + DC.NONE, "dxy_p0_" + DC.NONE, "pit_p0_" + DC.NONE}       # (the individual in no population)


def left_to_right(blk):
    tot, n = 0.0, 0
    for v in blk.ravel().tolist():
        if v == v:
            tot, n = tot + v, n + 1
    return tot / n if n else np.nan


def test_p_holds_blocks_whose_mean_depends_on_the_order_of_the_sum():
    """shares found with these seeds: 1835 of the 4464 cells (0.41) between individuals whose block has 8 values and more, added left to
    right, and 27 of the 80 cells (0.34) within an individual of three haplotypes and more, as twice the triangle's sum, differ from
    np.nanmean of the block (both orientations, windows of 40 and 300 sites; the one-site window is left out)"""
    c = DC.P_case()
    lay = c["lay"]
    ploidy = sorted({len(s) for s in lay.ind_slots.values()})
    assert ploidy == [1, 2, 3, 4, 6] and lay.n_samp == 58 and lay.n_pops == 2
    names = lay.ind_order
    up = [names[s] < names[t] for s in range(len(names)) for t in range(s + 1, len(names))]
    assert 0.2 < np.mean(up) < 0.8                                       # both orientations of samp_rank among the pairs in slot order
    big = big_diff = own = own_diff = 0
    for w in (1, 2):
        aln, D, Cm = DC.counts("P")[w]
        dm = orc.dist_from_counts(D, Cm)
        np.fill_diagonal(dm, np.nan)
        rows = {}
        for r, s in enumerate(aln.sample_names):
            rows.setdefault(s, []).append(r)
        want = DC.P_expect(False, False)[w]
        for a in rows:
            for b in rows:
                blk = dm[np.ix_(rows[a], rows[b])]
                if a == b and len(rows[a]) >= 3:
                    tri = blk[np.triu_indices(len(rows[a]), 1)]
                    ok = ~np.isnan(tri)
                    tot = 0.0
                    for v in tri[ok].tolist():
                        tot += v
                    own += 1
                    own_diff += bool(ok.any() and (2 * tot) / (2 * int(ok.sum())) != want[a][b])
                elif a != b and blk.size >= 8 and np.isfinite(want[a][b]):
                    big += 1
                    big_diff += left_to_right(blk) != want[a][b]
    print("blocks of 8 values and more:", big, "differ:", big_diff, "; within an individual:", own, "differ:", own_diff)
    assert big >= 1000 and big_diff >= 0.1 * big
    assert own >= 40 and own_diff >= 0.1 * own


def test_g_has_pairs_of_the_second_trip_with_counts_at_the_threshold():
    g = DC.G_case()
    lay, D, Cm = g["lay"], g["D"], g["C"]
    n = lay.n_samp
    assert n == 1030 and n * (n + 1) // 2 > DC.G_FIRST_LATE and 1000 * 1001 // 2 < DC.G_FIRST_LATE
    assert sorted({len(s) for s in lay.ind_slots.values()}) == [1, 2]
    assert np.array_equal(D, D.transpose(0, 2, 1)) and np.array_equal(Cm, Cm.transpose(0, 2, 1)) and (D <= Cm).all() and (D >= 0).all()
    s, t = np.triu_indices(n)
    assert all(lay.sample_pair_index(int(s[k]), int(t[k])) == k for k in (0, 1, n - 1, n, 2 * n - 1, len(s) - 1, DC.G_FIRST_LATE))
    late = np.arange(len(s)) >= DC.G_FIRST_LATE
    for win in range(2):
        tab = DC.pair_table_np(D[win], Cm[win], lay, DC.G_MIN_SITES, False)
        assert np.isfinite(tab[late]).sum() >= 1000
        hap_s = np.array([lay.ind_slots[nm][0] for nm in lay.ind_order])
        seen = set()
        for k in np.flatnonzero(late):
            if s[k] != t[k]:
                seen.add(int(Cm[win, hap_s[s[k]], hap_s[t[k]]]))
        assert {0, DC.G_MIN_SITES, DC.G_MIN_SITES - 1} <= seen


@pytest.mark.parametrize("include_same", [False, True])
def test_the_numpy_form_of_small_blocks_equals_the_oracle_on_sampled_pairs(include_same):
    """pair_table_np against orc.ind_pair_dists on the 210 pairs of 20 of G's individuals, the last ones among them"""
    g = DC.G_case()
    lay = g["lay"]
    rng = np.random.default_rng(11)
    pick = np.sort(np.concatenate([rng.choice(1000, size=14, replace=False), np.arange(1024, 1030)]))
    for ms in (None, DC.G_MIN_SITES):
        tab = DC.pair_table_np(g["D"][0], g["C"][0], lay, ms, include_same)
        slots = [h for s in pick for h in lay.ind_slots[lay.ind_order[s]]]
        Dm, Cm = g["D"][0][np.ix_(slots, slots)].astype(np.int64), g["C"][0][np.ix_(slots, slots)].astype(np.int64)
        dm = orc.dist_from_counts(Dm, Cm)
        if ms:
            few = Cm < ms
            np.fill_diagonal(few, False)                  # (a minSites of indPairTable's own masks pairs, not the diagonal's zeros)
            dm[few] = np.nan
        aln = orc.Aln(np.zeros((len(slots), 0), dtype=np.int64), [lay.hap_names[h] for h in slots], [lay.hap_sample_name[h] for h in slots],
                      [None] * len(slots))
        want, _ = orc.ind_pair_dists(aln, dm, include_same)
        n_nan = 0
        for i, s in enumerate(pick):
            for t in pick[i:]:
                got, w = tab[lay.sample_pair_index(int(s), int(t))], want[lay.ind_order[s]][lay.ind_order[t]]
                assert (got == w) or (np.isnan(got) and np.isnan(w)), (s, t, got, w)
                n_nan += bool(np.isnan(w))
        assert 4 * n_nan <= 210, n_nan


def test_s_puts_both_sum_orders_into_every_batch():
    c = DC.S_case()
    lens = c["wins"]
    assert len(lens) == 100 and lens.count(0) == 1 and lens.count(1) == 1 and c["lay"].n_hap == 400 and c["lay"].n_pops == 4
    assert all(sorted(set(lens[k:k + 4])) [-1] == 300 and 64 in lens[k:k + 4] for k in range(0, 97))
    assert [lens[w] for w in DC.S_CHECKED] == [64, 300] * 3
    assert np.array_equal(c["lo"][1:], c["hi"][:-1])
