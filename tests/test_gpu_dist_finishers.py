"""-m gpu: the finishers behind pi / dxy / Fst -- k_popdist_fin<0|1|2> + k_popstats, k_popdist_np + k_popstats_np -- and behind the
individual-pair distances -- k_indpair_fin -- on the cases of tests/dist_cases.py: rectangles on both sides of every stride of the
fixed-tree finisher, twelve populations, minData and minSites at equality, the NumPy-order kernel at its last layout (361 haplotypes,
1024 runs) and the two layouts past it, individuals of three to six haplotypes, the second trip of k_indpair_fin's grid, a pass in
sub-batches that holds both sum orders.  tests/test_dist_cases.py shows without a GPU that the cases contain all this.  The
expectations are the oracle's and NumPy's alone.

Strictness: counts are integers and equal; sums in NumPy's order equal the oracle bit for bit (gpu_util.same: nan equals nan); sums
of the fixed trees lie within the bound derived in dist_cases.fixed_tree_bound from the exact sums (math.fsum) -- (n + 2) 2^-53 of a
sum of n quotients, (n + 4) 2^-53 of pi, dxy and pi_t, the propagated bound of Fst -- and their nan are the oracle's.

Largest share of each bound seen on the MI355X (set_sum_order(2), cases F1 / F2 / F2h / F0 / M / M1 / N362 / N363): sums 0.36 and pi 0.39
(F0), dxy 0.16 and Fst 0.081 (M) -- all in blocks of a handful of quotients, where the bound is a few units in the last place; the
blocks of 10^5 quotients (N362, N363) stay below 0.0002.  The 300-site windows of S: pi 0.0003, dxy 0.0002, Fst below 0.00005."""
import numpy as np
import pytest

import dist_cases as DC
import gpu_util as G
from genomics_general_amd import _lib

pytestmark = pytest.mark.gpu

ROWS_OF = {"F2": "F1"}                               # F2: F1's rows, and so F1's expectations, under PG_NO_DIP


def engine_of(c, order=None):
    e = G.Engine(0)
    e.set_layout(c["lay"])
    e.load_sites(c["gt"])
    if order is not None:
        e.set_sum_order(order)
    return e


def table_stats(wb, min_sites, min_data):
    """WindowBatch.groupDistTable as {column name: values over the windows}"""
    tab, cols = wb.groupDistTable(True, min_sites, min_data)
    assert tab.shape == (wb.n, len(cols)) and len(set(cols)) == len(cols)
    return {key: tab[:, k] for k, key in enumerate(cols)}


def same_arrays(a, b):
    """gpu_util.same for every element"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    nan = np.isnan(a)
    return bool(a.shape == b.shape and np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan], b[~nan])
                and np.array_equal(np.signbit(a[~nan]), np.signbit(b[~nan])))


def check_fixed(name, st, windows, min_sites, min_data, worst):
    """the statistics st of the case's windows against the exact sums: the oracle's nan, and values within the derived bounds"""
    lay = DC.case(name)["lay"]
    for k, w in enumerate(windows):
        out, sums = DC.expect(name, w, min_sites, min_data)
        for key, kind, pops in DC.stat_keys(lay):
            got, want = st[key][k], out[key]
            if not np.isfinite(want):
                assert G.same(got, want), (name, w, key, min_sites, min_data, got, want)
                continue
            ref, bound = DC.fixed_tree_bound(kind, pops, sums)
            err = abs(got - ref)
            assert np.isfinite(got) and err <= bound, (name, w, key, min_sites, min_data, got, ref, err, bound)
            if bound > 0:
                worst[kind] = max(worst.get(kind, 0.0), err / bound)


def check_sums(name, tot, cnt, min_sites, worst):
    """groupDistSums: every unordered pair once -- on a symmetric block half the oracle's cells and half their sum (exactly)"""
    c = DC.case(name)
    lay, names = c["lay"], c["lay"].sampleData.popNames
    for w in range(len(c["wins"])):
        _, sums = DC.expect(name, w, min_sites)
        for x in range(lay.n_pops):
            for y in range(x, lay.n_pops):
                nv, _, fs = sums["pi_" + names[x]] if x == y else sums[DC.pair_key("dxy", names[x], names[y])]
                n, exact = (nv // 2, fs / 2) if x == y else (nv, fs)
                k = lay.pop_pair_index(x, y)
                assert cnt[w, k] == n, (name, w, x, y, min_sites, cnt[w, k], n)
                err, bound = abs(tot[w, k] - exact), (n + 2) * DC.U * exact
                assert err <= bound, (name, w, x, y, min_sites, tot[w, k], exact, err, bound)
                if bound > 0:
                    worst["sum"] = max(worst.get("sum", 0.0), err / bound)


def hole_runs(name):
    """(minData, ...) of the window with the missing individual: every valid share of dist_cases.hole_shares and the next float above"""
    if "hole" not in DC.CASES[name]:
        return []
    return sorted({md for _, _, share in DC.hole_shares(name).values() for md in (share, float(np.nextafter(share, 1)))})


@pytest.mark.parametrize("name", ["F1", "F2", "F2h", "F0", "M", "M1", "N362", "N363"])
def test_fixed_trees_within_the_derived_bounds(name, monkeypatch):
    """set_sum_order(2): k_popdist_fin + k_popstats for every window, through groupDistSums and groupDistTable (the shares of the
    bounds seen: the module's docstring)"""
    rows = ROWS_OF.get(name, name)
    if name == "F2":
        G.set_mode(monkeypatch, "PG_NO_DIP")
    c = DC.case(rows)
    e = engine_of(c, 2)
    try:
        worst = {}
        everything = list(range(len(c["wins"])))
        for ms in (1, DC.min_sites_of(rows)):
            wb = e.batch(c["lo"], c["hi"])
            tot, cnt = wb.groupDistSums(ms)
            check_sums(rows, tot, cnt, ms, worst)
            check_fixed(rows, table_stats(wb, ms, DC.MIN_DATA), everything, ms, DC.MIN_DATA, worst)
        for md in hole_runs(rows):
            wb = e.batch(c["lo"][DC.WIN_HOLE:DC.WIN_HOLE + 1], c["hi"][DC.WIN_HOLE:DC.WIN_HOLE + 1])
            check_fixed(rows, table_stats(wb, 1, md), [DC.WIN_HOLE], 1, md, worst)
        print(name, "largest share of the bound:", {k: round(v, 4) for k, v in worst.items()})
    finally:
        e.close()


@pytest.mark.parametrize("name", ["N362", "N363"])
def test_layouts_past_the_numpy_order_tree_take_the_fixed_trees_by_themselves(name):
    """the default order: 362 haplotypes make 1025 runs, 363 more than 131 072 values: np_prepare leaves both layouts, short windows
    included, to the fixed trees"""
    c = DC.case(name)
    e = engine_of(c)
    try:
        worst = {}
        for ms in (1, DC.min_sites_of(name)):
            check_fixed(name, table_stats(e.batch(c["lo"], c["hi"]), ms, DC.MIN_DATA), [0, 1], ms, DC.MIN_DATA, worst)
        print(name, "largest share of the bound:", {k: round(v, 4) for k, v in worst.items()})
    finally:
        e.close()


def count_numpy_order(name, e):
    """(cells compared, cells that are not the oracle's bit for bit, the first few of them)"""
    c = DC.case(name)
    lay = c["lay"]
    cells, bad = 0, []
    runs = [(c["lo"], c["hi"], list(range(len(c["wins"]))), ms, DC.MIN_DATA) for ms in (1, DC.min_sites_of(name))]
    runs += [(c["lo"][DC.WIN_HOLE:DC.WIN_HOLE + 1], c["hi"][DC.WIN_HOLE:DC.WIN_HOLE + 1], [DC.WIN_HOLE], 1, md) for md in hole_runs(name)]
    for lo, hi, windows, ms, md in runs:
        st = table_stats(e.batch(lo, hi), ms, md)
        for k, w in enumerate(windows):
            out, _ = DC.expect(name, w, ms, md)
            for key, _, _ in DC.stat_keys(lay):
                cells += 1
                if not G.same(st[key][k], out[key]):
                    bad.append((w, key, ms, md, st[key][k], out[key]))
    return cells, bad


@pytest.mark.parametrize("name", ["F0", "F1", "M", "M1", "N361"])
def test_numpy_order_equals_the_oracle_bit_for_bit(name):
    """set_sum_order(1): NumPy's order for every window.  M, M1 and N361 take k_popdist_np + k_popstats_np; N361 is the launch with 1024
    runs, every slot of the tree's LDS in use.  F0 and F1 hold blocks of 513^2 = 263 169 and 514^2 = 264 196 values, more than the
    131 072 that kernel's LDS takes: k_popdist_np_big walks them a piece of 8192 values at a time.  Before that kernel existed the
    library left such a layout to the fixed trees under every sum order, and this comparison failed: 237 of the 1024 cells of F0 and
    175 of the 576 cells of F1 differed from the oracle in the last bits"""
    e = engine_of(DC.case(name), 1)
    try:
        cells, bad = count_numpy_order(name, e)
        print(name, "cells:", cells, "not bit for bit:", len(bad), bad[:5])
        assert not bad, (name, cells, len(bad), bad[:5])
    finally:
        e.close()


def test_361_haplotypes_take_numpy_order_by_themselves():
    """the default order, as the drivers run: windows of 37 and 200 sites (up to 256: NumPy's order) on the largest layout it takes"""
    e = engine_of(DC.case("N361"))
    try:
        cells, bad = count_numpy_order("N361", e)
        assert cells == 16 and not bad, (cells, bad[:5])
    finally:
        e.close()


@pytest.mark.parametrize("include_same", [False, True])
@pytest.mark.parametrize("masked", [False, True])
def test_individual_pair_means_of_polyploids_equal_the_oracle_bit_for_bit(masked, include_same):
    """case P: indPairDists (rows: the haplotypes of the individual whose name sorts first) and indPairTable(first="slot") (rows: the
    earlier individual in slot order) against orc.ind_pair_dists for every pair in the orientation named, on the plain matrix and
    after a groupDistStats that leaves its minSites mask.  Before k_indpair_fin added blocks of 8 values and more in NumPy's order
    (left to right then; twice the triangle's sum within an individual) this failed in all four cases: of the 5133 cells of a table
    934 (by name) and 940 (by slot) differed in the last bit on the plain matrix, 886 and 878 after the mask, with and without
    includeSameWithSame alike"""
    c = DC.P_case()
    lay = c["lay"]
    names, n = lay.ind_order, lay.n_samp
    e = engine_of(c)
    try:
        wb = e.batch(c["lo"], c["hi"])
        if masked:
            wb.groupDistStats(True, DC.min_sites_of("P"), DC.MIN_DATA)
        want = DC.P_expect(masked, include_same)
        got = wb.indPairDists(includeSameWithSame=include_same)
        by_name = [(w, a, b) for w in range(len(want)) for a in names for b in names if a <= b and not G.same(got[a][b][w], want[w][a][b])]
        tab = np.array(wb.indPairTable(includeSameWithSame=include_same, first="slot"))
        by_slot = [(w, s, t) for w in range(len(want)) for s in range(n) for t in range(s, n)
                   if not G.same(tab[w, lay.sample_pair_index(s, t)], want[w][names[s]][names[t]])]
        finite = sum(np.isfinite(want[w][a][b]) for w in range(len(want)) for a in names for b in names if a <= b)
        print("cells:", len(want) * n * (n + 1) // 2, "finite:", finite, "not bit for bit by name:", len(by_name), "by slot:", len(by_slot))
        assert finite > 3000
        assert not by_name and not by_slot, (len(by_name), by_name[:5], len(by_slot), by_slot[:5])
    finally:
        e.close()


@pytest.mark.parametrize("include_same", [False, True])
def test_the_second_trip_of_the_individual_pair_grid(include_same):
    """case G, 530 965 pairs for 2048 x 256 threads: every cell of indPairTableFromCounts on supplied counts (cells with C = 0, minSites
    and minSites - 1 among the pairs of the second trip) and of indPairTable on a window of real rows against the NumPy form of blocks
    of at most four values; the table from the window's counts equals the table from its rows"""
    g = DC.G_case()
    lay = g["lay"]
    e = G.Engine(0)
    try:
        e.set_layout(lay)
        e.load_sites(g["gt"])
        got = e.indPairTableFromCounts(g["D"], g["C"], include_same, DC.G_MIN_SITES)
        for win in range(2):
            want = DC.pair_table_np(g["D"][win], g["C"][win], lay, DC.G_MIN_SITES, include_same)
            assert np.isfinite(want[DC.G_FIRST_LATE:]).sum() >= 1000 and same_arrays(got[win], want), (win, int((got[win] != want).sum()))
        D, Cm = DC.slot_counts(g["gt"])
        for ms in (None, DC.G_ROW_MIN_SITES):
            rows = np.array(e.batch([0], [40]).indPairTable(include_same, ms, first="slot"))
            want = DC.pair_table_np(D, Cm, lay, ms, include_same)
            assert same_arrays(rows[0], want), (ms, int((rows[0] != want).sum()))
            Dd, Cd = e.batch([0], [40]).pairCounts(reference_order=False)
            assert same_arrays(e.indPairTableFromCounts(Dd, Cd, include_same, ms)[0], rows[0]), ms
    finally:
        e.close()


def test_tables_of_a_pass_in_sub_batches_hold_both_sum_orders_at_their_rows():
    """case S under 64 MiB of scratch: pg_popdist_stats' consume(w0, nb) writes its three tables at w0 and launches both orders in every
    batch; the individual-pair table is copied back batch by batch.  Both tables of the whole pass equal the windows computed one at a
    time; six windows of the first, a middle and the last batch equal the oracle (64 sites: bit for bit; 300 sites: the derived
    bounds); the pack family's launch count shows that the passes were cut"""
    c = DC.S_case()
    lay = c["lay"]
    e = engine_of(c)
    try:
        e.set_scratch_limit(64 << 20)
        e.kernel_time_select(None)
        e.kernel_time_reset()
        tab, cols = e.batch(c["lo"], c["hi"]).groupDistTable(True, DC.S_MIN_SITES, DC.MIN_DATA)
        launches = [e.kernel_time(_lib.K_PACK)[1]]
        e.kernel_time_reset()
        pairs = np.array(e.batch(c["lo"], c["hi"]).indPairTable(False, DC.S_MIN_SITES))
        launches.append(e.kernel_time(_lib.K_PACK)[1])
        print("pack launches:", launches)
        assert min(launches) >= 3, launches
        for w in range(len(c["wins"])):
            lo, hi = c["lo"][w:w + 1], c["hi"][w:w + 1]
            assert same_arrays(e.batch(lo, hi).groupDistTable(True, DC.S_MIN_SITES, DC.MIN_DATA)[0][0], tab[w]), w
            assert same_arrays(e.batch(lo, hi).indPairTable(False, DC.S_MIN_SITES)[0], pairs[w]), w
        worst = {}
        for w in DC.S_CHECKED:
            out, sums, D, Cm = DC.S_expect(w)
            for key, kind, pops in DC.stat_keys(lay):
                got = tab[w, cols.index(key)]
                if c["wins"][w] <= 256 or not np.isfinite(out[key]):
                    assert G.same(got, out[key]), (w, key, got, out[key])
                else:
                    ref, bound = DC.fixed_tree_bound(kind, pops, sums)
                    assert abs(got - ref) <= bound, (w, key, got, ref, bound)
                    worst[kind] = max(worst.get(kind, 0.0), abs(got - ref) / bound)
            assert same_arrays(pairs[w], DC.pair_table_np(D, Cm, lay, DC.S_MIN_SITES, False)), w
        print("largest share of the bound:", {k: round(v, 4) for k, v in worst.items()})
        assert np.isnan(tab[31]).all() and np.isnan(pairs[31]).all()                 # the empty window
    finally:
        e.close()


def test_a_driver_recomputes_long_windows_of_a_large_layout_in_numpy_order(tmp_path, monkeypatch, capfd):
    """popgenWindows.py on two populations of 190 diploids (760 haplotypes in the x + y block: k_popdist_np_big's layout), windows of
    500 sites, --roundTo 12: every value is within reach of a rounding tie of the twelfth digit, so cli._refine_long_windows computes
    every window again under set_sum_order(1), and the text must be the oracle's command line's, cell for cell"""
    import json
    import oracle_cli
    import test_gpu_golden as GG
    from genomics_general_amd import synth
    n_dip, L = 380, 1500
    names = ["s%d" % d for d in range(n_dip)]
    path = str(tmp_path / "large.geno")
    codes = synth.gen_codes(777, np.zeros(L, dtype=np.int64), np.arange(1, L + 1), n_dip, 2, var_thr=20000, miss_thr=3000)
    synth.write_geno_fast(path, codes, names, "scaf1", 1)
    argv = ["-g", path, "-f", "phased", "-w", "500", "-m", "40", "--roundTo", "12", "--analysis", "popDist", "popPairDist",
            "-p", "b", ",".join(names[:190]), "-p", "a", ",".join(names[190:])]
    want = oracle_cli.run("popgenWindows.py", argv)
    monkeypatch.setenv("PG_TIMING", "1")
    out = str(tmp_path / "out.csv")
    GG.MAINS["popgenWindows.py"](argv + ["-o", out])
    with open(out) as f:
        got = f.read()
    assert len(want.splitlines()) == 4 and got == want
    timing = [ln for ln in capfd.readouterr().err.splitlines() if ln.startswith("PG_TIMING ")]
    assert json.loads(timing[-1][len("PG_TIMING "):]).get("windows_recomputed_in_numpy_order", 0) == 3
