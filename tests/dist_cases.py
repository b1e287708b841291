"""Seeded cases for the finishers behind pi / dxy / Fst and the individual-pair distances -- k_popdist_fin<0|1|2> + k_popstats,
k_popdist_np + k_popstats_np, k_indpair_fin -- at the sizes where their loops turn over.  Builders only: layouts, rows, windows and
what the oracle (oracle/popgen_oracle.py) and NumPy make of them; no engine.  tests/test_dist_cases.py shows without a GPU that the
cases contain what they are built for; tests/test_gpu_dist_finishers.py runs the device over them.

F1    all diploid, populations of 1, 2, 16, 17, 23 and 257 individuals and 3 individuals in none: k_popdist_fin<1> takes individual
      pairs, 256 threads two per trip: rectangles of 1 .. 256 (16 x 16), 272, 391, 529 (23 x 23), 257 k and 257 x 257 pairs, the
      triangles x = y on both sides of 256 and 512; 257 is a column population (256 / 257 = 0 rows per stride)
F2    F1's rows under PG_NO_DIP; F2h: the same rows with one half-called genotype (`A|N`) in every window, after which the library
      takes the called counts per haplotype by itself: k_popdist_fin<2>
F0    ploidy 1, 2 and 3 mixed, populations of 1, 3, 31, 32, 33, 255, 256 and 257 haplotypes: k_popdist_fin<0> takes haplotype pairs four
      per trip: 31 x 33 = 1023, 32 x 32 = 1024, 32 x 33 = 1056, column populations on both sides of 256, one population of a single haploid
M     12 populations of 1 .. 5 diploids named p0 .. p11 (sorted: p0, p1, p10, p11, p2, ...: pop_rank orients the blocks); M1: one population
N361  two populations of 180 + 181 haplotypes: (x + y)^2 = 130 321 values in exactly 1024 runs, the most the NumPy-order kernel
      takes; N362 (181 + 181: 1025 runs) and N363 (181 + 182: 131 769 values) are left to the fixed trees
P     58 individuals of ploidy 1, 2, 3, 4 and 6 in two populations and none: haplotype blocks of 8 values and more for k_indpair_fin
G     1030 individuals of ploidy 1 and 2: 530 965 pairs, more than the 2048 x 256 threads of k_indpair_fin's grid
S     200 diploids in 4 populations under 100 consecutive windows of 64 and 300 sites: a pass in sub-batches with both sum orders in each

The windows of F / M: 300, 0, 40 and 1 sites with 10 % missing calls, and a window of 300 sites in which the first individual of one
population is missing at every site (WIN_HOLE): the valid share of that population's blocks is then known exactly."""
import functools

import numpy as np

from genomics_general_amd.samples import HapLayout, SampleData
from oracle import popgen_oracle as orc

U = 2.0 ** -53
NONE = "~none"                                       # the oracle's group of the individuals in no population (sorts last)
WINS = [300, 0, 40, 1, 300]
WIN_SHORT, WIN_HOLE = 2, 4                           # the window minSites is read from, the window with the missing individual
N_WINS = [37, 200]
MIN_DATA = 0.01

CASES = {
    "F1": dict(seed=7101, pops=[[2] * n for n in (1, 2, 16, 17, 23, 257)], nopop=[2, 2, 2], hole=3),
    "F0": dict(seed=7102, mixed=(1, 3, 31, 32, 33, 255, 256, 257), nopop=[2, 1], hole=4),
    "M": dict(seed=7103, pops=[[2] * n for n in (3, 1, 5, 2, 4, 1, 5, 2, 3, 4, 1, 5)], nopop=[], hole=2),
    "M1": dict(seed=7104, pops=[[2] * 7], nopop=[2], hole=0),
    "N361": dict(seed=7105, pops=[[2] * 90, [2] * 90 + [1]], nopop=[], wins=N_WINS),
    "N362": dict(seed=7106, pops=[[2] * 90 + [1], [1] + [2] * 90], nopop=[], wins=N_WINS),
    "N363": dict(seed=7107, pops=[[2] * 90 + [1], [2] * 91], nopop=[], wins=N_WINS),
}
CASES["F2h"] = dict(CASES["F1"], half_called=True)


def make_layout(rng, pop_ploidies, nopop_ploidies, fmt="phased"):
    """individuals h0, h1, ... dealt to the populations at random: neither the reference's row order (haplotype names sorted) nor the
    sorted order of the individuals is the slot order"""
    groups = [list(p) for p in pop_ploidies] + [list(nopop_ploidies)]
    n = sum(len(g) for g in groups)
    names = ["h%d" % k for k in range(n)]
    deal = rng.permutation(n)
    members, ploidy_of, at = [], {}, 0
    for g in groups:
        mem = [names[k] for k in sorted(deal[at:at + len(g)])]
        at += len(g)
        for nm, pl in zip(mem, g):
            ploidy_of[nm] = int(pl)
        members.append(mem)
    sd = SampleData(indNames=list(names), popNames=["p%d" % k for k in range(len(pop_ploidies))], popInds=members[:-1], ploidyDict=ploidy_of)
    return HapLayout(sd, names, fmt)


def _mixed(rng, n_hap):
    """ploidies 1 .. 3 that add up to n_hap"""
    out = []
    while sum(out) < n_hap:
        out.append(int(min(rng.integers(1, 4), n_hap - sum(out))))
    return out


def make_rows(rng, L, lay, miss=0.10, by_individual=False):
    """allele codes (1, 2, 4, 8; 0 = missing) [L][n_hap] in slot order: two alleles per site, the second at a frequency of the
    site and the population; missing calls per haplotype, or per individual (`N|N`: the called counts per individual stay valid)"""
    H = lay.n_hap
    base = rng.integers(0, 4, size=L)
    freq = rng.random((L, lay.n_pops + 1)) * 0.6
    alt = rng.random((L, H)) < freq[:, lay.hap_pop]
    rows = (1 << ((base[:, None] + alt) % 4)).astype(np.int8)
    if by_individual:
        rows[(rng.random((L, lay.n_samp)) < miss)[:, lay.hap_sample]] = 0
    else:
        rows[rng.random((L, H)) < miss] = 0
    return rows


def bounds_of(lengths):
    hi = np.cumsum(lengths).astype(np.int64)
    return hi - np.array(lengths, dtype=np.int64), hi


def all_diploid(lay):
    return all(len(lay.ind_slots[nm]) == 2 for nm in lay.ind_order)


def form_of(lay, no_dip=False, half_called=False):
    """which form of k_popdist_fin a layout takes (pg_launch_popdist_fin): 0 unless every individual is diploid (a HapLayout's
    populations always begin and end on an individual); then 1 on called counts per individual, 2 on called counts per haplotype"""
    if not all_diploid(lay):
        return 0
    return 2 if (no_dip or half_called) else 1


def rectangles(lay, form):
    """{(x, y): pairs the block's 256 threads share out}: haplotype pairs (form 0) or individual pairs"""
    unit = 1 if form == 0 else 2
    return {(x, y): (lay.pop_sizes[x] // unit) * (lay.pop_sizes[y] // unit) for x in range(lay.n_pops) for y in range(x, lay.n_pops)}


def np_runs(n):
    """the runs (of at most 128 values) NumPy's pairwise sum cuts n values into: pieces of the ufunc buffer (8192 values), a piece
    halved -- the first half rounded down to a multiple of 8 -- until at most 128 values are left"""
    def piece(m):
        if m <= 128:
            return 1
        half = m // 2
        half -= half % 8
        return piece(half) + piece(m - half)
    return sum(piece(min(8192, n - at)) for at in range(0, n, 8192))


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: lay, gt (rows in slot order), lo, hi; hole_pop, hole_k (haplotypes missing throughout WIN_HOLE) where the case has one"""
    p = CASES[name]
    rng = np.random.default_rng(p["seed"])
    pops = p["pops"] if "pops" in p else [_mixed(rng, n) for n in p["mixed"]]
    lay = make_layout(rng, pops, p["nopop"])
    wins = p.get("wins", WINS)
    dip = all_diploid(lay)
    gt = np.concatenate([make_rows(rng, L, lay, by_individual=dip) for L in wins], axis=0)
    lo, hi = bounds_of(wins)
    out = dict(name=name, lay=lay, lo=lo, hi=hi, wins=wins)
    if "hole" in p:
        slots = np.flatnonzero(lay.hap_pop == p["hole"])
        gone = slots[lay.hap_sample[slots] == lay.hap_sample[slots[0]]]          # the population's first individual
        gt[lo[WIN_HOLE]:hi[WIN_HOLE], gone] = 0
        out.update(hole_pop=p["hole"], hole_k=len(gone))
    if p.get("half_called"):
        # `A|N`: in every window one genotype with both haplotypes called loses its second one
        rng2 = np.random.default_rng(p["seed"] + 1000)
        for a, b in zip(lo, hi):
            if b == a:
                continue
            whole = np.argwhere((gt[a:b, 0::2] != 0) & (gt[a:b, 1::2] != 0))
            site, s = whole[rng2.integers(0, len(whole))]
            gt[a + site, 2 * s + 1] = 0
    out["gt"] = np.ascontiguousarray(gt)
    return out


def oracle_aln(lay, gt, a, b):
    aln, _ = orc.aln_from_codes(gt[a:b], lay.hap_names, lay.hap_sample_name, [g if g is not None else NONE for g in lay.hap_group])
    return aln


@functools.lru_cache(maxsize=None)
def counts(name):
    """per window (aln, D, C): the oracle's alignment and pair counts, made once"""
    c = P_case() if name == "P" else case(name)
    out = []
    for a, b in zip(c["lo"], c["hi"]):
        aln = oracle_aln(c["lay"], c["gt"], int(a), int(b))
        out.append((aln,) + orc.pair_counts_gemm(aln, dtype=np.float32))
    return out


@functools.lru_cache(maxsize=None)
def min_sites_of(name):
    """a called count the oracle's C really contains, together with the count below it, near the 15th percentile of the case's
    short window: pairs with c == minSites and with c == minSites - 1 both occur"""
    _, _, C = counts(name)[0 if name.startswith("N") else 1 if name == "P" else WIN_SHORT]           # 37 or 40 sites
    v = np.sort(C[np.triu_indices(len(C), 1)])
    have = set(v.tolist())
    thr = int(v[int(0.15 * len(v))])
    while not (thr in have and thr - 1 in have):
        thr += 1
    return thr


@functools.lru_cache(maxsize=None)
def expect(name, w, min_sites, min_data=MIN_DATA):
    """(the oracle's groupDistStats of window w, its block sums): orc.group_dist_stats(..., with_sums=True)"""
    aln, D, C = counts(name)[w]
    out, _, sums = orc.group_dist_stats(aln, D, C, True, min_sites, min_data, with_sums=True)
    return out, sums


def pair_key(stat, a, b):
    """the oracle's key of a population pair's block sums (np.unique's order of the two names)"""
    return "%s_%s_%s" % ((stat,) + tuple(sorted([a, b])))


def stat_keys(lay):
    """the statistics of the layout's populations, as (key in the oracle's dictionary, kind, population names)"""
    names = lay.sampleData.popNames
    out = [("pi_" + a, "pi", (a,)) for a in names]
    for x in range(len(names) - 1):
        for y in range(x + 1, len(names)):
            out.append(("dxy_%s_%s" % (names[x], names[y]), "dxy", (names[x], names[y])))
            out.append(("Fst_%s_%s" % (names[x], names[y]), "Fst", (names[x], names[y])))
    return out


def exact_mean(block):
    """(valid cells, size, fsum) -> the mean of the valid quotients, one rounding of the exact sum and one of the division; nan for none"""
    nv, _, fs = block
    return fs / nv if nv > 0 else np.nan


def fixed_tree_bound(kind, pops, sums):
    """(reference value from the exact sums, absolute bound) for a statistic whose float64 sums are formed in SOME fixed order.
    Quotients d / c are non-negative and each within one ulp (2 U relative); n of them added in any order: (n - 1) U more; the
    reference's fsum one rounding: the sum within (n + 2) U.  pi and dxy add a division on either side: (n + 4) U, n the number of
    quotients the device adds -- every unordered pair once, half the cells of a symmetric block.  pi_t of Fst is put together from
    three such sums: n quotients in a fixed grouping, n - 1 additions as before, (n + 4) U as well.  Fst = 1 - pi_s / pi_t: the
    three means' bounds added, 4 U for the weights, the weighted sum and the division, times |pi_s / pi_t|, plus U for the
    subtraction (|Fst| <= 1)"""
    if kind == "pi":
        nv, _, _ = sums["pi_" + pops[0]]
        ref = exact_mean(sums["pi_" + pops[0]])
        return ref, (nv // 2 + 4) * U * abs(ref)
    if kind == "dxy":
        blk = sums[pair_key("dxy", *pops)]
        ref = exact_mean(blk)
        return ref, (blk[0] + 4) * U * abs(ref)
    a, b = sorted(pops)
    bx, by, bt = sums["pi_" + a], sums["pi_" + b], sums[pair_key("pit", a, b)]
    na, nb = int(round(bx[1] ** 0.5)), int(round(by[1] ** 0.5))
    w = 1. * na / (na + nb)
    pi_s = w * exact_mean(bx) + (1 - w) * exact_mean(by)
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.float64(pi_s) / np.float64(exact_mean(bt))
    rel = (bx[0] // 2 + 4) * U + (by[0] // 2 + 4) * U + (bt[0] // 2 + 4) * U + 4 * U
    return 1 - r, rel * abs(r) + U


def hole_shares(name):
    """the window with the missing individual under minSites 1: {statistic key: (valid cells, size, the reference's own float
    expression of the valid share)} for pi of the population, dxy and -- through pi_t -- Fst with its neighbour"""
    c = case(name)
    names = c["lay"].sampleData.popNames
    a = names[c["hole_pop"]]
    _, sums = expect(name, WIN_HOLE, 1)
    out = {"pi_" + a: sums["pi_" + a]}
    if len(names) > 1:
        b = names[c["hole_pop"] + 1 if c["hole_pop"] + 1 < len(names) else c["hole_pop"] - 1]
        out["dxy_%s_%s" % tuple(sorted([a, b], key=names.index))] = sums[pair_key("dxy", a, b)]
        out["Fst_%s_%s" % tuple(sorted([a, b], key=names.index))] = sums[pair_key("pit", a, b)]
    return {k: (nv, size, 1 - (1. * (size - nv) / size)) for k, (nv, size, _) in out.items()}


# ---- k_indpair_fin --------------------------------------------------------------------------------------------------------------
P_WINS = [1, 40, 300]


@functools.lru_cache(maxsize=None)
def P_case():
    rng = np.random.default_rng(7201)
    ploidy = [int(v) for v in rng.choice([1, 2, 3, 4, 6], size=58)]
    lay = make_layout(rng, [ploidy[:29], ploidy[29:56]], ploidy[56:])
    gt = np.concatenate([make_rows(rng, L, lay) for L in P_WINS], axis=0)
    lo, hi = bounds_of(P_WINS)
    return dict(name="P", lay=lay, gt=np.ascontiguousarray(gt), lo=lo, hi=hi, wins=P_WINS)


@functools.lru_cache(maxsize=None)
def P_expect(masked, include_same):
    """per window the oracle's indPairDists {a: {b: value}} (rows: the haplotypes of a), after groupDistStats(minSites) when masked"""
    out = []
    for aln, D, C in counts("P"):
        dm = orc.group_dist_stats(aln, D, C, True, min_sites_of("P"), MIN_DATA)[1] if masked else orc.dist_from_counts(D, C)
        out.append(orc.ind_pair_dists(aln, dm, include_same)[0])
    return out


def slot_counts(gt):
    """the oracle's D, C of the rows gt [L][n_hap] with the haplotypes left in slot order"""
    lut = np.full(256, -999, dtype=np.int64)
    lut[1], lut[2], lut[4], lut[8] = 0, 1, 2, 3
    num = np.ascontiguousarray(lut[np.asarray(gt).astype(np.uint8)].T)
    return orc.pair_counts_gemm(orc.Aln(num, [], [], []), dtype=np.float32)


def pair_table_np(D, C, lay, min_sites, include_same):
    """np.nanmean of every individual pair's haplotype block for individuals of at most two haplotypes, all pairs at once: the block's
    cells added in row order from 0.0 (NumPy's order for fewer than 8 values), a nan as 0.0; rows: the earlier individual in slot
    order.  D, C symmetric [n_hap][n_hap] in slot order; the diagonal nan, or a zero that counts.  [pair (s <= t)] as
    lay.sample_pair_index orders them"""
    start = np.array([lay.ind_slots[nm][0] for nm in lay.ind_order])
    pl = np.array([len(lay.ind_slots[nm]) for nm in lay.ind_order])
    assert pl.max() <= 2
    s, t = np.triu_indices(lay.n_samp)
    thr = max(int(min_sites or 0), 1)
    tot, cnt = np.zeros(len(s)), np.zeros(len(s), dtype=np.int64)
    for i in (0, 1):
        for j in (0, 1):
            live = (pl[s] > i) & (pl[t] > j)
            a, b = np.where(live, start[s] + i, 0), np.where(live, start[t] + j, 0)
            ok = live & (a != b) & (C[a, b] >= thr)
            tot = tot + np.where(ok, D[a, b] / np.where(ok, C[a, b], 1), 0.0)
            cnt += ok
            if include_same:
                cnt += live & (a == b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(cnt > 0, tot / cnt, np.nan)


G_MIN_SITES = 20
G_ROW_MIN_SITES = 29                                 # of the window of 40 real rows: pairs share 32 called sites on average
G_FIRST_LATE = 2048 * 256                            # the first pair of the grid's second trip


@functools.lru_cache(maxsize=None)
def G_case():
    """dict: lay (1030 individuals of ploidy 1 and 2 in no population), D, C (int32 [2][n_hap][n_hap], symmetric, D <= C drawn from the
    seed; cells with C = 0, G_MIN_SITES and G_MIN_SITES - 1 planted among the last individuals), gt (40 sites of real rows)"""
    rng = np.random.default_rng(7301)
    names = ["h%d" % k for k in range(1030)]
    ploidy = {nm: int(v) for nm, v in zip(names, rng.choice([1, 2], size=1030))}
    lay = HapLayout(SampleData(indNames=list(names), ploidyDict=ploidy), names, "phased")
    H = lay.n_hap
    C = np.triu(rng.integers(0, 60, size=(2, H, H)), 1)
    D = np.triu((rng.random((2, H, H)) * (C + 1)).astype(np.int64), 1)
    for k, v in enumerate([0, G_MIN_SITES, G_MIN_SITES - 1] * 8):
        C[:, H - 40 - k, H - 1 - k] = v
        D[:, H - 40 - k, H - 1 - k] = v // 2
    C, D = C + C.transpose(0, 2, 1), D + D.transpose(0, 2, 1)
    gt = make_rows(rng, 40, lay)
    return dict(lay=lay, D=np.ascontiguousarray(D, dtype=np.int32), C=np.ascontiguousarray(C, dtype=np.int32), gt=gt)


# ---- sub-batches ----------------------------------------------------------------------------------------------------------------
S_MIN_SITES = 5
S_CHECKED = (0, 1, 50, 51, 98, 99)                   # windows of the first, a middle and the last batch: 64 and 300 sites each


@functools.lru_cache(maxsize=None)
def S_case():
    rng = np.random.default_rng(7401)
    lay = make_layout(rng, [[2] * 50] * 4, [])
    lens = [64, 300] * 50
    lens[31], lens[66] = 0, 1
    gt = make_rows(rng, sum(lens), lay, by_individual=True)
    lo, hi = bounds_of(lens)
    return dict(name="S", lay=lay, gt=gt, lo=lo, hi=hi, wins=lens)


@functools.lru_cache(maxsize=None)
def S_expect(w):
    """window w of S: (the oracle's groupDistStats, its block sums, D, C in slot order)"""
    c = S_case()
    a, b = int(c["lo"][w]), int(c["hi"][w])
    aln = oracle_aln(c["lay"], c["gt"], a, b)
    D, C = orc.pair_counts_gemm(aln, dtype=np.float32)
    out, _, sums = orc.group_dist_stats(aln, D, C, True, S_MIN_SITES, MIN_DATA, with_sums=True)
    return (out, sums) + slot_counts(c["gt"][a:b])
