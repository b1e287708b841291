"""Seeded cases for the float finishers behind the pair counts -- k_hapstats (H12stats), k_sample_het (sampleHet), k_paint -- at the
sizes where their loops turn over.  Builders only: rows, layouts, windows and what the oracle (oracle/popgen_oracle.py) and the
NumPy model (tests/paint_model.py) make of them; no parser and no engine.  tests/test_finisher_cases.py shows without a GPU that the
cases contain what they are built for; tests/test_gpu_finishers.py and tests/test_gpu_paint.py run the device over the same cases.

hapStats  the haplotypes of a population are copies of founder haplotypes, window by window: group sizes drawn from GROUPS_A (or
          GROUPS_B: smaller groups, more clusters; GROUPS_C: larger ones), members dealt to random rows.  A window is clean, carries
          a low per-site mutation rate ("mut"), makes every group a chain of copies each a few sites from the one before ("drift":
          matches are not transitive under maxDist > 0, and which of several tied rows founds a cluster changes the sizes), or has
          5 % missing calls ("miss": the minSites mask of a preceding groupDistStats removes some pairs of a 40-site window, not
          all).  Individuals are named h0, h1, ... and dealt to the populations at random, so the reference's row order (names
          sorted) is not the slot order.
    Hs    haploid, populations of 1, 2, 31, 32, 33, 64, 65, 255, 256 and 257 haplotypes (around the 32-bit mask word and the 256
          threads of the row loop), three individuals in no population
    Hd    haploid, populations of 513 and 600: more than 1024 slots, third trips of the row loop, more than 512 clusters
    Dd    phased diploids, populations of 2 x {16, 17, 64, 65} haplotypes; DdN: the same rows with some `A|N` genotypes, which
          withdraw the per-individual called counts
    X4    phased diploids with four alleles at nearly every site: a fresh engine's first pass overflows its reservation and starts over
indHet    90 samples of ploidy 1, 2, 3 and 4 over 7 windows (630 cells: a third block of 256 threads), and the same rows under 400
          short windows for a pass in sub-batches
paint     A and B as tests/test_gpu_paint.py has had them; C: 260 individuals, reference lists of 1024, 1000 and 24 (2048 in all,
          the limit, with duplicates); D: 130 individuals, 64 populations (the limit) of 1, 2 and 3; S: 600 individuals under 27
          short windows, whose matrices exceed the smallest scratch limit twice over; F: four-allele rows, a pass that starts over"""
import functools

import numpy as np

import paint_model
from genomics_general_amd.samples import HapLayout, SampleData
from oracle import popgen_oracle as orc

GROUPS_A = (1, 1, 1, 2, 2, 3, 5, 9)
GROUPS_B = (1, 1, 1, 1, 2, 2, 3)
GROUPS_C = (2, 3, 5, 9, 9, 14)
HAP_STATES = ("plain", "popdist", "indpair")        # the cached matrix: as counted, after groupDistStats(minSites), after indPairDists(False)
HAP_MAX_DISTS = (-1, 0, 0.01)
HAP_MIN_SITES = 36                                  # of the "popdist" state: 40 sites with 5 % missing calls share 36 on average

# (sites, kind, group sizes); the empty and the one-site window stand inside the list: under a scratch limit they fall into later batches
_WINS_S = [(300, "clean", GROUPS_A), (40, "miss", GROUPS_A), (1200, "clean", GROUPS_A), (0, "clean", GROUPS_A), (40, "clean", GROUPS_B),
           (300, "mut", GROUPS_A), (1, "clean", GROUPS_A), (300, "miss", GROUPS_B), (40, "mut", GROUPS_A), (1200, "drift", GROUPS_C),
           (40, "miss", GROUPS_B), (300, "clean", GROUPS_B), (300, "drift", GROUPS_C)]
_WINS_D = [(300, "clean", GROUPS_A), (0, "clean", GROUPS_A), (300, "mut", GROUPS_B), (40, "miss", GROUPS_A), (1, "clean", GROUPS_A),
           (1200, "clean", GROUPS_B), (300, "drift", GROUPS_C)]
HAP_CASES = {
    "Hs": dict(seed=5101, ploidy=1, pops=[1, 2, 31, 32, 33, 64, 65, 255, 256, 257], nopop=3, wins=_WINS_S),
    "Hd": dict(seed=5102, ploidy=1, pops=[513, 600], nopop=0, wins=_WINS_D),
    "Dd": dict(seed=5103, ploidy=2, pops=[16, 17, 64, 65], nopop=0, wins=_WINS_S),
    "DdN": dict(seed=5103, ploidy=2, pops=[16, 17, 64, 65], nopop=0, wins=_WINS_S, half_called=0.03),
    "X4": dict(seed=5104, ploidy=2, pops=[17, 33, 65], nopop=2, four=True,
               wins=[(700, "clean", GROUPS_A), (0, "clean", GROUPS_A), (500, "mut", GROUPS_A), (1, "clean", GROUPS_A), (600, "miss", GROUPS_B)]),
}


def _layout(rng, ploidy, pops, nopop, fmt):
    """individuals h0, h1, ... dealt to the populations at random"""
    n = sum(pops) + nopop
    names = ["h%d" % k for k in range(n)]
    deal = rng.permutation(n)
    members, at = [], 0
    for s in pops:
        members.append([names[k] for k in deal[at:at + s]])
        at += s
    ploidy_of = {nm: (ploidy[k] if isinstance(ploidy, list) else ploidy) for k, nm in enumerate(names)}
    sd = SampleData(indNames=list(names), popNames=["p%d" % k for k in range(len(pops))], popInds=members, ploidyDict=ploidy_of)
    lay = HapLayout(sd, names, fmt)
    assert list(lay.ref_order) != list(range(lay.n_hap))
    return lay


def _window_rows(rng, L, kind, sizes_from, lay, four):
    """allele codes (1, 2, 4, 8; 0 = missing) [L][n_hap] in slot order"""
    H = lay.n_hap
    allele = np.zeros((L, H), dtype=np.int64)
    base = rng.integers(0, 4, size=L)
    for p in range(-1, lay.n_pops):
        slots = np.where(lay.hap_pop == p)[0]
        n = len(slots)
        if n == 0:
            continue
        if p < 0:
            group_of = np.arange(n)
        else:
            sizes = []
            while sum(sizes) < n:
                sizes.append(int(rng.choice(sizes_from)))
            sizes[-1] -= sum(sizes) - n
            group_of = rng.permutation(np.repeat(np.arange(len(sizes)), sizes))
        ng = int(group_of.max()) + 1
        if four:
            founders = rng.integers(0, 4, size=(L, ng))
        else:
            founders = (base[:, None] + (rng.random((L, ng)) < 0.5)) % 4       # two alleles per site
        a = founders[:, group_of]
        if kind == "mut" and L > 0:
            flip = rng.random((L, n)) < 0.6 / L                                  # about every second haplotype differs from its founder
            other = (a + 1 + rng.integers(0, 3, size=(L, n))) % 4 if four else (2 * base[:, None] + 1 - a) % 4
            a = np.where(flip, other, a)
        if kind == "drift":
            # a group is a chain: every member copies the one before it and changes a few sites more (0.4 % of them on average), so
            # that under maxDist 0.01 a haplotype matches its neighbours along the chain and not the far end: tied rows whose
            # matches differ, and clusters that depend on which of them is taken
            for g in range(ng):
                cols = np.flatnonzero(group_of == g)
                for prev, col in zip(cols[:-1], cols[1:]):
                    a[:, col] = a[:, prev]
                    at = rng.integers(0, L, size=rng.poisson(0.004 * L))
                    a[at, col] = (2 * base[at] + 1 - a[at, col]) % 4
        allele[:, slots] = a
    rows = (1 << allele).astype(np.int8)
    if kind == "miss":
        # per individual (`N|N`): the haplotypes of a diploid stay called together, the per-individual called counts stay valid
        rows[(rng.random((L, lay.n_samp)) < 0.05)[:, lay.hap_sample]] = 0
    return rows


@functools.lru_cache(maxsize=None)
def hap_case(name):
    """dict: lay, gt (rows in slot order), lo, hi, wins (the window table)"""
    p = HAP_CASES[name]
    rng = np.random.default_rng(p["seed"])
    lay = _layout(rng, p["ploidy"], p["pops"], p["nopop"], "haplo" if p["ploidy"] == 1 else "phased")
    gt = np.concatenate([_window_rows(rng, L, kind, sizes, lay, p.get("four", False)) for L, kind, sizes in p["wins"]], axis=0)
    if p.get("half_called"):
        # `A|N`: the second haplotype of an individual missing where the first is called
        second = np.array([lay.ind_slots[nm][1] for nm in lay.ind_order])
        hole = np.random.default_rng(p["seed"] + 1000).random((len(gt), len(second))) < p["half_called"]
        sub = gt[:, second]
        sub[hole] = 0
        gt[:, second] = sub
    hi = np.cumsum([w[0] for w in p["wins"]]).astype(np.int64)
    lo = hi - np.array([w[0] for w in p["wins"]], dtype=np.int64)
    return dict(name=name, lay=lay, gt=np.ascontiguousarray(gt), lo=lo, hi=hi, wins=p["wins"])


def oracle_aln(lay, gt, a, b):
    aln, _ = orc.aln_from_codes(gt[a:b], lay.hap_names, lay.hap_sample_name, [g if g is not None else "~none" for g in lay.hap_group])
    return aln


@functools.lru_cache(maxsize=None)
def hap_counts(name):
    """per window (aln, D, C): the oracle's alignment and pair counts, made once"""
    c = hap_case(name)
    out = []
    for a, b in zip(c["lo"], c["hi"]):
        aln = oracle_aln(c["lay"], c["gt"], int(a), int(b))
        D, C = orc.pair_counts_gemm(aln, dtype=np.float32)
        out.append((aln, D, C))
    return out


def cached_dist(aln, D, C, state, min_sites=HAP_MIN_SITES):
    """the distance matrix the reference's worker has cached in that state"""
    if state == "popdist":
        return orc.group_dist_stats(aln, D, C, False, min_sites, 0.01)[1]
    dm = orc.dist_from_counts(D, C)
    if state == "indpair":
        np.fill_diagonal(dm, np.nan)                 # (genomics.py:940: what indPairDists leaves; orc.ind_pair_dists does the same)
    return dm


@functools.lru_cache(maxsize=None)
def hap_expect(name, state, max_dist):
    """per window the oracle's H12stats"""
    return [orc.h12_stats(aln, cached_dist(aln, D, C, state), max_dist) for aln, D, C in hap_counts(name)]


def greedy_trace(match, rule="first"):
    """distMat_to_cluster_sizes' loop (orc.h12_stats) with the rows kept in place: the cluster sizes, and for every step at which
    several alive rows share the maximum and do not all have the same alive matches (so the rule decides which cluster is founded):
    (row distance between the first tied row and the farthest one with other matches, whether some tied row's matches differ from
    the first one's only in columns from 32 on).  rule "last" takes the last tied row instead: what a wrong tie break would give"""
    match = np.asarray(match, dtype=bool)
    n = len(match)
    alive = np.ones(n, dtype=bool)
    counts = match.sum(axis=1).astype(np.int64)
    sizes, ties = [], []
    while alive.any():
        c = np.where(alive, counts, -1)
        m = int(c.max())
        if m <= 1:
            sizes += [1] * int(alive.sum())
            break
        tied = np.flatnonzero(c == m)
        most = tied[0] if rule == "first" else tied[-1]
        if len(tied) > 1:
            sets = match[tied] & alive
            other = (sets != sets[0]).any(axis=1)
            if other.any():
                xor = sets[other] ^ sets[0]
                ties.append((int(tied[other][-1] - tied[0]), bool((~xor[:, :32].any(axis=1)).any())))
        leave = match[most] & alive
        sizes.append(m)
        alive &= ~match[most]
        counts -= match[:, leave].sum(axis=1)
    return sizes, ties


def h_of_sizes(sizes):
    """H1, H12, H2 as genomics.py:1088-1096 forms them from the cluster sizes"""
    sizes = np.array(sizes)
    f = sizes / sizes.sum()
    H1 = (f ** 2).sum()
    return (H1, H1 + 2 * f[0] * f[1], (f[1:] ** 2).sum()) if len(f) > 1 else (H1, H1, 0)


# ---- indHet -------------------------------------------------------------------------------------------------------------------
HET_WINS = [300, 0, 41, 1, 40, 2, 3]
HET_MIN_SITES = 38                                  # of a preceding groupDistStats: the windows of 40 and 41 sites share about 36
HET_SUB_MIN_SITES = 14                              # ... under the short windows of the pass in sub-batches


@functools.lru_cache(maxsize=None)
def het_case():
    """90 samples of ploidy 1 .. 4 in two populations; 10 % missing calls.  dict: lay, gt, lo, hi (the 7 windows), sub_lo, sub_hi (400
    windows of 0, 1, 5, 17 and 30 sites over the same rows: at least 0.21 MB of matrices each, 86 MB in all, three batches of at
    most 32 MiB under the smallest scratch limit)"""
    rng = np.random.default_rng(5201)
    ploidy = [int(v) for v in rng.choice([1, 2, 2, 2, 3, 4], size=90)]
    lay = _layout(rng, ploidy, [40, 45], 5, "phased")
    L = sum(HET_WINS)
    base = rng.integers(0, 4, size=L)
    rows = (1 << ((base[:, None] + (rng.random((L, lay.n_hap)) < 0.3)) % 4)).astype(np.int8)
    rows[rng.random(rows.shape) < 0.10] = 0
    hi = np.cumsum(HET_WINS).astype(np.int64)
    lo = hi - np.array(HET_WINS, dtype=np.int64)
    k = np.arange(400)
    sub_lo = (k * 7) % (L - 30)
    sub_hi = sub_lo + np.array([17, 0, 30, 1, 5])[k % 5]
    return dict(lay=lay, gt=rows, lo=lo, hi=hi, sub_lo=sub_lo.astype(np.int64), sub_hi=sub_hi.astype(np.int64))


@functools.lru_cache(maxsize=None)
def het_expect(sub, masked):
    """per window (the oracle's sampleHet, the diploids' jointly called counts by name); masked: after groupDistStats(minSites)"""
    c = het_case()
    lay = c["lay"]
    out = []
    for a, b in zip(c["sub_lo" if sub else "lo"], c["sub_hi" if sub else "hi"]):
        aln = oracle_aln(lay, c["gt"], int(a), int(b))
        D, C = orc.pair_counts_gemm(aln)
        dm = cached_dist(aln, D, C, "popdist" if masked else "plain", HET_SUB_MIN_SITES if sub else HET_MIN_SITES)
        rows = {}
        for r, s in enumerate(aln.sample_names):
            rows.setdefault(s, []).append(r)
        called = {s: int(C[x[0], x[1]]) for s, x in rows.items() if len(x) == 2}
        out.append((orc.sample_het(aln, dm, C), called))
    return out


# ---- paint --------------------------------------------------------------------------------------------------------------------
PAINT_SHAPES = {
    "A": dict(seed=4101, n=70, sizes=[1, 2, 7, 8, 9, 33], wins=[0, 3, 8, 12, 16, 40, 257, 600], miss=0.30, min_sites=6, n_src=6),
    "B": dict(seed=4102, n=200, sizes=[130, 64], wins=[50, 300, 1000], miss=0.10, min_sites=20, n_src=2),
    # lists drawn with replacement from the individuals of the population's source: 2048 reference individuals among 260
    "C": dict(seed=4103, n=260, sizes=[1024, 1000, 24], wins=[300, 0, 40, 300], miss=0.30, min_sites=16, n_src=3, replace=True),
    "D": dict(seed=4104, n=130, sizes=[1, 2, 3] * 21 + [2], wins=[40, 0, 300, 12], miss=0.30, min_sites=6, n_src=8),
    "S": dict(seed=4105, n=600, sizes=[5, 9, 12], wins=[17, 3, 30] + [12, 40, 8, 16, 0, 24, 1] * 3 + [30, 2, 17], miss=0.30, min_sites=6, n_src=3),
    "F": dict(seed=4106, n=70, sizes=[5, 9, 12], wins=[600, 0, 800, 12], miss=0.30, min_sites=6, n_src=3, four=True),
}


@functools.lru_cache(maxsize=None)
def paint_case(name):
    """(layout, rows in slot order, window bounds, reference lists, D, C in the alignment's order with the called counts on C's
    diagonal); individuals are named h0, h1, ... so that the sorted order (h0, h1, h10, ...) is not the file's"""
    p = PAINT_SHAPES[name]
    rng = np.random.default_rng(p["seed"])
    n = p["n"]
    names = ["h%d" % k for k in range(n)]
    lay = HapLayout(SampleData(indNames=list(names), ploidyDict={nm: 1 for nm in names}), names, "haplo")
    assert list(lay.ref_order) != list(range(n))
    L = sum(p["wins"])
    if p.get("replace"):
        src = rng.integers(0, p["n_src"], size=n)             # by alignment row
        ref_lists = [[int(v) for v in rng.choice(np.flatnonzero(src == k % p["n_src"]), size=s)] for k, s in enumerate(p["sizes"])]
    else:
        # reference individuals: a random choice of the alignment's rows, a population drawing its alleles from its own source; one
        # individual is in two populations and one twice in the same
        perm = rng.permutation(n)
        ref_lists, at = [], 0
        for s in p["sizes"]:
            ref_lists.append([int(v) for v in perm[at:at + s]])
            at += s
        ref_lists[-1][-1] = ref_lists[-1][0]
        ref_lists[0][0] = ref_lists[-1][1]
        src = rng.integers(0, p["n_src"], size=n)             # by alignment row
        for k, r in enumerate(ref_lists):
            src[r] = k % p["n_src"]
    freq = rng.choice([0.05, 0.3, 0.7, 0.95], size=(L, p["n_src"]))
    # a fifth of the individuals draw every site from a source of its own: near no population in particular (noresult cells)
    src_site = np.where(rng.random(n) < 0.2, rng.integers(0, p["n_src"], size=(L, n)), src[None, :])
    alt = rng.random((L, n)) < np.take_along_axis(freq, src_site, axis=1)
    base = rng.integers(0, 4, size=L)
    allele = np.where(alt, (base[:, None] + 1 + rng.integers(0, 2, size=(L, 1))) % 4, base[:, None])
    if p.get("four"):
        # nearly every site with four alleles: four calls in ten are replaced by any allele
        allele = np.where(rng.random((L, n)) < 0.4, rng.integers(0, 4, size=(L, n)), allele)
    rows = (1 << allele).astype(np.int8)                      # allele codes 1, 2, 4, 8; 0 = missing
    rows[rng.random((L, n)) < p["miss"]] = 0
    hi = np.cumsum(p["wins"]).astype(np.int64)
    lo = hi - np.array(p["wins"], dtype=np.int64)
    D = np.zeros((len(lo), n, n), dtype=np.int64)
    C = np.zeros_like(D)
    for w, (a, b) in enumerate(zip(lo, hi)):
        g = rows[a:b]
        called = (g != 0).astype(np.float64)                  # (counts below 2^53: exact in float64)
        Cw = called.T @ called
        same = sum((g == code).astype(np.float64).T @ (g == code).astype(np.float64) for code in (1, 2, 4, 8))
        C[w] = Cw.astype(np.int64)
        D[w] = (Cw - same).astype(np.int64)
    gt = np.zeros((L, n), dtype=np.int8)
    gt[:, lay.ref_order] = rows                               # slot (= file) order: alignment row k is slot ref_order[k]
    return lay, gt, lo, hi, ref_lists, D, C


@functools.lru_cache(maxsize=None)
def paint_expect(name, p_threshold, delta_threshold, noresult):
    """the model's decisions, its cells with a nan mean, and what the windows contained"""
    _, _, _, _, ref_lists, D, C = paint_case(name)
    info = {}
    out, nan_mean = paint_model.paint_windows(D, C, ref_lists, PAINT_SHAPES[name]["min_sites"], p_threshold=p_threshold,
                                              delta_threshold=delta_threshold, noresult=noresult, info=info)
    return out, nan_mean, info
