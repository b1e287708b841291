"""Seeded cases for the site-statistics kernels -- k_abba_q, k_abba_reduce, k_quartet_np (ABBABABA, fourPop) and k_popfreq_q, k_popfreq,
k_popfreq_ordered (groupFreqStats) -- past the layout every other test gives them (four populations of equal size, in slot order,
nobody left over).  Builders only: layouts, rows, windows and what the oracle (oracle/popgen_oracle.py) makes of them; no parser and
no engine.  tests/test_quartet_cases.py shows without a GPU that the cases contain what they are built for; tests/test_gpu_quartet.py
runs the device over the same cases.

Layouts   individuals h0, h1, ... of ploidy 1 and 2 dealt to the populations at random (the reference's row order, names sorted, is
          not the slot order); the populations' sizes in haplotype slots are given, so that their slot ranges start and end where the
          nibble masks of range_counts_x4 and the per-lane masks of the screening pass (umask) turn over
    N     73 slots: populations of 7, 9, 1, 33, 5, 3 and 11 haplotypes and three individuals in no population (NPASS 1); N50: the
          same layout with half of the calls missing, for minData 0 (0/0 frequencies)
    E256, E257, E512, E513, E1024, E1025: exactly that many slots, on both sides of every dispatch border of the row width (NPASS 1 | 2,
          2 | 4, 4 | 0 and k_popfreq_q<4> | k_popfreq); six populations up to 257 slots, five above
    F13, F16, F16w, F16x, F17: 13, 16, 16, 16 and 17 populations for groupFreqStats (k_popfreq_q's lanes own the populations q, q + 4,
          q + 8, q + 12; 17 are refused), about 90, 90, 700, 1100 and 90 slots
Quartets  P1 .. P4 out of slot order, the outgroup first of the four in the row with P1 last, populations before, between and behind
          the four left out (as far as a layout of five or six populations has them: there the quartets leave out different ones);
          in N the population of one haplotype is P2 in one quartet and the outgroup in the other
Rows      two alleles per site with a frequency per population that is 0 (40 %), 1 (25 %), 1/2 (12 %: 50:50 sites) or uniform; 30 % of the sites invariant;
          at 60 % of the sites one population (or the individuals in none) carries a third allele at 30 % of its haplotypes -- inside
          the quartet that voids the site, outside it must not; missing calls by site: none at 55 % of the sites, 2, 10, 40 and 75 %
          at the others (6 % of all calls; groupFreqStats keeps the complete sites alone, and minData needs sites with few calls);
          two stretches of 40 sites where no population has a call
Windows   the whole range, windows that cross the 4096-site block of k_abba_q by 3 sites and by 1, one that ends on its edge, an
          empty one, one site, windows of at most 256 sites that start off a multiple of 128, windows without a good site, and ten
          of 300 to 700 sites"""
import functools

import numpy as np

from genomics_general_amd.samples import HapLayout, SampleData
from oracle import popgen_oracle as orc

L_NARROW, L_WIDE = 9000, 4500
BLANK = 40                                           # sites [3000, 3040) and [L - 40, L): no call in any population
MODES = ("abba", "minor", "polarize", "fixed")       # ABBABABA, and fourPop's three allele choices
MIN_DATA = (0, 0.3)

_Q7 = [("p5", "p1", "p4", "p2"), ("p5", "p2", "p3", "p1")]          # leave out p0, p3 / p4, p6; p2 is the one-haplotype population
_Q6 = [("p5", "p1", "p4", "p2"), ("p4", "p1", "p3", "p0")]          # leave out p0, p3 and p2, p5
_Q5 = [("p3", "p0", "p4", "p1"), ("p4", "p2", "p3", "p1")]          # leave out p2 and p0
# minData of exactly k / N: (value, population, k); 1/3 is also 3/9 and 11/33 of the other populations of the quartets
GRID = ((1 / 3, "p5", 1), (0.6, "p4", 3), (5 / 9, "p1", 5))

CASES = {
    "N": dict(seed=6104, L=L_NARROW, pops=[7, 9, 1, 33, 5, 3, 11], nopop=[1, 2, 1], quartets=_Q7),
    "N50": dict(seed=6102, L=L_NARROW, pops=[7, 9, 1, 33, 5, 3, 11], nopop=[1, 2, 1], quartets=_Q7, miss=0.5),
    "E256": dict(seed=6111, L=L_WIDE, pops=[7, 58, 39, 50, 40, 59], nopop=[1, 2], quartets=_Q6),
    "E257": dict(seed=6112, L=L_WIDE, pops=[7, 58, 39, 50, 40, 63], nopop=[], quartets=_Q6),
    "E512": dict(seed=6113, L=L_WIDE, pops=[7, 202, 103, 100, 100], nopop=[], quartets=_Q5),
    "E513": dict(seed=6114, L=L_WIDE, pops=[7, 202, 103, 100, 101], nopop=[], quartets=_Q5),
    "E1024": dict(seed=6115, L=L_WIDE, pops=[7, 402, 207, 200, 208], nopop=[], quartets=_Q5),
    "E1025": dict(seed=6116, L=L_WIDE, pops=[7, 402, 207, 200, 209], nopop=[], quartets=_Q5),
    "F13": dict(seed=6121, L=L_WIDE, pops=[2, 3, 5, 7, 9, 11, 13, 4, 6, 8, 10, 3, 7], nopop=[1, 2], quartets=[]),
    "F16": dict(seed=6122, L=L_WIDE, pops=[2, 3, 5, 7, 9, 11, 4, 6, 8, 10, 3, 5, 2, 4, 6, 3], nopop=[2, 1], quartets=[]),
    "F16w": dict(seed=6123, L=L_WIDE, pops=[40 + (7 * k) % 9 for k in range(16)], nopop=[], quartets=[]),
    "F16x": dict(seed=6124, L=L_WIDE, pops=[65 + (7 * k) % 9 for k in range(16)], nopop=[], quartets=[]),
    "F17": dict(seed=6125, L=300, pops=[2, 3, 5, 7, 9, 11, 4, 6, 8, 10, 3, 5, 2, 4, 6, 3, 2], nopop=[], quartets=[]),
}
QUARTET_CASES = ("N", "N50", "E256", "E257", "E512", "E513", "E1024", "E1025")
FREQ_CASES = ("F13", "F16", "F16w", "F16x", "E256", "E257", "E512", "E513", "E1024", "E1025")


def min_datas(name):
    """N50 is there for minData 0; N also takes the values of exactly k / N"""
    return MIN_DATA + tuple(g[0] for g in GRID) if name == "N" else MIN_DATA


def windows(L):
    w = [(0, L), (1, 4100), (4, 4100), (200, 4297), (300, 300), (77, 78), (130, 330), (4037, 4293), (L - BLANK, L), (3000, 3000 + BLANK)]
    return w + [(250 + 390 * k, 550 + 431 * k) for k in range(10)] if L >= L_WIDE else [(0, L), (7, 7), (3, 200)]


def empty_ok(L):
    """the sites where a population may be without any call (outside the two stretches where all are): inside the whole-range window
    and no other"""
    return (6000, 6200) if L == L_NARROW else (L - BLANK - 30, L - BLANK)


def _layout(rng, pops, nopop):
    """populations of the given numbers of haplotype slots made of individuals of ploidy 1 and 2, names dealt at random"""
    ploidies, members = [], []
    for h in pops:
        d = int(rng.integers(0, h // 2 + 1))                               # diploids; the rest haploid
        pl = [int(v) for v in rng.permutation([2] * d + [1] * (h - 2 * d))]
        members.append(list(range(len(ploidies), len(ploidies) + len(pl))))
        ploidies += pl
    ploidies += list(nopop)
    n = len(ploidies)
    deal = rng.permutation(n)
    names = ["h%d" % k for k in range(n)]
    of = ["h%d" % deal[k] for k in range(n)]                               # individual k carries the name h<deal[k]>
    sd = SampleData(indNames=list(names), popNames=["p%d" % k for k in range(len(pops))], popInds=[[of[k] for k in m] for m in members],
                    ploidyDict={of[k]: ploidies[k] for k in range(n)})
    lay = HapLayout(sd, names, "phased")
    assert lay.pop_sizes == list(pops) and lay.n_hap == sum(pops) + sum(nopop)
    assert list(lay.ref_order) != list(range(lay.n_hap))
    return lay


_REST = {1: (2, 3), 2: (1, 3), 3: (1, 2)}            # b = a + d (mod 4): the offsets of the two other bases


def _rows(rng, lay, L, miss):
    """allele codes (1, 2, 4, 8; 0 = missing) [L][n_hap] in slot order"""
    H = lay.n_hap
    grp = np.where(lay.hap_pop >= 0, lay.hap_pop, lay.n_pops)              # the individuals in no population: one more group
    G = int(grp.max()) + 1
    a = rng.integers(0, 4, size=L)
    d = rng.integers(1, 4, size=L)
    b = (a + d) % 4
    pick = rng.integers(0, 2, size=L)
    c = (a + np.array([_REST[int(x)][int(k)] for x, k in zip(d, pick)], dtype=np.int64).reshape(L)) % 4
    u = rng.random((L, G))
    f = np.where(u < 0.4, 0.0, np.where(u < 0.65, 1.0, np.where(u < 0.77, 0.5, rng.random((L, G)))))
    f[rng.random(L) < 0.3] = 0.0                                           # invariant sites
    allele = np.where(rng.random((L, H)) < f[:, grp], b[:, None], a[:, None])
    carrier = np.where(rng.random(L) < 0.6, rng.integers(0, G, size=L), -1)
    third = (grp[None, :] == carrier[:, None]) & (rng.random((L, H)) < 0.3)
    allele = np.where(third, c[:, None], allele)
    rows = (1 << allele).astype(np.int8)
    if miss is None:
        called = rows.copy()
        # a population without any call (a 0 / 0 frequency under minData 0, and with it nan sums) only among the sites of `empty_ok`,
        # where calls are rarer: the whole-range window has them, the other windows add up numbers
        lo, hi = empty_ok(L)
        rate = rng.choice([0.0, 0.02, 0.1, 0.4, 0.75], p=[0.57, 0.25, 0.10, 0.055, 0.025], size=L)
        rate[lo:hi] = rng.choice([0.0, 0.4, 0.75], p=[0.4, 0.3, 0.3], size=hi - lo)
        rows[rng.random((L, H)) < rate[:, None]] = 0
        for p in range(lay.n_pops):
            cols = np.flatnonzero(lay.hap_pop == p)
            for s in np.flatnonzero((rows[:, cols] == 0).all(axis=1)):
                if not lo <= s < hi:
                    k = cols[rng.integers(0, len(cols))]
                    rows[s, k] = called[s, k]
    else:
        rows[rng.random((L, H)) < miss] = 0
    if L >= L_WIDE:
        in_pop = lay.hap_pop >= 0
        for s in (3000, L - BLANK):
            sub = rows[s:s + BLANK]
            sub[:, in_pop] = 0
    return np.ascontiguousarray(rows)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict: name, lay, gt (rows in slot order), L, wins, quartets, and `start`: the populations' first slots (and the end of the last)"""
    p = CASES[name]
    rng = np.random.default_rng(p["seed"])
    lay = _layout(rng, p["pops"], p["nopop"])
    gt = _rows(rng, lay, p["L"], p.get("miss"))
    start = np.concatenate([[0], np.cumsum(lay.pop_sizes)]).astype(np.int64)
    return dict(name=name, lay=lay, gt=gt, L=p["L"], wins=windows(p["L"]), quartets=p["quartets"], start=start)


def pop_range(c, pop):
    k = c["lay"].sampleData.popNames.index(pop)
    return int(c["start"][k]), int(c["start"][k + 1])


@functools.lru_cache(maxsize=None)
def full_aln(name, merge_solo=False):
    """the oracle's alignment of all the sites; merge_solo: populations of one haplotype join the individuals in no population
    (groupFreqStats has no value for them: 0 / 0 per site and a division by zero in Tajima's D, genomics.py:612, 624)"""
    c = case(name)
    lay = c["lay"]
    solo = {lay.sampleData.popNames[k] for k, s in enumerate(lay.pop_sizes) if s < 2} if merge_solo else set()
    groups = [g if g is not None and g not in solo else "~none" for g in lay.hap_group]
    aln, _ = orc.aln_from_codes(c["gt"], lay.hap_names, lay.hap_sample_name, groups)
    return aln


def window_aln(name, a, b, merge_solo=False):
    full = full_aln(name, merge_solo)
    return orc.Aln(np.ascontiguousarray(full.num[:, a:b]), full.names, full.sample_names, full.groups)


def oracle_quartet(name, quartet, min_data, mode, a, b):
    """(statistics, window sums) of one window: orc.abbababa or orc.four_pop"""
    aln = window_aln(name, a, b)
    if mode == "abba":
        return orc.abbababa(aln, *quartet, min_data, with_sums=True)
    return orc.four_pop(aln, *quartet, min_data, mode == "polarize", mode == "fixed", with_sums=True)


@functools.lru_cache(maxsize=None)
def expect(name, qi, min_data, mode):
    """per window of the case (statistics, window sums), made once for all the tests"""
    c = case(name)
    return [oracle_quartet(name, c["quartets"][qi], min_data, mode, a, b) for a, b in c["wins"]]


@functools.lru_cache(maxsize=None)
def freq_expect(name):
    """per window the oracle's groupFreqStats (populations of two haplotypes or more)"""
    return [orc.group_freq_stats(window_aln(name, a, b, True)) for a, b in case(name)["wins"]]


def freq_pops(name):
    lay = case(name)["lay"]
    return [p for p, s in zip(lay.sampleData.popNames, lay.pop_sizes) if s >= 2]


# ---- what a site is, by NumPy alone (tests/test_quartet_cases.py holds it against the oracle's sitesUsed) ------------------------
@functools.lru_cache(maxsize=None)
def quartet_counts(name, qi):
    """cnt [4][L][4], n [4][L]: base counts and called haplotypes of P1 .. P4 at every site"""
    c = case(name)
    cnt = np.zeros((4, c["L"], 4), dtype=np.int64)
    for k, pop in enumerate(c["quartets"][qi]):
        s, e = pop_range(c, pop)
        for b in range(4):
            cnt[k, :, b] = (c["gt"][:, s:e] == (1 << b)).sum(axis=1)
    return cnt, cnt.sum(axis=2)


@functools.lru_cache(maxsize=None)
def site_flags(name, qi, min_data, mode):
    """(good, used) per site: genomics.py:1655-1662 and the allele choice of 1672 / 1610-1615 in integers"""
    c = case(name)
    cnt, n = quartet_counts(name, qi)
    tot = cnt.sum(axis=0)
    good = (tot > 0).sum(axis=1) == 2
    for k, pop in enumerate(c["quartets"][qi]):
        s, e = pop_range(c, pop)
        good &= n[k] * 1. / (e - s) >= min_data
    if mode == "minor":
        return good, good.copy()
    absent = (tot > 0) & (cnt[3] == 0) & (n[3] > 0)[:, None]             # the allele that P4 does not have (0 / 0 == 0 is False)
    used = good & absent.any(axis=1)
    if mode == "fixed":
        der = absent.argmax(axis=1)
        for k in range(3):
            ck = np.take_along_axis(cnt[k], der[:, None], axis=1)[:, 0]
            used &= (n[k] > 0) & ((ck == 0) | (ck == n[k]))
    return good, used


def wave_share(name, qi, min_data, mode, chunk=0):
    """the used sites of each of the four waves of a block of k_abba_q in the whole-range window: a wave takes SPW consecutive sites
    of every 4 * SPW (SPW = 32, 16, 8 under NPASS 1, 2, 4; 16 under the quad layout of rows above 1024 slots)"""
    c = case(name)
    slots = c["lay"].n_hap
    spw = 32 if slots <= 256 else 16 if slots <= 512 else 8 if slots <= 1024 else 16
    _, used = site_flags(name, qi, min_data, mode)
    site = np.arange(4096 * chunk, min(c["L"], 4096 * (chunk + 1)))
    wave = ((site - 4096 * chunk) // spw) % 4
    return [int(used[site[wave == w]].sum()) for w in range(4)]


# ---- the tree-order comparison ----------------------------------------------------------------------------------------------------
NORTH_STAR = 1e-6


def order_bound(entry, value):
    """how far a statistic may lie from the oracle's `value` when the same per-site terms are added up in another order, or None where
    the pair (window, statistic) is left out.  Two float64 sums of the same n terms t_i differ by at most (n - 1) 2^-52 sum|t_i| (each
    is within (n - 1) 2^-53 sum|t_i| of the exact sum, whatever its order); for a ratio A / B that is, to first order,
    (dA + |A / B| dB) / |B|.  On top come 2 ulp of the oracle's value (its own division and the device's).  Left out: B == 0 exactly,
    a bound that is not finite (nan terms: 0 / 0 frequencies) or above 1e-6, the project's tolerance"""
    A, absA, B, absB, n = entry
    dA = max(n - 1, 0) * 2.0 ** -52 * absA
    if B is None:
        bound = dA
    else:
        if B == 0:
            return None
        dB = max(n - 1, 0) * 2.0 ** -52 * absB
        with np.errstate(all="ignore"):
            bound = (dA + abs(A / B) * dB) / abs(B)
    if not np.isfinite(bound) or not np.isfinite(value) or bound > NORTH_STAR:
        return None
    return float(bound + 2 * np.spacing(abs(np.float64(value))))


# ---- more than 65535 windows -----------------------------------------------------------------------------------------------------
def turn_windows():
    """(lo, hi, which): 65535 + 65 windows of case N cycled over 31 distinct ones below site 4000 (an empty one and one without a
    good site among them) and then over 10 from site 8000 on (one without a good site); `which` indexes `distinct`"""
    first = [(17 + 97 * k, 17 + 97 * k + (k * 37) % 257) for k in range(30)] + [(3000, 3000 + BLANK)]
    second = [(8000 + 83 * k, 8000 + 83 * k + 1 + (k * 53) % 256) for k in range(9)] + [(L_NARROW - BLANK, L_NARROW)]
    distinct = first + second
    which = np.concatenate([np.arange(65535) % len(first), len(first) + np.arange(65) % len(second)])
    lo = np.array([distinct[k][0] for k in which], dtype=np.int64)
    hi = np.array([distinct[k][1] for k in which], dtype=np.int64)
    return lo, hi, which, distinct
