"""-m gpu: the fused form of k_pack3 (csrc/pg_pair2.hip) where its word loop turns over.  The loop takes two words per trip with two
sets of row registers that change roles, steps each word's buffer descriptor from the one before (csrc/pg_pair_common.h: PgWordWalk),
and compacts the polymorphic sites of a wave's words eight and 32 entries at a time.  Hence: windows of an odd and an even number of
iterations, parts that end inside a word, windows of fewer than eight words; 0 .. 33 polymorphic sites in the words of ONE wave (every
wave compacts its own words: every eighth of the window), sites of three and four alleles among them; 129, 200 and 224 units, diploid
and per haplotype (PG_NO_DIP); a half-called genotype in the last word of the last window; windows cut into parts that meet by atomics;
rows that start beyond 2^31 bytes into the resident buffer.  Everything runs under PG_PACK_FUSE=1 (the fused form anywhere in its
domain) and is held against the oracle bit for bit: D, C, and pi / dxy / Fst with their sums in NumPy's order."""
import numpy as np
import pytest

from genomics_general_amd import synth
from genomics_general_amd.engine import Engine
from genomics_general_amd.samples import HapLayout, SampleData
from oracle import popgen_oracle as orc

import gpu_util as G

pytestmark = pytest.mark.gpu

PG_K_PAIRWISE = 1               # include/popgen_hip.h: the called-count kernel's timing family (no launch of it = the fused form ran)

# (name, ploidies, environment switch): units = individuals of an all-diploid layout, haplotypes otherwise and under PG_NO_DIP
UNITS = [
    ("dip129", [2] * 129, None), ("dip200", [2] * 200, None), ("dip224", [2] * 224, None),
    ("nodip129", [2] * 64 + [1], "PG_NO_DIP"), ("nodip200", [2] * 100, "PG_NO_DIP"), ("nodip224", [2] * 112, "PG_NO_DIP"),
]


def ploidy_layout(ploidies, n_pops=4):
    names = ["s%d" % i for i in range(len(ploidies))]
    per = len(names) // n_pops
    pops = [names[k * per:(k + 1) * per] for k in range(n_pops)]
    pops[-1] += names[n_pops * per:]
    sd = SampleData(indNames=list(names), popNames=["p%d" % k for k in range(n_pops)], popInds=pops, ploidyDict=dict(zip(names, ploidies)))
    return HapLayout(sd, names, "phased")


def individual_of_slot(ploidies):
    return np.repeat(np.arange(len(ploidies)), ploidies)


def random_rows(rng, L, ploidies):
    """one-hot codes: 60 % of the sites carry one allele, 30 % two, 6 % three and 4 % four (the first of them in four of five
    haplotypes); 10 % of the genotypes missing, per INDIVIDUAL: the diploid shortcut holds"""
    n_hap = int(np.sum(ploidies))
    n_all = rng.choice([1, 2, 3, 4], size=(L, 1), p=[0.6, 0.3, 0.06, 0.04])
    order = np.argsort(rng.random((L, 4)), axis=1)                                   # the site's alleles: the first n_all of a permutation
    pick = np.where(rng.random((L, n_hap)) < 0.8, 0, rng.integers(0, 4, size=(L, n_hap)) % n_all)
    codes = (1 << np.take_along_axis(order, pick, axis=1)).astype(np.int8)
    miss = (rng.random((L, len(ploidies))) < 0.1)[:, individual_of_slot(ploidies)]
    codes[miss] = 0
    return codes


def fused_engine(ploidies, env, codes, monkeypatch):
    if env:
        monkeypatch.setenv(env, "1")
    monkeypatch.setenv("PG_PACK_FUSE", "1")
    lay = ploidy_layout(ploidies)
    e = Engine(0)
    e.set_layout(lay)
    e.set_sum_order(1)              # the float64 sums in NumPy's order for every window: the oracle's, to the last bit
    if codes is not None:
        e.load_sites(codes)
    e.kernel_time_select(None)
    return e, lay


def check_against_oracle(e, lay, wins, rows_of, min_sites=1, min_data=0.01, fused=True):
    """D, C and pi / dxy / Fst of the windows, bit for bit; rows_of(a, b): the genotype codes of sites [a, b)"""
    lo, hi = [w[0] for w in wins], [w[1] for w in wins]
    e.kernel_time_reset()
    wb = e.batch(lo, hi)
    D, C = wb.pairCounts(reference_order=True)
    assert (e.kernel_time(PG_K_PAIRWISE)[1] == 0) == fused, "called-count launches: %d" % e.kernel_time(PG_K_PAIRWISE)[1]
    st = wb.groupDistStats(True, min_sites, min_data)
    for k, (a, b) in enumerate(wins):
        aln, _ = orc.aln_from_codes(rows_of(a, b), lay.hap_names, lay.hap_sample_name, lay.hap_group)
        Do, Co = orc.pair_counts_gemm(aln)
        assert np.array_equal(C[k], Co), "C differs from the oracle in window %d = [%d, %d)" % (k, a, b)
        assert np.array_equal(D[k], Do), "D differs from the oracle in window %d = [%d, %d)" % (k, a, b)
        so, _ = orc.group_dist_stats(aln, Do, Co, True, min_sites, min_data)
        for key, v in so.items():
            assert G.same(st[key][k], v), (key, k, (a, b), st[key][k], v)


@pytest.mark.parametrize("name,ploidies,env", UNITS)
def test_window_lengths_around_the_word_and_the_iteration(name, ploidies, env, monkeypatch):
    """1, 31, 32, 33 sites (one word, ending inside it or not), 255, 256, 257 (one iteration of eight words, two), 8 * 32 * k +- 1 for
    k = 2, 3, 8 (odd and even numbers of iterations: the loop leaves in the middle of a trip or at its end), from starts that are no
    multiple of anything; few and short windows: one part each"""
    rng = np.random.default_rng(4000 + len(ploidies))
    L = 7000
    codes = random_rows(rng, L, ploidies)
    e, lay = fused_engine(ploidies, env, codes, monkeypatch)
    lens = [1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 767, 769, 2047, 2049]
    wins, at = [], 3
    for n in lens:
        wins.append((at, at + n))
        at += n // 2 + 5            # (overlapping windows: fewer rows to hold)
    assert at + 2049 <= L
    wins.append((L - 257, L))       # the last rows of the buffer: the word requested ahead lies past it
    check_against_oracle(e, lay, wins, lambda a, b: codes[a:b])
    e.close()


def planted_window(rng, codes, start, ploidies, n_sites, multi, packed):
    """rows [start, start + 1280) = 40 words, all one allele except n_sites polymorphic sites, every one of them in a word that wave 0
    packs (words 0, 8, 16, 24, 32 of the window): packed = in row order from word 0 on, otherwise dealt over the five words.
    multi: the second site gets three alleles and the last one four (k alleles are k - 1 entries of the compaction)."""
    n_hap = codes.shape[1]
    ind = individual_of_slot(ploidies)
    block = codes[start:start + 1280]
    block[:] = 1
    block[(rng.random((1280, len(ploidies))) < 0.1)[:, ind]] = 0
    spots = [256 * (i // 32) + (i % 32) for i in range(160)] if packed else [256 * (i % 5) + (i // 5) for i in range(160)]
    for i in range(n_sites):
        row = block[spots[i]]
        n_all = 2
        if multi and i == 1:
            n_all = 3
        if multi and i == n_sites - 1 and n_sites >= 3:
            n_all = 4
        alleles = rng.permutation(4)[:n_all]
        pick = rng.integers(0, n_all, size=n_hap)
        pick[:n_all] = np.arange(n_all)                 # every allele is there
        new = (1 << alleles[pick]).astype(np.int8)
        row[:] = np.where(row != 0, new, 0)
        row[:n_all] = new[:n_all]                        # ... in a called genotype (the first slots: whole individuals)
        row[n_all:2 * ((n_all + 1) // 2)] = new[0]
    return (start, start + 1280)


@pytest.mark.parametrize("name,ploidies,env", UNITS)
def test_polymorphic_sites_at_the_compaction_edges(name, ploidies, env, monkeypatch):
    """0, 1, 7, 8, 9, 31, 32 and 33 polymorphic sites in the words of one wave: the 8-entry dword and the 32-entry word of its
    compaction end exactly, one short and one over; with sites of three and four alleles the same counts of sites give 2 .. 36 entries"""
    rng = np.random.default_rng(5000 + len(ploidies))
    cases = [(n, multi, packed) for n in (0, 1, 7, 8, 9, 31, 32, 33) for multi in (False, True) for packed in (False, True)
             if not (multi and n < 2) and (packed or n != 0)]
    codes = np.ones((1280 * len(cases) + 64, int(np.sum(ploidies))), dtype=np.int8)
    wins = [planted_window(rng, codes, 7 + 1280 * k, ploidies, n, multi, packed) for k, (n, multi, packed) in enumerate(cases)]
    e, lay = fused_engine(ploidies, env, codes, monkeypatch)
    check_against_oracle(e, lay, wins, lambda a, b: codes[a:b])
    # the same sites in the words of another wave, and the next window's first sites behind them: every third window, begun one word
    # earlier (every other one) and ended five words later
    shifted =[(a - 32 * (k % 2), b + 160) for k, (a, b) in enumerate(wins[1:-1], 1)][::3]
    check_against_oracle(e, lay, shifted, lambda a, b: codes[a:b])
    e.close()


@pytest.mark.parametrize("n_dip,fused_after", [(100, True), (129, False)])
def test_parts_with_atomics_and_a_half_called_genotype_in_the_last_word(n_dip, fused_after, monkeypatch):
    """three windows of about 20 000 sites: nine parts a window, whose counts meet by atomics, parts that end inside a word.  Then one
    allele of the last individual goes missing in the last word of the last window: the kernel's `bad` flag withdraws the diploid
    shortcut and the call runs again per haplotype (200 units: fused again; 258: the two kernels) -- the oracle's counts either way"""
    ploidies = [2] * n_dip
    rng = np.random.default_rng(6000 + n_dip)
    L = 60100
    codes = random_rows(rng, L, ploidies)
    e, lay = fused_engine(ploidies, None, codes, monkeypatch)
    wins = [(5, 20001), (20001, 40030), (40030, 60075)]
    check_against_oracle(e, lay, wins, lambda a, b: codes[a:b], min_sites=50)
    e.close()
    codes[60071, 2 * n_dip - 1] = 0
    codes[60071, 2 * n_dip - 2] = 4
    e, lay = fused_engine(ploidies, None, codes, monkeypatch)
    check_against_oracle(e, lay, wins, lambda a, b: codes[a:b], min_sites=50, fused=fused_after)
    e.close()


def test_rows_beyond_two_to_the_31_bytes_into_the_resident_buffer(monkeypatch):
    """224 diploids: 224 bytes a row; the last 3000 of 10 000 000 resident rows start 2.24 * 10^9 bytes in, where a 32-bit byte offset
    has wrapped: the descriptor's base is stepped in 64 bits"""
    n, tail = 10_000_000, 3000
    ploidies = [2] * 224
    e, lay = fused_engine(ploidies, None, None, monkeypatch)
    assert (n - tail) * (lay.n_hap // 2) > 1 << 31
    names = ["s%d" % i for i in range(len(ploidies))]
    e.reserve(n)
    e.synth_fill(n - tail, tail, 0, synth.SEED_DEFAULT, tail, len(ploidies), 4, G.slot_gen_hap(names, lay), synth.VAR_THR, synth.MISS_THR)
    rows = e.download(n - tail, tail)
    wins = [(n - tail, n), (n - 2000, n - 1743), (n - 513, n), (n - 1, n)]
    check_against_oracle(e, lay, wins, lambda a, b: rows[a - (n - tail):b - (n - tail)])
    e.close()
