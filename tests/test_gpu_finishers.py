"""-m gpu: the float finishers behind the pair counts -- k_hapstats (WindowBatch.H12stats) and k_sample_het (WindowBatch.sampleHet) --
against the oracle, bit for bit (gpu_util.same: nan equals nan), on the cases of tests/finisher_cases.py: populations on both
sides of the 32-bit mask word and of the 256 threads of the row loop, cluster counts in every range of np_pairwise_sum
(csrc/pg_np_sum.h), tied rows far apart, every state of the cached matrix and maxDist -1, 0 and 0.01; a pass cut into sub-batches
under the smallest scratch limit (the w0 > 0 offsets of both kernels' outputs and of k_hapstats' bit rows); a pass that starts over.
tests/test_finisher_cases.py shows without a GPU that the cases contain all this.  The expectations are the oracle's alone."""
import numpy as np
import pytest

import finisher_cases as FC
import gpu_util as G
from genomics_general_amd import _lib
from oracle import popgen_oracle as orc

pytestmark = pytest.mark.gpu


def engine_of(case):
    e = G.Engine(0)
    e.set_layout(case["lay"])
    e.load_sites(case["gt"])
    return e


def into_state(wb, state, min_sites=FC.HAP_MIN_SITES):
    """the calls of the reference's worker that leave the cached matrix in that state"""
    if state == "popdist":
        wb.groupDistStats(False, min_sites, 0.01)
    elif state == "indpair":
        wb.indPairTable(includeSameWithSame=False, first="name")        # (indPairDists without its dictionary of a million views)


def assert_h12(name, state, max_dist, h):
    lay = FC.hap_case(name)["lay"]
    for w, want in enumerate(FC.hap_expect(name, state, max_dist)):
        for p in lay.sampleData.popNames:
            for st in ("H1_", "H12_", "H2_"):
                assert G.same(h[st + p][w], want[st + p]), (name, state, max_dist, st + p, w, h[st + p][w], want[st + p])


def assert_het(name, state, het):
    lay = FC.hap_case(name)["lay"]
    values = 0
    for w, (aln, D, C) in enumerate(FC.hap_counts(name)):
        want = orc.sample_het(aln, FC.cached_dist(aln, D, C, state), C)
        for nm in lay.ind_order:
            assert G.same(het[nm][w], want["het_" + nm]), (name, state, nm, w, het[nm][w], want["het_" + nm])
            values += not np.isnan(want["het_" + nm])
    return values


@pytest.mark.parametrize("state", FC.HAP_STATES)
@pytest.mark.parametrize("name", ["Hs", "Hd", "Dd", "DdN"])
def test_h12_and_sample_het_equal_the_oracle_bit_for_bit(name, state):
    e = engine_of(FC.hap_case(name))
    try:
        c = FC.hap_case(name)
        wb = e.batch(c["lo"], c["hi"])
        into_state(wb, state)
        values = assert_het(name, state, wb.sampleHet())
        assert (values > 0) == (name in ("Dd", "DdN"))                  # (haploid individuals have no value)
        for max_dist in FC.HAP_MAX_DISTS:
            assert_h12(name, state, max_dist, wb.H12stats(max_dist))
    finally:
        e.close()


@pytest.mark.parametrize("state", ["plain", "popdist"])
def test_h12_in_sub_batches_under_a_scratch_limit(state):
    """layout Hs under 64 MiB of scratch, the smallest limit: 8 MB of matrices per window, batches of at most four of the 13 windows;
    the empty and the one-site window stand in later batches.  k_hapstats writes window w0 + k of a batch to row k of its bit rows
    and of its result table; the host puts the table at w0"""
    c = FC.hap_case("Hs")
    e = engine_of(c)
    try:
        e.set_scratch_limit(64 << 20)
        e.kernel_time_select(None)
        wb = e.batch(c["lo"], c["hi"])
        into_state(wb, state)
        for max_dist in (0, 0.01):
            e.kernel_time_reset()
            h = wb.H12stats(max_dist)
            launches = e.kernel_time(_lib.K_PACK)[1]
            print("pack launches:", launches)
            assert launches >= 3, launches
            assert_h12("Hs", state, max_dist, h)
    finally:
        e.close()


def test_h12_and_sample_het_across_a_pass_that_starts_over():
    """layout X4, four alleles at nearly every site, on fresh engines: the first pass overflows the default reservation of virtual
    sites and every batch is run again; the second identical call packs half as often, which shows that the first was repeated"""
    c = FC.hap_case("X4")
    for what in ("h12", "het"):
        e = engine_of(c)
        try:
            e.kernel_time_select(None)
            launches = []
            for _ in range(2):
                e.kernel_time_reset()
                wb = e.batch(c["lo"], c["hi"])
                if what == "h12":
                    assert_h12("X4", "plain", 0.01, wb.H12stats(0.01))
                else:
                    assert assert_het("X4", "plain", wb.sampleHet()) > 50
                launches.append(e.kernel_time(_lib.K_PACK)[1])
            print(what, "pack launches:", launches)
            assert launches[1] >= 1 and launches[0] == 2 * launches[1], launches
        finally:
            e.close()


def assert_ind_het(sub, masked, het):
    lay = FC.het_case()["lay"]
    values = 0
    for w, (want, _) in enumerate(FC.het_expect(sub, masked)):
        for nm in lay.ind_order:
            assert G.same(het[nm][w], want["het_" + nm]), (sub, masked, nm, w, het[nm][w], want["het_" + nm])
            values += not np.isnan(want["het_" + nm])
    return values


@pytest.mark.parametrize("masked", [False, True])
def test_sample_het_with_mixed_ploidy_over_three_blocks(masked):
    """90 samples of ploidy 1 .. 4 over 7 windows: 630 threads, the third block partly filled; a value for the diploids alone"""
    c = FC.het_case()
    e = engine_of(c)
    try:
        wb = e.batch(c["lo"], c["hi"])
        if masked:
            into_state(wb, "popdist", FC.HET_MIN_SITES)
        assert assert_ind_het(False, masked, wb.sampleHet()) > 20
    finally:
        e.close()


def test_sample_het_in_sub_batches_under_a_scratch_limit():
    """the same rows under 400 short windows and 64 MiB of scratch: three batches, the result table of each at its w0"""
    c = FC.het_case()
    e = engine_of(c)
    try:
        e.set_scratch_limit(64 << 20)
        e.kernel_time_select(None)
        wb = e.batch(c["sub_lo"], c["sub_hi"])
        into_state(wb, "popdist", FC.HET_SUB_MIN_SITES)
        e.kernel_time_reset()
        het = wb.sampleHet()
        launches = e.kernel_time(_lib.K_PACK)[1]
        print("pack launches:", launches)
        assert launches >= 3, launches
        assert assert_ind_het(True, True, het) > 1000
    finally:
        e.close()
