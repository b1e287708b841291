// NumPy's order of a float64 sum, for the device finishers and, as plain host code, for the tests (tests/np_sum_main.cpp builds this
// file with g++ alone: it includes nothing of HIP).
#pragma once

#if defined(__HIPCC__)
#define PG_NP_SUM_FN __host__ __device__ inline
#else
#define PG_NP_SUM_FN inline
#endif

// float64 sum in the order NumPy's add.reduce visits a contiguous array, by one lane (k_hapstats: the reference's
// `(clusterFreq**2).sum()`, genomics.py:1088-1091; k_paint: np.nanmean of a population's distances): fewer than 8 elements left to
// right; up to 128 in eight strided partial sums combined as a tree, the tail added one by one; beyond that the range is halved (the
// first half rounded down to a multiple of 8), DEPTH times at most.  A half is at most 7 longer than half its parent, so a piece
// after k levels is shorter than n / 2^k + 7: DEPTH levels hold NumPy's order for every n up to 121 << DEPTH (2047 values take five
// levels, 2048 four); a longer array's last pieces would be summed as single runs, which NumPy would halve again.
// Both build lines carry -ffp-contract=off: no addition here may be fused with a product of the caller's.
template <int DEPTH>
PG_NP_SUM_FN double np_pairwise_sum(const double *a, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += a[i];
        return r;
    }
    if (n <= 128 || DEPTH == 0) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = a[j];
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += a[i + j];
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += a[i];
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum<(DEPTH > 0 ? DEPTH - 1 : 0)>(a, n2) + np_pairwise_sum<(DEPTH > 0 ? DEPTH - 1 : 0)>(a + n2, n - n2);
}

// The same order over values that are not stored: f(k) is element k of the flattened array, asked for exactly once (k_indpair_fin: the
// cells of an individual pair's haplotype block, a nan of the block as the 0.0 np.nanmean adds in its place).  A 26 x 26 block has 676
// values: DEPTH 3 holds up to 968.
template <int DEPTH, class F>
PG_NP_SUM_FN double np_pairwise_sum_of(F &f, int off, int n) {
    if (n < 8) {
        double r = 0.0;
        for (int i = 0; i < n; ++i) r += f(off + i);
        return r;
    }
    if (n <= 128 || DEPTH == 0) {
        double r[8];
        for (int j = 0; j < 8; ++j) r[j] = f(off + j);
        int i = 8;
        for (; i < n - (n % 8); i += 8)
            for (int j = 0; j < 8; ++j) r[j] += f(off + i + j);
        double res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
        for (; i < n; ++i) res += f(off + i);
        return res;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    return np_pairwise_sum_of<(DEPTH > 0 ? DEPTH - 1 : 0)>(f, off, n2) + np_pairwise_sum_of<(DEPTH > 0 ? DEPTH - 1 : 0)>(f, off + n2, n - n2);
}
