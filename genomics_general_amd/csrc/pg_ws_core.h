// The rules of the windowStats.py drop-in that the host route (pg_ws.cpp) and the device kernel (pg_ws_dev.hip: k_ws_stats) share:
// which spelling of a cell is converted in place and to what, the order-preserving key of a float64, the shape of NumPy's summation
// tree over a piece of values, one step of the radix select, and the finishing arithmetic of np.median, np.quantile (linear) and np.std.
// Plain code: g++ alone builds it (tests/ws_core_main.cpp), it includes nothing of HIP.  Every build line carries -ffp-contract=off:
// none of the expressions below may be fused.
#pragma once
#include <stdint.h>

#include "pg_np_sum.h"

#define PG_WS_FN PG_NP_SUM_FN

#define PG_WS_NSTAT 12                // mean median min max sd sum q5 q10 q25 q75 q90 q95, in this order everywhere
#define PG_WS_MEAN 0
#define PG_WS_MEDIAN 1
#define PG_WS_MIN 2
#define PG_WS_MAX 3
#define PG_WS_SD 4
#define PG_WS_SUM 5
#define PG_WS_Q0 6                    // the first of the six quantiles
#define PG_WS_NQ 6
#define PG_WS_PIECE 8192              // NumPy's add.reduce sums a contiguous array 8192 values at a time: ((p0 + p1) + p2) + ...
#define PG_WS_TREE_DEPTH 7            // a piece of 8192 values is halved seven times at most before every part holds 128 or fewer
#define PG_WS_MAX_LEAVES 192          // (a piece of up to 8192 values ends in 65 leaves at most; tests/ws_core_main.cpp aborts beyond)
#define PG_WS_NRANK (2 + 2 * PG_WS_NQ)   // the ranks asked of a sorted window: two for the median, two per quantile
#define PG_WS_ORDER_MASK (((1u << PG_WS_NQ) - 1u) << PG_WS_Q0 | 1u << PG_WS_MEDIAN)

// ---- a cell --------------------------------------------------------------------------------------------------------------------
// The regular spelling: [+-] digits [. digits] [e|E [+-] digits] with a digit on one side of the point at least, and `nan` in any
// case.  At most 15 significant digits behind the leading zeros and an effective decimal exponent of -22 .. 22: then the value is
// m * 10^e or m / 10^e with m and 10^e exact, ONE correctly rounded operation (Clinger's fast path), which is what float() returns.
// Everything else -- longer significands, larger exponents, inf, infinity, underscores, a sign in front of nan, blanks -- is irregular:
// returns false, and the caller converts the cell as NumPy does.
PG_WS_FN bool ws_cell(const unsigned char *s, int64_t n, double *out) {
    const double p10[23] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11,
                            1e12, 1e13, 1e14, 1e15, 1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22};
    if (n == 3 && (s[0] | 32) == 'n' && (s[1] | 32) == 'a' && (s[2] | 32) == 'n') {
        *out = __builtin_nan("");
        return true;
    }
    int64_t i = 0;
    bool neg = false;
    if (i < n && (s[i] == '+' || s[i] == '-')) neg = s[i++] == '-';
    uint64_t m = 0;
    int nd = 0, digits = 0;
    int64_t e10 = 0;
    for (; i < n && s[i] >= '0' && s[i] <= '9'; ++i, ++digits) {
        if (nd == 0 && s[i] == '0') continue;
        if (++nd > 15) return false;
        m = m * 10 + (uint64_t)(s[i] - '0');
    }
    if (i < n && s[i] == '.') {
        for (++i; i < n && s[i] >= '0' && s[i] <= '9'; ++i, ++digits) {
            --e10;
            if (nd == 0 && s[i] == '0') continue;
            if (++nd > 15) return false;
            m = m * 10 + (uint64_t)(s[i] - '0');
        }
    }
    if (digits == 0) return false;
    if (i < n && (s[i] | 32) == 'e') {
        ++i;
        bool eneg = false;
        if (i < n && (s[i] == '+' || s[i] == '-')) eneg = s[i++] == '-';
        int64_t e = 0;
        int ed = 0;
        for (; i < n && s[i] >= '0' && s[i] <= '9'; ++i, ++ed) {
            if (e > 100000) return false;
            e = e * 10 + (s[i] - '0');
        }
        if (ed == 0) return false;
        e10 += eneg ? -e : e;
    }
    if (i != n) return false;
    double v;
    if (m == 0)
        v = 0.0;
    else if (e10 < -22 || e10 > 22)
        return false;
    else
        v = e10 >= 0 ? (double)m * p10[e10] : (double)m / p10[-e10];
    *out = neg ? -v : v;
    return true;
}

// the bytes str.split() cuts at in ASCII text
PG_WS_FN bool ws_blank(unsigned char ch) { return ch == ' ' || (ch >= 9 && ch <= 13) || (ch >= 28 && ch <= 31); }

// ---- order --------------------------------------------------------------------------------------------------------------------
// float64 -> uint64 whose unsigned order is the order of the values (-inf lowest; -0.0 in front of 0.0) and back.  No nan comes here.
PG_WS_FN uint64_t ws_key(double x) {
    uint64_t b;
    __builtin_memcpy(&b, &x, 8);
    return (b >> 63) ? ~b : b | (1ull << 63);
}
PG_WS_FN double ws_unkey(uint64_t k) {
    const uint64_t b = (k >> 63) ? k & ~(1ull << 63) : ~k;
    double x;
    __builtin_memcpy(&x, &b, 8);
    return x;
}

// one step of the radix select: hist counts, per value of the byte looked at, the keys that agree with the prefix found so far; the
// bin that holds rank *rank (0-based among those keys), *rank made relative to that bin
PG_WS_FN int ws_radix_pick(const uint32_t *hist, uint64_t *rank) {
    uint64_t before = 0;
    int b = 0;
    for (; b < 255; ++b) {
        if (*rank < before + hist[b]) break;
        before += hist[b];
    }
    *rank -= before;
    return b;
}

// ---- NumPy's summation tree over a piece of n <= PG_WS_PIECE values --------------------------------------------------------------
// np_pairwise_sum (pg_np_sum.h) halves a run until its parts hold 128 values or fewer.  ws_tree_leaves lists those parts in order
// (k of them; a lane each sums one with np_pairwise_sum<0>), ws_tree_combine adds their sums in the recursion's order.
template <int D>
PG_WS_FN void ws_tree_leaves(int off, int n, int *offs, int *lens, int &k) {
    if (n <= 128 || D == 0) {
        offs[k] = off;
        lens[k] = n;
        ++k;
        return;
    }
    int n2 = n / 2;
    n2 -= n2 % 8;
    ws_tree_leaves<(D > 0 ? D - 1 : 0)>(off, n2, offs, lens, k);
    ws_tree_leaves<(D > 0 ? D - 1 : 0)>(off + n2, n - n2, offs, lens, k);
}
template <int D>
PG_WS_FN double ws_tree_combine(int n, const double *leaf, int &k) {
    if (n <= 128 || D == 0) return leaf[k++];
    int n2 = n / 2;
    n2 -= n2 % 8;
    const double l = ws_tree_combine<(D > 0 ? D - 1 : 0)>(n2, leaf, k);
    const double r = ws_tree_combine<(D > 0 ? D - 1 : 0)>(n - n2, leaf, k);
    return l + r;
}

// add.reduce over a contiguous array of any length, by one thread: the pieces left to right
PG_WS_FN double ws_np_sum(const double *a, int64_t n) {
    if (n <= 0) return 0.0;
    double s = 0.0;
    for (int64_t at = 0; at < n; at += PG_WS_PIECE) {
        const int m = (int)(n - at < PG_WS_PIECE ? n - at : PG_WS_PIECE);
        const double p = np_pairwise_sum<PG_WS_TREE_DEPTH>(a + at, m);
        s = at == 0 ? p : s + p;
    }
    return s;
}

// ---- finishing -----------------------------------------------------------------------------------------------------------------
// the quantiles of --stats q5 .. q95 as the reference spells them (windowStats.py:175-180)
PG_WS_FN double ws_quantile_of(int k) {
    const double q[PG_WS_NQ] = {0.05, 0.1, 0.25, 0.75, 0.9, 0.95};
    return q[k];
}

// np.quantile's linear method over n >= 1 sorted values (_function_base_impl.py: _quantile, _get_indexes, _get_gamma): the virtual
// index (n - 1) * q, its floor and the next rank; an index at or behind the last rank takes the last value twice, with the weight
// index + 1 that follows from the rank -1 NumPy writes for it
PG_WS_FN void ws_quantile_ranks(int64_t n, double q, int64_t *prev, int64_t *next, double *t) {
    const double v = (double)(n - 1) * q;
    if (v >= (double)(n - 1)) {
        *prev = *next = n - 1;
        *t = v + 1.0;
        return;
    }
    const double f = __builtin_floor(v);
    *prev = (int64_t)f;
    *next = *prev + 1;
    *t = v - f;
}
// _lerp: a + (b - a) * t, from the other end for t >= 0.5
PG_WS_FN double ws_lerp(double a, double b, double t) {
    const double d = b - a;
    const double up = d * t;
    double r = a + up;
    if (t >= 0.5) {
        const double down = d * (1.0 - t);
        r = b - down;
    }
    return r;
}
// np.median: the mean of the middle value, or of the two (their sum over 2.0)
PG_WS_FN void ws_median_ranks(int64_t n, int64_t *a, int64_t *b) {
    *b = n / 2;
    *a = n % 2 ? *b : *b - 1;
}
PG_WS_FN double ws_median(double a, double b, int64_t n) {
    if (n % 2) return b;
    const double s = a + b;
    return s / 2.0;
}
PG_WS_FN double ws_mean(double sum, int64_t n) { return sum / (double)n; }
// np.std: the deviations x - mean squared and summed in add.reduce's order (by the caller), over n, the root
PG_WS_FN double ws_dev2(double x, double mean) {
    const double d = x - mean;
    return d * d;
}
PG_WS_FN double ws_sd(double sum2, int64_t n) {
    const double var = sum2 / (double)n;
    return __builtin_sqrt(var);
}

// the ranks a window of n >= 1 values is asked for (those of the statistics in `mask`; -1 otherwise): [0], [1] the median's, then
// two per quantile
PG_WS_FN void ws_ranks(int64_t n, uint32_t mask, int64_t *rank, double *t) {
    for (int j = 0; j < PG_WS_NRANK; ++j) rank[j] = -1;
    if (mask & (1u << PG_WS_MEDIAN)) ws_median_ranks(n, &rank[0], &rank[1]);
    for (int k = 0; k < PG_WS_NQ; ++k)
        if (mask & (1u << (PG_WS_Q0 + k))) ws_quantile_ranks(n, ws_quantile_of(k), &rank[2 + 2 * k], &rank[3 + 2 * k], &t[k]);
}
// ... and the statistics from the values at those ranks
PG_WS_FN void ws_order_stats(int64_t n, uint32_t mask, const double *at_rank, const double *t, double *out) {
    if (mask & (1u << PG_WS_MEDIAN)) out[PG_WS_MEDIAN] = ws_median(at_rank[0], at_rank[1], n);
    for (int k = 0; k < PG_WS_NQ; ++k)
        if (mask & (1u << (PG_WS_Q0 + k))) out[PG_WS_Q0 + k] = ws_lerp(at_rank[2 + 2 * k], at_rank[3 + 2 * k], t[k]);
}
