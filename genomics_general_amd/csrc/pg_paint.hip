// distPaint.py's per-window decision on the device (distPaint.py:26-44, 62-87): for every window and individual, which reference
// population the individual is nearest to -- from the pair counts D (differences) and C (jointly called sites) that the pack and pair
// kernels leave in ctx->Dmat / ctx->Cmat, read in place.
//
//   k_paint   one wavefront per (window, individual), four to a block.
//     1. the quotients d = D / C of the individual against every reference individual (all populations laid end to end, duplicates
//        kept) go into LDS once: IEEE float64 divisions (this file is compiled like the others, without fast-math: equal quotients
//        decide ranks); nan where C < minSites or C == 0.  The pair matrices carry no diagonal: C of an individual with itself is its
//        own called count (k_hap_called), D is 0.
//     2. lane p forms np.nanmean of population p: nan as 0, the sum in NumPy's order for a contiguous 1-d array by the one-lane routine
//        k_hapstats uses (np_pairwise_sum, pg_np_sum.h), divided by the number of values that are not nan.
//     3. best = np.argmin(means): the first nan if there is one, else the first minimum.
//     4. test mode: for every other population q without a nan on either side, the doubled rank sum of the best population's values
//        among both lists, 2 s = sum_a (1 + 2 #{v < d_a} + #{v == d_a}) (average ranks; the count of equals includes d_a), as integer
//        counts by lanes striding over a and a reduction across the wave, against crit[best][q]: the largest 2 s whose p-value is
//        <= p_threshold for the two sizes (the host's table; -1: none).  Integer and exact.  One comparison above its limit: noresult.
//        delta mode: no nan among the means: noresult if (second smallest - smallest) < delta, else best.  A nan among them: Python's
//        sorted() of such a list depends on its order, so the cell is appended to a list (cell index, its means) and the host
//        finishes it with sorted() itself.
#include "pg_ctx.h"
#include "pg_wave.h"

#include <algorithm>
#include <vector>

#define PAINT_WAVES 4
#define PAINT_MAX_REFS 2048     // reference individuals over all populations: 4 waves x 2048 quotients = 64 KB of LDS
#define PAINT_MAX_POPS 64       // one lane per population

namespace {

__device__ __forceinline__ double paint_nan() { return __longlong_as_double(0x7ff8000000000000ll); }

__global__ __launch_bounds__(64 * PAINT_WAVES) void k_paint(const int32_t *__restrict__ Cmat, const int32_t *__restrict__ Dmat, int N, int cN,
                                                            int cshift, const unsigned long long *__restrict__ called, int n_ind,
                                                            const int32_t *__restrict__ ind_slot, int n_pops,
                                                            const int32_t *__restrict__ ref_start, const int32_t *__restrict__ ref_slot,
                                                            int min_sites, int mode, const long long *__restrict__ crit, double delta,
                                                            int noresult, int32_t *__restrict__ out, long long cell0,
                                                            unsigned long long *__restrict__ n_flagged, long long *__restrict__ flag_cell,
                                                            double *__restrict__ flag_means) {
    extern __shared__ __attribute__((aligned(16))) double paint_lds[];      // [PAINT_WAVES][R] quotients; no static LDS beside it
    const int R = ref_start[n_pops];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int win = blockIdx.y, k = blockIdx.x * PAINT_WAVES + wave;
    const bool live = k < n_ind;                                  // (a wave past the last individual still meets the barriers)
    double *q = paint_lds + (size_t)wave * R;
    const int32_t *Cw = Cmat + (size_t)win * cN * cN, *Dw = Dmat + (size_t)win * N * N;
    const int thr = min_sites > 1 ? min_sites : 1;
    if (live) {
        const int i = ind_slot[k];
        for (int r = lane; r < R; r += 64) {
            const int j = ref_slot[r];
            long long cv, dv;
            if (i == j) {
                cv = (long long)called[(size_t)win * N + i];
                dv = 0;
            } else {
                const int a = i < j ? i : j, b = i < j ? j : i;      // the pair kernels store the upper triangles
                cv = Cw[(size_t)(a >> cshift) * cN + (b >> cshift)];
                dv = Dw[(size_t)a * N + b];
            }
            q[r] = cv >= thr ? (double)dv / (double)cv : paint_nan();
        }
    }
    __syncthreads();
    if (!live) return;                                            // (no barrier below this line)
    // lane p: np.nanmean of population p and whether it holds a nan
    double mean = 0.0;
    bool has_nan = false;
    if (lane < n_pops) {
        const int s = ref_start[lane], n = ref_start[lane + 1] - s;
        // np.nanmean: nan as 0 (written back into the lane's own segment: a list with a nan is never ranked below), the sum in
        // NumPy's order (np_pairwise_sum, pg_np_sum.h: at most PAINT_MAX_REFS = 2048 values, which take up to five levels of halves --
        // 2047 does, 2048 takes four --; the depth of 6 holds the order up to 121 << 6 values), over the values that are not nan
        int cnt = 0;
        for (int t = 0; t < n; ++t) {
            if (q[s + t] == q[s + t]) ++cnt;
            else q[s + t] = 0.0;
        }
        has_nan = cnt < n;
        mean = cnt > 0 ? np_pairwise_sum<6>(q + s, n) / (double)cnt : paint_nan();
    }
    const unsigned long long nan_lists = __ballot(has_nan);
    // np.argmin: the first nan, else the first minimum
    int best = 0;
    double m0 = __shfl(mean, 0, 64);
    bool any_nan_mean = m0 != m0;
    for (int p = 1; p < n_pops; ++p) {
        const double m = __shfl(mean, p, 64);
        if (m != m) {
            if (!any_nan_mean) { best = p; m0 = m; }
            any_nan_mean = true;
        } else if (!any_nan_mean && m < m0) {
            best = p;
            m0 = m;
        }
    }
    int result = best;
    if (mode == 0) {
        const int bs = ref_start[best], nb = ref_start[best + 1] - bs;
        for (int p = 0; p < n_pops; ++p) {
            if (p == best || ((nan_lists >> best) & 1ull) || ((nan_lists >> p) & 1ull)) continue;   // (a nan p-value never rejects)
            const long long limit = crit[(size_t)best * n_pops + p];
            const int ps = ref_start[p], np_ = ref_start[p + 1] - ps;
            long long twice_s = 0;
            for (int a = lane; a < nb; a += 64) {
                const double da = q[bs + a];
                int less = 0, eq = 0;
                for (int t = 0; t < nb; ++t) {                    // (every lane reads the same word: an LDS broadcast)
                    const double v = q[bs + t];
                    less += v < da ? 1 : 0;
                    eq += v == da ? 1 : 0;
                }
                for (int t = 0; t < np_; ++t) {
                    const double v = q[ps + t];
                    less += v < da ? 1 : 0;
                    eq += v == da ? 1 : 0;
                }
                twice_s += 1 + 2 * (long long)less + eq;
            }
            twice_s = pg_wave_sum(twice_s);
            if (twice_s > limit) {                                // (limit -1: no rank sum of these sizes reaches the threshold)
                result = noresult;
                break;
            }
        }
    } else if (any_nan_mean) {
        // the host's: Python's sorted() of a list with a nan depends on the list's order
        unsigned long long at = 0;
        if (lane == 0) {
            at = atomicAdd(n_flagged, 1ull);
            flag_cell[at] = cell0 + (long long)win * n_ind + k;
        }
        at = __shfl(at, 0, 64);
        if (lane < n_pops) flag_means[at * (unsigned long long)n_pops + lane] = mean;
    } else {
        double m1 = 0.0;
        bool have = false;
        for (int p = 0; p < n_pops; ++p) {
            const double m = __shfl(mean, p, 64);
            if (p != best && (!have || m < m1)) { m1 = m; have = true; }
        }
        if (m1 - m0 < delta) result = noresult;
    }
    if (lane == 0) out[(size_t)win * n_ind + k] = result;
}

}  // namespace

extern "C" int pg_paint(pg_ctx *c, const int64_t *lo, const int64_t *hi, int n_win, int n_ind, const int32_t *ind_slot, int n_pops,
                        const int32_t *ref_start, const int32_t *ref_slot, int min_sites, int mode, const int64_t *crit, double delta,
                        int noresult, int32_t *decision_out, int64_t *n_flagged_out, int64_t *flag_cell_out, double *flag_means_out) {
    if (!c) return pg_fail(PG_ERR_ARG, "null ctx");
    if (c->n_hap <= 0) return pg_fail(PG_ERR_STATE, "pg_set_samples must be called first");
    if (n_flagged_out) *n_flagged_out = 0;
    // (the two haplotypes of a diploid individual would meet on C's diagonal, which the pair kernels do not store)
    if (c->n_samp != c->n_hap) return pg_fail(PG_ERR_STATE, "pg_paint: every sample must be haploid (%d samples, %d haplotypes)", c->n_samp, c->n_hap);
    if (mode != 0 && mode != 1) return pg_fail(PG_ERR_ARG, "pg_paint: mode %d (0 = rank-sum test, 1 = delta)", mode);
    if (n_ind < 1 || !ind_slot || !ref_start || !ref_slot) return pg_fail(PG_ERR_ARG, "pg_paint: null or empty sample arguments");
    if (n_pops < 1 || n_pops > PAINT_MAX_POPS) return pg_fail(PG_ERR_ARG, "pg_paint: %d reference populations (1 .. %d)", n_pops, PAINT_MAX_POPS);
    if (mode == 1 && n_pops < 2) return pg_fail(PG_ERR_ARG, "pg_paint: the delta mode needs two populations");
    if (mode == 0 && !crit) return pg_fail(PG_ERR_ARG, "pg_paint: the test mode needs the table of critical rank sums");
    if (mode == 1 && (!n_flagged_out || !flag_cell_out || !flag_means_out)) return pg_fail(PG_ERR_ARG, "pg_paint: the delta mode needs the arrays of the cells left to the host");
    if (ref_start[0] != 0) return pg_fail(PG_ERR_ARG, "pg_paint: ref_start[0] != 0");
    for (int p = 0; p < n_pops; ++p)
        if (ref_start[p + 1] <= ref_start[p]) return pg_fail(PG_ERR_ARG, "pg_paint: reference population %d has no individuals", p);
    const int R = ref_start[n_pops];
    if (R > PAINT_MAX_REFS) return pg_fail(PG_ERR_ARG, "pg_paint: %d reference individuals (at most %d)", R, PAINT_MAX_REFS);
    for (int r = 0; r < R; ++r)
        if (ref_slot[r] < 0 || ref_slot[r] >= c->n_hap) return pg_fail(PG_ERR_ARG, "pg_paint: reference slot %d outside 0 .. %d", ref_slot[r], c->n_hap - 1);
    for (int k = 0; k < n_ind; ++k)
        if (ind_slot[k] < 0 || ind_slot[k] >= c->n_hap) return pg_fail(PG_ERR_ARG, "pg_paint: individual slot %d outside 0 .. %d", ind_slot[k], c->n_hap - 1);
    if (n_win < 0) return pg_fail(PG_ERR_ARG, "negative window count");
    if (n_win == 0) return PG_OK;
    if (!decision_out) return pg_fail(PG_ERR_ARG, "null output");
    HIPCHK(hipSetDevice(c->device));
    pg_ctx::Paint &P = c->paint;
    int rc;
    {
        std::vector<int32_t> tab((size_t)n_ind + n_pops + 1 + R);
        std::copy(ind_slot, ind_slot + n_ind, tab.begin());
        std::copy(ref_start, ref_start + n_pops + 1, tab.begin() + n_ind);
        std::copy(ref_slot, ref_slot + R, tab.begin() + n_ind + n_pops + 1);
        if ((rc = P.tab.ensure(tab.size())) != PG_OK) return rc;
        HIPCHK(hipMemcpy(P.tab.p, tab.data(), tab.size() * 4, hipMemcpyHostToDevice));                 // (pageable source: a synchronous copy)
        if ((rc = P.crit.ensure((size_t)n_pops * n_pops)) != PG_OK) return rc;
        if (mode == 0) HIPCHK(hipMemcpy(P.crit.p, crit, (size_t)n_pops * n_pops * 8, hipMemcpyHostToDevice));
    }
    const int32_t *d_ind = P.tab.p, *d_start = P.tab.p + n_ind, *d_ref = P.tab.p + n_ind + n_pops + 1;
    const size_t cells = (size_t)n_win * n_ind;
    if ((rc = P.count.ensure(1)) != PG_OK) return rc;
    if (mode == 1) {
        if ((rc = P.cell.ensure(cells)) != PG_OK) return rc;
        if ((rc = P.means.ensure(cells * n_pops)) != PG_OK) return rc;
    }
    const size_t lds = (size_t)PAINT_WAVES * R * sizeof(double);
    rc = pg_pairwise_each(c, lo, hi, n_win, [&](int w0, int nb) -> int {
        int r;
        // (a pass that the pack kernels' flag makes start over begins at window 0 again: so does the list)
        if (w0 == 0) HIPCHK(hipMemsetAsync(P.count.p, 0, 8, c->stream));
        if ((r = P.out.ensure((size_t)nb * n_ind)) != PG_OK) return r;
        if ((r = c->res_i64.ensure((size_t)nb * c->n_hap)) != PG_OK) return r;
        int64_t max_len = 0;
        for (int w = w0; w < w0 + nb; ++w) max_len = std::max(max_len, hi[w] - lo[w]);
        hipEvent_t e0, e1;
        if ((r = pg_time_begin(c, PG_K_PAINT_CALLED, &e0, &e1)) != PG_OK) return r;
        HIPCHK(hipMemsetAsync(c->res_i64.p, 0, (size_t)nb * c->n_hap * 8, c->stream));
        pg_launch_hap_called(c->stream, c->gt.p, c->RS, c->n_hap, c->cur_win_lo, c->cur_win_hi, nb,
                             (int)((max_len + PG_SITES_PER_BLOCK - 1) / PG_SITES_PER_BLOCK), reinterpret_cast<unsigned long long *>(c->res_i64.p));
        if ((r = pg_time_end(c, PG_K_PAINT_CALLED, e0, e1, 1)) != PG_OK) return r;
        HIPCHK(hipGetLastError());
        if ((r = pg_time_begin(c, PG_K_PAINT, &e0, &e1)) != PG_OK) return r;
        hipLaunchKernelGGL(k_paint, dim3((n_ind + PAINT_WAVES - 1) / PAINT_WAVES, nb), dim3(64 * PAINT_WAVES), lds, c->stream, c->Cmat.p, c->Dmat.p,
                           c->n_hap, c->cN, c->cshift, reinterpret_cast<const unsigned long long *>(c->res_i64.p), n_ind, d_ind, n_pops, d_start, d_ref,
                           min_sites, mode, reinterpret_cast<const long long *>(P.crit.p), delta, noresult, P.out.p, (long long)w0 * n_ind,
                           reinterpret_cast<unsigned long long *>(P.count.p), reinterpret_cast<long long *>(P.cell.p), P.means.p);
        if ((r = pg_time_end(c, PG_K_PAINT, e0, e1, 1)) != PG_OK) return r;
        HIPCHK(hipGetLastError());
        HIPCHK(hipMemcpyAsync(decision_out + (size_t)w0 * n_ind, P.out.p, (size_t)nb * n_ind * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        return PG_OK;
    });
    if (rc != PG_OK) return rc;
    if (mode == 1) {
        int64_t n = 0;
        HIPCHK(hipMemcpy(&n, P.count.p, 8, hipMemcpyDeviceToHost));
        if (n < 0 || (size_t)n > cells) return pg_fail(PG_ERR_STATE, "pg_paint: %lld cells left to the host of %zu", (long long)n, cells);
        if (n > 0) {
            HIPCHK(hipMemcpy(flag_cell_out, P.cell.p, (size_t)n * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(flag_means_out, P.means.p, (size_t)n * n_pops * 8, hipMemcpyDeviceToHost));
        }
        *n_flagged_out = n;
    }
    return PG_OK;
}
