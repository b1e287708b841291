// Site-frequency spectra (the sfs.py drop-in, cli.sfs_main): per site the count of a target allele in every ingroup population,
// then one cell of every spectrum group (a mixed-radix index over the group's populations) gets `count += 1` per interval that
// holds the site and `first = min(first, line ordinal)`.
//
//   k_sfs_rows     resident rows: base counts per population (range_counts), completeness of the ingroup, target allele, scatter
//   k_sfs_base     uploaded int32 [n][n_cols][4] base counts (a freq.py table): target allele, scatter
//   k_sfs_target   uploaded int32 [n][n_in] target counts: scatter
//   k_sfs_compact  the touched cells of the dense tables, appended to a list (two passes: count, fill)
//
// The scatter is a histogram in which most sites hit one cell (the monomorphic one), so no thread adds to memory by itself:
//   * groups whose table (cells x (intervals + 1) words) fits the block's LDS budget are counted in u32 LDS tables and flushed to the
//     global u64 tables once per block; inside a wave the lanes that hold the first active lane's cell are added as one (ballot),
//     the others add to LDS one by one;
//   * the other groups go to global memory with full aggregation inside the wave: loop over the distinct cells present, the lowest
//     lane of each adds the lane count and takes the minimum ordinal (the ordinals rise with the lane, so that is its own).
// Integer atomics only: the result does not depend on the order of arrival.
#include "pg_ctx.h"
#include "pg_range_counts.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>

#define SFS_BLOCK 256
#define SFS_MAX_DIM 4
#define SFS_MAX_IN 32          // ingroup populations (their target counts of a block's 256 sites sit in LDS: 32 KiB at most)
#define SFS_LDS_WORDS 8192     // u32 words of LDS tables per block (32 KiB; with the target counts 64 KiB at most: DESIGN.md)
#define SFS_NONE 0xFFFFFFFFFFFFFFFFull

struct SfsGroup {
    int32_t nd;
    int32_t pop[SFS_MAX_DIM];   // indices into the ingroup list
    int32_t ext[SFS_MAX_DIM];
    int32_t lds_off;            // first word of the group's LDS table (counts [cells][NI], then first [cells]); -1: global route
    int64_t base;               // first cell of the group in the global tables
    int64_t cells;
};

struct SfsArgs {
    const SfsGroup *groups;
    int32_t n_groups, n_in, NI, has_iv;
    int32_t lds_words;
    int32_t pop_ext[SFS_MAX_IN];
    unsigned long long *count;  // [total cells][NI]
    unsigned long long *first;  // [total cells]
    // membership (has_iv): per row its scaffold run and position, per run a list of (start, end, interval id); a run without a
    // list takes no part (contigs left out by --include / --exclude, scaffolds without a region)
    const int32_t *row_run;
    const int64_t *pos;
    const int32_t *run_off;
    const int64_t *iv_start, *iv_end;
    const int32_t *iv_id;
    unsigned long long ord0;    // line ordinal of row 0 of this launch
    int64_t n;
    int32_t *flag;              // raised by a count that is negative or beyond its population's extent
};

// ---- the target allele (sfs.py:60-85), shared by the resident rows and the baseCounts tables; host-callable for the tests ----
// tot: the ingroup's totals; out: the outgroup's counts (has_out).  Returns the base, or -1 for a site that is left out.
// Unpolarised: totalBaseCounts.argsort()[-2] over all four totals -- NumPy's small-array argsort is not stable, so the permutation
// comes from the table pgf_order uses (PGF_ARGSORT4, pg_filter_core.h), keyed by the number of smaller values per element.
__host__ __device__ inline int sfs_target_base(const long long tot[4], const long long out[4], int has_out) {
    int n_all = 0, n_out = 0;
    for (int b = 0; b < 4; ++b) {
        const bool o = has_out && out[b] > 0;
        n_all += (tot[b] > 0 || o) ? 1 : 0;
        n_out += o ? 1 : 0;
    }
    if (n_all < 1 || n_all > 2) return -1;
    if (has_out) {
        if (n_out == 0 || (1 & n_out) != 1) return -1;         // `outgroupMono & nOutAlleles != 1` binds as (True & nOut) != 1
        for (int b = 0; b < 4; ++b)
            if (!(out[b] > 0) && tot[b] > 0) return b;
        for (int b = 0; b < 4; ++b)
            if (!(tot[b] > 0)) return b;                        // invariant site: the first absent base, which counts 0
        return -1;
    }
    int key = 0;
    for (int i = 0; i < 4; ++i) {
        int below = 0;
        for (int j = 0; j < 4; ++j) below += tot[j] < tot[i] ? 1 : 0;
        key |= below << (2 * i);
    }
    return (PGF_ARGSORT4[key] >> 4) & 3;                        // argsort()[-2]
}

extern "C" int pg_sfs_target_base(const int64_t *tot4, const int64_t *out4, int *base_out) {
    if (!tot4 || !base_out) return pg_fail(PG_ERR_ARG, "pg_sfs_target_base: null argument");
    long long t[4], o[4] = {0, 0, 0, 0};
    for (int b = 0; b < 4; ++b) {
        t[b] = tot4[b];
        if (out4) o[b] = out4[b];
    }
    *base_out = sfs_target_base(t, o, out4 ? 1 : 0);
    return PG_OK;
}

// ---- the scatter -------------------------------------------------------------------------------------------
__device__ __forceinline__ bool sfs_in(const SfsArgs &A, int j, int64_t p) { return A.iv_start[j] <= p && p <= A.iv_end[j]; }

__device__ __forceinline__ unsigned long long sfs_shfl64(unsigned long long v, int src) {
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((unsigned long long)hi << 32) | lo;
}

// every lane of the block calls this, converged (`valid` says whether the lane holds a site); i = the lane's row in the launch
// (consecutive over the lanes of a wave); t = the lane's target counts in LDS, t[k * SFS_BLOCK]
__device__ __forceinline__ void sfs_scatter(const SfsArgs &A, uint32_t *tab, const uint32_t *t, bool valid, int64_t i) {
    const int lane = threadIdx.x & 63;
    int j = 0, je = 0;
    int64_t p = 0;
    if (A.has_iv) {
        if (valid) {
            const int r = A.row_run[i];
            j = A.run_off[r];
            je = A.run_off[r + 1];
            p = A.pos[i];
            while (j < je && !sfs_in(A, j, p)) ++j;
        }
        valid = valid && j < je;                                // in no interval: the site is skipped
    }
    const int NI = A.NI;
    for (int g = 0; g < A.n_groups; ++g) {
        const SfsGroup &G = A.groups[g];
        unsigned long long cell = 0;
        if (valid)
            for (int d = 0; d < G.nd; ++d) cell = cell * (unsigned long long)G.ext[d] + t[G.pop[d] * SFS_BLOCK];
        if (G.lds_off >= 0) {
            uint32_t *cnt = tab + G.lds_off, *fst = cnt + G.cells * NI;
            const uint32_t key = (uint32_t)cell, rel = (uint32_t)i;
            bool act = valid, need_min = valid;
            const unsigned long long m = __ballot(act);
            if (m) {                                            // the first active lane's cell, for every lane that holds it
                const int leader = __ffsll((long long)m) - 1;
                const uint32_t k0 = (uint32_t)__shfl((int)key, leader);
                const bool same = act && key == k0;
                const unsigned long long ms = __ballot(same);
                if (lane == leader) {
                    if (!A.has_iv) atomicAdd(&cnt[(size_t)k0 * NI], (uint32_t)__popcll(ms));
                    atomicMin(&fst[k0], rel);                   // the lowest lane of the set: the lowest ordinal
                }
                need_min = act && !same;
                if (!A.has_iv) act = need_min;
            }
            if (need_min) atomicMin(&fst[key], rel);
            if (act) {
                if (!A.has_iv) atomicAdd(&cnt[(size_t)key * NI], 1u);
                else
                    for (int jj = j; jj < je; ++jj)
                        if (sfs_in(A, jj, p)) atomicAdd(&cnt[(size_t)key * NI + A.iv_id[jj]], 1u);
            }
        } else {
            // global route: one atomic per distinct cell of the wave
            const unsigned long long gcell = (unsigned long long)G.base + cell, ord = A.ord0 + (unsigned long long)i;
            bool act = valid;
            for (;;) {
                const unsigned long long m = __ballot(act);
                if (!m) break;
                const int leader = __ffsll((long long)m) - 1;
                const unsigned long long k0 = sfs_shfl64(gcell, leader);
                const bool same = act && gcell == k0;
                const unsigned long long ms = __ballot(same);
                if (lane == leader) {
                    if (!A.has_iv) atomicAdd(&A.count[k0 * NI], (unsigned long long)__popcll(ms));
                    atomicMin(&A.first[k0], ord);               // the lowest lane of the set: the lowest ordinal
                }
                act = act && !same;
            }
            if (A.has_iv) {
                // the lanes walk their interval lists in step; per step the (cell, interval) pairs present are added as above
                int jj = j;
                bool more = valid;
                while (__ballot(more)) {
                    const unsigned long long key = more ? gcell * NI + A.iv_id[jj] : 0ull;
                    bool a2 = more;
                    for (;;) {
                        const unsigned long long m = __ballot(a2);
                        if (!m) break;
                        const int leader = __ffsll((long long)m) - 1;
                        const unsigned long long k0 = sfs_shfl64(key, leader);
                        const bool same = a2 && key == k0;
                        const unsigned long long ms = __ballot(same);
                        if (lane == leader) atomicAdd(&A.count[k0], (unsigned long long)__popcll(ms));
                        a2 = a2 && !same;
                    }
                    if (more) {
                        ++jj;
                        while (jj < je && !sfs_in(A, jj, p)) ++jj;
                        more = jj < je;
                    }
                }
            }
        }
    }
}

__device__ __forceinline__ void sfs_tables_init(const SfsArgs &A, uint32_t *tab) {
    for (int g = 0; g < A.n_groups; ++g) {
        const SfsGroup &G = A.groups[g];
        if (G.lds_off < 0) continue;
        const int nc = (int)G.cells * A.NI, nw = nc + (int)G.cells;
        for (int w = threadIdx.x; w < nw; w += SFS_BLOCK) tab[G.lds_off + w] = w < nc ? 0u : 0xFFFFFFFFu;
    }
    __syncthreads();
}

__device__ __forceinline__ void sfs_tables_flush(const SfsArgs &A, const uint32_t *tab) {
    __syncthreads();
    for (int g = 0; g < A.n_groups; ++g) {
        const SfsGroup &G = A.groups[g];
        if (G.lds_off < 0) continue;
        const int nc = (int)G.cells * A.NI, nw = nc + (int)G.cells;
        for (int w = threadIdx.x; w < nw; w += SFS_BLOCK) {
            const uint32_t v = tab[G.lds_off + w];
            if (w < nc) {
                if (v) atomicAdd(&A.count[(size_t)G.base * A.NI + w], (unsigned long long)v);
            } else if (v != 0xFFFFFFFFu) {
                atomicMin(&A.first[(size_t)G.base + (w - nc)], A.ord0 + v);
            }
        }
    }
}

__device__ __forceinline__ uint32_t sfs_pick(const uint32_t c[4], int b) { return b == 0 ? c[0] : b == 1 ? c[1] : b == 2 ? c[2] : c[3]; }

struct SfsPops {
    int32_t in_pop[SFS_MAX_IN];   // rows: population of the layout; tables: column of the table
    int32_t out_pop;              // -1: unpolarised
};

extern __shared__ uint32_t sfs_smem[];

__global__ __launch_bounds__(SFS_BLOCK) void k_sfs_rows(const SfsArgs A, const SfsPops Q, const int8_t *__restrict__ gt, int RS,
                                                        int64_t site_lo, const int32_t *__restrict__ pop_start) {
    uint32_t *tab = sfs_smem, *t = sfs_smem + A.lds_words + threadIdx.x;
    sfs_tables_init(A, tab);
    for (int64_t i0 = (int64_t)blockIdx.x * SFS_BLOCK; i0 < A.n; i0 += (int64_t)gridDim.x * SFS_BLOCK) {
        const int64_t i = i0 + threadIdx.x;
        bool valid = i < A.n;
        if (valid) {
            const uint32_t *row = reinterpret_cast<const uint32_t *>(gt + (site_lo + i) * (int64_t)RS);
            long long tot[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0};
            uint32_t c[4];
            for (int k = 0; k < A.n_in; ++k) {
                const int s = pop_start[Q.in_pop[k]], e = pop_start[Q.in_pop[k] + 1];
                range_counts(row, s, e, c);
                valid = valid && (int)(c[0] + c[1] + c[2] + c[3]) == e - s;       // every slot of every ingroup population is called
                tot[0] += c[0]; tot[1] += c[1]; tot[2] += c[2]; tot[3] += c[3];
            }
            int base = -1;
            if (valid) {
                if (Q.out_pop >= 0) {
                    range_counts(row, pop_start[Q.out_pop], pop_start[Q.out_pop + 1], c);
                    out[0] = c[0]; out[1] = c[1]; out[2] = c[2]; out[3] = c[3];
                }
                base = sfs_target_base(tot, out, Q.out_pop >= 0);
                valid = base >= 0;
            }
            if (valid)
                for (int k = 0; k < A.n_in; ++k) {                                  // (the row is in the cache now)
                    range_counts(row, pop_start[Q.in_pop[k]], pop_start[Q.in_pop[k] + 1], c);
                    t[k * SFS_BLOCK] = sfs_pick(c, base);
                }
        }
        sfs_scatter(A, tab, t, valid, i);
    }
    sfs_tables_flush(A, tab);
}

__global__ __launch_bounds__(SFS_BLOCK) void k_sfs_base(const SfsArgs A, const SfsPops Q, const int32_t *__restrict__ cnt, int n_cols) {
    uint32_t *tab = sfs_smem, *t = sfs_smem + A.lds_words + threadIdx.x;
    sfs_tables_init(A, tab);
    for (int64_t i0 = (int64_t)blockIdx.x * SFS_BLOCK; i0 < A.n; i0 += (int64_t)gridDim.x * SFS_BLOCK) {
        const int64_t i = i0 + threadIdx.x;
        bool valid = i < A.n;
        if (valid) {
            const int4 *c4 = reinterpret_cast<const int4 *>(cnt + (size_t)i * n_cols * 4);
            long long tot[4] = {0, 0, 0, 0}, out[4] = {0, 0, 0, 0};
            bool bad = false;
            for (int k = 0; k < A.n_in; ++k) {
                const int4 v = c4[Q.in_pop[k]];
                bad = bad || v.x < 0 || v.y < 0 || v.z < 0 || v.w < 0;
                tot[0] += v.x; tot[1] += v.y; tot[2] += v.z; tot[3] += v.w;
            }
            if (Q.out_pop >= 0) {
                const int4 v = c4[Q.out_pop];
                bad = bad || v.x < 0 || v.y < 0 || v.z < 0 || v.w < 0;
                out[0] = v.x; out[1] = v.y; out[2] = v.z; out[3] = v.w;
            }
            const int base = bad ? -1 : sfs_target_base(tot, out, Q.out_pop >= 0);
            valid = base >= 0;
            if (valid)
                for (int k = 0; k < A.n_in; ++k) {
                    const int4 v = c4[Q.in_pop[k]];
                    const int x = base == 0 ? v.x : base == 1 ? v.y : base == 2 ? v.z : v.w;
                    bad = bad || x >= A.pop_ext[k];
                    t[k * SFS_BLOCK] = (uint32_t)x;
                }
            if (bad) {
                atomicOr(A.flag, 1);
                valid = false;
            }
        }
        sfs_scatter(A, tab, t, valid, i);
    }
    sfs_tables_flush(A, tab);
}

__global__ __launch_bounds__(SFS_BLOCK) void k_sfs_target(const SfsArgs A, const int32_t *__restrict__ tc) {
    uint32_t *tab = sfs_smem, *t = sfs_smem + A.lds_words + threadIdx.x;
    sfs_tables_init(A, tab);
    for (int64_t i0 = (int64_t)blockIdx.x * SFS_BLOCK; i0 < A.n; i0 += (int64_t)gridDim.x * SFS_BLOCK) {
        const int64_t i = i0 + threadIdx.x;
        bool valid = i < A.n;
        if (valid) {
            bool bad = false;
            for (int k = 0; k < A.n_in; ++k) {
                const int x = tc[(size_t)i * A.n_in + k];
                bad = bad || x < 0 || x >= A.pop_ext[k];
                t[k * SFS_BLOCK] = (uint32_t)x;
            }
            if (bad) {
                atomicOr(A.flag, 1);
                valid = false;
            }
        }
        sfs_scatter(A, tab, t, valid, i);
    }
    sfs_tables_flush(A, tab);
}

// the touched cells (first != all-ones), appended in any order: fill == 0 only counts them
__global__ __launch_bounds__(256) void k_sfs_compact(const unsigned long long *__restrict__ first, const unsigned long long *__restrict__ count,
                                                     int64_t total, int NI, int fill, unsigned long long *__restrict__ counter, int64_t cap,
                                                     int64_t *__restrict__ cell_out, unsigned long long *__restrict__ first_out,
                                                     unsigned long long *__restrict__ count_out) {
    const int lane = threadIdx.x & 63;
    for (int64_t c0 = (int64_t)blockIdx.x * 256; c0 < total; c0 += (int64_t)gridDim.x * 256) {
        const int64_t cell = c0 + threadIdx.x;
        const unsigned long long f = cell < total ? first[cell] : SFS_NONE;
        const bool touched = f != SFS_NONE;
        const unsigned long long m = __ballot(touched);
        if (!m) continue;
        const int leader = __ffsll((long long)m) - 1;
        unsigned long long at = 0;
        if (lane == leader) at = atomicAdd(counter, (unsigned long long)__popcll(m));
        at = sfs_shfl64(at, leader) + (unsigned long long)__popcll(m & ((1ull << lane) - 1ull));
        if (fill && touched && (int64_t)at < cap) {
            cell_out[at] = cell;
            first_out[at] = f;
            for (int k = 0; k < NI; ++k) count_out[at * NI + k] = count[(size_t)cell * NI + k];
        }
    }
}

// ---- host side -----------------------------------------------------------------------------------------------
struct pg_sfs_state {
    std::vector<SfsGroup> groups;
    DevBuf<SfsGroup> d_groups;
    DevBuf<unsigned long long> count, first, counter, out_first, out_count;
    DevBuf<int64_t> out_cell, pos, iv_se;
    DevBuf<int32_t> row_run, run_off, iv_id, table, flag;
    int n_in = 0, NI = 1, lds_words = 0;
    int32_t pop_ext[SFS_MAX_IN] = {};
    int64_t total = 0, chunk = 1 << 22;
    hipEvent_t e0 = nullptr, e1 = nullptr;
};

static void sfs_free(pg_ctx *c) {
    pg_sfs_state *S = static_cast<pg_sfs_state *>(c->sfs);
    if (!S) return;
    S->d_groups.release(); S->count.release(); S->first.release(); S->counter.release(); S->out_first.release(); S->out_count.release();
    S->out_cell.release(); S->pos.release(); S->iv_se.release(); S->row_run.release(); S->run_off.release(); S->iv_id.release();
    S->table.release(); S->flag.release();
    if (S->e0) (void)hipEventDestroy(S->e0);
    if (S->e1) (void)hipEventDestroy(S->e1);
    delete S;
    c->sfs = nullptr;
}

extern "C" int pg_sfs_end(pg_ctx *c) {
    if (!c) return pg_fail(PG_ERR_ARG, "null ctx");
    if (!c->sfs) return PG_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream));
    sfs_free(c);
    return PG_OK;
}

extern "C" int pg_sfs_begin(pg_ctx *c, int n_in, const int32_t *pop_ext, int n_groups, const int32_t *group_nd, const int32_t *group_pops,
                            int n_intervals, int64_t *cells_out, int32_t *on_lds_out) {
    if (!c) return pg_fail(PG_ERR_ARG, "null ctx");
    if (n_in < 1 || n_in > SFS_MAX_IN) return pg_fail(PG_ERR_ARG, "pg_sfs_begin: 1 to %d ingroup populations, not %d", SFS_MAX_IN, n_in);
    if (!pop_ext || !group_nd || !group_pops || n_groups < 1) return pg_fail(PG_ERR_ARG, "pg_sfs_begin: null argument or no group");
    if (n_intervals < 1) return pg_fail(PG_ERR_ARG, "pg_sfs_begin: at least one interval");
    HIPCHK(hipSetDevice(c->device));
    if (c->sfs) {
        HIPCHK(hipStreamSynchronize(c->stream));
        sfs_free(c);
    }
    for (int k = 0; k < n_in; ++k)
        if (pop_ext[k] < 1) return pg_fail(PG_ERR_ARG, "pg_sfs_begin: population %d has extent %d", k, pop_ext[k]);
    const char *env = getenv("PG_SFS_LDS");
    const bool use_lds = !(env && env[0] == '0');
    std::vector<SfsGroup> groups((size_t)n_groups);
    double cells_all = 0.0;
    int64_t total = 0;
    int lds_used = 0;
    for (int g = 0; g < n_groups; ++g) {
        SfsGroup &G = groups[(size_t)g];
        memset(&G, 0, sizeof(G));
        G.nd = group_nd[g];
        if (G.nd < 1 || G.nd > SFS_MAX_DIM) return pg_fail(PG_ERR_ARG, "pg_sfs_begin: group %d has %d populations (1 to %d)", g, G.nd, SFS_MAX_DIM);
        double cells_f = 1.0;
        int64_t cells = 1;
        for (int d = 0; d < G.nd; ++d) {
            const int p = group_pops[(size_t)g * SFS_MAX_DIM + d];
            if (p < 0 || p >= n_in) return pg_fail(PG_ERR_ARG, "pg_sfs_begin: group %d names population %d of %d", g, p, n_in);
            G.pop[d] = p;
            G.ext[d] = pop_ext[p];
            cells_f *= (double)pop_ext[p];
            if (cells_f < 4e18) cells *= pop_ext[p];
        }
        cells_all += cells_f;
        const double bytes = cells_all * (double)(n_intervals + 1) * 8.0;
        if (bytes > (double)c->scratch_limit)
            return pg_fail(PG_ERR_ARG, "pg_sfs_begin: the spectra's dense tables need %.0f bytes (%.2f GiB), more than the scratch budget of %lld bytes "
                                       "(PG_SCRATCH_GIB)", bytes, bytes / 1073741824.0, (long long)c->scratch_limit);
        G.base = total;
        G.cells = cells;
        total += cells;
        G.lds_off = -1;
        const int64_t words = cells * (int64_t)(n_intervals + 1);
        if (use_lds && words <= SFS_LDS_WORDS - lds_used) {
            G.lds_off = lds_used;
            lds_used += (int)words;
        }
        if (cells_out) cells_out[g] = cells;
        if (on_lds_out) on_lds_out[g] = G.lds_off >= 0 ? 1 : 0;
    }
    pg_sfs_state *S = new pg_sfs_state();
    c->sfs = S;
    S->groups = groups;
    S->n_in = n_in;
    S->NI = n_intervals;
    S->lds_words = lds_used;
    S->total = total;
    memcpy(S->pop_ext, pop_ext, (size_t)n_in * sizeof(int32_t));
    if (const char *e = getenv("PG_SFS_CHUNK")) {
        const long long v = atoll(e);
        if (v > 0) S->chunk = std::min<long long>(v, 1ll << 30);
    }
    int rc;
    if ((rc = S->d_groups.upload(groups.data(), groups.size(), c->stream)) != PG_OK || (rc = S->count.alloc((size_t)total * n_intervals)) != PG_OK ||
        (rc = S->first.alloc((size_t)total)) != PG_OK || (rc = S->counter.alloc(1)) != PG_OK || (rc = S->flag.alloc(1)) != PG_OK) {
        sfs_free(c);
        return rc;
    }
    hipError_t e = hipMemsetAsync(S->count.p, 0, (size_t)total * n_intervals * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(S->first.p, 0xFF, (size_t)total * 8, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(S->flag.p, 0, 4, c->stream);
    if (e == hipSuccess) e = hipEventCreate(&S->e0);
    if (e == hipSuccess) e = hipEventCreate(&S->e1);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);       // (`groups` is pageable: the upload has left it)
    if (e != hipSuccess) {
        sfs_free(c);
        return pg_fail(PG_ERR_HIP, "pg_sfs_begin: %s", hipGetErrorString(e));
    }
    return PG_OK;
}

// membership lists of one call (n_runs == 0: every site counts, for interval 0)
static int sfs_stage_filter(pg_ctx *c, pg_sfs_state *S, SfsArgs &A, int64_t n, int n_runs, const int32_t *run_off, const int64_t *iv_start,
                            const int64_t *iv_end, const int32_t *iv_id, const int32_t *row_run, const int64_t *pos, const char *who) {
    A.has_iv = 0;
    if (n_runs <= 0) {
        if (S->NI != 1) return pg_fail(PG_ERR_ARG, "%s: %d intervals were announced, the call names none", who, S->NI);
        return PG_OK;
    }
    if (!run_off || !row_run || !pos) return pg_fail(PG_ERR_ARG, "%s: null membership argument", who);
    const int n_iv = run_off[n_runs];
    if (run_off[0] != 0 || n_iv < 0 || (n_iv > 0 && (!iv_start || !iv_end || !iv_id))) return pg_fail(PG_ERR_ARG, "%s: bad interval lists", who);
    for (int r = 0; r < n_runs; ++r)
        if (run_off[r + 1] < run_off[r]) return pg_fail(PG_ERR_ARG, "%s: bad interval lists", who);
    for (int j = 0; j < n_iv; ++j)
        if (iv_id[j] < 0 || iv_id[j] >= S->NI) return pg_fail(PG_ERR_ARG, "%s: interval id %d out of range [0,%d)", who, iv_id[j], S->NI);
    for (int64_t i = 0; i < n; ++i)
        if (row_run[i] < 0 || row_run[i] >= n_runs) return pg_fail(PG_ERR_ARG, "%s: row %lld is of run %d of %d", who, (long long)i, row_run[i], n_runs);
    int rc;
    if ((rc = S->run_off.ensure_roomy((size_t)n_runs + 1)) != PG_OK || (rc = S->iv_se.ensure_roomy((size_t)2 * n_iv + 2)) != PG_OK ||
        (rc = S->iv_id.ensure_roomy((size_t)n_iv + 1)) != PG_OK || (rc = S->row_run.ensure_roomy((size_t)n)) != PG_OK ||
        (rc = S->pos.ensure_roomy((size_t)n)) != PG_OK)
        return rc;
    HIPCHK(hipMemcpyAsync(S->run_off.p, run_off, ((size_t)n_runs + 1) * 4, hipMemcpyHostToDevice, c->stream));
    if (n_iv > 0) {
        HIPCHK(hipMemcpyAsync(S->iv_se.p, iv_start, (size_t)n_iv * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(S->iv_se.p + n_iv, iv_end, (size_t)n_iv * 8, hipMemcpyHostToDevice, c->stream));
        HIPCHK(hipMemcpyAsync(S->iv_id.p, iv_id, (size_t)n_iv * 4, hipMemcpyHostToDevice, c->stream));
    }
    HIPCHK(hipMemcpyAsync(S->row_run.p, row_run, (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(S->pos.p, pos, (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    A.has_iv = 1;
    A.run_off = S->run_off.p;
    A.iv_start = S->iv_se.p;
    A.iv_end = S->iv_se.p + n_iv;
    A.iv_id = S->iv_id.p;
    return PG_OK;
}

static void sfs_args(pg_sfs_state *S, SfsArgs &A) {
    memset(&A, 0, sizeof(A));
    A.groups = S->d_groups.p;
    A.n_groups = (int)S->groups.size();
    A.n_in = S->n_in;
    A.NI = S->NI;
    A.lds_words = S->lds_words;
    memcpy(A.pop_ext, S->pop_ext, sizeof(A.pop_ext));
    A.count = S->count.p;
    A.first = S->first.p;
    A.flag = S->flag.p;
}

static inline unsigned sfs_grid(int64_t n) { return (unsigned)std::min<int64_t>((n + SFS_BLOCK - 1) / SFS_BLOCK, 2048); }
static inline size_t sfs_lds_bytes(const pg_sfs_state *S) { return ((size_t)S->lds_words + (size_t)S->n_in * SFS_BLOCK) * 4; }

// what every add call ends with: the kernels' error flag, the elapsed time of the launches
static int sfs_finish(pg_ctx *c, pg_sfs_state *S, double *ms_out, const char *who) {
    int32_t flag = 0;
    HIPCHK(hipMemcpyAsync(&flag, S->flag.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    if (ms_out) {
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, S->e0, S->e1));
        *ms_out = ms;
    }
    if (flag) {
        HIPCHK(hipMemsetAsync(S->flag.p, 0, 4, c->stream));
        return pg_fail(PG_ERR_ARG, "%s: a count is negative or beyond its population's extent (the rows of this call are partly counted)", who);
    }
    return PG_OK;
}

static int sfs_pops(pg_sfs_state *S, SfsPops &Q, const int32_t *in_pops, int out_pop, int limit, const char *who) {
    if (!in_pops) return pg_fail(PG_ERR_ARG, "%s: null population list", who);
    memset(&Q, 0, sizeof(Q));
    for (int k = 0; k < S->n_in; ++k) {
        if (in_pops[k] < 0 || in_pops[k] >= limit) return pg_fail(PG_ERR_ARG, "%s: population %d out of range [0,%d)", who, in_pops[k], limit);
        Q.in_pop[k] = in_pops[k];
    }
    if (out_pop < -1 || out_pop >= limit) return pg_fail(PG_ERR_ARG, "%s: outgroup %d out of range [0,%d)", who, out_pop, limit);
    Q.out_pop = out_pop;
    return PG_OK;
}

extern "C" int pg_sfs_add_sites(pg_ctx *c, int64_t site_lo, int64_t site_hi, uint64_t ord0, const int32_t *in_pops, int out_pop, int n_runs,
                                const int32_t *run_off, const int64_t *iv_start, const int64_t *iv_end, const int32_t *iv_id,
                                const int32_t *row_run, const int64_t *pos, double *ms_out) {
    if (!c) return pg_fail(PG_ERR_ARG, "null ctx");
    pg_sfs_state *S = static_cast<pg_sfs_state *>(c->sfs);
    if (!S) return pg_fail(PG_ERR_STATE, "pg_sfs_begin must be called first");
    if (c->n_hap <= 0) return pg_fail(PG_ERR_STATE, "pg_set_samples must be called first");
    if (site_lo < 0 || site_hi < site_lo || site_hi > c->cap_sites) return pg_fail(PG_ERR_ARG, "site range out of bounds");
    if (c->n_pops < 1) return pg_fail(PG_ERR_STATE, "no populations set");
    SfsPops Q;
    int rc = sfs_pops(S, Q, in_pops, out_pop, c->n_pops, "pg_sfs_add_sites");
    if (rc != PG_OK) return rc;
    for (int k = 0; k < S->n_in; ++k)
        if (c->h_pop_start[(size_t)Q.in_pop[k] + 1] - c->h_pop_start[(size_t)Q.in_pop[k]] >= S->pop_ext[k])
            return pg_fail(PG_ERR_ARG, "pg_sfs_add_sites: population %d has more haplotype slots than its extent %d allows", Q.in_pop[k], S->pop_ext[k]);
    const int64_t n = site_hi - site_lo;
    if (ms_out) *ms_out = 0.0;
    if (n == 0) return PG_OK;
    HIPCHK(hipSetDevice(c->device));
    SfsArgs A;
    sfs_args(S, A);
    if ((rc = sfs_stage_filter(c, S, A, n, n_runs, run_off, iv_start, iv_end, iv_id, row_run, pos, "pg_sfs_add_sites")) != PG_OK) return rc;
    HIPCHK(hipEventRecord(S->e0, c->stream));
    for (int64_t s = 0; s < n; s += S->chunk) {
        const int64_t m = std::min(S->chunk, n - s);
        A.n = m;
        A.ord0 = ord0 + (uint64_t)s;
        A.row_run = A.has_iv ? S->row_run.p + s : nullptr;
        A.pos = A.has_iv ? S->pos.p + s : nullptr;
        hipLaunchKernelGGL(k_sfs_rows, dim3(sfs_grid(m)), dim3(SFS_BLOCK), sfs_lds_bytes(S), c->stream, A, Q, c->gt.p, c->RS, site_lo + s, c->pop_start.p);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(S->e1, c->stream));
    return sfs_finish(c, S, ms_out, "pg_sfs_add_sites");
}

// table routes: which = 0 base counts int32 [n][n_cols][4] (in_pops / out_pop are columns), 1 target counts int32 [n][n_in]
static int sfs_add_table(pg_ctx *c, int which, const int32_t *values, int64_t n, int n_cols, uint64_t ord0, const int32_t *in_pops, int out_pop,
                         int n_runs, const int32_t *run_off, const int64_t *iv_start, const int64_t *iv_end, const int32_t *iv_id,
                         const int32_t *row_run, const int64_t *pos, double *ms_out, const char *who) {
    if (!c) return pg_fail(PG_ERR_ARG, "null ctx");
    pg_sfs_state *S = static_cast<pg_sfs_state *>(c->sfs);
    if (!S) return pg_fail(PG_ERR_STATE, "pg_sfs_begin must be called first");
    if (n < 0) return pg_fail(PG_ERR_ARG, "%s: negative row count", who);
    SfsPops Q;
    memset(&Q, 0, sizeof(Q));
    Q.out_pop = -1;
    int rc;
    if (which == 0) {
        if (n_cols < 1) return pg_fail(PG_ERR_ARG, "%s: no columns", who);
        if ((rc = sfs_pops(S, Q, in_pops, out_pop, n_cols, who)) != PG_OK) return rc;
    }
    if (ms_out) *ms_out = 0.0;
    if (n == 0) return PG_OK;
    if (!values) return pg_fail(PG_ERR_ARG, "%s: null table", who);
    HIPCHK(hipSetDevice(c->device));
    SfsArgs A;
    sfs_args(S, A);
    if ((rc = sfs_stage_filter(c, S, A, n, n_runs, run_off, iv_start, iv_end, iv_id, row_run, pos, who)) != PG_OK) return rc;
    const size_t per_row = which == 0 ? (size_t)n_cols * 4 : (size_t)S->n_in;
    if ((rc = S->table.ensure_roomy((size_t)n * per_row)) != PG_OK) return rc;
    HIPCHK(hipMemcpyAsync(S->table.p, values, (size_t)n * per_row * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipEventRecord(S->e0, c->stream));
    for (int64_t s = 0; s < n; s += S->chunk) {
        const int64_t m = std::min(S->chunk, n - s);
        A.n = m;
        A.ord0 = ord0 + (uint64_t)s;
        A.row_run = A.has_iv ? S->row_run.p + s : nullptr;
        A.pos = A.has_iv ? S->pos.p + s : nullptr;
        if (which == 0)
            hipLaunchKernelGGL(k_sfs_base, dim3(sfs_grid(m)), dim3(SFS_BLOCK), sfs_lds_bytes(S), c->stream, A, Q, S->table.p + (size_t)s * per_row, n_cols);
        else
            hipLaunchKernelGGL(k_sfs_target, dim3(sfs_grid(m)), dim3(SFS_BLOCK), sfs_lds_bytes(S), c->stream, A, S->table.p + (size_t)s * per_row);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(S->e1, c->stream));
    return sfs_finish(c, S, ms_out, who);
}

extern "C" int pg_sfs_add_base_counts(pg_ctx *c, const int32_t *cnt, int64_t n, int n_cols, uint64_t ord0, const int32_t *in_cols, int out_col,
                                      int n_runs, const int32_t *run_off, const int64_t *iv_start, const int64_t *iv_end, const int32_t *iv_id,
                                      const int32_t *row_run, const int64_t *pos, double *ms_out) {
    return sfs_add_table(c, 0, cnt, n, n_cols, ord0, in_cols, out_col, n_runs, run_off, iv_start, iv_end, iv_id, row_run, pos, ms_out,
                         "pg_sfs_add_base_counts");
}

extern "C" int pg_sfs_add_target_counts(pg_ctx *c, const int32_t *tc, int64_t n, uint64_t ord0, int n_runs, const int32_t *run_off,
                                        const int64_t *iv_start, const int64_t *iv_end, const int32_t *iv_id, const int32_t *row_run,
                                        const int64_t *pos, double *ms_out) {
    return sfs_add_table(c, 1, tc, n, 0, ord0, nullptr, -1, n_runs, run_off, iv_start, iv_end, iv_id, row_run, pos, ms_out,
                         "pg_sfs_add_target_counts");
}

extern "C" int pg_sfs_read(pg_ctx *c, int64_t cap, int64_t *cell_out, uint64_t *first_out, uint64_t *count_out, int64_t *n_out) {
    if (!c) return pg_fail(PG_ERR_ARG, "null ctx");
    pg_sfs_state *S = static_cast<pg_sfs_state *>(c->sfs);
    if (!S) return pg_fail(PG_ERR_STATE, "pg_sfs_begin must be called first");
    if (!n_out || cap < 0 || (cap > 0 && (!cell_out || !first_out || !count_out))) return pg_fail(PG_ERR_ARG, "pg_sfs_read: null output");
    HIPCHK(hipSetDevice(c->device));
    int rc;
    if (cap > 0 && ((rc = S->out_cell.ensure_roomy((size_t)cap)) != PG_OK || (rc = S->out_first.ensure_roomy((size_t)cap)) != PG_OK ||
                    (rc = S->out_count.ensure_roomy((size_t)cap * S->NI)) != PG_OK))
        return rc;
    HIPCHK(hipMemsetAsync(S->counter.p, 0, 8, c->stream));
    const unsigned grid = (unsigned)std::min<int64_t>((S->total + 255) / 256, 8192);
    hipLaunchKernelGGL(k_sfs_compact, dim3(grid), dim3(256), 0, c->stream, S->first.p, S->count.p, S->total, S->NI, cap > 0 ? 1 : 0, S->counter.p, cap,
                       S->out_cell.p, S->out_first.p, S->out_count.p);
    HIPCHK(hipGetLastError());
    unsigned long long n = 0;
    HIPCHK(hipMemcpyAsync(&n, S->counter.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipStreamSynchronize(c->stream));
    *n_out = (int64_t)n;
    if (cap > 0) {
        const size_t m = (size_t)std::min<int64_t>((int64_t)n, cap);
        if (m) {
            HIPCHK(hipMemcpy(cell_out, S->out_cell.p, m * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(first_out, S->out_first.p, m * 8, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(count_out, S->out_count.p, m * S->NI * 8, hipMemcpyDeviceToHost));
        }
    }
    return PG_OK;
}

// k_site_counts alone over resident rows, timed with events and without the copy to the host: the yardstick tools/sfs_bench.py holds
// the accumulation against (both kernels read every row once)
extern "C" int pg_sfs_time_site_counts(pg_ctx *c, int64_t site_lo, int64_t site_hi, double *ms_out) {
    if (!c) return pg_fail(PG_ERR_ARG, "null ctx");
    if (c->n_hap <= 0) return pg_fail(PG_ERR_STATE, "pg_set_samples must be called first");
    if (site_lo < 0 || site_hi < site_lo || site_hi > c->cap_sites) return pg_fail(PG_ERR_ARG, "site range out of bounds");
    if (c->n_pops < 1) return pg_fail(PG_ERR_STATE, "no populations set");
    if (!ms_out) return pg_fail(PG_ERR_ARG, "null output");
    *ms_out = 0.0;
    if (site_hi == site_lo) return PG_OK;
    HIPCHK(hipSetDevice(c->device));
    const int64_t chunk = 1 << 22;
    int rc = c->site_tmp.ensure((size_t)std::min(site_hi - site_lo, chunk) * c->n_pops * 4);
    if (rc != PG_OK) return rc;
    hipEvent_t e0, e1;
    HIPCHK(hipEventCreate(&e0));
    HIPCHK(hipEventCreate(&e1));
    hipError_t err = hipEventRecord(e0, c->stream);
    for (int64_t s = site_lo; s < site_hi && err == hipSuccess; s += chunk) {
        pg_launch_site_counts(c->stream, c->gt.p, c->RS, s, std::min(site_hi, s + chunk), c->pop_start.p, c->n_pops, c->site_tmp.p);
        err = hipGetLastError();
    }
    if (err == hipSuccess) err = hipEventRecord(e1, c->stream);
    if (err == hipSuccess) err = hipStreamSynchronize(c->stream);
    float ms = 0.f;
    if (err == hipSuccess) err = hipEventElapsedTime(&ms, e0, e1);
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    if (err != hipSuccess) return pg_fail(PG_ERR_HIP, "pg_sfs_time_site_counts: %s", hipGetErrorString(err));
    *ms_out = ms;
    return PG_OK;
}
