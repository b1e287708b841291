// The device side of the windowStats.py drop-in: the value store [selected column][site] of float64, resident on the device;
// k_ws_lines, which parses a block of the table's lines into it through a text slot of pg_line_slot.h (see the kernel: a wavefront per
// line, decimal text to float64 by pg_ws_core.h's cell rule; a block with a line outside the regular spelling is the host route's); and
// k_ws_stats, a workgroup per (window, column) over a range of sites of one column.
//
// The workgroup walks its range 256 sites at a time and compacts the non-nan values, in file order, into an LDS piece of up to
// PG_WS_PIECE values: ballots rank the lanes of a wave, the waves' totals rank the waves.  A full piece (and the last, shorter one) is
// summed as NumPy's add.reduce sums 8192 contiguous values: the parts of 128 values or fewer the recursion ends in (ws_tree_leaves)
// by a lane each with eight strided accumulators (np_pairwise_sum<0>), their sums added in the recursion's order (ws_tree_combine);
// the pieces' sums are added left to right.  That pass gives sum, mean, min, max and the count.  np.std's pass over (x - mean)^2 is
// the same walk over the squares.  The order statistics take the values' keys (ws_key) once more:
//   LDS tier   up to lds_vals values: a bitonic sort of the keys in the piece, every asked rank read from the sorted run;
//   big tier   more: per asked rank a radix select over the keys in global memory, eight passes of a 256-bin histogram in LDS that
//              narrow a prefix; no scratch that grows with the window.
// np.median's and np.quantile's arithmetic (pg_ws_core.h) finishes both.  One workgroup never shares windows: a window of one site
// costs a workgroup of which one lane has work, which the launch of 3000 such windows absorbs (profiles/wstats/README.md).
// -ffp-contract=off on the build line: no product here may be fused into a sum.
#include <algorithm>
#include <vector>

#include "pg_ctx.h"
#include "pg_wave.h"
#include "pg_ws_core.h"

namespace {

constexpr int WS_THREADS = 256;
constexpr int WS_WAVES = WS_THREADS / 64;

struct WsShared {
    double piece[PG_WS_PIECE + WS_THREADS];      // the compacted values (as keys for the order statistics); a chunk of slack
    double leaf[PG_WS_MAX_LEAVES];
    int leaf_off[PG_WS_MAX_LEAVES], leaf_len[PG_WS_MAX_LEAVES];
    int n_leaf;
    int wave_tot[WS_WAVES];
    double total;                                // the pieces' sums so far
    int have_total;
    double red[2 * WS_WAVES];
    uint32_t hist[256];
    uint64_t prefix, rank;
    double at_rank[PG_WS_NRANK];
};

// the sum of piece[0, m) in add.reduce's order, added to S.total (every thread calls; m is the same for all)
__device__ void ws_piece_sum(WsShared &S, int m, int tid) {
    if (tid == 0) {
        int k = 0;
        ws_tree_leaves<PG_WS_TREE_DEPTH>(0, m, S.leaf_off, S.leaf_len, k);
        S.n_leaf = k;
    }
    __syncthreads();
    if (tid < S.n_leaf) S.leaf[tid] = np_pairwise_sum<0>(S.piece + S.leaf_off[tid], S.leaf_len[tid]);
    __syncthreads();
    if (tid == 0) {
        int k = 0;
        const double p = ws_tree_combine<PG_WS_TREE_DEPTH>(m, S.leaf, k);
        S.total = S.have_total ? S.total + p : p;
        S.have_total = 1;
    }
    __syncthreads();
}

// One walk over x[lo, hi): the non-nan values (SQUARES: their squared deviations from `mean`) compacted in order and summed piece by
// piece into S.total; returns their number.  mn / mx: this thread's smallest and largest value.
template <bool SQUARES>
__device__ int64_t ws_walk_sum(WsShared &S, const double *__restrict__ x, int64_t lo, int64_t hi, double mean, int tid, double &mn, double &mx) {
    const int lane = tid & 63, wave = tid >> 6;
    if (tid == 0) {
        S.total = 0.0;
        S.have_total = 0;
    }
    int fill = 0;
    int64_t n = 0;
    for (int64_t base = lo; base < hi; base += WS_THREADS) {
        const int64_t i = base + tid;
        const double v = i < hi ? x[i] : __builtin_nan("");
        const bool ok = v == v;
        const unsigned long long b = __ballot(ok);
        if (lane == 0) S.wave_tot[wave] = __popcll(b);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < WS_WAVES; ++k) {
            before += k < wave ? S.wave_tot[k] : 0;
            tot += S.wave_tot[k];
        }
        if (ok) {
            S.piece[fill + before + __popcll(b & ((1ull << lane) - 1ull))] = SQUARES ? ws_dev2(v, mean) : v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
        }
        fill += tot;
        n += tot;
        __syncthreads();
        if (fill >= PG_WS_PIECE) {
            ws_piece_sum(S, PG_WS_PIECE, tid);
            const int rest = fill - PG_WS_PIECE;             // fewer than a chunk
            const double keep = tid < rest ? S.piece[PG_WS_PIECE + tid] : 0.0;
            __syncthreads();
            if (tid < rest) S.piece[tid] = keep;
            fill = rest;
            __syncthreads();
        }
    }
    if (fill > 0) ws_piece_sum(S, fill, tid);
    __syncthreads();
    return n;
}

// the keys of the n <= PG_WS_PIECE non-nan values of x[lo, hi) into the piece, sorted
__device__ void ws_sort_keys(WsShared &S, const double *__restrict__ x, int64_t lo, int64_t hi, int n, int tid) {
    uint64_t *key = reinterpret_cast<uint64_t *>(S.piece);
    const int lane = tid & 63, wave = tid >> 6;
    int fill = 0;
    for (int64_t base = lo; base < hi; base += WS_THREADS) {
        const int64_t i = base + tid;
        const double v = i < hi ? x[i] : __builtin_nan("");
        const bool ok = v == v;
        const unsigned long long b = __ballot(ok);
        if (lane == 0) S.wave_tot[wave] = __popcll(b);
        __syncthreads();
        int before = 0, tot = 0;
#pragma unroll
        for (int k = 0; k < WS_WAVES; ++k) {
            before += k < wave ? S.wave_tot[k] : 0;
            tot += S.wave_tot[k];
        }
        if (ok) key[fill + before + __popcll(b & ((1ull << lane) - 1ull))] = ws_key(v);
        fill += tot;
        __syncthreads();
    }
    int P = 1;
    while (P < n) P <<= 1;
    for (int i = n + tid; i < P; i += WS_THREADS) key[i] = ~0ull;         // (above every key of a value: +inf's is 0xFFF0...)
    __syncthreads();
    for (int k = 2; k <= P; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = tid; i < P; i += WS_THREADS) {
                const int p = i ^ j;
                if (p > i) {
                    const uint64_t a = key[i], c = key[p];
                    const bool up = (i & k) == 0;
                    if ((a > c) == up) {
                        key[i] = c;
                        key[p] = a;
                    }
                }
            }
            __syncthreads();
        }
}

// the key of rank `rank` (0-based) among the non-nan values of x[lo, hi): every thread returns it
__device__ uint64_t ws_radix_select(WsShared &S, const double *__restrict__ x, int64_t lo, int64_t hi, int64_t rank, int tid) {
    if (tid == 0) {
        S.prefix = 0;
        S.rank = (uint64_t)rank;
    }
    uint64_t known = 0;                                       // the bits of the prefix found so far
    for (int shift = 56; shift >= 0; shift -= 8) {
        S.hist[tid] = 0;                                      // (WS_THREADS == 256 bins)
        __syncthreads();
        const uint64_t prefix = S.prefix;
        for (int64_t i = lo + tid; i < hi; i += WS_THREADS) {
            const double v = x[i];
            if (v == v) {
                const uint64_t k = ws_key(v);
                if ((k & known) == prefix) atomicAdd(&S.hist[(k >> shift) & 255], 1u);
            }
        }
        __syncthreads();
        if (tid == 0) {
            uint64_t r = S.rank;
            const int bin = ws_radix_pick(S.hist, &r);
            S.rank = r;
            S.prefix = prefix | (uint64_t)bin << shift;
        }
        known |= 255ull << shift;
        __syncthreads();
    }
    const uint64_t found = S.prefix;
    __syncthreads();                                          // (the next select begins by writing S.prefix)
    return found;
}

__global__ __launch_bounds__(WS_THREADS) void k_ws_stats(const double *__restrict__ store, int64_t pitch, int n_cols,
                                                         const int64_t *__restrict__ win_lo, const int64_t *__restrict__ win_hi, int64_t w0,
                                                         uint32_t mask, int lds_vals, double *__restrict__ out, long long *__restrict__ cnt,
                                                         uint8_t *__restrict__ flag, unsigned long long *__restrict__ tiers) {
    __shared__ WsShared S;
    const int tid = threadIdx.x;
    const int64_t w = w0 + blockIdx.x;
    const int c = blockIdx.y;
    const int64_t lo = win_lo[w], hi = win_hi[w];
    const double *x = store + (size_t)c * pitch;
    const size_t cell = (size_t)w * n_cols + c;
    double *o = out + cell * PG_WS_NSTAT;
    const double nan = __builtin_nan(""), inf = __builtin_inf();

    double mn = inf, mx = -inf;
    const int64_t n = ws_walk_sum<false>(S, x, lo, hi, 0.0, tid, mn, mx);
    if (n == 0) {
        if (tid == 0) {
            for (int s = 0; s < PG_WS_NSTAT; ++s)
                if (mask & (1u << s)) o[s] = s == PG_WS_SUM ? 0.0 : nan;
            cnt[cell] = 0;
            flag[cell] = (mask & (1u << PG_WS_MIN | 1u << PG_WS_MAX)) ? 1 : 0;
        }
        return;
    }
    // min and max over the workgroup (either zero may stand for a zero: NumPy leaves the choice open as well)
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const double a = __shfl_xor(mn, d, 64), b = __shfl_xor(mx, d, 64);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
    }
    if ((tid & 63) == 0) {
        S.red[2 * (tid >> 6)] = mn;
        S.red[2 * (tid >> 6) + 1] = mx;
    }
    __syncthreads();
    const double sum = S.total, mean = ws_mean(sum, n);
    if (tid == 0) {
        for (int k = 0; k < WS_WAVES; ++k) {
            mn = S.red[2 * k] < mn ? S.red[2 * k] : mn;
            mx = S.red[2 * k + 1] > mx ? S.red[2 * k + 1] : mx;
        }
        if (mask & (1u << PG_WS_SUM)) o[PG_WS_SUM] = sum;
        if (mask & (1u << PG_WS_MEAN)) o[PG_WS_MEAN] = mean;
        if (mask & (1u << PG_WS_MIN)) o[PG_WS_MIN] = mn;
        if (mask & (1u << PG_WS_MAX)) o[PG_WS_MAX] = mx;
        cnt[cell] = n;
        flag[cell] = 0;
    }
    __syncthreads();
    if (mask & (1u << PG_WS_SD)) {
        double a = 0.0, b = 0.0;
        ws_walk_sum<true>(S, x, lo, hi, mean, tid, a, b);
        if (tid == 0) o[PG_WS_SD] = ws_sd(S.total, n);
        __syncthreads();
    }
    if (!(mask & PG_WS_ORDER_MASK)) return;
    int64_t rank[PG_WS_NRANK];
    double t[PG_WS_NQ];
    ws_ranks(n, mask, rank, t);
    if (n <= lds_vals) {
        ws_sort_keys(S, x, lo, hi, (int)n, tid);
        if (tid == 0) {
            const uint64_t *key = reinterpret_cast<const uint64_t *>(S.piece);
            for (int j = 0; j < PG_WS_NRANK; ++j) S.at_rank[j] = rank[j] >= 0 ? ws_unkey(key[rank[j]]) : nan;
            atomicAdd(&tiers[0], 1ull);
        }
    } else {
        for (int j = 0; j < PG_WS_NRANK; ++j) {
            if (rank[j] < 0) continue;
            int same = -1;                                    // a rank asked before: the median's among the quantiles', a rank twice
            for (int i = 0; i < j; ++i)
                if (rank[i] == rank[j]) same = i;
            if (same >= 0) {
                if (tid == 0) S.at_rank[j] = S.at_rank[same];
                continue;
            }
            const uint64_t k = ws_radix_select(S, x, lo, hi, rank[j], tid);
            if (tid == 0) S.at_rank[j] = ws_unkey(k);
        }
        if (tid == 0) atomicAdd(&tiers[1], 1ull);
    }
    __syncthreads();
    if (tid == 0) ws_order_stats(n, mask, S.at_rank, t, o);
}

struct WsDev {
    DevBuf<double> store, out, copy;
    DevBuf<int64_t> win, cnt;
    DevBuf<uint8_t> flag;
    DevBuf<unsigned long long> tiers;
    int n_cols = 0;
    int64_t n_sites = 0, pitch = 0;               // sites held; sites a column has room for
    void release() {
        store.release();
        out.release();
        copy.release();
        win.release();
        cnt.release();
        flag.release();
        tiers.release();
    }
};

constexpr int64_t WS_BATCH = 1 << 20;             // windows per launch at most (the grid's x; the results of a batch come back at once)
constexpr uint32_t WS_MAX_LINE = 0x3fffffffu;     // line bytes k_ws_lines takes

// ---- the lines of a block parsed into the store ----------------------------------------------------------------------------------
struct WsLineArgs {
    const uint8_t *text;
    const int64_t *nl;
    int64_t n_lines;
    int n_fields, n_sel;
    const int32_t *sel_field;                     // the field (0 = the scaffold) of selected column j
    uint32_t *rlen;                               // per line: 1 a site, 0 a '#' line
    const int64_t *rank;                          // the sites in front of the line in the block
    double *store;
    int64_t pitch, base;                          // the block's first site lands at store[column * pitch + base]
    int64_t *pos, *soff;                          // per site: the position; where its scaffold stands in the text
    int32_t *slen;
    uint8_t *runf;                                // per site: another scaffold than the site before (the block's first site: 1)
    long long *status;
};

// A wavefront per line.  The fields are cut where str.split() cuts them: a field begins at a byte that is no blank behind a blank (or
// the line's start) and ends in front of the next blank; ballots rank the beginnings and the ends into two tables in LDS.  RENDER 0
// decides: a '#' line is no site; a line of another field count than the header's, with a byte that is not ASCII or a carriage return,
// a position that is not 1 .. 18 digits, or a selected cell outside pg_ws_core.h's regular spelling hands the BLOCK to the host route.
// The scan ranks the sites.  RENDER 1 converts again, lanes strided over the selected columns, and writes each value at its place.
template <int RENDER>
__global__ __launch_bounds__(64) void k_ws_lines(WsLineArgs A) {
    extern __shared__ uint32_t ws_fields[];
    uint32_t *fs = ws_fields, *fe = ws_fields + A.n_fields;
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= A.n_lines) return;
    if (RENDER && (A.rlen[i] == 0 || A.status[PGL_ST_BITS] != 0)) return;
    const int64_t ls = i ? A.nl[i - 1] + 1 : 0, le = A.nl[i];
    const uint8_t *line = A.text + ls;
    bool host = le - ls > (int64_t)WS_MAX_LINE || le == ls;                 // (a blank line: the reference dies on it)
    const uint32_t n = host ? 0 : (uint32_t)(le - ls);
    if (n > 0 && line[0] == '#') {
        if (!RENDER && lane == 0) A.rlen[i] = 0;
        return;
    }
    uint32_t nb = 0, ne = 0;
    bool odd = false;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t k = base + (uint32_t)lane;
        const bool in = k < n;
        const uint8_t b = in ? line[k] : (uint8_t)' ';
        const bool blank = ws_blank(b);
        const bool before = !in || k == 0 || ws_blank(line[k - 1]);
        const bool after = !in || k + 1 == n || ws_blank(line[k + 1]);
        const bool beg = in && !blank && before, end = in && !blank && after;
        const unsigned long long mb = __ballot(beg), me = __ballot(end), lower = (1ull << lane) - 1ull;
        if (beg) {
            const uint32_t idx = nb + (uint32_t)__popcll(mb & lower);
            if (idx < (uint32_t)A.n_fields) fs[idx] = k;
        }
        if (end) {
            const uint32_t idx = ne + (uint32_t)__popcll(me & lower);
            if (idx < (uint32_t)A.n_fields) fe[idx] = k + 1;
        }
        nb += (uint32_t)__popcll(mb);
        ne += (uint32_t)__popcll(me);
        odd = odd || __ballot(in && (b >= 0x80 || b == '\r')) != 0;
    }
    host = host || odd || nb != (uint32_t)A.n_fields;
    __syncthreads();
    int64_t pos = 0;
    if (!host) {
        const uint32_t pl = fe[1] - fs[1];
        bool plain = pl >= 1 && pl <= 18;
        for (uint32_t k = 0; plain && k < pl; ++k) {
            const uint8_t d = line[fs[1] + k];
            plain = d >= '0' && d <= '9';
            pos = pos * 10 + (d - '0');
        }
        host = !plain;
    }
    bool bad = false;
    if (!host)
        for (int j = lane; j < A.n_sel; j += 64) {
            const int f = A.sel_field[j];
            double x;
            if (!ws_cell(line + fs[f], (int64_t)(fe[f] - fs[f]), &x)) {
                bad = true;
                break;
            }
            if (RENDER) A.store[(size_t)j * A.pitch + A.base + A.rank[i]] = x;
        }
    host = host || __ballot(bad) != 0;
    if (!RENDER) {
        if (lane == 0) {
            A.rlen[i] = host ? 0 : 1;
            if (host) pg_raise_host(A.status, i);
        }
        return;
    }
    if (host || lane != 0) return;                                          // (host: not reached, the first run kept the line)
    const int64_t r = A.rank[i];
    A.pos[r] = pos;
    A.soff[r] = ls + fs[0];
    A.slen[r] = (int32_t)(fe[0] - fs[0]);
    // the site before: the nearest line in front that is no '#' line (all lines of a block the device keeps are sites or '#' lines)
    int64_t j = i - 1;
    for (; j >= 0; --j) {
        const int64_t s = j ? A.nl[j - 1] + 1 : 0;
        if (A.text[s] != '#') break;
    }
    uint8_t differ = 1;
    if (j >= 0) {
        int64_t s = j ? A.nl[j - 1] + 1 : 0;
        const int64_t e = A.nl[j];
        while (s < e && ws_blank(A.text[s])) ++s;
        int64_t t = s;
        while (t < e && !ws_blank(A.text[t])) ++t;
        differ = t - s != (int64_t)(fe[0] - fs[0]);
        for (int64_t k = 0; !differ && k < t - s; ++k) differ = A.text[s + k] != line[fs[0] + k];
    }
    A.runf[r] = differ;
}

// room for `need` sites a column, what the store holds kept (the device idle: the old store goes away)
int ws_grow(pg_ctx *c, WsDev *W, int64_t need) {
    if (need <= W->pitch) return PG_OK;
    if (need >= (1ll << 31)) return pg_fail(PG_ERR_ARG, "windowStats: %lld sites (fewer than 2^31)", (long long)need);
    int64_t pitch = std::max<int64_t>(std::max<int64_t>(need, 2 * W->pitch), 1 << 12);
    if ((double)pitch * W->n_cols * 8.0 > (double)c->scratch_limit) pitch = need;
    if ((double)pitch * W->n_cols * 8.0 > (double)c->scratch_limit)
        return pg_fail(PG_ERR_ARG, "windowStats: %d columns of %lld sites need %.2f GiB, the scratch budget (PG_SCRATCH_GIB) is %.2f GiB",
                       W->n_cols, (long long)need, (double)pitch * W->n_cols * 8.0 / (1 << 30), (double)c->scratch_limit / (1 << 30));
    HIPCHK(hipDeviceSynchronize());
    DevBuf<double> bigger;
    int rc = bigger.ensure((size_t)pitch * W->n_cols);
    if (rc != PG_OK) return rc;
    if (W->n_sites > 0) {
        const hipError_t e = hipMemcpy2D(bigger.p, (size_t)pitch * 8, W->store.p, (size_t)W->pitch * 8, (size_t)W->n_sites * 8, (size_t)W->n_cols,
                                         hipMemcpyDeviceToDevice);
        if (e != hipSuccess) {
            bigger.release();
            return pg_fail(PG_ERR_HIP, "hipMemcpy2D: %s", hipGetErrorString(e));
        }
    }
    W->store.release();
    W->store = bigger;                            // (DevBuf is a plain record: the allocation moves)
    W->pitch = pitch;
    return PG_OK;
}

int ws_check_slot(pg_ctx *c, int slot, const char *who) { return pg_line_check_slot(c, slot, c ? &c->wsl : nullptr, who, "pg_ws_dev_config"); }

}  // namespace

extern "C" int pg_ws_end(pg_ctx *c) {
    if (!c || !c->ws) return PG_OK;
    (void)hipSetDevice(c->device);
    (void)hipDeviceSynchronize();
    WsDev *W = static_cast<WsDev *>(c->ws);
    W->release();
    delete W;
    c->ws = nullptr;
    c->wsl.configured = false;
    return PG_OK;
}

extern "C" int pg_ws_reserve(pg_ctx *c, int n_cols, int64_t n_sites) {
    if (!c) return pg_fail(PG_ERR_ARG, "null ctx");
    if (n_cols < 1 || n_cols > 65535) return pg_fail(PG_ERR_ARG, "pg_ws_reserve: %d columns (1 .. 65535)", n_cols);
    if (n_sites < 0 || n_sites >= (1ll << 31)) return pg_fail(PG_ERR_ARG, "pg_ws_reserve: %lld sites (fewer than 2^31)", (long long)n_sites);
    HIPCHK(hipSetDevice(c->device));
    if (!c->ws) c->ws = new WsDev();
    WsDev *W = static_cast<WsDev *>(c->ws);
    if (W->n_cols && W->n_cols != n_cols) return pg_fail(PG_ERR_STATE, "pg_ws_reserve: the store has %d columns, not %d", W->n_cols, n_cols);
    W->n_cols = n_cols;
    int rc;
    if ((rc = W->tiers.ensure(2)) != PG_OK) return rc;
    if ((rc = ws_grow(c, W, std::max<int64_t>(n_sites, 1))) != PG_OK) return rc;
    W->n_sites = n_sites;
    return PG_OK;
}

extern "C" int pg_ws_put(pg_ctx *c, int col, int64_t site0, const double *vals, int64_t n) {
    if (!c || !c->ws) return pg_fail(PG_ERR_STATE, "pg_ws_reserve must be called first");
    WsDev *W = static_cast<WsDev *>(c->ws);
    if (col < 0 || col >= W->n_cols || site0 < 0 || n < 0 || site0 + n > W->n_sites)
        return pg_fail(PG_ERR_ARG, "pg_ws_put: column %d, sites %lld + %lld outside the store of %d x %lld", col, (long long)site0,
                       (long long)n, W->n_cols, (long long)W->n_sites);
    if (n == 0) return PG_OK;
    if (!vals) return pg_fail(PG_ERR_ARG, "pg_ws_put: null values");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpy(W->store.p + (size_t)col * W->pitch + site0, vals, (size_t)n * 8, hipMemcpyHostToDevice));
    return PG_OK;
}

// ---- the route of the lines: a block through a text slot (pg_line_slot.h) ---------------------------------------------------------
// n_fields: the header's fields (scaffold and position among them); sel_field[n_sel]: the field of every selected column.
// *taken_out = 0: the field tables of a line do not fit LDS, the host route parses
extern "C" int pg_ws_dev_config(pg_ctx *c, int n_fields, int n_sel, const int32_t *sel_field, int *taken_out) {
    if (!c || !taken_out || n_fields < 3 || n_sel < 1 || !sel_field) return pg_fail(PG_ERR_ARG, "pg_ws_dev_config: bad argument");
    *taken_out = 0;
    c->wsl.configured = false;
    for (int j = 0; j < n_sel; ++j)
        if (sel_field[j] < 2 || sel_field[j] >= n_fields) return pg_fail(PG_ERR_ARG, "pg_ws_dev_config: a selected field outside the header");
    if ((size_t)n_fields * 8 > 60 * 1024) return PG_OK;
    HIPCHK(hipSetDevice(c->device));
    int rc = c->wsl.sel_field.upload(sel_field, (size_t)n_sel, c->stream_up);
    if (rc != PG_OK) return rc;
    HIPCHK(hipStreamSynchronize(c->stream_up));
    c->wsl.n_fields = n_fields;
    c->wsl.n_sel = n_sel;
    c->wsl.configured = true;
    *taken_out = 1;
    return PG_OK;
}

extern "C" int pg_ws_dev_submit(pg_ctx *c, int slot, const char *text, int64_t len) {
    int rc = ws_check_slot(c, slot, "pg_ws_dev_submit");
    return rc != PG_OK ? rc : pg_line_submit_plain(c, slot, c->wsl.s[slot], text, len, "pg_ws_dev_submit");
}

extern "C" int pg_ws_dev_submit_bgzf(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                                     const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                                     int64_t text_len) {
    int rc = ws_check_slot(c, slot, "pg_ws_dev_submit_bgzf");
    if (rc != PG_OK) return rc;
    if (text_len < 0) return pg_fail(PG_ERR_ARG, "pg_ws_dev_submit_bgzf: bad argument");
    return pg_line_submit_bgzf(c, slot, c->wsl.s[slot], comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, 1024,
                               false, false);
}

// Queues the kernels of the block in `slot`; base: the sites the store holds in front of it (pg_ws_reserve), behind which the block's
// sites land -- the store grows for every line of the block
extern "C" int pg_ws_dev_parse(pg_ctx *c, int slot, int64_t base, int64_t *n_lines_out) {
    int rc = ws_check_slot(c, slot, "pg_ws_dev_parse");
    if (rc != PG_OK) return rc;
    if (!c->ws) return pg_fail(PG_ERR_STATE, "pg_ws_reserve must be called first");
    WsDev *W = static_cast<WsDev *>(c->ws);
    if (!n_lines_out || base != W->n_sites || W->n_cols != c->wsl.n_sel) return pg_fail(PG_ERR_ARG, "pg_ws_dev_parse: bad argument");
    pg_ctx::WsLines &D = c->wsl;
    pg_ctx::WsLines::Slot &E = D.s[slot];
    int64_t n_lines = 0;
    bool nothing = true;
    *n_lines_out = 0;
    rc = pg_line_parse_begin(c, slot, E, &n_lines, &nothing, "pg_ws_dev_parse");
    *n_lines_out = n_lines;
    if (rc != PG_OK || nothing) return rc;
    if (n_lines > 0x7fffffffll) return pg_fail(PG_ERR_ARG, "pg_ws_dev_parse: more than 2^31 lines in a block");
    if ((rc = ws_grow(c, W, base + n_lines)) != PG_OK) return rc;
    hipStream_t st = c->stream_up;
    const size_t nl = (size_t)n_lines;
    if ((rc = E.rlen.ensure_roomy(nl)) != PG_OK || (rc = E.roff.ensure_roomy(nl)) != PG_OK || (rc = E.rank.ensure_roomy(nl)) != PG_OK ||
        (rc = E.pos.ensure_roomy(nl)) != PG_OK || (rc = E.soff.ensure_roomy(nl)) != PG_OK || (rc = E.slen.ensure_roomy(nl)) != PG_OK ||
        (rc = E.runf.ensure_roomy(nl)) != PG_OK)
        return rc;
    E.base = base;
    if ((rc = pg_line_status_upload(E, st)) != PG_OK) return rc;
    pg_ctx::TokSlot &T = c->tok[slot];
    WsLineArgs A;
    A.text = T.tp;
    A.nl = T.nl.p;
    A.n_lines = n_lines;
    A.n_fields = D.n_fields;
    A.n_sel = D.n_sel;
    A.sel_field = D.sel_field.p;
    A.rlen = E.rlen.p;
    A.rank = E.rank.p;
    A.store = W->store.p;
    A.pitch = W->pitch;
    A.base = base;
    A.pos = E.pos.p;
    A.soff = E.soff.p;
    A.slen = E.slen.p;
    A.runf = E.runf.p;
    A.status = reinterpret_cast<long long *>(E.status.p);
    const size_t lds = (size_t)D.n_fields * 8;
    hipLaunchKernelGGL((k_ws_lines<0>), dim3((unsigned)n_lines), dim3(64), lds, st, A);
    HIPCHK(hipGetLastError());
    pg_rows_scan_queue(st, E.rlen.p, n_lines, E.roff.p, A.status, n_lines + 1, E.rank.p);
    hipLaunchKernelGGL((k_ws_lines<1>), dim3((unsigned)n_lines), dim3(64), lds, st, A);
    HIPCHK(hipGetLastError());
    if ((rc = pg_line_parse_end(c, E, st)) != PG_OK) return rc;
    ++D.blocks;
    return PG_OK;
}

// Waits for the block's kernels.  *host_line_out < 0: *n_sites_out sites stand in the store behind the block's base (pg_ws_reserve
// then takes them in; pg_ws_dev_meta gives their positions and scaffolds); else the block goes to the host route
extern "C" int pg_ws_dev_collect(pg_ctx *c, int slot, int64_t *n_sites_out, int64_t *host_line_out, int64_t *n_lines_out) {
    int rc = ws_check_slot(c, slot, "pg_ws_dev_collect");
    if (rc != PG_OK) return rc;
    if (!n_sites_out || !host_line_out) return pg_fail(PG_ERR_ARG, "pg_ws_dev_collect: null argument");
    PgLineResult R;
    rc = pg_line_collect(c, slot, c->wsl, c->wsl.s[slot], false, nullptr, n_lines_out, &R, "pg_ws_dev_collect");
    *host_line_out = R.host_line;
    *n_sites_out = R.rows;
    return rc;
}

// the collected block's first n sites: positions, run flags, where the scaffolds stand in the block's text
extern "C" int pg_ws_dev_meta(pg_ctx *c, int slot, int64_t n, int64_t *pos, uint8_t *runf, int64_t *soff, int32_t *slen) {
    int rc = ws_check_slot(c, slot, "pg_ws_dev_meta");
    if (rc != PG_OK) return rc;
    pg_ctx::WsLines::Slot &E = c->wsl.s[slot];
    if (n < 0 || (size_t)n > E.pos.cap || (n && (!pos || !runf || !soff || !slen))) return pg_fail(PG_ERR_ARG, "pg_ws_dev_meta: bad argument");
    if (n == 0) return PG_OK;
    if ((rc = pg_copy_back(c, pos, E.pos.p, n * 8)) != PG_OK || (rc = pg_copy_back(c, runf, E.runf.p, n)) != PG_OK ||
        (rc = pg_copy_back(c, soff, E.soff.p, n * 8)) != PG_OK || (rc = pg_copy_back(c, slen, E.slen.p, n * 4)) != PG_OK)
        return rc;
    return PG_OK;
}

extern "C" int pg_ws_dev_text(pg_ctx *c, int slot, int64_t off, int64_t len, uint8_t *dst) {
    int rc = ws_check_slot(c, slot, "pg_ws_dev_text");
    return rc != PG_OK ? rc : pg_line_text(c, slot, off, len, dst, "pg_ws_dev_text: bad range");
}

extern "C" int pg_ws_dev_stats(pg_ctx *c, int64_t *blocks_out, int64_t *host_blocks_out) {
    return pg_line_stats(c ? &c->wsl : nullptr, blocks_out, host_blocks_out, "pg_ws_dev_stats");
}

extern "C" int pg_ws_stats(pg_ctx *c, const int64_t *lo, const int64_t *hi, int64_t n_win, uint32_t mask, int lds_vals, double *out,
                           int64_t *cnt, uint8_t *flag, int64_t *tier_out, double *ms_out) {
    if (!c || !c->ws) return pg_fail(PG_ERR_STATE, "pg_ws_reserve must be called first");
    WsDev *W = static_cast<WsDev *>(c->ws);
    if (ms_out) *ms_out = 0.0;
    if (tier_out) tier_out[0] = tier_out[1] = 0;
    if (n_win < 0) return pg_fail(PG_ERR_ARG, "negative window count");
    if (mask == 0 || mask >> PG_WS_NSTAT) return pg_fail(PG_ERR_ARG, "pg_ws_stats: statistics mask 0x%x", mask);
    if (lds_vals == 0) lds_vals = PG_WS_LDS_DEFAULT;
    if (lds_vals < 1 || lds_vals > PG_WS_PIECE) return pg_fail(PG_ERR_ARG, "pg_ws_stats: %d values in LDS (1 .. %d)", lds_vals, PG_WS_PIECE);
    if (n_win == 0) return PG_OK;
    if (!lo || !hi || !out || !cnt || !flag) return pg_fail(PG_ERR_ARG, "pg_ws_stats: null arguments");
    for (int64_t w = 0; w < n_win; ++w)
        if (lo[w] < 0 || hi[w] < lo[w] || hi[w] > W->n_sites)
            return pg_fail(PG_ERR_ARG, "pg_ws_stats: window %lld = [%lld, %lld) outside the store's %lld sites", (long long)w, (long long)lo[w],
                           (long long)hi[w], (long long)W->n_sites);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream_up));   // (the store's last block was written on the copy stream)
    const int nc = W->n_cols;
    const int64_t max_batch = std::min(WS_BATCH, n_win);
    int rc;
    if ((rc = W->win.ensure_roomy((size_t)2 * max_batch)) != PG_OK || (rc = W->out.ensure_roomy((size_t)max_batch * nc * PG_WS_NSTAT)) != PG_OK ||
        (rc = W->cnt.ensure_roomy((size_t)max_batch * nc)) != PG_OK || (rc = W->flag.ensure_roomy((size_t)max_batch * nc)) != PG_OK)
        return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    // (every failure behind this point comes back through `run`, and the events are given back below)
    auto run = [&]() -> int {
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipMemsetAsync(W->tiers.p, 0, 16, c->stream));
        for (int64_t w0 = 0; w0 < n_win; w0 += WS_BATCH) {
            const int64_t nb = std::min(WS_BATCH, n_win - w0);
            const size_t cells = (size_t)nb * nc;
            HIPCHK(hipMemcpyAsync(W->win.p, lo + w0, (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemcpyAsync(W->win.p + nb, hi + w0, (size_t)nb * 8, hipMemcpyHostToDevice, c->stream));
            HIPCHK(hipMemsetAsync(W->out.p, 0, cells * PG_WS_NSTAT * 8, c->stream));
            HIPCHK(hipEventRecord(e0, c->stream));
            hipLaunchKernelGGL(k_ws_stats, dim3((unsigned)nb, (unsigned)nc), dim3(WS_THREADS), 0, c->stream, W->store.p, W->pitch, nc, W->win.p,
                               W->win.p + nb, (int64_t)0, mask, lds_vals, W->out.p, reinterpret_cast<long long *>(W->cnt.p), W->flag.p, W->tiers.p);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(e1, c->stream));
            HIPCHK(hipMemcpyAsync(out + (size_t)w0 * nc * PG_WS_NSTAT, W->out.p, cells * PG_WS_NSTAT * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(cnt + (size_t)w0 * nc, W->cnt.p, cells * 8, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipMemcpyAsync(flag + (size_t)w0 * nc, W->flag.p, cells, hipMemcpyDeviceToHost, c->stream));
            HIPCHK(hipStreamSynchronize(c->stream));
            float ms = 0.f;
            HIPCHK(hipEventElapsedTime(&ms, e0, e1));
            if (ms_out) *ms_out += ms;
        }
        if (tier_out) {
            unsigned long long t[2];
            HIPCHK(hipMemcpy(t, W->tiers.p, 16, hipMemcpyDeviceToHost));
            tier_out[0] = (int64_t)t[0];
            tier_out[1] = (int64_t)t[1];
        }
        return PG_OK;
    };
    rc = run();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    return rc;
}

extern "C" int pg_ws_copy_time(pg_ctx *c, double *ms_out) {
    if (!c || !c->ws) return pg_fail(PG_ERR_STATE, "pg_ws_reserve must be called first");
    if (!ms_out) return pg_fail(PG_ERR_ARG, "null output");
    WsDev *W = static_cast<WsDev *>(c->ws);
    HIPCHK(hipSetDevice(c->device));
    const size_t n = (size_t)W->pitch * W->n_cols;
    int rc;
    if ((rc = W->copy.ensure(n)) != PG_OK) return rc;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    auto run = [&]() -> int {
        HIPCHK(hipEventCreate(&e0));
        HIPCHK(hipEventCreate(&e1));
        HIPCHK(hipEventRecord(e0, c->stream));
        HIPCHK(hipMemcpyAsync(W->copy.p, W->store.p, n * 8, hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(hipEventRecord(e1, c->stream));
        HIPCHK(hipStreamSynchronize(c->stream));
        float ms = 0.f;
        HIPCHK(hipEventElapsedTime(&ms, e0, e1));
        *ms_out = ms;
        return PG_OK;
    };
    rc = run();
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    W->copy.release();
    return rc;
}
