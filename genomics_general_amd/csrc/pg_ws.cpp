// The host route of the windowStats.py drop-in.  pg_ws_text parses a block of lines -- scaffold, position, then the cells of the
// selected columns with pg_ws_core.h's rule -- into float64 columns; a cell of another spelling is listed for the caller, who converts
// it as NumPy does.  pg_ws_stats_host computes a window's statistics over a column's non-nan values with std::sort and the core's
// arithmetic, the sums in add.reduce's order.  Lines end at \n (the caller has turned \r\n and a lone \r of a text-mode file into \n);
// fields are cut at runs of the bytes str.split() cuts at.  No GPU context is needed: tests/test_wstats_cpu.py calls both through the
// library on a machine without a GPU.
#include "pg_ws_core.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <thread>
#include <vector>

namespace {

struct WsIrr {
    int64_t site, sel, off, len;
};

struct WsShare {                       // what a thread found in its lines
    std::vector<WsIrr> irr;
    int err = 0;
    int64_t err_line = -1;
};

// the next field of [p, end): blanks skipped; false at the end of the line
inline bool next_field(const unsigned char *&p, const unsigned char *end, const unsigned char *&f, int64_t &len) {
    while (p < end && ws_blank(*p)) ++p;
    if (p >= end) return false;
    f = p;
    while (p < end && !ws_blank(*p)) ++p;
    len = p - f;
    return true;
}

template <class F>
void run_threads(int n_threads, int64_t n_items, F f) {
    if (n_threads <= 1 || n_items < 2) {
        f(0, 0, n_items);
        return;
    }
    const int nt = (int)std::min<int64_t>(n_threads, n_items);
    std::vector<std::thread> th;
    for (int t = 0; t < nt; ++t) th.emplace_back([&, t] { f(t, n_items * t / nt, n_items * (t + 1) / nt); });
    for (auto &x : th) x.join();
}

}  // namespace

// Error codes of a line (the first such line ends the block: the sites in front of it stand): 1 a line of fewer fields than the
// selected columns need (a blank line among them), 2 -- exact -- a line of more value fields than the header names, 7 a byte that is
// not ASCII.  A position that is not 1 .. 18 digits is listed as an irregular cell of column -1.
// sel_col[k]: the value field (0 = the field behind the position) of selected column k; n_names: the header's value names.
// vals: [n_sel][pitch] float64, row k the sites of selected column k; scaf_off / scaf_len: where each site's scaffold stands in text;
// new_run[s]: site s > 0 stands on another scaffold than site s - 1 (new_run[0] = 1: the caller knows the block before).
// irr: [cap_irr][4] = site, selected column (-1: the position), offset and length of the cell in text; *n_irr_out may exceed cap_irr
// (the caller comes again with more room).
extern "C" int pg_ws_text(const char *text_, int64_t len, int n_sel, const int32_t *sel_col, int n_names, int exact, int n_threads,
                          int64_t cap_sites, double *vals, int64_t pitch, int64_t *pos, int64_t *scaf_off, int32_t *scaf_len,
                          uint8_t *new_run, int64_t cap_irr, int64_t *irr, int64_t *n_sites_out, int64_t *n_irr_out,
                          int64_t *n_lines_out, int *err_out, int64_t *err_line_out, int64_t *err_site_out) {
    if (len < 0 || n_sel < 0 || !n_sites_out || !n_irr_out || !n_lines_out || !err_out || !err_line_out || !err_site_out) return 2;
    const unsigned char *text = reinterpret_cast<const unsigned char *>(text_);
    // the lines, and the site each line that is not a '#' line becomes
    std::vector<int64_t> start;
    for (int64_t at = 0; at < len;) {
        start.push_back(at);
        const void *nl = memchr(text + at, '\n', (size_t)(len - at));
        at = nl ? (const unsigned char *)nl - text + 1 : len;
    }
    const int64_t n_lines = (int64_t)start.size();
    start.push_back(len);
    std::vector<int64_t> site_of((size_t)n_lines + 1);
    int64_t n_sites = 0;
    for (int64_t l = 0; l < n_lines; ++l) {
        site_of[l] = n_sites;
        if (text[start[l]] != '#') ++n_sites;
    }
    site_of[n_lines] = n_sites;
    *n_lines_out = n_lines;
    *n_sites_out = 0;
    *n_irr_out = 0;
    *err_out = 0;
    *err_line_out = *err_site_out = -1;
    if (n_sites > cap_sites) {
        *n_sites_out = n_sites;          // (more room is needed: nothing was written)
        return 0;
    }
    if (n_sites && (!vals || !pos || !scaf_off || !scaf_len || !new_run || !sel_col || pitch < n_sites)) return 2;
    int need = 0;
    for (int k = 0; k < n_sel; ++k) need = std::max(need, sel_col[k] + 1);
    if (exact) need = n_names;
    std::vector<int32_t> sel_of((size_t)std::max(need, 1), -1), sel_next((size_t)std::max(n_sel, 1), -1);
    for (int k = n_sel - 1; k >= 0; --k) {       // a field may be selected more than once (--columns a a)
        sel_next[k] = sel_of[sel_col[k]];
        sel_of[sel_col[k]] = k;
    }
    const int nt = std::max(1, n_threads);
    std::vector<WsShare> share((size_t)nt);
    run_threads(nt, n_lines, [&](int t, int64_t l0, int64_t l1) {
        WsShare &W = share[t];
        for (int64_t l = l0; l < l1 && !W.err; ++l) {
            const unsigned char *p = text + start[l], *end = text + start[l + 1];
            if (*p == '#') continue;
            if (end > p && end[-1] == '\n') --end;
            const int64_t s = site_of[l];
            for (const unsigned char *q = p; q < end; ++q)
                if (*q >= 128) {
                    W.err = 7;
                    break;
                }
            const unsigned char *f;
            int64_t fl;
            if (!W.err && !next_field(p, end, f, fl)) W.err = 1;
            if (W.err) {
                W.err_line = l;
                break;
            }
            scaf_off[s] = f - text;
            scaf_len[s] = (int32_t)std::min<int64_t>(fl, INT32_MAX);
            if (!next_field(p, end, f, fl)) {
                W.err = 1;
                W.err_line = l;
                break;
            }
            bool plain = fl >= 1 && fl <= 18;
            int64_t v = 0;
            for (int64_t i = 0; plain && i < fl; ++i) {
                plain = f[i] >= '0' && f[i] <= '9';
                v = v * 10 + (f[i] - '0');
            }
            pos[s] = plain ? v : 0;
            if (!plain) W.irr.push_back({s, -1, (int64_t)(f - text), fl});
            int col = 0;
            for (; next_field(p, end, f, fl); ++col) {
                if (col >= need) {
                    if (exact) W.err = 2;
                    break;
                }
                for (int k = sel_of[col]; k >= 0; k = sel_next[k]) {
                    double x;
                    if (!ws_cell(f, fl, &x)) {
                        x = __builtin_nan("");
                        W.irr.push_back({s, k, (int64_t)(f - text), fl});
                    }
                    vals[(size_t)k * pitch + s] = x;
                }
            }
            if (!W.err && col < need) W.err = 1;
            if (W.err) W.err_line = l;
        }
    });
    int64_t err_line = -1;
    int err = 0;
    for (auto &W : share)
        if (W.err && (err_line < 0 || W.err_line < err_line)) err = W.err, err_line = W.err_line;
    const int64_t good = err ? site_of[err_line] : n_sites;
    int64_t n_irr = 0;
    for (auto &W : share)
        for (auto &x : W.irr) {
            if (x.site >= good) continue;
            if (n_irr < cap_irr && irr) memcpy(irr + 4 * n_irr, &x, sizeof x);
            ++n_irr;
        }
    for (int64_t s = 0; s < good; ++s)
        new_run[s] = s == 0 || scaf_len[s] != scaf_len[s - 1] || memcmp(text + scaf_off[s], text + scaf_off[s - 1], (size_t)scaf_len[s]) != 0;
    *n_sites_out = good;
    *n_irr_out = n_irr;
    *err_out = err;
    *err_line_out = err_line;
    *err_site_out = err ? good : -1;
    return 0;
}

// One window of one column: the non-nan values of x[lo, hi) in order -> out[PG_WS_NSTAT] (the statistics of `mask`; the others are left
// alone), their number, and whether min / max were asked of nothing.  work: room for hi - lo values.
static void ws_window_host(const double *x, int64_t lo, int64_t hi, uint32_t mask, double *work, double *out, int64_t *cnt, uint8_t *flag) {
    int64_t n = 0;
    for (int64_t i = lo; i < hi; ++i)
        if (x[i] == x[i]) work[n++] = x[i];
    *cnt = n;
    *flag = 0;
    const double nan = __builtin_nan("");
    if (n == 0) {
        for (int s = 0; s < PG_WS_NSTAT; ++s)
            if (mask & (1u << s)) out[s] = s == PG_WS_SUM ? 0.0 : nan;
        if (mask & (1u << PG_WS_MIN | 1u << PG_WS_MAX)) *flag = 1;
        return;
    }
    const double sum = ws_np_sum(work, n), mean = ws_mean(sum, n);
    if (mask & (1u << PG_WS_SUM)) out[PG_WS_SUM] = sum;
    if (mask & (1u << PG_WS_MEAN)) out[PG_WS_MEAN] = mean;
    if (mask & (1u << PG_WS_MIN)) out[PG_WS_MIN] = *std::min_element(work, work + n);
    if (mask & (1u << PG_WS_MAX)) out[PG_WS_MAX] = *std::max_element(work, work + n);
    if (mask & PG_WS_ORDER_MASK) {
        int64_t rank[PG_WS_NRANK];
        double t[PG_WS_NQ], at_rank[PG_WS_NRANK];
        ws_ranks(n, mask, rank, t);
        // (the keys' order: a total one, as the device sorts by)
        std::vector<uint64_t> key((size_t)n);
        for (int64_t i = 0; i < n; ++i) key[i] = ws_key(work[i]);
        int asked = 0;
        for (int j = 0; j < PG_WS_NRANK; ++j) asked += rank[j] >= 0;
        const bool sorted = asked > 4 || n < 64;
        if (sorted) std::sort(key.begin(), key.end());
        for (int j = 0; j < PG_WS_NRANK; ++j) {
            // (a rank is read before the next selection moves the keys again)
            if (!sorted && rank[j] >= 0) std::nth_element(key.begin(), key.begin() + rank[j], key.end());
            at_rank[j] = rank[j] >= 0 ? ws_unkey(key[rank[j]]) : nan;
        }
        ws_order_stats(n, mask, at_rank, t, out);
    }
    if (mask & (1u << PG_WS_SD)) {               // (last: it writes over the values)
        for (int64_t i = 0; i < n; ++i) work[i] = ws_dev2(work[i], mean);
        out[PG_WS_SD] = ws_sd(ws_np_sum(work, n), n);
    }
}

// vals: [n_cols][pitch]; windows [lo[w], hi[w]) of sites; out: [n_win][n_cols][PG_WS_NSTAT], cnt and flag: [n_win][n_cols]
extern "C" int pg_ws_stats_host(const double *vals, int64_t pitch, int n_cols, const int64_t *lo, const int64_t *hi, int64_t n_win,
                                uint32_t mask, int n_threads, double *out, int64_t *cnt, uint8_t *flag) {
    if (n_win < 0 || n_cols < 0) return 2;
    if (n_win == 0 || n_cols == 0) return 0;
    if (!vals || !lo || !hi || !out || !cnt || !flag) return 2;
    for (int64_t w = 0; w < n_win; ++w)
        if (lo[w] < 0 || hi[w] < lo[w] || hi[w] > pitch) return 2;
    run_threads(std::max(1, n_threads), n_win, [&](int, int64_t w0, int64_t w1) {
        std::vector<double> work;
        for (int64_t w = w0; w < w1; ++w) {
            if ((int64_t)work.size() < hi[w] - lo[w]) work.resize((size_t)(hi[w] - lo[w]));
            for (int c = 0; c < n_cols; ++c) {
                const size_t cell = (size_t)w * n_cols + c;
                ws_window_host(vals + (size_t)c * pitch, lo[w], hi[w], mask, work.data(), out + cell * PG_WS_NSTAT, &cnt[cell], &flag[cell]);
            }
        }
    });
    return 0;
}
