// `.geno` sites filtered on the device: the filterGenotypes.py drop-in's route for the regular spelling of a line (fields split by
// single tabs, the header's number of fields, ASCII).  The per-cell and per-site rules are csrc/pg_filter_core.h (the host route
// pg_filter_text in pg_filter.cpp runs the same functions); this file is the division of the work over the chip and the host side of
// the entry points.
//
//   k_filt_lines<0>  a wavefront per line: the line's tabs ranked by ballots into LDS, the contig looked up (a lane per listed name),
//                    a lane per selected column classifies its cells, the sums reduced across the wave, siteTest; the line's flags,
//                    its position (thinning) and its row's size
//   k_filt_thin      (--thinDist only) a lane per pod walks its lines in order over the flags and positions (filterGenotypes.py:41-55)
//   scan             the rows' places (k_rows_scan, pg_line_slot.hip)
//   k_filt_lines<1>  a wavefront per written line: the first two fields copied, the cells rendered, placed by a wave scan of their sizes
// The text arrives in the tokenizer's text slot with its line feeds listed (pg_tok_text_submit / pg_tok_lines).  A line outside the
// regular spelling, or one on which the reference raises, hands the BLOCK to the host route (pg_filter_dev_collect reports the line).
#include "pg_ctx.h"
#include "pg_filter_core.h"
#include "pg_line_fields.h"
#include "pg_wave.h"

#include <algorithm>
#include <cstring>

namespace {

// per-line flags of k_filt_lines<0>
#define PGF_L_KEPT 1        // not skipped by --include / --exclude
#define PGF_L_PASS 2        // siteTest passes (or --noTest)
#define PGF_L_TEST_ERR 4    // siteTest raises
#define PGF_L_ROW_ERR 8     // rendering the row raises

#define PGF_MAX_CELL_IN 40  // cell bytes the device takes (PGF_MAXA alleles phased: 31)

struct FiltArgs {
    const uint8_t *text;
    const int64_t *nl;
    int64_t n_lines;
    const int32_t *sel_col, *sel_ploidy;
    const uint32_t *sel_popmask, *coff;
    const uint8_t *contigs, *cflags;
    uint8_t *flags;
    uint32_t *rlen;
    int64_t *pos, *roff;
    uint8_t *out;
    long long *status;
};

// the cells of the selected columns classified and summed: tot over the wave (the same on every lane), the populations' sums in LDS
// (`pop`, n_pops records behind the tab table, added by LDS atomics: no per-lane array).  Returns false (on every lane) when some cell
// needs the host
__device__ bool line_sums(const FiltArgs &A, const PgfConfig &cfg, const uint8_t *line, const uint32_t *tabs, uint32_t n, int lane,
                          PgfCounts *tot, PgfCounts *pop) {
    int32_t *pw = reinterpret_cast<int32_t *>(pop);
    for (int k = lane; k < cfg.n_pops * (int)(sizeof(PgfCounts) / 4); k += 64) pw[k] = 0;
    __syncthreads();
    PgfCounts t = {};
    bool bad = false;
    for (int j = lane; j < cfg.n_sel; j += 64) {
        uint32_t s, e;
        field_at(tabs, A.sel_col[j], cfg.n_cols, n, &s, &e);
        PgfGeno g;
        if (e - s > PGF_MAX_CELL_IN || pgf_classify(line + s, (int)(e - s), cfg.in_fmt, A.sel_ploidy[j], cfg.force_ploidy, cfg.partial_to_missing, &g)) {
            bad = true;
            break;
        }
        pgf_add(g, &t);
        const uint32_t mask = A.sel_popmask[j];
        if (mask) {
            PgfCounts one = {};
            pgf_add(g, &one);
            for (uint32_t m = mask; m; m &= m - 1) {
                PgfCounts &q = pop[__builtin_ctz(m)];
                for (int b = 0; b < 4; ++b)
                    if (one.c[b]) atomicAdd(&q.c[b], one.c[b]);
                if (one.calls) atomicAdd(&q.calls, one.calls);
                if (one.not_nn) atomicAdd(&q.not_nn, one.not_nn);
            }
        }
    }
    __syncthreads();
    if (__ballot(bad)) return false;
    for (int b = 0; b < 4; ++b) tot->c[b] = pg_wave_sum(t.c[b]);
    tot->calls = pg_wave_sum(t.calls);
    tot->hets = pg_wave_sum(t.hets);
    tot->not_nn = pg_wave_sum(t.not_nn);
    return true;
}

// one row's size / its text
template <int RENDER>
__global__ __launch_bounds__(64) void k_filt_lines(FiltArgs A, PgfConfig cfg) {
    extern __shared__ uint32_t tabs[];
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= A.n_lines) return;
    if (RENDER && (A.rlen[i] == 0 || A.status[PGL_ST_BITS] != 0)) return;   // (a raised status: the block is the host's, its rows are not written)
    const int64_t ls = i ? A.nl[i - 1] + 1 : 0, le = A.nl[i];
    const uint8_t *line = A.text + ls;
    if (le - ls > 0x7fffffffll) {
        if (!RENDER && lane == 0) { A.flags[i] = 0; A.rlen[i] = 0; pg_raise_host(A.status, i); }
        return;
    }
    const uint32_t n = (uint32_t)(le - ls);
    if (!line_tabs(line, n, cfg.n_cols, lane, tabs)) {
        if (!RENDER && lane == 0) { A.flags[i] = 0; A.rlen[i] = 0; pg_raise_host(A.status, i); }
        return;
    }
    const uint32_t f0e = tabs[0], f1s = tabs[0] + 1, f1e = cfg.n_cols > 2 ? tabs[1] : n;
    if (!RENDER && cfg.contig_mode) {                              // filterGenotypes.py:37
        bool in = false, ex = false;
        for (int j = lane; j < cfg.n_contigs; j += 64) {
            const uint32_t cs = A.coff[j], cl = A.coff[j + 1] - 1 - cs;
            bool eq = cl == f0e;
            for (uint32_t k = 0; eq && k < cl; ++k) eq = A.contigs[cs + k] == line[k];
            in = in || (eq && (A.cflags[j] & 1));
            ex = ex || (eq && (A.cflags[j] & 2));
        }
        in = __ballot(in) != 0;
        ex = __ballot(ex) != 0;
        if (((cfg.contig_mode & 1) && !in) || ((cfg.contig_mode & 2) && ex)) {
            if (lane == 0) { A.flags[i] = 0; A.rlen[i] = 0; }
            return;
        }
    }
    PgfCounts tot;
    PgfCounts *pop = reinterpret_cast<PgfCounts *>(tabs + cfg.n_cols);
    if (!line_sums(A, cfg, line, tabs, n, lane, &tot, pop)) {       // (a cell the reference raises on is worded by the host)
        if (!RENDER && lane == 0) { A.flags[i] = 0; A.rlen[i] = 0; pg_raise_host(A.status, i); }
        return;
    }
    int order[4];
    const int nA = pgf_order(tot.c, order);
    if (!RENDER) {
        uint8_t fl = PGF_L_KEPT;
        bool host = false;
        if (cfg.thin_dist) {
            int64_t pos = 0;
            host = pgf_parse_pos(line + f1s, (int)(f1e - f1s), &pos) != 0;
            if (lane == 0) A.pos[i] = pos;
        }
        const int t = cfg.no_test ? 1 : pgf_site_test(cfg, tot, pop);
        if (t == 1) fl |= PGF_L_PASS;
        if (t < 0) fl |= PGF_L_TEST_ERR;
        uint32_t len = 0;
        if (t == 1) {                                              // the row's size: CHROM \t POS, a tab and the text of every cell, \n
            bool err = false;
            int sum = 0;
            char cell[PGF_CELL_MAX];
            for (int j = lane; j < cfg.n_sel; j += 64) {
                uint32_t s, e;
                field_at(tabs, A.sel_col[j], cfg.n_cols, n, &s, &e);
                PgfGeno g;
                pgf_classify(line + s, (int)(e - s), cfg.in_fmt, A.sel_ploidy[j], cfg.force_ploidy, cfg.partial_to_missing, &g);
                const int L = pgf_render(cfg, g, order, nA, cell);
                if (L < 0) err = true;
                else sum += L + 1;
            }
            sum = pg_wave_sum(sum);
            if (__ballot(err)) fl |= PGF_L_ROW_ERR;
            else len = f1e + (uint32_t)sum + 1;
        }
        // without thinning a raised siteTest or row stops here; with it, k_filt_thin decides whether the line gets that far
        if (!cfg.thin_dist && (fl & (PGF_L_TEST_ERR | PGF_L_ROW_ERR))) host = true;
        if (lane == 0) {
            A.flags[i] = fl;
            A.rlen[i] = (fl & PGF_L_ROW_ERR) ? 0 : len;
            if (host) pg_raise_host(A.status, i);
        }
        return;
    }
    // RENDER: CHROM \t POS as they stand, then the cells
    uint8_t *o = A.out + A.roff[i];
    for (uint32_t k = (uint32_t)lane; k < f1e; k += 64) o[k] = line[k];
    uint32_t at = f1e;
    char cell[PGF_CELL_MAX];
    for (int base = 0; base < cfg.n_sel; base += 64) {
        const int j = base + lane;
        int L = 0;
        if (j < cfg.n_sel) {
            uint32_t s, e;
            field_at(tabs, A.sel_col[j], cfg.n_cols, n, &s, &e);
            PgfGeno g;
            pgf_classify(line + s, (int)(e - s), cfg.in_fmt, A.sel_ploidy[j], cfg.force_ploidy, cfg.partial_to_missing, &g);
            L = pgf_render(cfg, g, order, nA, cell);
            if (L < 0) L = 0;                                      // (cannot happen: k_filt_lines<0> sent such rows to the host)
        }
        const int w = j < cfg.n_sel ? L + 1 : 0;
        const int off = pg_wave_excl_scan(w, lane);
        if (j < cfg.n_sel) {
            uint8_t *d = o + at + (uint32_t)off;
            d[0] = '\t';
            for (int k = 0; k < L; ++k) d[1 + k] = (uint8_t)cell[k];
        }
        at += (uint32_t)__shfl(off + w, 63, 64);
    }
    if (lane == 0) o[at] = '\n';
}

// --thinDist: a lane per pod of the block (the block starts at a pod boundary), its lines walked in order (filterGenotypes.py:32-55)
__global__ __launch_bounds__(64) void k_filt_thin(FiltArgs A, PgfConfig cfg) {
    const int64_t p = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const int64_t a = p * cfg.pod_size;
    if (a >= A.n_lines) return;
    const int64_t b = std::min<int64_t>(A.n_lines, a + cfg.pod_size);
    bool have = false;
    int64_t last_s = 0, last_n = 0, last_pos = 0;
    for (int64_t i = a; i < b; ++i) {
        const uint8_t fl = A.flags[i];
        if (!(fl & PGF_L_KEPT)) continue;
        const int64_t ls = i ? A.nl[i - 1] + 1 : 0;
        int64_t cn = 0;
        while (A.text[ls + cn] != '\t') ++cn;                     // (k_filt_lines<0> checked the tabs of a kept line)
        bool same = have && cn == last_n;
        for (int64_t k = 0; same && k < cn; ++k) same = A.text[ls + k] == A.text[last_s + k];
        if (!same) { last_s = ls; last_n = cn; have = true; }
        const bool keep = pgf_thin_keep(same, A.pos[i], &last_pos, cfg.thin_dist);
        if (keep && (fl & PGF_L_TEST_ERR)) { pg_raise_host(A.status, i); return; }
        const bool pass = keep && (fl & PGF_L_PASS);
        if (pass && (fl & PGF_L_ROW_ERR)) { pg_raise_host(A.status, i); return; }
        if (pass) last_pos = A.pos[i];
        else A.rlen[i] = 0;
    }
}

int check_slot(pg_ctx *c, int slot, const char *who) { return pg_line_check_slot(c, slot, c ? &c->filt : nullptr, who, "pg_filter_dev_config"); }

}  // namespace

extern "C" int pg_filter_dev_config(pg_ctx *c, const pg_filter_cfg *cfg, const int32_t *sel_col, const int32_t *sel_ploidy,
                                    const uint32_t *sel_popmask, const char *contigs, int n_contig_bytes, const uint8_t *contig_flags,
                                    int *taken_out) {
    if (!c || !cfg || !taken_out || n_contig_bytes < 0 || cfg->n_sel < 0 || cfg->n_pops < 0 || cfg->n_contigs < 0 ||
        (cfg->n_sel && (!sel_col || !sel_ploidy || !sel_popmask)) || (cfg->n_contigs && (!contigs || !contig_flags)) ||
        (cfg->thin_dist && cfg->pod_size < 1))
        return pg_fail(PG_ERR_ARG, "pg_filter_dev_config: bad argument");
    *taken_out = 0;
    pg_ctx::FiltDev &D = c->filt;
    D.configured = false;
    // the tab table of a line lives in LDS (4 bytes per field, one wavefront per block); at most PGF_MAXPOP populations
    if (cfg->n_cols < 2 || (size_t)cfg->n_cols * 4 + (size_t)cfg->n_pops * sizeof(PgfCounts) > 60 * 1024 || cfg->n_pops > PGF_MAXPOP) return PG_OK;
    for (int j = 0; j < cfg->n_sel; ++j)
        if (sel_col[j] < 0 || sel_col[j] >= cfg->n_cols || sel_ploidy[j] > PGF_MAXA) return PG_OK;
    std::vector<uint32_t> coff{0};
    for (int k = 0; k < cfg->n_contigs; ++k) {
        const void *z = (int)coff.back() < n_contig_bytes ? memchr(contigs + coff.back(), 0, (size_t)(n_contig_bytes - (int)coff.back())) : nullptr;
        if (!z) return pg_fail(PG_ERR_ARG, "pg_filter_dev_config: contig list shorter than n_contigs");
        coff.push_back((uint32_t)(static_cast<const char *>(z) - contigs) + 1);
    }
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    const size_t ns = (size_t)std::max(cfg->n_sel, 1), nc = (size_t)std::max(cfg->n_contigs, 1);
    int rc;
    if ((rc = D.sel_col.ensure(ns)) != PG_OK || (rc = D.sel_ploidy.ensure(ns)) != PG_OK || (rc = D.sel_popmask.ensure(ns)) != PG_OK ||
        (rc = D.coff.ensure(nc + 1)) != PG_OK || (rc = D.contigs.ensure((size_t)n_contig_bytes + 1)) != PG_OK || (rc = D.cflags.ensure(nc)) != PG_OK)
        return rc;
    if (cfg->n_sel) {
        HIPCHK(hipMemcpy(D.sel_col.p, sel_col, (size_t)cfg->n_sel * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(D.sel_ploidy.p, sel_ploidy, (size_t)cfg->n_sel * 4, hipMemcpyHostToDevice));
        HIPCHK(hipMemcpy(D.sel_popmask.p, sel_popmask, (size_t)cfg->n_sel * 4, hipMemcpyHostToDevice));
    }
    HIPCHK(hipMemcpy(D.coff.p, coff.data(), coff.size() * 4, hipMemcpyHostToDevice));
    if (n_contig_bytes) HIPCHK(hipMemcpy(D.contigs.p, contigs, (size_t)n_contig_bytes, hipMemcpyHostToDevice));
    if (cfg->n_contigs) HIPCHK(hipMemcpy(D.cflags.p, contig_flags, (size_t)cfg->n_contigs, hipMemcpyHostToDevice));
    D.cfg = *cfg;
    D.configured = true;
    *taken_out = 1;
    return PG_OK;
}

// A block of whole lines (the last byte a line feed, else the block is the host's) into text slot `slot`; first_line: the block's first
// data line of the file (with thinning a multiple of the pod size: a pod never spans two blocks)
extern "C" int pg_filter_dev_submit(pg_ctx *c, int slot, const char *text, int64_t len, int64_t first_line) {
    int rc = check_slot(c, slot, "pg_filter_dev_submit");
    if (rc != PG_OK) return rc;
    if ((!text && len) || len < 0 || first_line < 0) return pg_fail(PG_ERR_ARG, "pg_filter_dev_submit: no text");
    pg_ctx::FiltDev::Slot &F = c->filt.s[slot];
    if (c->filt.cfg.thin_dist && first_line % c->filt.cfg.pod_size)
        return pg_fail(PG_ERR_ARG, "pg_filter_dev_submit: with --thinDist a block starts at a pod (line %lld)", (long long)first_line);
    F.first_line = first_line;
    return pg_line_submit_text(c, slot, F, text, -1, 0, len, len > 0 && text[len - 1] == '\n');
}

// The same for a block that is still bgzipped: the members cross PCIe deflated, k_inflate writes their text behind `head` in the slot
// and lists its line feeds (pg_tok_bgzf_submit).  Not with thinning (the pods are cut in text).  Whether the text ends in a line feed is
// read on the device once the line feeds are counted (the file's last block may not).
extern "C" int pg_filter_dev_submit_bgzf(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                                         const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                                         int64_t text_len, int64_t first_line) {
    int rc = check_slot(c, slot, "pg_filter_dev_submit_bgzf");
    if (rc != PG_OK) return rc;
    if (c->filt.cfg.thin_dist) return pg_fail(PG_ERR_ARG, "pg_filter_dev_submit_bgzf: not with --thinDist (pods are cut in text)");
    if (first_line < 0 || text_len < 0) return pg_fail(PG_ERR_ARG, "pg_filter_dev_submit_bgzf: bad argument");
    pg_ctx::FiltDev::Slot &F = c->filt.s[slot];
    F.first_line = first_line;
    return pg_line_submit_bgzf(c, slot, F, comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, 1024, false, false);
}

// bgzf_members != 0: the rows of every block filtered from now on are also deflated on the device (k_deflate: BGZF members of 65 280
// bytes of rows, no end-of-file member); pg_filter_dev_collect reports their bytes, pg_filter_dev_rows_bgzf fetches them
extern "C" int pg_filter_dev_set_output(pg_ctx *c, int bgzf_members) {
    if (!c) return pg_fail(PG_ERR_ARG, "pg_filter_dev_set_output: null context");
    c->filt.bgzf_rows = bgzf_members != 0;
    return PG_OK;
}

namespace {

FiltArgs filt_args(pg_ctx *c, int slot) {
    pg_ctx::FiltDev &D = c->filt;
    pg_ctx::FiltDev::Slot &F = D.s[slot];
    pg_ctx::TokSlot &T = c->tok[slot];
    FiltArgs A;
    A.text = T.tp;
    A.nl = T.nl.p;
    A.n_lines = F.L.n_lines;
    A.sel_col = D.sel_col.p;
    A.sel_ploidy = D.sel_ploidy.p;
    A.sel_popmask = D.sel_popmask.p;
    A.coff = D.coff.p;
    A.contigs = D.contigs.p;
    A.cflags = D.cflags.p;
    A.flags = F.flags.p;
    A.rlen = F.rlen.p;
    A.pos = F.pos.p;
    A.roff = F.roff.p;
    A.out = F.out.p;
    A.status = reinterpret_cast<long long *>(F.status.p);
    return A;
}

size_t filt_lds(const PgfConfig &cfg) { return (size_t)cfg.n_cols * 4 + (size_t)cfg.n_pops * sizeof(PgfCounts); }

// the rows' text (k_filt_lines<1>) and, for -o x.gz, their members (k_deflate), then the status back to the host (the block: queued)
int queue_render(pg_ctx *c, int slot, hipStream_t st) {
    pg_ctx::FiltDev &D = c->filt;
    pg_ctx::FiltDev::Slot &F = D.s[slot];
    const FiltArgs A = filt_args(c, slot);
    hipLaunchKernelGGL((k_filt_lines<1>), dim3((unsigned)F.L.n_lines), dim3(64), filt_lds(D.cfg), st, A, D.cfg);
    HIPCHK(hipGetLastError());
    if (D.bgzf_rows) {
        int rc = pg_deflate_queue(c, st, F.df, F.out.p, A.status + PGL_ST_BYTES, F.out_cap, A.status, A.status + PGL_ST_BGZF_BYTES);
        if (rc != PG_OK) return rc;
    }
    return pg_line_parse_end(c, F, st);
}

// rows longer than their room: room for `need` bytes of them (k_deflate reads 32 bytes past the rows), rendered once more
int render_again(pg_ctx *c, int slot, int64_t need, hipStream_t st) {
    pg_ctx::FiltDev::Slot &F = c->filt.s[slot];
    int rc = F.out.ensure_roomy((size_t)need + 4096 + 64);
    if (rc != PG_OK) return rc;
    F.out_cap = (int64_t)F.out.cap - 64;
    return queue_render(c, slot, st);
}

}  // namespace

// Queues the kernels of the block in `slot` (waits for the number of its lines only)
extern "C" int pg_filter_dev_parse(pg_ctx *c, int slot) {
    int rc = check_slot(c, slot, "pg_filter_dev_parse");
    if (rc != PG_OK) return rc;
    pg_ctx::FiltDev &D = c->filt;
    pg_ctx::FiltDev::Slot &F = D.s[slot];
    // a block without a final line feed (the file's partial last line) is the host's; a '\r' in a line sends it there too (k_filt_lines)
    int64_t n_lines = 0;
    bool nothing = true;
    if ((rc = pg_line_parse_begin(c, slot, F, &n_lines, &nothing, "pg_filter_dev_parse")) != PG_OK || nothing) return rc;
    hipStream_t st = c->stream_up;
    pg_ctx::TokSlot &T = c->tok[slot];
    if ((rc = F.flags.ensure_roomy((size_t)n_lines)) != PG_OK || (rc = F.rlen.ensure_roomy((size_t)n_lines)) != PG_OK ||
        (rc = F.roff.ensure_roomy((size_t)n_lines)) != PG_OK || (rc = F.pos.ensure_roomy((size_t)n_lines)) != PG_OK)
        return rc;
    // rows: the text's own size for most formats; a larger total (str(tuple) cells, padded ploidies) grows the buffer in collect
    F.out_cap = std::max<int64_t>(F.out_cap, T.len + n_lines * 16 + 4096);
    if ((rc = F.out.ensure_roomy((size_t)F.out_cap + 64)) != PG_OK) return rc;
    F.out_cap = (int64_t)F.out.cap - 64;                          // (k_deflate reads 32 bytes past the rows)
    if ((rc = pg_line_status_upload(F, st)) != PG_OK) return rc;
    const FiltArgs A = filt_args(c, slot);
    hipLaunchKernelGGL((k_filt_lines<0>), dim3((unsigned)n_lines), dim3(64), filt_lds(D.cfg), st, A, D.cfg);
    if (D.cfg.thin_dist) {
        const int64_t pods = (n_lines + D.cfg.pod_size - 1) / D.cfg.pod_size;
        hipLaunchKernelGGL(k_filt_thin, dim3((unsigned)((pods + 63) / 64)), dim3(64), 0, st, A, D.cfg);
    }
    pg_rows_scan_queue(st, F.rlen.p, n_lines, F.roff.p, A.status, F.out_cap);
    if ((rc = queue_render(c, slot, st)) != PG_OK) return rc;
    ++D.blocks;
    return PG_OK;
}

// Waits for the block's kernels.  *host_line_out < 0: the rows are ready (*rows_len_out bytes, *n_rows_out rows: pg_filter_dev_rows;
// *bgzf_len_out bytes of members: pg_filter_dev_rows_bgzf); else the block goes to the host route -- line *host_line_out is the first
// the device does not take.  Rows longer than the buffer (the scan knows their total) grow it and are rendered again.
extern "C" int pg_filter_dev_collect(pg_ctx *c, int slot, int64_t *rows_len_out, int64_t *n_rows_out, int64_t *host_line_out,
                                     int64_t *bgzf_len_out, int64_t *n_lines_out) {
    int rc = check_slot(c, slot, "pg_filter_dev_collect");
    if (rc != PG_OK) return rc;
    if (!rows_len_out || !n_rows_out || !host_line_out) return pg_fail(PG_ERR_ARG, "pg_filter_dev_collect: null argument");
    PgLineResult R;
    rc = pg_line_collect(c, slot, c->filt, c->filt.s[slot], c->filt.bgzf_rows, render_again, n_lines_out, &R, "pg_filter_dev_collect");
    *host_line_out = R.host_line;
    *rows_len_out = R.bytes;
    *n_rows_out = R.rows;
    if (bgzf_len_out) *bgzf_len_out = R.bgzf_bytes;
    return rc;
}

extern "C" int pg_filter_dev_rows(pg_ctx *c, int slot, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_filter_dev_rows");
    return rc != PG_OK ? rc : pg_line_rows(c, c->filt.s[slot].out, dst, len, "pg_filter_dev_rows: bad length");
}

extern "C" int pg_filter_dev_rows_bgzf(pg_ctx *c, int slot, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_filter_dev_rows_bgzf");
    return rc != PG_OK ? rc : pg_line_rows(c, c->filt.s[slot].df.comp, dst, len, "pg_filter_dev_rows_bgzf: bad length");
}

// the text of the collected block -> dst (a block that goes to the host route and whose text the host never had: BGZF)
extern "C" int pg_filter_dev_text(pg_ctx *c, int slot, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_filter_dev_text");
    return rc != PG_OK ? rc : pg_line_text(c, slot, 0, len, dst, "pg_filter_dev_text: bad length");
}

extern "C" int pg_filter_dev_stats(pg_ctx *c, int64_t *blocks_out, int64_t *host_blocks_out) {
    return pg_line_stats(c ? &c->filt : nullptr, blocks_out, host_blocks_out, "pg_filter_dev_stats");
}
