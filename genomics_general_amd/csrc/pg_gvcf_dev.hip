// `.geno` sites written as VCF rows on the device: the genoToVCF.py drop-in's route for the regular spelling of a line (fields split by
// single tabs, the header's number of fields, ASCII, a position of digits only).  The per-site and per-cell rules are
// csrc/pg_gvcf_core.h (the host route pg_gvcf_text in pg_gvcf.cpp runs the same functions); this file is the division of the work over
// the chip and the host side of the entry points.
//
//   k_gvcf_lines<0>  a wavefront per line: the line's tabs ranked by ballots into LDS (pg_line_fields.h), lanes strided over the
//                    selected columns classify their cells, the four base counts and the cells' bytes reduced across the wave; with -r
//                    the scaffold's hash summed a lane a byte and looked up in the table over the fasta's names, the base read; the
//                    alleles ordered (pgg_alleles); the row's size
//   scan             the rows' places (k_rows_scan, pg_line_slot.hip)
//   k_gvcf_lines<1>  the same walk for a written line, then: CHROM \t POS copied, ID .. FORMAT written, the cells coded and placed by
//                    a wave scan of their sizes
// The text arrives in the tokenizer's text slot with its line feeds listed (pg_line_slot.h: submit, parse, collect).  A line outside
// the regular spelling, or one the run stops on, hands the BLOCK to the host route (pg_gvcf_dev_collect reports the line).
#include "pg_ctx.h"
#include "pg_gvcf_core.h"
#include "pg_line_fields.h"
#include "pg_wave.h"

#include <algorithm>
#include <cstring>

namespace {

#define PGG_MAX_CELL_IN 40          // cell bytes the device takes (PGF_MAXA alleles phased: 31)
#define PGG_MAX_LINE 0x3fffffffu    // line bytes the device takes (a row of three times that still fits 32 bits)

struct GvcfArgs {
    const uint8_t *text;
    const int64_t *nl;
    int64_t n_lines;
    const int32_t *sel_col;
    pgg_ref R;
    uint32_t *rlen;
    int64_t *roff;
    uint8_t *out;
    long long *status;
};

// one row's size / its text
template <int RENDER>
__global__ __launch_bounds__(64) void k_gvcf_lines(GvcfArgs A, PggConfig cfg) {
    extern __shared__ uint32_t tabs[];
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= A.n_lines) return;
    if (RENDER && (A.rlen[i] == 0 || A.status[PGL_ST_BITS] != 0)) return;   // (a raised status: the block is the host's, its rows are not written)
    const int64_t ls = i ? A.nl[i - 1] + 1 : 0, le = A.nl[i];
    const uint8_t *line = A.text + ls;
    bool host = le - ls > (int64_t)PGG_MAX_LINE;
    const uint32_t n = host ? 0 : (uint32_t)(le - ls);
    if (!host && n > 0 && line[0] == '#') {                                // genomics.py:1936: no site
        if (!RENDER && lane == 0) A.rlen[i] = 0;
        return;
    }
    host = host || !line_tabs(line, n, cfg.n_cols, lane, tabs);
    const uint32_t f0e = host ? 0 : tabs[0], f1e = host ? 0 : tabs[1];      // (n_cols >= 3: pg_gvcf_dev_config)
    int64_t pos = 0;
    const uint32_t pz = host ? 0 : pgg_pos_zeros(line + f0e + 1, (int64_t)f1e - (int64_t)f0e - 1);   // not in the row (str(int))
    host = host || !pgg_pos_plain(line + f0e + 1 + pz, (int64_t)f1e - (int64_t)f0e - 1 - (int64_t)pz, &pos);
    const uint32_t head = f1e - pz;                                        // bytes of CHROM \t POS in the row
    PgfCounts t = {};
    int cells = 0;
    if (!host) {
        bool bad = false;
        for (int j = lane; j < cfg.n_sel; j += 64) {
            uint32_t s, e;
            field_at(tabs, A.sel_col[j], cfg.n_cols, n, &s, &e);
            PgfGeno g;
            if (e - s > PGG_MAX_CELL_IN || pgg_classify(line + s, (int)(e - s), cfg.in_fmt, &g)) {
                bad = true;
                break;
            }
            pgf_add(g, &t);
            cells += pgg_cell_len(g) + 1;
        }
        host = __ballot(bad) != 0;                                         // (a cell the run stops on is worded by the host)
    }
    char ref = 0;
    if (!host && cfg.has_ref) {
        const int32_t s = line_scaffold(A.R.F, line, f0e, lane);
        host = s < 0 || pgg_ref_base(A.R, s, pos, &ref) != 0;
    }
    if (host) {
        if (!RENDER && lane == 0) { A.rlen[i] = 0; pg_raise_host(A.status, i); }
        return;
    }
    int32_t c[4];
    for (int b = 0; b < 4; ++b) c[b] = pg_wave_sum(t.c[b]);
    char al[PGG_MAX_ALLELES];
    const int nA = pgg_alleles(c, cfg.has_ref != 0, ref, al);
    if (!RENDER) {                                                         // CHROM \t POS, ID .. FORMAT, a tab and the text of every cell, \n
        cells = pg_wave_sum(cells);
        if (lane == 0) A.rlen[i] = head + 3u + (uint32_t)pgg_ref_alt_len(nA) + PGG_FIXED_LEN + (uint32_t)cells + 1u;
        return;
    }
    uint8_t *o = A.out + A.roff[i];
    for (uint32_t k = (uint32_t)lane; k < head; k += 64) o[k] = line[k <= f0e ? k : k + pz];
    char mid[24];
    const int ml = pgg_middle(al, nA, mid);
#pragma unroll
    for (int k = 0; k < 24; ++k)
        if (lane == k && k < ml) o[head + (uint32_t)k] = (uint8_t)mid[k];
    uint32_t at = head + (uint32_t)ml;
    char cell[2 * PGF_MAXA];
    for (int base = 0; base < cfg.n_sel; base += 64) {
        const int j = base + lane;
        int L = 0;
        if (j < cfg.n_sel) {
            uint32_t s, e;
            field_at(tabs, A.sel_col[j], cfg.n_cols, n, &s, &e);
            PgfGeno g;
            pgg_classify(line + s, (int)(e - s), cfg.in_fmt, &g);
            L = pgg_cell(g, al, nA, cell);
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

int check_slot(pg_ctx *c, int slot, const char *who) { return pg_line_check_slot(c, slot, c ? &c->gvcf : nullptr, who, "pg_gvcf_dev_config"); }

}  // namespace

extern "C" int pg_gvcf_dev_config(pg_ctx *c, const pg_gvcf_cfg *cfg, const int32_t *sel_col, const char *ref_names, const int64_t *name_off,
                                  const int64_t *seq_len, const int64_t *seq_off, const int32_t *table, uint32_t mask, int32_t n_seq,
                                  const uint8_t *seq, int64_t seq_bytes, int *taken_out) {
    if (!c || !cfg || !taken_out || cfg->n_sel < 0 || (cfg->n_sel && !sel_col) || n_seq < 0 || seq_bytes < 0 ||
        (cfg->has_ref && (n_seq < 1 || !ref_names || !name_off || !seq_len || !seq_off || !table || (mask & (mask + 1)) || (seq_bytes && !seq))))
        return pg_fail(PG_ERR_ARG, "pg_gvcf_dev_config: bad argument");
    *taken_out = 0;
    pg_ctx::GvcfDev &D = c->gvcf;
    D.configured = false;
    // the tab table of a line lives in LDS (4 bytes per field, one wavefront per block); a site has CHROM, POS and a cell at least
    if (cfg->n_cols < 3 || cfg->n_sel < 1 || (size_t)cfg->n_cols * 4 > 60 * 1024) return PG_OK;
    for (int j = 0; j < cfg->n_sel; ++j)
        if (sel_col[j] < 2 || sel_col[j] >= cfg->n_cols) return pg_fail(PG_ERR_ARG, "pg_gvcf_dev_config: a selected column outside the header");
    if (cfg->has_ref) {
        for (int32_t s = 0; s < n_seq; ++s)
            if (name_off[s + 1] < name_off[s] || seq_len[s] < 0 || seq_off[s] < 0 || seq_off[s] + seq_len[s] > seq_bytes)
                return pg_fail(PG_ERR_ARG, "pg_gvcf_dev_config: a sequence outside the uploaded bytes");
        for (uint32_t k = 0; k <= mask; ++k)
            if (table[k] >= n_seq) return pg_fail(PG_ERR_ARG, "pg_gvcf_dev_config: a table entry outside the names");
        if (seq_bytes > c->scratch_limit) {                        // the sequences stay resident beside the blocks
            *taken_out = -1;
            return PG_OK;
        }
    }
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream_up;
    HIPCHK(hipStreamSynchronize(st));
    int rc;
    if ((rc = D.sel_col.upload(sel_col, (size_t)cfg->n_sel, st)) != PG_OK) return rc;
    if (cfg->has_ref) {
        const size_t nb = (size_t)name_off[n_seq];
        if ((rc = D.names.upload(reinterpret_cast<const uint8_t *>(ref_names), std::max<size_t>(nb, 1), st)) != PG_OK ||
            (rc = D.name_off.upload(name_off, (size_t)n_seq + 1, st)) != PG_OK || (rc = D.seq_len.upload(seq_len, (size_t)n_seq, st)) != PG_OK ||
            (rc = D.seq_off.upload(seq_off, (size_t)n_seq, st)) != PG_OK || (rc = D.table.upload(table, (size_t)mask + 1, st)) != PG_OK ||
            (rc = D.seq.ensure((size_t)seq_bytes + 1)) != PG_OK)
            return rc;
        if (seq_bytes) HIPCHK(hipMemcpyAsync(D.seq.p, seq, (size_t)seq_bytes, hipMemcpyHostToDevice, st));
    }
    HIPCHK(hipStreamSynchronize(st));                              // (the tables: host memory that goes away)
    D.mask = mask;
    D.n_seq = cfg->has_ref ? n_seq : 0;
    D.cfg = *cfg;
    D.configured = true;
    *taken_out = 1;
    return PG_OK;
}

// A block of whole lines (the last byte a line feed, else the block is the host's) into text slot `slot`
extern "C" int pg_gvcf_dev_submit(pg_ctx *c, int slot, const char *text, int64_t len) {
    int rc = check_slot(c, slot, "pg_gvcf_dev_submit");
    return rc != PG_OK ? rc : pg_line_submit_plain(c, slot, c->gvcf.s[slot], text, len, "pg_gvcf_dev_submit");
}

// The same for a block that is still bgzipped: the members cross PCIe deflated, k_inflate writes their text behind `head` in the slot
// and lists its line feeds.  Whether the text ends in a line feed is read on the device once the line feeds are counted
extern "C" int pg_gvcf_dev_submit_bgzf(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                                       const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                                       int64_t text_len) {
    int rc = check_slot(c, slot, "pg_gvcf_dev_submit_bgzf");
    if (rc != PG_OK) return rc;
    if (text_len < 0) return pg_fail(PG_ERR_ARG, "pg_gvcf_dev_submit_bgzf: bad argument");
    return pg_line_submit_bgzf(c, slot, c->gvcf.s[slot], comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, 1024,
                               false, false);
}

// bgzf_members != 0: the rows of every block from now on are also deflated on the device (k_deflate: BGZF members of 65 280 bytes of
// rows, no end-of-file member); pg_gvcf_dev_collect reports their bytes, pg_gvcf_dev_rows_bgzf fetches them
extern "C" int pg_gvcf_dev_set_output(pg_ctx *c, int bgzf_members) {
    if (!c) return pg_fail(PG_ERR_ARG, "pg_gvcf_dev_set_output: null context");
    c->gvcf.bgzf_rows = bgzf_members != 0;
    return PG_OK;
}

namespace {

GvcfArgs gvcf_args(pg_ctx *c, int slot) {
    pg_ctx::GvcfDev &D = c->gvcf;
    pg_ctx::GvcfDev::Slot &G = D.s[slot];
    pg_ctx::TokSlot &T = c->tok[slot];
    GvcfArgs A;
    A.text = T.tp;
    A.nl = T.nl.p;
    A.n_lines = G.L.n_lines;
    A.sel_col = D.sel_col.p;
    A.R.F = pgm_fai{D.names.p, D.name_off.p, D.seq_len.p, D.table.p, D.mask, D.n_seq};
    A.R.seq = D.seq.p;
    A.R.seq_off = D.seq_off.p;
    A.rlen = G.rlen.p;
    A.roff = G.roff.p;
    A.out = G.out.p;
    A.status = reinterpret_cast<long long *>(G.status.p);
    return A;
}

// the rows' text (k_gvcf_lines<1>) and, for -o x.gz, their members (k_deflate), then the status back to the host (the block: queued)
int queue_render(pg_ctx *c, int slot, hipStream_t st) {
    pg_ctx::GvcfDev &D = c->gvcf;
    pg_ctx::GvcfDev::Slot &G = D.s[slot];
    const GvcfArgs A = gvcf_args(c, slot);
    hipLaunchKernelGGL((k_gvcf_lines<1>), dim3((unsigned)G.L.n_lines), dim3(64), (size_t)D.cfg.n_cols * 4, st, A, D.cfg);
    HIPCHK(hipGetLastError());
    if (D.bgzf_rows) {
        int rc = pg_deflate_queue(c, st, G.df, G.out.p, A.status + PGL_ST_BYTES, G.out_cap, A.status, A.status + PGL_ST_BGZF_BYTES);
        if (rc != PG_OK) return rc;
    }
    return pg_line_parse_end(c, G, st);
}

// rows longer than their room: room for `need` bytes of them (k_deflate reads 32 bytes past the rows), rendered once more
int render_again(pg_ctx *c, int slot, int64_t need, hipStream_t st) {
    pg_ctx::GvcfDev::Slot &G = c->gvcf.s[slot];
    int rc = G.out.ensure_roomy((size_t)need + 4096 + 64);
    if (rc != PG_OK) return rc;
    G.out_cap = (int64_t)G.out.cap - 64;
    return queue_render(c, slot, st);
}

}  // namespace

// Queues the kernels of the block in `slot` (waits for the number of its lines only)
extern "C" int pg_gvcf_dev_parse(pg_ctx *c, int slot) {
    int rc = check_slot(c, slot, "pg_gvcf_dev_parse");
    if (rc != PG_OK) return rc;
    pg_ctx::GvcfDev &D = c->gvcf;
    pg_ctx::GvcfDev::Slot &G = D.s[slot];
    int64_t n_lines = 0;
    bool nothing = true;
    if ((rc = pg_line_parse_begin(c, slot, G, &n_lines, &nothing, "pg_gvcf_dev_parse")) != PG_OK || nothing) return rc;
    if (n_lines > 0x7fffffffll) return pg_fail(PG_ERR_ARG, "pg_gvcf_dev_parse: more than 2^31 lines in a block");
    hipStream_t st = c->stream_up;
    pg_ctx::TokSlot &T = c->tok[slot];
    if ((rc = G.rlen.ensure_roomy((size_t)n_lines)) != PG_OK || (rc = G.roff.ensure_roomy((size_t)n_lines)) != PG_OK) return rc;
    // rows: a phased line's own size and ID .. FORMAT; pairs and diplo cells grow to three bytes, and their larger total grows the
    // buffer in collect
    G.out_cap = std::max<int64_t>(G.out_cap, T.len + n_lines * 32 + 4096);
    if ((rc = G.out.ensure_roomy((size_t)G.out_cap + 64)) != PG_OK) return rc;
    G.out_cap = (int64_t)G.out.cap - 64;                          // (k_deflate reads 32 bytes past the rows)
    if ((rc = pg_line_status_upload(G, st)) != PG_OK) return rc;
    const GvcfArgs A = gvcf_args(c, slot);
    hipLaunchKernelGGL((k_gvcf_lines<0>), dim3((unsigned)n_lines), dim3(64), (size_t)D.cfg.n_cols * 4, st, A, D.cfg);
    HIPCHK(hipGetLastError());
    pg_rows_scan_queue(st, G.rlen.p, n_lines, G.roff.p, A.status, G.out_cap);
    if ((rc = queue_render(c, slot, st)) != PG_OK) return rc;
    ++D.blocks;
    return PG_OK;
}

// Waits for the block's kernels.  *host_line_out < 0: the rows are ready (*rows_len_out bytes, *n_rows_out rows: pg_gvcf_dev_rows;
// *bgzf_len_out bytes of members: pg_gvcf_dev_rows_bgzf); else the block goes to the host route -- line *host_line_out is the first
// the device does not take.  Rows longer than the buffer (the scan knows their total) grow it and are rendered again.
extern "C" int pg_gvcf_dev_collect(pg_ctx *c, int slot, int64_t *rows_len_out, int64_t *n_rows_out, int64_t *host_line_out,
                                   int64_t *bgzf_len_out, int64_t *n_lines_out) {
    int rc = check_slot(c, slot, "pg_gvcf_dev_collect");
    if (rc != PG_OK) return rc;
    if (!rows_len_out || !n_rows_out || !host_line_out) return pg_fail(PG_ERR_ARG, "pg_gvcf_dev_collect: null argument");
    PgLineResult R;
    rc = pg_line_collect(c, slot, c->gvcf, c->gvcf.s[slot], c->gvcf.bgzf_rows, render_again, n_lines_out, &R, "pg_gvcf_dev_collect");
    *host_line_out = R.host_line;
    *rows_len_out = R.bytes;
    *n_rows_out = R.rows;
    if (bgzf_len_out) *bgzf_len_out = R.bgzf_bytes;
    return rc;
}

extern "C" int pg_gvcf_dev_rows(pg_ctx *c, int slot, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_gvcf_dev_rows");
    return rc != PG_OK ? rc : pg_line_rows(c, c->gvcf.s[slot].out, dst, len, "pg_gvcf_dev_rows: bad length");
}

extern "C" int pg_gvcf_dev_rows_bgzf(pg_ctx *c, int slot, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_gvcf_dev_rows_bgzf");
    return rc != PG_OK ? rc : pg_line_rows(c, c->gvcf.s[slot].df.comp, dst, len, "pg_gvcf_dev_rows_bgzf: bad length");
}

// the text of the collected block -> dst (a block that goes to the host route and whose text the host never had: BGZF)
extern "C" int pg_gvcf_dev_text(pg_ctx *c, int slot, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_gvcf_dev_text");
    return rc != PG_OK ? rc : pg_line_text(c, slot, 0, len, dst, "pg_gvcf_dev_text: bad length");
}

extern "C" int pg_gvcf_dev_stats(pg_ctx *c, int64_t *blocks_out, int64_t *host_blocks_out) {
    return pg_line_stats(c ? &c->gvcf : nullptr, blocks_out, host_blocks_out, "pg_gvcf_dev_stats");
}
