// Biallelic `.geno` sites written as EIGENSTRAT rows on the device: the genoToEigenstrat.py drop-in's route for the regular spelling of
// a line (fields split by single tabs, the header's number of fields, ASCII, a position of digits only, cells of at most nine alleles).
// The per-site and per-cell rules are csrc/pg_eig_core.h (the host route pg_eig_text in pg_eig.cpp runs the same functions); this
// file is the division of the work over the chip and the host side of the entry points.
//
//   k_eig_lines<0>  a wavefront per line: the line's tabs ranked by ballots into LDS (pg_line_fields.h), lanes strided over ALL sample
//                   columns classify their cells, the four base counts reduced across the wave; a site of exactly two bases is kept
//                   (pge_site: its alleles, the counted one); the scaffold's hash summed a lane a byte and looked up in the table over
//                   the --chromFile's names; the .snp row's size
//   scan            every kept line's rank (its .geno row lies at rank x (n_sel + 1)) and its .snp row's place (k_rows_scan, pg_line_slot.hip)
//   k_eig_lines<1>  a kept line again: lanes strided over the SELECTED columns write their digit; the .snp row: the site's index (the
//                   block's first plus the line's), the label, the position's text without its leading zeros, the two bases
// Two outputs per block: the .geno bytes follow from PGL_ST_ROWS, PGL_ST_BYTES counts the .snp bytes.  The text arrives in the
// tokenizer's text slot with its line feeds listed (pg_line_slot.h: submit, parse, collect).  A line outside the regular spelling, a
// '#' line, or a line the run stops on hands the BLOCK to the host route (pg_eig_dev_collect reports the line).
#include "pg_ctx.h"
#include "pg_eig_core.h"
#include "pg_line_fields.h"
#include "pg_wave.h"

#include <algorithm>
#include <cstring>

namespace {

#define PGE_MAX_CELL_IN (2 * PGE_DEV_ALLELES - 1)   // cell bytes the device takes (nine alleles phased)
#define PGE_MAX_LINE 0x3fffffffu                    // line bytes the device takes

struct EigArgs {
    const uint8_t *text;
    const int64_t *nl;
    int64_t n_lines, first_site;
    const int32_t *sel_col;
    pgm_fai F;
    const uint8_t *labels;
    const int64_t *label_off;
    uint32_t *rlen;
    uint8_t *site;       // a0 | a1 << 2 | counted << 4 of a kept line
    int32_t *entry;      // its label's entry
    int64_t *roff, *rank;
    uint8_t *snp, *geno;
    long long *status;
};

// a site's decision and its .snp row's size / both rows' text
template <int RENDER>
__global__ __launch_bounds__(64) void k_eig_lines(EigArgs A, PgeConfig cfg) {
    extern __shared__ uint32_t tabs[];
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= A.n_lines) return;
    if (RENDER && (A.rlen[i] == 0 || A.status[PGL_ST_BITS] != 0)) return;   // (a raised status: the block is the host's, its rows are not written)
    const int64_t ls = i ? A.nl[i - 1] + 1 : 0, le = A.nl[i];
    const uint8_t *line = A.text + ls;
    bool host = le - ls > (int64_t)PGE_MAX_LINE;
    const uint32_t n = host ? 0 : (uint32_t)(le - ls);
    host = host || (n > 0 && line[0] == '#');                              // no site, and none counted: the host route keeps the index
    host = host || !line_tabs(line, n, cfg.n_cols, lane, tabs);
    const uint32_t f0e = host ? 0 : tabs[0], f1e = host ? 0 : tabs[1];      // (n_cols >= 3: pg_eig_dev_config)
    int64_t pos = 0;
    const uint32_t pz = host ? 0 : pgg_pos_zeros(line + f0e + 1, (int64_t)f1e - (int64_t)f0e - 1);   // not in the row (str(int))
    host = host || !pgg_pos_plain(line + f0e + 1 + pz, (int64_t)f1e - (int64_t)f0e - 1 - (int64_t)pz, &pos);
    const uint32_t pos_len = f1e - f0e - 1 - pz;
    if (!RENDER) {
        PgfCounts t = {};
        if (!host) {
            bool bad = false;
            for (int c = 2 + lane; c < cfg.n_cols; c += 64) {              // every sample of the file
                uint32_t s, e;
                field_at(tabs, c, cfg.n_cols, n, &s, &e);
                PgfGeno g;
                if (e - s > PGE_MAX_CELL_IN || pgg_classify(line + s, (int)(e - s), cfg.in_fmt, &g) || g.n > PGE_DEV_ALLELES) {
                    bad = true;
                    break;
                }
                pgf_add(g, &t);
            }
            host = __ballot(bad) != 0;                                     // (a cell the run stops on is worded by the host)
        }
        if (host) {
            if (lane == 0) { A.rlen[i] = 0; pg_raise_host(A.status, i); }
            return;
        }
        int32_t c[4];
        for (int b = 0; b < 4; ++b) c[b] = pg_wave_sum(t.c[b]);
        PgeSite site;
        if (!pge_site(c, &site)) {
            if (lane == 0) A.rlen[i] = 0;
            return;
        }
        int32_t e = A.F.n ? line_scaffold(A.F, line, f0e, lane) : -1;
        if (e < 0) e = cfg.n_scaf;                                         // str(nullChrom)
        if (lane == 0) {
            A.rlen[i] = pge_snp_len(A.first_site + i, (uint32_t)(A.label_off[e + 1] - A.label_off[e]), pos_len);
            A.site[i] = (uint8_t)(site.a0 | (site.a1 << 2) | (site.counted << 4));
            A.entry[i] = e;
        }
        return;
    }
    if (host) return;                                                      // (not reached: the first run kept the line)
    const uint8_t sb = A.site[i];
    const int counted = (sb >> 4) & 3;
    uint8_t *gr = A.geno + A.rank[i] * (int64_t)(cfg.n_sel + 1);
    for (int j = lane; j < cfg.n_sel; j += 64) {                           // the selected samples
        uint32_t s, e;
        field_at(tabs, A.sel_col[j], cfg.n_cols, n, &s, &e);
        PgfGeno g;
        pgg_classify(line + s, (int)(e - s), cfg.in_fmt, &g);
        gr[j] = (uint8_t)('0' + pge_count(g, counted));
    }
    if (lane == 0) gr[cfg.n_sel] = '\n';
    uint8_t *o = A.snp + A.roff[i];
    char num[20];
    const int nd = pgg_pos_text(A.first_site + i, num);
#pragma unroll
    for (int k = 0; k < 20; ++k)
        if (lane == k && k < nd) o[k] = (uint8_t)num[k];
    uint32_t at = (uint32_t)nd;
    if (lane == 0) o[at] = '\t';
    ++at;
    const int32_t e = A.entry[i];
    const int64_t lo = A.label_off[e];
    const uint32_t ll = (uint32_t)(A.label_off[e + 1] - lo);
    for (uint32_t k = (uint32_t)lane; k < ll; k += 64) o[at + k] = A.labels[lo + k];
    at += ll;
    if (lane < 5) o[at + (uint32_t)lane] = (uint8_t)(lane == 0 || lane == 4 ? '\t' : lane == 2 ? '.' : '0');
    at += 5;
    for (uint32_t k = (uint32_t)lane; k < pos_len; k += 64) o[at + k] = line[f0e + 1 + pz + k];
    at += pos_len;
    if (lane < 5)
        o[at + (uint32_t)lane] = (uint8_t)(lane == 0 || lane == 2 ? '\t' : lane == 1 ? pge_base_char(sb & 3) : lane == 3 ? pge_base_char((sb >> 2) & 3) : '\n');
}

int check_slot(pg_ctx *c, int slot, const char *who) { return pg_line_check_slot(c, slot, c ? &c->eig : nullptr, who, "pg_eig_dev_config"); }

EigArgs eig_args(pg_ctx *c, int slot) {
    pg_ctx::EigDev &D = c->eig;
    pg_ctx::EigDev::Slot &E = D.s[slot];
    pg_ctx::TokSlot &T = c->tok[slot];
    EigArgs A;
    A.text = T.tp;
    A.nl = T.nl.p;
    A.n_lines = E.L.n_lines;
    A.first_site = E.first_site;
    A.sel_col = D.sel_col.p;
    A.F = pgm_fai{D.names.p, D.name_off.p, nullptr, D.table.p, D.mask, D.cfg.n_scaf};
    A.labels = D.labels.p;
    A.label_off = D.label_off.p;
    A.rlen = E.rlen.p;
    A.site = E.site.p;
    A.entry = E.entry.p;
    A.roff = E.roff.p;
    A.rank = E.rank.p;
    A.snp = E.snp.p;
    A.geno = E.geno.p;
    A.status = reinterpret_cast<long long *>(E.status.p);
    return A;
}

// both rows' text (k_eig_lines<1>), then the status back to the host (the block: queued)
int queue_render(pg_ctx *c, int slot, hipStream_t st) {
    pg_ctx::EigDev &D = c->eig;
    pg_ctx::EigDev::Slot &E = D.s[slot];
    const EigArgs A = eig_args(c, slot);
    hipLaunchKernelGGL((k_eig_lines<1>), dim3((unsigned)E.L.n_lines), dim3(64), (size_t)D.cfg.n_cols * 4, st, A, D.cfg);
    HIPCHK(hipGetLastError());
    return pg_line_parse_end(c, E, st);
}

// .snp rows longer than their room: room for `need` bytes of them, both rows' text once more
int render_again(pg_ctx *c, int slot, int64_t need, hipStream_t st) {
    pg_ctx::EigDev::Slot &E = c->eig.s[slot];
    int rc = E.snp.ensure_roomy((size_t)need + 4096);
    if (rc != PG_OK) return rc;
    E.snp_cap = (int64_t)E.snp.cap;
    return queue_render(c, slot, st);
}

}  // namespace

extern "C" int pg_eig_dev_config(pg_ctx *c, const pg_eig_cfg *cfg, const int32_t *sel_col, const char *names, const int64_t *name_off,
                                 const int32_t *table, uint32_t mask, const char *labels, const int64_t *label_off, int *taken_out) {
    if (!c || !cfg || !taken_out || cfg->n_sel < 0 || (cfg->n_sel && !sel_col) || cfg->n_scaf < 0 || !labels || !label_off ||
        (cfg->n_scaf && (!names || !name_off || !table || (mask & (mask + 1)) || (uint64_t)mask + 1 < 2ull * (uint64_t)cfg->n_scaf)))
        return pg_fail(PG_ERR_ARG, "pg_eig_dev_config: bad argument");
    *taken_out = 0;
    pg_ctx::EigDev &D = c->eig;
    D.configured = false;
    // the offsets of --cumulativePos are a walk over the kept sites in file order: the host route's.  The tab table of a line lives in
    // LDS (4 bytes per field, one wavefront per block); a site has a scaffold, a position and a cell at least
    if (cfg->cumulative || cfg->n_cols < 3 || cfg->n_sel < 1 || (size_t)cfg->n_cols * 4 > 60 * 1024) return PG_OK;
    for (int j = 0; j < cfg->n_sel; ++j)
        if (sel_col[j] < 2 || sel_col[j] >= cfg->n_cols) return pg_fail(PG_ERR_ARG, "pg_eig_dev_config: a selected column outside the header");
    if (cfg->n_scaf > PG_EIG_MAX_SCAF) {
        *taken_out = -1;
        return PG_OK;
    }
    for (int32_t e = 0; e <= cfg->n_scaf; ++e) {
        if (label_off[e + 1] < label_off[e] || (e < cfg->n_scaf && name_off[e + 1] < name_off[e]))
            return pg_fail(PG_ERR_ARG, "pg_eig_dev_config: offsets that do not rise");
        if (label_off[e + 1] - label_off[e] > PG_EIG_MAX_LABEL) {
            *taken_out = -1;
            return PG_OK;
        }
    }
    if (cfg->n_scaf)
        for (uint32_t k = 0; k <= mask; ++k)
            if (table[k] >= cfg->n_scaf) return pg_fail(PG_ERR_ARG, "pg_eig_dev_config: a table entry outside the names");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream_up;
    HIPCHK(hipStreamSynchronize(st));
    int rc;
    const size_t lb = (size_t)label_off[cfg->n_scaf + 1];
    if ((rc = D.sel_col.upload(sel_col, (size_t)cfg->n_sel, st)) != PG_OK ||
        (rc = D.labels.upload(reinterpret_cast<const uint8_t *>(labels), std::max<size_t>(lb, 1), st)) != PG_OK ||
        (rc = D.label_off.upload(label_off, (size_t)cfg->n_scaf + 2, st)) != PG_OK)
        return rc;
    if (cfg->n_scaf) {
        const size_t nb = (size_t)name_off[cfg->n_scaf];
        if ((rc = D.names.upload(reinterpret_cast<const uint8_t *>(names), std::max<size_t>(nb, 1), st)) != PG_OK ||
            (rc = D.name_off.upload(name_off, (size_t)cfg->n_scaf + 1, st)) != PG_OK || (rc = D.table.upload(table, (size_t)mask + 1, st)) != PG_OK)
            return rc;
    }
    HIPCHK(hipStreamSynchronize(st));                              // (the tables: host memory that goes away)
    D.mask = mask;
    D.cfg = *cfg;
    D.configured = true;
    *taken_out = 1;
    return PG_OK;
}

// A block of whole lines (the last byte a line feed, else the block is the host's) into text slot `slot`
extern "C" int pg_eig_dev_submit(pg_ctx *c, int slot, const char *text, int64_t len) {
    int rc = check_slot(c, slot, "pg_eig_dev_submit");
    return rc != PG_OK ? rc : pg_line_submit_plain(c, slot, c->eig.s[slot], text, len, "pg_eig_dev_submit");
}

// The same for a block that is still bgzipped: the members cross PCIe deflated, k_inflate writes their text behind `head` in the slot
// and lists its line feeds.  Whether the text ends in a line feed is read on the device once the line feeds are counted
extern "C" int pg_eig_dev_submit_bgzf(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                                      const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                                      int64_t text_len) {
    int rc = check_slot(c, slot, "pg_eig_dev_submit_bgzf");
    if (rc != PG_OK) return rc;
    if (text_len < 0) return pg_fail(PG_ERR_ARG, "pg_eig_dev_submit_bgzf: bad argument");
    return pg_line_submit_bgzf(c, slot, c->eig.s[slot], comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, 1024,
                               false, false);
}

// Queues the kernels of the block in `slot` (waits for the number of its lines only).  first_site: the sites in front of the block
extern "C" int pg_eig_dev_parse(pg_ctx *c, int slot, int64_t first_site, int64_t *n_lines_out) {
    int rc = check_slot(c, slot, "pg_eig_dev_parse");
    if (rc != PG_OK) return rc;
    if (first_site < 0 || !n_lines_out) return pg_fail(PG_ERR_ARG, "pg_eig_dev_parse: bad argument");
    pg_ctx::EigDev &D = c->eig;
    pg_ctx::EigDev::Slot &E = D.s[slot];
    int64_t n_lines = 0;
    bool nothing = true;
    *n_lines_out = 0;
    rc = pg_line_parse_begin(c, slot, E, &n_lines, &nothing, "pg_eig_dev_parse");
    *n_lines_out = n_lines;
    if (rc != PG_OK || nothing) return rc;
    if (n_lines > 0x7fffffffll) return pg_fail(PG_ERR_ARG, "pg_eig_dev_parse: more than 2^31 lines in a block");
    hipStream_t st = c->stream_up;
    E.first_site = first_site;
    const size_t nl = (size_t)n_lines;
    if ((rc = E.rlen.ensure_roomy(nl)) != PG_OK || (rc = E.roff.ensure_roomy(nl)) != PG_OK || (rc = E.rank.ensure_roomy(nl)) != PG_OK ||
        (rc = E.site.ensure_roomy(nl)) != PG_OK || (rc = E.entry.ensure_roomy(nl)) != PG_OK ||
        (rc = E.geno.ensure_roomy(nl * ((size_t)D.cfg.n_sel + 1))) != PG_OK)     // every line kept: the .geno rows never outgrow this
        return rc;
    // .snp rows: an index, a label of a few characters, a position; longer labels make a larger total, which grows the buffer in collect
    E.snp_cap = std::max<int64_t>(E.snp_cap, n_lines * 32 + 256);
    if ((rc = E.snp.ensure_roomy((size_t)E.snp_cap)) != PG_OK) return rc;
    E.snp_cap = (int64_t)E.snp.cap;
    if ((rc = pg_line_status_upload(E, st)) != PG_OK) return rc;
    const EigArgs A = eig_args(c, slot);
    hipLaunchKernelGGL((k_eig_lines<0>), dim3((unsigned)n_lines), dim3(64), (size_t)D.cfg.n_cols * 4, st, A, D.cfg);
    HIPCHK(hipGetLastError());
    pg_rows_scan_queue(st, E.rlen.p, n_lines, E.roff.p, A.status, E.snp_cap, E.rank.p);
    if ((rc = queue_render(c, slot, st)) != PG_OK) return rc;
    ++D.blocks;
    return PG_OK;
}

// Waits for the block's kernels.  *host_line_out < 0: the rows are ready (*n_rows_out rows: their .geno rows are n_sel + 1 bytes each,
// their .snp rows *snp_len_out bytes: pg_eig_dev_rows); else the block goes to the host route -- line *host_line_out is the first the
// device does not take.  .snp rows longer than the buffer (the scan knows their total) grow it and are rendered again.
extern "C" int pg_eig_dev_collect(pg_ctx *c, int slot, int64_t *snp_len_out, int64_t *n_rows_out, int64_t *host_line_out, int64_t *n_lines_out) {
    int rc = check_slot(c, slot, "pg_eig_dev_collect");
    if (rc != PG_OK) return rc;
    if (!snp_len_out || !n_rows_out || !host_line_out) return pg_fail(PG_ERR_ARG, "pg_eig_dev_collect: null argument");
    PgLineResult R;
    rc = pg_line_collect(c, slot, c->eig, c->eig.s[slot], false, render_again, n_lines_out, &R, "pg_eig_dev_collect");
    *host_line_out = R.host_line;
    *snp_len_out = R.bytes;
    *n_rows_out = R.rows;
    return rc;
}

extern "C" int pg_eig_dev_rows(pg_ctx *c, int slot, int which, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_eig_dev_rows");
    if (rc != PG_OK) return rc;
    if (which < 0 || which > 1) return pg_fail(PG_ERR_ARG, "pg_eig_dev_rows: bad length");
    return pg_line_rows(c, which ? c->eig.s[slot].snp : c->eig.s[slot].geno, dst, len, "pg_eig_dev_rows: bad length");
}

// the text of the collected block -> dst (a block that goes to the host route and whose text the host never had: BGZF)
extern "C" int pg_eig_dev_text(pg_ctx *c, int slot, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_eig_dev_text");
    return rc != PG_OK ? rc : pg_line_text(c, slot, 0, len, dst, "pg_eig_dev_text: bad length");
}

extern "C" int pg_eig_dev_stats(pg_ctx *c, int64_t *blocks_out, int64_t *host_blocks_out) {
    return pg_line_stats(c ? &c->eig : nullptr, blocks_out, host_blocks_out, "pg_eig_dev_stats");
}
