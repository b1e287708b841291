// `.geno` lines turned into sequences on the device: the genoToSeq.py drop-in's route for the regular spelling of a line (fields split
// by single tabs, the header's number of fields, ASCII; every selected cell 2 * ploidy - 1 characters long under --splitPhased, one
// character otherwise).  The per-line and per-cell rules are csrc/pg_seq_core.h (the host route pg_seq_text in pg_seq.cpp runs the same
// functions); this file is the division of the work over the chip and the host side of the entry points.
//
//   k_seq_lines  a wavefront per line: '#' lines marked, the line's tabs ranked by ballots into LDS, the field count against the
//                header's, a lane per output sequence checks its cell's length, the position as int64, whether the scaffold differs
//                from the site's before
//   scan         the kept lines' row indices (k_rows_scan, pg_line_slot.hip)
//   k_seq_rows   a thread per line: the sites' records gathered at their rows (line, position, run flag, where the line begins)
//   k_seq_tile   the transpose: a workgroup takes PGS_TILE_LINES consecutive sites and a tile of output sequences; each of its waves
//                reads a line in 64-byte steps, ranks its tabs, a lane per sequence puts the sequence's character into the LDS tile
//                (pitch PGS_TILE_PITCH); then every thread takes 16 bytes of one sequence from the tile and stores them to
//                out[q][site0 ..] in one piece -- 128 contiguous bytes per sequence and tile.  --NtoGap is applied on the way
// The text arrives in the tokenizer's text slot with its line feeds listed (pg_tok_text_submit / pg_tok_lines).  A line outside the
// regular spelling, or one on which the reference raises, hands the BLOCK to the host route (pg_seq_dev_collect reports the line).
#include "pg_ctx.h"
#include "pg_seq_core.h"
#include "pg_wave.h"

#include <algorithm>
#include <cstring>

namespace {

#define PGS_LDS_BYTES (64 * 1024)   // what a workgroup of k_seq_tile may use: four tab tables and the tile
#define PGS_TILE_THREADS 256

struct SeqArgs {
    const uint8_t *text;
    const int64_t *nl;
    int64_t n_lines, pitch;
    const int32_t *sel_col, *sel_off, *sel_len;
    uint32_t *keep;
    uint8_t *runf, *rrun, *out;
    int64_t *row, *pos, *rpos, *rstart, *line_of;
    long long *status;
    int tile_seqs;
};

// the line's tabs into LDS (tabs[k]: the offset of tab k); false when the line is not of the regular spelling (the host's then).  The
// same rule as line_tabs of pg_filter_dev.hip, kept apart from it: that file stays as it is
__device__ bool seq_line_tabs(const uint8_t *line, uint32_t n, int n_cols, int lane, uint32_t *tabs, bool check) {
    uint32_t ntab = 0;
    bool irr = n == 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t k = base + (uint32_t)lane;
        const uint8_t b = k < n ? line[k] : (uint8_t)'x';
        const bool tab = k < n && b == '\t';
        const uint64_t m = __ballot(tab);
        if (tab) {
            const uint32_t idx = ntab + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (idx < (uint32_t)(n_cols - 1)) tabs[idx] = k;
        }
        ntab += (uint32_t)__popcll(m);
        if (check) irr = irr || __ballot(k < n && pgs_irregular(b)) != 0;
    }
    __syncthreads();
    if (!check) return true;
    if (irr || ntab != (uint32_t)(n_cols - 1)) return false;
    bool empty = false;
    for (int c = lane; c < n_cols; c += 64) {
        const uint32_t s = c ? tabs[c - 1] + 1 : 0, e = c < n_cols - 1 ? tabs[c] : n;
        empty = empty || e <= s;
    }
    return __ballot(empty) == 0;
}

__device__ inline void seq_line_at(const SeqArgs &A, int64_t i, int64_t *ls, int64_t *le) {
    *ls = i ? A.nl[i - 1] + 1 : 0;
    *le = A.nl[i];
}

__global__ __launch_bounds__(64) void k_seq_lines(SeqArgs A, pg_seq_cfg cfg) {
    extern __shared__ uint32_t tabs[];
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= A.n_lines) return;
    int64_t ls, le;
    seq_line_at(A, i, &ls, &le);
    const uint8_t *line = A.text + ls;
    if (le > ls && line[0] == '#') {                              // genomics.py:1936, 1943
        if (lane == 0) { A.keep[i] = 0; A.runf[i] = 0; A.pos[i] = 0; }
        return;
    }
    bool host = le - ls > 0x7fffffffll;
    const uint32_t n = host ? 0 : (uint32_t)(le - ls);
    host = host || !seq_line_tabs(line, n, cfg.n_cols, lane, tabs, true);
    if (!host) {
        bool bad = false;
        for (int q = lane; q < cfg.n_seq; q += 64) {
            const int c = A.sel_col[q];
            const uint32_t s = tabs[c - 1] + 1, e = c < cfg.n_cols - 1 ? tabs[c] : n;
            bad = bad || pgs_cell_width(e - s, cfg.split ? A.sel_len[q] : 1) != 1;
        }
        host = __ballot(bad) != 0;
    }
    int64_t pos = 0;
    uint8_t run = 1;
    if (!host) {
        const uint32_t f0e = tabs[0], f1s = tabs[0] + 1, f1e = cfg.n_cols > 2 ? tabs[1] : n;
        host = pgs_parse_pos(line + f1s, (int64_t)(f1e - f1s), &pos) != 0;
        // the site before: the nearest line above that is no '#' line (none: the block's first site opens a run)
        int64_t j = i - 1, ps = 0, pe = 0;
        for (; j >= 0; --j) {
            seq_line_at(A, j, &ps, &pe);
            if (!(pe > ps && A.text[ps] == '#')) break;
        }
        if (j >= 0 && pe - ps > (int64_t)f0e) {
            const uint8_t *prev = A.text + ps;
            bool differ = false;
            for (uint32_t k = (uint32_t)lane; k <= f0e; k += 64) differ = differ || (k < f0e ? prev[k] != line[k] : prev[k] != '\t');
            run = __ballot(differ) != 0;
        }
    }
    if (lane == 0) {
        A.keep[i] = host ? 0 : 1;
        A.runf[i] = run;
        A.pos[i] = pos;
        if (host) pg_raise_host(A.status, i);
    }
}

__global__ __launch_bounds__(256) void k_seq_rows(SeqArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_lines || !A.keep[i] || A.status[0] != 0) return;
    const int64_t r = A.row[i];
    A.line_of[r] = i;
    A.rpos[r] = A.pos[i];
    A.rrun[r] = A.runf[i];
    A.rstart[r] = i ? A.nl[i - 1] + 1 : 0;
}

__global__ __launch_bounds__(PGS_TILE_THREADS) void k_seq_tile(SeqArgs A, pg_seq_cfg cfg) {
    extern __shared__ uint32_t lds[];
    if (A.status[0] != 0) return;                                 // (the block is the host's)
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    int64_t site0, q0;
    const int ns = (int)pgs_tile_count(A.status[3], PGS_TILE_LINES, blockIdx.x, &site0);
    const int nq = (int)pgs_tile_count(cfg.n_seq, A.tile_seqs, blockIdx.y, &q0);
    if (ns == 0 || nq == 0) return;
    uint32_t *tabs = lds + (size_t)wave * (size_t)cfg.n_cols;
    uint8_t *tile = reinterpret_cast<uint8_t *>(lds + 4 * (size_t)cfg.n_cols);
    // (1) the lines of the tile, a wave each in turn: tabs ranked, a lane per sequence takes its character
    for (int it = 0; it < PGS_TILE_LINES / 4; ++it) {
        const int l = it * 4 + wave;
        const bool live = l < ns;
        int64_t ls = 0, le = 0;
        if (live) seq_line_at(A, A.line_of[site0 + l], &ls, &le);
        const uint8_t *line = A.text + ls;
        seq_line_tabs(line, (uint32_t)(le - ls), cfg.n_cols, lane, tabs, false);   // (k_seq_lines checked the spelling; syncs inside)
        if (live)
            for (int qq = lane; qq < nq; qq += 64) {
                const int q = (int)q0 + qq;
                tile[(size_t)qq * PGS_TILE_PITCH + (size_t)l] = pgs_map(line[tabs[A.sel_col[q] - 1] + 1 + (uint32_t)A.sel_off[q]], cfg.n_to_gap);
            }
        __syncthreads();
    }
    // (2) 16 bytes of one sequence per thread: four words out of the tile, one store (bytes at the matrix's edge)
    const int segs = PGS_TILE_LINES / PGS_STORE;
    for (int item = (int)threadIdx.x; item < nq * segs; item += PGS_TILE_THREADS) {
        const int qq = item / segs, seg = item % segs;
        const int nb = pgs_store_bytes(ns, seg);
        if (nb == 0) continue;
        const uint32_t *w = reinterpret_cast<const uint32_t *>(tile + (size_t)qq * PGS_TILE_PITCH + (size_t)seg * PGS_STORE);
        uint8_t *dst = A.out + (size_t)(q0 + qq) * (size_t)A.pitch + (size_t)site0 + (size_t)seg * PGS_STORE;
        const uint4 v = make_uint4(w[0], w[1], w[2], w[3]);
        if (nb == PGS_STORE) {
            *reinterpret_cast<uint4 *>(dst) = v;
        } else {
            const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
            for (int k = 0; k < nb; ++k) dst[k] = (uint8_t)(vv[k >> 2] >> (8 * (k & 3)));
        }
    }
}

int check_slot(pg_ctx *c, int slot, const char *who) { return pg_line_check_slot(c, slot, c ? &c->seq : nullptr, who, "pg_seq_dev_config"); }

SeqArgs seq_args(pg_ctx *c, int slot) {
    pg_ctx::SeqDev &D = c->seq;
    pg_ctx::SeqDev::Slot &Q = D.s[slot];
    pg_ctx::TokSlot &T = c->tok[slot];
    SeqArgs A;
    A.text = T.tp;
    A.nl = T.nl.p;
    A.n_lines = Q.L.n_lines;
    A.pitch = Q.pitch;
    A.sel_col = D.sel_col.p;
    A.sel_off = D.sel_off.p;
    A.sel_len = D.sel_len.p;
    A.keep = Q.keep.p;
    A.runf = Q.runf.p;
    A.rrun = Q.rrun.p;
    A.out = Q.out.p;
    A.row = Q.row.p;
    A.pos = Q.pos.p;
    A.rpos = Q.rpos.p;
    A.rstart = Q.rstart.p;
    A.line_of = Q.line_of.p;
    A.status = reinterpret_cast<long long *>(Q.status.p);
    A.tile_seqs = D.tile_seqs;
    return A;
}

}  // namespace

extern "C" int pg_seq_dev_config(pg_ctx *c, const pg_seq_cfg *cfg, const int32_t *sel_col, const int32_t *sel_off, const int32_t *sel_len,
                                 int tile_seqs, int *taken_out) {
    if (!c || !cfg || !taken_out || cfg->n_seq < 1 || cfg->n_cols < 3 || !sel_col || !sel_off || !sel_len || tile_seqs < 0)
        return pg_fail(PG_ERR_ARG, "pg_seq_dev_config: bad argument");
    // what k_seq_tile reads without looking again: a column of the header behind the position, an offset inside the demanded cell
    for (int q = 0; q < cfg->n_seq; ++q)
        if (sel_col[q] < 2 || sel_col[q] >= cfg->n_cols || sel_off[q] < 0 || sel_len[q] < 0 || (cfg->split ? sel_off[q] >= sel_len[q] : sel_off[q] != 0))
            return pg_fail(PG_ERR_ARG, "pg_seq_dev_config: sequence %d: column %d, offset %d, cell length %d", q, sel_col[q], sel_off[q], sel_len[q]);
    *taken_out = 0;
    pg_ctx::SeqDev &D = c->seq;
    D.configured = false;
    const int tq = pgs_tile_seqs(cfg->n_cols, cfg->n_seq, tile_seqs, PGS_LDS_BYTES);
    if (tq == 0) return PG_OK;                                    // (a header too wide for four tab tables in LDS)
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    const size_t ns = (size_t)cfg->n_seq;
    int rc;
    if ((rc = D.sel_col.ensure(ns)) != PG_OK || (rc = D.sel_off.ensure(ns)) != PG_OK || (rc = D.sel_len.ensure(ns)) != PG_OK) return rc;
    HIPCHK(hipMemcpy(D.sel_col.p, sel_col, ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.sel_off.p, sel_off, ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.sel_len.p, sel_len, ns * 4, hipMemcpyHostToDevice));
    D.cfg = *cfg;
    D.tile_seqs = tq;
    D.configured = true;
    *taken_out = 1;
    return PG_OK;
}

// A block of whole lines (the last byte a line feed, else the block is the host's) into text slot `slot`
extern "C" int pg_seq_dev_submit(pg_ctx *c, int slot, const char *text, int64_t len) {
    int rc = check_slot(c, slot, "pg_seq_dev_submit");
    return rc != PG_OK ? rc : pg_line_submit_plain(c, slot, c->seq.s[slot], text, len, "pg_seq_dev_submit");
}

// The same for a block that is still bgzipped: the members cross PCIe deflated, k_inflate writes their text behind `head` in the slot
// and lists its line feeds (pg_tok_bgzf_submit).  Whether the text ends in a line feed is read on the device once the line feeds are
// counted (the file's last block may not).
extern "C" int pg_seq_dev_submit_bgzf(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                                      const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                                      int64_t text_len) {
    int rc = check_slot(c, slot, "pg_seq_dev_submit_bgzf");
    if (rc != PG_OK) return rc;
    if (text_len < 0) return pg_fail(PG_ERR_ARG, "pg_seq_dev_submit_bgzf: bad argument");
    return pg_line_submit_bgzf(c, slot, c->seq.s[slot], comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, 1024,
                               false, false);
}

// Queues the kernels of the block in `slot` (waits for the number of its lines only)
extern "C" int pg_seq_dev_parse(pg_ctx *c, int slot) {
    int rc = check_slot(c, slot, "pg_seq_dev_parse");
    if (rc != PG_OK) return rc;
    pg_ctx::SeqDev &D = c->seq;
    pg_ctx::SeqDev::Slot &Q = D.s[slot];
    // a block without a final line feed (the file's partial last line) is the host's
    int64_t n_lines = 0;
    bool nothing = true;
    if ((rc = pg_line_parse_begin(c, slot, Q, &n_lines, &nothing, "pg_seq_dev_parse")) != PG_OK || Q.L.state == PGL_EMPTY) return rc;
    Q.pitch = pgs_pitch(n_lines);
    Q.timed = false;
    if (nothing) return PG_OK;
    hipStream_t st = c->stream_up;
    const size_t nl = (size_t)n_lines;
    if ((rc = Q.keep.ensure_roomy(nl)) != PG_OK || (rc = Q.runf.ensure_roomy(nl)) != PG_OK || (rc = Q.rrun.ensure_roomy(nl)) != PG_OK ||
        (rc = Q.row.ensure_roomy(nl)) != PG_OK || (rc = Q.pos.ensure_roomy(nl)) != PG_OK || (rc = Q.rpos.ensure_roomy(nl)) != PG_OK ||
        (rc = Q.rstart.ensure_roomy(nl)) != PG_OK || (rc = Q.line_of.ensure_roomy(nl)) != PG_OK ||
        (rc = Q.out.ensure_roomy((size_t)D.cfg.n_seq * (size_t)Q.pitch)) != PG_OK)
        return rc;
    if (D.timing) {
        for (hipEvent_t *e : {&Q.t0, &Q.t1, &Q.t2, &Q.t3})
            if (!*e) HIPCHK(hipEventCreate(e));
    }
    if ((rc = pg_line_status_upload(Q, st)) != PG_OK) return rc;
    // the matrix's pad bytes (behind the last site of a sequence, up to the pitch) are zero whatever the slot held before
    HIPCHK(hipMemsetAsync(Q.out.p, 0, (size_t)D.cfg.n_seq * (size_t)Q.pitch, st));
    const SeqArgs A = seq_args(c, slot);
    if (D.timing) HIPCHK(hipEventRecord(Q.t0, st));
    hipLaunchKernelGGL(k_seq_lines, dim3((unsigned)n_lines), dim3(64), (size_t)D.cfg.n_cols * 4, st, A, D.cfg);
    HIPCHK(hipGetLastError());
    if (D.timing) HIPCHK(hipEventRecord(Q.t1, st));
    // the kept lines' rows: the scan of the 0 / 1 flags; their number lands in status[3] (and, as a sum of ones, in status[2])
    pg_rows_scan_queue(st, Q.keep.p, n_lines, Q.row.p, A.status, 0x7fffffffffffffffll);
    hipLaunchKernelGGL(k_seq_rows, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, st, A);
    HIPCHK(hipGetLastError());
    const unsigned tiles = (unsigned)(Q.pitch / PGS_TILE_LINES), qtiles = (unsigned)((D.cfg.n_seq + D.tile_seqs - 1) / D.tile_seqs);
    const size_t lds = (size_t)D.cfg.n_cols * 16 + (size_t)D.tile_seqs * PGS_TILE_PITCH;
    if (D.timing) HIPCHK(hipEventRecord(Q.t2, st));
    hipLaunchKernelGGL(k_seq_tile, dim3(tiles, qtiles), dim3(PGS_TILE_THREADS), lds, st, A, D.cfg);
    HIPCHK(hipGetLastError());
    if (D.timing) {
        HIPCHK(hipEventRecord(Q.t3, st));
        Q.timed = true;
    }
    if ((rc = pg_line_parse_end(c, Q, st)) != PG_OK) return rc;
    ++D.blocks;
    return PG_OK;
}

extern "C" int pg_seq_dev_collect(pg_ctx *c, int slot, int64_t *n_sites_out, int64_t *host_line_out, int64_t *n_lines_out, int64_t *pitch_out) {
    int rc = check_slot(c, slot, "pg_seq_dev_collect");
    if (rc != PG_OK) return rc;
    if (!n_sites_out || !host_line_out) return pg_fail(PG_ERR_ARG, "pg_seq_dev_collect: null argument");
    pg_ctx::SeqDev::Slot &Q = c->seq.s[slot];
    const bool empty = Q.L.state == PGL_EMPTY;
    PgLineResult R;
    rc = pg_line_collect(c, slot, c->seq, Q, false, nullptr, n_lines_out, &R, "pg_seq_dev_collect");
    *host_line_out = R.host_line;
    *n_sites_out = R.rows;
    if (pitch_out) *pitch_out = rc == PG_OK && !empty ? Q.pitch : 0;
    if (rc != PG_OK || empty || !Q.timed) return rc;
    float a = 0, b = 0;
    Q.timed = false;
    HIPCHK(hipEventElapsedTime(&a, Q.t0, Q.t1));
    HIPCHK(hipEventElapsedTime(&b, Q.t2, Q.t3));
    c->seq.lines_ms += a;
    c->seq.tile_ms += b;
    return PG_OK;
}

extern "C" int pg_seq_dev_rows(pg_ctx *c, int slot, int q0, int q1, uint8_t *dst, int64_t dst_pitch, int64_t width) {
    int rc = check_slot(c, slot, "pg_seq_dev_rows");
    if (rc != PG_OK) return rc;
    pg_ctx::SeqDev::Slot &Q = c->seq.s[slot];
    if (q0 < 0 || q1 < q0 || q1 > c->seq.cfg.n_seq || width < 0 || width > Q.pitch || dst_pitch < width || (size_t)c->seq.cfg.n_seq * (size_t)Q.pitch > Q.out.cap ||
        (q1 > q0 && width && !dst))
        return pg_fail(PG_ERR_ARG, "pg_seq_dev_rows: bad range or width");
    if (q1 == q0 || width == 0) return PG_OK;
    HIPCHK(hipSetDevice(c->device));
    if ((rc = pg_small_stream(c)) != PG_OK) return rc;
    HIPCHK(hipMemcpy2DAsync(dst, (size_t)dst_pitch, Q.out.p + (size_t)q0 * (size_t)Q.pitch, (size_t)Q.pitch, (size_t)width, (size_t)(q1 - q0),
                            hipMemcpyDeviceToHost, c->tok_small));
    HIPCHK(hipStreamSynchronize(c->tok_small));
    return PG_OK;
}

extern "C" int pg_seq_dev_meta(pg_ctx *c, int slot, int64_t *pos_dst, uint8_t *run_dst, int64_t *start_dst) {
    int rc = check_slot(c, slot, "pg_seq_dev_meta");
    if (rc != PG_OK) return rc;
    pg_ctx::SeqDev::Slot &Q = c->seq.s[slot];
    const int64_t n = Q.h_status.p ? Q.h_status.p[PGL_ST_ROWS] : 0;
    if (Q.h_status.p && Q.h_status.p[PGL_ST_BITS]) return pg_fail(PG_ERR_STATE, "pg_seq_dev_meta: the block in slot %d is the host's", slot);
    if (n < 0 || (size_t)n > Q.rpos.cap) return pg_fail(PG_ERR_STATE, "pg_seq_dev_meta: nothing collected in slot %d", slot);
    if (n == 0) return PG_OK;
    if (!pos_dst || !run_dst || !start_dst) return pg_fail(PG_ERR_ARG, "pg_seq_dev_meta: null argument");
    if ((rc = pg_copy_back(c, pos_dst, Q.rpos.p, n * 8)) != PG_OK || (rc = pg_copy_back(c, run_dst, Q.rrun.p, n)) != PG_OK) return rc;
    return pg_copy_back(c, start_dst, Q.rstart.p, n * 8);
}

// bytes [off, off + len) of the collected block's text (a run's scaffold name; the whole block when it goes to the host route and the
// host never had its text: BGZF)
extern "C" int pg_seq_dev_text(pg_ctx *c, int slot, int64_t off, int64_t len, uint8_t *dst) {
    int rc = check_slot(c, slot, "pg_seq_dev_text");
    return rc != PG_OK ? rc : pg_line_text(c, slot, off, len, dst, "pg_seq_dev_text: bad range");
}

extern "C" int pg_seq_dev_timing(pg_ctx *c, int on) {
    if (!c) return pg_fail(PG_ERR_ARG, "pg_seq_dev_timing: null context");
    c->seq.timing = on != 0;
    return PG_OK;
}

extern "C" int pg_seq_dev_stats(pg_ctx *c, int64_t *blocks_out, int64_t *host_blocks_out, double *lines_ms_out, double *tile_ms_out) {
    int rc = pg_line_stats(c ? &c->seq : nullptr, blocks_out, host_blocks_out, "pg_seq_dev_stats");
    if (rc != PG_OK) return rc;
    if (lines_ms_out) *lines_ms_out = c->seq.lines_ms;
    if (tile_ms_out) *tile_ms_out = c->seq.tile_ms;
    return PG_OK;
}
