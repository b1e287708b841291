// `.geno` sites written as PED rows and MAP lines on the device: the genoToPlink.py drop-in's route for the regular spelling of a line
// (fields split by single tabs, the header's number of fields, ASCII, a position of digits only) whose selected cells have the
// configured lengths -- the file's first site sets them, sample by sample.  The per-cell rules are csrc/pg_ped_core.h (the host route
// pg_ped_text in pg_ped.cpp runs the same functions); this file is the division of the work over the chip and the host side of the
// entry points.
//
//   k_ped_lines  a wavefront per line: '#' lines marked, the line's tabs ranked by ballots into LDS, the field count against the
//                header's, lanes strided over the selected columns check their cell's length against the sample's (and its letter
//                under -f diplo), the position, whether the scaffold differs from the site's before, the .map row's size
//   scans        the kept lines' row indices, the .map rows' places (k_rows_scan, pg_line_slot.hip)
//   k_ped_map    a wavefront per kept line: its record at its row (where the line begins, the run flag), its .map row
//   k_ped_tile   the transpose: a workgroup takes PGP_TILE_LINES consecutive sites and a tile of samples; each of its waves reads a
//                line in 64-byte steps, ranks its tabs, a lane per sample expands the sample's cell into its 2 a_q bytes (allele,
//                blank) in the LDS tile; then every thread takes 16 bytes of one sample from the tile and stores them to the
//                sample's row in one piece -- 512 contiguous bytes per diploid sample and tile
// The matrix: sample q's row of 2 a_q bytes a site begins at woff[q] x pitch (woff: the bytes a site takes in the samples before).
// Two outputs per block: the matrix follows from PGL_ST_ROWS, PGL_ST_BYTES counts the .map bytes.  A line outside the regular
// spelling, or with a cell of another length, hands the BLOCK to the host route (pg_ped_dev_collect reports the line).
#include "pg_ctx.h"
#include "pg_line_fields.h"
#include "pg_ped_core.h"
#include "pg_wave.h"

#include <algorithm>
#include <cstring>

namespace {

#define PGP_LDS_BYTES (64 * 1024)   // what a workgroup of k_ped_tile may use: four tab tables and the tile
#define PGP_TILE_THREADS 256
#define PGP_MAX_LINE 0x3fffffffu    // line bytes the device takes

struct PedArgs {
    const uint8_t *text;
    const int64_t *nl;
    int64_t n_lines, pitch;
    const int32_t *sel_col, *sel_len, *sel_w;
    const int64_t *sel_woff;
    uint32_t *keep, *rlen;
    uint8_t *runf, *rrun, *out, *map;
    int64_t *row, *roff, *rstart, *line_of;
    long long *status;
    int tile_seqs, wmax;
};

__device__ inline void ped_line_at(const PedArgs &A, int64_t i, int64_t *ls, int64_t *le) {
    *ls = i ? A.nl[i - 1] + 1 : 0;
    *le = A.nl[i];
}

// the line's first n_cols - 1 tabs into LDS, unchecked (k_ped_lines took the line); the caller puts a barrier behind it
__device__ inline void ped_tabs(const uint8_t *line, uint32_t n, int n_cols, int lane, uint32_t *tabs) {
    uint32_t ntab = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t k = base + (uint32_t)lane;
        const bool tab = k < n && line[k] == '\t';
        const uint64_t m = __ballot(tab);
        if (tab) {
            const uint32_t idx = ntab + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (idx < (uint32_t)(n_cols - 1)) tabs[idx] = k;
        }
        ntab += (uint32_t)__popcll(m);
    }
}

__global__ __launch_bounds__(64) void k_ped_lines(PedArgs A, PgpConfig cfg) {
    extern __shared__ uint32_t tabs[];
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= A.n_lines) return;
    int64_t ls, le;
    ped_line_at(A, i, &ls, &le);
    const uint8_t *line = A.text + ls;
    if (le > ls && line[0] == '#') {                              // genomics.py:1943
        if (lane == 0) { A.keep[i] = 0; A.runf[i] = 0; A.rlen[i] = 0; }
        return;
    }
    bool host = le - ls > (int64_t)PGP_MAX_LINE;
    const uint32_t n = host ? 0 : (uint32_t)(le - ls);
    host = host || !line_tabs(line, n, cfg.n_cols, lane, tabs);
    if (!host) {
        bool bad = false;
        for (int q = lane; q < cfg.n_sel; q += 64) {
            uint32_t s, e;
            field_at(tabs, A.sel_col[q], cfg.n_cols, n, &s, &e);
            bad = bad || e - s != (uint32_t)A.sel_len[q] || pgp_cell_check(line + s, (int64_t)(e - s), cfg.fmt) != 0;
        }
        host = __ballot(bad) != 0;                                // (a cell the run stops on is worded by the host)
    }
    uint32_t rlen = 0;
    uint8_t run = 1;
    if (!host) {
        const uint32_t f0e = tabs[0], f1e = tabs[1];              // (n_cols >= 3: pg_ped_dev_config)
        int64_t pos = 0;
        const uint32_t pz = pgg_pos_zeros(line + f0e + 1, (int64_t)f1e - (int64_t)f0e - 1);      // not in the row (str(int))
        host = !pgg_pos_plain(line + f0e + 1 + pz, (int64_t)f1e - (int64_t)f0e - 1 - (int64_t)pz, &pos);
        rlen = pgp_map_len(f0e, f1e - f0e - 1 - pz);
        // the site before: the nearest line above that is no '#' line (none: the block's first site opens a run)
        int64_t j = i - 1, ps = 0, pe = 0;
        for (; j >= 0; --j) {
            ped_line_at(A, j, &ps, &pe);
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
        A.rlen[i] = host ? 0 : rlen;
        if (host) pg_raise_host(A.status, i);
    }
}

// a kept line's record at its row; its .map row: scaffold ' ' position " 0 " position '\n' (left out while the rows' room is short)
__global__ __launch_bounds__(64) void k_ped_map(PedArgs A) {
    const int lane = (int)threadIdx.x;
    const int64_t i = blockIdx.x;
    if (i >= A.n_lines || !A.keep[i] || (A.status[PGL_ST_BITS] & PG_ST_HOST)) return;
    int64_t ls, le;
    ped_line_at(A, i, &ls, &le);
    const uint8_t *line = A.text + ls;
    const uint32_t n = (uint32_t)(le - ls);
    if (lane == 0) {
        const int64_t r = A.row[i];
        A.line_of[r] = i;
        A.rrun[r] = A.runf[i];
        A.rstart[r] = ls;
    }
    if (A.status[PGL_ST_BITS] != 0) return;
    uint32_t t0 = n, t1 = n;
    int found = 0;
    for (uint32_t base = 0; base < n && found < 2; base += 64) {  // the line's first two tabs
        const uint32_t k = base + (uint32_t)lane;
        uint64_t m = __ballot(k < n && line[k] == '\t');
        for (; m && found < 2; m &= m - 1, ++found) (found ? t1 : t0) = base + (uint32_t)__ffsll((long long)m) - 1;
    }
    const uint32_t f0e = t0, pz = pgg_pos_zeros(line + f0e + 1, (int64_t)t1 - (int64_t)f0e - 1);
    const uint32_t ps = f0e + 1 + pz, pl = t1 - ps;
    uint8_t *o = A.map + A.roff[i];
    for (uint32_t k = (uint32_t)lane; k < f0e; k += 64) o[k] = line[k];
    o += f0e;
    if (lane == 0) o[0] = ' ';
    if (lane >= 1 && lane <= 3) o[pl + (uint32_t)lane] = (uint8_t)(lane == 2 ? '0' : ' ');
    if (lane == 4) o[2 * pl + 4] = '\n';
    for (uint32_t k = (uint32_t)lane; k < pl; k += 64) {
        o[1 + k] = line[ps + k];
        o[pl + 4 + k] = line[ps + k];
    }
}

__global__ __launch_bounds__(PGP_TILE_THREADS) void k_ped_tile(PedArgs A, PgpConfig cfg) {
    extern __shared__ uint32_t lds[];
    if (A.status[PGL_ST_BITS] & PG_ST_HOST) return;               // (the block is the host's)
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    int64_t site0, q0;
    const int ns = (int)pgp_tile_count(A.status[PGL_ST_ROWS], PGP_TILE_LINES, blockIdx.x, &site0);
    const int nq = (int)pgp_tile_count(cfg.n_sel, A.tile_seqs, blockIdx.y, &q0);
    if (ns == 0 || nq == 0) return;
    uint32_t *tabs = lds + (size_t)wave * (size_t)cfg.n_cols;
    uint8_t *tile = reinterpret_cast<uint8_t *>(lds + 4 * (size_t)cfg.n_cols);
    const size_t tp = (size_t)pgp_tile_pitch(A.wmax);
    // (1) the lines of the tile, a wave each in turn: tabs ranked, a lane per sample expands its cell
    for (int it = 0; it < PGP_TILE_LINES / 4; ++it) {
        const int l = it * 4 + wave;
        const bool live = l < ns;
        int64_t ls = 0, le = 0;
        if (live) ped_line_at(A, A.line_of[site0 + l], &ls, &le);
        const uint8_t *line = A.text + ls;
        ped_tabs(line, (uint32_t)(le - ls), cfg.n_cols, lane, tabs);
        __syncthreads();
        if (live)
            for (int qq = lane; qq < nq; qq += 64) {
                const int q = (int)q0 + qq, w = A.sel_w[q];
                const uint8_t *cell = line + tabs[A.sel_col[q] - 1] + 1;
                uint8_t *o = tile + (size_t)qq * tp + (size_t)l * (size_t)w;
                if (w == 4) {                                     // a diploid's two alleles: one word
                    *reinterpret_cast<uint32_t *>(o) = (uint32_t)pgp_allele(cell, cfg.fmt, 0) | 0x20u << 8 | (uint32_t)pgp_allele(cell, cfg.fmt, 1) << 16 | 0x20u << 24;
                } else {
                    uint16_t *o2 = reinterpret_cast<uint16_t *>(o);
                    for (int k = 0; k < w / 2; ++k) o2[k] = (uint16_t)(pgp_allele(cell, cfg.fmt, k) | 0x20u << 8);
                }
            }
        __syncthreads();
    }
    // (2) 16 bytes of one sample per thread: four words out of the tile, one store (bytes at the row's end)
    const int segs = PGP_TILE_LINES * A.wmax / PGP_STORE;
    for (int item = (int)threadIdx.x; item < nq * segs; item += PGP_TILE_THREADS) {
        const int qq = item / segs, seg = item % segs, q = (int)q0 + qq;
        const int w = A.sel_w[q];
        const int nb = pgp_store_bytes((int64_t)ns * w, seg);
        if (nb == 0) continue;
        const uint32_t *src = reinterpret_cast<const uint32_t *>(tile + (size_t)qq * tp + (size_t)seg * PGP_STORE);
        uint8_t *dst = A.out + (size_t)A.sel_woff[q] * (size_t)A.pitch + (size_t)site0 * (size_t)w + (size_t)seg * PGP_STORE;
        const uint4 v = make_uint4(src[0], src[1], src[2], src[3]);
        if (nb == PGP_STORE) {
            *reinterpret_cast<uint4 *>(dst) = v;
        } else {
            const uint32_t vv[4] = {v.x, v.y, v.z, v.w};
            for (int k = 0; k < nb; ++k) dst[k] = (uint8_t)(vv[k >> 2] >> (8 * (k & 3)));
        }
    }
}

int check_slot(pg_ctx *c, int slot, const char *who) { return pg_line_check_slot(c, slot, c ? &c->ped : nullptr, who, "pg_ped_dev_config"); }

PedArgs ped_args(pg_ctx *c, int slot) {
    pg_ctx::PedDev &D = c->ped;
    pg_ctx::PedDev::Slot &P = D.s[slot];
    pg_ctx::TokSlot &T = c->tok[slot];
    PedArgs A;
    A.text = T.tp;
    A.nl = T.nl.p;
    A.n_lines = P.L.n_lines;
    A.pitch = P.pitch;
    A.sel_col = D.sel_col.p;
    A.sel_len = D.sel_len.p;
    A.sel_w = D.sel_w.p;
    A.sel_woff = D.sel_woff.p;
    A.keep = P.keep.p;
    A.rlen = P.rlen.p;
    A.runf = P.runf.p;
    A.rrun = P.rrun.p;
    A.out = P.out.p;
    A.map = P.map.p;
    A.row = P.row.p;
    A.roff = P.roff.p;
    A.rstart = P.rstart.p;
    A.line_of = P.line_of.p;
    A.status = reinterpret_cast<long long *>(P.status.p);
    A.tile_seqs = D.tile_seqs;
    A.wmax = D.wmax;
    return A;
}

}  // namespace

extern "C" int pg_ped_dev_config(pg_ctx *c, const pg_ped_cfg *cfg, const int32_t *sel_col, const int32_t *sel_len, int tile_seqs, int *taken_out) {
    if (!c || !cfg || !taken_out || cfg->n_sel < 1 || cfg->n_cols < 3 || !sel_col || !sel_len || tile_seqs < 0 || cfg->fmt < PGP_F_PHASED ||
        cfg->fmt > PGP_F_CHARS)
        return pg_fail(PG_ERR_ARG, "pg_ped_dev_config: bad argument");
    for (int q = 0; q < cfg->n_sel; ++q)
        if (sel_col[q] < 2 || sel_col[q] >= cfg->n_cols) return pg_fail(PG_ERR_ARG, "pg_ped_dev_config: sample %d: column %d", q, sel_col[q]);
    *taken_out = 0;
    pg_ctx::PedDev &D = c->ped;
    D.configured = false;
    // what k_ped_tile reads without looking again: cells of exactly these lengths, PG_PED_DEV_ALLELES alleles at most
    std::vector<int32_t> w((size_t)cfg->n_sel);
    std::vector<int64_t> woff((size_t)cfg->n_sel);
    int wmax = 0;
    int64_t wsum = 0;
    for (int q = 0; q < cfg->n_sel; ++q) {
        if (!pgp_dev_len(cfg->fmt, sel_len[q])) return PG_OK;
        w[(size_t)q] = 2 * pgp_alleles(cfg->fmt, sel_len[q]);
        woff[(size_t)q] = wsum;
        wsum += w[(size_t)q];
        wmax = std::max(wmax, w[(size_t)q]);
    }
    const int tq = pgp_tile_seqs(cfg->n_cols, cfg->n_sel, wmax, tile_seqs, PGP_LDS_BYTES);
    if (tq == 0) return PG_OK;                                    // (a header too wide for four tab tables in LDS)
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    const size_t ns = (size_t)cfg->n_sel;
    int rc;
    if ((rc = D.sel_col.ensure(ns)) != PG_OK || (rc = D.sel_len.ensure(ns)) != PG_OK || (rc = D.sel_w.ensure(ns)) != PG_OK ||
        (rc = D.sel_woff.ensure(ns)) != PG_OK)
        return rc;
    HIPCHK(hipMemcpy(D.sel_col.p, sel_col, ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.sel_len.p, sel_len, ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.sel_w.p, w.data(), ns * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.sel_woff.p, woff.data(), ns * 8, hipMemcpyHostToDevice));
    D.cfg = *cfg;
    D.tile_seqs = tq;
    D.wmax = wmax;
    D.wsum = wsum;
    D.configured = true;
    *taken_out = 1;
    return PG_OK;
}

// A block of whole lines (the last byte a line feed, else the block is the host's) into text slot `slot`
extern "C" int pg_ped_dev_submit(pg_ctx *c, int slot, const char *text, int64_t len) {
    int rc = check_slot(c, slot, "pg_ped_dev_submit");
    return rc != PG_OK ? rc : pg_line_submit_plain(c, slot, c->ped.s[slot], text, len, "pg_ped_dev_submit");
}

// The same for a block that is still bgzipped: the members cross PCIe deflated, k_inflate writes their text behind `head` in the slot
// and lists its line feeds.  Whether the text ends in a line feed is read on the device once the line feeds are counted
extern "C" int pg_ped_dev_submit_bgzf(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                                      const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                                      int64_t text_len) {
    int rc = check_slot(c, slot, "pg_ped_dev_submit_bgzf");
    if (rc != PG_OK) return rc;
    if (text_len < 0) return pg_fail(PG_ERR_ARG, "pg_ped_dev_submit_bgzf: bad argument");
    return pg_line_submit_bgzf(c, slot, c->ped.s[slot], comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, 1024,
                               false, false);
}

namespace {

// the .map rows (k_ped_map), then -- first: the transpose and -- the status back to the host (the block: queued)
int queue_map(pg_ctx *c, int slot, hipStream_t st, bool first) {
    pg_ctx::PedDev &D = c->ped;
    pg_ctx::PedDev::Slot &P = D.s[slot];
    const PedArgs A = ped_args(c, slot);
    hipLaunchKernelGGL(k_ped_map, dim3((unsigned)P.L.n_lines), dim3(64), 0, st, A);
    HIPCHK(hipGetLastError());
    if (first) {
        const unsigned tiles = (unsigned)(P.pitch / PGP_TILE_LINES), qtiles = (unsigned)((D.cfg.n_sel + D.tile_seqs - 1) / D.tile_seqs);
        const size_t lds = (size_t)D.cfg.n_cols * 16 + (size_t)D.tile_seqs * (size_t)pgp_tile_pitch(D.wmax);
        hipLaunchKernelGGL(k_ped_tile, dim3(tiles, qtiles), dim3(PGP_TILE_THREADS), lds, st, A, D.cfg);
        HIPCHK(hipGetLastError());
    }
    return pg_line_parse_end(c, P, st);
}

// .map rows longer than their room: room for `need` bytes of them, written once more (the matrix stands)
int map_again(pg_ctx *c, int slot, int64_t need, hipStream_t st) {
    pg_ctx::PedDev::Slot &P = c->ped.s[slot];
    int rc = P.map.ensure_roomy((size_t)need + 4096);
    if (rc != PG_OK) return rc;
    P.map_cap = (int64_t)P.map.cap;
    return queue_map(c, slot, st, false);
}

}  // namespace

// Queues the kernels of the block in `slot` (waits for the number of its lines only)
extern "C" int pg_ped_dev_parse(pg_ctx *c, int slot) {
    int rc = check_slot(c, slot, "pg_ped_dev_parse");
    if (rc != PG_OK) return rc;
    pg_ctx::PedDev &D = c->ped;
    pg_ctx::PedDev::Slot &P = D.s[slot];
    int64_t n_lines = 0;
    bool nothing = true;
    if ((rc = pg_line_parse_begin(c, slot, P, &n_lines, &nothing, "pg_ped_dev_parse")) != PG_OK || P.L.state == PGL_EMPTY) return rc;
    P.pitch = pgp_pitch(n_lines);
    if (nothing) return PG_OK;
    if (n_lines > 0x7fffffffll) return pg_fail(PG_ERR_ARG, "pg_ped_dev_parse: more than 2^31 lines in a block");
    hipStream_t st = c->stream_up;
    const size_t nl = (size_t)n_lines;
    if ((rc = P.keep.ensure_roomy(nl)) != PG_OK || (rc = P.rlen.ensure_roomy(nl)) != PG_OK || (rc = P.runf.ensure_roomy(nl)) != PG_OK ||
        (rc = P.rrun.ensure_roomy(nl)) != PG_OK || (rc = P.row.ensure_roomy(nl)) != PG_OK || (rc = P.roff.ensure_roomy(nl)) != PG_OK ||
        (rc = P.rstart.ensure_roomy(nl)) != PG_OK || (rc = P.line_of.ensure_roomy(nl)) != PG_OK ||
        (rc = P.out.ensure_roomy((size_t)D.wsum * (size_t)P.pitch)) != PG_OK)
        return rc;
    // .map rows: a scaffold's name of a few characters, the position twice; longer ones make a larger total, which grows the buffer
    // in collect
    P.map_cap = std::max<int64_t>(P.map_cap, n_lines * 32 + 256);
    if ((rc = P.map.ensure_roomy((size_t)P.map_cap)) != PG_OK) return rc;
    P.map_cap = (int64_t)P.map.cap;
    if ((rc = pg_line_status_upload(P, st)) != PG_OK) return rc;
    const PedArgs A = ped_args(c, slot);
    hipLaunchKernelGGL(k_ped_lines, dim3((unsigned)n_lines), dim3(64), (size_t)D.cfg.n_cols * 4, st, A, D.cfg);
    HIPCHK(hipGetLastError());
    // the kept lines' rows: the scan of the 0 / 1 flags; then the .map rows' places: their bytes land in status[PGL_ST_BYTES], the
    // number of sites (every site has a row) in status[PGL_ST_ROWS]
    pg_rows_scan_queue(st, P.keep.p, n_lines, P.row.p, A.status, 0x7fffffffffffffffll);
    pg_rows_scan_queue(st, P.rlen.p, n_lines, P.roff.p, A.status, P.map_cap);
    if ((rc = queue_map(c, slot, st, true)) != PG_OK) return rc;
    ++D.blocks;
    return PG_OK;
}

// Waits for the block's kernels.  *host_line_out < 0: the matrix and the .map rows are ready (pg_ped_dev_rows, pg_ped_dev_meta); else
// the block goes to the host route -- line *host_line_out is the first the device does not take.  .map rows longer than the buffer
// (the scan knows their total) grow it and are written again.
extern "C" int pg_ped_dev_collect(pg_ctx *c, int slot, int64_t *n_sites_out, int64_t *map_len_out, int64_t *host_line_out, int64_t *n_lines_out,
                                  int64_t *pitch_out) {
    int rc = check_slot(c, slot, "pg_ped_dev_collect");
    if (rc != PG_OK) return rc;
    if (!n_sites_out || !map_len_out || !host_line_out) return pg_fail(PG_ERR_ARG, "pg_ped_dev_collect: null argument");
    pg_ctx::PedDev::Slot &P = c->ped.s[slot];
    const bool empty = P.L.state == PGL_EMPTY;
    PgLineResult R;
    rc = pg_line_collect(c, slot, c->ped, P, false, map_again, n_lines_out, &R, "pg_ped_dev_collect");
    if (pitch_out) *pitch_out = rc == PG_OK && !empty ? P.pitch : 0;
    *host_line_out = R.host_line;
    *map_len_out = R.bytes;
    *n_sites_out = R.rows;
    return rc;
}

// which = 0: the first len bytes of the matrix (sample q's row at woff[q] x pitch); 1: the .map rows
extern "C" int pg_ped_dev_rows(pg_ctx *c, int slot, int which, uint8_t *dst, int64_t len) {
    int rc = check_slot(c, slot, "pg_ped_dev_rows");
    if (rc != PG_OK) return rc;
    if (which < 0 || which > 1) return pg_fail(PG_ERR_ARG, "pg_ped_dev_rows: bad output");
    return pg_line_rows(c, which ? c->ped.s[slot].map : c->ped.s[slot].out, dst, len, "pg_ped_dev_rows: bad length");
}

// per site of the collected block: 1 where its scaffold differs from the site's before, where its line begins in the text
extern "C" int pg_ped_dev_meta(pg_ctx *c, int slot, uint8_t *run_dst, int64_t *start_dst) {
    int rc = check_slot(c, slot, "pg_ped_dev_meta");
    if (rc != PG_OK) return rc;
    pg_ctx::PedDev::Slot &P = c->ped.s[slot];
    const int64_t n = P.h_status.p ? P.h_status.p[PGL_ST_ROWS] : 0;
    if (P.h_status.p && P.h_status.p[PGL_ST_BITS]) return pg_fail(PG_ERR_STATE, "pg_ped_dev_meta: the block in slot %d is the host's", slot);
    if (n < 0 || (size_t)n > P.rrun.cap) return pg_fail(PG_ERR_STATE, "pg_ped_dev_meta: nothing collected in slot %d", slot);
    if (n == 0) return PG_OK;
    if (!run_dst || !start_dst) return pg_fail(PG_ERR_ARG, "pg_ped_dev_meta: null argument");
    if ((rc = pg_copy_back(c, run_dst, P.rrun.p, n)) != PG_OK) return rc;
    return pg_copy_back(c, start_dst, P.rstart.p, n * 8);
}

// bytes [off, off + len) of the collected block's text (a run's scaffold name; the whole block when it goes to the host route and the
// host never had its text: BGZF)
extern "C" int pg_ped_dev_text(pg_ctx *c, int slot, int64_t off, int64_t len, uint8_t *dst) {
    int rc = check_slot(c, slot, "pg_ped_dev_text");
    return rc != PG_OK ? rc : pg_line_text(c, slot, off, len, dst, "pg_ped_dev_text: bad range");
}

extern "C" int pg_ped_dev_tile_seqs(pg_ctx *c, int *tile_seqs_out) {
    if (!c || !tile_seqs_out || !c->ped.configured) return pg_fail(PG_ERR_ARG, "pg_ped_dev_tile_seqs: not configured");
    *tile_seqs_out = c->ped.tile_seqs;
    return PG_OK;
}

extern "C" int pg_ped_dev_stats(pg_ctx *c, int64_t *blocks_out, int64_t *host_blocks_out) {
    return pg_line_stats(c ? &c->ped : nullptr, blocks_out, host_blocks_out, "pg_ped_dev_stats");
}
