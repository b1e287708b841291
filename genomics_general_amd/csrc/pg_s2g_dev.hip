// Sequences written as `.geno` sites on the device: the seqToGeno.py drop-in's route.  Two stages meet in the residue store, the
// sequences' characters side by side in device memory with feeds and blanks gone; the per-byte and per-line rules are
// csrc/pg_s2g_core.h (the host route pg_s2g_strip / pg_s2g_text in pg_s2g.cpp runs the same functions); this file is the division of
// the work over the chip and the host side of the entry points.
//
// Stage 1, a fasta block in one of the tokenizer's text slots (csrc/pg_line_slot.h):
//   k_s2g_lines   a wavefront per line, 16 bytes a lane and step: head lines ('>' first) marked, irregular bytes (a blank, a tab or \r in a sequence line, \r,
//                 a second '>' or text that is not ASCII anywhere) raise the block to the host, the line's residue count
//   scans         the head lines' ranks, the sequence lines' places in the store (k_rows_scan, pg_line_slot.hip)
//   k_s2g_heads   a thread per line: a head line's record (where it begins, its length, the block's residues in front of it)
//   k_s2g_gather  a wavefront per sequence line: its bytes to store[base + place], byte stores up to the first multiple of 16 of the
//                 destination, 16-byte stores behind it
// Stage 2, a range of output lines cut into jobs of PGS_TILE_SITES consecutive sites of one segment:
//   k_s2g_tile    a workgroup takes a job and a tile of haplotypes: 128 contiguous store bytes per haplotype into an LDS tile (aligned
//                 words funnelled: the store offsets are arbitrary), then each wave writes whole lines, its lanes consecutive 16-byte
//                 pieces of the line, every byte the prefix's (name, position), the template's literal or tile[h][site].  A line
//                 begins at the closed form pgs_line_start: no scan.  The tile of haplotypes y writes the template bytes
//                 [tstart[y], tstart[y + 1]) of each line, tile 0 the prefix too.
//   k_deflate     (-g x.gz) BGZF members of the rows where they lie (pg_deflate.hip)
#include "pg_ctx.h"
#include "pg_s2g_core.h"
#include "pg_wave.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

#define PGS_LDS_BYTES (60 * 1024)   // what a workgroup of k_s2g_tile may use: the tile and its share of the template
#define PGS_TILE_THREADS 256
#define PGS_STORE_SLACK 64          // bytes behind the store's last residue that the tile's aligned words may touch
#define PGS_MAX_LINE 0x7fffffffll   // line bytes the device takes

struct S2gLineArgs {
    const uint8_t *text;
    const int64_t *nl;
    int64_t n_lines, base;
    uint32_t *cnt, *head;
    int64_t *roff, *hrow, *hrec;
    uint8_t *store;
    long long *status;
    int open;                       // a record is open where the block begins (else its first line must be a head line)
};

__device__ inline void s2g_line_at(const S2gLineArgs &A, int64_t i, int64_t *ls, int64_t *le) {
    *ls = i ? A.nl[i - 1] + 1 : 0;
    *le = A.nl[i];
}

__global__ __launch_bounds__(256) void k_s2g_lines(S2gLineArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= A.n_lines) return;
    int64_t ls, le;
    s2g_line_at(A, i, &ls, &le);
    const uint8_t *line = A.text + ls;
    const int64_t n = le - ls;
    const bool head = pgs_is_head(line, n);
    bool bad = n > PGS_MAX_LINE || (i == 0 && !A.open && !head);
    for (int64_t k = (int64_t)lane * PGS_STORE; k < n; k += 64 * PGS_STORE) {                  // 16 bytes a lane and step
        uint8_t b[PGS_STORE];
        const int m = (int)std::min<int64_t>(PGS_STORE, n - k);
        if (m == PGS_STORE) {
            __builtin_memcpy(b, line + k, PGS_STORE);
        } else {
            for (int q = 0; q < m; ++q) b[q] = line[k + q];
        }
        for (int q = 0; q < m; ++q) bad = bad || pgs_irregular(b[q], k + q == 0, head);
    }
    const bool host = __ballot(bad) != 0;
    if (lane == 0) {
        A.head[i] = head ? 1u : 0u;
        A.cnt[i] = host ? 0u : pgs_line_residues(line, n);
        if (host) pg_raise_host(A.status, i);
    }
}

// the number of head lines (the first scan's total) out of the way of the second scan
__global__ void k_s2g_note(long long *status) { status[PGL_ST_BGZF_BYTES] = status[PGL_ST_ROWS]; }

__global__ __launch_bounds__(256) void k_s2g_heads(S2gLineArgs A) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_lines || !A.head[i] || (A.status[PGL_ST_BITS] & PG_ST_HOST)) return;
    int64_t ls, le;
    s2g_line_at(A, i, &ls, &le);
    int64_t *r = A.hrec + 3 * A.hrow[i];
    r[0] = ls;
    r[1] = le - ls;
    r[2] = A.roff[i];
}

__global__ __launch_bounds__(256) void k_s2g_gather(S2gLineArgs A) {
    const int lane = (int)(threadIdx.x & 63);
    const int64_t i = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (i >= A.n_lines || A.status[PGL_ST_BITS] != 0) return;     // (the block is the host's)
    const int64_t n = A.cnt[i];
    if (n == 0) return;
    int64_t ls, le;
    s2g_line_at(A, i, &ls, &le);
    const uint8_t *src = A.text + ls;
    uint8_t *dst = A.store + A.base + A.roff[i];
    const int64_t lead = std::min<int64_t>(n, (int64_t)((PGS_STORE - (reinterpret_cast<uintptr_t>(dst) & (PGS_STORE - 1))) & (PGS_STORE - 1)));
    if (lane < lead) dst[lane] = src[lane];
    const int64_t full = (n - lead) / PGS_STORE;
    for (int64_t k = lane; k < full; k += 64) {
        uint4 v;
        __builtin_memcpy(&v, src + lead + k * PGS_STORE, PGS_STORE);
        *reinterpret_cast<uint4 *>(dst + lead + k * PGS_STORE) = v;
    }
    const int64_t done = lead + full * PGS_STORE;
    if (done + lane < n) dst[done + lane] = src[done + lane];      // (fewer than 16 bytes are left)
}

struct S2gJob {
    int64_t site0, out_at;          // the job's first site; where that site's line begins in the range's output
    int32_t seg, ns;                // its segment, its sites (1 .. PGS_TILE_SITES)
};

struct S2gTileArgs {
    const uint8_t *store;
    const S2gJob *jobs;
    const uint8_t *names;
    const int64_t *name_off;        // n_segs + 1
    const int64_t *hap_off;         // n_segs x n_haps
    const int32_t *tmpl, *tstart;
    uint8_t *out;
    int n_haps, tmpl_len, tile_seqs;
};

__global__ __launch_bounds__(PGS_TILE_THREADS) void k_s2g_tile(S2gTileArgs A) {
    extern __shared__ uint32_t lds[];
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const S2gJob job = A.jobs[blockIdx.x];
    const int ty = (int)blockIdx.y;
    int64_t h0;
    const int nh = (int)pgs_tile_count(A.n_haps, A.tile_seqs, ty, &h0);
    if (nh == 0 || job.ns <= 0) return;
    const int j0 = A.tstart[ty], j1 = A.tstart[ty + 1];
    uint8_t *tile = reinterpret_cast<uint8_t *>(lds);
    int32_t *ltm = reinterpret_cast<int32_t *>(lds + (size_t)A.tile_seqs * (PGS_TILE_PITCH / 4));
    for (int j = (int)threadIdx.x; j < j1 - j0; j += PGS_TILE_THREADS) ltm[j] = A.tmpl[j0 + j];
    // (1) 128 contiguous bytes of the store per haplotype: aligned words, funnelled by the offset's low bits
    const int64_t *hoff = A.hap_off + (int64_t)job.seg * A.n_haps + h0;
    for (int item = (int)threadIdx.x; item < nh * (PGS_TILE_SITES / 4); item += PGS_TILE_THREADS) {
        const int hh = item / (PGS_TILE_SITES / 4), w = item % (PGS_TILE_SITES / 4);
        if (4 * w >= job.ns) continue;
        const uint8_t *src = A.store + hoff[hh] + job.site0;
        const int shift = (int)(reinterpret_cast<uintptr_t>(src) & 3);
        const uint32_t *al = reinterpret_cast<const uint32_t *>(src - shift) + w;
        lds[(size_t)hh * (PGS_TILE_PITCH / 4) + (size_t)w] = pgs_funnel(al[0], shift ? al[1] : 0u, shift);
    }
    __syncthreads();
    // (2) whole lines, a wave each in turn: its lanes take consecutive 16-byte pieces of this tile's bytes of the line
    const uint8_t *name = A.names + A.name_off[job.seg];
    const uint32_t name_len = (uint32_t)(A.name_off[job.seg + 1] - A.name_off[job.seg]);
    const uint64_t fixed = pgs_line_fixed(name_len, (uint32_t)A.tmpl_len);
    const uint64_t start0 = pgs_line_start((uint64_t)job.site0, fixed);
    for (int l = wave; l < job.ns; l += PGS_TILE_THREADS / 64) {
        const uint64_t x = (uint64_t)job.site0 + (uint64_t)l, pos = x + 1;
        const int d = pgs_digits(pos);
        const int64_t pl = (int64_t)name_len + 2 + d;
        const int64_t ls = job.out_at + (int64_t)(pgs_line_start(x, fixed) - start0);
        const int64_t a = ls + (ty ? pl + j0 : 0), b = ls + pl + j1;
        const int64_t n_st = pgs_store_count(a, b);
        for (int64_t k = lane; k < n_st; k += 64) {
            int64_t lo, hi;
            pgs_store_at(a, b, k, &lo, &hi);
            uint32_t v[4] = {0, 0, 0, 0};
            for (int64_t q = lo; q < hi; ++q) {
                const int64_t p = q - ls;
                uint8_t byte;
                if (p < pl) {
                    byte = pgs_prefix_byte(name, name_len, pos, d, (uint32_t)p);
                } else {
                    const int32_t t = ltm[p - pl - j0];
                    byte = pgs_is_lit(t) ? pgs_lit_byte(t) : tile[(size_t)(t - (int32_t)h0) * PGS_TILE_PITCH + (size_t)l];
                }
                const int at = (int)(q - lo);
                v[at >> 2] |= (uint32_t)byte << (8 * (at & 3));
            }
            if (hi - lo == PGS_STORE) {
                *reinterpret_cast<uint4 *>(A.out + lo) = make_uint4(v[0], v[1], v[2], v[3]);
            } else {
                for (int64_t q = lo; q < hi; ++q) A.out[q] = (uint8_t)(v[(q - lo) >> 2] >> (8 * ((q - lo) & 3)));
            }
        }
    }
}

int check_slot(pg_ctx *c, int slot, const char *who) { return pg_line_check_slot(c, slot, c ? &c->s2g : nullptr, who, "pg_s2g_dev_begin"); }

// room for `need` residues in the store, the first `keep` of them kept
int store_room(pg_ctx *c, int64_t need, int64_t keep) {
    pg_ctx::S2gDev &D = c->s2g;
    if ((size_t)need + PGS_STORE_SLACK <= D.store.cap) return PG_OK;
    HIPCHK(hipStreamSynchronize(c->stream_up));
    DevBuf<uint8_t> next;
    int rc = next.alloc((size_t)need + (size_t)need / 2 + PGS_STORE_SLACK + 4096);
    if (rc != PG_OK) return rc;
    if (keep > 0) HIPCHK(hipMemcpy(next.p, D.store.p, (size_t)keep, hipMemcpyDeviceToDevice));
    D.store.release();
    D.store = next;
    return PG_OK;
}

}  // namespace

// The route's store, with room for store_hint residues to begin with (it grows)
extern "C" int pg_s2g_dev_begin(pg_ctx *c, int64_t store_hint) {
    if (!c || store_hint < 0) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_begin: bad argument");
    HIPCHK(hipSetDevice(c->device));
    pg_ctx::S2gDev &D = c->s2g;
    D.configured = false;
    D.planned = false;
    D.blocks = D.host_blocks = D.out_ranges = 0;
    int rc = D.store.ensure((size_t)store_hint + PGS_STORE_SLACK + 4096);
    if (rc != PG_OK) return rc;
    D.configured = true;
    return PG_OK;
}

// A block of whole lines (the last byte a line feed, else the block is the host's) into text slot `slot`
extern "C" int pg_s2g_dev_submit(pg_ctx *c, int slot, const char *text, int64_t len) {
    int rc = check_slot(c, slot, "pg_s2g_dev_submit");
    return rc != PG_OK ? rc : pg_line_submit_plain(c, slot, c->s2g.s[slot], text, len, "pg_s2g_dev_submit");
}

// The same for a block that is still bgzipped: the members cross PCIe deflated, k_inflate writes their text behind `head` in the slot
extern "C" int pg_s2g_dev_submit_bgzf(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                                      const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                                      int64_t text_len) {
    int rc = check_slot(c, slot, "pg_s2g_dev_submit_bgzf");
    if (rc != PG_OK) return rc;
    if (text_len < 0) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_submit_bgzf: bad argument");
    return pg_line_submit_bgzf(c, slot, c->s2g.s[slot], comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, 64,
                               false, false);
}

// Queues the kernels of the block in `slot`: its residues go to store[base ..); open: a record is open where the block begins
extern "C" int pg_s2g_dev_parse(pg_ctx *c, int slot, int64_t base, int open) {
    int rc = check_slot(c, slot, "pg_s2g_dev_parse");
    if (rc != PG_OK) return rc;
    if (base < 0) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_parse: bad base");
    pg_ctx::S2gDev &D = c->s2g;
    pg_ctx::S2gDev::Slot &P = D.s[slot];
    int64_t n_lines = 0;
    bool nothing = true;
    if ((rc = pg_line_parse_begin(c, slot, P, &n_lines, &nothing, "pg_s2g_dev_parse")) != PG_OK || nothing) return rc;
    if (n_lines > 0x7fffffffll) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_parse: more than 2^31 lines in a block");
    hipStream_t st = c->stream_up;
    pg_ctx::TokSlot &T = c->tok[slot];
    const size_t nl = (size_t)n_lines;
    if ((rc = store_room(c, base + T.len, base)) != PG_OK) return rc;
    if ((rc = P.cnt.ensure_roomy(nl)) != PG_OK || (rc = P.head.ensure_roomy(nl)) != PG_OK || (rc = P.roff.ensure_roomy(nl)) != PG_OK ||
        (rc = P.hrow.ensure_roomy(nl)) != PG_OK || (rc = P.hrec.ensure_roomy(3 * nl)) != PG_OK)
        return rc;
    if ((rc = pg_line_status_upload(P, st)) != PG_OK) return rc;
    S2gLineArgs A;
    A.text = T.tp;
    A.nl = T.nl.p;
    A.n_lines = n_lines;
    A.base = base;
    A.cnt = P.cnt.p;
    A.head = P.head.p;
    A.roff = P.roff.p;
    A.hrow = P.hrow.p;
    A.hrec = P.hrec.p;
    A.store = D.store.p;
    A.status = reinterpret_cast<long long *>(P.status.p);
    A.open = open;
    const unsigned waves4 = (unsigned)((n_lines + 3) / 4);
    hipLaunchKernelGGL(k_s2g_lines, dim3(waves4), dim3(256), 0, st, A);
    HIPCHK(hipGetLastError());
    pg_rows_scan_queue(st, P.head.p, n_lines, P.hrow.p, A.status, 0x7fffffffffffffffll);
    hipLaunchKernelGGL(k_s2g_note, dim3(1), dim3(1), 0, st, A.status);
    pg_rows_scan_queue(st, P.cnt.p, n_lines, P.roff.p, A.status, T.len);          // (a line's residues are its bytes at most: no overflow)
    hipLaunchKernelGGL(k_s2g_heads, dim3((unsigned)((n_lines + 255) / 256)), dim3(256), 0, st, A);
    hipLaunchKernelGGL(k_s2g_gather, dim3(waves4), dim3(256), 0, st, A);
    HIPCHK(hipGetLastError());
    if ((rc = pg_line_parse_end(c, P, st)) != PG_OK) return rc;
    ++D.blocks;
    return PG_OK;
}

// Waits for the block's kernels.  *host_line_out < 0: *n_res_out residues stand in the store behind the block's base, *n_heads_out
// head lines were seen (pg_s2g_dev_heads); else the block goes to the host route -- line *host_line_out is the first the device does
// not take -- and the store behind the base is to be written by pg_s2g_dev_put
extern "C" int pg_s2g_dev_collect(pg_ctx *c, int slot, int64_t *n_res_out, int64_t *n_heads_out, int64_t *host_line_out, int64_t *n_lines_out) {
    int rc = check_slot(c, slot, "pg_s2g_dev_collect");
    if (rc != PG_OK) return rc;
    if (!n_res_out || !n_heads_out || !host_line_out) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_collect: null argument");
    PgLineResult R;
    rc = pg_line_collect(c, slot, c->s2g, c->s2g.s[slot], true, nullptr, n_lines_out, &R, "pg_s2g_dev_collect");
    *host_line_out = R.host_line;
    *n_res_out = R.bytes;
    *n_heads_out = R.bgzf_bytes;                                  // (k_s2g_note put the head lines' number there)
    return rc;
}

// the collected block's head lines, three words each: where the line begins in the text, its bytes, the block's residues in front
extern "C" int pg_s2g_dev_heads(pg_ctx *c, int slot, int64_t *dst, int64_t n_heads) {
    int rc = check_slot(c, slot, "pg_s2g_dev_heads");
    if (rc != PG_OK) return rc;
    pg_ctx::S2gDev::Slot &P = c->s2g.s[slot];
    if (n_heads < 0 || (n_heads && !dst) || (size_t)n_heads * 3 > P.hrec.cap) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_heads: bad count");
    return n_heads ? pg_copy_back(c, dst, P.hrec.p, n_heads * 24) : PG_OK;
}

// bytes [off, off + len) of the collected block's text (a head line; the whole block when it goes to the host route and the host
// never had its text: BGZF)
extern "C" int pg_s2g_dev_text(pg_ctx *c, int slot, int64_t off, int64_t len, uint8_t *dst) {
    int rc = check_slot(c, slot, "pg_s2g_dev_text");
    return rc != PG_OK ? rc : pg_line_text(c, slot, off, len, dst, "pg_s2g_dev_text: bad range");
}

// len residues from the host to store[off ..) (a block the host route stripped; a phylip file's sequences), what stands in front kept
extern "C" int pg_s2g_dev_put(pg_ctx *c, int64_t off, const uint8_t *src, int64_t len) {
    if (!c || !c->s2g.configured || off < 0 || len < 0 || (len && !src)) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_put: bad argument");
    HIPCHK(hipSetDevice(c->device));
    int rc = store_room(c, off + len, off);
    if (rc != PG_OK || len == 0) return rc;
    HIPCHK(hipMemcpyAsync(c->s2g.store.p + off, src, (size_t)len, hipMemcpyHostToDevice, c->stream_up));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    return PG_OK;
}

// store[off .. off + len) to the host (a run that goes on on the host route)
extern "C" int pg_s2g_dev_get(pg_ctx *c, int64_t off, int64_t len, uint8_t *dst) {
    if (!c || !c->s2g.configured || off < 0 || len < 0 || (len && !dst) || (size_t)(off + len) > c->s2g.store.cap)
        return pg_fail(PG_ERR_ARG, "pg_s2g_dev_get: bad range");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    return len ? pg_copy_back(c, dst, c->s2g.store.p + off, len) : PG_OK;
}

// The output's description: the row template (tmpl_len entries: pgs_lit(byte), or a haplotype's index below n_haps, each index once
// and in rising order), n_segs segments with their names (names[name_off[s] .. name_off[s + 1])) and, per segment and haplotype, where
// its residues begin in the store; seg_sites: the segments' sites; store_len: the residues the store holds (every haplotype's sites
// must lie inside); tile_seqs: haplotypes per tile of k_s2g_tile (0: as many as the LDS holds)
extern "C" int pg_s2g_dev_plan(pg_ctx *c, const int32_t *tmpl, int32_t tmpl_len, int32_t n_haps, const char *names, const int64_t *name_off,
                               int64_t n_segs, const int64_t *seg_sites, const int64_t *hap_off, int64_t store_len, int tile_seqs,
                               int *tile_seqs_out) {
    if (!c || !c->s2g.configured || !tmpl || tmpl_len < 1 || n_haps < 1 || n_haps > PGS_MAX_HAPS || !name_off || n_segs < 1 || !hap_off || !seg_sites ||
        tile_seqs < 0 || store_len < 0)
        return pg_fail(PG_ERR_ARG, "pg_s2g_dev_plan: bad argument");
    pg_ctx::S2gDev &D = c->s2g;
    D.planned = false;
    if ((size_t)store_len + PGS_STORE_SLACK > D.store.cap) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_plan: the store holds fewer residues");
    const int tq = pgs_tile_seqs(n_haps, tile_seqs, PGS_LDS_BYTES);
    const int n_tiles = (n_haps + tq - 1) / tq;
    std::vector<int32_t> tstart((size_t)n_tiles + 1, 0);
    const int32_t broken = pgs_tile_starts(tmpl, tmpl_len, n_haps, tq, tstart.data());
    if (broken) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_plan: template entry %d: the haplotypes' indices must rise by one, four entries each at most", broken - 1);
    for (int64_t s = 0; s < n_segs; ++s) {
        if (name_off[s + 1] < name_off[s] || name_off[s + 1] - name_off[s] > PGS_MAX_NAME) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_plan: bad name table");
        for (int32_t h = 0; h < n_haps; ++h)
            if (seg_sites[s] < 0 || hap_off[s * n_haps + h] < 0 || hap_off[s * n_haps + h] + seg_sites[s] > store_len)
                return pg_fail(PG_ERR_ARG, "pg_s2g_dev_plan: segment %lld, haplotype %d: its sites lie outside the store", (long long)s, h);
    }
    if (name_off[0] != 0 || (name_off[n_segs] && !names)) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_plan: bad name table");
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    int rc;
    if ((rc = D.tmpl.ensure((size_t)tmpl_len)) != PG_OK || (rc = D.tstart.ensure((size_t)n_tiles + 1)) != PG_OK ||
        (rc = D.names.ensure((size_t)name_off[n_segs] + 1)) != PG_OK || (rc = D.name_off.ensure((size_t)n_segs + 1)) != PG_OK ||
        (rc = D.hap_off.ensure((size_t)n_segs * (size_t)n_haps)) != PG_OK)
        return rc;
    HIPCHK(hipMemcpy(D.tmpl.p, tmpl, (size_t)tmpl_len * 4, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.tstart.p, tstart.data(), ((size_t)n_tiles + 1) * 4, hipMemcpyHostToDevice));
    if (name_off[n_segs]) HIPCHK(hipMemcpy(D.names.p, names, (size_t)name_off[n_segs], hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.name_off.p, name_off, ((size_t)n_segs + 1) * 8, hipMemcpyHostToDevice));
    HIPCHK(hipMemcpy(D.hap_off.p, hap_off, (size_t)n_segs * (size_t)n_haps * 8, hipMemcpyHostToDevice));
    D.h_name_off.assign(name_off, name_off + n_segs + 1);
    D.h_seg_sites.assign(seg_sites, seg_sites + n_segs);
    D.tmpl_len = tmpl_len;
    D.n_haps = n_haps;
    D.n_segs = n_segs;
    D.tile_seqs = tq;
    D.n_tiles = n_tiles;
    D.store_len = store_len;
    D.planned = true;
    if (tile_seqs_out) *tile_seqs_out = tq;
    return PG_OK;
}

// A range of the output: n_pieces pieces, piece k the lines x0[k] .. x1[k] - 1 of segment seg[k], one behind the other.  out_len must
// be what the closed form gives.  The rows lie on the device behind it (pg_s2g_dev_rows, which = 0); bgzf != 0: k_deflate makes BGZF
// members of them too (*bgzf_len_out bytes, which = 1).  
extern "C" int pg_s2g_dev_emit(pg_ctx *c, const int32_t *seg, const int64_t *x0, const int64_t *x1, int64_t n_pieces, int64_t out_len, int bgzf,
                               int64_t *bgzf_len_out) {
    if (!c || !c->s2g.configured || !c->s2g.planned) return pg_fail(PG_ERR_STATE, "pg_s2g_dev_emit: pg_s2g_dev_plan must be called first");
    if (n_pieces < 0 || (n_pieces && (!seg || !x0 || !x1)) || out_len < 0) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_emit: bad argument");
    pg_ctx::S2gDev &D = c->s2g;
    if (bgzf_len_out) *bgzf_len_out = 0;
    std::vector<S2gJob> jobs;
    int64_t at = 0;
    for (int64_t k = 0; k < n_pieces; ++k) {
        if (seg[k] < 0 || seg[k] >= D.n_segs || x0[k] < 0 || x1[k] < x0[k] || x1[k] > D.h_seg_sites[(size_t)seg[k]]) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_emit: bad piece %lld", (long long)k);
        const uint64_t fixed = pgs_line_fixed((uint32_t)(D.h_name_off[(size_t)seg[k] + 1] - D.h_name_off[(size_t)seg[k]]), (uint32_t)D.tmpl_len);
        const uint64_t start0 = pgs_line_start((uint64_t)x0[k], fixed);
        for (int64_t s = x0[k]; s < x1[k]; s += PGS_TILE_SITES)
            jobs.push_back(S2gJob{s, at + (int64_t)(pgs_line_start((uint64_t)s, fixed) - start0), seg[k], (int32_t)std::min<int64_t>(PGS_TILE_SITES, x1[k] - s)});
        at += (int64_t)(pgs_line_start((uint64_t)x1[k], fixed) - start0);
    }
    if (at != out_len) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_emit: the pieces take %lld bytes, not %lld", (long long)at, (long long)out_len);
    D.out_len = out_len;
    if (jobs.empty()) return PG_OK;
    if (jobs.size() > 0x7fffffffull) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_emit: more than 2^31 tiles in a range");
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream_up;
    int rc;
    if ((rc = D.out.ensure_roomy((size_t)out_len + 64)) != PG_OK || (rc = D.jobs.ensure_roomy(jobs.size() * sizeof(S2gJob))) != PG_OK ||
        (rc = D.est.status.ensure(PGL_STATUS_WORDS)) != PG_OK || (rc = D.est.h_status.ensure(PGL_STATUS_WORDS)) != PG_OK)
        return rc;
    HIPCHK(hipMemcpyAsync(D.jobs.p, jobs.data(), jobs.size() * sizeof(S2gJob), hipMemcpyHostToDevice, st));
    S2gTileArgs A;
    A.store = D.store.p;
    A.jobs = reinterpret_cast<const S2gJob *>(D.jobs.p);
    A.names = D.names.p;
    A.name_off = D.name_off.p;
    A.hap_off = D.hap_off.p;
    A.tmpl = D.tmpl.p;
    A.tstart = D.tstart.p;
    A.out = D.out.p;
    A.n_haps = D.n_haps;
    A.tmpl_len = D.tmpl_len;
    A.tile_seqs = D.tile_seqs;
    const size_t lds = (size_t)D.tile_seqs * (PGS_TILE_PITCH + 16);
    hipLaunchKernelGGL(k_s2g_tile, dim3((unsigned)jobs.size(), (unsigned)D.n_tiles), dim3(PGS_TILE_THREADS), lds, st, A);
    HIPCHK(hipGetLastError());
    if (bgzf) {
        pgl_preset(D.est.h_status.p, false);
        D.est.h_status.p[PGL_ST_BYTES] = out_len;
        if ((rc = pg_line_status_upload(D.est, st)) != PG_OK) return rc;
        long long *est = reinterpret_cast<long long *>(D.est.status.p);
        if ((rc = pg_deflate_queue(c, st, c->deflate, D.out.p, est + PGL_ST_BYTES, (int64_t)D.out.cap - 64, est, est + PGL_ST_BGZF_BYTES)) != PG_OK)
            return rc;
        HIPCHK(hipMemcpyAsync(D.est.h_status.p, D.est.status.p, PGL_STATUS_WORDS * 8, hipMemcpyDeviceToHost, st));
    }
    HIPCHK(hipStreamSynchronize(st));                             // (jobs leaves scope; the rows are read next)
    if (bgzf && bgzf_len_out) *bgzf_len_out = D.est.h_status.p[PGL_ST_BGZF_BYTES];
    ++D.out_ranges;
    return PG_OK;
}

// which = 0: the range's rows; 1: its BGZF members
extern "C" int pg_s2g_dev_rows(pg_ctx *c, int which, uint8_t *dst, int64_t len) {
    if (!c || !c->s2g.configured || which < 0 || which > 1) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_rows: bad argument");
    DevBuf<uint8_t> &B = which ? c->deflate.comp : c->s2g.out;
    return pg_line_rows(c, B, dst, len, "pg_s2g_dev_rows: bad length");
}

extern "C" int pg_s2g_dev_stats(pg_ctx *c, int64_t *blocks_out, int64_t *host_blocks_out, int64_t *out_ranges_out) {
    if (!out_ranges_out) return pg_fail(PG_ERR_ARG, "pg_s2g_dev_stats: null argument");
    int rc = pg_line_stats(c ? &c->s2g : nullptr, blocks_out, host_blocks_out, "pg_s2g_dev_stats");
    if (rc == PG_OK) *out_ranges_out = c->s2g.out_ranges;
    return rc;
}
