// `.geno` files joined by site on the device: the mergeGeno.py drop-in's route for lines of the regular spelling (fields split by single
// tabs, no other ASCII whitespace, the header's field count, ASCII, a final line feed) and a one-byte separator.  The per-line rules are
// csrc/pg_merge_core.h (the host route pg_merge_text in pg_merge.cpp runs the same functions), the rounds are planned by
// csrc/pg_merge_plan.h; this file is the division of the work over the chip and the host side of the entry points.
//
// Every input file owns a text region with its line feeds listed.  A block arrives through the tokenizer's text slot 0 (text copied, or
// bgzip's members inflated by k_inflate) and is put behind the lines the rounds before left in the region (two buffers, turn about).
//
//   k_merge_keys   a wavefront per line -- the check of the spelling reads every byte of the line, 64 consecutive bytes a step, which a
//                  lane per line would spread over 64 lines; not measured against it.  The tabs are counted by ballots, the first two
//                  give the scaffold and the position; the scaffold's hash is a sum over its bytes (a lane a byte), looked up in an
//                  open-addressed table over the .fai's names: a few probes a line however many names the .fai has.  (Comparing a
//                  line's name with the line before first, and resolving the index once per run of equal names, is not done and
//                  not measured.)  It writes the key, the bytes of
//                  `scaffold <tab> position`, and a flag for a line that is no site or is outside the regular spelling
//   k_merge_stop   a thread per line: the first line that is no site or does not lie behind the line before (atomicMin per file)
//   k_merge_lines  the sparse methods, a thread per line of the candidate files: binary searches in the other files' keys give the
//   k_merge_pos    presence mask and the line's place in the merged order; the dense methods, a thread per position of the range.
//                  Rule 3, then the length of the written line (0: nothing is written)
//   scan           the lines' places (k_rows_scan, pg_line_slot.hip)
//   k_merge_emit   a wavefront per written line: a lane per file finds the file's line, then the head (copied from the text, or the
//                  .fai's name and the position rendered) and every file's cells or dummy cells, 64 consecutive bytes a step, tabs
//                  turned into the separator.  Plain vector stores
#include "pg_ctx.h"
#include "pg_merge_core.h"
#include "pg_wave.h"

#include <algorithm>
#include <cstring>

int pg_tok_text_submit(pg_ctx *c, int slot, const char *text, int fd, int64_t file_offset, int64_t len);
int pg_tok_lines(pg_ctx *c, int slot, int64_t *n_lines_out);
int pg_tok_bgzf_submit(pg_ctx *c, int slot, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                       const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                       int64_t text_len, int64_t line_len_hint);
int pg_tok_crc_result(pg_ctx *c, int slot);

namespace {

#define PGM_NONE 0x7fffffffffffffffll
#define PGM_FSTAT 8     // per file on the device: [0] stopping line, [1] first line outside the regular spelling, [2] [3] the key of the
                        // last line consumed, [4] lines of the round, [5] where the region begins behind the round

struct MFile {
    DevBuf<uint8_t> text[2], flag;
    DevBuf<int64_t> nl[2], kpos;
    DevBuf<int32_t> kscaf;
    DevBuf<uint32_t> head;
    int cur = 0;
    int64_t len = 0, n_lines = 0, n_ok = 0, base_line = 0, base_byte = 0, keyed = 0;
    void release() {
        for (int k = 0; k < 2; ++k) { text[k].release(); nl[k].release(); }
        flag.release(); kpos.release(); kscaf.release(); head.release();
    }
};

struct MergeDev {
    pg_merge_cfg cfg;
    uint8_t sep = '\t';
    int32_t n_cols[PGM_MAX_FILES] = {};
    DevBuf<uint8_t> names, missing, out;
    DevBuf<int64_t> name_off, fai_len, off, src;
    DevBuf<int32_t> table;
    DevBuf<uint32_t> len;
    uint32_t mask = 0;
    MFile f[PGM_MAX_FILES];
    DevBuf<pgm_view> views;
    HostPin<pgm_view> h_views;
    DevBuf<long long> fstat, info, status;
    HostPin<long long> h_fstat, h_info, h_status;
    pg_ctx::Deflate df;
    bool bgzf = false, timing = false;
    hipEvent_t ev[4] = {};
    int64_t rounds = 0, out_bytes = 0, bgzf_bytes = 0;
    double keys_ms = 0, match_ms = 0, emit_ms = 0;
};

__global__ __launch_bounds__(256) void k_merge_nl(const int64_t *__restrict__ src, int64_t n, int64_t shift, int64_t *__restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] = src[i] + shift;
}

__global__ void k_merge_reset(long long *fs) {
    fs[0] = PGM_NONE;
    fs[1] = PGM_NONE;
}

struct KeysArgs {
    const uint8_t *text;
    const int64_t *nl;
    int64_t first, n_lines, base;
    int n_cols;
    int32_t *kscaf;
    int64_t *kpos;
    uint32_t *head;
    uint8_t *flag;
    long long *fs;
};

__global__ __launch_bounds__(256) void k_merge_keys(KeysArgs A, pgm_fai F) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t i = A.first + (int64_t)blockIdx.x * 4 + wave;
    if (i >= A.n_lines) return;
    const int64_t ls = i ? A.nl[i - 1] + 1 : 0, le = A.nl[i];
    const uint8_t *line = A.text + ls;
    bool irr = le - ls <= 0 || le - ls > 0x7fffffffll;
    const uint32_t n = irr ? 0u : (uint32_t)(le - ls);
    uint32_t ntab = 0, t0 = 0, t1 = 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t k = base + (uint32_t)lane;
        const bool in = k < n;
        const uint8_t b = in ? line[k] : (uint8_t)'x';
        const uint8_t before = in && k > 0 ? line[k - 1] : (uint8_t)'x';
        const bool tab = in && b == '\t';
        const bool bad = in && (pgm_irregular(b) || (tab && (k == 0 || k == n - 1 || before == '\t')));
        const uint64_t m = __ballot(tab);
        irr = irr || __ballot(bad) != 0;
        if (m) {
            const uint64_t m2 = m & (m - 1);
            if (ntab == 0) {
                t0 = base + (uint32_t)__ffsll((unsigned long long)m) - 1;
                if (m2) t1 = base + (uint32_t)__ffsll((unsigned long long)m2) - 1;
            } else if (ntab == 1)
                t1 = base + (uint32_t)__ffsll((unsigned long long)m) - 1;
        }
        ntab += (uint32_t)__popcll(m);
    }
    int why = PGM_OK;
    int32_t scaf = -1;
    int64_t pos = 0;
    uint32_t head = 0;
    if (irr || ntab != (uint32_t)(A.n_cols - 1)) {
        why = PGM_IRREGULAR;
    } else {
        const uint32_t e1 = A.n_cols > 2 ? t1 : n;
        head = e1;
        uint32_t sum = 0;
        for (uint32_t k = (uint32_t)lane; k < t0; k += 64) sum += pgm_hash_byte(line[k], k);
        sum = pg_wave_sum(sum);
        if (F.n > 0) {
            for (uint32_t at = pgm_hash_end(sum, t0) & F.mask;; at = (at + 1) & F.mask) {
                const int32_t e = F.table[at];
                if (e < 0) break;
                const int64_t a = F.name_off[e];
                if (F.name_off[e + 1] - a != (int64_t)t0) continue;
                bool differ = false;
                for (uint32_t k = (uint32_t)lane; k < t0; k += 64) differ = differ || F.names[a + k] != line[k];
                if (__ballot(differ) == 0) { scaf = e; break; }
            }
        }
        if (scaf < 0) {
            why = PGM_STOP_SCAF;
        } else {
            why = pgm_parse_pos(line + t0 + 1, (int64_t)e1 - (int64_t)t0 - 1, &pos);
            if (why == PGM_OK && (pos < 1 || pos > F.len[scaf])) why = PGM_STOP_RANGE;
            if (why == PGM_E_DIGITS) why = PGM_IRREGULAR;              // (the host route words the rejection)
            if (why != PGM_OK) scaf = -1;
        }
    }
    if (lane == 0) {
        A.kscaf[i] = scaf;
        A.kpos[i] = pos;
        A.head[i] = head;
        A.flag[i] = (uint8_t)why;
        if (why == PGM_IRREGULAR) atomicMin(A.fs + 1, (long long)i);
    }
}

__global__ __launch_bounds__(256) void k_merge_stop(KeysArgs A) {
    const int64_t i = A.first + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= A.n_lines) return;
    bool bad = A.flag[i] != PGM_OK;
    if (!bad) {
        if (i == A.base) bad = A.fs[2] >= 0 && !pgm_key_less((int32_t)A.fs[2], A.fs[3], A.kscaf[i], A.kpos[i]);
        else bad = A.flag[i - 1] == PGM_OK && !pgm_key_less(A.kscaf[i - 1], A.kpos[i - 1], A.kscaf[i], A.kpos[i]);
    }
    if (bad) atomicMin(A.fs, (long long)i);
}

// per file: what pg_merge_dev_keys reports (see include/popgen_hip.h)
__global__ void k_merge_info(const pgm_view *V, const uint8_t *const *flags, const int64_t *lens, const long long *fstat, int n_files, long long *info) {
    const int f = (int)threadIdx.x;
    if (f >= n_files) return;
    const pgm_view v = V[f];
    const long long *fs = fstat + f * PGM_FSTAT;
    const int64_t n_lines = v.hi;
    const int64_t stop = fs[0] < n_lines ? fs[0] : n_lines;
    const bool ragged = lens[f] > 0 && (n_lines == 0 || v.nl[n_lines - 1] != lens[f] - 1);
    long long *o = info + f * 8;
    o[0] = n_lines - v.lo;
    o[1] = stop - v.lo;
    o[2] = stop > v.lo ? v.kscaf[stop - 1] : -1;
    o[3] = stop > v.lo ? v.kpos[stop - 1] : 0;
    o[4] = stop < n_lines ? (flags[f][stop] ? flags[f][stop] : PGM_STOP_ORDER) : 0;
    o[5] = stop - v.lo;
    o[6] = ((fs[1] < n_lines && fs[1] <= stop) || ragged) ? 1 : 0;       // (behind a stopping line of the regular spelling nothing counts)
    o[7] = lens[f] - (v.lo ? v.nl[v.lo - 1] + 1 : 0);            // (what the rounds consumed is no longer resident)
}

__global__ __launch_bounds__(256) void k_merge_lines(const pgm_view *V, pg_merge_cfg cfg, int f, int32_t hs, int64_t hp, uint32_t *len, int64_t *src,
                                                     int64_t n_slots, long long *status) {
    const int64_t i = V[f].lo + (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= V[f].hi) return;
    int64_t slot = 0;
    const int64_t n = pgm_match_line(cfg, V, f, i, hs, hp, &slot);
    if (slot < 0 || slot >= n_slots || n > 0xffffffffll) {            // (cannot be: the slots are a permutation; a line of 4 GiB is the host's)
        atomicOr(reinterpret_cast<unsigned long long *>(status), (unsigned long long)PG_ST_HOST);
        return;
    }
    len[slot] = (uint32_t)n;
    src[slot] = ((int64_t)f << 56) | i;
}

__global__ __launch_bounds__(256) void k_merge_pos(const pgm_view *V, pg_merge_cfg cfg, pgm_fai F, int32_t s, int64_t p0, int64_t n, uint32_t *len,
                                                   long long *status) {
    const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    const int64_t m = pgm_match_pos(cfg, V, F, s, p0 + 1 + j);
    if (m > 0xffffffffll) atomicOr(reinterpret_cast<unsigned long long *>(status), (unsigned long long)PG_ST_HOST);
    len[j] = m > 0xffffffffll ? 0u : (uint32_t)m;
}

// per file: the lines at or below the horizon, where the region begins behind them, the key of the last one
__global__ void k_merge_done(const pgm_view *V, int n_files, int32_t hs, int64_t hp, long long *fstat) {
    const int f = (int)threadIdx.x;
    if (f >= n_files) return;
    const pgm_view v = V[f];
    const int64_t e = pgm_upper_bound(v, hs, hp);
    long long *fs = fstat + f * PGM_FSTAT;
    fs[4] = e - v.lo;
    fs[5] = e > v.lo ? v.nl[e - 1] + 1 : -1;
    if (e > v.lo) {
        fs[2] = v.kscaf[e - 1];
        fs[3] = v.kpos[e - 1];
    }
}

__device__ __forceinline__ int64_t shfl64(int64_t v, int lane) {
    const int lo = __shfl((int)(uint32_t)(uint64_t)v, lane, 64), hi = __shfl((int)(uint32_t)((uint64_t)v >> 32), lane, 64);
    return (int64_t)(((uint64_t)(uint32_t)hi << 32) | (uint64_t)(uint32_t)lo);
}

__global__ __launch_bounds__(256) void k_merge_emit(const pgm_view *V, pg_merge_cfg cfg, pgm_fai F, uint8_t sep, const uint8_t *missing, int dense,
                                                    int32_t s, int64_t p0, const uint32_t *len, const int64_t *off, const int64_t *src,
                                                    int64_t n_slots, uint8_t *out) {
    const int lane = (int)(threadIdx.x & 63), wave = (int)(threadIdx.x >> 6);
    const int64_t slot = (int64_t)blockIdx.x * 4 + wave;
    if (slot >= n_slots || len[slot] == 0) return;
    int32_t ks = s;
    int64_t kp = p0 + 1 + slot;
    if (!dense) {
        const int64_t w = src[slot];
        const int f0 = (int)(w >> 56);
        const int64_t i0 = w & 0x00ffffffffffffffll;
        ks = V[f0].kscaf[i0];
        kp = V[f0].kpos[i0];
    }
    const int64_t mine = lane < cfg.n_files ? pgm_find(V[lane], ks, kp) : -1;
    const uint64_t held = __ballot(mine >= 0);
    uint8_t *o = out + off[slot];
    int64_t w = 0;
    if (held) {
        const int g = __ffsll((unsigned long long)held) - 1;
        const int64_t li = shfl64(mine, g);
        int64_t ls, le;
        pgm_line_at(V[g], li, &ls, &le);
        const int64_t hl = V[g].head[li];
        const uint8_t *t = V[g].text + ls;
        for (int64_t k = lane; k < hl; k += 64) {
            const uint8_t b = t[k];
            o[k] = b == '\t' ? sep : b;
        }
        w = hl;
    } else {
        const int64_t a = F.name_off[ks], nn = F.name_off[ks + 1] - a;
        for (int64_t k = lane; k < nn; k += 64) o[k] = F.names[a + k];
        const int nd = pgm_digits(kp);
        if (lane == 0) o[nn] = sep;
        if (lane < nd) {
            int64_t v = kp;
            for (int k = 0; k < nd - 1 - lane; ++k) v /= 10;
            o[nn + 1 + lane] = (uint8_t)('0' + v % 10);
        }
        w = nn + 1 + nd;
    }
    for (int g = 0; g < cfg.n_files; ++g) {
        if (!(cfg.out_mask >> g & 1u)) continue;
        const int64_t li = shfl64(mine, g);
        if (li >= 0) {
            int64_t ls, le;
            pgm_line_at(V[g], li, &ls, &le);
            const int64_t hl = V[g].head[li], cnt = le - ls - hl;
            const uint8_t *t = V[g].text + ls + hl;
            for (int64_t k = lane; k < cnt; k += 64) {
                const uint8_t b = t[k];
                o[w + k] = b == '\t' ? sep : b;
            }
            w += cnt;
        } else {
            const int64_t per = 1 + cfg.missing_len, cnt = (int64_t)V[g].n_cells * per;
            for (int64_t k = lane; k < cnt; k += 64) {
                const int64_t r = k % per;
                o[w + k] = r == 0 ? sep : missing[r - 1];
            }
            w += cnt;
        }
    }
    if (lane == 0) o[w] = '\n';
}

MergeDev *state(pg_ctx *c) { return c ? static_cast<MergeDev *>(c->merge) : nullptr; }

int check(pg_ctx *c, const char *who) {
    if (!c) return pg_fail(PG_ERR_ARG, "%s: null context", who);
    if (!c->merge) return pg_fail(PG_ERR_STATE, "%s: pg_merge_dev_config must be called first", who);
    return PG_OK;
}

pgm_fai fai_of(const MergeDev &D) { return pgm_fai{D.names.p, D.name_off.p, D.fai_len.p, D.table.p, D.mask, D.cfg.n_fai}; }

// the files' views to the device; hi: the lines resident (before the keys are known) or the consumable ones
int put_views(pg_ctx *c, MergeDev &D, bool consumable) {
    const int nf = D.cfg.n_files;
    int rc;
    if ((rc = D.views.ensure(PGM_MAX_FILES)) != PG_OK || (rc = D.h_views.ensure(PGM_MAX_FILES)) != PG_OK) return rc;
    for (int f = 0; f < nf; ++f) {
        MFile &M = D.f[f];
        pgm_view &v = D.h_views.p[f];
        v.text = M.text[M.cur].p;
        v.nl = M.nl[M.cur].p;
        v.kscaf = M.kscaf.p;
        v.kpos = M.kpos.p;
        v.head = M.head.p;
        v.lo = M.base_line;
        v.hi = consumable ? M.n_ok : M.n_lines;
        v.n_cells = D.n_cols[f] > 2 ? D.n_cols[f] - 2 : 0;
        v.n_cols = D.n_cols[f];
    }
    HIPCHK(hipMemcpyAsync(D.views.p, D.h_views.p, sizeof(pgm_view) * (size_t)nf, hipMemcpyHostToDevice, c->stream_up));
    return PG_OK;
}

// the block in the tokenizer's slot 0 behind what the rounds before left of file f
int take_block(pg_ctx *c, MergeDev &D, int f) {
    hipStream_t st = c->stream_up;
    int64_t n_new = 0;
    int rc = pg_tok_lines(c, 0, &n_new);
    if (rc != PG_OK) return rc;
    pg_ctx::TokSlot &T = c->tok[0];
    MFile &M = D.f[f];
    const int64_t new_len = T.len, rem_len = M.len - M.base_byte, rem_lines = M.n_lines - M.base_line;
    const int nxt = M.cur ^ 1;
    if ((rc = M.text[nxt].ensure_roomy((size_t)(rem_len + new_len) + 64)) != PG_OK || (rc = M.nl[nxt].ensure_roomy((size_t)(rem_lines + n_new) + 1)) != PG_OK)
        return rc;
    if (rem_len) HIPCHK(hipMemcpyAsync(M.text[nxt].p, M.text[M.cur].p + M.base_byte, (size_t)rem_len, hipMemcpyDeviceToDevice, st));
    if (new_len) HIPCHK(hipMemcpyAsync(M.text[nxt].p + rem_len, T.tp, (size_t)new_len, hipMemcpyDeviceToDevice, st));
    if (rem_lines) hipLaunchKernelGGL(k_merge_nl, dim3((unsigned)((rem_lines + 255) / 256)), dim3(256), 0, st, M.nl[M.cur].p + M.base_line, rem_lines, -M.base_byte, M.nl[nxt].p);
    if (n_new) hipLaunchKernelGGL(k_merge_nl, dim3((unsigned)((n_new + 255) / 256)), dim3(256), 0, st, T.nl.p, n_new, rem_len, M.nl[nxt].p + rem_lines);
    hipLaunchKernelGGL(k_merge_reset, dim3(1), dim3(1), 0, st, D.fstat.p + f * PGM_FSTAT);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(st));                              // (slot 0 takes the next file's block)
    if ((rc = pg_tok_crc_result(c, 0)) != PG_OK) return rc;
    M.cur = nxt;
    M.len = rem_len + new_len;
    M.n_lines = rem_lines + n_new;
    M.n_ok = 0;
    M.base_line = M.base_byte = M.keyed = 0;
    return PG_OK;
}

float elapsed(hipEvent_t a, hipEvent_t b) {
    float ms = 0;
    return hipEventElapsedTime(&ms, a, b) == hipSuccess ? ms : 0.f;
}

}  // namespace

extern "C" int pg_merge_dev_end(pg_ctx *c) {
    MergeDev *D = state(c);
    if (!D) return PG_OK;
    (void)hipSetDevice(c->device);
    (void)hipStreamSynchronize(c->stream_up);
    for (MFile &M : D->f) M.release();
    D->names.release(); D->missing.release(); D->out.release(); D->name_off.release(); D->fai_len.release(); D->off.release(); D->src.release();
    D->table.release(); D->len.release(); D->views.release(); D->h_views.release(); D->fstat.release(); D->info.release(); D->status.release();
    D->h_fstat.release(); D->h_info.release(); D->h_status.release(); D->df.release();
    for (hipEvent_t &e : D->ev)
        if (e) (void)hipEventDestroy(e);
    delete D;
    c->merge = nullptr;
    return PG_OK;
}

extern "C" int pg_merge_dev_config(pg_ctx *c, const pg_merge_cfg *cfg, const char *sep, const char *missing, const char *fai_names,
                                   const int64_t *name_off, const int64_t *fai_len, const int32_t *n_cols, int *taken_out) {
    if (!c || !cfg || !taken_out || !n_cols || cfg->n_files < 1 || cfg->n_files > PGM_MAX_FILES || cfg->n_fai < 0 || cfg->method < 0 || cfg->method > 2 ||
        cfg->sep_len < 0 || cfg->missing_len < 0 || (cfg->n_fai > 0 && (!fai_names || !name_off || !fai_len)) || (cfg->sep_len && !sep) ||
        (cfg->missing_len && !missing))
        return pg_fail(PG_ERR_ARG, "pg_merge_dev_config: bad argument");
    *taken_out = 0;
    pg_merge_dev_end(c);
    if (cfg->sep_len != 1 || cfg->missing_len > PGM_MAX_MISSING || cfg->n_fai < 1) return PG_OK;
    for (int f = 0; f < cfg->n_files; ++f)
        if (n_cols[f] < 2) return PG_OK;
    for (int32_t s = 0; s < cfg->n_fai; ++s)
        if (name_off[s + 1] < name_off[s]) return pg_fail(PG_ERR_ARG, "pg_merge_dev_config: the names' offsets do not increase");
    HIPCHK(hipSetDevice(c->device));
    MergeDev *D = new MergeDev();
    c->merge = D;
    D->cfg = *cfg;
    D->sep = (uint8_t)sep[0];
    memcpy(D->n_cols, n_cols, sizeof(int32_t) * (size_t)cfg->n_files);
    uint32_t size = 4;
    while (size < 2u * (uint32_t)cfg->n_fai) size <<= 1;
    std::vector<int32_t> table(size, -1);
    D->mask = size - 1;
    const uint8_t *names = reinterpret_cast<const uint8_t *>(fai_names);
    for (int32_t s = 0; s < cfg->n_fai; ++s) {
        uint32_t at = pgm_hash(names + name_off[s], name_off[s + 1] - name_off[s]) & D->mask;
        while (table[at] >= 0) at = (at + 1) & D->mask;
        table[at] = s;
    }
    hipStream_t st = c->stream_up;
    const size_t nb = (size_t)name_off[cfg->n_fai];
    int rc;
    if (nb == 0) return pg_fail(PG_ERR_ARG, "pg_merge_dev_config: the .fai's names are empty");
    if ((rc = D->names.upload(names, nb, st)) != PG_OK) return rc;
    if ((rc = D->name_off.upload(name_off, (size_t)cfg->n_fai + 1, st)) != PG_OK || (rc = D->fai_len.upload(fai_len, (size_t)cfg->n_fai, st)) != PG_OK ||
        (rc = D->table.upload(table.data(), size, st)) != PG_OK || (rc = D->missing.ensure(PGM_MAX_MISSING)) != PG_OK)
        return rc;
    if (cfg->missing_len) HIPCHK(hipMemcpyAsync(D->missing.p, missing, (size_t)cfg->missing_len, hipMemcpyHostToDevice, st));
    if ((rc = D->fstat.ensure(PGM_MAX_FILES * PGM_FSTAT)) != PG_OK || (rc = D->h_fstat.ensure(PGM_MAX_FILES * PGM_FSTAT)) != PG_OK ||
        (rc = D->info.ensure(PGM_MAX_FILES * 8 + 3 * PGM_MAX_FILES)) != PG_OK || (rc = D->h_info.ensure(PGM_MAX_FILES * 8 + 3 * PGM_MAX_FILES)) != PG_OK ||
        (rc = D->status.ensure(8)) != PG_OK || (rc = D->h_status.ensure(8)) != PG_OK)
        return rc;
    for (int f = 0; f < PGM_MAX_FILES; ++f) {
        long long *fs = D->h_fstat.p + f * PGM_FSTAT;
        fs[0] = fs[1] = PGM_NONE;
        fs[2] = -1;
        fs[3] = fs[4] = fs[5] = fs[6] = fs[7] = 0;
    }
    HIPCHK(hipMemcpyAsync(D->fstat.p, D->h_fstat.p, sizeof(long long) * PGM_MAX_FILES * PGM_FSTAT, hipMemcpyHostToDevice, st));
    HIPCHK(hipStreamSynchronize(st));                              // (the names, the table: host memory that goes away)
    *taken_out = 1;
    return PG_OK;
}

extern "C" int pg_merge_dev_submit(pg_ctx *c, int f, const char *text, int64_t len) {
    int rc = check(c, "pg_merge_dev_submit");
    if (rc != PG_OK) return rc;
    MergeDev &D = *state(c);
    if (f < 0 || f >= D.cfg.n_files || len < 0 || (len && !text)) return pg_fail(PG_ERR_ARG, "pg_merge_dev_submit: bad file or text");
    if ((rc = pg_tok_text_submit(c, 0, text, -1, 0, len)) != PG_OK) return rc;
    return take_block(c, D, f);
}

extern "C" int pg_merge_dev_submit_bgzf(pg_ctx *c, int f, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off, const uint32_t *in_len,
                                        const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head, int64_t head_len,
                                        int64_t text_len) {
    int rc = check(c, "pg_merge_dev_submit_bgzf");
    if (rc != PG_OK) return rc;
    MergeDev &D = *state(c);
    if (f < 0 || f >= D.cfg.n_files || text_len < 0) return pg_fail(PG_ERR_ARG, "pg_merge_dev_submit_bgzf: bad file or length");
    if ((rc = pg_tok_bgzf_submit(c, 0, comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, 1024)) != PG_OK) return rc;
    return take_block(c, D, f);
}

extern "C" int pg_merge_dev_keys(pg_ctx *c, int64_t *info) {
    int rc = check(c, "pg_merge_dev_keys");
    if (rc != PG_OK) return rc;
    if (!info) return pg_fail(PG_ERR_ARG, "pg_merge_dev_keys: null argument");
    MergeDev &D = *state(c);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream_up;
    const int nf = D.cfg.n_files;
    const pgm_fai F = fai_of(D);
    if (D.timing)
        for (hipEvent_t &e : D.ev)
            if (!e) HIPCHK(hipEventCreate(&e));
    if (D.timing) HIPCHK(hipEventRecord(D.ev[0], st));
    for (int f = 0; f < nf; ++f) {
        MFile &M = D.f[f];
        if (M.keyed >= M.n_lines) continue;
        const size_t n = (size_t)M.n_lines;
        if (M.keyed == 0 && ((rc = M.kscaf.ensure_roomy(n)) != PG_OK || (rc = M.kpos.ensure_roomy(n)) != PG_OK || (rc = M.head.ensure_roomy(n)) != PG_OK ||
                             (rc = M.flag.ensure_roomy(n)) != PG_OK))
            return rc;
        if (M.kscaf.cap < n) return pg_fail(PG_ERR_STATE, "pg_merge_dev_keys: the keys of file %d do not cover its lines", f);
        const KeysArgs A{M.text[M.cur].p, M.nl[M.cur].p, M.keyed, M.n_lines, M.base_line, D.n_cols[f], M.kscaf.p, M.kpos.p, M.head.p, M.flag.p,
                         D.fstat.p + f * PGM_FSTAT};
        const int64_t todo = M.n_lines - M.keyed;
        hipLaunchKernelGGL(k_merge_keys, dim3((unsigned)((todo + 3) / 4)), dim3(256), 0, st, A, F);
        hipLaunchKernelGGL(k_merge_stop, dim3((unsigned)((todo + 255) / 256)), dim3(256), 0, st, A);
        HIPCHK(hipGetLastError());
        M.keyed = M.n_lines;
    }
    if (D.timing) HIPCHK(hipEventRecord(D.ev[1], st));
    if ((rc = put_views(c, D, false)) != PG_OK) return rc;
    // the flags' addresses and the regions' lengths ride behind the info words
    long long *h = D.h_info.p + PGM_MAX_FILES * 8;
    for (int f = 0; f < nf; ++f) {
        h[f] = (long long)reinterpret_cast<uintptr_t>(D.f[f].flag.p);
        h[PGM_MAX_FILES + f] = D.f[f].len;
    }
    long long *d = D.info.p + PGM_MAX_FILES * 8;
    HIPCHK(hipMemcpyAsync(d, h, sizeof(long long) * 2 * PGM_MAX_FILES, hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(k_merge_info, dim3(1), dim3(64), 0, st, D.views.p, reinterpret_cast<const uint8_t *const *>(d),
                       reinterpret_cast<const int64_t *>(d + PGM_MAX_FILES), D.fstat.p, nf, D.info.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D.h_info.p, D.info.p, sizeof(long long) * 8 * (size_t)nf, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (D.timing) D.keys_ms += elapsed(D.ev[0], D.ev[1]);
    for (int f = 0; f < nf; ++f) {
        const long long *o = D.h_info.p + f * 8;
        for (int k = 0; k < 8; ++k) info[f * 8 + k] = o[k];
        D.f[f].n_ok = D.f[f].base_line + o[1];
    }
    return PG_OK;
}

extern "C" int pg_merge_dev_set_output(pg_ctx *c, int bgzf) {
    int rc = check(c, "pg_merge_dev_set_output");
    if (rc != PG_OK) return rc;
    state(c)->bgzf = bgzf != 0;
    return PG_OK;
}

extern "C" int pg_merge_dev_merge(pg_ctx *c, int dense, int32_t from_scaf, int64_t from_pos, int32_t hor_scaf, int64_t hor_pos, int64_t *done,
                                  int64_t *bytes_out, int64_t *rows_out, int64_t *bgzf_out) {
    int rc = check(c, "pg_merge_dev_merge");
    if (rc != PG_OK) return rc;
    MergeDev &D = *state(c);
    if (!done || !bytes_out || !rows_out || !bgzf_out) return pg_fail(PG_ERR_ARG, "pg_merge_dev_merge: null argument");
    const int nf = D.cfg.n_files;
    if (hor_scaf < 0 || hor_scaf >= D.cfg.n_fai || (dense && (from_scaf != hor_scaf || from_pos < 0 || hor_pos < from_pos)))
        return pg_fail(PG_ERR_ARG, "pg_merge_dev_merge: the range (%d, %lld] .. (%d, %lld] is none of the .fai or crosses a scaffold", (int)from_scaf,
                       (long long)from_pos, (int)hor_scaf, (long long)hor_pos);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream_up;
    const pgm_fai F = fai_of(D);
    if ((rc = put_views(c, D, true)) != PG_OK) return rc;
    int64_t n_slots = 0;
    const int nc = pgm_cand_files(D.cfg);
    if (dense) n_slots = hor_pos - from_pos;
    else
        for (int f = 0; f < nc; ++f) n_slots += D.f[f].n_ok - D.f[f].base_line;
    const size_t ns = (size_t)std::max<int64_t>(n_slots, 1);
    if ((rc = D.len.ensure_roomy(ns)) != PG_OK || (rc = D.off.ensure_roomy(ns)) != PG_OK || (!dense && (rc = D.src.ensure_roomy(ns)) != PG_OK)) return rc;
    long long *status = D.status.p;
    HIPCHK(hipMemsetAsync(status, 0, sizeof(long long) * 8, st));
    if (D.timing) HIPCHK(hipEventRecord(D.ev[0], st));
    if (dense) {
        if (n_slots) hipLaunchKernelGGL(k_merge_pos, dim3((unsigned)((n_slots + 255) / 256)), dim3(256), 0, st, D.views.p, D.cfg, F, hor_scaf, from_pos, n_slots, D.len.p, status);
    } else {
        for (int f = 0; f < nc; ++f) {
            const int64_t n = D.f[f].n_ok - D.f[f].base_line;
            if (n) hipLaunchKernelGGL(k_merge_lines, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, D.views.p, D.cfg, f, hor_scaf, hor_pos, D.len.p, D.src.p, n_slots, status);
        }
    }
    HIPCHK(hipGetLastError());
    if (D.timing) HIPCHK(hipEventRecord(D.ev[1], st));
    pg_rows_scan_queue(st, D.len.p, n_slots, D.off.p, status, PGM_NONE);
    hipLaunchKernelGGL(k_merge_done, dim3(1), dim3(64), 0, st, D.views.p, nf, hor_scaf, hor_pos, D.fstat.p);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(D.h_status.p, status, sizeof(long long) * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipMemcpyAsync(D.h_fstat.p, D.fstat.p, sizeof(long long) * PGM_FSTAT * (size_t)nf, hipMemcpyDeviceToHost, st));
    HIPCHK(hipStreamSynchronize(st));
    if (D.h_status.p[0]) return pg_fail(PG_ERR_STATE, "pg_merge_dev_merge: a written line does not fit 4 GiB");
    const int64_t total = D.h_status.p[2];
    *bytes_out = total;
    *rows_out = D.h_status.p[3];
    *bgzf_out = 0;
    D.out_bytes = total;
    D.bgzf_bytes = 0;
    if ((rc = D.out.ensure_roomy((size_t)total + 64)) != PG_OK) return rc;
    if (total) {
        if (D.timing) HIPCHK(hipEventRecord(D.ev[2], st));
        hipLaunchKernelGGL(k_merge_emit, dim3((unsigned)((n_slots + 3) / 4)), dim3(256), 0, st, D.views.p, D.cfg, F, D.sep, D.missing.p, dense ? 1 : 0, hor_scaf,
                           from_pos, D.len.p, D.off.p, D.src.p, n_slots, D.out.p);
        HIPCHK(hipGetLastError());
        if (D.timing) HIPCHK(hipEventRecord(D.ev[3], st));
        if (D.bgzf) {
            HIPCHK(hipMemsetAsync(D.out.p + total, 0, 64, st));
            if ((rc = pg_deflate_queue(c, st, D.df, D.out.p, status + 2, total, nullptr, status + 4)) != PG_OK) return rc;
            HIPCHK(hipMemcpyAsync(D.h_status.p + 4, status + 4, sizeof(long long), hipMemcpyDeviceToHost, st));
        }
        HIPCHK(hipStreamSynchronize(st));
        if (D.bgzf) *bgzf_out = D.bgzf_bytes = D.h_status.p[4];
        if (D.timing) D.emit_ms += elapsed(D.ev[2], D.ev[3]);
    }
    if (D.timing) D.match_ms += elapsed(D.ev[0], D.ev[1]);
    for (int f = 0; f < nf; ++f) {
        MFile &M = D.f[f];
        const long long *fs = D.h_fstat.p + f * PGM_FSTAT;
        done[4 * f] = fs[4];
        done[4 * f + 1] = fs[4] > 0 ? fs[5] - M.base_byte : 0;
        done[4 * f + 2] = fs[2];
        done[4 * f + 3] = fs[3];
        if (fs[4] > 0) {
            M.base_line += fs[4];
            M.base_byte = fs[5];
        }
    }
    ++D.rounds;
    return PG_OK;
}

extern "C" int pg_merge_dev_rows(pg_ctx *c, int bgzf, uint8_t *dst, int64_t len) {
    int rc = check(c, "pg_merge_dev_rows");
    if (rc != PG_OK) return rc;
    MergeDev &D = *state(c);
    const int64_t have = bgzf ? D.bgzf_bytes : D.out_bytes;
    if (len < 0 || len != have || (len && !dst)) return pg_fail(PG_ERR_ARG, "pg_merge_dev_rows: the round left %lld bytes, %lld are asked for", (long long)have, (long long)len);
    if (len == 0) return PG_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, bgzf ? D.df.comp.p : D.out.p, (size_t)len, hipMemcpyDeviceToHost, c->stream_up));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    return PG_OK;
}

extern "C" int pg_merge_dev_advance(pg_ctx *c, const int64_t *done, const int32_t *prev_scaf, const int64_t *prev_pos) {
    int rc = check(c, "pg_merge_dev_advance");
    if (rc != PG_OK) return rc;
    MergeDev &D = *state(c);
    if (!done || !prev_scaf || !prev_pos) return pg_fail(PG_ERR_ARG, "pg_merge_dev_advance: null argument");
    HIPCHK(hipSetDevice(c->device));
    const int nf = D.cfg.n_files;
    for (int f = 0; f < nf; ++f) {
        MFile &M = D.f[f];
        if (done[2 * f] < 0 || done[2 * f + 1] < 0 || M.base_byte + done[2 * f + 1] > M.len)
            return pg_fail(PG_ERR_ARG, "pg_merge_dev_advance: file %d does not hold that many bytes", f);
        M.base_line = std::min(M.base_line + done[2 * f], M.n_lines);
        M.base_byte += done[2 * f + 1];
        M.keyed = M.base_line;                                     // the lines left are keyed again: their flags start over
        M.n_ok = M.base_line;
        long long *fs = D.h_fstat.p + f * PGM_FSTAT;
        fs[0] = fs[1] = PGM_NONE;
        fs[2] = prev_scaf[f];
        fs[3] = prev_pos[f];
        fs[4] = fs[5] = fs[6] = fs[7] = 0;
    }
    HIPCHK(hipMemcpyAsync(D.fstat.p, D.h_fstat.p, sizeof(long long) * PGM_FSTAT * (size_t)nf, hipMemcpyHostToDevice, c->stream_up));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    return PG_OK;
}

extern "C" int pg_merge_dev_text(pg_ctx *c, int f, uint8_t *dst, int64_t len) {
    int rc = check(c, "pg_merge_dev_text");
    if (rc != PG_OK) return rc;
    MergeDev &D = *state(c);
    if (f < 0 || f >= D.cfg.n_files) return pg_fail(PG_ERR_ARG, "pg_merge_dev_text: bad file");
    MFile &M = D.f[f];
    if (len != M.len - M.base_byte || (len && !dst)) return pg_fail(PG_ERR_ARG, "pg_merge_dev_text: file %d holds %lld bytes", f, (long long)(M.len - M.base_byte));
    if (len == 0) return PG_OK;
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipMemcpyAsync(dst, M.text[M.cur].p + M.base_byte, (size_t)len, hipMemcpyDeviceToHost, c->stream_up));
    HIPCHK(hipStreamSynchronize(c->stream_up));
    return PG_OK;
}

extern "C" int pg_merge_dev_timing(pg_ctx *c, int on) {
    int rc = check(c, "pg_merge_dev_timing");
    if (rc != PG_OK) return rc;
    state(c)->timing = on != 0;
    return PG_OK;
}

extern "C" int pg_merge_dev_stats(pg_ctx *c, int64_t *rounds_out, double *keys_ms_out, double *match_ms_out, double *emit_ms_out) {
    int rc = check(c, "pg_merge_dev_stats");
    if (rc != PG_OK) return rc;
    MergeDev &D = *state(c);
    if (rounds_out) *rounds_out = D.rounds;
    if (keys_ms_out) *keys_ms_out = D.keys_ms;
    if (match_ms_out) *match_ms_out = D.match_ms;
    if (emit_ms_out) *emit_ms_out = D.emit_ms;
    return PG_OK;
}
