// The block-slot protocol of pg_line_slot.h carried out: what pg_vcf_dev_*, pg_filter_dev_*, pg_gvcf_dev_*, pg_eig_dev_*, pg_ped_dev_*,
// pg_seq_dev_* and pg_s2g_dev_* do alike around their own kernels -- the slot's checks, submit, the two ends of parse, the status
// words' way to the device, the scan that places a block's rows (k_rows_scan), all of collect but the out-parameters, the copies back
// and the block counts.  The order of calls per stream is written out in that header.
#include "pg_ctx.h"

#include <algorithm>

namespace {

// the rows' places: exclusive sums of rlen over the lines (one block, every thread a stretch of lines), their total and number; RANK:
// every line's rank among the lines that have a row as well; a total beyond the output buffer raises PG_ST_OVERFLOW
template <bool RANK>
__global__ __launch_bounds__(1024) void k_rows_scan(const uint32_t *__restrict__ rlen, int64_t n_lines, int64_t *__restrict__ roff,
                                                     long long *__restrict__ status, int64_t out_cap, int64_t *__restrict__ rank) {
    __shared__ long long sh[1024], shn[1024];
    const int64_t per = (n_lines + 1023) / 1024;
    const int64_t a = std::min<int64_t>(n_lines, (int64_t)threadIdx.x * per), b = std::min<int64_t>(n_lines, a + per);
    long long mine = 0, rows = 0;
    for (int64_t k = a; k < b; ++k) {
        mine += rlen[k];
        rows += rlen[k] != 0;
    }
    sh[threadIdx.x] = mine;
    shn[threadIdx.x] = rows;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const long long x = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0, y = (int)threadIdx.x >= d ? shn[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += x;
        shn[threadIdx.x] += y;
        __syncthreads();
    }
    long long run = sh[threadIdx.x] - mine, r = shn[threadIdx.x] - rows;
    for (int64_t k = a; k < b; ++k) {
        roff[k] = run;
        if (RANK) rank[k] = r;
        run += rlen[k];
        r += rlen[k] != 0;
    }
    if (threadIdx.x == 1023) {
        status[PGL_ST_BYTES] = sh[1023];
        status[PGL_ST_ROWS] = shn[1023];
        if (sh[1023] > out_cap) atomicOr(reinterpret_cast<unsigned long long *>(status + PGL_ST_BITS), (unsigned long long)PG_ST_OVERFLOW);
    }
}

}  // namespace

void pg_rows_scan_queue(hipStream_t st, const uint32_t *rlen, int64_t n_lines, int64_t *roff, long long *status, int64_t out_cap, int64_t *rank) {
    if (rank) hipLaunchKernelGGL(k_rows_scan<true>, dim3(1), dim3(1024), 0, st, rlen, n_lines, roff, status, out_cap, rank);
    else hipLaunchKernelGGL(k_rows_scan<false>, dim3(1), dim3(1024), 0, st, rlen, n_lines, roff, status, out_cap, rank);
}

int pg_small_stream(pg_ctx *c) {
    if (!c->tok_small) HIPCHK(hipStreamCreateWithFlags(&c->tok_small, hipStreamNonBlocking));
    return PG_OK;
}

int pg_copy_back(pg_ctx *c, void *dst, const void *src, int64_t len) {
    HIPCHK(hipSetDevice(c->device));
    int rc = pg_small_stream(c);
    if (rc != PG_OK) return rc;
    HIPCHK(hipMemcpyAsync(dst, src, (size_t)len, hipMemcpyDeviceToHost, c->tok_small));
    HIPCHK(hipStreamSynchronize(c->tok_small));
    return PG_OK;
}

int pg_line_check_slot(pg_ctx *c, int slot, const PgLineRoute *D, const char *who, const char *config_name) {
    if (!c || slot < 0 || slot > 1) return pg_fail(PG_ERR_ARG, "%s: bad context or slot", who);
    if (!D->configured) return pg_fail(PG_ERR_STATE, "%s: %s must be called first", who, config_name);
    return PG_OK;
}

int pg_line_submit_text(pg_ctx *c, int slot, PgLineDev &S, const char *text, int fd, int64_t file_offset, int64_t len, bool last_is_newline) {
    int rc = pg_tok_text_submit(c, slot, text, fd, file_offset, len);
    if (rc == PG_OK) pgl_submit(S.L, len, true, last_is_newline);
    return rc;
}

int pg_line_submit_plain(pg_ctx *c, int slot, PgLineDev &S, const char *text, int64_t len, const char *who) {
    if ((!text && len) || len < 0) return pg_fail(PG_ERR_ARG, "%s: no text", who);
    return pg_line_submit_text(c, slot, S, text, -1, 0, len, len > 0 && text[len - 1] == '\n');
}

int pg_line_submit_bgzf(pg_ctx *c, int slot, PgLineDev &S, const uint8_t *comp, int64_t comp_len, const uint32_t *in_off,
                        const uint32_t *in_len, const uint32_t *out_len, const uint32_t *crc, int64_t n_members, const char *head,
                        int64_t head_len, int64_t text_len, int64_t line_len_hint, bool last_known, bool last_is_newline) {
    int rc = pg_tok_bgzf_submit(c, slot, comp, comp_len, in_off, in_len, out_len, crc, n_members, head, head_len, text_len, line_len_hint);
    if (rc == PG_OK) pgl_submit(S.L, text_len, last_known, last_is_newline);
    return rc;
}

int pg_line_parse_begin(pg_ctx *c, int slot, PgLineDev &S, int64_t *n_lines_out, bool *nothing_out, const char *who) {
    *n_lines_out = 0;
    *nothing_out = true;
    const PgLineGate gate = pgl_parse_gate(S.L);
    if (gate == PGL_NOTHING) return PG_OK;
    if (gate != PGL_GO) return pg_fail(PG_ERR_STATE, "%s: nothing submitted to slot %d", who, slot);
    HIPCHK(hipSetDevice(c->device));
    hipStream_t st = c->stream_up;
    int64_t n_lines = 0;
    int rc = pg_tok_lines(c, slot, &n_lines);
    if (rc != PG_OK) { S.L.state = PGL_IDLE; return rc; }
    S.L.n_lines = *n_lines_out = n_lines;
    if ((rc = S.status.ensure(PGL_STATUS_WORDS)) != PG_OK || (rc = S.h_status.ensure(PGL_STATUS_WORDS)) != PG_OK) return rc;
    if (!S.done) HIPCHK(hipEventCreateWithFlags(&S.done, hipEventDisableTiming));
    if (S.L.tail_unknown && n_lines > 0) {                        // does the inflated text end in a line feed (the file's last block may not)?
        int64_t last = -1;
        HIPCHK(hipMemcpyAsync(&last, c->tok[slot].nl.p + n_lines - 1, 8, hipMemcpyDeviceToHost, st));
        HIPCHK(hipStreamSynchronize(st));
        pgl_tail_read(S.L, last);
    }
    *nothing_out = pgl_host_now(n_lines, S.L.no_final_newline);
    pgl_preset(S.h_status.p, *nothing_out);
    if (*nothing_out) {                                           // nothing to queue: collect reports the block as the host's
        S.L.state = PGL_QUEUED;
        HIPCHK(hipEventRecord(S.done, st));
    }
    return PG_OK;
}

int pg_line_status_upload(PgLineDev &S, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(S.status.p, S.h_status.p, PGL_STATUS_WORDS * 8, hipMemcpyHostToDevice, st));
    return PG_OK;
}

int pg_line_parse_end(pg_ctx *c, PgLineDev &S, hipStream_t st) {
    HIPCHK(hipMemcpyAsync(S.h_status.p, S.status.p, PGL_STATUS_WORDS * 8, hipMemcpyDeviceToHost, st));
    HIPCHK(hipEventRecord(S.done, st));
    S.L.state = PGL_QUEUED;
    return PG_OK;
}

int pg_line_collect_wait(pg_ctx *c, int slot, PgLineDev &S, const char *who) {
    const PgLineGate gate = pgl_collect_gate(S.L);
    if (gate == PGL_NOTHING) { S.L.state = PGL_IDLE; return PG_OK; }
    if (gate != PGL_GO) return pg_fail(PG_ERR_STATE, "%s: nothing parsed in slot %d", who, slot);
    HIPCHK(hipSetDevice(c->device));
    HIPCHK(hipEventSynchronize(S.done));
    S.L.state = PGL_IDLE;
    return pg_tok_crc_result(c, slot);
}

int pg_line_collect(pg_ctx *c, int slot, PgLineRoute &D, PgLineDev &S, bool bgzf_rows, PgLineAgain again, int64_t *n_lines_out,
                    PgLineResult *R, const char *who) {
    *R = PgLineResult{-1, 0, 0, 0, false};
    if (n_lines_out) *n_lines_out = 0;
    const bool empty = S.L.state == PGL_EMPTY;
    int rc = pg_line_collect_wait(c, slot, S, who);
    if (rc != PG_OK || empty) return rc;
    if (n_lines_out) *n_lines_out = S.L.n_lines;
    if (again && pgl_render_again(S.h_status.p)) {
        hipStream_t st = c->stream_up;
        pgl_preset_again(S.h_status.p, bgzf_rows);
        if ((rc = pg_line_status_upload(S, st)) != PG_OK || (rc = again(c, slot, S.h_status.p[PGL_ST_BYTES], st)) != PG_OK) return rc;
        HIPCHK(hipEventSynchronize(S.done));
        S.L.state = PGL_IDLE;
    }
    *R = pgl_decode(S.h_status.p, bgzf_rows);
    if (R->host_block) ++D.host_blocks;
    return PG_OK;
}

int pg_line_text(pg_ctx *c, int slot, int64_t off, int64_t len, uint8_t *dst, const char *bad) {
    pg_ctx::TokSlot &T = c->tok[slot];
    if (!pgl_range_ok(off, len, T.len, dst != nullptr, T.tp != nullptr)) return pg_fail(PG_ERR_ARG, "%s", bad);
    return len ? pg_copy_back(c, dst, T.tp + off, len) : PG_OK;
}

int pg_line_rows(pg_ctx *c, const DevBuf<uint8_t> &B, uint8_t *dst, int64_t len, const char *bad) {
    if (!pgl_rows_ok(len, B.cap, dst != nullptr)) return pg_fail(PG_ERR_ARG, "%s", bad);
    return len ? pg_copy_back(c, dst, B.p, len) : PG_OK;
}

int pg_line_stats(const PgLineRoute *D, int64_t *blocks_out, int64_t *host_blocks_out, const char *who) {
    if (!D || !blocks_out || !host_blocks_out) return pg_fail(PG_ERR_ARG, "%s: null argument", who);
    *blocks_out = D->blocks;
    *host_blocks_out = D->host_blocks;
    return PG_OK;
}
