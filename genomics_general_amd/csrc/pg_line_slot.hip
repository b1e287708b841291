// The block-slot protocol of pg_line_slot.h carried out: what pg_vcf_dev_*, pg_filter_dev_* and pg_seq_dev_* do alike around their own
// kernels.  The order of calls per stream is written out in that header.
#include "pg_ctx.h"

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

int pg_line_check_slot(pg_ctx *c, int slot, bool configured, const char *who, const char *config_name) {
    if (!c || slot < 0 || slot > 1) return pg_fail(PG_ERR_ARG, "%s: bad context or slot", who);
    if (!configured) return pg_fail(PG_ERR_STATE, "%s: %s must be called first", who, config_name);
    return PG_OK;
}

int pg_line_submit_text(pg_ctx *c, int slot, PgLineDev &S, const char *text, int fd, int64_t file_offset, int64_t len, bool last_is_newline) {
    int rc = pg_tok_text_submit(c, slot, text, fd, file_offset, len);
    if (rc == PG_OK) pgl_submit(S.L, len, true, last_is_newline);
    return rc;
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
