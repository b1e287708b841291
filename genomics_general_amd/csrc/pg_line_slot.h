// The block slot of the seven per-line device routes (parseVCF: pg_vcf_dev.hip, filterGenotypes: pg_filter_dev.hip, genoToVCF:
// pg_gvcf_dev.hip, genoToEigenstrat: pg_eig_dev.hip, genoToPlink: pg_ped_dev.hip, genoToSeq: pg_seq_dev.hip, seqToGeno: pg_s2g_dev.hip),
// decided apart from its launches: a block of whole lines goes through one of the tokenizer's two text slots in three calls -- submit,
// parse, collect -- and reports through five status words.  Here: the slot's states and gates, the status words a block starts from and
// what collect makes of them, whether the rows are rendered a second time and from which words, and the argument checks of the copies
// back.  Plain C++17 with no HIP header, so that a CPU program can walk every state and decision (tests/line_slot_main.cpp); the
// pg_line_* helpers (pg_line_slot.hip) carry them out, the route files keep their kernels.
//
// The status words (int64, on the device and in page-locked host memory; the kernels raise them, collect reads them):
//   [PGL_ST_BITS]        PG_ST_HOST: some line needs the host route; PG_ST_OVERFLOW: the rows exceed the output buffer
//   [PGL_ST_HOST_LINE]   the first line that needs the host route (an atomic minimum: preset to the largest int64)
//   [PGL_ST_BYTES]       bytes of the rows            [PGL_ST_ROWS]  rows (genoToSeq: sites)
//   [PGL_ST_BGZF_BYTES]  bytes of the rows as BGZF members (the routes that deflate their rows on the device)
//
// The order of calls per block (st: the context's copy stream, where every route's kernels run; S: the route's slot):
//   submit   pg_line_submit_text / _plain / _bgzf: pg_tok_text_submit / pg_tok_bgzf_submit (the text to the device, or its members
//            inflated there; line feeds counted behind it), then pgl_submit
//   parse    pg_line_parse_begin: pgl_parse_gate; pg_tok_lines (waits for the count, queues the line-feed positions on st); only with
//            tail_unknown, the last line feed's position copied back and st waited for; pgl_preset into the host words; a block that is
//            the host's as it stands: S.done recorded on st, queued, nothing else
//            the route: its buffers sized, pg_line_status_upload (the host words to the device on st), its kernels on st -- the rows'
//            places by pg_rows_scan_queue (k_rows_scan)
//            pg_line_parse_end: the device words copied back, S.done recorded (on st, or the stream the route's last kernel ran on), queued
//   collect  pg_line_collect: whether the block is empty read first; pg_line_collect_wait (pgl_collect_gate; S.done waited for; idle;
//            pg_tok_crc_result); only where pgl_render_again: pgl_preset_again into the host words, pg_line_status_upload, the route's
//            second render (its buffer grown for the rows' bytes, its render kernels on st, pg_line_parse_end), S.done waited for a
//            second time, idle; pgl_decode of the host words, a host block counted
//            the route: the result into its out-parameters, its rows copied back on the small stream (pg_line_rows, pg_line_text:
//            pg_copy_back)
#pragma once

#include <cstdint>

#define PG_ST_HOST 1ll      // some line of the block goes through the host route
#define PG_ST_OVERFLOW 2ll  // the rows did not fit the output buffer: grow it, render again

enum { PGL_ST_BITS = 0, PGL_ST_HOST_LINE = 1, PGL_ST_BYTES = 2, PGL_ST_ROWS = 3, PGL_ST_BGZF_BYTES = 4, PGL_STATUS_WORDS = 5 };

enum PgLineState { PGL_IDLE = 0, PGL_SUBMITTED = 1, PGL_QUEUED = 2, PGL_EMPTY = 3 };   // EMPTY: a block of no bytes, nothing on the device

struct PgLineSlot {
    int state = PGL_IDLE;
    int64_t text_len = 0, n_lines = 0;
    bool no_final_newline = false;   // the text does not end in a line feed (the file's partial last line): the block is the host's
    bool tail_unknown = false;       // ... which parse has yet to read on the device, once the line feeds are counted
};

// a block of len bytes has reached the tokenizer's slot.  last_known: the caller has seen the block's last byte (a bgzipped block whose
// caller has not: tail_unknown)
inline void pgl_submit(PgLineSlot &L, int64_t len, bool last_known, bool last_is_newline) {
    L.text_len = len;
    L.n_lines = 0;
    L.no_final_newline = len > 0 && last_known && !last_is_newline;
    L.tail_unknown = len > 0 && !last_known;
    L.state = len ? PGL_SUBMITTED : PGL_EMPTY;
}

enum PgLineGate { PGL_GO = 0, PGL_NOTHING = 1, PGL_WRONG_STATE = 2 };   // NOTHING: an empty block, the call returns PG_OK at once

inline PgLineGate pgl_parse_gate(const PgLineSlot &L) {
    return L.state == PGL_EMPTY ? PGL_NOTHING : L.state == PGL_SUBMITTED ? PGL_GO : PGL_WRONG_STATE;
}
inline PgLineGate pgl_collect_gate(const PgLineSlot &L) {
    return L.state == PGL_EMPTY ? PGL_NOTHING : L.state == PGL_QUEUED ? PGL_GO : PGL_WRONG_STATE;
}

// tail_unknown: last_nl is where the last of the counted line feeds stands
inline void pgl_tail_read(PgLineSlot &L, int64_t last_nl) { L.no_final_newline = last_nl != L.text_len - 1; }

// the block is the host's before any kernel has seen it: no final line feed, or no line feed at all (one unfinished line)
inline bool pgl_host_now(int64_t n_lines, bool no_final_newline) { return no_final_newline || n_lines == 0; }

// the status words a block starts from
inline void pgl_preset(int64_t *status, bool host_now) {
    status[PGL_ST_BITS] = host_now ? PG_ST_HOST : 0;
    status[PGL_ST_HOST_LINE] = host_now ? 0 : 0x7fffffffffffffffll;
    status[PGL_ST_BYTES] = status[PGL_ST_ROWS] = status[PGL_ST_BGZF_BYTES] = 0;
}

// what collect reports.  host_line < 0: the rows are ready; else the block goes to the host route (it counts as a host block) and
// host_line is the first line the device does not take -- 0 when only the rows' room gave out
struct PgLineResult {
    int64_t host_line, bytes, rows, bgzf_bytes;
    bool host_block;
};

inline PgLineResult pgl_decode(const int64_t *status, bool bgzf_rows) {
    if (status[PGL_ST_BITS]) return {(status[PGL_ST_BITS] & PG_ST_HOST) ? status[PGL_ST_HOST_LINE] : 0, 0, 0, 0, true};
    return {-1, status[PGL_ST_BYTES], status[PGL_ST_ROWS], bgzf_rows ? status[PGL_ST_BGZF_BYTES] : 0, false};
}

// collect: the rows' room alone gave out -- no line needs the host, so the route grows its buffer and renders a second time
inline bool pgl_render_again(const int64_t *status) { return status[PGL_ST_BITS] == PG_ST_OVERFLOW; }

// the status words the second render starts from: the scan's bytes and rows stay; the members' bytes go where the render is deflated again
inline void pgl_preset_again(int64_t *status, bool bgzf_rows) {
    status[PGL_ST_BITS] = 0;
    if (bgzf_rows) status[PGL_ST_BGZF_BYTES] = 0;
}

// a copy back of bytes [off, off + len) of `have`: the range lies inside, and where len > 0 there is a source and a destination
inline bool pgl_range_ok(int64_t off, int64_t len, int64_t have, bool has_dst, bool has_src) {
    return off >= 0 && len >= 0 && off + len <= have && (len == 0 || (has_dst && has_src));
}
// ... of the first len bytes of a row buffer of `cap` bytes
inline bool pgl_rows_ok(int64_t len, uint64_t cap, bool has_dst) { return len >= 0 && (uint64_t)len <= cap && (len == 0 || has_dst); }
