// csrc/pg_line_slot.h walked as a program of its own (no GPU, no library): every state of a PgLineSlot against every event, the
// decision that a block is the host's before any kernel runs, the status words a block starts from, and what collect makes of the
// words that come back, whether the rows are rendered a second time and from which words, and the range checks of the copies back.
// The expected values are written out here as the seven routes' pg_*_dev_* entry points gave them before the protocol was lifted
// out of their files: states 0 idle, 1 submitted, 2 queued, 3 empty; status bit 1 a line needs the host, bit 2 the rows exceed their
// buffer.  Prints "N checks, 0 bad"; exit status 1 when a check fails.
#include "../genomics_general_amd/csrc/pg_line_slot.h"

#include <cstdio>

static int n_checks = 0, n_bad = 0;

static void check(bool ok, const char *what, int a = 0, int b = 0) {
    ++n_checks;
    if (!ok) {
        ++n_bad;
        fprintf(stderr, "line_slot_main: %s (%d, %d)\n", what, a, b);
    }
}

// the events as the entry points apply them: 'gate' results 0 go on, 1 return PG_OK at once, 2 PG_ERR_STATE
static int parse(PgLineSlot &L, int64_t n_lines, int64_t last_nl) {
    const PgLineGate g = pgl_parse_gate(L);
    if (g != PGL_GO) return (int)g;
    L.n_lines = n_lines;
    if (L.tail_unknown && n_lines > 0) pgl_tail_read(L, last_nl);
    L.state = PGL_QUEUED;                                         // (host now or kernels queued: queued either way)
    return 0;
}
static int collect(PgLineSlot &L) {
    const PgLineGate g = pgl_collect_gate(L);
    if (g == PGL_NOTHING || g == PGL_GO) L.state = PGL_IDLE;
    return (int)g;
}

int main() {
    static_assert(PGL_IDLE == 0 && PGL_SUBMITTED == 1 && PGL_QUEUED == 2 && PGL_EMPTY == 3, "the states' numbers");
    static_assert(PGL_ST_BITS == 0 && PGL_ST_HOST_LINE == 1 && PGL_ST_BYTES == 2 && PGL_ST_ROWS == 3 && PGL_ST_BGZF_BYTES == 4 &&
                      PGL_STATUS_WORDS == 5 && PGL_STATUS_WORDS * 8 == 40, "the status words' places");
    static_assert(PG_ST_HOST == 1 && PG_ST_OVERFLOW == 2, "the status bits");

    // ---- state x event: the state after, and what the call answers (0 goes on / done, 1 PG_OK at once, 2 PG_ERR_STATE) ----
    //                                  event:  submit 0      submit 7      parse         collect
    static const int after[4][4] = {/* idle      */ {3, 1, 0, 0},
                                    /* submitted */ {3, 1, 2, 1},
                                    /* queued    */ {3, 1, 2, 0},
                                    /* empty     */ {3, 1, 3, 0}};
    static const int answer[4][4] = {/* idle      */ {0, 0, 2, 2},
                                     /* submitted */ {0, 0, 0, 2},
                                     /* queued    */ {0, 0, 2, 0},
                                     /* empty     */ {0, 0, 1, 1}};
    for (int s = 0; s < 4; ++s)
        for (int e = 0; e < 4; ++e) {
            PgLineSlot L;
            L.state = s;
            L.text_len = 100;
            int got = 0;
            if (e == 0) pgl_submit(L, 0, true, false);
            else if (e == 1) pgl_submit(L, 7, true, true);
            else if (e == 2) got = parse(L, 3, 99);
            else got = collect(L);
            check(L.state == after[s][e], "state after an event", s, e);
            check(got == answer[s][e], "answer to an event", s, e);
        }
    // the sequences named in the protocol: a block through all three calls; collect twice; parse without submit; an empty block
    {
        PgLineSlot L;
        check(parse(L, 1, 0) == 2 && L.state == 0, "parse without submit");
        pgl_submit(L, 12, true, true);
        check(L.state == 1 && L.text_len == 12 && !L.no_final_newline && !L.tail_unknown, "submit of 12 bytes");
        check(parse(L, 2, 11) == 0 && L.state == 2 && L.n_lines == 2, "parse");
        check(parse(L, 2, 11) == 2 && L.state == 2, "parse twice");
        check(collect(L) == 0 && L.state == 0, "collect");
        check(collect(L) == 2 && L.state == 0, "collect twice");
        pgl_submit(L, 0, true, false);
        check(L.state == 3 && L.text_len == 0 && !L.no_final_newline && !L.tail_unknown, "submit of no bytes");
        check(parse(L, 0, 0) == 1 && L.state == 3, "parse of an empty block");
        check(collect(L) == 1 && L.state == 0, "collect of an empty block");
        check(collect(L) == 2 && L.state == 0, "collect of an empty block twice");
        pgl_submit(L, 0, false, false);
        check(L.state == 3 && !L.no_final_newline && !L.tail_unknown, "submit of no bytes, the tail unknown");
    }
    // the last byte: known and a line feed, known and none, unknown (read once the line feeds are counted)
    {
        PgLineSlot L;
        pgl_submit(L, 12, true, false);
        check(L.state == 1 && L.no_final_newline && !L.tail_unknown, "no final line feed, known at submit");
        pgl_submit(L, 12, false, false);
        check(L.state == 1 && !L.no_final_newline && L.tail_unknown, "the tail unknown at submit");
        check(parse(L, 2, 11) == 0 && !L.no_final_newline, "the last line feed is the last byte");
        pgl_submit(L, 12, false, true);                          // (last_is_newline means nothing when the byte is not known)
        check(L.tail_unknown && !L.no_final_newline, "the tail unknown, whatever the other flag");
        check(parse(L, 2, 8) == 0 && L.no_final_newline, "the last line feed is not the last byte");
        pgl_submit(L, 12, false, false);
        check(parse(L, 0, -1) == 0 && !L.no_final_newline, "no line feed at all: nothing read back");
        pgl_submit(L, 12, true, true);
        check(!L.tail_unknown && !L.no_final_newline, "a later submit clears both");
    }

    // ---- host_now and the preset, n_lines in {0, 1} x no_final_newline in {0, 1} ----
    static const bool want_host[2][2] = {{true, true}, {false, true}};     // [n_lines][no_final_newline]
    for (int n = 0; n < 2; ++n)
        for (int f = 0; f < 2; ++f) {
            const bool h = pgl_host_now(n, f != 0);
            check(h == want_host[n][f], "host_now", n, f);
            int64_t st[6] = {-5, -5, -5, -5, -5, -5};
            pgl_preset(st, h);
            const int64_t w0 = want_host[n][f] ? 1 : 0, w1 = want_host[n][f] ? 0 : 0x7fffffffffffffffll;
            check(st[0] == w0 && st[1] == w1 && st[2] == 0 && st[3] == 0 && st[4] == 0 && st[5] == -5, "the preset", n, f);
        }
    check(pgl_host_now(1000000, false) == false && pgl_host_now(1000000, true) == true, "host_now of a large block");

    // ---- the collect decode: status words {bits, first host line, bytes, rows, BGZF bytes}, bgzf_rows off and on ----
    struct Case {
        int64_t st[5];
        int bgzf_rows;
        int64_t host_line, bytes, rows, bgzf_bytes;
        bool host_block;
    };
    static const Case cases[] = {
        // neither bit: the rows are ready
        {{0, 0x7fffffffffffffffll, 300, 7, 90}, 0, -1, 300, 7, 0, false},
        {{0, 0x7fffffffffffffffll, 300, 7, 90}, 1, -1, 300, 7, 90, false},
        {{0, 0x7fffffffffffffffll, 0, 0, 0}, 1, -1, 0, 0, 0, false},
        // the host bit alone: the first such line, nothing else
        {{1, 5, 300, 7, 90}, 0, 5, 0, 0, 0, true},
        {{1, 5, 300, 7, 90}, 1, 5, 0, 0, 0, true},
        {{1, 0, 0, 0, 0}, 0, 0, 0, 0, 0, true},                  // (the preset of a block that is the host's as it stands)
        // the overflow bit alone: line 0
        {{2, 0x7fffffffffffffffll, 300, 7, 0}, 0, 0, 0, 0, 0, true},
        {{2, 0x7fffffffffffffffll, 300, 7, 0}, 1, 0, 0, 0, 0, true},
        // both bits: the host bit's line
        {{3, 9, 300, 7, 0}, 0, 9, 0, 0, 0, true},
        {{3, 9, 300, 7, 0}, 1, 9, 0, 0, 0, true},
    };
    for (size_t k = 0; k < sizeof(cases) / sizeof(cases[0]); ++k) {
        const Case &c = cases[k];
        const PgLineResult r = pgl_decode(c.st, c.bgzf_rows != 0);
        check(r.host_line == c.host_line && r.bytes == c.bytes && r.rows == c.rows && r.bgzf_bytes == c.bgzf_bytes && r.host_block == c.host_block,
              "the collect decode", (int)k, c.bgzf_rows);
    }

    // ---- the second render (pg_filter_dev_collect, pg_gvcf_dev_collect, pg_eig_dev_collect, pg_ped_dev_collect before they shared it):
    // only when the overflow bit stands alone; it starts from the same words with the bits cleared -- and, in the two routes that
    // deflate their rows, the members' bytes
    static const bool want_again[4] = {false, false, true, false};         // bits 0, HOST, OVERFLOW, HOST | OVERFLOW
    for (int bits = 0; bits < 4; ++bits) {
        const int64_t st[5] = {bits, 4, 300, 7, 90};
        check(pgl_render_again(st) == want_again[bits], "render again", bits);
    }
    for (int bgzf = 0; bgzf < 2; ++bgzf) {
        int64_t st[6] = {2, 0x7fffffffffffffffll, 300, 7, 90, -5};
        pgl_preset_again(st, bgzf != 0);
        check(st[0] == 0 && st[1] == 0x7fffffffffffffffll && st[2] == 300 && st[3] == 7 && st[4] == (bgzf ? 0 : 90) && st[5] == -5,
              "the second render's preset", bgzf);
        check(!pgl_render_again(st) && pgl_decode(st, bgzf != 0).bytes == 300 && pgl_decode(st, bgzf != 0).rows == 7, "... read by collect", bgzf);
    }

    // ---- the copies back.  pg_*_dev_text: bytes [off, off + len) of a text of `have` bytes (the routes that take no offset: off = 0) ----
    {
        const int64_t have = 10;
        static const int64_t v[5] = {0, 1, have - 1, have, have + 1};
        static const bool want_in[5][5] = {/* off 0        */ {true, true, true, true, false},       // len 0, 1, have - 1, have, have + 1
                                           /* off 1        */ {true, true, true, false, false},
                                           /* off have - 1 */ {true, true, false, false, false},
                                           /* off have     */ {true, false, false, false, false},
                                           /* off have + 1 */ {false, false, false, false, false}};
        for (int a = 0; a < 5; ++a)
            for (int b = 0; b < 5; ++b) check(pgl_range_ok(v[a], v[b], have, true, true) == want_in[a][b], "a text range", a, b);
        check(!pgl_range_ok(-1, 1, have, true, true) && !pgl_range_ok(-1, 0, have, true, true), "a negative offset");
        check(!pgl_range_ok(0, -1, have, true, true) && !pgl_range_ok(have, -1, have, true, true), "a negative length");
        check(pgl_range_ok(0, 0, have, false, true) && pgl_range_ok(have, 0, have, false, true), "no destination, nothing to copy");
        check(!pgl_range_ok(0, 1, have, false, true) && !pgl_range_ok(0, have, have, false, true), "no destination");
        check(!pgl_range_ok(0, 1, have, true, false) && !pgl_range_ok(0, 1, 0, true, false), "no text in the slot");
        check(pgl_range_ok(0, 0, 0, true, false) && pgl_range_ok(0, 0, 0, false, false), "no text in the slot, nothing to copy");
        check(pgl_range_ok(0, 0, 0, true, true) && !pgl_range_ok(0, 1, 0, true, true), "a text of no bytes");
    }
    // pg_*_dev_rows / _rows_bgzf: the first len bytes of a buffer of `cap` bytes
    {
        const uint64_t cap = 4096;
        check(pgl_rows_ok(0, cap, true) && pgl_rows_ok(1, cap, true) && pgl_rows_ok((int64_t)cap, cap, true), "rows inside their buffer");
        check(!pgl_rows_ok((int64_t)cap + 1, cap, true), "rows beyond their buffer");
        check(!pgl_rows_ok(-1, cap, true), "a negative number of row bytes");
        check(pgl_rows_ok(0, cap, false) && !pgl_rows_ok(1, cap, false), "rows without a destination");
        check(pgl_rows_ok(0, 0, true) && !pgl_rows_ok(1, 0, true), "a buffer never made");
    }
    printf("%d checks, %d bad\n", n_checks, n_bad);
    return n_bad ? 1 : 0;
}
