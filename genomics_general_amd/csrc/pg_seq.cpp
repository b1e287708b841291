// The host route of the genoToSeq.py drop-in (pg_seq_text): every spelling the reference's `line.split()` takes, the blocks the device
// route hands back, and PG_SEQ_DEVICE=0.  Lines end at \n (the driver has turned \r\n and a lone \r into \n, as the reference's
// text-mode file does), fields are cut at runs of ASCII whitespace, a line whose first byte is '#' is skipped.  Two passes with the
// functions of pg_seq_core.h: the first checks every line and sizes the sequences, the second copies the characters.  No GPU context is
// needed, and nothing but the C library: tests/seq_host_main.cpp compiles this file on its own.
#include "pg_seq_core.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <vector>

namespace {

struct Span {
    int64_t s, e;
};

// the line's fields (at most `cap` + 1 of them are looked at); false: a byte that is not ASCII
bool split_line(const uint8_t *line, int64_t n, size_t cap, std::vector<Span> &f) {
    f.clear();
    for (int64_t k = 0; k < n; ++k)
        if (line[k] >= 0x80) return false;
    int64_t at = 0, fs, fe;
    while (f.size() <= cap && pgs_next_field(line, n, &at, &fs, &fe)) f.push_back(Span{fs, fe});
    return true;
}

template <class T>
T *grab(size_t n) {
    return static_cast<T *>(malloc((n ? n : 1) * sizeof(T)));
}

}  // namespace

extern "C" void pg_seq_free(pg_seq_block *b) {
    if (!b) return;
    free(b->seq);
    free(b->off);
    free(b->pos);
    free(b->run_start);
    free(b->run_name);
    b->seq = nullptr;
    b->off = b->pos = b->run_start = b->run_name = nullptr;
}

extern "C" int pg_seq_text(const pg_seq_cfg *cfg, const int32_t *sel_col, const int32_t *sel_off, const int32_t *sel_len, const char *text_c,
                           int64_t len, pg_seq_block *out) {
    if (!cfg || !out || len < 0 || (len && !text_c) || cfg->n_seq < 0 || cfg->n_cols < 2 || (cfg->n_seq && (!sel_col || !sel_off || !sel_len)))
        return PG_ERR_ARG;
    for (int q = 0; q < cfg->n_seq; ++q)
        if (sel_col[q] < 2 || sel_col[q] >= cfg->n_cols || sel_off[q] < 0 || sel_len[q] < 0 || (sel_len[q] ? sel_off[q] >= sel_len[q] : sel_off[q] != 0))
            return PG_ERR_ARG;
    memset(out, 0, sizeof(*out));
    out->err_line = -1;
    const uint8_t *text = reinterpret_cast<const uint8_t *>(text_c);
    const size_t nq = (size_t)cfg->n_seq, n_cols = (size_t)cfg->n_cols;

    // pass 1: the lines, their errors, positions and runs; what every sequence gets
    std::vector<Span> lines, fields;                 // the kept lines
    std::vector<int64_t> pos, run_start, run_name, tot(nq, 0);
    int64_t stride = -1;                             // the one width of every (line, sequence) so far; -2: they differ
    int64_t prev_s = -1, prev_n = 0;                 // the scaffold of the kept line before
    int64_t li = 0;
    for (int64_t a = 0; a < len; ++li) {
        const void *z = memchr(text + a, '\n', (size_t)(len - a));
        const int64_t e = z ? static_cast<const uint8_t *>(z) - text : len;
        const uint8_t *line = text + a;
        const int64_t n = e - a;
        const int64_t next = e + 1;
        if (n > 0 && line[0] == '#') { a = next; continue; }
        int err = 0;
        if (!split_line(line, n, n_cols, fields)) err = PGS_E_ASCII;
        else if (fields.size() < n_cols) err = PGS_E_COLS;
        else if (fields.size() > n_cols && cfg->exact_cols) err = PGS_E_MORE;
        int64_t p = 0;
        if (!err && pgs_parse_pos(line + fields[1].s, fields[1].e - fields[1].s, &p)) err = PGS_E_POS;
        if (!err)
            for (size_t q = 0; q < nq; ++q) {
                const Span c = fields[(size_t)sel_col[q]];
                const int w = pgs_cell_width(c.e - c.s, sel_len[q]);
                if (sel_len[q] && !w) { err = PGS_E_CELL; break; }
                tot[q] += w;
                if (stride == -1) stride = w;
                else if (stride != w) stride = -2;
            }
        if (err) {
            // the sums of the line are taken back: the block ends in front of it
            out->err_line = li;
            out->err_code = err;
            if (err == PGS_E_CELL || stride == -2) {
                std::fill(tot.begin(), tot.end(), 0);
                stride = -2;                         // (recounted below from the kept lines)
            }
            break;
        }
        const int64_t fn = fields[0].e - fields[0].s;
        if (prev_s < 0 || fn != prev_n || memcmp(text + prev_s, line + fields[0].s, (size_t)fn) != 0) {
            run_start.push_back((int64_t)lines.size());
            run_name.push_back(a + fields[0].s);
            run_name.push_back(fn);
        }
        prev_s = a + fields[0].s;
        prev_n = fn;
        lines.push_back(Span{a, e});
        pos.push_back(p);
        a = next;
    }
    const size_t n_sites = lines.size();
    if (out->err_line >= 0 && stride == -2) {        // the totals of the lines in front of the error
        for (size_t i = 0; i < n_sites; ++i) {
            split_line(text + lines[i].s, lines[i].e - lines[i].s, n_cols, fields);
            for (size_t q = 0; q < nq; ++q) {
                const Span c = fields[(size_t)sel_col[q]];
                tot[q] += pgs_cell_width(c.e - c.s, sel_len[q]);
            }
        }
    }
    if (stride < 0) stride = n_sites ? 0 : 1;        // widths differ: offsets; no site at all: a stride of one
    if (out->err_line >= 0 && stride > 0)
        for (size_t q = 0; q < nq; ++q) tot[q] = (int64_t)n_sites * stride;

    // pass 2: the characters
    int64_t total = 0;
    std::vector<int64_t> base(nq + 1, 0);
    for (size_t q = 0; q < nq; ++q) {
        base[q] = total;
        total += tot[q];
    }
    base[nq] = total;
    out->n_sites = (int64_t)n_sites;
    out->n_runs = (int64_t)run_start.size();
    out->stride = stride;
    out->seq_bytes = total;
    out->seq = grab<uint8_t>((size_t)total);
    out->off = stride ? nullptr : grab<int64_t>(nq * (n_sites + 1));
    out->pos = grab<int64_t>(n_sites);
    out->run_start = grab<int64_t>(run_start.size());
    out->run_name = grab<int64_t>(run_name.size());
    if (!out->seq || (!stride && !out->off) || !out->pos || !out->run_start || !out->run_name) {
        pg_seq_free(out);
        return PG_ERR_ARG;
    }
    if (n_sites) memcpy(out->pos, pos.data(), n_sites * 8);
    if (!run_start.empty()) {
        memcpy(out->run_start, run_start.data(), run_start.size() * 8);
        memcpy(out->run_name, run_name.data(), run_name.size() * 8);
    }
    std::vector<int64_t> at(base.begin(), base.end() - 1);
    for (size_t i = 0; i < n_sites; ++i) {
        const uint8_t *line = text + lines[i].s;
        split_line(line, lines[i].e - lines[i].s, n_cols, fields);
        for (size_t q = 0; q < nq; ++q) {
            const Span c = fields[(size_t)sel_col[q]];
            if (out->off) out->off[q * (n_sites + 1) + i] = at[q];
            if (sel_len[q]) {
                out->seq[at[q]++] = pgs_map(line[c.s + sel_off[q]], cfg->n_to_gap);
            } else {
                for (int64_t k = c.s; k < c.e; ++k) out->seq[at[q]++] = pgs_map(line[k], cfg->n_to_gap);
            }
        }
    }
    if (out->off)
        for (size_t q = 0; q < nq; ++q) out->off[q * (n_sites + 1) + n_sites] = at[q];
    return PG_OK;
}
