// The host route of the genoToVCF.py drop-in (pg_gvcf_text): every spelling the reference's `line.split(None, 2)` / `split()` takes,
// the blocks the device route hands back, and PG_GVCF_DEVICE=0.  Lines are cut as the reference's text-mode file cuts them (universal
// newlines: \n, \r\n and a lone \r end a line; stdin: \n only), fields at runs of ASCII whitespace; the lines are split over host
// threads, each walking its share in order with the per-site / per-cell functions of pg_gvcf_core.h.  No GPU context is needed, and
// nothing but the C++ library: tests/gvcf_host_main.cpp compiles this file on its own.
#include "pg_gvcf_core.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace {

struct GvcfTables {
    const PggConfig *cfg;
    const int32_t *sel_col, *prev_same;
    pgg_ref R;
};

struct Field {
    const uint8_t *p;
    int64_t len;
};

struct Run {
    std::string out;
    int64_t rows = 0;
    int64_t err_line = -1;
    int err = 0;
};

// lines [a, b) of the block
void gvcf_lines(const GvcfTables &T, const uint8_t *text, const std::vector<int64_t> &ls, const std::vector<int64_t> &le, int64_t a, int64_t b, Run *R) {
    const PggConfig &cfg = *T.cfg;
    std::vector<Field> f;
    std::vector<PgfGeno> g((size_t)std::max(cfg.n_sel, 1));
    char cell[2 * PGF_MAXA], mid[32], num[24], al[PGG_MAX_ALLELES];
    for (int64_t i = a; i < b; ++i) {
        const uint8_t *p = text + ls[(size_t)i];
        const int64_t n = le[(size_t)i] - ls[(size_t)i];
        if (n > 0 && p[0] == '#') continue;                                // genomics.py:1936
        auto fail = [&](int code) { R->err_line = i; R->err = code; };
        for (int64_t k = 0; k < n; ++k)
            if (p[k] >= 0x80) { fail(PGG_E_ASCII); return; }
        f.clear();
        for (int64_t k = 0; k < n;) {
            while (k < n && pgm_is_space(p[k])) ++k;
            if (k >= n) break;
            const int64_t s = k;
            while (k < n && !pgm_is_space(p[k])) ++k;
            f.push_back(Field{p + s, k - s});
        }
        if (f.size() < 2) { fail(PGG_E_COLS); return; }                    // lineData[-1] / lineData[posCol] (IndexError)
        int64_t pos = 0;
        int e = pgg_parse_pos(f[1].p, f[1].len, &pos);
        if (e) { fail(e); return; }
        // the cells: what follows the second field -- of a line of two fields the second itself (lineData[-1])
        const int64_t c0 = f.size() == 2 ? 1 : 2, n_cells = (int64_t)f.size() - c0;
        PgfCounts tot = {};
        for (int j = 0; j < cfg.n_sel; ++j) {
            int64_t c = T.sel_col[j] - 2;
            while (c >= n_cells && c >= 0) c = T.prev_same ? (int64_t)T.prev_same[c + 2] - 2 : -1;
            if (c < 0) { fail(PGG_E_COLS); return; }
            const Field &x = f[(size_t)(c0 + c)];
            if (x.len > 0x7fffffff) { fail(PGG_E_CELL); return; }
            e = pgg_classify(x.p, (int)x.len, cfg.in_fmt, &g[(size_t)j]);
            if (e) { fail(e); return; }
            pgf_add(g[(size_t)j], &tot);
        }
        char ref = 0;
        if (cfg.has_ref) {
            const int32_t s = pgm_lookup(T.R.F, f[0].p, f[0].len);
            if (s < 0) { fail(PGG_E_SCAF); return; }
            e = pgg_ref_base(T.R, s, pos, &ref);
            if (e) { fail(e); return; }
        }
        const int nA = pgg_alleles(tot.c, cfg.has_ref != 0, ref, al);
        R->out.append(reinterpret_cast<const char *>(f[0].p), (size_t)f[0].len);
        R->out.push_back('\t');
        R->out.append(num, (size_t)pgg_pos_text(pos, num));
        R->out.append(mid, (size_t)pgg_middle(al, nA, mid));
        for (int j = 0; j < cfg.n_sel; ++j) {
            R->out.push_back('\t');
            R->out.append(cell, (size_t)pgg_cell(g[(size_t)j], al, nA, cell));
        }
        R->out.push_back('\n');
        ++R->rows;
    }
}

}  // namespace

extern "C" int pg_gvcf_ref_table(const char *ref_names, const int64_t *name_off, int32_t n_seq, int32_t *table, uint32_t mask) {
    if (n_seq < 0 || !table || (mask & (mask + 1)) || mask < 3 || (uint64_t)mask + 1 < 2ull * (uint64_t)n_seq || (n_seq && (!ref_names || !name_off)))
        return PG_ERR_ARG;
    for (uint32_t k = 0; k <= mask; ++k) table[k] = -1;
    const uint8_t *names = reinterpret_cast<const uint8_t *>(ref_names);
    for (int32_t s = 0; s < n_seq; ++s) {
        if (name_off[s + 1] < name_off[s]) return PG_ERR_ARG;
        uint32_t at = pgm_hash(names + name_off[s], name_off[s + 1] - name_off[s]) & mask;
        while (table[at] >= 0) at = (at + 1) & mask;
        table[at] = s;
    }
    return PG_OK;
}

extern "C" int pg_gvcf_text(const pg_gvcf_cfg *cfg, const int32_t *sel_col, const int32_t *prev_same, const char *ref_names, const int64_t *name_off,
                            const int64_t *seq_len, const int64_t *seq_off, const int32_t *table, uint32_t mask, int32_t n_seq, const uint8_t *seq,
                            const char *text, int64_t len, int n_threads, char *out, int64_t out_cap, int64_t *rows_len_out, int64_t *n_rows_out,
                            int64_t *err_line_out, int *err_code_out) {
    if (!cfg || !rows_len_out || !n_rows_out || !err_line_out || !err_code_out || (len && !text) || len < 0 || out_cap < 0 || (out_cap && !out) ||
        cfg->n_sel < 0 || (cfg->n_sel > 0 && !sel_col) || n_seq < 0 ||
        (cfg->has_ref && (n_seq < 1 || !ref_names || !name_off || !seq_len || !seq_off || !table || !seq)))
        return PG_ERR_ARG;
    for (int j = 0; j < cfg->n_sel; ++j)
        if (sel_col[j] < 2 || sel_col[j] >= cfg->n_cols) return PG_ERR_ARG;
    *rows_len_out = *n_rows_out = 0;
    *err_line_out = -1;
    *err_code_out = 0;
    GvcfTables T;
    T.cfg = cfg;
    T.sel_col = sel_col;
    T.prev_same = prev_same;
    T.R.F = pgm_fai{reinterpret_cast<const uint8_t *>(ref_names), name_off, seq_len, table, mask, cfg->has_ref ? n_seq : 0};
    T.R.seq = seq;
    T.R.seq_off = seq_off;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
    const bool uni = cfg->universal_newlines != 0;
    std::vector<int64_t> ls, le;
    for (int64_t k = 0; k < len;) {
        const int64_t s = k;
        while (k < len && t[k] != '\n' && !(uni && t[k] == '\r')) ++k;
        ls.push_back(s);
        le.push_back(k);
        if (k < len) k += (t[k] == '\r' && k + 1 < len && t[k + 1] == '\n') ? 2 : 1;
    }
    const int64_t n_lines = (int64_t)ls.size();
    const int nt = std::max(1, n_threads);
    const int64_t per = std::max<int64_t>(4096, (n_lines + nt - 1) / nt);
    std::vector<int64_t> cuts{0};
    while (cuts.back() < n_lines) cuts.push_back(std::min(n_lines, cuts.back() + per));
    const size_t nr = cuts.size() - 1;
    std::vector<Run> runs(nr);
    if (nr == 1) gvcf_lines(T, t, ls, le, 0, n_lines, &runs[0]);
    else if (nr > 1) {
        std::vector<std::thread> th;
        for (size_t r = 0; r < nr; ++r) th.emplace_back(gvcf_lines, std::cref(T), t, std::cref(ls), std::cref(le), cuts[r], cuts[r + 1], &runs[r]);
        for (auto &x : th) x.join();
    }
    int64_t total = 0, rows = 0;
    size_t upto = nr;
    for (size_t r = 0; r < nr; ++r) {
        total += (int64_t)runs[r].out.size();
        rows += runs[r].rows;
        if (runs[r].err) {                                  // the first line that stops the run, in input order: the rows before it stand
            *err_line_out = runs[r].err_line;
            *err_code_out = runs[r].err;
            upto = r + 1;
            break;
        }
    }
    *rows_len_out = total;
    *n_rows_out = rows;
    if (total > out_cap) return PG_OK;                      // (the caller comes back with the room)
    int64_t at = 0;
    for (size_t r = 0; r < upto; ++r) {
        if (!runs[r].out.empty()) memcpy(out + at, runs[r].out.data(), runs[r].out.size());
        at += (int64_t)runs[r].out.size();
    }
    return PG_OK;
}
