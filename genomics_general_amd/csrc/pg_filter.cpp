// The host route of the filterGenotypes.py drop-in (pg_filter_text): every spelling the reference's `line.split()` takes, the blocks the
// device route hands back, and PG_FILTER_DEVICE=0.  Lines are cut as the reference's text-mode file cuts them (universal newlines:
// \n, \r\n and a lone \r end a line), fields at runs of ASCII whitespace; the pods (filterGenotypes.py:393-403) are split over host
// threads, each walking its lines in order with the per-cell / per-site functions of pg_filter_core.h.  No GPU context is needed.
#include "pg_ctx.h"
#include "pg_filter_core.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

int pg_host_threads();

namespace {

struct FiltTables {
    const PgfConfig *cfg;
    const int32_t *sel_col, *sel_ploidy;
    const uint32_t *sel_popmask;
    std::vector<std::string> names;
    std::vector<uint8_t> flags;
};

inline bool is_ws(uint8_t b) { return b == ' ' || b == '\t' || b == '\v' || b == '\f' || b == '\r' || (b >= 0x1c && b <= 0x1f); }

struct Field {
    const uint8_t *p;
    int len;
};

// the contig test of filterGenotypes.py:37: true = the line is skipped
bool contig_skipped(const FiltTables &T, const uint8_t *p, int len) {
    if (!T.cfg->contig_mode) return false;
    bool in = false, ex = false;
    for (size_t k = 0; k < T.names.size(); ++k)
        if ((int)T.names[k].size() == len && memcmp(T.names[k].data(), p, (size_t)len) == 0) {
            in = in || (T.flags[k] & 1);
            ex = ex || (T.flags[k] & 2);
        }
    return ((T.cfg->contig_mode & 1) && !in) || ((T.cfg->contig_mode & 2) && ex);
}

struct Run {
    std::string out;
    int64_t rows = 0;
    int64_t err_line = -1;
    int err = 0;
};

// lines [a, b) of the block (starts / ends), the first of them line `first` of the block; the pods' state resets where
// (first_line + index) % pod_size == 0
void filter_lines(const FiltTables &T, const uint8_t *text, const std::vector<int64_t> &ls, const std::vector<int64_t> &le, int64_t a, int64_t b,
                  int64_t first_line, Run *R) {
    const PgfConfig &cfg = *T.cfg;
    std::vector<Field> f;
    std::vector<PgfGeno> g((size_t)cfg.n_sel);
    std::vector<PgfCounts> pop((size_t)std::max(cfg.n_pops, 1));
    std::string last_scaf;
    bool have_scaf = false;
    int64_t last_pos = 0;
    char cell[PGF_CELL_MAX];
    for (int64_t i = a; i < b; ++i) {
        if (cfg.thin_dist && (first_line + i) % cfg.pod_size == 0) have_scaf = false;          // lastScaf = None per pod
        const uint8_t *p = text + ls[(size_t)i];
        const int64_t n = le[(size_t)i] - ls[(size_t)i];
        auto fail = [&](int code) { R->err_line = i; R->err = code; };
        f.clear();
        for (int64_t k = 0; k < n;) {
            while (k < n && is_ws(p[k])) ++k;
            if (k >= n) break;
            const int64_t s = k;
            while (k < n && !is_ws(p[k])) ++k;
            if (k - s > 0x7fffffff) { fail(PGF_E_CELL); return; }
            f.push_back(Field{p + s, (int)(k - s)});
        }
        for (int64_t k = 0; k < n; ++k)
            if (p[k] >= 0x80) { fail(PGF_E_CELL); return; }
        if (f.empty()) { fail(PGF_E_COLS); return; }
        if (contig_skipped(T, f[0].p, f[0].len)) continue;
        PgfCounts tot = {};
        for (int k = 0; k < cfg.n_pops; ++k) pop[(size_t)k] = PgfCounts{};
        for (int j = 0; j < cfg.n_sel; ++j) {
            const int c = T.sel_col[j];
            if (c >= (int)f.size()) { fail(PGF_E_COLS); return; }
            const int e = pgf_classify(f[(size_t)c].p, f[(size_t)c].len, cfg.in_fmt, T.sel_ploidy[j], cfg.force_ploidy, cfg.partial_to_missing,
                                       &g[(size_t)j]);
            if (e) { fail(e); return; }
            pgf_add(g[(size_t)j], &tot);
            for (uint32_t m = T.sel_popmask[j]; m; m &= m - 1) pgf_add(g[(size_t)j], &pop[(size_t)__builtin_ctz(m)]);
        }
        bool good = true;
        int64_t pos = 0;
        if (cfg.thin_dist) {
            if (f.size() < 2) { fail(PGF_E_COLS); return; }
            if (pgf_parse_pos(f[1].p, f[1].len, &pos)) { fail(PGF_E_POS); return; }
            const bool same = have_scaf && last_scaf.size() == (size_t)f[0].len && memcmp(last_scaf.data(), f[0].p, (size_t)f[0].len) == 0;
            if (!same) {
                last_scaf.assign(reinterpret_cast<const char *>(f[0].p), (size_t)f[0].len);
                have_scaf = true;
            }
            good = pgf_thin_keep(same, pos, &last_pos, cfg.thin_dist);
        }
        if (good && !cfg.no_test) {
            const int t = pgf_site_test(cfg, tot, pop.data());
            if (t < 0) { fail(-t); return; }
            good = t == 1;
        }
        if (!good) continue;
        int order[4];
        const int nA = pgf_order(tot.c, order);
        const size_t mark = R->out.size();
        R->out.append(reinterpret_cast<const char *>(f[0].p), (size_t)f[0].len);
        if (f.size() > 1) {
            R->out.push_back('\t');
            R->out.append(reinterpret_cast<const char *>(f[1].p), (size_t)f[1].len);
        }
        for (int j = 0; j < cfg.n_sel; ++j) {
            const int L = pgf_render(cfg, g[(size_t)j], order, nA, cell);
            if (L < 0) { R->out.resize(mark); fail(-L); return; }
            R->out.push_back('\t');
            R->out.append(cell, (size_t)L);
        }
        R->out.push_back('\n');
        ++R->rows;
        if (cfg.thin_dist) last_pos = pos;
    }
}

}  // namespace

extern "C" int pg_filter_text(const pg_filter_cfg *cfg, const int32_t *sel_col, const int32_t *sel_ploidy, const uint32_t *sel_popmask,
                              const char *contigs, int n_contig_bytes, const uint8_t *contig_flags, const char *text, int64_t len,
                              int64_t first_line, int n_threads, char **rows_out, int64_t *rows_len_out, int64_t *n_rows_out,
                              int64_t *err_line_out, int *err_code_out) {
    if (!cfg || !rows_out || !rows_len_out || !n_rows_out || !err_line_out || !err_code_out || (len && !text) || len < 0 || first_line < 0 ||
        (cfg->n_sel > 0 && (!sel_col || !sel_ploidy || !sel_popmask)) || cfg->n_sel < 0 || cfg->n_pops < 0 || cfg->n_pops > PGF_MAXPOP ||
        (cfg->thin_dist && cfg->pod_size < 1) || n_contig_bytes < 0 || (cfg->n_contigs > 0 && (!contigs || !contig_flags)))
        return pg_fail(PG_ERR_ARG, "pg_filter_text: bad argument");
    *rows_out = nullptr;
    *rows_len_out = *n_rows_out = 0;
    *err_line_out = -1;
    *err_code_out = 0;
    FiltTables T;
    T.cfg = cfg;
    T.sel_col = sel_col;
    T.sel_ploidy = sel_ploidy;
    T.sel_popmask = sel_popmask;
    for (int k = 0, at = 0; k < cfg->n_contigs; ++k) {
        const void *z = at < n_contig_bytes ? memchr(contigs + at, 0, (size_t)(n_contig_bytes - at)) : nullptr;
        if (!z) return pg_fail(PG_ERR_ARG, "pg_filter_text: contig list shorter than n_contigs");
        const int e = (int)(static_cast<const char *>(z) - contigs);
        T.names.emplace_back(contigs + at, (size_t)(e - at));
        T.flags.push_back(contig_flags[k]);
        at = e + 1;
    }
    // the lines: universal newlines for a file read in text mode; stdin splits at \n only (its \r is whitespace in the line)
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
    // split at pod boundaries over the threads (without thinning any line is a boundary)
    int nt = n_threads > 0 ? n_threads : pg_host_threads();
    const int64_t unit = cfg->thin_dist ? cfg->pod_size : 4096;
    std::vector<int64_t> cuts{0};
    {
        const int64_t per = std::max<int64_t>(unit, (n_lines + nt - 1) / std::max(nt, 1));
        int64_t at = 0;
        while (at < n_lines) {
            int64_t nx = at + per;
            if (cfg->thin_dist) nx = ((first_line + nx + cfg->pod_size - 1) / cfg->pod_size) * cfg->pod_size - first_line;
            at = std::min(n_lines, nx);
            cuts.push_back(at);
        }
    }
    const size_t nr = cuts.size() - 1;
    std::vector<Run> runs(nr);
    if (nr == 1) filter_lines(T, t, ls, le, 0, n_lines, first_line, &runs[0]);
    else if (nr > 1) {
        std::vector<std::thread> th;
        for (size_t r = 0; r < nr; ++r) th.emplace_back(filter_lines, std::cref(T), t, std::cref(ls), std::cref(le), cuts[r], cuts[r + 1], first_line, &runs[r]);
        for (auto &x : th) x.join();
    }
    int64_t total = 0, rows = 0;
    size_t upto = nr;
    for (size_t r = 0; r < nr; ++r) {
        total += (int64_t)runs[r].out.size();
        rows += runs[r].rows;
        if (runs[r].err) {                                  // the first line that raises, in input order: the rows before it stand
            *err_line_out = runs[r].err_line;
            *err_code_out = runs[r].err;
            upto = r + 1;
            break;
        }
    }
    char *o = static_cast<char *>(malloc((size_t)total + 1));
    if (!o) return pg_fail(PG_ERR_ARG, "pg_filter_text: out of host memory (%lld bytes)", (long long)total);
    int64_t at = 0;
    for (size_t r = 0; r < upto; ++r) {
        memcpy(o + at, runs[r].out.data(), runs[r].out.size());
        at += (int64_t)runs[r].out.size();
    }
    *rows_out = o;
    *rows_len_out = at;
    *n_rows_out = rows;
    return PG_OK;
}

extern "C" void pg_filter_free(char *rows) { free(rows); }
