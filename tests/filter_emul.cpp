// The device route of the filterGenotypes.py drop-in walked on the host: the same pgf_classify / pgf_add / pgf_site_test / pgf_render
// the kernels of genomics_general_amd/csrc/pg_filter_dev.hip are made of (csrc/pg_filter_core.h, compiled here by g++), with the
// kernels' division of the work restated serially: k_filt_lines<0> = the loop over lines (regular spelling, contig, sums, siteTest,
// flags, sizes), k_filt_thin = a walk per pod, the scan = the running offset, k_filt_lines<1> = the rows' text.  tests/test_filter_emul.py
// puts it in the device's place inside the driver and holds the output against the host route.  Test infrastructure.
#include "../genomics_general_amd/csrc/pg_filter_core.h"

#include <cstring>
#include <string>
#include <vector>

namespace {

enum { KEPT = 1, PASS = 2, TEST_ERR = 4, ROW_ERR = 8 };

// the line's tab table (k_filt_lines: line_tabs); false: not the regular spelling
bool line_tabs(const uint8_t *l, uint32_t n, int n_cols, std::vector<uint32_t> &tabs) {
    tabs.clear();
    if (n == 0) return false;
    for (uint32_t k = 0; k < n; ++k) {
        const uint8_t b = l[k];
        if (b == ' ' || b == '\v' || b == '\f' || b == '\r' || (b >= 0x1c && b <= 0x1f) || b >= 0x80) return false;
        if (b == '\t') tabs.push_back(k);
    }
    if ((int)tabs.size() != n_cols - 1) return false;
    for (int c = 0; c < n_cols; ++c) {
        const uint32_t s = c ? tabs[(size_t)c - 1] + 1 : 0, e = c < n_cols - 1 ? tabs[(size_t)c] : n;
        if (e <= s) return false;
    }
    return true;
}

void field(const std::vector<uint32_t> &tabs, int c, int n_cols, uint32_t n, uint32_t *s, uint32_t *e) {
    *s = c ? tabs[(size_t)c - 1] + 1 : 0;
    *e = c < n_cols - 1 ? tabs[(size_t)c] : n;
}

}  // namespace

// One block: 0 and the rows in out (*out_len bytes), or 1 and *host_line (the block is the host route's), or -1 (out too small)
extern "C" int pgf_emul_block(const pg_filter_cfg *cfgp, const int32_t *sel_col, const int32_t *sel_ploidy, const uint32_t *sel_popmask,
                              const char *contigs, int n_contig_bytes, const uint8_t *contig_flags, const char *text, int64_t len,
                              char *out, int64_t cap, int64_t *out_len, int64_t *host_line) {
    const PgfConfig &cfg = *cfgp;
    *out_len = 0;
    *host_line = -1;
    if (len == 0) return 0;
    if (text[len - 1] != '\n') { *host_line = 0; return 1; }
    std::vector<std::string> names;
    for (int k = 0, at = 0; k < cfg.n_contigs && at < n_contig_bytes; ++k) {
        names.emplace_back(contigs + at);
        at += (int)names.back().size() + 1;
    }
    const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
    std::vector<int64_t> nl;
    for (int64_t k = 0; k < len; ++k)
        if (t[k] == '\n') nl.push_back(k);
    const int64_t n_lines = (int64_t)nl.size();
    std::vector<uint8_t> flags((size_t)n_lines, 0);
    std::vector<uint32_t> rlen((size_t)n_lines, 0);
    std::vector<int64_t> pos((size_t)n_lines, 0);
    std::vector<uint32_t> tabs;
    char cell[PGF_CELL_MAX];
    auto sums = [&](const uint8_t *l, uint32_t n, PgfCounts *tot, PgfCounts *pop) {
        *tot = PgfCounts{};
        for (int k = 0; k < cfg.n_pops; ++k) pop[k] = PgfCounts{};
        for (int j = 0; j < cfg.n_sel; ++j) {
            uint32_t s, e;
            field(tabs, sel_col[j], cfg.n_cols, n, &s, &e);
            PgfGeno g;
            if (e - s > 40 || pgf_classify(l + s, (int)(e - s), cfg.in_fmt, sel_ploidy[j], cfg.force_ploidy, cfg.partial_to_missing, &g)) return false;
            pgf_add(g, tot);
            for (uint32_t m = sel_popmask[j]; m; m &= m - 1) pgf_add(g, &pop[__builtin_ctz(m)]);
        }
        return true;
    };
    // k_filt_lines<0>
    for (int64_t i = 0; i < n_lines; ++i) {
        const int64_t ls = i ? nl[(size_t)i - 1] + 1 : 0;
        const uint8_t *l = t + ls;
        const uint32_t n = (uint32_t)(nl[(size_t)i] - ls);
        if (!line_tabs(l, n, cfg.n_cols, tabs)) { *host_line = i; return 1; }
        const uint32_t f0e = tabs[0], f1s = tabs[0] + 1, f1e = cfg.n_cols > 2 ? tabs[1] : n;
        if (cfg.contig_mode) {
            bool in = false, ex = false;
            for (size_t k = 0; k < names.size(); ++k)
                if (names[k].size() == f0e && memcmp(names[k].data(), l, f0e) == 0) {
                    in = in || (contig_flags[k] & 1);
                    ex = ex || (contig_flags[k] & 2);
                }
            if (((cfg.contig_mode & 1) && !in) || ((cfg.contig_mode & 2) && ex)) continue;
        }
        PgfCounts tot, pop[PGF_MAXPOP];
        if (!sums(l, n, &tot, pop)) { *host_line = i; return 1; }
        uint8_t fl = KEPT;
        if (cfg.thin_dist && pgf_parse_pos(l + f1s, (int)(f1e - f1s), &pos[(size_t)i])) { *host_line = i; return 1; }
        const int r = cfg.no_test ? 1 : pgf_site_test(cfg, tot, pop);
        if (r == 1) fl |= PASS;
        if (r < 0) fl |= TEST_ERR;
        uint32_t size = 0;
        if (r == 1) {
            int order[4];
            const int nA = pgf_order(tot.c, order);
            uint32_t sum = 0;
            for (int j = 0; j < cfg.n_sel && !(fl & ROW_ERR); ++j) {
                uint32_t s, e;
                field(tabs, sel_col[j], cfg.n_cols, n, &s, &e);
                PgfGeno g;
                pgf_classify(l + s, (int)(e - s), cfg.in_fmt, sel_ploidy[j], cfg.force_ploidy, cfg.partial_to_missing, &g);
                const int L = pgf_render(cfg, g, order, nA, cell);
                if (L < 0) fl |= ROW_ERR;
                else sum += (uint32_t)L + 1;
            }
            if (!(fl & ROW_ERR)) size = f1e + sum + 1;
        }
        if (!cfg.thin_dist && (fl & (TEST_ERR | ROW_ERR))) { *host_line = i; return 1; }
        flags[(size_t)i] = fl;
        rlen[(size_t)i] = (fl & ROW_ERR) ? 0 : size;
    }
    // k_filt_thin
    if (cfg.thin_dist)
        for (int64_t a = 0; a < n_lines; a += cfg.pod_size) {
            const int64_t b = a + cfg.pod_size < n_lines ? a + cfg.pod_size : n_lines;
            bool have = false;
            int64_t last_s = 0, last_n = 0, last_pos = 0;
            for (int64_t i = a; i < b; ++i) {
                const uint8_t fl = flags[(size_t)i];
                if (!(fl & KEPT)) continue;
                const int64_t ls = i ? nl[(size_t)i - 1] + 1 : 0;
                int64_t cn = 0;
                while (t[ls + cn] != '\t') ++cn;
                const bool same = have && cn == last_n && memcmp(t + ls, t + last_s, (size_t)cn) == 0;
                if (!same) { last_s = ls; last_n = cn; have = true; }
                const bool keep = pgf_thin_keep(same, pos[(size_t)i], &last_pos, cfg.thin_dist);
                if (keep && (fl & TEST_ERR)) { *host_line = i; return 1; }
                const bool pass = keep && (fl & PASS);
                if (pass && (fl & ROW_ERR)) { *host_line = i; return 1; }
                if (pass) last_pos = pos[(size_t)i];
                else rlen[(size_t)i] = 0;
            }
        }
    // the scan and k_filt_lines<1>
    int64_t at = 0;
    for (int64_t i = 0; i < n_lines; ++i) {
        if (!rlen[(size_t)i]) continue;
        if (at + rlen[(size_t)i] > cap) return -1;
        const int64_t ls = i ? nl[(size_t)i - 1] + 1 : 0;
        const uint8_t *l = t + ls;
        const uint32_t n = (uint32_t)(nl[(size_t)i] - ls);
        line_tabs(l, n, cfg.n_cols, tabs);
        PgfCounts tot, pop[PGF_MAXPOP];
        sums(l, n, &tot, pop);
        int order[4];
        const int nA = pgf_order(tot.c, order);
        const uint32_t f1e = cfg.n_cols > 2 ? tabs[1] : n;
        char *o = out + at;
        memcpy(o, l, f1e);
        uint32_t w = f1e;
        for (int j = 0; j < cfg.n_sel; ++j) {
            uint32_t s, e;
            field(tabs, sel_col[j], cfg.n_cols, n, &s, &e);
            PgfGeno g;
            pgf_classify(l + s, (int)(e - s), cfg.in_fmt, sel_ploidy[j], cfg.force_ploidy, cfg.partial_to_missing, &g);
            const int L = pgf_render(cfg, g, order, nA, cell);
            o[w++] = '\t';
            memcpy(o + w, cell, (size_t)L);
            w += (uint32_t)L;
        }
        o[w++] = '\n';
        if (w != rlen[(size_t)i]) return -2;                     // (the sizes of the first pass and the text of the second disagree)
        at += w;
    }
    *out_len = at;
    return 0;
}
