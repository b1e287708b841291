// The device route of the genoToEigenstrat.py drop-in walked on the host: what k_eig_lines and k_rows_scan
// (genomics_general_amd/csrc/pg_eig_dev.hip) do with a block -- the regular-spelling test, the position, the cells of ALL columns in
// the lanes' order and their base counts summed lane by lane, the site's decision, the label's entry, the .snp row's size, the ranks
// and places, the digits of the SELECTED columns at rank x (n_sel + 1), the .snp row's bytes at their place -- with the very functions
// of pg_eig_core.h, compiled by g++.  tests/test_eig_emul.py puts it in the device's place inside the driver.  No GPU, no HIP.
#include "../genomics_general_amd/csrc/pg_eig_core.h"

#include <cstring>
#include <vector>

namespace {

const uint32_t MAX_CELL_IN = 2 * PGE_DEV_ALLELES - 1;

struct Line {
    const uint8_t *p;
    uint32_t n;
    std::vector<uint32_t> tabs;
};

// line_tabs (pg_line_fields.h) without the ballots
bool regular(Line &L, int n_cols) {
    L.tabs.clear();
    if (L.n == 0) return false;
    for (uint32_t k = 0; k < L.n; ++k) {
        const uint8_t b = L.p[k];
        if (b == '\t') L.tabs.push_back(k);
        else if (b == ' ' || b == '\v' || b == '\f' || b == '\r' || (b >= 0x1c && b <= 0x1f) || b >= 0x80) return false;
    }
    if ((int)L.tabs.size() != n_cols - 1) return false;
    for (int c = 0; c < n_cols; ++c) {
        const uint32_t s = c ? L.tabs[(size_t)c - 1] + 1 : 0, e = c < n_cols - 1 ? L.tabs[(size_t)c] : L.n;
        if (e <= s) return false;
    }
    return true;
}

void field(const Line &L, int c, int n_cols, uint32_t *s, uint32_t *e) {
    *s = L.tabs[(size_t)c - 1] + 1;
    *e = c < n_cols - 1 ? L.tabs[(size_t)c] : L.n;
}

struct Site {
    uint32_t rlen = 0, pz = 0, f0e = 0, pos_len = 0;
    int32_t entry = 0;
    PgeSite site{0, 0, 0};
};

// k_eig_lines<0> for one line: 0 decided (S->rlen: kept), 1 the host's
int size_line(const PgeConfig &cfg, const pgm_fai &F, const int64_t *label_off, int64_t index, Line &L, Site *S) {
    if (L.n > 0 && L.p[0] == '#') return 1;
    if (!regular(L, cfg.n_cols)) return 1;
    const uint32_t f0e = L.tabs[0], f1e = L.tabs[1];
    int64_t pos = 0;
    const uint32_t pz = pgg_pos_zeros(L.p + f0e + 1, (int64_t)f1e - f0e - 1);
    if (!pgg_pos_plain(L.p + f0e + 1 + pz, (int64_t)f1e - f0e - 1 - pz, &pos)) return 1;
    PgfCounts lane_sum[64] = {};
    for (int lane = 0; lane < 64; ++lane)
        for (int c = 2 + lane; c < cfg.n_cols; c += 64) {
            uint32_t s, e;
            field(L, c, cfg.n_cols, &s, &e);
            PgfGeno g;
            if (e - s > MAX_CELL_IN || pgg_classify(L.p + s, (int)(e - s), cfg.in_fmt, &g) || g.n > PGE_DEV_ALLELES) return 1;
            pgf_add(g, &lane_sum[lane]);
        }
    int32_t c4[4] = {0, 0, 0, 0};
    for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < 4; ++b) c4[b] += lane_sum[lane].c[b];
    S->rlen = 0;
    if (!pge_site(c4, &S->site)) return 0;
    int32_t e = pgm_lookup(F, L.p, f0e);
    if (e < 0) e = cfg.n_scaf;
    S->entry = e;
    S->f0e = f0e;
    S->pz = pz;
    S->pos_len = f1e - f0e - 1 - pz;
    S->rlen = pge_snp_len(index, (uint32_t)(label_off[e + 1] - label_off[e]), S->pos_len);
    return 0;
}

}  // namespace

// 0: *n_rows rows, n_sel + 1 bytes each in geno, *snp_len bytes in snp; 1: the block is the host's (*host_line its first such line);
// -1: snp too small; -2: the size pass and the render pass disagree
extern "C" int pge_emul_block(const pg_eig_cfg *cfg, const int32_t *sel_col, const char *names, const int64_t *name_off, const int32_t *table,
                              uint32_t mask, const char *labels, const int64_t *label_off, int64_t first_site, const char *text, int64_t len,
                              uint8_t *geno, uint8_t *snp, int64_t snp_cap, int64_t *n_rows, int64_t *snp_len, int64_t *host_line) {
    *n_rows = *snp_len = 0;
    *host_line = -1;
    if (len == 0) return 0;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
    if (t[len - 1] != '\n') { *host_line = 0; return 1; }
    const pgm_fai F{reinterpret_cast<const uint8_t *>(names), name_off, nullptr, table, mask, cfg->n_scaf};
    std::vector<Line> lines;
    for (int64_t k = 0; k < len;) {
        const uint8_t *e = static_cast<const uint8_t *>(memchr(t + k, '\n', (size_t)(len - k)));
        lines.push_back(Line{t + k, (uint32_t)(e - (t + k)), {}});
        k = (e - t) + 1;
    }
    std::vector<Site> sites(lines.size());
    std::vector<int64_t> roff(lines.size()), rank(lines.size());
    int64_t total = 0, rows = 0;
    for (size_t i = 0; i < lines.size(); ++i) {
        if (size_line(*cfg, F, label_off, first_site + (int64_t)i, lines[i], &sites[i])) { *host_line = (int64_t)i; return 1; }
        roff[i] = total;                                           // k_rows_scan
        rank[i] = rows;
        total += sites[i].rlen;
        rows += sites[i].rlen != 0;
    }
    if (total > snp_cap) return -1;
    char num[24], tail[8];
    for (size_t i = 0; i < lines.size(); ++i) {                    // k_eig_lines<1>
        const Site &S = sites[i];
        if (!S.rlen) continue;
        const Line &L = lines[i];
        uint8_t *gr = geno + rank[i] * (int64_t)(cfg->n_sel + 1);
        for (int j = 0; j < cfg->n_sel; ++j) {
            uint32_t s, e;
            field(L, sel_col[j], cfg->n_cols, &s, &e);
            PgfGeno g;
            pgg_classify(L.p + s, (int)(e - s), cfg->in_fmt, &g);
            gr[j] = (uint8_t)('0' + pge_count(g, S.site.counted));
        }
        gr[cfg->n_sel] = '\n';
        uint8_t *o = snp + roff[i];
        uint32_t w = (uint32_t)pgg_pos_text(first_site + (int64_t)i, num);
        memcpy(o, num, w);
        o[w++] = '\t';
        const uint32_t ll = (uint32_t)(label_off[S.entry + 1] - label_off[S.entry]);
        memcpy(o + w, labels + label_off[S.entry], ll);
        w += ll;
        memcpy(o + w, "\t0.0\t", 5);
        w += 5;
        memcpy(o + w, L.p + S.f0e + 1 + S.pz, S.pos_len);
        w += S.pos_len;
        w += (uint32_t)pge_snp_tail(S.site, tail);
        memcpy(o + w - 5, tail, 5);
        if (w != S.rlen) return -2;
    }
    *n_rows = rows;
    *snp_len = total;
    return 0;
}
