// The device route of the genoToVCF.py drop-in walked on the host: what k_gvcf_lines (genomics_general_amd/csrc/pg_gvcf_dev.hip) does
// with a block -- the regular-spelling test, the position, the cells of the selected columns in the lanes' order, the base counts, the
// reference base, the alleles, the row's size, the scan, the row's bytes at their place -- with the very functions of pg_gvcf_core.h,
// compiled by g++.  tests/test_gvcf_emul.py puts it in the device's place inside the driver.  No GPU, no HIP.
#include "../genomics_general_amd/csrc/pg_gvcf_core.h"

#include <cstring>
#include <vector>

namespace {

const int MAX_CELL_IN = 40;

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

struct Site {
    bool skip = false;
    uint32_t head = 0, pz = 0, f0e = 0, len = 0;
    int nA = 0;
    char al[PGG_MAX_ALLELES];
};

// k_gvcf_lines<0> for one line: 0 a row (or a '#' line), 1 the host's
int size_line(const PggConfig &cfg, const int32_t *sel_col, const pgg_ref &R, Line &L, Site *S) {
    if (L.n > 0 && L.p[0] == '#') { S->skip = true; return 0; }
    if (!regular(L, cfg.n_cols)) return 1;
    const uint32_t f0e = L.tabs[0], f1e = L.tabs[1];
    int64_t pos = 0;
    const uint32_t pz = pgg_pos_zeros(L.p + f0e + 1, (int64_t)f1e - f0e - 1);
    if (!pgg_pos_plain(L.p + f0e + 1 + pz, (int64_t)f1e - f0e - 1 - pz, &pos)) return 1;
    PgfCounts lane_sum[64] = {};
    uint32_t cells = 0;
    for (int lane = 0; lane < 64; ++lane)
        for (int j = lane; j < cfg.n_sel; j += 64) {
            const int c = sel_col[j];
            const uint32_t s = L.tabs[(size_t)c - 1] + 1, e = c < cfg.n_cols - 1 ? L.tabs[(size_t)c] : L.n;
            PgfGeno g;
            if (e - s > (uint32_t)MAX_CELL_IN || pgg_classify(L.p + s, (int)(e - s), cfg.in_fmt, &g)) return 1;
            pgf_add(g, &lane_sum[lane]);
            cells += (uint32_t)pgg_cell_len(g) + 1;
        }
    int32_t c4[4] = {0, 0, 0, 0};
    for (int lane = 0; lane < 64; ++lane)
        for (int b = 0; b < 4; ++b) c4[b] += lane_sum[lane].c[b];
    char ref = 0;
    if (cfg.has_ref) {
        const int32_t s = pgm_lookup(R.F, L.p, f0e);
        if (s < 0 || pgg_ref_base(R, s, pos, &ref)) return 1;
    }
    S->nA = pgg_alleles(c4, cfg.has_ref != 0, ref, S->al);
    S->f0e = f0e;
    S->pz = pz;
    S->head = f1e - pz;
    S->len = S->head + 3u + (uint32_t)pgg_ref_alt_len(S->nA) + PGG_FIXED_LEN + cells + 1u;
    return 0;
}

}  // namespace

// 0: *rows_len bytes of rows in out; 1: the block is the host's (*host_line its first such line); -1: out too small
extern "C" int pgg_emul_block(const pg_gvcf_cfg *cfg, const int32_t *sel_col, const char *ref_names, const int64_t *name_off, const int64_t *seq_len,
                              const int64_t *seq_off, const int32_t *table, uint32_t mask, int32_t n_seq, const uint8_t *seq, const char *text,
                              int64_t len, uint8_t *out, int64_t cap, int64_t *rows_len, int64_t *host_line) {
    *rows_len = 0;
    *host_line = -1;
    if (len == 0) return 0;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
    if (t[len - 1] != '\n') { *host_line = 0; return 1; }
    pgg_ref R;
    R.F = pgm_fai{reinterpret_cast<const uint8_t *>(ref_names), name_off, seq_len, table, mask, cfg->has_ref ? n_seq : 0};
    R.seq = seq;
    R.seq_off = seq_off;
    std::vector<Line> lines;
    for (int64_t k = 0; k < len;) {
        const uint8_t *e = static_cast<const uint8_t *>(memchr(t + k, '\n', (size_t)(len - k)));
        lines.push_back(Line{t + k, (uint32_t)(e - (t + k)), {}});
        k = (e - t) + 1;
    }
    std::vector<Site> sites(lines.size());
    int64_t total = 0;
    for (size_t i = 0; i < lines.size(); ++i) {
        if (size_line(*cfg, sel_col, R, lines[i], &sites[i])) { *host_line = (int64_t)i; return 1; }
        total += sites[i].len;
    }
    if (total > cap) return -1;
    int64_t at = 0;
    char mid[24], cell[2 * PGF_MAXA];
    for (size_t i = 0; i < lines.size(); ++i) {                    // k_gvcf_lines<1>
        const Site &S = sites[i];
        if (S.skip) continue;
        const Line &L = lines[i];
        uint8_t *o = out + at;
        for (uint32_t k = 0; k < S.head; ++k) o[k] = L.p[k <= S.f0e ? k : k + S.pz];
        uint32_t w = S.head + (uint32_t)pgg_middle(S.al, S.nA, mid);
        memcpy(o + S.head, mid, w - S.head);
        for (int j = 0; j < cfg->n_sel; ++j) {
            const int c = sel_col[j];
            const uint32_t s = L.tabs[(size_t)c - 1] + 1, e = c < cfg->n_cols - 1 ? L.tabs[(size_t)c] : L.n;
            PgfGeno g;
            pgg_classify(L.p + s, (int)(e - s), cfg->in_fmt, &g);
            o[w++] = '\t';
            w += (uint32_t)pgg_cell(g, S.al, S.nA, cell);
            memcpy(o + w - pgg_cell_len(g), cell, (size_t)pgg_cell_len(g));
        }
        o[w++] = '\n';
        if (w != S.len) return -2;                                 // the size pass and the render pass disagree
        at += S.len;
    }
    *rows_len = at;
    return 0;
}
