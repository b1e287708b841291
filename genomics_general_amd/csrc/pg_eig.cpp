// The host route of the genoToEigenstrat.py drop-in (pg_eig_text): every spelling the reference's `line.split(None, 2)` / `split()`
// takes, the blocks the device route hands back, --cumulativePos, a header with a repeated name, and PG_EIG_DEVICE=0.  Lines are cut as
// the reference's text-mode file cuts them (universal newlines: \n, \r\n and a lone \r end a line; stdin: \n only), fields at runs of
// ASCII whitespace; the lines are split over host threads, each walking its share in order with the per-site / per-cell functions of
// pg_eig_core.h.  --cumulativePos is a walk over the kept sites in file order: the threads leave a record per kept site, one thread
// writes their .snp rows.  No GPU context is needed, and nothing but the C++ library: tests/eig_host_main.cpp compiles this file on its
// own.
#include "pg_eig_core.h"

#include <algorithm>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

namespace {

struct EigTables {
    const PgeConfig *cfg;
    const int32_t *sel_col, *prev_same, *next_same;
    pgm_fai F;                                   // the --chromFile's scaffolds (F.len unused)
    const char *labels;
    const int64_t *label_off;                    // n_scaf + 2: entry n_scaf is str(nullChrom)
};

struct Field {
    const uint8_t *p;
    int64_t len;
};

// a kept site whose .snp row waits for the walk (--cumulativePos)
struct Rec {
    int64_t line, index, pos;
    const uint8_t *scaf;
    int64_t scaf_len;
    size_t geno_before;
    PgeSite site;
};

struct Run {
    std::string geno, snp;
    std::vector<Rec> recs;
    int64_t rows = 0;
    int64_t err_line = -1;
    int err = 0;
};

int32_t entry_of(const EigTables &T, const uint8_t *s, int64_t len) {
    const int32_t e = pgm_lookup(T.F, s, len);
    return e < 0 ? T.cfg->n_scaf : e;
}

void snp_row(const EigTables &T, std::string *out, int64_t index, int32_t entry, int64_t pos, const PgeSite &site) {
    char num[24], tail[8];
    out->append(num, (size_t)pgg_pos_text(index, num));
    out->push_back('\t');
    out->append(T.labels + T.label_off[entry], (size_t)(T.label_off[entry + 1] - T.label_off[entry]));
    out->append("\t0.0\t", 5);
    out->append(num, (size_t)pgg_pos_text(pos, num));
    out->append(tail, (size_t)pge_snp_tail(site, tail));
}

// lines [a, b) of the block; sidx: the sites in front of each line
void eig_lines(const EigTables &T, const uint8_t *text, const std::vector<int64_t> &ls, const std::vector<int64_t> &le, const std::vector<int64_t> &sidx,
               int64_t a, int64_t b, Run *R) {
    const PgeConfig &cfg = *T.cfg;
    const int64_t n_names = cfg.n_cols - 2;
    std::vector<Field> f;
    std::vector<PgfGeno> g((size_t)std::max<int64_t>(n_names, 1));
    std::vector<uint8_t> have((size_t)std::max<int64_t>(n_names, 1));
    char num[4];
    for (int64_t i = a; i < b; ++i) {
        const uint8_t *p = text + ls[(size_t)i];
        const int64_t n = le[(size_t)i] - ls[(size_t)i];
        if (n > 0 && p[0] == '#') continue;                                // genomics.py:1936
        auto fail = [&](int code) { R->err_line = i; R->err = code; };
        for (int64_t k = 0; k < n; ++k)
            if (p[k] >= 0x80) { fail(PGE_E_ASCII); return; }
        f.clear();
        for (int64_t k = 0; k < n;) {
            while (k < n && pgm_is_space(p[k])) ++k;
            if (k >= n) break;
            const int64_t s = k;
            while (k < n && !pgm_is_space(p[k])) ++k;
            f.push_back(Field{p + s, k - s});
        }
        if (f.size() < 2) { fail(PGE_E_COLS); return; }                    // lineData[-1] / lineData[posCol] (IndexError)
        int64_t pos = 0;
        int e = pgg_parse_pos(f[1].p, f[1].len, &pos);
        if (e) { fail(e); return; }
        // the cells: what follows the second field -- of a line of two fields the second itself (lineData[-1]); dict(zip(names, cells))
        // keeps of a repeated name the last cell the line has
        const int64_t c0 = f.size() == 2 ? 1 : 2, n_cells = std::min<int64_t>((int64_t)f.size() - c0, n_names);
        PgfCounts tot = {};
        for (int64_t c = 0; c < n_cells; ++c) {
            const int32_t nx = T.next_same ? T.next_same[c + 2] : -1;
            have[(size_t)c] = !(nx >= 0 && nx - 2 < n_cells);
            if (!have[(size_t)c]) continue;
            const Field &x = f[(size_t)(c0 + c)];
            if (x.len > 0x7fffffff) { fail(PGE_E_CELL); return; }
            e = pgg_classify(x.p, (int)x.len, cfg.in_fmt, &g[(size_t)c]);
            if (e) { fail(e); return; }
            pgf_add(g[(size_t)c], &tot);
        }
        PgeSite site;
        if (!pge_site(tot.c, &site)) continue;
        const size_t geno_before = R->geno.size();
        for (int j = 0; j < cfg.n_sel; ++j) {
            int64_t c = T.sel_col[j] - 2;
            while (c >= n_cells && c >= 0) c = T.prev_same ? (int64_t)T.prev_same[c + 2] - 2 : -1;
            if (c < 0) {
                R->geno.resize(geno_before);
                fail(PGE_E_NOCELL);
                return;
            }
            R->geno.append(num, (size_t)pge_count_text(pge_count(g[(size_t)c], site.counted), num));
        }
        R->geno.push_back('\n');
        ++R->rows;
        const int64_t index = sidx[(size_t)i];
        if (cfg.cumulative) R->recs.push_back(Rec{i, index, pos, f[0].p, f[0].len, geno_before, site});
        else snp_row(T, &R->snp, index, entry_of(T, f[0].p, f[0].len), pos, site);
    }
}

}  // namespace

extern "C" int pg_eig_text(const pg_eig_cfg *cfg, const int32_t *sel_col, const int32_t *prev_same, const int32_t *next_same, const char *names,
                           const int64_t *name_off, const int32_t *table, uint32_t mask, const char *labels, const int64_t *label_off,
                           const int32_t *label_key, pg_eig_state *state, int64_t *offsets, char *scaf_io, const char *text, int64_t len,
                           int n_threads, char *geno, int64_t geno_cap, char *snp, int64_t snp_cap, int64_t *geno_len_out, int64_t *snp_len_out,
                           int64_t *n_rows_out, int64_t *n_sites_out, int64_t *err_line_out, int *err_code_out) {
    if (!cfg || !state || !geno_len_out || !snp_len_out || !n_rows_out || !n_sites_out || !err_line_out || !err_code_out || (len && !text) ||
        len < 0 || geno_cap < 0 || snp_cap < 0 || (geno_cap && !geno) || (snp_cap && !snp) || cfg->n_sel < 0 || (cfg->n_sel > 0 && !sel_col) ||
        cfg->n_cols < 2 || cfg->n_scaf < 0 || !labels || !label_off || (cfg->n_scaf && (!names || !name_off || !table)) ||
        (cfg->cumulative && (!label_key || !offsets || !scaf_io)))
        return PG_ERR_ARG;
    for (int j = 0; j < cfg->n_sel; ++j)
        if (sel_col[j] < 2 || sel_col[j] >= cfg->n_cols) return PG_ERR_ARG;
    *geno_len_out = *snp_len_out = *n_rows_out = *n_sites_out = 0;
    *err_line_out = -1;
    *err_code_out = 0;
    EigTables T;
    T.cfg = cfg;
    T.sel_col = sel_col;
    T.prev_same = prev_same;
    T.next_same = next_same;
    T.F = pgm_fai{reinterpret_cast<const uint8_t *>(names), name_off, nullptr, table, mask, cfg->n_scaf};
    T.labels = labels;
    T.label_off = label_off;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
    const bool uni = cfg->universal_newlines != 0;
    std::vector<int64_t> ls, le, sidx;
    int64_t sites = state->sites;
    for (int64_t k = 0; k < len;) {
        const int64_t s = k;
        while (k < len && t[k] != '\n' && !(uni && t[k] == '\r')) ++k;
        ls.push_back(s);
        le.push_back(k);
        sidx.push_back(sites);
        if (!(k > s && t[s] == '#')) ++sites;
        if (k < len) k += (t[k] == '\r' && k + 1 < len && t[k + 1] == '\n') ? 2 : 1;
    }
    const int64_t n_lines = (int64_t)ls.size();
    const int nt = std::max(1, n_threads);
    const int64_t per = std::max<int64_t>(4096, (n_lines + nt - 1) / nt);
    std::vector<int64_t> cuts{0};
    while (cuts.back() < n_lines) cuts.push_back(std::min(n_lines, cuts.back() + per));
    const size_t nr = cuts.size() - 1;
    std::vector<Run> runs(nr);
    if (nr == 1) eig_lines(T, t, ls, le, sidx, 0, n_lines, &runs[0]);
    else if (nr > 1) {
        std::vector<std::thread> th;
        for (size_t r = 0; r < nr; ++r)
            th.emplace_back(eig_lines, std::cref(T), t, std::cref(ls), std::cref(le), std::cref(sidx), cuts[r], cuts[r + 1], &runs[r]);
        for (auto &x : th) x.join();
    }
    // --cumulativePos (genoToEigenstrat.py:59-68): the kept sites in file order; a scaffold change gives the chromosome left behind
    // the last written position as its offset
    pg_eig_state st = *state;
    std::vector<int64_t> off;
    std::string scaf;
    if (cfg->cumulative) {
        int32_t n_keys = 0;
        for (int32_t e = 0; e <= cfg->n_scaf; ++e) n_keys = std::max(n_keys, label_key[e] + 1);
        off.assign(offsets, offsets + n_keys);
        if (st.scaf_len >= 0) scaf.assign(scaf_io, (size_t)st.scaf_len);
        bool stopped = false;
        for (size_t r = 0; r < nr && !stopped; ++r) {
            Run &R = runs[r];
            for (const Rec &x : R.recs) {
                if (st.scaf_len < 0 || (int64_t)scaf.size() != x.scaf_len || memcmp(scaf.data(), x.scaf, (size_t)x.scaf_len) != 0) {
                    if (st.entry >= 0) off[(size_t)label_key[st.entry]] = st.pos;
                    scaf.assign(reinterpret_cast<const char *>(x.scaf), (size_t)x.scaf_len);
                    st.scaf_len = x.scaf_len;
                    st.entry = entry_of(T, x.scaf, x.scaf_len);
                }
                if (label_key[st.entry] < 0) {                    // chromOffset[chrom]: KeyError
                    R.geno.resize(x.geno_before);
                    R.rows = (int64_t)(&x - R.recs.data());
                    R.err_line = x.line;
                    R.err = PGE_E_OFFSET;
                    stopped = true;
                    break;
                }
                st.pos = x.pos + off[(size_t)label_key[st.entry]];
                snp_row(T, &R.snp, x.index, st.entry, st.pos, x.site);
            }
            if (R.err) stopped = true;
        }
    }
    int64_t gl = 0, sl = 0, rows = 0;
    size_t upto = nr;
    for (size_t r = 0; r < nr; ++r) {
        gl += (int64_t)runs[r].geno.size();
        sl += (int64_t)runs[r].snp.size();
        rows += runs[r].rows;
        if (runs[r].err) {                                  // the first line that stops the run, in input order: the rows before it stand
            *err_line_out = runs[r].err_line;
            *err_code_out = runs[r].err;
            upto = r + 1;
            break;
        }
    }
    *geno_len_out = gl;
    *snp_len_out = sl;
    *n_rows_out = rows;
    *n_sites_out = *err_code_out ? sidx[(size_t)*err_line_out] - state->sites : sites - state->sites;
    if (gl > geno_cap || sl > snp_cap) return PG_OK;        // (the caller comes back with the room; the state stands as it was)
    int64_t ga = 0, sa = 0;
    for (size_t r = 0; r < upto; ++r) {
        if (!runs[r].geno.empty()) memcpy(geno + ga, runs[r].geno.data(), runs[r].geno.size());
        if (!runs[r].snp.empty()) memcpy(snp + sa, runs[r].snp.data(), runs[r].snp.size());
        ga += (int64_t)runs[r].geno.size();
        sa += (int64_t)runs[r].snp.size();
    }
    st.sites = state->sites + *n_sites_out;
    if (cfg->cumulative) {
        std::copy(off.begin(), off.end(), offsets);
        if (st.scaf_len > 0) memcpy(scaf_io, scaf.data(), (size_t)st.scaf_len);
    }
    *state = st;
    return PG_OK;
}
