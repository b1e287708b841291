// The host route of the genoToPlink.py drop-in (pg_ped_text): every spelling the reference's `line.split(None, 2)` / `split()` takes,
// cells of any length, the blocks the device route hands back, and PG_PED_DEVICE=0.  Lines end at \n (the driver turns a text-mode
// file's \r\n and \r into \n first), fields at runs of ASCII whitespace.  The lines are split over host threads and walked twice with
// the functions of pg_ped_core.h: the first walk checks the lines, cuts the block into runs of one scaffold and finds, per run and
// sample, the shortest cell; the second writes every cell's alleles at its place in the sample's bytes -- as many as the run's
// shortest cell gives -- and the .map rows.  No GPU context is needed, and nothing but the C++ library: tests/plink_host_main.cpp
// compiles this file on its own.
#include "pg_ped_core.h"

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <thread>
#include <vector>

namespace {

struct Field {
    const uint8_t *p;
    int64_t len;
};

// a stretch of sites of one scaffold within a thread's share of the lines
struct Piece {
    int64_t n = 0, name_off = 0, name_len = 0;
    int64_t run = 0, before = 0;                 // the block's run it belongs to, the run's sites in front of it
    std::vector<int32_t> min;                    // per sample: the shortest cell
};

struct Share {
    std::vector<Piece> pieces;
    int64_t n_sites = 0, map_bytes = 0, map_at = 0;
    int64_t err_line = -1;
    int err = 0;
};

struct Lines {
    const PgpConfig *cfg;
    const int32_t *sel_col;
    const uint8_t *text;
    std::vector<int64_t> ls, le;
};

// the fields of a line; false: text that is not ASCII
bool split(const uint8_t *p, int64_t n, std::vector<Field> *f) {
    f->clear();
    for (int64_t k = 0; k < n; ++k)
        if (p[k] >= 0x80) return false;
    for (int64_t k = 0; k < n;) {
        while (k < n && pgm_is_space(p[k])) ++k;
        if (k >= n) break;
        const int64_t s = k;
        while (k < n && !pgm_is_space(p[k])) ++k;
        f->push_back(Field{p + s, k - s});
    }
    return true;
}

// the first walk over lines [a, b)
void check_lines(const Lines &L, int64_t a, int64_t b, Share *S) {
    const PgpConfig &cfg = *L.cfg;
    const int64_t n_names = cfg.n_cols - 2;
    std::vector<Field> f;
    char num[24];
    for (int64_t i = a; i < b; ++i) {
        const uint8_t *p = L.text + L.ls[(size_t)i];
        const int64_t n = L.le[(size_t)i] - L.ls[(size_t)i];
        if (n > 0 && p[0] == '#') continue;                                // genomics.py:1943
        auto fail = [&](int code) { S->err_line = i; S->err = code; };
        if (!split(p, n, &f)) { fail(PGP_E_ASCII); return; }
        if (f.size() < 2) { fail(PGP_E_COLS); return; }                    // lineData[-1] / lineData[posCol] (IndexError)
        int64_t pos = 0;
        const int e = pgg_parse_pos(f[1].p, f[1].len, &pos);
        if (e) { fail(e); return; }
        // the cells: what follows the second field -- of a line of two fields the second itself (lineData[-1])
        const int64_t c0 = f.size() == 2 ? 1 : 2, n_cells = (int64_t)f.size() - c0;
        if (cfg.exact_cols && n_cells != n_names) { fail(PGP_E_COUNT); return; }
        if (S->pieces.empty() || S->pieces.back().name_len != f[0].len ||
            memcmp(L.text + S->pieces.back().name_off, f[0].p, (size_t)f[0].len) != 0) {
            S->pieces.emplace_back();
            Piece &P = S->pieces.back();
            P.name_off = f[0].p - L.text;
            P.name_len = f[0].len;
            P.min.assign((size_t)cfg.n_sel, 0x7fffffff);
        }
        Piece &P = S->pieces.back();
        for (int j = 0; j < cfg.n_sel; ++j) {
            const int64_t c = L.sel_col[j] - 2;
            if (c >= n_cells) { fail(PGP_E_SHORT); return; }               // siteData["GTs"][name] (KeyError)
            const Field &x = f[(size_t)(c0 + c)];
            if (pgp_cell_check(x.p, x.len, cfg.fmt)) { fail(PGP_E_DIPLO); return; }
            P.min[(size_t)j] = (int32_t)std::min<int64_t>(P.min[(size_t)j], x.len);
        }
        ++P.n;
        ++S->n_sites;
        S->map_bytes += pgp_map_len((uint32_t)f[0].len, (uint32_t)pgg_pos_text(pos, num));
    }
}

// the second walk: every selected cell's alleles and the .map rows at their places
void write_lines(const Lines &L, int64_t a, int64_t b, const Share *S, const pg_ped_block *B, const std::vector<int64_t> *base,
                 const std::vector<int32_t> *wid) {
    const PgpConfig &cfg = *L.cfg;
    std::vector<Field> f;
    char num[24];
    size_t piece = 0;
    int64_t in_piece = 0;
    uint8_t *m = B->map + S->map_at;
    for (int64_t i = a; i < b && piece < S->pieces.size(); ++i) {
        const uint8_t *p = L.text + L.ls[(size_t)i];
        const int64_t n = L.le[(size_t)i] - L.ls[(size_t)i];
        if (n > 0 && p[0] == '#') continue;
        split(p, n, &f);
        const Piece &P = S->pieces[piece];
        const int64_t c0 = f.size() == 2 ? 1 : 2, at = P.before + in_piece;
        for (int j = 0; j < cfg.n_sel; ++j) {
            const size_t rj = (size_t)P.run * (size_t)cfg.n_sel + (size_t)j;
            const int32_t w = (*wid)[rj];
            pgp_render(f[(size_t)(c0 + L.sel_col[j] - 2)].p, cfg.fmt, w / 2, B->seq + B->seq_off[j] + (*base)[rj] + at * w);
        }
        int64_t pos = 0;
        pgg_parse_pos(f[1].p, f[1].len, &pos);
        const int nd = pgg_pos_text(pos, num);
        memcpy(m, f[0].p, (size_t)f[0].len);
        m += f[0].len;
        *m++ = ' ';
        memcpy(m, num, (size_t)nd);
        m += nd;
        memcpy(m, " 0 ", 3);
        m += 3;
        memcpy(m, num, (size_t)nd);
        m += nd;
        *m++ = '\n';
        if (++in_piece == P.n) {
            ++piece;
            in_piece = 0;
        }
    }
}

template <typename T>
T *take(size_t n) {
    return static_cast<T *>(malloc(std::max<size_t>(n, 1) * sizeof(T)));
}

}  // namespace

extern "C" void pg_ped_free(pg_ped_block *B) {
    if (!B) return;
    free(B->seq); free(B->seq_off); free(B->run_start); free(B->run_name); free(B->run_min); free(B->map);
    B->seq = B->map = nullptr;
    B->seq_off = B->run_start = B->run_name = nullptr;
    B->run_min = nullptr;
}

extern "C" int pg_ped_text(const pg_ped_cfg *cfg, const int32_t *sel_col, const char *text, int64_t len, int n_threads, pg_ped_block *B) {
    if (!cfg || !B || (len && !text) || len < 0 || cfg->n_sel < 1 || !sel_col || cfg->n_cols < 3 || cfg->fmt < PGP_F_PHASED || cfg->fmt > PGP_F_CHARS)
        return PG_ERR_ARG;
    for (int j = 0; j < cfg->n_sel; ++j)
        if (sel_col[j] < 2 || sel_col[j] >= cfg->n_cols) return PG_ERR_ARG;
    memset(B, 0, sizeof *B);
    B->err_line = -1;
    Lines L;
    L.cfg = cfg;
    L.sel_col = sel_col;
    L.text = reinterpret_cast<const uint8_t *>(text);
    for (int64_t k = 0; k < len;) {
        const void *e = memchr(L.text + k, '\n', (size_t)(len - k));
        const int64_t end = e ? static_cast<const uint8_t *>(e) - L.text : len;
        L.ls.push_back(k);
        L.le.push_back(end);
        k = end + 1;
    }
    const int64_t n_lines = (int64_t)L.ls.size();
    const int nt = std::max(1, n_threads);
    const int64_t per = std::max<int64_t>(2048, (n_lines + nt - 1) / nt);
    std::vector<int64_t> cuts{0};
    while (cuts.back() < n_lines) cuts.push_back(std::min(n_lines, cuts.back() + per));
    const size_t ns = cuts.size() - 1;
    std::vector<Share> shares(ns);
    auto spread = [&](auto fn) {
        if (ns == 1) fn(0);
        else if (ns > 1) {
            std::vector<std::thread> th;
            for (size_t s = 0; s < ns; ++s) th.emplace_back(fn, s);
            for (auto &x : th) x.join();
        }
    };
    spread([&](size_t s) { check_lines(L, cuts[s], cuts[s + 1], &shares[s]); });
    for (const Share &S : shares)
        if (S.err) {                                             // the first line that stops the run, in input order
            B->err_line = S.err_line;
            B->err_code = S.err;
            return PG_OK;
        }
    // the block's runs: a share's first piece goes on with the run in front of it when the scaffold is the same
    std::vector<const Piece *> first;                            // a run's first piece
    std::vector<int64_t> run_n;
    for (Share &S : shares) {
        S.map_at = B->map_bytes;
        B->map_bytes += S.map_bytes;
        B->n_sites += S.n_sites;
        for (size_t k = 0; k < S.pieces.size(); ++k) {
            Piece &P = S.pieces[k];
            const bool on = k == 0 && !first.empty() && first.back()->name_len == P.name_len &&
                            memcmp(L.text + first.back()->name_off, L.text + P.name_off, (size_t)P.name_len) == 0;
            if (!on) {
                first.push_back(&P);
                run_n.push_back(0);
            }
            P.run = (int64_t)first.size() - 1;
            P.before = run_n.back();
            run_n.back() += P.n;
        }
    }
    const size_t nr = first.size(), nq = (size_t)cfg->n_sel;
    B->n_runs = (int64_t)nr;
    B->seq_off = take<int64_t>(nq + 1);
    B->run_start = take<int64_t>(nr);
    B->run_name = take<int64_t>(2 * nr);
    B->run_min = take<int32_t>(nr * nq);
    B->map = take<uint8_t>((size_t)B->map_bytes);
    if (!B->seq_off || !B->run_start || !B->run_name || !B->run_min || !B->map) {
        pg_ped_free(B);
        return PG_ERR_STATE;
    }
    for (size_t k = 0; k < nr * nq; ++k) B->run_min[k] = 0x7fffffff;
    for (const Share &S : shares)
        for (const Piece &P : S.pieces)
            for (size_t j = 0; j < nq; ++j) B->run_min[(size_t)P.run * nq + j] = std::min(B->run_min[(size_t)P.run * nq + j], P.min[j]);
    int64_t at = 0;
    for (size_t r = 0; r < nr; ++r) {
        B->run_start[r] = at;
        B->run_name[2 * r] = first[r]->name_off;
        B->run_name[2 * r + 1] = first[r]->name_len;
        at += run_n[r];
    }
    std::vector<int64_t> base(std::max<size_t>(nr * nq, 1));     // where a run's sites begin within its sample's bytes
    std::vector<int32_t> wid(std::max<size_t>(nr * nq, 1));      // bytes a site of the run takes there
    int64_t total = 0;
    for (size_t j = 0; j < nq; ++j) {
        B->seq_off[j] = total;
        int64_t mine = 0;
        for (size_t r = 0; r < nr; ++r) {
            wid[r * nq + j] = 2 * pgp_alleles(cfg->fmt, B->run_min[r * nq + j]);
            base[r * nq + j] = mine;
            mine += run_n[r] * wid[r * nq + j];
        }
        total += mine;
    }
    B->seq_off[nq] = B->seq_bytes = total;
    B->seq = take<uint8_t>((size_t)total);
    if (!B->seq) {
        pg_ped_free(B);
        return PG_ERR_STATE;
    }
    spread([&](size_t s) { write_lines(L, cuts[s], cuts[s + 1], &shares[s], B, &base, &wid); });
    return PG_OK;
}
