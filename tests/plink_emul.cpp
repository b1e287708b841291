// The device route of the genoToPlink.py drop-in walked on the host: what k_ped_lines, the scans, k_ped_map and k_ped_tile
// (genomics_general_amd/csrc/pg_ped_dev.hip) do with a block -- the regular-spelling test, the selected cells against the configured
// lengths in the lanes' order, the position, the run flag against the site before, the .map row's size, the kept lines' rows and the
// rows' places, the .map rows' bytes, and the transpose tile by tile: a lane per sample expands its cell into the tile (pitch
// pgp_tile_pitch), every thread's item takes PGP_STORE bytes of one sample out of it to woff[q] x pitch -- with the very functions of
// pg_ped_core.h, compiled by g++.  tests/test_plink_emul.py puts it in the device's place inside the driver.  No GPU, no HIP.
#include "../genomics_general_amd/csrc/pg_ped_core.h"

#include <cstring>
#include <vector>

namespace {

struct Line {
    const uint8_t *p;
    uint32_t n;
    int64_t start;
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

}  // namespace

// the samples of a tile as pg_ped_dev_config computes them (64 KiB of LDS)
extern "C" int pgp_emul_tile_seqs(const pg_ped_cfg *cfg, const int32_t *sel_len, int want) {
    int wmax = 0;
    for (int q = 0; q < cfg->n_sel; ++q) {
        if (!pgp_dev_len(cfg->fmt, sel_len[q])) return 0;
        wmax = wmax > 2 * pgp_alleles(cfg->fmt, sel_len[q]) ? wmax : 2 * pgp_alleles(cfg->fmt, sel_len[q]);
    }
    return pgp_tile_seqs(cfg->n_cols, cfg->n_sel, wmax, want, 64 * 1024);
}

// 0: *n_sites sites -- the matrix in out (pitch pgp_pitch(lines), out_cap bytes), *map_len bytes in map, per site run[] and start[];
// 1: the block is the host's (*host_line its first such line); -1: map or out too small; -2: the size pass and the writing disagree
extern "C" int pgp_emul_block(const pg_ped_cfg *cfg, const int32_t *sel_col, const int32_t *sel_len, int tile_seqs, const char *text, int64_t len,
                              uint8_t *out, int64_t out_cap, uint8_t *map, int64_t map_cap, uint8_t *run, int64_t *start, int64_t *n_sites,
                              int64_t *map_len, int64_t *host_line, int64_t *pitch_out) {
    *n_sites = *map_len = *pitch_out = 0;
    *host_line = -1;
    if (len == 0) return 0;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
    if (t[len - 1] != '\n') { *host_line = 0; return 1; }
    std::vector<Line> lines;
    for (int64_t k = 0; k < len;) {
        const uint8_t *e = static_cast<const uint8_t *>(memchr(t + k, '\n', (size_t)(len - k)));
        lines.push_back(Line{t + k, (uint32_t)(e - (t + k)), k, {}});
        k = (e - t) + 1;
    }
    const int nq = cfg->n_sel;
    std::vector<int32_t> w((size_t)nq);
    std::vector<int64_t> woff((size_t)nq);
    int wmax = 0;
    int64_t wsum = 0;
    for (int q = 0; q < nq; ++q) {
        w[(size_t)q] = 2 * pgp_alleles(cfg->fmt, sel_len[q]);
        woff[(size_t)q] = wsum;
        wsum += w[(size_t)q];
        wmax = wmax > w[(size_t)q] ? wmax : w[(size_t)q];
    }
    // k_ped_lines
    std::vector<uint32_t> keep(lines.size()), rlen(lines.size());
    std::vector<uint8_t> runf(lines.size());
    int64_t prev = -1;                                                 // the site before
    for (size_t i = 0; i < lines.size(); ++i) {
        Line &L = lines[i];
        if (L.n > 0 && L.p[0] == '#') { keep[i] = 0; rlen[i] = 0; continue; }
        bool host = !regular(L, cfg->n_cols);
        for (int lane = 0; lane < 64 && !host; ++lane)
            for (int q = lane; q < nq; q += 64) {
                uint32_t s, e;
                field(L, sel_col[q], cfg->n_cols, &s, &e);
                if (e - s != (uint32_t)sel_len[q] || pgp_cell_check(L.p + s, (int64_t)(e - s), cfg->fmt)) host = true;
            }
        if (!host) {
            const uint32_t f0e = L.tabs[0], f1e = L.tabs[1];
            int64_t pos = 0;
            const uint32_t pz = pgg_pos_zeros(L.p + f0e + 1, (int64_t)f1e - f0e - 1);
            host = !pgg_pos_plain(L.p + f0e + 1 + pz, (int64_t)f1e - f0e - 1 - pz, &pos);
            rlen[i] = pgp_map_len(f0e, f1e - f0e - 1 - pz);
            runf[i] = 1;
            if (prev >= 0 && lines[(size_t)prev].n > f0e)
                runf[i] = !(memcmp(lines[(size_t)prev].p, L.p, f0e) == 0 && lines[(size_t)prev].p[f0e] == '\t');
        }
        if (host) { *host_line = (int64_t)i; return 1; }
        keep[i] = 1;
        prev = (int64_t)i;
    }
    // the scans, k_ped_map
    const int64_t pitch = pgp_pitch((int64_t)lines.size());
    *pitch_out = pitch;
    std::vector<int64_t> line_of;
    int64_t total = 0;
    for (size_t i = 0; i < lines.size(); ++i) {
        if (!keep[i]) continue;
        const Line &L = lines[i];
        if (total + rlen[i] > map_cap) return -1;
        run[line_of.size()] = runf[i];
        start[line_of.size()] = L.start;
        line_of.push_back((int64_t)i);
        const uint32_t f0e = L.tabs[0], pz = pgg_pos_zeros(L.p + f0e + 1, (int64_t)L.tabs[1] - f0e - 1), ps = f0e + 1 + pz, pl = L.tabs[1] - ps;
        uint8_t *o = map + total;
        memcpy(o, L.p, f0e);
        o += f0e;
        *o++ = ' ';
        memcpy(o, L.p + ps, pl);
        o += pl;
        memcpy(o, " 0 ", 3);
        o += 3;
        memcpy(o, L.p + ps, pl);
        o += pl;
        *o++ = '\n';
        if (o - (map + total) != (int64_t)rlen[i]) return -2;
        total += rlen[i];
    }
    const int64_t ns_all = (int64_t)line_of.size();
    if (wsum * pitch > out_cap) return -1;
    // k_ped_tile
    const int64_t tp = pgp_tile_pitch(wmax);
    std::vector<uint8_t> tile((size_t)(tile_seqs * tp));
    const int segs = PGP_TILE_LINES * wmax / PGP_STORE;
    for (int64_t bx = 0; bx < pitch / PGP_TILE_LINES; ++bx)
        for (int64_t by = 0; by < (nq + tile_seqs - 1) / tile_seqs; ++by) {
            int64_t site0, q0;
            const int ns = (int)pgp_tile_count(ns_all, PGP_TILE_LINES, bx, &site0), nt = (int)pgp_tile_count(nq, tile_seqs, by, &q0);
            if (ns == 0 || nt == 0) continue;
            memset(tile.data(), 0xee, tile.size());
            for (int l = 0; l < ns; ++l) {
                const Line &L = lines[(size_t)line_of[(size_t)(site0 + l)]];
                for (int qq = 0; qq < nt; ++qq) {
                    const int q = (int)q0 + qq;
                    pgp_render(L.p + L.tabs[(size_t)sel_col[q] - 1] + 1, cfg->fmt, w[(size_t)q] / 2, tile.data() + qq * tp + (int64_t)l * w[(size_t)q]);
                }
            }
            for (int item = 0; item < nt * segs; ++item) {
                const int qq = item / segs, seg = item % segs, q = (int)q0 + qq;
                const int nb = pgp_store_bytes((int64_t)ns * w[(size_t)q], seg);
                if (nb == 0) continue;
                const int64_t at = woff[(size_t)q] * pitch + site0 * w[(size_t)q] + (int64_t)seg * PGP_STORE;
                if (at + nb > out_cap) return -1;
                memcpy(out + at, tile.data() + qq * tp + (int64_t)seg * PGP_STORE, (size_t)nb);
            }
        }
    *n_sites = ns_all;
    *map_len = total;
    return 0;
}
