// The device route of the genoToSeq.py drop-in walked on the host: the same pgs_* functions the kernels of
// genomics_general_amd/csrc/pg_seq_dev.hip are made of (csrc/pg_seq_core.h, compiled here by g++), with the kernels' division of the work
// restated serially: k_seq_lines = the loop over lines ('#' lines, the tab table, field count, the selected cells' lengths, position, run
// flag), the scan = the running row, k_seq_rows = the sites' records, k_seq_tile = the loops over site tiles and sequence tiles, the
// tile in "LDS" with its pitch, the 16-byte words of the store phase with the edge arithmetic.  tests/test_seq_emul.py puts it in the
// device's place inside the driver and holds the output against the goldens and the host route.  Test infrastructure.
#include "../genomics_general_amd/csrc/pg_seq_core.h"

#include <algorithm>
#include <cstring>
#include <vector>

namespace {

// the line's tab table (k_seq_lines: seq_line_tabs); false: not the regular spelling
bool line_tabs(const uint8_t *l, uint32_t n, int n_cols, std::vector<uint32_t> &tabs) {
    tabs.clear();
    if (n == 0) return false;
    for (uint32_t k = 0; k < n; ++k) {
        if (pgs_irregular(l[k])) return false;
        if (l[k] == '\t') tabs.push_back(k);
    }
    if ((int)tabs.size() != n_cols - 1) return false;
    for (int c = 0; c < n_cols; ++c) {
        const uint32_t s = c ? tabs[(size_t)c - 1] + 1 : 0, e = c < n_cols - 1 ? tabs[(size_t)c] : n;
        if (e <= s) return false;
    }
    return true;
}

}  // namespace

// One block of whole lines (the last byte a line feed).  0: the matrix out[n_seq][pitch] (pitch = pgs_pitch(lines), the caller's
// buffer holds n_seq * pitch bytes and keeps what it held wherever no site is written), *n_sites, pos / run / start per site; 1:
// *host_line is the first line the device does not take; -1: bad arguments; -2: a store of the tile phase would leave the matrix
extern "C" int pgs_emul_block(const pg_seq_cfg *cfg, const int32_t *sel_col, const int32_t *sel_off, const int32_t *sel_len, int tile_seqs,
                              const char *text_c, int64_t len, uint8_t *out, int64_t pitch, int64_t *pos_out, uint8_t *run_out,
                              int64_t *start_out, int64_t *n_sites, int64_t *host_line) {
    const uint8_t *text = reinterpret_cast<const uint8_t *>(text_c);
    if (len <= 0 || text[len - 1] != '\n') return -1;
    std::vector<int64_t> nl;
    for (int64_t k = 0; k < len; ++k)
        if (text[k] == '\n') nl.push_back(k);
    const int64_t n_lines = (int64_t)nl.size();
    if (pitch != pgs_pitch(n_lines)) return -1;
    const int tq = pgs_tile_seqs(cfg->n_cols, cfg->n_seq, tile_seqs, 64 * 1024);
    if (tq == 0) return -1;
    auto line_at = [&](int64_t i, int64_t *ls, int64_t *le) { *ls = i ? nl[(size_t)i - 1] + 1 : 0; *le = nl[(size_t)i]; };

    // k_seq_lines
    std::vector<uint32_t> keep((size_t)n_lines), tabs;
    std::vector<uint8_t> runf((size_t)n_lines);
    std::vector<int64_t> pos((size_t)n_lines);
    int64_t first_host = -1;
    for (int64_t i = 0; i < n_lines; ++i) {
        int64_t ls, le;
        line_at(i, &ls, &le);
        const uint8_t *line = text + ls;
        if (le > ls && line[0] == '#') { keep[(size_t)i] = 0; continue; }
        const uint32_t n = (uint32_t)(le - ls);
        bool host = !line_tabs(line, n, cfg->n_cols, tabs);
        for (int q = 0; !host && q < cfg->n_seq; ++q) {
            const int c = sel_col[q];
            const uint32_t s = tabs[(size_t)c - 1] + 1, e = c < cfg->n_cols - 1 ? tabs[(size_t)c] : n;
            host = pgs_cell_width(e - s, cfg->split ? sel_len[q] : 1) != 1;
        }
        uint8_t run = 1;
        if (!host) {
            const uint32_t f0e = tabs[0], f1s = tabs[0] + 1, f1e = cfg->n_cols > 2 ? tabs[1] : n;
            host = pgs_parse_pos(line + f1s, (int64_t)(f1e - f1s), &pos[(size_t)i]) != 0;
            int64_t j = i - 1, ps = 0, pe = 0;
            for (; j >= 0; --j) {
                line_at(j, &ps, &pe);
                if (!(pe > ps && text[ps] == '#')) break;
            }
            if (j >= 0 && pe - ps > (int64_t)f0e) {
                bool differ = false;
                for (uint32_t k = 0; k <= f0e; ++k) differ = differ || (k < f0e ? text[ps + k] != line[k] : text[ps + k] != '\t');
                run = differ;
            }
        }
        keep[(size_t)i] = host ? 0 : 1;
        runf[(size_t)i] = run;
        if (host && first_host < 0) first_host = i;
    }
    if (first_host >= 0) {
        *host_line = first_host;
        return 1;
    }
    // the scan and k_seq_rows
    std::vector<int64_t> line_of;
    for (int64_t i = 0; i < n_lines; ++i)
        if (keep[(size_t)i]) {
            const int64_t r = (int64_t)line_of.size();
            line_of.push_back(i);
            pos_out[r] = pos[(size_t)i];
            run_out[r] = runf[(size_t)i];
            start_out[r] = i ? nl[(size_t)i - 1] + 1 : 0;
        }
    const int64_t n_rows = (int64_t)line_of.size();
    *n_sites = n_rows;
    // k_seq_tile: the grid is laid over the LINES (the host does not know the sites' number when it launches), tiles behind the sites leave
    std::vector<uint8_t> tile((size_t)tq * PGS_TILE_PITCH);
    const int64_t tiles = pitch / PGS_TILE_LINES, qtiles = (cfg->n_seq + tq - 1) / tq;
    for (int64_t bx = 0; bx < tiles; ++bx)
        for (int64_t by = 0; by < qtiles; ++by) {
            int64_t site0, q0;
            const int ns = (int)pgs_tile_count(n_rows, PGS_TILE_LINES, bx, &site0);
            const int nq = (int)pgs_tile_count(cfg->n_seq, tq, by, &q0);
            if (ns == 0 || nq == 0) continue;
            std::fill(tile.begin(), tile.end(), (uint8_t)0xA5);
            for (int it = 0; it < PGS_TILE_LINES / 4; ++it)
                for (int wave = 0; wave < 4; ++wave) {
                    const int l = it * 4 + wave;
                    if (l >= ns) continue;
                    int64_t ls, le;
                    line_at(line_of[(size_t)(site0 + l)], &ls, &le);
                    const uint8_t *line = text + ls;
                    tabs.clear();
                    for (int64_t k = 0; k < le - ls; ++k)
                        if (line[k] == '\t') tabs.push_back((uint32_t)k);
                    for (int qq = 0; qq < nq; ++qq) {
                        const int q = (int)q0 + qq;
                        const int64_t at = (int64_t)tabs[(size_t)sel_col[q] - 1] + 1 + sel_off[q];
                        if (at >= le - ls) return -2;
                        tile[(size_t)qq * PGS_TILE_PITCH + (size_t)l] = pgs_map(line[at], cfg->n_to_gap);
                    }
                }
            const int segs = PGS_TILE_LINES / PGS_STORE;
            for (int item = 0; item < nq * segs; ++item) {
                const int qq = item / segs, seg = item % segs;
                const int nb = pgs_store_bytes(ns, seg);
                if (nb == 0) continue;
                const int64_t at = (q0 + qq) * pitch + site0 + (int64_t)seg * PGS_STORE;
                // nothing outside [n_seq][n_sites]
                if (q0 + qq >= cfg->n_seq || site0 + (int64_t)seg * PGS_STORE + nb > n_rows || at % PGS_STORE) return -2;
                memcpy(out + at, tile.data() + (size_t)qq * PGS_TILE_PITCH + (size_t)seg * PGS_STORE, (size_t)nb);
            }
        }
    return 0;
}
