// The device route of the mergeGeno.py drop-in walked on the host: the same pgm_* functions the kernels of
// genomics_general_amd/csrc/pg_merge_dev.hip are made of (csrc/pg_merge_core.h, compiled here by g++), with the kernels' division of the
// work restated serially: k_merge_keys = the loop over the new lines (pgm_line_key), k_merge_stop = the first line that is no site or
// does not lie behind the line before, k_merge_lines / k_merge_pos = the loops over the candidates (pgm_match_line / pgm_match_pos: the
// slots, the lengths), the scan = the running offset, k_merge_done = the lines at or below the horizon, k_merge_emit = the loop over the
// slots, every byte checked to lie inside the line's place.  The regions carry what a round leaves, as the device's do.
// tests/test_merge_emul.py puts it in the device's place inside the driver.  Test infrastructure.
#include "../genomics_general_amd/csrc/pg_merge_core.h"

#include <cstring>
#include <string>
#include <vector>

namespace {

const int64_t NONE = 0x7fffffffffffffffll;

struct EFile {
    std::vector<uint8_t> text, flag;
    std::vector<int64_t> nl, kpos;
    std::vector<int32_t> kscaf;
    std::vector<uint32_t> head;
    int64_t n_ok = 0, base_line = 0, base_byte = 0, keyed = 0, stop = NONE, irr = NONE;
    int32_t prev_scaf = -1;
    int64_t prev_pos = 0;
};

struct Emul {
    pg_merge_cfg cfg;
    uint8_t sep;
    std::string missing;
    std::vector<uint8_t> names;
    std::vector<int64_t> name_off, fai_len;
    std::vector<int32_t> table, n_cols;
    uint32_t mask;
    std::vector<EFile> f;
    std::vector<uint8_t> out;
    int64_t rounds = 0;
};

pgm_fai fai_of(const Emul &E) { return pgm_fai{E.names.data(), E.name_off.data(), E.fai_len.data(), E.table.data(), E.mask, E.cfg.n_fai}; }

void views_of(const Emul &E, pgm_view *V) {
    for (int f = 0; f < E.cfg.n_files; ++f) {
        const EFile &M = E.f[(size_t)f];
        V[f] = pgm_view{M.text.data(), M.nl.data(), M.kscaf.data(), M.kpos.data(), M.head.data(), M.base_line, M.n_ok,
                        E.n_cols[(size_t)f] > 2 ? E.n_cols[(size_t)f] - 2 : 0, E.n_cols[(size_t)f]};
    }
}

}  // namespace

extern "C" void *pgm_emul_config(const pg_merge_cfg *cfg, const char *sep, const char *missing, const char *fai_names, const int64_t *name_off,
                                 const int64_t *fai_len, const int32_t *n_cols) {
    if (cfg->sep_len != 1 || cfg->missing_len > PGM_MAX_MISSING || cfg->n_fai < 1) return nullptr;
    for (int f = 0; f < cfg->n_files; ++f)
        if (n_cols[f] < 2) return nullptr;
    Emul *E = new Emul();
    E->cfg = *cfg;
    E->sep = (uint8_t)sep[0];
    E->missing.assign(missing, (size_t)cfg->missing_len);
    E->names.assign(fai_names, fai_names + name_off[cfg->n_fai]);
    E->name_off.assign(name_off, name_off + cfg->n_fai + 1);
    E->fai_len.assign(fai_len, fai_len + cfg->n_fai);
    E->n_cols.assign(n_cols, n_cols + cfg->n_files);
    uint32_t size = 4;
    while (size < 2u * (uint32_t)cfg->n_fai) size <<= 1;
    E->table.assign(size, -1);
    E->mask = size - 1;
    for (int32_t s = 0; s < cfg->n_fai; ++s) {
        uint32_t at = pgm_hash(E->names.data() + name_off[s], name_off[s + 1] - name_off[s]) & E->mask;
        while (E->table[at] >= 0) at = (at + 1) & E->mask;
        E->table[at] = s;
    }
    E->f.resize((size_t)cfg->n_files);
    return E;
}

extern "C" void pgm_emul_free(void *e) { delete static_cast<Emul *>(e); }

// pgm_hash itself: tests/merge_edge_cases.py searches name sets with a port of it
extern "C" uint32_t pgm_emul_hash(const uint8_t *s, int64_t len) { return pgm_hash(s, len); }

// a block behind what the rounds before left of file f (take_block)
extern "C" int pgm_emul_submit(void *e, int f, const char *text, int64_t len) {
    Emul &E = *static_cast<Emul *>(e);
    EFile &M = E.f[(size_t)f];
    std::vector<uint8_t> t(M.text.begin() + M.base_byte, M.text.end());
    std::vector<int64_t> nl;
    for (size_t k = (size_t)M.base_line; k < M.nl.size(); ++k) nl.push_back(M.nl[k] - M.base_byte);
    const int64_t rem = (int64_t)t.size();
    t.insert(t.end(), text, text + len);
    for (int64_t k = 0; k < len; ++k)
        if (text[k] == '\n') nl.push_back(rem + k);
    M.text.swap(t);
    M.nl.swap(nl);
    M.base_line = M.base_byte = M.keyed = M.n_ok = 0;
    M.stop = M.irr = NONE;
    return 0;
}

extern "C" int pgm_emul_keys(void *e, int64_t *info) {
    Emul &E = *static_cast<Emul *>(e);
    const pgm_fai F = fai_of(E);
    for (int f = 0; f < E.cfg.n_files; ++f) {
        EFile &M = E.f[(size_t)f];
        const int64_t n_lines = (int64_t)M.nl.size();
        M.kscaf.resize((size_t)n_lines);
        M.kpos.resize((size_t)n_lines);
        M.head.resize((size_t)n_lines);
        M.flag.resize((size_t)n_lines);
        for (int64_t i = M.keyed; i < n_lines; ++i) {             // k_merge_keys
            const int64_t ls = i ? M.nl[(size_t)i - 1] + 1 : 0, le = M.nl[(size_t)i];
            const int why = pgm_line_key(F, M.text.data() + ls, le - ls, E.n_cols[(size_t)f], &M.kscaf[(size_t)i], &M.kpos[(size_t)i], &M.head[(size_t)i]);
            M.flag[(size_t)i] = (uint8_t)why;
            if (why == PGM_IRREGULAR && i < M.irr) M.irr = i;
        }
        for (int64_t i = M.keyed; i < n_lines; ++i) {             // k_merge_stop
            bool bad = M.flag[(size_t)i] != PGM_OK;
            if (!bad) {
                if (i == M.base_line) bad = M.prev_scaf >= 0 && !pgm_key_less(M.prev_scaf, M.prev_pos, M.kscaf[(size_t)i], M.kpos[(size_t)i]);
                else bad = M.flag[(size_t)i - 1] == PGM_OK && !pgm_key_less(M.kscaf[(size_t)i - 1], M.kpos[(size_t)i - 1], M.kscaf[(size_t)i], M.kpos[(size_t)i]);
            }
            if (bad && i < M.stop) M.stop = i;
        }
        M.keyed = n_lines;
        const int64_t stop = M.stop < n_lines ? M.stop : n_lines, len = (int64_t)M.text.size();   // k_merge_info
        const bool ragged = len > 0 && (n_lines == 0 || M.nl[(size_t)n_lines - 1] != len - 1);
        int64_t *o = info + f * 8;
        o[0] = n_lines - M.base_line;
        o[1] = stop - M.base_line;
        o[2] = stop > M.base_line ? M.kscaf[(size_t)stop - 1] : -1;
        o[3] = stop > M.base_line ? M.kpos[(size_t)stop - 1] : 0;
        o[4] = stop < n_lines ? (M.flag[(size_t)stop] ? M.flag[(size_t)stop] : PGM_STOP_ORDER) : 0;
        o[5] = stop - M.base_line;
        o[6] = ((M.irr < n_lines && M.irr <= stop) || ragged) ? 1 : 0;
        o[7] = len - M.base_byte;
        M.n_ok = stop;
    }
    return 0;
}

// 0, or -2: a byte of k_merge_emit would leave its line's place; -3: the slots are no permutation
extern "C" int pgm_emul_merge(void *e, int dense, int32_t from_scaf, int64_t from_pos, int32_t hs, int64_t hp, int64_t *done, int64_t *bytes_out,
                              int64_t *rows_out) {
    Emul &E = *static_cast<Emul *>(e);
    const pg_merge_cfg &c = E.cfg;
    const pgm_fai F = fai_of(E);
    pgm_view V[PGM_MAX_FILES];
    views_of(E, V);
    const int nc = pgm_cand_files(c);
    int64_t n_slots = 0;
    if (dense) n_slots = hp - from_pos;
    else
        for (int f = 0; f < nc; ++f) n_slots += V[f].hi - V[f].lo;
    std::vector<int64_t> len((size_t)n_slots, -1), src((size_t)n_slots, -1), off((size_t)n_slots);
    if (dense) {                                                  // k_merge_pos
        for (int64_t j = 0; j < n_slots; ++j) len[(size_t)j] = pgm_match_pos(c, V, F, hs, from_pos + 1 + j);
    } else {                                                      // k_merge_lines
        for (int f = 0; f < nc; ++f)
            for (int64_t i = V[f].lo; i < V[f].hi; ++i) {
                int64_t slot = -1;
                const int64_t n = pgm_match_line(c, V, f, i, hs, hp, &slot);
                if (slot < 0 || slot >= n_slots || len[(size_t)slot] != -1) return -3;
                len[(size_t)slot] = n;
                src[(size_t)slot] = ((int64_t)f << 56) | i;
            }
    }
    int64_t total = 0, rows = 0;                                  // the scan
    for (int64_t j = 0; j < n_slots; ++j) {
        if (len[(size_t)j] < 0) return -3;
        off[(size_t)j] = total;
        total += len[(size_t)j];
        rows += len[(size_t)j] != 0;
    }
    E.out.assign((size_t)total, 0xEE);
    for (int64_t slot = 0; slot < n_slots; ++slot) {              // k_merge_emit
        if (len[(size_t)slot] == 0) continue;
        int32_t ks = hs;
        int64_t kp = from_pos + 1 + slot;
        if (!dense) {
            const int f0 = (int)(src[(size_t)slot] >> 56);
            const int64_t i0 = src[(size_t)slot] & 0x00ffffffffffffffll;
            ks = V[f0].kscaf[i0];
            kp = V[f0].kpos[i0];
        }
        int64_t mine[PGM_MAX_FILES];
        int first = -1;
        for (int g = 0; g < c.n_files; ++g) {
            mine[g] = pgm_find(V[g], ks, kp);
            if (mine[g] >= 0 && first < 0) first = g;
        }
        uint8_t *o = E.out.data() + off[(size_t)slot];
        const int64_t room = len[(size_t)slot];
        int64_t w = 0;
        auto put = [&](int64_t at, uint8_t b) {
            if (at < 0 || at >= room) return false;
            o[at] = b;
            return true;
        };
        if (first >= 0) {
            int64_t ls, le;
            pgm_line_at(V[first], mine[first], &ls, &le);
            const int64_t hl = V[first].head[mine[first]];
            for (int64_t k = 0; k < hl; ++k) {
                const uint8_t b = V[first].text[ls + k];
                if (!put(k, b == '\t' ? E.sep : b)) return -2;
            }
            w = hl;
        } else {
            const int64_t a = F.name_off[ks], nn = F.name_off[ks + 1] - a;
            for (int64_t k = 0; k < nn; ++k)
                if (!put(k, F.names[a + k])) return -2;
            const int nd = pgm_digits(kp);
            if (!put(nn, E.sep)) return -2;
            for (int lane = 0; lane < nd; ++lane) {
                int64_t v = kp;
                for (int k = 0; k < nd - 1 - lane; ++k) v /= 10;
                if (!put(nn + 1 + lane, (uint8_t)('0' + v % 10))) return -2;
            }
            w = nn + 1 + nd;
        }
        for (int g = 0; g < c.n_files; ++g) {
            if (!(c.out_mask >> g & 1u)) continue;
            if (mine[g] >= 0) {
                int64_t ls, le;
                pgm_line_at(V[g], mine[g], &ls, &le);
                const int64_t hl = V[g].head[mine[g]], cnt = le - ls - hl;
                for (int64_t k = 0; k < cnt; ++k) {
                    const uint8_t b = V[g].text[ls + hl + k];
                    if (!put(w + k, b == '\t' ? E.sep : b)) return -2;
                }
                w += cnt;
            } else {
                const int64_t per = 1 + c.missing_len, cnt = (int64_t)V[g].n_cells * per;
                for (int64_t k = 0; k < cnt; ++k)
                    if (!put(w + k, k % per == 0 ? E.sep : (uint8_t)E.missing[(size_t)(k % per - 1)])) return -2;
                w += cnt;
            }
        }
        if (w != room - 1 || !put(w, '\n')) return -2;
    }
    for (int f = 0; f < c.n_files; ++f) {                         // k_merge_done
        EFile &M = E.f[(size_t)f];
        const int64_t end = pgm_upper_bound(V[f], hs, hp), cnt = end - V[f].lo;
        done[4 * f] = cnt;
        done[4 * f + 1] = cnt > 0 ? M.nl[(size_t)end - 1] + 1 - M.base_byte : 0;
        if (cnt > 0) {
            M.prev_scaf = M.kscaf[(size_t)end - 1];
            M.prev_pos = M.kpos[(size_t)end - 1];
            M.base_line = end;
            M.base_byte = M.nl[(size_t)end - 1] + 1;
        }
        done[4 * f + 2] = M.prev_scaf;
        done[4 * f + 3] = M.prev_pos;
    }
    *bytes_out = total;
    *rows_out = rows;
    ++E.rounds;
    return 0;
}

extern "C" void pgm_emul_rows(void *e, uint8_t *dst) {
    Emul &E = *static_cast<Emul *>(e);
    if (!E.out.empty()) memcpy(dst, E.out.data(), E.out.size());
}

extern "C" int pgm_emul_advance(void *e, const int64_t *done, const int32_t *prev_scaf, const int64_t *prev_pos) {
    Emul &E = *static_cast<Emul *>(e);
    for (int f = 0; f < E.cfg.n_files; ++f) {
        EFile &M = E.f[(size_t)f];
        if (M.base_byte + done[2 * f + 1] > (int64_t)M.text.size()) return -1;
        M.base_line += done[2 * f];
        if (M.base_line > (int64_t)M.nl.size()) M.base_line = (int64_t)M.nl.size();
        M.base_byte += done[2 * f + 1];
        M.keyed = M.n_ok = M.base_line;
        M.stop = M.irr = NONE;
        M.prev_scaf = prev_scaf[f];
        M.prev_pos = prev_pos[f];
    }
    return 0;
}

extern "C" int64_t pgm_emul_text(void *e, int f, uint8_t *dst) {
    EFile &M = static_cast<Emul *>(e)->f[(size_t)f];
    const int64_t n = (int64_t)M.text.size() - M.base_byte;
    if (dst && n) memcpy(dst, M.text.data() + M.base_byte, (size_t)n);
    return n;
}
