// The host route of the mergeGeno.py drop-in: one round of the join over the files' resident lines, for every spelling line.split()
// takes (runs of any ASCII whitespace between the fields, ragged lines, blank lines), for separators of any length, and under
// PG_MERGE_DEVICE=0.  The keys, the rule for written sites and the horizon are the functions the device route is made of
// (pg_merge_core.h, pg_merge_plan.h); a round of either route gives the same bytes.
#include "pg_merge_core.h"
#include "pg_merge_plan.h"

#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

int pg_fail(int code, const char *fmt, ...);

namespace {

struct Line {
    int64_t start, end;      // the line without its line feed
    int64_t next;            // where the line behind it begins
    int64_t tail;            // where its third field begins (end: none)
    pgm_site key;
};

struct File {
    std::vector<Line> lines;     // the consumable ones
    const uint8_t *text = nullptr;
};

// the line's first two fields as split() cuts them; false: fewer than two
bool two_fields(const uint8_t *l, int64_t n, int64_t f[4], int64_t *tail) {
    int64_t k = 0;
    for (int q = 0; q < 2; ++q) {
        while (k < n && pgm_is_space(l[k])) ++k;
        if (k >= n) return false;
        f[2 * q] = k;
        while (k < n && !pgm_is_space(l[k])) ++k;
        f[2 * q + 1] = k;
    }
    while (k < n && pgm_is_space(l[k])) ++k;
    *tail = k;
    return true;
}

void put_cells(std::string &out, const uint8_t *l, int64_t a, int64_t n, const std::string &sep) {
    int64_t k = a;
    while (true) {
        while (k < n && pgm_is_space(l[k])) ++k;
        if (k >= n) return;
        const int64_t s = k;
        while (k < n && !pgm_is_space(l[k])) ++k;
        out += sep;
        out.append(reinterpret_cast<const char *>(l + s), (size_t)(k - s));
    }
}

}  // namespace

extern "C" int pg_merge_text(const pg_merge_cfg *cfg, const char *sep_c, const char *missing_c, const char *fai_names, const int64_t *name_off,
                             const int64_t *fai_len, pg_merge_input *in, int64_t out_cap, pg_merge_result *res) {
    if (!cfg || !in || !res || cfg->n_files < 1 || cfg->n_files > PGM_MAX_FILES || cfg->n_fai < 0 || cfg->sep_len < 0 || cfg->missing_len < 0 ||
        (cfg->n_fai > 0 && (!fai_names || !name_off || !fai_len)) || (cfg->sep_len && !sep_c) || (cfg->missing_len && !missing_c))
        return pg_fail(PG_ERR_ARG, "pg_merge_text: bad argument");
    const int nf = cfg->n_files;
    const std::string sep(sep_c ? sep_c : "", (size_t)cfg->sep_len), missing(missing_c ? missing_c : "", (size_t)cfg->missing_len);
    res->out = nullptr;
    res->out_len = res->rows = 0;
    res->last = res->stalled = 0;
    res->err_code = 0;
    res->err_file = -1;
    res->err_line = -1;
    // the table over the .fai's names
    uint32_t size = 4;
    while (size < 2u * (uint32_t)cfg->n_fai) size <<= 1;
    std::vector<int32_t> table(size, -1);
    pgm_fai F{reinterpret_cast<const uint8_t *>(fai_names), name_off, fai_len, table.data(), size - 1, cfg->n_fai};
    int64_t max_name = 0;
    for (int32_t s = 0; s < cfg->n_fai; ++s) {
        const int64_t n = name_off[s + 1] - name_off[s];
        if (n > max_name) max_name = n;
        uint32_t at = pgm_hash(F.names + name_off[s], n) & F.mask;
        while (table[at] >= 0) at = (at + 1) & F.mask;
        table[at] = s;
    }
    // the consumable lines of every file and their keys
    std::vector<File> files((size_t)nf);
    std::vector<pgm_file_state> st((size_t)nf);
    std::vector<int32_t> n_cells((size_t)nf);
    for (int f = 0; f < nf; ++f) {
        pg_merge_input &I = in[f];
        if (I.len < 0 || (I.len && !I.text)) return pg_fail(PG_ERR_ARG, "pg_merge_text: file %d has no text", f);
        n_cells[(size_t)f] = I.n_cols > 2 ? I.n_cols - 2 : 0;
        I.stop = 0;
        I.stop_line = -1;
        I.lines_done = I.bytes_done = 0;
        File &L = files[(size_t)f];
        L.text = reinterpret_cast<const uint8_t *>(I.text);
        pgm_site prev{I.prev_scaf, I.prev_pos};
        int64_t at = 0, li = 0;
        while (at < I.len) {
            const uint8_t *l = L.text + at;
            const void *nlp = memchr(l, '\n', (size_t)(I.len - at));
            const int64_t n = nlp ? static_cast<const uint8_t *>(nlp) - l : I.len - at;
            for (int64_t k = 0; k < n; ++k)
                if (l[k] >= 0x80) {
                    res->err_code = PGM_E_ASCII;
                    res->err_file = f;
                    res->err_line = li;
                    return PG_OK;
                }
            int64_t fd[4], tail = n;
            int why = PGM_OK;
            pgm_site key{-1, 0};
            if (!two_fields(l, n, fd, &tail)) why = PGM_STOP_FIELDS;
            else why = pgm_key(F, l + fd[0], fd[1] - fd[0], l + fd[2], fd[3] - fd[2], &key.scaf, &key.pos);
            if (why == PGM_E_DIGITS) {
                res->err_code = PGM_E_DIGITS;
                res->err_file = f;
                res->err_line = li;
                return PG_OK;
            }
            if (why == PGM_OK && prev.scaf >= 0 && !(prev < key)) why = PGM_STOP_ORDER;
            if (why != PGM_OK) {
                I.stop = why;
                I.stop_line = li;
                break;
            }
            L.lines.push_back(Line{at, at + n, at + n + (nlp ? 1 : 0), at + tail, key});
            prev = key;
            at += n + (nlp ? 1 : 0);
            ++li;
        }
        st[(size_t)f].open = I.open && !I.stop;
        st[(size_t)f].has_lines = !L.lines.empty();
        st[(size_t)f].last = L.lines.empty() ? pgm_site{-1, 0} : L.lines.back().key;
    }
    const bool dense = pgm_dense(*cfg);
    const int64_t fixed = pgm_fixed_bytes(*cfg, n_cells.data(), max_name);
    const pgm_round R = pgm_plan_round(st.data(), nf, fai_len, cfg->n_fai, pgm_site{res->from_scaf, res->from_pos}, dense,
                                       pgm_max_positions(out_cap, fixed));
    res->stalled = R.stalled;
    res->last = R.last;
    if (R.stalled) {
        res->hor_scaf = res->from_scaf;
        res->hor_pos = res->from_pos;
        res->last = 0;
        return PG_OK;
    }
    res->hor_scaf = R.horizon.scaf;
    res->hor_pos = R.horizon.pos;
    // the join: every file's cursor walks its lines up to the horizon
    std::string out;
    std::vector<size_t> cur((size_t)nf, 0);
    auto live = [&](int f) { return cur[(size_t)f] < files[(size_t)f].lines.size() && !(R.horizon < files[(size_t)f].lines[cur[(size_t)f]].key); };
    auto write_site = [&](pgm_site k, uint32_t mask) {
        if (!pgm_written(*cfg, mask)) return;
        bool head = false;
        for (int f = 0; f < nf && !head; ++f)
            if (mask >> f & 1u) {
                const Line &ln = files[(size_t)f].lines[cur[(size_t)f]];
                int64_t fd[4], tail;
                two_fields(files[(size_t)f].text + ln.start, ln.end - ln.start, fd, &tail);
                out.append(reinterpret_cast<const char *>(files[(size_t)f].text + ln.start + fd[0]), (size_t)(fd[1] - fd[0]));
                out += sep;
                out.append(reinterpret_cast<const char *>(files[(size_t)f].text + ln.start + fd[2]), (size_t)(fd[3] - fd[2]));
                head = true;
            }
        if (!head) {
            out.append(fai_names + name_off[k.scaf], (size_t)(name_off[k.scaf + 1] - name_off[k.scaf]));
            out += sep;
            out += std::to_string((long long)k.pos);
        }
        for (int f = 0; f < nf; ++f) {
            if (!(cfg->out_mask >> f & 1u)) continue;
            if (mask >> f & 1u) {
                const Line &ln = files[(size_t)f].lines[cur[(size_t)f]];
                put_cells(out, files[(size_t)f].text, ln.tail, ln.end, sep);
            } else
                for (int32_t c = 0; c < n_cells[(size_t)f]; ++c) { out += sep; out += missing; }
        }
        out += '\n';
        ++res->rows;
    };
    if (dense && cfg->n_fai > 0) {
        for (int64_t p = R.from.pos + 1; p <= R.horizon.pos; ++p) {
            const pgm_site k{R.horizon.scaf, p};
            uint32_t mask = 0;
            for (int f = 0; f < nf; ++f)
                if (live(f) && files[(size_t)f].lines[cur[(size_t)f]].key == k) mask |= 1u << f;
            write_site(k, mask);
            for (int f = 0; f < nf; ++f)
                if (mask >> f & 1u) ++cur[(size_t)f];
        }
    } else {
        while (true) {
            bool any = false;
            pgm_site k{0, 0};
            for (int f = 0; f < nf; ++f)
                if (live(f) && (!any || files[(size_t)f].lines[cur[(size_t)f]].key < k)) { k = files[(size_t)f].lines[cur[(size_t)f]].key; any = true; }
            if (!any) break;
            uint32_t mask = 0;
            for (int f = 0; f < nf; ++f)
                if (live(f) && files[(size_t)f].lines[cur[(size_t)f]].key == k) mask |= 1u << f;
            write_site(k, mask);
            for (int f = 0; f < nf; ++f)
                if (mask >> f & 1u) ++cur[(size_t)f];
        }
    }
    for (int f = 0; f < nf; ++f) {
        // (a dense round leaves no line at or below its horizon behind: the keys lie behind `from`, inside the scaffolds)
        while (live(f)) ++cur[(size_t)f];
        const size_t n = cur[(size_t)f];
        in[f].lines_done = (int64_t)n;
        in[f].bytes_done = n ? files[(size_t)f].lines[n - 1].next : 0;
        if (n) {
            in[f].prev_scaf = files[(size_t)f].lines[n - 1].key.scaf;
            in[f].prev_pos = files[(size_t)f].lines[n - 1].key.pos;
        }
    }
    res->out_len = (int64_t)out.size();
    res->out = static_cast<char *>(malloc(out.size() ? out.size() : 1));
    if (!res->out) return pg_fail(PG_ERR_ARG, "pg_merge_text: out of memory");
    memcpy(res->out, out.data(), out.size());
    return PG_OK;
}

// The plan of the device route's round, from what pg_merge_dev_keys reports (info: 8 words a file) and from whether each file's input
// goes on.  round: [0] [1] where the round begins, [2] [3] its horizon, [4] stalled, [5] last, [6] dense
extern "C" int pg_merge_plan(const pg_merge_cfg *cfg, const int64_t *fai_len, const int32_t *n_cols, int64_t max_name, const int64_t *info,
                             const int32_t *open, int64_t out_cap, int32_t from_scaf, int64_t from_pos, int64_t *round) {
    if (!cfg || !n_cols || !info || !open || !round || cfg->n_files < 1 || cfg->n_files > PGM_MAX_FILES || (cfg->n_fai > 0 && !fai_len))
        return pg_fail(PG_ERR_ARG, "pg_merge_plan: bad argument");
    pgm_file_state st[PGM_MAX_FILES];
    int32_t n_cells[PGM_MAX_FILES];
    for (int f = 0; f < cfg->n_files; ++f) {
        const int64_t *o = info + f * 8;
        st[f].open = open[f] && !o[4];
        st[f].has_lines = o[1] > 0;
        st[f].last = pgm_site{(int32_t)o[2], o[3]};
        n_cells[f] = n_cols[f] > 2 ? n_cols[f] - 2 : 0;
    }
    const bool dense = pgm_dense(*cfg);
    const pgm_round R = pgm_plan_round(st, cfg->n_files, fai_len, cfg->n_fai, pgm_site{from_scaf, from_pos}, dense,
                                       pgm_max_positions(out_cap, pgm_fixed_bytes(*cfg, n_cells, max_name)));
    round[0] = R.from.scaf;
    round[1] = R.from.pos;
    round[2] = R.horizon.scaf;
    round[3] = R.horizon.pos;
    round[4] = R.stalled;
    round[5] = R.last && !R.stalled;
    round[6] = dense;
    return PG_OK;
}

extern "C" void pg_merge_free(pg_merge_result *res) {
    if (res && res->out) {
        free(res->out);
        res->out = nullptr;
    }
}
