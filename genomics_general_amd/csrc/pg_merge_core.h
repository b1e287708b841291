// `.geno` files joined by site the way mergeGeno.py joins them: the per-line rules of the drop-in as plain functions, written once and
// compiled twice -- by hipcc into k_merge_keys / k_merge_lines / k_merge_pos / k_merge_emit (pg_merge_dev.hip) and by the host compiler into
// pg_merge_text (pg_merge.cpp: the host route, every spelling line.split() accepts) and tests/merge_emul.cpp.
//
// What they restate (mergeGeno.py:57-88, without the walk over every position of the genome):
//   a SITE is (index of the scaffold's line in the .fai, position in 1 .. length); sites are ordered by that pair
//   a file contributes the longest prefix of its data lines whose sites are valid and strictly increasing: the first line that
//     breaks this STOPS the file (the reference's pending line never matches again)
//   which sites are written (--method, --unionMin, --mustIncludeFirst) and what a written line holds
// The device takes lines of the REGULAR spelling only: fields split by single tabs, no other ASCII whitespace, the header's number of
// fields, ASCII.  Any other line hands the round to the host route, which gives the same bytes.
#pragma once
#include <stdint.h>

#include "../../include/popgen_hip.h"

#if defined(__HIPCC__)
#define PGM_HD __host__ __device__ inline
#else
#define PGM_HD inline
#endif

#define PGM_MAX_FILES 32
#define PGM_MAX_MISSING 64          // bytes of --missing the device route takes
#define PGM_MAX_DIGITS 18           // digits of a length or a position

// why a line is not a site of its file (the flag k_merge_keys writes per line)
enum {
    PGM_OK = 0,
    PGM_IRREGULAR = 1,   // not the regular spelling: the round is the host route's
    PGM_STOP_POS = 2,    // the position is no canonical decimal (a sign, a leading zero, another character, no digit)
    PGM_STOP_RANGE = 3,  // the position lies outside 1 .. the scaffold's length
    PGM_STOP_SCAF = 4,   // the scaffold is not in the .fai
    PGM_STOP_ORDER = 5,  // the site is not behind the site of the line before
    PGM_STOP_FIELDS = 6, // fewer than two fields (a blank line)
    PGM_E_ASCII = 7,     // rejected: text that is not ASCII
    PGM_E_DIGITS = 8,    // rejected: a position of more than 18 digits
};

enum { PGM_INTERSECT = 0, PGM_UNION = 1, PGM_ALL = 2 };

// the .fai on either side: names side by side, where each begins, the lengths, and an open-addressed table over the names
struct pgm_fai {
    const uint8_t *names;
    const int64_t *name_off;   // n + 1
    const int64_t *len;        // n
    const int32_t *table;      // mask + 1 entries: a scaffold's index or -1
    uint32_t mask;
    int32_t n;
};

// the resident lines of one file: lines [lo, hi) are its sites still to be written (hi: the stopping line, or the end of the block)
struct pgm_view {
    const uint8_t *text;
    const int64_t *nl;         // where each line's line feed is
    const int32_t *kscaf;      // the key of each line
    const int64_t *kpos;
    const uint32_t *head;      // bytes of `scaffold <tab> position` of each line
    int64_t lo, hi;
    int32_t n_cells;           // header fields beyond the second: the dummy cells of a site the file does not hold
    int32_t n_cols;
};

// the characters str.split() splits an ASCII line at
PGM_HD bool pgm_is_space(uint8_t b) { return b == ' ' || (b >= '\t' && b <= '\r') || (b >= 0x1c && b <= 0x1f); }
// a byte that takes a line out of the regular spelling
PGM_HD bool pgm_irregular(uint8_t b) { return b >= 0x80 || (b != '\t' && pgm_is_space(b)); }

PGM_HD bool pgm_key_less(int32_t s1, int64_t p1, int32_t s2, int64_t p2) { return s1 < s2 || (s1 == s2 && p1 < p2); }

// str(position) == field: a canonical decimal.  PGM_OK and *v, PGM_STOP_POS, or PGM_E_DIGITS (digits only, more than 18 of them)
PGM_HD int pgm_parse_pos(const uint8_t *s, int64_t len, int64_t *v) {
    if (len < 1) return PGM_STOP_POS;
    int64_t x = 0;
    for (int64_t k = 0; k < len; ++k) {
        if (s[k] < '0' || s[k] > '9') return PGM_STOP_POS;
        if (k < PGM_MAX_DIGITS) x = x * 10 + (s[k] - '0');
    }
    if (s[0] == '0') return PGM_STOP_POS;
    if (len > PGM_MAX_DIGITS) return PGM_E_DIGITS;
    *v = x;
    return PGM_OK;
}

PGM_HD int pgm_digits(int64_t v) {
    int n = 1;
    while (v >= 10) { v /= 10; ++n; }
    return n;
}

// the hash of a scaffold name: a sum over its bytes, so that the lanes of a wave each add theirs
PGM_HD uint32_t pgm_hash_byte(uint8_t b, uint32_t k) {
    uint32_t x = ((uint32_t)b + 1u) * 0x9E3779B1u + k * 0x85EBCA6Bu;
    x ^= x >> 15;
    x *= 0x2C1B3C6Du;
    x ^= x >> 12;
    return x;
}
PGM_HD uint32_t pgm_hash_end(uint32_t sum, uint32_t len) {
    uint32_t x = sum + len * 0xC2B2AE35u;
    x ^= x >> 16;
    x *= 0x7FEB352Du;
    x ^= x >> 15;
    return x;
}
PGM_HD uint32_t pgm_hash(const uint8_t *s, int64_t len) {
    uint32_t sum = 0;
    for (int64_t k = 0; k < len; ++k) sum += pgm_hash_byte(s[k], (uint32_t)k);
    return pgm_hash_end(sum, (uint32_t)len);
}
// the scaffold's index in the .fai, -1 when it is not there: a few probes whatever the number of names
PGM_HD int32_t pgm_lookup(const pgm_fai &F, const uint8_t *s, int64_t len) {
    if (F.n == 0) return -1;
    for (uint32_t at = pgm_hash(s, len) & F.mask;; at = (at + 1) & F.mask) {
        const int32_t e = F.table[at];
        if (e < 0) return -1;
        const int64_t a = F.name_off[e], n = F.name_off[e + 1] - a;
        if (n != len) continue;
        bool same = true;
        for (int64_t k = 0; k < n && same; ++k) same = F.names[a + k] == s[k];
        if (same) return e;
    }
}

// the key of a line whose first two fields are known: PGM_OK and (*scaf, *pos), or why the line is no site
PGM_HD int pgm_key(const pgm_fai &F, const uint8_t *name, int64_t name_len, const uint8_t *num, int64_t num_len, int32_t *scaf, int64_t *pos) {
    const int32_t s = pgm_lookup(F, name, name_len);
    if (s < 0) return PGM_STOP_SCAF;
    const int rc = pgm_parse_pos(num, num_len, pos);
    if (rc != PGM_OK) return rc;
    if (*pos < 1 || *pos > F.len[s]) return PGM_STOP_RANGE;
    *scaf = s;
    return PGM_OK;
}

// One line of the regular spelling, serially (tests/merge_emul.cpp; k_merge_keys does the same with a wave): the flag, the key and
// the bytes of `scaffold <tab> position`
PGM_HD int pgm_line_key(const pgm_fai &F, const uint8_t *l, int64_t n, int n_cols, int32_t *scaf, int64_t *pos, uint32_t *head) {
    *scaf = -1;
    *pos = 0;
    *head = 0;
    if (n > 0x7fffffffll) return PGM_IRREGULAR;
    int64_t tabs = 0, t0 = -1, t1 = -1;
    bool irr = n == 0;
    for (int64_t k = 0; k < n; ++k) {
        if (pgm_irregular(l[k])) irr = true;
        if (l[k] == '\t') {
            if (k == 0 || k == n - 1 || l[k - 1] == '\t') irr = true;          // an empty field
            if (tabs == 0) t0 = k;
            if (tabs == 1) t1 = k;
            ++tabs;
        }
    }
    if (irr || tabs != n_cols - 1) return PGM_IRREGULAR;
    const int64_t e1 = n_cols > 2 ? t1 : n;
    *head = (uint32_t)e1;
    const int rc = pgm_key(F, l, t0, l + t0 + 1, e1 - t0 - 1, scaf, pos);
    if (rc == PGM_E_DIGITS) return PGM_IRREGULAR;                               // (the host route words the rejection)
    if (rc != PGM_OK) *scaf = -1;
    return rc;
}

// the first line of keys[lo .. hi) that is not below / that is above (s, p)
PGM_HD int64_t pgm_lower_bound(const pgm_view &V, int32_t s, int64_t p) {
    int64_t a = V.lo, b = V.hi;
    while (a < b) {
        const int64_t m = a + (b - a) / 2;
        if (pgm_key_less(V.kscaf[m], V.kpos[m], s, p)) a = m + 1;
        else b = m;
    }
    return a;
}
PGM_HD int64_t pgm_upper_bound(const pgm_view &V, int32_t s, int64_t p) {
    int64_t a = V.lo, b = V.hi;
    while (a < b) {
        const int64_t m = a + (b - a) / 2;
        if (pgm_key_less(s, p, V.kscaf[m], V.kpos[m])) b = m;
        else a = m + 1;
    }
    return a;
}
// the line of the file that holds the site, -1 when none does
PGM_HD int64_t pgm_find(const pgm_view &V, int32_t s, int64_t p) {
    const int64_t i = pgm_lower_bound(V, s, p);
    return i < V.hi && V.kscaf[i] == s && V.kpos[i] == p ? i : -1;
}

PGM_HD uint32_t pgm_full_mask(int n_files) { return n_files >= 32 ? 0xffffffffu : (1u << n_files) - 1u; }

// rule 3: is the site written, given the files that hold it
PGM_HD bool pgm_written(const pg_merge_cfg &c, uint32_t mask) {
    const uint32_t full = pgm_full_mask(c.n_files);
    const uint32_t first = c.must_first <= 0 ? 0u : (c.must_first >= c.n_files ? full : (1u << c.must_first) - 1u);
    if (c.method == PGM_INTERSECT && mask != full) return false;
    if ((mask & first) != first) return false;
    int r = 0;
    for (uint32_t m = mask; m; m &= m - 1) ++r;
    return c.method == PGM_ALL || (c.method == PGM_UNION && r >= c.union_min) || (c.method == PGM_INTERSECT && r == c.n_files);
}
// do sites that no file holds get written (then the candidates are the positions of the genome, not the files' lines)
PGM_HD bool pgm_dense(const pg_merge_cfg &c) { return pgm_written(c, 0u); }
// the files whose lines are the candidates otherwise: a written site is held by file 0 whenever a first file must be there
PGM_HD int pgm_cand_files(const pg_merge_cfg &c) { return c.method == PGM_INTERSECT || c.must_first >= 1 ? 1 : c.n_files; }

PGM_HD void pgm_line_at(const pgm_view &V, int64_t i, int64_t *ls, int64_t *le) {
    *ls = i ? V.nl[i - 1] + 1 : 0;
    *le = V.nl[i];
}
// what a file adds to a written line (one-byte separator): its cells behind a separator, or its dummy cells
PGM_HD int64_t pgm_part_len(const pg_merge_cfg &c, const pgm_view &V, int64_t line) {
    if (line < 0) return (int64_t)V.n_cells * (1 + c.missing_len);
    int64_t ls, le;
    pgm_line_at(V, line, &ls, &le);
    return le - ls - (int64_t)V.head[line];                       // (the tab in front of the cells becomes the separator)
}
// the length of a written line, its line feed included; line[f]: the line of file f that holds the site or -1
PGM_HD int64_t pgm_line_len(const pg_merge_cfg &c, const pgm_view *V, const int64_t *line, int64_t head_len) {
    int64_t n = head_len + 1;
    for (int f = 0; f < c.n_files; ++f)
        if (c.out_mask >> f & 1u) n += pgm_part_len(c, V[f], line[f]);
    return n;
}

// A candidate of the sparse methods: line i of file f (f below pgm_cand_files).  Its slot in the merged order of the candidate files'
// lines, and the length of the line it writes: 0 when a lower file holds the site too (that file's line writes it), when the site lies
// behind the horizon, or when rule 3 drops it
PGM_HD int64_t pgm_match_line(const pg_merge_cfg &c, const pgm_view *V, int f, int64_t i, int32_t hs, int64_t hp, int64_t *slot) {
    const int32_t s = V[f].kscaf[i];
    const int64_t p = V[f].kpos[i];
    const int nc = pgm_cand_files(c);
    int64_t at = i - V[f].lo;
    int64_t line[PGM_MAX_FILES];
    uint32_t mask = 0;
    bool owner = true;
    for (int g = 0; g < c.n_files; ++g) {
        int64_t lb = g == f ? i : pgm_lower_bound(V[g], s, p);
        const bool here = g == f || (lb < V[g].hi && V[g].kscaf[lb] == s && V[g].kpos[lb] == p);
        line[g] = here ? lb : -1;
        if (here) mask |= 1u << g;
        if (g != f && g < nc) at += (lb - V[g].lo) + (here && g < f ? 1 : 0);
        if (here && g < f) owner = false;
    }
    *slot = at;
    if (!owner || pgm_key_less(hs, hp, s, p) || !pgm_written(c, mask)) return 0;
    return pgm_line_len(c, V, line, V[f].head[i]);
}

// A candidate of the dense methods: position p of scaffold s.  The length of the line it writes (0: rule 3 drops it)
PGM_HD int64_t pgm_match_pos(const pg_merge_cfg &c, const pgm_view *V, const pgm_fai &F, int32_t s, int64_t p) {
    int64_t line[PGM_MAX_FILES];
    uint32_t mask = 0;
    int64_t head = -1;
    for (int g = 0; g < c.n_files; ++g) {
        line[g] = pgm_find(V[g], s, p);
        if (line[g] >= 0) {
            mask |= 1u << g;
            if (head < 0) head = V[g].head[line[g]];
        }
    }
    if (!pgm_written(c, mask)) return 0;
    if (head < 0) head = (F.name_off[s + 1] - F.name_off[s]) + 1 + pgm_digits(p);
    return pgm_line_len(c, V, line, head);
}

// the bytes of a written line no file's cells add to, at most: scaffold, separator, position, line feed, every file's dummy cells
PGM_HD int64_t pgm_fixed_bytes(const pg_merge_cfg &c, const int32_t *n_cells, int64_t max_name) {
    int64_t n = max_name + c.sep_len + PGM_MAX_DIGITS + 1;
    for (int f = 0; f < c.n_files; ++f)
        if (c.out_mask >> f & 1u) n += (int64_t)n_cells[f] * (c.sep_len + c.missing_len);
    return n;
}
