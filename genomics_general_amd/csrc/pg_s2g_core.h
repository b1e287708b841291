// Sequences written as `.geno` sites the way seqToGeno.py writes them: the per-byte and per-line rules of the drop-in as plain
// functions, written once and compiled twice -- by hipcc into k_s2g_lines / k_s2g_gather / k_s2g_tile (pg_s2g_dev.hip) and by the host
// compiler into pg_s2g_strip / pg_s2g_text (pg_s2g.cpp: the host route), tests/s2g_emul.cpp and tests/s2g_host_main.cpp.
//
// What they restate:
//   parseFasta: s[s.index("\n"):].replace("\n","").replace(" ","")      genomics.py:2256-2261
//   the lines: chrom \t str(x+1) \t "\t".join(cells) \n                 seqToGeno.py:71, 76, 98
//   "|".join of a group's sequences                                     genomics.py:439
// Two stages meet in the residue store: the sequences' characters side by side, feeds and blanks gone.  A line of the output is
//   name '\t' str(x + 1) '\t' body
// where the body follows one row template for every line of a segment: per byte a literal ('\t', '|', '\n') or the index of a
// haplotype, whose residue at site x stands in the store at hap_off[h] + x.  Everything in a line but the digits has one length, L0,
// so line x of a segment begins at x * L0 + (digits of 1 .. x), a closed form: an output range can be cut at any site.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define PGS_HD __host__ __device__ inline
#else
#define PGS_HD inline
#endif

#define PGS_TILE_SITES 128   // sites of one tile of k_s2g_tile
#define PGS_TILE_PITCH 132   // bytes between two haplotypes of the LDS tile: 33 words, an odd number, so that the lanes of a wave that
                             // fill one line (consecutive haplotypes, one site) meet in no bank
#define PGS_STORE 16         // bytes of one store
#define PGS_MAX_HAPS 32768   // haplotypes of a line the row template can name
#define PGS_MAX_NAME 4096    // bytes of a scaffold name

// ---- stage 1: the lines of a fasta block ----------------------------------------------------------------------------------------
// a byte the device's copy does not take: \r (the text-mode file of the reference turns it into a line feed), a '>' that is not a
// line's first byte (it splits a record), text that is not ASCII and, outside a head line, a blank (removed by the reference) or a
// tab.  `first`: the byte is its line's first; `in_head`: the line is a head line
PGS_HD bool pgs_irregular(uint8_t b, bool first, bool in_head) {
    return b == '\r' || b >= 0x80 || (b == '>' && !first) || (!in_head && (b == ' ' || b == '\t'));
}

// a head line: '>' first
PGS_HD bool pgs_is_head(const uint8_t *line, int64_t n) { return n > 0 && line[0] == '>'; }

// the residues a regular line gives: none for a head line, else every byte
PGS_HD uint32_t pgs_line_residues(const uint8_t *line, int64_t n) { return pgs_is_head(line, n) ? 0u : (uint32_t)n; }

// what the reference removes from a record's text behind its first line feed
PGS_HD bool pgs_dropped(uint8_t b) { return b == '\n' || b == ' '; }

// ---- stage 2: the lines of the output -------------------------------------------------------------------------------------------
// decimal digits of v (1 for 0)
PGS_HD int pgs_digits(uint64_t v) {
    int d = 1;
    while (v >= 10) {
        v /= 10;
        ++d;
    }
    return d;
}

PGS_HD uint64_t pgs_pow10(int d) {
    uint64_t p = 1;
    while (d-- > 0) p *= 10;
    return p;
}

// digits of 1 .. x together: (x + 1) d - (10^d - 1) / 9 with d the digits of x; modulo 2^64 (x below 10^18 fits)
PGS_HD uint64_t pgs_digit_sum(uint64_t x) {
    const int d = pgs_digits(x);
    return (x + 1) * (uint64_t)d - (pgs_pow10(d) - 1) / 9;
}

// bytes of a line without its digits: name '\t' '\t' and the template
PGS_HD uint64_t pgs_line_fixed(uint32_t name_len, uint32_t tmpl_len) { return (uint64_t)name_len + 2 + tmpl_len; }

// where line x (position x + 1) of a segment begins, counted from its line 0
PGS_HD uint64_t pgs_line_start(uint64_t x, uint64_t fixed) { return x * fixed + pgs_digit_sum(x); }

// a template entry: a literal byte, or a haplotype's index
PGS_HD int32_t pgs_lit(uint8_t b) { return -1 - (int32_t)b; }
PGS_HD bool pgs_is_lit(int32_t t) { return t < 0; }
PGS_HD uint8_t pgs_lit_byte(int32_t t) { return (uint8_t)(-1 - t); }

// byte p of a line's prefix name '\t' str(pos) '\t' (p below name_len + digits + 2)
PGS_HD uint8_t pgs_prefix_byte(const uint8_t *name, uint32_t name_len, uint64_t pos, int digits, uint32_t p) {
    if (p < name_len) return name[p];
    if (p == name_len || p == name_len + 1 + (uint32_t)digits) return '\t';
    return (uint8_t)('0' + (pos / pgs_pow10(digits - 1 - (int)(p - name_len - 1))) % 10);
}

// the bytes [a, b) of the output in stores of PGS_STORE bytes at multiples of PGS_STORE: how many stores cover them, and store k's
// part of them [*lo, *hi) -- PGS_STORE bytes: one full store; fewer: byte stores, so that nothing outside [a, b) is written
PGS_HD int64_t pgs_store_count(int64_t a, int64_t b) { return b > a ? (b - 1) / PGS_STORE - a / PGS_STORE + 1 : 0; }
PGS_HD void pgs_store_at(int64_t a, int64_t b, int64_t k, int64_t *lo, int64_t *hi) {
    const int64_t s = (a / PGS_STORE + k) * PGS_STORE;
    *lo = s < a ? a : s;
    *hi = s + PGS_STORE > b ? b : s + PGS_STORE;
}

// tile t of n items in tiles of `tile`: its first item and how many it holds (0: the tile lies behind the items)
PGS_HD int64_t pgs_tile_count(int64_t n, int64_t tile, int64_t t, int64_t *first) {
    *first = t * tile;
    if (*first >= n) return 0;
    return n - *first < tile ? n - *first : tile;
}

// haplotypes of one tile: as many as the LDS holds beside the tile's share of the template, `want` when that is fewer (0: no wish)
PGS_HD int pgs_tile_seqs(int n_haps, int want, int64_t lds_bytes) {
    int64_t tq = lds_bytes / (PGS_TILE_PITCH + 16);               // (a haplotype's row, and room for its template entries: 4 x 4 bytes)
    if (tq > n_haps) tq = n_haps;
    if (want > 0 && want < tq) tq = want;
    return tq > 0 ? (int)tq : 1;
}

// the template's share per tile of tq haplotypes: tile y writes the entries [tstart[y], tstart[y + 1]) of every line, from its first
// haplotype's entry up to the next tile's (tstart: room for the tiles + 1).  The haplotypes' indices must stand in the template once
// each, in rising order, with at most four entries a haplotype and tile: 0, or 1 + the entry that breaks the rule (tmpl_len + 1: a
// count other than n_haps)
PGS_HD int32_t pgs_tile_starts(const int32_t *tmpl, int32_t tmpl_len, int32_t n_haps, int tq, int32_t *tstart) {
    const int n_tiles = (n_haps + tq - 1) / tq;
    int32_t seen = 0;
    for (int32_t j = 0; j < tmpl_len; ++j) {
        if (pgs_is_lit(tmpl[j])) continue;
        if (tmpl[j] != seen || seen >= n_haps) return j + 1;
        if (seen % tq == 0) tstart[seen / tq] = seen ? j : 0;
        ++seen;
    }
    if (seen != n_haps) return tmpl_len + 1;
    tstart[n_tiles] = tmpl_len;
    for (int y = 0; y < n_tiles; ++y)
        if (tstart[y + 1] - tstart[y] > 4 * tq) return tstart[y] + 1;
    return 0;
}

// word w of a haplotype's tile row out of the aligned words around its store bytes: lo the word that holds byte 4 w of the row, hi
// the one behind it, shift the row's first byte within its word
PGS_HD uint32_t pgs_funnel(uint32_t lo, uint32_t hi, int shift) { return shift ? (lo >> (8 * shift)) | (hi << (32 - 8 * shift)) : lo; }
