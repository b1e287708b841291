// `.geno` sites written as VCF rows the way genoToVCF.py writes them: the per-site and per-cell halves of the drop-in as plain
// functions, written once and compiled twice -- by hipcc into k_gvcf_lines (pg_gvcf_dev.hip: a wavefront per line, lanes strided over
// the selected columns) and by the host compiler into pg_gvcf_text (pg_gvcf.cpp: the host route, every spelling line.split() accepts)
// and tests/gvcf_emul.cpp.
//
// What they restate:
//   makeVCFline                                        VCF_processing/genoToVCF.py:5-21
//   Genotype.__init__ / asCoded                        genomics.py:317-365   (pgf_classify of pg_filter_core.h)
//   GenomeSite.alleles(byFreq=True) / asList("coded")  genomics.py:531-557   (pgf_add / pgf_order of pg_filter_core.h)
//   the fasta's names                                  the open-addressed table of pg_merge_core.h (pgm_fai / pgm_lookup)
// The genotypes counted and written are those of the selected samples only.  Where the reference dies with a traceback these
// functions return a PGG_E_* code; the driver stops with the line.
#pragma once
#include <stdint.h>

#include "pg_filter_core.h"
#include "pg_merge_core.h"

#define PGG_HD PGF_HD

#define PGG_MAX_ALLELES 5    // the reference base in front of A C G T (or of the lone "N")
#define PGG_FIXED_LEN 9      // "\t.\t.\t.\tGT"

enum { PGG_IN_PHASED = PGF_IN_PHASED, PGG_IN_DIPLO = PGF_IN_DIPLO, PGG_IN_PAIRS = PGF_IN_ALLELES };

// why a line stops the run
enum {
    PGG_E_COLS = 1,      // fewer cells than a selected column needs, or fewer than two fields (KeyError / IndexError)
    PGG_E_DIPLO = 2,     // -f diplo: a cell outside A C G K M N S R T W Y
    PGG_E_POS = 3,       // a position int() does not take
    PGG_E_SCAF = 4,      // -r: the fasta has no such scaffold (KeyError)
    PGG_E_RANGE = 5,     // -r: the position lies beyond the scaffold's sequence (IndexError)
    PGG_E_BELOW = 6,     // -r: a position below 1 (the reference reads a base from the sequence's end: not followed)
    PGG_E_ASCII = 7,     // rejected: text that is not ASCII
    PGG_E_DIGITS = 8,    // rejected: a position of more than 18 digits
    PGG_E_CELL = 9,      // rejected: a genotype of more than PGF_MAXA alleles
};

typedef pg_gvcf_cfg PggConfig;

// the fasta on either side: the names' table and where each sequence lies in `seq` (F.len: its bases)
struct pgg_ref {
    pgm_fai F;
    const uint8_t *seq;
    const int64_t *seq_off;
};

// int(token) of ASCII text without whitespace: a sign, digits, single underscores between digits.  0 and *v, PGG_E_POS, or
// PGG_E_DIGITS (leading zeros do not count towards the 18)
PGG_HD int pgg_parse_pos(const uint8_t *s, int64_t len, int64_t *v) {
    int64_t k = 0;
    bool neg = false;
    if (k < len && (s[k] == '+' || s[k] == '-')) { neg = s[k] == '-'; ++k; }
    if (k >= len) return PGG_E_POS;
    int64_t x = 0;
    int digits = 0;
    bool prev_digit = false;
    for (; k < len; ++k) {
        if (s[k] == '_') {
            if (!prev_digit || k + 1 >= len) return PGG_E_POS;
            prev_digit = false;
            continue;
        }
        if (s[k] < '0' || s[k] > '9') return PGG_E_POS;
        prev_digit = true;
        if (digits || s[k] != '0') ++digits;
        if (digits <= PGM_MAX_DIGITS) x = x * 10 + (s[k] - '0');
    }
    if (digits > PGM_MAX_DIGITS) return PGG_E_DIGITS;
    *v = neg ? -x : x;
    return 0;
}

// the device's positions: the zeros in front of a position's last digit (str(int) drops them) ...
PGG_HD uint32_t pgg_pos_zeros(const uint8_t *s, int64_t len) {
    uint32_t z = 0;
    while ((int64_t)z + 1 < len && s[z] == '0') ++z;
    return z;
}
// ... and behind them digits only, 18 at most: the row takes them as they stand
PGG_HD bool pgg_pos_plain(const uint8_t *s, int64_t len, int64_t *v) {
    if (len < 1 || len > PGM_MAX_DIGITS) return false;
    int64_t x = 0;
    for (int64_t k = 0; k < len; ++k) {
        if (s[k] < '0' || s[k] > '9') return false;
        x = x * 10 + (s[k] - '0');
    }
    *v = x;
    return true;
}

// str(position) into o (20 bytes); returns its length
PGG_HD int pgg_pos_text(int64_t v, char *o) {
    char t[20];
    int n = 0, L = 0;
    uint64_t u = v < 0 ? (uint64_t)(-v) : (uint64_t)v;
    do { t[n++] = (char)('0' + u % 10); u /= 10; } while (u);
    if (v < 0) o[L++] = '-';
    while (n) o[L++] = t[--n];
    return L;
}

// the reference base of (scaffold index, position): 0 and *base, or PGG_E_BELOW / PGG_E_RANGE
PGG_HD int pgg_ref_base(const pgg_ref &R, int32_t scaf, int64_t pos, char *base) {
    if (pos < 1) return PGG_E_BELOW;
    if (pos > R.F.len[scaf]) return PGG_E_RANGE;
    *base = (char)R.seq[R.seq_off[scaf] + pos - 1];
    return 0;
}

// the site's alleles (genoToVCF.py:7-13): by frequency, ["N"] when there is none, the reference base moved or put in front
PGG_HD int pgg_alleles(const int32_t *counts, bool has_ref, char ref, char *al) {
    int order[4];
    const int m = pgf_order(counts, order);
    int n = 0;
    if (has_ref) al[n++] = ref;
    for (int k = 0; k < m; ++k) {
        const char b = "ACGT"[order[k]];
        if (!(has_ref && b == ref)) al[n++] = b;
    }
    if (m == 0 && !(has_ref && ref == 'N')) al[n++] = 'N';
    return n;
}

// bytes of REF \t ALT
PGG_HD int pgg_ref_alt_len(int nA) { return 2 + (nA > 1 ? 2 * (nA - 1) - 1 : 1); }

// "\t.\t" REF "\t" ALT "\t.\t.\t.\tGT" into o (3 + pgg_ref_alt_len + PGG_FIXED_LEN bytes at most: 21); returns its length
PGG_HD int pgg_middle(const char *al, int nA, char *o) {
    int L = 0;
    o[L++] = '\t'; o[L++] = '.'; o[L++] = '\t';
    o[L++] = al[0];
    o[L++] = '\t';
    if (nA > 1)
        for (int k = 1; k < nA; ++k) {
            if (k > 1) o[L++] = ',';
            o[L++] = al[k];
        }
    else
        o[L++] = '.';
    const char *fixed = "\t.\t.\t.\tGT";
    for (int k = 0; k < PGG_FIXED_LEN; ++k) o[L++] = fixed[k];
    return L;
}

// bytes of a genotype's cell: its alleles' indices, or '.', joined by the phase character
PGG_HD int pgg_cell_len(const PgfGeno &g) { return 2 * g.n - 1; }

// Genotype.asCoded over dict(zip(alleles, "0".."4")) into o (pgg_cell_len bytes)
PGG_HD int pgg_cell(const PgfGeno &g, const char *al, int nA, char *o) {
    bool ok = true;
    char code[PGF_MAXA];
    for (int k = 0; k < g.n; ++k) {
        int c = -1;
        for (int j = 0; j < nA; ++j)
            if (al[j] == g.a[k]) c = j;
        ok = ok && c >= 0;
        code[k] = (char)('0' + c);
    }
    int L = 0;
    for (int k = 0; k < g.n; ++k) {
        if (k) o[L++] = g.phase;
        o[L++] = ok ? code[k] : '.';
    }
    return L;
}

// one selected cell -> its genotype; 0 or PGG_E_*
PGG_HD int pgg_classify(const uint8_t *s, int len, int in_fmt, PgfGeno *g) {
    const int e = pgf_classify(s, len, in_fmt, -1, 0, 0, g);
    if (!e) return 0;
    for (int k = 0; k < len; ++k)
        if (s[k] >= 0x80) return PGG_E_ASCII;
    return e == PGF_E_DIPLO_IN ? PGG_E_DIPLO : PGG_E_CELL;
}
