// Biallelic `.geno` sites written as EIGENSTRAT rows the way tools/genoToEigenstrat.py writes them: the per-site and per-cell halves of
// the drop-in as plain functions, written once and compiled twice -- by hipcc into k_eig_lines (pg_eig_dev.hip: a wavefront per line,
// lanes strided over all columns to count, over the selected ones to write) and by the host compiler into pg_eig_text (pg_eig.cpp: the
// host route, every spelling line.split() accepts) and tests/eig_emul.cpp.
//
// What they restate:
//   the per-site loop                                  tools/genoToEigenstrat.py:48-73
//   Genotype.__init__ / asCount                        genomics.py:317-370   (pgf_classify of pg_filter_core.h)
//   GenomeSite.alleles / asList("count", missing=9)    genomics.py:535-557   (pgf_add / pgf_order of pg_filter_core.h)
//   int(position) / str(position)                      pgg_parse_pos / pgg_pos_zeros / pgg_pos_plain / pgg_pos_text of pg_gvcf_core.h
//   the --chromFile's scaffolds                        the open-addressed table of pg_merge_core.h (pgm_fai / pgm_lookup)
// The bases are counted over ALL samples of the file, the digits written for the selected ones.  Where the reference dies with a
// traceback these functions return a PGE_E_* code; the driver stops with the line.
#pragma once
#include <stdint.h>

#include "pg_gvcf_core.h"

#define PGE_HD PGF_HD

#define PGE_MISSING 9        // the digit of a genotype with an allele outside ACGT
#define PGE_SNP_FIXED 11     // "\t", "\t0.0\t" and "\t" a0 "\t" a1 "\n" around the index, the label and the position
#define PGE_DEV_ALLELES 9    // alleles of a cell the device takes: its count is one digit

enum { PGE_IN_PHASED = PGF_IN_PHASED, PGE_IN_DIPLO = PGF_IN_DIPLO };

// why a line stops the run (the codes pgg_classify and pgg_parse_pos return keep their numbers)
enum {
    PGE_E_COLS = PGG_E_COLS,        // a blank or one-field line (IndexError)
    PGE_E_DIPLO = PGG_E_DIPLO,      // -f diplo: a cell outside A C G K M N S R T W Y
    PGE_E_POS = PGG_E_POS,          // a position int() does not take
    PGE_E_NOCELL = 4,               // a kept site's selected sample without a cell (KeyError)
    PGE_E_OFFSET = 5,               // --cumulativePos: the scaffold's label is no key of the offsets (KeyError)
    PGE_E_ASCII = PGG_E_ASCII,      // rejected: text that is not ASCII
    PGE_E_DIGITS = PGG_E_DIGITS,    // rejected: a position of more than 18 digits
    PGE_E_CELL = PGG_E_CELL,        // rejected: a genotype of more than PGF_MAXA alleles
};

typedef pg_eig_cfg PgeConfig;

// a kept site: its two bases in alphabetical order and the one that is counted (indices into "ACGT")
struct PgeSite {
    int8_t a0, a1, counted;
};

// len(alleles) == 2 from the four base counts; the counted allele is alleles(byFreq=True)[-1]
PGE_HD bool pge_site(const int32_t *counts, PgeSite *s) {
    if (pgf_n_alleles(counts) != 2) return false;
    int order[4] = {0, 0, 0, 0};
    pgf_order(counts, order);
    s->counted = (int8_t)order[1];
    s->a0 = (int8_t)(order[0] < order[1] ? order[0] : order[1]);
    s->a1 = (int8_t)(order[0] < order[1] ? order[1] : order[0]);
    return true;
}

// Genotype.asCount(countAllele, missing=9): the genotype's alleles that are the counted base, 9 when any is not one of ACGT
PGE_HD int pge_count(const PgfGeno &g, int counted) {
    if (g.missing) return PGE_MISSING;
    int m = 0;
    for (int k = 0; k < g.n; ++k) m += pgf_base(g.a[k]) == counted;
    return m;
}

// str(count) into o (2 bytes at most); returns its length
PGE_HD int pge_count_text(int m, char *o) {
    int L = 0;
    if (m >= 10) o[L++] = (char)('0' + m / 10);
    o[L++] = (char)('0' + m % 10);
    return L;
}

PGE_HD int pge_digits(int64_t v) {
    char t[20];
    return pgg_pos_text(v, t);
}

// bytes of the .snp row: str(index) \t label \t 0.0 \t str(position) \t a0 \t a1 \n
PGE_HD uint32_t pge_snp_len(int64_t index, uint32_t label_len, uint32_t pos_len) {
    return (uint32_t)pge_digits(index) + label_len + pos_len + PGE_SNP_FIXED;
}

PGE_HD char pge_base_char(int b) { return b == 0 ? 'A' : b == 1 ? 'C' : b == 2 ? 'G' : 'T'; }

// the row's text behind the label: "\t0.0\t" ... and behind the position: "\t" a0 "\t" a1 "\n"
PGE_HD int pge_snp_tail(const PgeSite &s, char *o) {
    o[0] = '\t'; o[1] = pge_base_char(s.a0); o[2] = '\t'; o[3] = pge_base_char(s.a1); o[4] = '\n';
    return 5;
}
