// `.geno` sites written as PED rows and MAP lines the way tools/genoToPlink.py writes them: the per-cell rules of the drop-in as plain
// functions, written once and compiled twice -- by hipcc into k_ped_lines / k_ped_map / k_ped_tile (pg_ped_dev.hip) and by the host
// compiler into pg_ped_text (pg_ped.cpp: the host route, every spelling line.split() accepts, cells of any length),
// tests/plink_emul.cpp and tests/plink_host_main.cpp.
//
// What they restate:
//   splitSeq (zip(*sequence), [::2] under phased)      genomics.py:390-396
//   haplo() / diploHaploDict                           genomics.py:14-27
//   the interleaving and the rows                      tools/genoToPlink.py:50, 61-72
//   int(position) / str(position)                      pgg_parse_pos / pgg_pos_zeros / pgg_pos_plain / pgg_pos_text of pg_gvcf_core.h
// zip() cuts every cell of a sample within a run to the run's shortest, m characters: pgp_alleles(fmt, m) alleles a site, a prefix of
// what any longer cell would give.  Where the reference dies with a traceback these functions return a PGP_E_* code; the driver stops
// with the line.
#pragma once
#include <stdint.h>

#include "pg_gvcf_core.h"

#define PGP_HD PGF_HD

#define PGP_TILE_LINES 128   // kept lines of one tile of k_ped_tile
#define PGP_STORE 16         // bytes of one store of k_ped_tile
#define PGP_TILE_PAD 4       // bytes behind a sample's 128 sites in the LDS tile: the pitch is an odd number of words, so that neither
                             // the lanes that write one line's cells (a sample per lane) nor the ones that read a sample's words meet
                             // in one bank
#define PGP_MAP_FIXED 5      // ' ', " 0 " and '\n' around the scaffold and the position's two copies

enum { PGP_F_PHASED = 0, PGP_F_DIPLO = 1, PGP_F_CHARS = 2 };   // CHARS: haplo, pairs, alleles

// why a line stops the run
enum {
    PGP_E_COLS = PGG_E_COLS,        // a blank or one-field line (IndexError)
    PGP_E_DIPLO = PGG_E_DIPLO,      // -f diplo: a cell outside A C G K M N S R T W Y (KeyError)
    PGP_E_POS = PGG_E_POS,          // a position int() does not take (ValueError)
    PGP_E_COUNT = 4,                // no -s: the line's cells are not the header's (the assertion of addSite)
    PGP_E_SHORT = 5,                // -s: the line ends before a selected column (KeyError)
    PGP_E_ASCII = PGG_E_ASCII,      // text that is not ASCII
    PGP_E_DIGITS = PGG_E_DIGITS,    // a position of more than 18 digits
};

typedef pg_ped_cfg PgpConfig;

// the alleles a cell cut to m characters gives: phased the characters 0, 2, 4 .. below m, diplo the letter's pair, else all m
PGP_HD int pgp_alleles(int fmt, int64_t m) {
    if (m <= 0) return 0;
    return fmt == PGP_F_PHASED ? (int)((m + 1) / 2) : fmt == PGP_F_DIPLO ? 2 : (int)m;
}

#define PGP_PAIR(a, b) ((uint32_t)(a) | ((uint32_t)(b) << 8))

// diploHaploDict: the two alleles of a letter as lo | hi << 8, 0 for a letter outside the table
PGP_HD uint32_t pgp_diplo(uint8_t b) {
    switch (b) {
    case 'A': return PGP_PAIR('A', 'A');
    case 'C': return PGP_PAIR('C', 'C');
    case 'G': return PGP_PAIR('G', 'G');
    case 'K': return PGP_PAIR('G', 'T');
    case 'M': return PGP_PAIR('A', 'C');
    case 'N': return PGP_PAIR('N', 'N');
    case 'S': return PGP_PAIR('C', 'G');
    case 'R': return PGP_PAIR('A', 'G');
    case 'T': return PGP_PAIR('T', 'T');
    case 'W': return PGP_PAIR('A', 'T');
    case 'Y': return PGP_PAIR('C', 'T');
    default: return 0;
    }
}

// allele k of a cell (k below pgp_alleles of its length)
PGP_HD uint8_t pgp_allele(const uint8_t *cell, int fmt, int k) {
    return fmt == PGP_F_PHASED ? cell[2 * k] : fmt == PGP_F_DIPLO ? (uint8_t)(pgp_diplo(cell[0]) >> (8 * k)) : cell[k];
}

// a selected cell against the format: 0, or PGP_E_DIPLO (one letter of the table is all -f diplo takes)
PGP_HD int pgp_cell_check(const uint8_t *cell, int64_t len, int fmt) {
    return fmt == PGP_F_DIPLO && (len != 1 || pgp_diplo(cell[0]) == 0) ? PGP_E_DIPLO : 0;
}

// the first `a` alleles of a cell, each followed by a blank, into o (2 a bytes)
PGP_HD void pgp_render(const uint8_t *cell, int fmt, int a, uint8_t *o) {
    for (int k = 0; k < a; ++k) {
        o[2 * k] = pgp_allele(cell, fmt, k);
        o[2 * k + 1] = ' ';
    }
}

// bytes of a .map row: scaffold ' ' str(position) " 0 " str(position) '\n'
PGP_HD uint32_t pgp_map_len(uint32_t scaf_len, uint32_t pos_len) { return scaf_len + 2 * pos_len + PGP_MAP_FIXED; }

// the device's cells: a configured length the route takes (an odd one under phased, PG_PED_DEV_ALLELES alleles at most)
PGP_HD bool pgp_dev_len(int fmt, int32_t len) {
    if (len < 1 || (fmt == PGP_F_PHASED && len % 2 == 0) || (fmt == PGP_F_DIPLO && len != 1)) return false;
    return pgp_alleles(fmt, len) <= PG_PED_DEV_ALLELES;
}

// the matrix of a block on the device: sample q's row of 2 a_q bytes a site begins at woff[q] * pitch; the pitch holds whole tiles
PGP_HD int64_t pgp_pitch(int64_t n_lines) {
    const int64_t t = (n_lines + PGP_TILE_LINES - 1) / PGP_TILE_LINES;
    return (t > 0 ? t : 1) * PGP_TILE_LINES;
}

// tile t of n items in tiles of `tile`: its first item and how many it holds (0: the tile lies behind the items)
PGP_HD int64_t pgp_tile_count(int64_t n, int64_t tile, int64_t t, int64_t *first) {
    *first = t * tile;
    if (*first >= n) return 0;
    return n - *first < tile ? n - *first : tile;
}

// bytes between two samples of the LDS tile when the widest takes wmax bytes a site
PGP_HD int64_t pgp_tile_pitch(int wmax) { return (int64_t)PGP_TILE_LINES * wmax + PGP_TILE_PAD; }

// store `seg` (PGP_STORE bytes) of a tile's sample row of `bytes` bytes: how many of its bytes belong to the row -- PGP_STORE: one
// full store; fewer: byte stores, so that nothing is written behind the row
PGP_HD int pgp_store_bytes(int64_t bytes, int seg) {
    const int64_t left = bytes - (int64_t)seg * PGP_STORE;
    return left >= PGP_STORE ? PGP_STORE : (left > 0 ? (int)left : 0);
}

// samples of one tile: as many as the LDS holds beside the four waves' tab tables (n_cols words each), `want` when that is fewer
// (0: no wish); 0: the header is too wide for the device route
PGP_HD int pgp_tile_seqs(int n_cols, int n_sel, int wmax, int want, int64_t lds_bytes) {
    const int64_t room = lds_bytes - (int64_t)n_cols * 16, p = pgp_tile_pitch(wmax);
    if (room < p) return 0;
    int64_t tq = room / p;
    if (tq > n_sel) tq = n_sel;
    if (want > 0 && want < tq) tq = want;
    return tq > 0 ? (int)tq : 1;
}
