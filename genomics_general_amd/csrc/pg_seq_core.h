// `.geno` lines turned into sequences the way genoToSeq.py turns them: the per-line and per-cell rules of the drop-in as plain functions,
// written once and compiled twice -- by hipcc into k_seq_lines / k_seq_tile (pg_seq_dev.hip) and by the host compiler into pg_seq_text
// (pg_seq.cpp: the host route, every spelling line.split() accepts), tests/seq_emul.cpp and tests/seq_host_main.cpp.
//
// What they restate:
//   parseGenoLine (split, list(GT)[::2])               genomics.py:1884-1902
//   GenoFileReader.siteBySite / nextSite ('#' lines)   genomics.py:1934-1945
//   makeAlnString's missingtrans (--NtoGap)            genomics.py:2237
// An output sequence q is one character offset of one file column: (sel_col[q], sel_off[q]); sel_len[q] is the length its cell must
// have (2 * ploidy - 1 under --splitPhased), 0 = the cell is copied whole whatever its length.  Where the reference raises, or would
// shift the sequences against each other, these functions return a PGS_E_* code; the driver stops with the line.
#pragma once
#include <stdint.h>

#include "../../include/popgen_hip.h"

#if defined(__HIPCC__)
#define PGS_HD __host__ __device__ inline
#else
#define PGS_HD inline
#endif

#define PGS_TILE_LINES 128   // kept lines of one tile of k_seq_tile: 128 bytes per sequence and tile, stored as eight 16-byte words
#define PGS_TILE_PITCH 132   // bytes between two sequences of the tile in LDS: 33 words, so that neither the lanes that write one line's
                             // characters (a sequence per lane) nor the ones that read a sequence's words meet in one bank
#define PGS_STORE 16         // bytes of one store of k_seq_tile

// why a line stops the run
enum {
    PGS_E_COLS = 1,    // blank line / fewer fields than the header (IndexError, KeyError or the assertion of addSite)
    PGS_E_MORE = 2,    // more fields than the header when every column is taken (the assertion of addSite)
    PGS_E_CELL = 3,    // --splitPhased: a selected cell is not 2 * ploidy - 1 characters long
    PGS_E_POS = 4,     // a position int() does not take, or one beyond 18 digits
    PGS_E_ASCII = 5,   // text that is not ASCII
};

// the characters str.split() splits an ASCII line at
PGS_HD bool pgs_is_space(uint8_t b) { return b == ' ' || (b >= '\t' && b <= '\r') || (b >= 0x1c && b <= 0x1f); }

// a byte that takes a line out of the regular spelling (fields split by single tabs, ASCII): the block is the host route's then
PGS_HD bool pgs_irregular(uint8_t b) { return b >= 0x80 || (b != '\t' && pgs_is_space(b)); }

// the next field of line[0 .. n) at or behind *at, as line.split() cuts it: false when none is left
PGS_HD bool pgs_next_field(const uint8_t *line, int64_t n, int64_t *at, int64_t *fs, int64_t *fe) {
    int64_t k = *at;
    while (k < n && pgs_is_space(line[k])) ++k;
    if (k >= n) { *at = k; return false; }
    *fs = k;
    while (k < n && !pgs_is_space(line[k])) ++k;
    *fe = k;
    *at = k;
    return true;
}

// a cell of `len` characters against what sequence q demands of it; the bytes it gives that sequence (0: an error)
PGS_HD int pgs_cell_width(int64_t len, int32_t want) {
    if (want == 0) return (int)len;
    return len == want ? 1 : 0;
}

// makeAlnString(NtoGap=True): N and n become -
PGS_HD uint8_t pgs_map(uint8_t b, int n_to_gap) { return n_to_gap && (b == 'N' || b == 'n') ? (uint8_t)'-' : b; }

// int(token): optional sign, digits (18 significant ones at most); 0 and *v, or PGS_E_POS
PGS_HD int pgs_parse_pos(const uint8_t *s, int64_t len, int64_t *v) {
    int64_t k = 0;
    bool neg = false;
    if (k < len && (s[k] == '+' || s[k] == '-')) { neg = s[k] == '-'; ++k; }
    if (k >= len) return PGS_E_POS;
    while (k < len - 1 && s[k] == '0') ++k;
    if (len - k > 18) return PGS_E_POS;
    int64_t x = 0;
    for (; k < len; ++k) {
        if (s[k] < '0' || s[k] > '9') return PGS_E_POS;
        x = x * 10 + (s[k] - '0');
    }
    *v = neg ? -x : x;
    return 0;
}

// the matrix of a block on the device: [n_seq][pitch] bytes, a sequence's sites side by side; the pitch holds whole tiles
PGS_HD int64_t pgs_pitch(int64_t n_lines) {
    const int64_t t = (n_lines + PGS_TILE_LINES - 1) / PGS_TILE_LINES;
    return (t > 0 ? t : 1) * PGS_TILE_LINES;
}

// tile t of n items in tiles of `tile`: its first item and how many it holds (0: the tile lies behind the items)
PGS_HD int64_t pgs_tile_count(int64_t n, int64_t tile, int64_t t, int64_t *first) {
    *first = t * tile;
    if (*first >= n) return 0;
    return n - *first < tile ? n - *first : tile;
}

// word `seg` (PGS_STORE bytes) of a tile's sequence: how many of its bytes are sites of the matrix -- PGS_STORE: one full store; fewer:
// byte stores, so that nothing is written behind the last site
PGS_HD int pgs_store_bytes(int64_t count, int seg) {
    const int64_t left = count - (int64_t)seg * PGS_STORE;
    return left >= PGS_STORE ? PGS_STORE : (left > 0 ? (int)left : 0);
}

// sequences of one tile: as many as the LDS holds beside the four waves' tab tables (n_cols words each), `want` when that is fewer
// (0: no wish); 0: the header is too wide for the device route
PGS_HD int pgs_tile_seqs(int n_cols, int n_seq, int want, int64_t lds_bytes) {
    const int64_t room = lds_bytes - (int64_t)n_cols * 16;
    if (room < PGS_TILE_PITCH) return 0;
    int64_t tq = room / PGS_TILE_PITCH;
    if (tq > n_seq) tq = n_seq;
    if (want > 0 && want < tq) tq = want;
    return tq > 0 ? (int)tq : 1;
}
