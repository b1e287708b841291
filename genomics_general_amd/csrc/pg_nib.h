// Resident row codec, shared by the device kernels and the host layer.
//
// A resident site row holds two haplotype slots per byte: byte j = code(slot 2j) | code(slot 2j+1) << 4, codes one-hot
// (A 1, C 2, G 4, T 8, 0 = missing).  The row pitch is RS = round_up(n_hap, 16) / 2 bytes (a multiple of 8), pad nibbles are 0.
// Under a diploid layout byte k is individual k's genotype, the same byte as a `.pgeno` cell.  The C-ABI keeps int8 rows (one
// byte per slot, pitch S = 2 * RS) at its boundary; the helpers below convert between the two.
//
// Every writer owns whole bytes: no two threads set the two nibbles of one byte.
#pragma once
#include <stdint.h>

#define PG_NIB_HD __host__ __device__ inline

// int8 row pitch (slots, multiple of 16) -> resident row pitch in bytes
PG_NIB_HD int pg_nib_pitch(int S) { return S >> 1; }

// slot h of a resident row
PG_NIB_HD uint32_t pg_nib_at(const uint8_t *row, int h) { return (row[h >> 1] >> (4 * (h & 1))) & 15u; }

// four slots (16 bits of a resident row) -> four int8 codes, slot k in byte k
PG_NIB_HD uint32_t pg_nib_expand4(uint32_t x) {
    const uint32_t t = (x & 0xFFu) | ((x & 0xFF00u) << 8);          // bytes: slots 0|1, 0, slots 2|3, 0
    return (t & 0x000F000Fu) | ((t << 4) & 0x0F000F00u);
}

// four int8 codes (slot k in byte k, high nibbles zero) -> 16 bits of a resident row
PG_NIB_HD uint32_t pg_nib_pack4(uint32_t w) {
    const uint32_t t = (w | (w >> 4)) & 0x00FF00FFu;                 // bytes: slots 0|1, -, slots 2|3, -
    return (t & 0xFFu) | ((t >> 8) & 0xFF00u);
}
