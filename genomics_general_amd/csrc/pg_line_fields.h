// The fields of a line of the regular spelling, for the kernels that take a wavefront per line (k_filt_lines: pg_filter_dev.hip,
// k_gvcf_lines: pg_gvcf_dev.hip, k_eig_lines: pg_eig_dev.hip): the line's tabs ranked by ballots into a table in LDS, a field read from
// that table, the line's scaffold looked up in a table over names.  Device code only; everything inlines.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pg_merge_core.h"
#include "pg_wave.h"

// the cell of field c: [s, e) within the line, from the tab table
__device__ inline void field_at(const uint32_t *tabs, int c, int n_cols, uint32_t n, uint32_t *s, uint32_t *e) {
    *s = c ? tabs[c - 1] + 1 : 0;
    *e = c < n_cols - 1 ? tabs[c] : n;
}

// the scaffold of the line (its first t0 bytes) in a table over names (the fasta's: k_gvcf_lines, the --chromFile's: k_eig_lines), -1
// when it is not there; the same on every lane
__device__ inline int32_t line_scaffold(const pgm_fai &F, const uint8_t *line, uint32_t t0, int lane) {
    uint32_t sum = 0;
    for (uint32_t k = (uint32_t)lane; k < t0; k += 64) sum += pgm_hash_byte(line[k], k);
    sum = pg_wave_sum(sum);
    for (uint32_t at = pgm_hash_end(sum, t0) & F.mask;; at = (at + 1) & F.mask) {
        const int32_t e = F.table[at];
        if (e < 0) return -1;
        const int64_t a = F.name_off[e];
        if (F.name_off[e + 1] - a != (int64_t)t0) continue;
        bool differ = false;
        for (uint32_t k = (uint32_t)lane; k < t0; k += 64) differ = differ || F.names[a + k] != line[k];
        if (__ballot(differ) == 0) return e;
    }
}

// the line's tabs into LDS; false when the line is not of the regular spelling (the host's then)
__device__ inline bool line_tabs(const uint8_t *line, uint32_t n, int n_cols, int lane, uint32_t *tabs) {
    uint32_t ntab = 0;
    bool irr = n == 0;
    for (uint32_t base = 0; base < n; base += 64) {
        const uint32_t k = base + (uint32_t)lane;
        const uint8_t b = k < n ? line[k] : (uint8_t)'x';
        const bool tab = k < n && b == '\t';
        const bool odd = k < n && (b == ' ' || b == '\v' || b == '\f' || b == '\r' || (b >= 0x1c && b <= 0x1f) || b >= 0x80);
        const uint64_t m = __ballot(tab);
        if (tab) {
            const uint32_t idx = ntab + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (idx < (uint32_t)(n_cols - 1)) tabs[idx] = k;
        }
        ntab += (uint32_t)__popcll(m);
        irr = irr || __ballot(odd) != 0;
    }
    if (irr || ntab != (uint32_t)(n_cols - 1)) return false;
    __syncthreads();
    bool empty = false;
    for (int c = lane; c < n_cols; c += 64) {
        uint32_t s, e;
        field_at(tabs, c, n_cols, n, &s, &e);
        empty = empty || e <= s;
    }
    return __ballot(empty) == 0;
}
