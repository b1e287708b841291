// Per-site population base counts on resident rows (one-hot nibbles, pg_nib.h): shared by pg_kernels.hip and pg_sfs.hip.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

__device__ __forceinline__ void count_dword(uint32_t v, uint32_t cnt[4]) {
    cnt[0] += __popc(v & 0x11111111u);
    cnt[1] += __popc(v & 0x22222222u);
    cnt[2] += __popc(v & 0x44444444u);
    cnt[3] += __popc(v & 0x88888888u);
}

// nibble masks of the first / last dword of the slot range [s,e) (e > s)
__device__ __forceinline__ uint32_t nib_mask_first(int s) { return ~0u << (4 * (s & 7)); }
__device__ __forceinline__ uint32_t nib_mask_last(int e) {
    const int hi = ((e - 1) & 7) + 1;
    return hi == 8 ? 0xFFFFFFFFu : ((1u << (4 * hi)) - 1u);
}

__device__ __forceinline__ void range_counts(const uint32_t *__restrict__ row, int s, int e, uint32_t cnt[4]) {
    cnt[0] = cnt[1] = cnt[2] = cnt[3] = 0u;
    if (e <= s) return;
    const int d0 = s >> 3, d1 = (e - 1) >> 3;
    const uint32_t m_first = nib_mask_first(s), m_last = nib_mask_last(e);
    if (d0 == d1) {
        count_dword(row[d0] & m_first & m_last, cnt);
        return;
    }
    count_dword(row[d0] & m_first, cnt);
    for (int d = d0 + 1; d < d1; ++d) count_dword(row[d], cnt);
    count_dword(row[d1] & m_last, cnt);
}
