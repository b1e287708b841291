// Whole-wave (64 lanes) pieces that the text and statistics kernels share: scans, butterflies, lane reads, and the status word
// through which a text kernel sends a block to the host parser.  Device code only; everything inlines.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "pg_line_slot.h"

// inclusive / exclusive prefix sum over the wave's lanes
__device__ __forceinline__ int pg_wave_incl_scan(int x, int lane) {
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int y = __shfl_up(x, d, 64);
        if (lane >= d) x += y;
    }
    return x;
}
__device__ __forceinline__ int pg_wave_excl_scan(int x, int lane) { return pg_wave_incl_scan(x, lane) - x; }

// Sum over the wave, the same on every lane: an xor butterfly that steps 32, 16, ..., 1.  The ORDER is part of a float64 result
// (the statistics kernels promise bit-identical sums whatever the launch shape), so it is fixed here for every type.
template <typename T>
__device__ __forceinline__ T pg_wave_sum(T x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x += __shfl_xor(x, d, 64);
    return x;
}
__device__ __forceinline__ uint32_t pg_wave_xor(uint32_t x) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) x ^= (uint32_t)__shfl_xor((int)x, d, 64);
    return x;
}

// lane reads: pg_rl wants a lane the compiler already knows to be wave-uniform, pg_rl_any makes it so (v_readfirstlane) first
__device__ __forceinline__ uint32_t pg_rl(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ int pg_rl_any(int v, int lane) { return __builtin_amdgcn_readlane(v, __builtin_amdgcn_readfirstlane(lane)); }
__device__ __forceinline__ uint32_t pg_rfl(uint32_t v) { return (uint32_t)__builtin_amdgcn_readfirstlane((int)v); }

// the status words of a block (pg_line_slot.h): a line that needs the host parser
__device__ __forceinline__ void pg_raise_host(long long *status, long long line) {
    atomicOr(reinterpret_cast<unsigned long long *>(status + PGL_ST_BITS), (unsigned long long)PG_ST_HOST);
    atomicMin(status + PGL_ST_HOST_LINE, line);
}
