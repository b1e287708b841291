// What the pair-count kernels share (k_pack3's fused form, k_pairC_big, k_pairC_tile, k_pairC_fp4 / k_pairD_fp4, k_pairC / k_pairD):
// how blocks are dealt to windows, how a 32 x 32 accumulator tile reaches the window's matrix, and the launchers' part rules.
// The dealing is plain C++ (PG_HD), so that a CPU program can walk it (tests/pair_deal_main.cpp); the rest needs hipcc.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define PG_HD __host__ __device__ __forceinline__
#else
#define PG_HD inline
#endif

// XCD-aware 1-D grid: block b runs on XCD b % 8.  All `per_win` blocks of a window go to one XCD, so that the window's planes are
// served by that XCD's L2: in rows of 8 windows, window 8 * row + xcd runs on XCD xcd.  The last n_win % 8 windows (all of them
// when a job has fewer than 8, e.g. a whole-genome distMat) cannot fill a row: their blocks are dealt to the 8 XCDs in equal
// contiguous runs, so that no XCD idles and neighbouring blocks still share an L2.  block -> (window, rest in 0 .. per_win - 1);
// false for the surplus blocks at the end of the grid (block-uniform).
PG_HD bool pg_deal_window(unsigned block, int per_win, int n_win, int &win, int &rem) {
    const int xcd = block & 7;
    const int v = block >> 3;
    const int full = n_win >> 3;
    if (v < full * per_win) {
        win = (v / per_win) * 8 + xcd;
        rem = v % per_win;
        return true;
    }
    const int total = (n_win & 7) * per_win, q = (total + 7) >> 3;
    const int vt = v - full * per_win, lin = xcd * q + vt;
    if (vt >= q || lin >= total) return false;
    win = full * 8 + lin / per_win;
    rem = lin % per_win;
    return true;
}

// the grid that pg_deal_window expects
inline int64_t pg_deal_blocks(int n_win, int64_t per_win) { return (int64_t)((n_win + 7) / 8) * per_win * 8; }

// The rows of every eighth word (32 sites) of a window part, as the waves of k_pack3's fused form read them: each word behind a
// buffer descriptor of its own, base = the word's first row, records = the bytes of its rows inside the part.  A part may be longer
// than 32-bit offsets reach, so the base stays in 64 bits and only offsets inside a word go through the descriptor's range check.
// From one word of a wave to its next the base moves by 8 * 32 rows (an add with carry) and the rows left shrink by 256; a word
// past the part, or past the window's end inside the part's last word, has its rows clipped to 0 .. 32, and zero records read as zero
// whatever the base.  Plain C++, so that a CPU program can walk it (tests/word_walk_main.cpp).
struct PgWordWalk {
    uint64_t base;                           // address of the word's first row
    int left;                                // rows from there to the end of the part (or of the window); may be negative

    // word w0 of the window [lo, hi) of rows of RS bytes at `rows`; the part ends before word w_end
    PG_HD void start(uint64_t rows, int RS, int64_t lo, int64_t hi, int w_end, int w0) {
        const int64_t end = hi < lo + 32ll * w_end ? hi : lo + 32ll * w_end, row = lo + 32ll * w0;
        base = rows + (uint64_t)row * (uint64_t)RS;
        left = (int)(end - row);             // a part stays below 2^23 sites (pg_exact_parts) and w0 within eight words of it
    }
    // (the product between the two clips keeps them a scalar min and a scalar max: clipped back to back they become one
    // three-operand median, a vector instruction, and a descriptor in vector registers is loaded through in a loop over its values)
    PG_HD int records(int RS) const {
        const int n = (left > 32 ? 32 : left) * RS;
        return n < 0 ? 0 : n;
    }
    PG_HD void advance(int RS) {
        base += (uint64_t)(8 * 32) * (uint64_t)RS;
        left -= 8 * 32;
    }
};

#ifdef __HIPCC__
#include <hip/hip_runtime.h>

typedef int v4i __attribute__((ext_vector_type(4)));
typedef int v8i __attribute__((ext_vector_type(8)));
typedef float v16f __attribute__((ext_vector_type(16)));

// One MX fp4 product, 32 x 32 x 64, both operands e2m1 (the first four registers of a and b; the others are not read).  Scale
// operands 0, 0 select the unscaled encoding v_mfma_f32_32x32x64_f8f6f4 -- both scales 2^0 --: one instruction word pair less per
// product than the v_mfma_ld_scale + v_mfma pair, and no scale register to read.
__device__ __forceinline__ v16f pg_mfma_fp4(const v8i &a, const v8i &b, const v16f &c) {
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a, b, c, 4, 4, 0, 0, 0, 0);
}

__device__ __forceinline__ uint32_t comp(const uint4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

__device__ __forceinline__ uint32_t lds_addr(const void *p) {
    return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}

// Accumulator tile (I, J) -> upper triangle of the window's n x n matrix M.  C/D layout of the 32 x 32 product: column = lane & 31,
// row = (reg & 3) + 8 (reg >> 2) + 4 (lane >> 5).  An accumulator holds count / SCALE (SCALE = 4: 0.5 x 0.5 products; 1: the
// count itself, no multiply).  Parts of a window (`atomic`) meet in a zeroed matrix by integer atomics; zeros are not sent.
template <int SCALE>
__device__ __forceinline__ void pg_store_tile(const v16f &acc, int I, int J, int lane, int n, int diag, int atomic, int32_t *__restrict__ M) {
    const int col = 32 * J + (lane & 31);
    if (col >= n) return;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int row = 32 * I + (reg & 3) + 8 * (reg >> 2) + 4 * (lane >> 5);
        if (row >= n || row > col || (row == col && !diag)) continue;
        const int32_t v = (int32_t)(SCALE == 1 ? acc[reg] : acc[reg] * (float)SCALE);
        int32_t *dst = &M[(size_t)row * n + col];
        if (atomic) { if (v) atomicAdd(dst, v); }
        else *dst = v;
    }
}

// ---- host: into how many parts a launcher cuts the windows' step range ----------------------------------------------------------
// More parts while the grid stays below `wave_target` waves and a part keeps `min_steps` steps: wanted when windows x waves per
// window cannot give every SIMD a few waves.
static inline int pg_pick_parts(int n_win, int waves_per_win, int64_t steps_per_window, int min_steps, int wave_target) {
    const int64_t waves = (int64_t)n_win * waves_per_win;
    int kp = 1;
    while (kp < 64 && waves * kp < wave_target && steps_per_window / (kp * 2) >= min_steps) kp *= 2;
    return kp;
}

// An f32 accumulator holds a count (or count / 4) exactly while count < 2^24: no part of any window may see more than 2^23 sites
// (a margin of two).
static inline int pg_exact_parts(int64_t max_sites) { return (int)((max_sites + (1 << 23) - 1) >> 23); }

// the parts of a window are combined by atomics: n_win matrices of n x n counts start from zero
static inline void pg_zero_if_parts(hipStream_t st, int32_t *M, int n_win, int n, int64_t kparts) {
    if (kparts > 1) (void)hipMemsetAsync(M, 0, (size_t)n_win * n * n * 4, st);
}
#endif  // __HIPCC__
