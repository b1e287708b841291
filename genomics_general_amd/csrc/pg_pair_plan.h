// The host side of the pack-and-pair pass, decided apart from its launches: the switches, which kernels take a shape, how the
// windows are cut into batches and how a batch's staging vector and scratch are laid out.  Plain C++17 with no HIP header, so that
// a CPU program can walk every decision (tests/pair_plan_main.cpp); pairwise_batches (pg_abi.cpp) carries the plan out.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdlib>
#include <cstring>

#define PG_XV_PLANES 2        // planes per word of virtual biallelic sites: x ("carries the tested allele"), v (called, not excluded)

// Input words (of 32 sites) per compaction group of the pack kernels = per block: 64 (2048 sites); 128 when that still leaves the
// chip several times oversubscribed with blocks: larger groups end in fewer partial XV words (k_pairD's work) and amortise a
// block's start-up; measured on the north-star shape (50 000 -> 25 000 two-wave blocks): k_pack3 -5 %, k_pairD -3.5 %; on C2 (5000
// -> 2600 one-wave blocks, fewer than the chip holds) k_pack3 +5 %; and 32 when 64 would leave fewer than two waves per SIMD slot
// (C2: 4883 one-wave blocks; measured 0.44 - 0.47 ms with 32 against 0.465 - 0.484 with 64).  pg_plan_pair_pass picks.
#define PG_GROUP 64
#define PG_GROUP_MAX 128
// Words of virtual sites reserved per group, worst case (every site with four alleles) / default: enough whenever a window has no
// more virtual sites than sites (a biallelic site is one virtual site; + 1 for the group's partial last word).  k_pack2 / k_pack3
// raise bit 1 of the flag word when a window needs more; the host then repeats the call with PG_XV_CAP (and keeps it for good).
#define PG_XV_CAP(grp) (3 * (grp))
#define PG_XV_CAP_DEFAULT(grp) ((grp) + 1)

// k_pairC_tile's domain (pg_pair_tile.hip): stages of PG_TILE_GP_C pairs of groups, a ring PG_TILE_NSTG deep in 64 KiB of LDS (the
// launcher runs two stages; the bound on the planes is still that of three)
constexpr int PG_TILE_NSTG = 3, PG_TILE_GP_C = 2, PG_TILE_RING_BYTES = 64 * 1024;

// ---- the switches ---------------------------------------------------------------------------------------------------------------
// Every environment switch of the pass, named here and nowhere else.  Read afresh by pg_set_samples (the plane stride) and at the
// start of every pass: the tests change modes between engines inside one process.
struct PgPairSwitches {
    bool valu = false;             // PG_PAIR_VALU: the popcount kernels k_pairC / k_pairD count the pairs (A/B runs, tests)
    bool pack2 = false;            // PG_PACK2: k_pack2 instead of k_pack3 (A/B runs, tests)
    int burst = -1;                // PG_PACK_BURST=0: k_pack3 without its burst stores (A/B runs, tests); unset = -1
    int perm = -1;                 // PG_PACK_PERM=k (experiment): windows in the order 0, P, 2P, ... (pg_pack_perm); unset = -1
    int fuse = -1;                 // PG_PACK_FUSE: 1 the fused pack kernel anywhere in its domain, 0 nowhere, unset (-1) where it pays
    int group_words = 0;           // PG_GROUP_WORDS: the compaction group (A/B runs); 0 = unset
    bool overlap = false;          // PG_OVERLAP=n: the two-stream pipeline with n sub-batches (8 below n = 2)
    int n_sub = 8;
    bool no_dip = false;           // PG_NO_DIP: per-haplotype called counts from the start
    bool tile_b = true, tile_c = true;          // PG_PAIR_TILE: a 'b' admits k_pairC_big, a 'c' k_pairC_tile; unset = "bc"
    bool blocks_per_cu = false;    // PG_PACK_BLOCKS_PER_CU: no kernel reads it any more; setting it still keeps the two-kernel pack path
    // a switch that tunes or selects the two pack kernels keeps them
    bool keeps_two_kernels() const { return valu || pack2 || burst >= 0 || group_words || blocks_per_cu || overlap || perm >= 0; }
};

inline PgPairSwitches pg_pair_switches() {
    PgPairSwitches s;
    s.valu = getenv("PG_PAIR_VALU") != nullptr;
    s.pack2 = getenv("PG_PACK2") != nullptr;
    if (const char *e = getenv("PG_PACK_BURST")) s.burst = atoi(e) != 0;
    if (const char *e = getenv("PG_PACK_PERM")) s.perm = std::max(0, atoi(e));
    if (const char *e = getenv("PG_PACK_FUSE")) s.fuse = atoi(e) != 0;
    if (const char *e = getenv("PG_GROUP_WORDS")) s.group_words = std::min(PG_GROUP_MAX, std::max(8, atoi(e) / 4 * 4));
    if (const char *e = getenv("PG_OVERLAP")) { s.overlap = true; s.n_sub = atoi(e) >= 2 ? atoi(e) : 8; }
    s.no_dip = getenv("PG_NO_DIP") != nullptr;
    if (const char *e = getenv("PG_PAIR_TILE")) { s.tile_b = strchr(e, 'b') != nullptr; s.tile_c = strchr(e, 'c') != nullptr; }
    s.blocks_per_cu = getenv("PG_PACK_BLOCKS_PER_CU") != nullptr;
    return s;
}

// ---- shapes and predicates ------------------------------------------------------------------------------------------------------
// plane stride: 32 haplotypes (one tile of the matrix-core pair kernels); the popcount kernels work on 64-lane column chunks
inline int pg_plane_stride(int n_hap, const PgPairSwitches &sw) { return sw.valu ? (n_hap + 63) / 64 * 64 : (n_hap + 31) / 32 * 32; }
// a pass starts with called counts per individual where every individual has two haplotypes (pairwise_run takes it back on a mismatch)
inline bool pg_start_dip(bool all_diploid, const PgPairSwitches &sw) { return all_diploid && !sw.no_dip; }

struct PgPairShape {
    int N, NP, n_units, NPv;       // haplotypes, their plane stride; units of the called counts (individuals when dip), theirs
    bool dip;
};
inline PgPairShape pg_pair_shape(int n_hap, int NP, bool dip) {
    const int n_units = dip ? n_hap / 2 : n_hap;
    return {n_hap, NP, n_units, dip ? (NP % 64 ? (n_units + 31) / 32 * 32 : (n_units + 63) / 64 * 64) : NP, dip};
}

// k_pairC_big: planes of up to 7 tiles of 32 units (the ring holds the T tile rows of a pair of groups, whatever the plane's stride)
inline bool pg_pair_big_fits(const PgPairShape &s, const PgPairSwitches &sw) {
    const int T = (s.n_units + 31) / 32;
    return sw.tile_b && T >= 1 && T <= 7 && s.NPv >= 32 * T;
}
// k_pairC_tile: a stage must fit the ring
inline bool pg_pair_tile_fits(const PgPairShape &s, const PgPairSwitches &sw) {
    const int64_t stage = (int64_t)2 * PG_TILE_GP_C * s.NPv * 16;
    return sw.tile_c && s.NPv % 32 == 0 && stage * PG_TILE_NSTG <= PG_TILE_RING_BYTES;
}
// The fused form of k_pack3 takes called counts that k_pairC_big would form and rows that one wave spans (up to 512 slots).  By
// itself the library takes it from 1024 windows a call and more than 128 units on (measurements: pg_pair2.hip); PG_PACK_FUSE=1
// takes it anywhere in its domain, PG_PACK_FUSE=0 keeps the two kernels, and so does every switch that tunes or selects them.
inline bool pg_pack_fuse_fits(const PgPairShape &s, const PgPairSwitches &sw, int n_win) {
    if (sw.fuse >= 0 ? sw.fuse == 0 : (n_win < 1024 || s.n_units <= 128)) return false;
    return !sw.keeps_two_kernels() && s.NP <= 512 && s.n_units >= 1 && pg_pair_big_fits(s, sw);
}

// Who packs: k_pack3 up to 4096 slots; beyond (or k_pack2 forced beyond one of ITS blocks, 1024 slots) k_pack2 behind the presence
// pre-pass (measurements: pg_pair2.hip)
enum PgPackRoute { PG_PACK_FUSED, PG_PACK_3, PG_PACK_2, PG_PACK_2_PRESENCE };
enum PgCRoute { PG_C_IN_PACK, PG_C_BIG, PG_C_TILE, PG_C_FP4, PG_C_POPCOUNT };      // who counts the called pairs
enum PgDRoute { PG_D_FP4, PG_D_POPCOUNT };                                         // who counts the differences

inline PgPackRoute pg_pack_route(int NP, const PgPairSwitches &sw) {
    const int threads = NP / 4;    // (k_pack3: a lane covers 8 slots = one dword of a resident row; k_pack2: 4 slots)
    if (threads <= 1024 && !sw.pack2) return PG_PACK_3;
    return threads <= 256 ? PG_PACK_2 : PG_PACK_2_PRESENCE;
}

inline bool pg_pack_needs_presence(int NP, const PgPairSwitches &sw) { return pg_pack_route(NP, sw) == PG_PACK_2_PRESENCE; }
// k_pack3's form with burst stores: blocks of up to two waves (512 slots)
inline bool pg_pack3_burst(int NP, const PgPairSwitches &sw) { return sw.burst != 0 && (NP / 4 + 1) / 2 <= 128; }
// PG_PACK_PERM=k: the stride P of the window order 0, P, 2P, ... (mod n): the number coprime with n next to n / k
inline int pg_pack_perm(const PgPairSwitches &sw, int n) {
    if (sw.perm <= 1 || n <= 2 * sw.perm) return 1;
    auto gcd = [](int a, int b) { while (b) { const int t = a % b; a = b; b = t; } return a; };
    int perm = n / sw.perm;
    while (gcd(perm, n) != 1) ++perm;
    return perm;
}

// the fused form's argument block: pack and called counts in one kernel, no called plane (pg_pair2.hip)
struct PgFuseArgs {
    int32_t n_win, kparts, n_units, T, diag;
    int32_t *Cmat;
    signed char a[8][4], b[8][2];           // wave w forms the tiles (a[w][p], b[w][p & 1]), p = 0 .. 3, of those mask[w] names
    unsigned char mask[8];
};
// Tiles of the upper triangle of T x T dealt to the 8 waves, four products a[p] x b[p & 1] each: 2 x 2 blocks of tile rows
// (2i, 2i+1) x tile columns (2j, 2j+1), j >= i -- six of them up to T = 6 --; at T = 7 the last tile column goes to two waves of its
// own, rows 0 .. 3 and 4 .. 6 (28 tiles, 4 + 3 of them there).  Products outside the triangle run on cell 0 and are not stored.
inline void pg_fuse_tasks(int T, PgFuseArgs &fa) {
    memset(fa.a, 0, sizeof fa.a);
    memset(fa.b, 0, sizeof fa.b);
    memset(fa.mask, 0, sizeof fa.mask);
    const int Tb = T == 7 ? 6 : T;
    int wv = 0;
    for (int i = 0; i < Tb; i += 2)
        for (int j = i; j < Tb; j += 2, ++wv)
            for (int p = 0; p < 4; ++p) {
                const int I = i + (p >> 1), J = j + (p & 1);
                if (I < Tb && J < Tb && I <= J) {
                    fa.a[wv][p] = (signed char)I;
                    fa.b[wv][p & 1] = (signed char)J;
                    fa.mask[wv] |= (unsigned char)(1u << p);
                }
            }
    if (T == 7)
        for (int i = 0; i < 7; i += 4, ++wv) {
            fa.b[wv][0] = fa.b[wv][1] = 6;
            for (int p = 0; p < 4 && i + p < 7; ++p) {
                fa.a[wv][p] = (signed char)(i + p);
                fa.mask[wv] |= (unsigned char)(1u << p);
            }
        }
}

// ---- the plan of one pass ---------------------------------------------------------------------------------------------------------
inline int64_t pg_window_words(int64_t len) { return (len + 31) / 32; }
inline int64_t pg_window_groups(int64_t len, int grp) { return (pg_window_words(len) + grp - 1) / grp; }

struct PgPairPlan {
    int grp, capg;                 // words per compaction group = per pack block; XV words reserved per group
    PgPackRoute pack;
    PgCRoute c_route;
    PgDRoute d_route;
    int64_t word_bytes, mat_bytes; // scratch per 32-site input word of a slot (planes) / per window (matrices)
    bool multi, two_streams;       // the pass exceeds the scratch limit / PG_OVERLAP's pipeline
    int n_sub;
    int64_t target_words, batch_bytes;          // a batch of more than one window holds at most this many words / bytes
    bool fused() const { return pack == PG_PACK_FUSED; }
    bool presence() const { return pack == PG_PACK_2_PRESENCE; }          // (fused: at most 512 slots, never the pre-pass)
};

inline PgPairPlan pg_plan_pair_pass(const PgPairShape &s, const PgPairSwitches &sw, const int64_t *lo, const int64_t *hi, int n_win,
                                    int64_t scratch_limit, bool xv_worst) {
    PgPairPlan p;
    p.mat_bytes = 4ll * s.N * s.N + 4ll * s.n_units * s.n_units;
    // compaction group (see PG_GROUP); PG_GROUP_WORDS overrides
    int64_t blocks64 = 0;
    for (int w = 0; w < n_win; ++w) blocks64 += pg_window_groups(hi[w] - lo[w], PG_GROUP);
    const int waves_per_block = (s.NP / 4 + 63) / 64;
    p.grp = blocks64 * waves_per_block >= 32768 ? PG_GROUP_MAX : blocks64 * waves_per_block < 8192 ? PG_GROUP / 2 : PG_GROUP;
    if (sw.group_words) p.grp = sw.group_words;
    p.capg = xv_worst ? PG_XV_CAP(p.grp) : PG_XV_CAP_DEFAULT(p.grp);
    // the fused form of the pack kernel counts the called pairs itself: no called plane, no C-count kernel.  Otherwise the pair
    // counts run on the matrix cores (exact MX fp4 products of the bit planes) unless PG_PAIR_VALU keeps the popcount kernels.
    p.pack = pg_pack_fuse_fits(s, sw, n_win) ? PG_PACK_FUSED : pg_pack_route(s.NP, sw);
    p.c_route = p.fused() ? PG_C_IN_PACK : sw.valu ? PG_C_POPCOUNT : pg_pair_big_fits(s, sw) ? PG_C_BIG : pg_pair_tile_fits(s, sw) ? PG_C_TILE : PG_C_FP4;
    p.d_route = sw.valu ? PG_D_POPCOUNT : PG_D_FP4;
    // called plane (unless fused) + reserved virtual-site planes (capg words per group)
    p.word_bytes = ((int64_t)s.NP * 4 * PG_XV_PLANES * p.capg + p.grp - 1) / p.grp + (p.fused() ? 0 : (int64_t)s.NPv * 4);
    int64_t total_words = 0;
    for (int w = 0; w < n_win; ++w) total_words += pg_window_groups(hi[w] - lo[w], p.grp) * p.grp;
    // A job that fits one batch runs as one batch on one stream: splitting it only to overlap the pack kernel with the pair
    // kernels is slower (measured: C2 1.44 vs 0.99 ms).  A job that needs several batches is cut at the scratch limit and its
    // sub-batches follow each other on the one stream: since the pair kernels run on the matrix cores, the pack kernel beside
    // them on a second stream costs more CU time than it hides (north-star shape 11.2 - 12.1 against 9.8 - 11.0 ms; one rank's
    // share of config 5, 150 GB: 40.1 ms pipelined).  PG_OVERLAP=1 brings the two-stream pipeline back (at least 8 sub-batches,
    // but none so small that it cannot fill the GPU; all but the first pack kernel beside the pair kernels of the sub-batch before).
    // (one batch uses one slot: it may take the whole scratch budget; sub-batches alternate between the two slots)
    p.multi = total_words * p.word_bytes + (int64_t)n_win * p.mat_bytes > scratch_limit;
    p.two_streams = sw.overlap;
    p.n_sub = sw.n_sub;
    p.target_words = sw.overlap ? std::max<int64_t>(total_words / sw.n_sub, 32768) : total_words;
    p.batch_bytes = p.multi || sw.overlap ? scratch_limit / 2 : scratch_limit;
    return p;
}

// A batch's staging vector [lo | hi | goff(n+1) | vgoff(n+1) | nw] of h_len int64 and what its scratch is sized to.  nw = int32 word
// counters of k_pack2, zero per window (and, in the presence-pre-pass mode, one slot per group for k_word_scan) -- they ride in
// the same copy instead of a memset.
struct PgBatchLayout {
    int w0, nb;
    size_t off_hi, off_goff, off_vgoff, off_nw, n_nw, h_len;       // (lo at 0; offsets in int64, n_nw in int32)
    int64_t ga, va, max_wds, sum_wds;      // groups, quadruples of words, the longest window's words and all words of the batch
    int max_groups;
    size_t n_Vp, n_XV, n_pres, n_Cmat, n_Dmat;  // elements; 0 where the plan's route has no such buffer
};

// the batch that starts at window w0: its windows, its groups and with them where the regions of its staging vector lie
inline PgBatchLayout pg_cut_batch(const PgPairPlan &p, const int64_t *lo, const int64_t *hi, int n_win, int w0) {
    PgBatchLayout L = {};
    int w1 = w0;
    while (w1 < n_win) {
        const int64_t groups = pg_window_groups(hi[w1] - lo[w1], p.grp), words = (L.ga + groups) * p.grp;
        const int64_t nbytes = words * p.word_bytes + (int64_t)(w1 - w0 + 1) * p.mat_bytes;
        if (w1 > w0 && (nbytes > p.batch_bytes || words > p.target_words)) break;
        L.ga += groups;
        ++w1;
        if (w1 - w0 >= 65535) break;                      // gridDim.y limit
    }
    const size_t nb = (size_t)(w1 - w0);
    L.w0 = w0;
    L.nb = w1 - w0;
    L.off_hi = nb;
    L.off_goff = 2 * nb;
    L.off_vgoff = 3 * nb + 1;
    L.off_nw = 4 * nb + 2;
    L.n_nw = nb + (p.presence() ? (size_t)L.ga : 0);
    L.h_len = L.off_nw + (L.n_nw + 1) / 2;
    return L;
}

// fills h[0 .. L.h_len) -- goff / vgoff are the prefix sums of the windows' groups / word quadruples -- and completes L
inline void pg_batch_fill(PgBatchLayout &L, const PgPairPlan &p, const PgPairShape &s, const int64_t *lo, const int64_t *hi, int64_t *h) {
    int64_t ga = 0;
    for (int k = 0; k < L.nb; ++k) {
        const int64_t len = hi[L.w0 + k] - lo[L.w0 + k], wds = pg_window_words(len), groups = pg_window_groups(len, p.grp);
        h[k] = lo[L.w0 + k];
        h[L.off_hi + k] = hi[L.w0 + k];
        h[L.off_goff + k] = ga;
        h[L.off_vgoff + k] = L.va;
        ga += groups;
        L.va += (wds + 3) / 4;
        L.max_wds = std::max(L.max_wds, wds);
        L.sum_wds += wds;
        L.max_groups = (int)std::max<int64_t>(L.max_groups, groups);
    }
    h[L.off_goff + L.nb] = ga;
    h[L.off_vgoff + L.nb] = L.va;
    memset(h + L.off_nw, 0, (L.h_len - L.off_nw) * 8);
    // + 4 word groups / words: the last stage (look-ahead load) of the pair kernels reads up to three past a part's range
    L.n_Vp = p.fused() ? 0 : (size_t)(std::max<int64_t>(L.va, 1) + 4) * s.NPv * 4;
    L.n_XV = ((size_t)std::max<int64_t>(L.ga, 1) * p.capg + 4) * PG_XV_PLANES * s.NP;
    L.n_pres = p.presence() ? (size_t)std::max<int64_t>(L.ga, 1) * p.grp * 4 : 0;
    L.n_Cmat = (size_t)L.nb * s.n_units * s.n_units;
    L.n_Dmat = (size_t)L.nb * s.N * s.N;
}
