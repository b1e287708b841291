// The device route of the seqToGeno.py drop-in walked on the host: the functions of genomics_general_amd/csrc/pg_s2g_core.h with 64
// emulated lanes per wavefront and emulated LDS tiles, in the division of work of k_s2g_lines / k_s2g_gather / k_s2g_tile
// (csrc/pg_s2g_dev.hip).  tests/test_s2g_emul.py puts it in the device's place inside the driver.
#include "../genomics_general_amd/csrc/pg_s2g_core.h"

#include <cstring>
#include <vector>

namespace {

const int LANES = 64, WAVES = 4;

}  // namespace

extern "C" {

int pgs_emul_tile_seqs(int n_haps, int want) { return pgs_tile_seqs(n_haps, want, 60 * 1024); }

// A block of whole lines as k_s2g_lines, the scans, k_s2g_heads and k_s2g_gather take it: its residues to store[base ..) (the store
// begins at a multiple of 16), heads[3 k ..] the head lines' records.  1: the block is handed back (*host_line the first line the
// device does not take), 0: *n_res residues, *n_heads head lines
int pgs_emul_block(const char *text_, int64_t len, int open, uint8_t *store, int64_t base, int64_t *heads, int64_t *n_res, int64_t *n_heads,
                   int64_t *host_line) {
    const uint8_t *text = reinterpret_cast<const uint8_t *>(text_);
    *n_res = *n_heads = 0;
    *host_line = -1;
    if (len == 0 || text[len - 1] != '\n') {
        *host_line = 0;
        return 1;
    }
    std::vector<int64_t> nl;
    for (int64_t k = 0; k < len; ++k)
        if (text[k] == '\n') nl.push_back(k);
    const int64_t n_lines = (int64_t)nl.size();
    std::vector<uint32_t> cnt((size_t)n_lines), head((size_t)n_lines);
    int64_t first_host = -1;
    for (int64_t i = 0; i < n_lines; ++i) {                        // k_s2g_lines: a wavefront per line
        const int64_t ls = i ? nl[(size_t)i - 1] + 1 : 0, n = nl[(size_t)i] - ls;
        const uint8_t *line = text + ls;
        const bool is_head = pgs_is_head(line, n);
        bool any = false;
        for (int lane = 0; lane < LANES; ++lane) {
            bool bad = i == 0 && !open && !is_head;
            for (int64_t k = (int64_t)lane * PGS_STORE; k < n; k += LANES * PGS_STORE)         // 16 bytes a lane and step
                for (int q = 0; q < PGS_STORE && k + q < n; ++q) bad = bad || pgs_irregular(line[k + q], k + q == 0, is_head);
            any = any || bad;                                      // (the ballot)
        }
        head[(size_t)i] = is_head;
        cnt[(size_t)i] = any ? 0u : pgs_line_residues(line, n);
        if (any && first_host < 0) first_host = i;
    }
    if (first_host >= 0) {
        *host_line = first_host;
        return 1;
    }
    int64_t res = 0, nh = 0;
    for (int64_t i = 0; i < n_lines; ++i) {                        // the scans, k_s2g_heads, k_s2g_gather
        const int64_t ls = i ? nl[(size_t)i - 1] + 1 : 0, n = cnt[(size_t)i];
        if (head[(size_t)i]) {
            heads[3 * nh] = ls;
            heads[3 * nh + 1] = nl[(size_t)i] - ls;
            heads[3 * nh + 2] = res;
            ++nh;
        }
        const uint8_t *src = text + ls;
        const int64_t at = base + res;
        const int64_t to16 = (PGS_STORE - (at & (PGS_STORE - 1))) & (PGS_STORE - 1), lead = n < to16 ? n : to16;
        const int64_t full = (n - lead) / PGS_STORE, done = lead + full * PGS_STORE;
        for (int lane = 0; lane < LANES; ++lane) {
            if (lane < lead) store[at + lane] = src[lane];
            for (int64_t k = lane; k < full; k += LANES) memcpy(store + at + lead + k * PGS_STORE, src + lead + k * PGS_STORE, PGS_STORE);
            if (done + lane < n) store[at + done + lane] = src[done + lane];
        }
        res += n;
    }
    *n_res = res;
    *n_heads = nh;
    return 0;
}

// A range of the output as k_s2g_tile writes it: jobs of PGS_TILE_SITES sites of one piece, a tile of tile_seqs haplotypes each; the
// store is readable 8 bytes past store_len.  -1: a store outside [0, out_len) or a template the route does not take
int pgs_emul_emit(const uint8_t *store, const int32_t *tmpl, int32_t tmpl_len, int32_t n_haps, const uint8_t *names, const int64_t *name_off,
                  const int64_t *hap_off, int tile_seqs, const int32_t *seg, const int64_t *x0, const int64_t *x1, int64_t n_pieces, uint8_t *out,
                  int64_t out_len) {
    const int n_tiles = (n_haps + tile_seqs - 1) / tile_seqs;
    std::vector<int32_t> tstart((size_t)n_tiles + 1, 0);
    if (pgs_tile_starts(tmpl, tmpl_len, n_haps, tile_seqs, tstart.data())) return -1;
    std::vector<uint32_t> lds((size_t)tile_seqs * (PGS_TILE_PITCH / 4));
    const uint8_t *tile = reinterpret_cast<const uint8_t *>(lds.data());
    int64_t at = 0;
    for (int64_t p = 0; p < n_pieces; ++p) {
        const uint8_t *name = names + name_off[seg[p]];
        const uint32_t name_len = (uint32_t)(name_off[seg[p] + 1] - name_off[seg[p]]);
        const uint64_t fixed = pgs_line_fixed(name_len, (uint32_t)tmpl_len);
        const uint64_t piece0 = pgs_line_start((uint64_t)x0[p], fixed);
        for (int64_t site0 = x0[p]; site0 < x1[p]; site0 += PGS_TILE_SITES) {
            const int ns = (int)(x1[p] - site0 < PGS_TILE_SITES ? x1[p] - site0 : PGS_TILE_SITES);
            const uint64_t start0 = pgs_line_start((uint64_t)site0, fixed);
            const int64_t out_at = at + (int64_t)(start0 - piece0);
            for (int ty = 0; ty < n_tiles; ++ty) {
                int64_t h0;
                const int nh = (int)pgs_tile_count(n_haps, tile_seqs, ty, &h0);
                const int j0 = tstart[(size_t)ty], j1 = tstart[(size_t)ty + 1];
                std::fill(lds.begin(), lds.end(), 0xeeeeeeeeu);
                for (int item = 0; item < nh * (PGS_TILE_SITES / 4); ++item) {         // (1) aligned words, funnelled
                    const int hh = item / (PGS_TILE_SITES / 4), w = item % (PGS_TILE_SITES / 4);
                    if (4 * w >= ns) continue;
                    const int64_t src = hap_off[(int64_t)seg[p] * n_haps + h0 + hh] + site0;
                    const int shift = (int)(src & 3);
                    uint32_t lo, hi = 0;
                    memcpy(&lo, store + src - shift + 4 * w, 4);
                    if (shift) memcpy(&hi, store + src - shift + 4 * w + 4, 4);
                    lds[(size_t)hh * (PGS_TILE_PITCH / 4) + (size_t)w] = pgs_funnel(lo, hi, shift);
                }
                for (int wave = 0; wave < WAVES; ++wave)                                 // (2) whole lines
                    for (int l = wave; l < ns; l += WAVES) {
                        const uint64_t x = (uint64_t)site0 + (uint64_t)l, pos = x + 1;
                        const int d = pgs_digits(pos);
                        const int64_t pl = (int64_t)name_len + 2 + d;
                        const int64_t ls = out_at + (int64_t)(pgs_line_start(x, fixed) - start0);
                        const int64_t a = ls + (ty ? pl + j0 : 0), b = ls + pl + j1;
                        const int64_t n_st = pgs_store_count(a, b);
                        for (int lane = 0; lane < LANES; ++lane)
                            for (int64_t k = lane; k < n_st; k += LANES) {
                                int64_t lo, hi;
                                pgs_store_at(a, b, k, &lo, &hi);
                                if (lo < 0 || hi > out_len || lo >= hi || (hi - lo == PGS_STORE && lo % PGS_STORE)) return -1;
                                for (int64_t q = lo; q < hi; ++q) {
                                    const int64_t pp = q - ls;
                                    uint8_t byte;
                                    if (pp < pl) {
                                        byte = pgs_prefix_byte(name, name_len, pos, d, (uint32_t)pp);
                                    } else {
                                        const int32_t t = tmpl[pp - pl];
                                        if (pp - pl < j0 || pp - pl >= j1) return -1;
                                        byte = pgs_is_lit(t) ? pgs_lit_byte(t) : tile[(size_t)(t - (int32_t)h0) * PGS_TILE_PITCH + (size_t)l];
                                    }
                                    if (out[q] != 0xdd) return -1;                       // (every byte is written once)
                                    out[q] = byte;
                                }
                            }
                    }
            }
        }
        at += (int64_t)(pgs_line_start((uint64_t)x1[p], fixed) - piece0);
    }
    return at == out_len ? 0 : -1;
}

// the closed form against a running sum for x = 0 .. upto, and against Python's numbers at single points
int64_t pgs_emul_digit_sum_mismatch(int64_t upto) {
    uint64_t run = 0;
    for (uint64_t x = 0; x <= (uint64_t)upto; ++x) {
        if (pgs_digit_sum(x) != run) return (int64_t)x;
        run += (uint64_t)pgs_digits(x + 1);
    }
    return -1;
}
uint64_t pgs_emul_digit_sum(uint64_t x) { return pgs_digit_sum(x); }
uint64_t pgs_emul_line_start(uint64_t x, uint64_t fixed) { return pgs_line_start(x, fixed); }

}  // extern "C"
