// The host route of the seqToGeno.py drop-in: pg_s2g_strip takes the feeds and blanks out of a fasta record's text (the residue store
// of the host route, and the blocks the device route hands back), pg_s2g_text writes the lines of an output range from the store, a
// share of the sites per host thread, with the functions of pg_s2g_core.h.  No GPU context is needed, and nothing but the C++
// library: tests/s2g_host_main.cpp compiles this file on its own.
#include "pg_s2g_core.h"

#include <algorithm>
#include <cstring>
#include <thread>
#include <vector>

extern "C" {

// text[0 .. len) without its line feeds and blanks into dst (room for len bytes); the number of bytes written.  n_threads shares of
// the text are counted, then copied to their places.
int64_t pg_s2g_strip(const char *text, int64_t len, uint8_t *dst, int n_threads) {
    if (!text || !dst || len <= 0) return 0;
    const uint8_t *t = reinterpret_cast<const uint8_t *>(text);
    int nt = std::max(1, std::min<int>(n_threads, (int)std::min<int64_t>(64, len / (1 << 20) + 1)));
    std::vector<int64_t> at((size_t)nt + 1, 0);
    auto share = [&](int k, bool copy) {
        const int64_t a = len * k / nt, b = len * (k + 1) / nt;
        if (!copy) {
            int64_t n = 0;
            for (int64_t i = a; i < b; ++i) n += !pgs_dropped(t[i]);
            at[(size_t)k + 1] = n;
            return;
        }
        uint8_t *o = dst + at[(size_t)k];
        for (int64_t i = a; i < b;) {                             // (lines are copied whole up to their feed or blank)
            int64_t j = i;
            while (j < b && !pgs_dropped(t[j])) ++j;
            std::memcpy(o, t + i, (size_t)(j - i));
            o += j - i;
            i = j + 1;
        }
    };
    for (int pass = 0; pass < 2; ++pass) {
        if (nt == 1) {
            share(0, pass == 1);
        } else {
            std::vector<std::thread> th;
            for (int k = 0; k < nt; ++k) th.emplace_back(share, k, pass == 1);
            for (auto &x : th) x.join();
        }
        if (pass == 0)
            for (int k = 0; k < nt; ++k) at[(size_t)k + 1] += at[(size_t)k];
    }
    return at[(size_t)nt];
}

// Lines x0 .. x1 - 1 of a segment into out: name '\t' str(x + 1) '\t' and the template's bytes, a literal or the residue of haplotype
// h at store[hap_off[h] + x].  out_len must be what the closed form gives, pgs_line_start(x1) - pgs_line_start(x0): else -1, and
// nothing is written.  Returns the bytes written.
int64_t pg_s2g_text(const uint8_t *store, const char *name, int32_t name_len, const int64_t *hap_off, const int32_t *tmpl, int32_t tmpl_len,
                    int64_t x0, int64_t x1, uint8_t *out, int64_t out_len, int n_threads) {
    if (x1 < x0 || x0 < 0 || name_len < 0 || tmpl_len < 0 || (name_len && !name) || (tmpl_len && !tmpl)) return -1;
    const uint64_t fixed = pgs_line_fixed((uint32_t)name_len, (uint32_t)tmpl_len);
    const uint64_t base = pgs_line_start((uint64_t)x0, fixed);
    if ((int64_t)(pgs_line_start((uint64_t)x1, fixed) - base) != out_len) return -1;
    if (x1 == x0) return 0;
    if (!out || !store) return -1;
    const uint8_t *nm = reinterpret_cast<const uint8_t *>(name);
    const int64_t n = x1 - x0;
    const int nt = (int)std::max<int64_t>(1, std::min<int64_t>(std::min(n_threads, 64), n / 4096 + 1));
    auto share = [&](int k) {
        const int64_t a = x0 + n * k / nt, b = x0 + n * (k + 1) / nt;
        uint8_t *o = out + (pgs_line_start((uint64_t)a, fixed) - base);
        for (int64_t x = a; x < b; ++x) {
            const uint64_t pos = (uint64_t)x + 1;
            const int d = pgs_digits(pos);
            const uint32_t pl = (uint32_t)name_len + 2 + (uint32_t)d;
            for (uint32_t p = 0; p < pl; ++p) o[p] = pgs_prefix_byte(nm, (uint32_t)name_len, pos, d, p);
            o += pl;
            for (int32_t j = 0; j < tmpl_len; ++j) o[j] = pgs_is_lit(tmpl[j]) ? pgs_lit_byte(tmpl[j]) : store[hap_off[tmpl[j]] + x];
            o += tmpl_len;
        }
    };
    if (nt == 1) {
        share(0);
    } else {
        std::vector<std::thread> th;
        for (int k = 0; k < nt; ++k) th.emplace_back(share, k);
        for (auto &x : th) x.join();
    }
    return out_len;
}

}  // extern "C"
