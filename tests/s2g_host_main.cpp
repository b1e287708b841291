// pg_s2g_strip and pg_s2g_text (genomics_general_amd/csrc/pg_s2g.cpp, the host route of the seqToGeno.py drop-in) on crafted
// inputs, built with -fsanitize=address,undefined by tests/test_s2g_cpu.py and run as a program of its own: every text, store and
// output is a heap buffer of exactly its size, so that a read or a write behind its end is seen.
#include "../genomics_general_amd/csrc/pg_s2g_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

extern "C" {
int64_t pg_s2g_strip(const char *text, int64_t len, uint8_t *dst, int n_threads);
int64_t pg_s2g_text(const uint8_t *store, const char *name, int32_t name_len, const int64_t *hap_off, const int32_t *tmpl, int32_t tmpl_len,
                    int64_t x0, int64_t x1, uint8_t *out, int64_t out_len, int n_threads);
}

namespace {

int failures = 0;

#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #x);            \
            ++failures;                                              \
        }                                                            \
    } while (0)

std::string strip(const std::string &text, int threads) {
    char *heap = static_cast<char *>(malloc(text.size() ? text.size() : 1));
    memcpy(heap, text.data(), text.size());
    uint8_t *dst = static_cast<uint8_t *>(malloc(text.size() ? text.size() : 1));
    const int64_t n = pg_s2g_strip(heap, (int64_t)text.size(), dst, threads);
    std::string out(reinterpret_cast<char *>(dst), (size_t)n);
    free(heap);
    free(dst);
    return out;
}

// the lines x0 .. x1 - 1 of the sequences (their groups' sizes in `ploidy`) by pg_s2g_text, and -- slow -- by string joins
bool lines(const std::vector<std::string> &seqs, const std::vector<int> &ploidy, const std::string &name, int64_t x0, int64_t x1, int threads) {
    std::string all;
    std::vector<int64_t> off;
    for (const std::string &s : seqs) {
        off.push_back((int64_t)all.size());
        all += s;
    }
    std::vector<int32_t> tmpl;
    int h = 0;
    for (size_t g = 0; g < ploidy.size(); ++g)
        for (int k = 0; k < ploidy[g]; ++k) {
            tmpl.push_back(h++);
            tmpl.push_back(pgs_lit((uint8_t)(k + 1 < ploidy[g] ? '|' : g + 1 < ploidy.size() ? '\t' : '\n')));
        }
    std::string want;
    for (int64_t x = x0; x < x1; ++x) {
        want += name + "\t" + std::to_string(x + 1) + "\t";
        for (int32_t t : tmpl) want += pgs_is_lit(t) ? (char)pgs_lit_byte(t) : seqs[(size_t)t][(size_t)x];
    }
    uint8_t *store = static_cast<uint8_t *>(malloc(all.size() ? all.size() : 1));
    memcpy(store, all.data(), all.size());
    uint8_t *out = static_cast<uint8_t *>(malloc(want.size() ? want.size() : 1));
    char *nm = static_cast<char *>(malloc(name.size() ? name.size() : 1));
    memcpy(nm, name.data(), name.size());
    const int64_t n = pg_s2g_text(store, nm, (int32_t)name.size(), off.data(), tmpl.data(), (int32_t)tmpl.size(), x0, x1, out, (int64_t)want.size(), threads);
    const bool ok = n == (int64_t)want.size() && memcmp(out, want.data(), want.size()) == 0;
    // a length the closed form does not give is refused before anything is written
    const bool refused = pg_s2g_text(store, nm, (int32_t)name.size(), off.data(), tmpl.data(), (int32_t)tmpl.size(), x0, x1, out, (int64_t)want.size() + 1, threads) == -1;
    free(store);
    free(out);
    free(nm);
    return ok && refused;
}

}  // namespace

int main() {
    CHECK(strip("", 1) == "");
    CHECK(strip("\n", 1) == "");
    CHECK(strip("ACGT", 1) == "ACGT");
    CHECK(strip("\nAC GT\n\n  TT\tA\r\n", 1) == "ACGTTT\tA\r");
    {
        std::string big, want;
        for (int k = 0; k < 3 << 20; ++k) {
            const char c = k % 61 == 60 ? '\n' : k % 977 == 5 ? ' ' : "ACGTN"[k % 5];
            big += c;
            if (c != '\n' && c != ' ') want += c;
        }
        CHECK(strip(big, 1) == want);
        CHECK(strip(big, 7) == want);
    }
    std::vector<std::string> seqs;
    for (int k = 0; k < 7; ++k) {
        std::string s;
        for (int x = 0; x < 12000; ++x) s += "ACGTN-acgt*"[(x * 7 + k * 3 + x / 11) % 11];
        seqs.push_back(s);
    }
    CHECK(lines(seqs, {1, 1, 1, 1, 1, 1, 1}, "contig0", 0, 12000, 1));
    CHECK(lines(seqs, {1, 1, 1, 1, 1, 1, 1}, "contig0", 0, 12000, 5));
    CHECK(lines(seqs, {2, 1, 4}, "c", 9, 1001, 3));
    CHECK(lines(seqs, {7}, "", 99, 10001, 2));
    CHECK(lines(seqs, {1, 2, 2, 2}, "a_long_scaffold_name", 11999, 12000, 4));
    CHECK(lines(seqs, {3, 4}, "x", 500, 500, 4));
    CHECK(lines({"A"}, {1}, "q", 0, 1, 8));
    // the closed form against a running sum
    uint64_t run = 0;
    for (uint64_t x = 0; x <= 100001; ++x) {
        CHECK(pgs_digit_sum(x) == run);
        run += (uint64_t)pgs_digits(x + 1);
    }
    if (failures) return 1;
    printf("s2g host ok\n");
    return 0;
}
