// csrc/pg_np_sum.h run as a program of its own (no GPU, no library): np_pairwise_sum, the one-lane float64 sum behind k_hapstats'
// H1 / H2 and k_paint's np.nanmean, as plain host code under AddressSanitizer and UndefinedBehaviorSanitizer.
//   np_sum_main IN OUT
// IN (binary, native endian): int64 count, then for every array int64 n and n float64 values.  OUT (text): a line per array with
// the bit patterns, as 16 hexadecimal digits each, of np_pairwise_sum<6>(a, n), np_pairwise_sum<9>(a, n) and, for n >= 1,
// np_pairwise_sum<9>(a + 1, n - 1) -- the view of the clusters behind the first that H2 sums -- (n == 0: the bits of 0.0), and of
// np_pairwise_sum_of<3> (n <= 968, what k_indpair_fin walks a haplotype block with; <9> beyond) over a function that hands out a[k] and
// notes that it was asked: exit status 2 if an element is asked for twice or never.
// Every array is copied into a heap block of exactly its own size, so that a read past either end is the sanitizer's to report.
// tests/test_host.py compares the bits with np.sum.  Exit status 1 on a malformed file.
#include "../genomics_general_amd/csrc/pg_np_sum.h"

#include <cstdint>
#include <cstdio>
#include <cstring>

static uint64_t bits(double v) {
    uint64_t u;
    memcpy(&u, &v, 8);
    return u;
}

int main(int argc, char **argv) {
    if (argc != 3) {
        fprintf(stderr, "usage: np_sum_main IN OUT\n");
        return 1;
    }
    FILE *in = fopen(argv[1], "rb"), *out = fopen(argv[2], "w");
    if (!in || !out) {
        fprintf(stderr, "np_sum_main: cannot open the files\n");
        return 1;
    }
    int64_t count = 0;
    if (fread(&count, 8, 1, in) != 1 || count < 0) {
        fprintf(stderr, "np_sum_main: no count\n");
        return 1;
    }
    for (int64_t k = 0; k < count; ++k) {
        int64_t n = -1;
        if (fread(&n, 8, 1, in) != 1 || n < 0 || n > (1 << 24)) {
            fprintf(stderr, "np_sum_main: array %lld: no length\n", (long long)k);
            return 1;
        }
        double *a = new double[(size_t)n];                         // (exactly n values: nothing to read beside them)
        if (n > 0 && fread(a, 8, (size_t)n, in) != (size_t)n) {
            fprintf(stderr, "np_sum_main: array %lld is cut short\n", (long long)k);
            return 1;
        }
        const double s6 = np_pairwise_sum<6>(a, (int)n), s9 = np_pairwise_sum<9>(a, (int)n);
        const double tail = n >= 1 ? np_pairwise_sum<9>(a + 1, (int)n - 1) : 0.0;
        unsigned char *asked = new unsigned char[(size_t)n]();
        auto cell = [&](int i) -> double {
            ++asked[i];
            return a[i];
        };
        const double of = n <= 968 ? np_pairwise_sum_of<3>(cell, 0, (int)n) : np_pairwise_sum_of<9>(cell, 0, (int)n);
        for (int64_t i = 0; i < n; ++i)
            if (asked[i] != 1) {
                fprintf(stderr, "np_sum_main: array %lld: element %lld asked for %d times\n", (long long)k, (long long)i, (int)asked[i]);
                return 2;
            }
        fprintf(out, "%016llx %016llx %016llx %016llx\n", (unsigned long long)bits(s6), (unsigned long long)bits(s9), (unsigned long long)bits(tail),
                (unsigned long long)bits(of));
        delete[] asked;
        delete[] a;
    }
    if (fclose(out) != 0) return 1;
    fclose(in);
    printf("%lld arrays\n", (long long)count);
    return 0;
}
