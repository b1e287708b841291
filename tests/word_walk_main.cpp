// The fused pack kernel's descriptor walk (csrc/pg_pair_common.h: PgWordWalk) on the CPU.  A wave of the kernel reads every
// eighth word (32 sites) of its window part and steps the word's descriptor from the one before; here every such walk is set
// against the descriptor worked out from the word's number, as the kernel did before it walked:
//   rows   = w < w_end ? min(hi - (lo + 32 w), 32) : 0,   records = rows * RS,   base = rows_ptr + (lo + 32 w) * RS  (any, if rows = 0)
// over windows of 0 .. 8 * 32 * k +- 1 sites, every number of parts, every wave, row pitches up to 2048 bytes, and windows whose
// rows start beyond 2^31 and 2^32 bytes into the resident buffer (the base is 64 bits wide; no offset leaves the word).
// Prints "<walks> walks, 0 bad"; exit status 1 and one line per failure otherwise.
#include "../genomics_general_amd/csrc/pg_pair_common.h"

#include <cstdio>

int main() {
    long long walks = 0, bad = 0;
    const uint64_t rows_ptr = 0x00007f0000000000ull;         // (48 bits, as a device address)
    const int64_t los[] = {0, 5, 12'000'000, 40'000'000};    // x 224 bytes a row: 0, ~1 KB, 2.7 GB (> 2^31), 8.9 GB (> 2^32)
    const int lens[] = {0, 1, 31, 32, 33, 255, 256, 257, 511, 512, 513, 767, 768, 769, 2047, 2048, 2049, 50'000};
    const int pitches[] = {1, 8, 100, 224, 2048};
    for (int64_t lo : los)
        for (int len : lens)
            for (int RS : pitches)
                for (int kparts = 1; kparts <= 7; ++kparts)
                    for (int kp = 0; kp < kparts; ++kp) {
                        const int64_t hi = lo + len;
                        const int W = (int)((hi - lo + 31) >> 5);
                        const int w_begin = (int)((long long)W * kp / kparts), w_end = (int)((long long)W * (kp + 1) / kparts);
                        const int nit = (w_end - w_begin + 7) >> 3;
                        for (int wave = 0; wave < 8; ++wave, ++walks) {
                            PgWordWalk walk;
                            walk.start(rows_ptr, RS, lo, hi, w_end, w_begin + wave);
                            // the kernel asks for nit + 1 descriptors: the first word, then one word ahead in each iteration
                            for (int it = 0; it <= nit; ++it, walk.advance(RS)) {
                                const int w = w_begin + 8 * it + wave;
                                const int64_t row = lo + 32ll * w;
                                const int rows = w < w_end ? (int)((hi - row) < 32 ? (hi - row) : 32) : 0;
                                const int rec = walk.records(RS);
                                bool ok = rec == rows * RS;
                                if (rows) ok = ok && walk.base == rows_ptr + (uint64_t)row * (uint64_t)RS;
                                // the bytes a descriptor lets through lie inside the window's rows
                                if (rec) ok = ok && walk.base >= rows_ptr + (uint64_t)lo * RS && walk.base + (uint64_t)rec <= rows_ptr + (uint64_t)hi * RS;
                                if (!ok) {
                                    std::printf("lo %lld len %d RS %d part %d/%d wave %d it %d: records %d (want %d), base %llx\n", (long long)lo, len,
                                                RS, kp, kparts, wave, it, rec, rows * RS, (unsigned long long)walk.base);
                                    ++bad;
                                }
                            }
                        }
                    }
    std::printf("%lld walks, %lld bad\n", walks, bad);
    return bad ? 1 : 0;
}
