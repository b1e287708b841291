// The pair kernels' block dealing (csrc/pg_pair_common.h: pg_deal_window / pg_deal_blocks) walked on the CPU: for every
// n_win in 0 .. 40 and per_win in 1 .. 7, over the blocks 0 .. pg_deal_blocks - 1,
//   1. the accepted blocks map one-to-one onto all n_win * per_win pairs (window, rest);
//   2. a window below 8 * (n_win / 8) has all its blocks on one XCD (block % 8), the XCD win % 8;
//   3. of the remaining windows' pairs, in the order (window, rest), every XCD gets one contiguous run of at most
//      ceil(total / 8), in the order of its blocks.
// Prints "<cases> cases, 0 bad"; exit status 1 and one line per failure otherwise.
#include "../genomics_general_amd/csrc/pg_pair_common.h"

#include <cstdio>
#include <vector>

int main() {
    int cases = 0, bad = 0;
    auto fail = [&](int n_win, int per_win, const char *what, long long block) {
        std::printf("n_win %d per_win %d: %s (block %lld)\n", n_win, per_win, what, block);
        ++bad;
    };
    for (int n_win = 0; n_win <= 40; ++n_win)
        for (int per_win = 1; per_win <= 7; ++per_win, ++cases) {
            const int64_t blocks = pg_deal_blocks(n_win, per_win);
            const int full = 8 * (n_win / 8), total = (n_win - full) * per_win, run_max = (total + 7) / 8;
            if (blocks % 8 != 0 || blocks < (int64_t)n_win * per_win) fail(n_win, per_win, "grid too small or not a multiple of 8", blocks);
            std::vector<int> seen((size_t)n_win * per_win, 0);
            std::vector<std::vector<int>> run(8);                    // per XCD: the remainder's pairs, linearised, in block order
            for (int64_t b = 0; b < blocks; ++b) {
                int win = -1, rem = -1;
                if (!pg_deal_window((unsigned)b, per_win, n_win, win, rem)) continue;
                if (win < 0 || win >= n_win || rem < 0 || rem >= per_win) {
                    fail(n_win, per_win, "pair out of range", b);
                    continue;
                }
                if (seen[(size_t)win * per_win + rem]++) fail(n_win, per_win, "pair dealt twice", b);
                if (win < full) {
                    if (b % 8 != win % 8) fail(n_win, per_win, "full row: window not on XCD win % 8", b);
                } else {
                    run[(size_t)(b % 8)].push_back((win - full) * per_win + rem);
                }
            }
            for (size_t k = 0; k < seen.size(); ++k)
                if (!seen[k]) fail(n_win, per_win, "pair never dealt", (long long)k);
            for (int x = 0; x < 8; ++x) {
                const std::vector<int> &r = run[(size_t)x];
                if ((int)r.size() > run_max) fail(n_win, per_win, "remainder: run longer than ceil(total / 8)", x);
                for (size_t k = 1; k < r.size(); ++k)
                    if (r[k] != r[k - 1] + 1) fail(n_win, per_win, "remainder: run not contiguous", x);
            }
        }
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
