// The planning of the mergeGeno.py drop-in's rounds (genomics_general_amd/csrc/pg_merge_plan.h) as a program of its own, meant for
// g++ -fsanitize=address,undefined: random key lists, block sizes and buffer sizes; the rounds are walked the way the driver walks them
// (a file is read further when its resident lines run low) and these properties are checked --
//   the rounds' sites, one after the other, are the sites one round over everything gives
//   no round is empty while a file has lines left (a dense round covers a position, a sparse one consumes a line)
//   a dense round's lines that no file adds to stay within the output budget (one line at least), whatever the resident input holds
//   a dense round makes all the progress it may: it ends at the horizon, at its scaffold's end, or after exactly max_positions
// Usage: merge_plan_main [cases].  Prints "ok <cases> <rounds>"; any failure prints the case and exits with status 1.
#include "../genomics_general_amd/csrc/pg_merge_plan.h"

#include <cstdio>
#include <cstdlib>
#include <deque>
#include <random>
#include <set>
#include <vector>

namespace {

struct Sim {
    std::vector<pgm_site> keys;
    size_t next = 0;
    size_t block = 1;
    std::deque<pgm_site> resident;
};

int fail(int c, const char *what) {
    printf("case %d: %s\n", c, what);
    return 1;
}

}  // namespace

int main(int argc, char **argv) {
    const int cases = argc > 1 ? atoi(argv[1]) : 200;
    std::mt19937_64 rng(20261019);
    long long rounds_total = 0;
    for (int c = 0; c < cases; ++c) {
        const int n_fai = (int)(rng() % 5);                       // (0: a .fai without scaffolds)
        std::vector<int64_t> len((size_t)n_fai);
        for (auto &l : len) l = (int64_t)(rng() % 40) - 2;        // (lengths of 0 and below: scaffolds without positions)
        const int nf = 1 + (int)(rng() % 5);
        const bool dense = rng() % 2;
        const int64_t line_bytes = 1 + (int64_t)(rng() % 30), fixed = 1 + (int64_t)(rng() % 20);
        const int64_t cap = (int64_t)(rng() % 3000);
        std::vector<Sim> F((size_t)nf);
        std::set<pgm_site> all;
        for (Sim &f : F) {
            f.block = 1 + (size_t)(rng() % 7);
            for (int s = 0; s < n_fai; ++s)
                for (int64_t p = 1; p <= len[(size_t)s]; ++p)
                    if (rng() % 3 == 0) { f.keys.push_back(pgm_site{s, p}); all.insert(pgm_site{s, p}); }
        }
        std::vector<pgm_site> want;
        if (dense) {
            for (int s = 0; s < n_fai; ++s)
                for (int64_t p = 1; p <= len[(size_t)s]; ++p) want.push_back(pgm_site{s, p});
        } else
            want.assign(all.begin(), all.end());
        std::vector<pgm_site> got;
        pgm_site prev{0, 0};
        if (n_fai == 0) {                                         // the driver writes the header and is done
            if (!want.empty()) return fail(c, "sites without a scaffold");
            continue;
        }
        for (int round = 0;; ++round) {
            if (round > 100000) return fail(c, "the rounds do not end");
            std::vector<pgm_file_state> st((size_t)nf);
            int64_t resident = 0;
            bool left = false;
            for (int f = 0; f < nf; ++f) {
                Sim &S = F[(size_t)f];
                while (S.resident.size() < S.block && S.next < S.keys.size()) S.resident.push_back(S.keys[S.next++]);
                st[(size_t)f].open = S.next < S.keys.size();
                st[(size_t)f].has_lines = !S.resident.empty();
                st[(size_t)f].last = S.resident.empty() ? pgm_site{-1, 0} : S.resident.back();
                resident += (int64_t)S.resident.size() * line_bytes;
                left = left || !S.resident.empty();
            }
            const int64_t max_pos = pgm_max_positions(cap, fixed);
            if (max_pos < 1 || (max_pos > 1 && max_pos * fixed > cap) || (max_pos + 1) * fixed <= cap) return fail(c, "max_positions is not the budget in lines");
            pgm_site h0 = pgm_genome_end(len.data(), n_fai);       // the horizon before a dense round is cut
            for (const pgm_file_state &s : st)
                if (s.open && s.has_lines && s.last < h0) h0 = s.last;
            const pgm_round R = pgm_plan_round(st.data(), nf, len.data(), n_fai, prev, dense, max_pos);
            if (R.stalled) return fail(c, "stalled though every open file holds a line");
            if (R.horizon < prev) return fail(c, "the horizon steps back");
            int64_t consumed = 0, written = 0, bytes = 0;
            std::set<pgm_site> here;
            for (Sim &S : F)
                while (!S.resident.empty() && !(R.horizon < S.resident.front())) {
                    if (!(prev < S.resident.front())) return fail(c, "a line at or below the horizon of the round before");
                    here.insert(S.resident.front());
                    S.resident.pop_front();
                    ++consumed;
                    bytes += line_bytes;
                }
            if (dense) {
                if (R.from.scaf != R.horizon.scaf) return fail(c, "a dense round crosses a scaffold");
                for (int64_t p = R.from.pos + 1; p <= R.horizon.pos; ++p) { got.push_back(pgm_site{R.horizon.scaf, p}); ++written; }
                for (const pgm_site &k : here)
                    if (k.scaf != R.horizon.scaf || k.pos <= R.from.pos) return fail(c, "a consumed line outside the dense round's range");
            } else {
                for (const pgm_site &k : here) { got.push_back(k); ++written; }
            }
            bytes += written * fixed;
            if (dense && written * fixed > (cap > fixed ? cap : fixed)) return fail(c, "a dense round's lines exceed the output budget");
            if (dense && bytes > (cap > fixed ? cap : fixed) + resident) return fail(c, "a dense round's output exceeds the budget and the resident text");
            if (dense && written < max_pos && !(R.horizon == h0) && R.horizon.pos != len[(size_t)R.horizon.scaf])
                return fail(c, "a dense round ends before the horizon, its scaffold's end and its budget");
            if (left && consumed == 0 && !(dense && written > 0)) return fail(c, "an empty round while a file has lines left");
            ++rounds_total;
            prev = R.horizon;
            if (R.last) break;
            if (!dense && !left) return fail(c, "no line is left and the round is not the last");
        }
        for (const Sim &S : F)
            if (!S.resident.empty() || S.next < S.keys.size()) return fail(c, "lines are left behind the last round");
        if (got.size() != want.size()) return fail(c, "the rounds' sites are not the one-round answer (their number)");
        for (size_t k = 0; k < got.size(); ++k)
            if (!(got[k] == want[k])) return fail(c, "the rounds' sites are not the one-round answer");
    }
    printf("ok %d %lld\n", cases, rounds_total);
    return 0;
}
