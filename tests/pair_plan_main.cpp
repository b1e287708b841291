// The plan of the pack-and-pair pass (csrc/pg_pair_plan.h) walked on the CPU over a grid of shapes, window lists, scratch limits and
// switches that straddles every boundary in it.
//   1. Every decision equals the one the library took before the plan was lifted out of pairwise_batches: argv[1] is
//      tests/golden/pair_plan/parent_decisions.txt, one line per case of make_grid(), in its order.  Columns of a line:
//        haplotypes, diploid layout, switch (without its PG_), windows, length pattern, scratch limit in MiB, worst-case XV reservation |
//        NP, NPv, dip, grp, capg, pack route, C route, D route | batches, end of the first batch,
//        FNV-1a over every batch (cut, sums, offsets, element counts of Vp / XV / pres / Cmat / Dmat, pack kernel, PG_PACK_PERM stride,
//        staging vector) and over the predicates, word_bytes, mat_bytes, target_words, multi, two_streams, n_sub
//   2. The batches tile [0, n_win) in order, none has more than 65535 windows, one of more than one window stays within its byte
//      limit (half the scratch limit when the pass is split); the staging regions follow each other and end at h_len, goff / vgoff
//      are the prefix sums, the word counters are zero and nothing is written past h_len.
//   3. pg_fuse_tasks gives every tile of the upper triangle to exactly one (wave, product), T = 1 .. 7.
// Prints "<cases> cases, 0 bad"; exit status 1 and one line per failure otherwise.
#include "../genomics_general_amd/csrc/pg_pair_plan.h"

#include <cstdio>
#include <string>
#include <vector>

struct Case {
    int n_hap;                     // haplotypes
    bool diploid;                  // every individual has two
    const char *env;               // "NAME=value" of the one switch set, or "" for none
    int n_win, pattern;
    int64_t scratch_limit;
    bool xv_worst;
};

// window lengths: uniform ones around a 32-site word, alternating ones around a group of 20 / 32 / 64 / 128 words, a mix, and
// windows around the 2^23 sites an f32 accumulator counts exactly
static int64_t pattern_len(int pattern, int k) {
    static const int64_t uniform[] = {0, 1, 31, 32, 33, 2000, 50000};
    static const int64_t mix[] = {0, 1, 31, 32, 33, 639, 641, 700, 1023, 1025, 2047, 2048, 2049, 4095, 4097, 50000};
    static const int64_t huge[] = {(1 << 23) - 1, (1 << 23) + 1, 5};
    if (pattern < 7) return uniform[pattern];
    static const int64_t group[] = {20, 32, 64, 128};
    if (pattern < 11) return group[pattern - 7] * 32 + (k & 1 ? 1 : -1);
    if (pattern == 11) return mix[k % 16];
    return huge[k % 3];
}
constexpr int N_PATTERNS = 13;

static std::vector<Case> make_grid() {
    static const char *const switches[] = {"", "PG_PAIR_VALU=1", "PG_PACK2=1", "PG_PACK_BURST=0", "PG_PACK_PERM=4", "PG_PACK_FUSE=0", "PG_PACK_FUSE=1",
                                           "PG_GROUP_WORDS=20", "PG_GROUP_WORDS=128", "PG_OVERLAP=1", "PG_OVERLAP=5", "PG_NO_DIP=1", "PG_PAIR_TILE=b",
                                           "PG_PAIR_TILE=c", "PG_PAIR_TILE=bc", "PG_PAIR_TILE=none", "PG_PACK_BLOCKS_PER_CU=2"};
    static const int units[] = {1, 32, 33, 128, 129, 224, 225, 340, 341, 512, 513, 1060, 4097};
    static const int n_wins[] = {0, 1, 7, 8, 9, 1023, 1024, 65535, 65536};
    const int64_t dflt = 48ll << 30, small = 64ll << 20;
    std::vector<Case> g;
    // every switch on every shape at the fused form's 1024 windows (diploid: NP % 64 is 0 and 32 across the units); the haploid
    // layout for the switches that look at the units
    for (const char *sw : switches)
        for (int u : units) g.push_back({2 * u, true, sw, 1024, 6, dflt, false});
    for (const char *sw : {"", "PG_PAIR_VALU=1", "PG_PACK2=1", "PG_PACK_FUSE=1", "PG_PAIR_TILE=c", "PG_PAIR_TILE=none"})
        for (int u : units) g.push_back({u, false, sw, 1024, 6, dflt, false});
    // every window count with every length pattern; fewer counts under the switches that change the pack route or the cut
    for (int n_win : n_wins)
        for (int p = 0; p < N_PATTERNS; ++p) g.push_back({258, true, "", n_win, p, dflt, false});
    for (int n_win : {1, 9, 1023, 65536})
        for (int p = 0; p < N_PATTERNS; ++p) {
            g.push_back({258, true, "PG_PACK_FUSE=1", n_win, p, dflt, false});
            g.push_back({1060, false, "PG_PACK2=1", n_win, p, dflt, false});
            g.push_back({1060, false, "PG_OVERLAP=5", n_win, p, dflt, false});
        }
    // the scratch limit and the XV reservation
    for (int64_t limit : {small, dflt})
        for (int xv = 0; xv < 2; ++xv)
            for (int u : {32, 225, 341, 4097})
                for (int n_win : {9, 1023, 65536})
                    for (const char *sw : {"", "PG_OVERLAP=1", "PG_PACK2=1"}) g.push_back({u < 4097 ? 2 * u : u, u < 4097, sw, n_win, 11, limit, xv != 0});
    // blocks x waves on both sides of 8192 and 32768: windows of one 64-word block, one wave (200 slots) and two waves (400)
    for (int waves = 1; waves <= 2; ++waves)
        for (int total : {8192, 32768})
            for (int d = -1; d <= 0; ++d)
                for (const char *sw : {"", "PG_GROUP_WORDS=128"}) g.push_back({200 * waves, true, sw, total / waves + d, 5, dflt, false});
    return g;
}

// what is decided for one case; `hash` covers every batch (cut, sums, offsets, sizes, staging vector) and, in a line, every field
struct Row {
    int NP = 0, NPv = 0, dip = 0, big_fits = 0, tile_fits = 0, fuse_fits = 0, presence = 0;
    int grp = 0, capg = 0, pack = 0, burst = 0, perm = 1, c_route = 0, d_route = 0;
    long long word_bytes = 0, mat_bytes = 0, target_words = 0;
    int multi = 0, two_streams = 0, n_sub = 0, n_batches = 0;
    long long w1 = 0;              // end of the first batch
    uint64_t hash = 1469598103934665603ull;
    void mix(uint64_t v) { hash = (hash ^ v) * 1099511628211ull; }
};

static std::string format_row(const Case &k, Row r) {
    for (long long v : {(long long)r.big_fits, (long long)r.tile_fits, (long long)r.fuse_fits, (long long)r.presence, (long long)r.burst, (long long)r.perm,
                        r.word_bytes, r.mat_bytes, r.target_words, (long long)r.multi, (long long)r.two_streams, (long long)r.n_sub})
        r.mix((uint64_t)v);
    char buf[256];
    snprintf(buf, sizeof buf, "%d %d %s %d %d %lld %d | %d %d %d %d %d %d %d %d | %d %lld %016llx", k.n_hap, (int)k.diploid, *k.env ? k.env + 3 : "-",
             k.n_win, k.pattern, (long long)(k.scratch_limit >> 20), (int)k.xv_worst, r.NP, r.NPv, r.dip, r.grp, r.capg, r.pack, r.c_route, r.d_route,
             r.n_batches, r.w1, (unsigned long long)r.hash);
    return buf;
}

static void make_windows(const Case &k, std::vector<int64_t> &lo, std::vector<int64_t> &hi) {
    lo.resize((size_t)k.n_win);
    hi.resize((size_t)k.n_win);
    int64_t at = 0;
    for (int w = 0; w < k.n_win; ++w) {
        lo[(size_t)w] = at;
        at += pattern_len(k.pattern, w);
        hi[(size_t)w] = at;
    }
}

struct EnvGuard {                  // the case's switch in the environment while it is decided
    std::string name;
    explicit EnvGuard(const char *env) {
        if (const char *eq = strchr(env, '=')) {
            name.assign(env, eq);
            setenv(name.c_str(), eq + 1, 1);
        }
    }
    ~EnvGuard() { if (!name.empty()) unsetenv(name.c_str()); }
};

static int bad = 0;
static void fail(const Case &k, const char *what, long long at) {
    std::printf("%d %d %s %d %d: %s (%lld)\n", k.n_hap, (int)k.diploid, *k.env ? k.env : "-", k.n_win, k.pattern, what, at);
    ++bad;
}

// the header's decisions for one case, and the properties of its batches that need no table
static Row decide(const Case &k, const std::vector<int64_t> &lov, const std::vector<int64_t> &hiv, std::vector<int64_t> &h) {
    Row r;
    const int64_t *lo = lov.data(), *hi = hiv.data();
    const PgPairSwitches sw = pg_pair_switches();
    const PgPairShape s = pg_pair_shape(k.n_hap, pg_plane_stride(k.n_hap, sw), pg_start_dip(k.diploid, sw));
    const PgPairPlan p = pg_plan_pair_pass(s, sw, lo, hi, k.n_win, k.scratch_limit, k.xv_worst);
    r.NP = s.NP; r.NPv = s.NPv; r.dip = s.dip;
    r.big_fits = pg_pair_big_fits(s, sw); r.tile_fits = pg_pair_tile_fits(s, sw); r.fuse_fits = pg_pack_fuse_fits(s, sw, k.n_win);
    r.presence = pg_pack_needs_presence(s.NP, sw);
    r.grp = p.grp; r.capg = p.capg; r.pack = p.pack; r.c_route = p.c_route; r.d_route = p.d_route;
    r.burst = p.pack == PG_PACK_3 && pg_pack3_burst(s.NP, sw);
    r.word_bytes = p.word_bytes; r.mat_bytes = p.mat_bytes; r.target_words = p.target_words;
    r.multi = p.multi; r.two_streams = p.two_streams; r.n_sub = p.n_sub;
    r.perm = 1;
    if (p.batch_bytes != (p.multi || p.two_streams ? k.scratch_limit / 2 : k.scratch_limit)) fail(k, "byte limit of a batch", p.batch_bytes);
    int w0 = 0;
    while (w0 < k.n_win) {
        PgBatchLayout L = pg_cut_batch(p, lo, hi, k.n_win, w0);
        const int w1 = w0 + L.nb;
        if (w1 <= w0 || w1 > k.n_win) { fail(k, "the batches do not tile the windows", w0); break; }
        if (w1 - w0 > 65535) fail(k, "more than 65535 windows in a batch", w0);
        if (L.w0 != w0) fail(k, "w0 of the layout", w0);
        if (L.nb > 1 && L.ga * p.grp * p.word_bytes + L.nb * p.mat_bytes > p.batch_bytes) fail(k, "a batch beyond its byte limit", w0);
        // regions in order, none overlapping, ending at h_len
        const size_t nb = (size_t)L.nb;
        if (L.off_hi != nb || L.off_goff != L.off_hi + nb || L.off_vgoff != L.off_goff + nb + 1 || L.off_nw != L.off_vgoff + nb + 1 ||
            L.n_nw != nb + (p.presence() ? (size_t)L.ga : 0) || L.h_len != L.off_nw + (L.n_nw + 1) / 2)
            fail(k, "staging regions", w0);
        if (h.size() < L.h_len + 1) h.resize(L.h_len + 1);
        std::fill(h.begin(), h.begin() + L.h_len + 1, -1);
        pg_batch_fill(L, p, s, lo, hi, h.data());
        if (h[L.h_len] != -1) fail(k, "the fill writes past h_len", w0);
        int64_t ga = 0, va = 0;
        for (int i = 0; i < L.nb; ++i) {
            const int64_t len = hi[w0 + i] - lo[w0 + i];
            if (h[i] != lo[w0 + i] || h[L.off_hi + i] != hi[w0 + i] || h[L.off_goff + i] != ga || h[L.off_vgoff + i] != va) fail(k, "lo / hi / prefix sums", w0 + i);
            ga += pg_window_groups(len, p.grp);
            va += ((len + 31) / 32 + 3) / 4;
        }
        if (h[L.off_goff + nb] != ga || h[L.off_vgoff + nb] != va || ga != L.ga || va != L.va) fail(k, "totals of the prefix sums", w0);
        for (size_t i = L.off_nw; i < L.h_len; ++i)
            if (h[i] != 0) fail(k, "word counters not zero", (long long)i);
        const int perm = p.pack == PG_PACK_3 ? pg_pack_perm(sw, L.nb) : 1;
        if (r.n_batches == 0) {
            r.perm = perm;
            r.w1 = w1;
        }
        for (uint64_t v : {(uint64_t)w1, (uint64_t)L.n_nw, (uint64_t)L.h_len, (uint64_t)L.ga, (uint64_t)L.va, (uint64_t)L.max_groups, (uint64_t)L.max_wds,
                           (uint64_t)L.sum_wds, (uint64_t)L.n_Vp, (uint64_t)L.n_XV, (uint64_t)L.n_pres, (uint64_t)L.n_Cmat, (uint64_t)L.n_Dmat, (uint64_t)p.pack,
                           (uint64_t)r.burst, (uint64_t)perm})
            r.mix(v);
        for (size_t i = 0; i < L.h_len; ++i) r.mix((uint64_t)h[i]);
        w0 = w1;
        ++r.n_batches;
    }
    return r;
}

// every tile of the upper triangle of T x T goes to exactly one (wave, product), and nothing outside it is marked
static int check_fuse_tasks() {
    int wrong = 0;
    for (int T = 1; T <= 7; ++T) {
        PgFuseArgs fa;
        pg_fuse_tasks(T, fa);
        int seen[7][7] = {};
        for (int w = 0; w < 8; ++w)
            for (int q = 0; q < 4; ++q)
                if (fa.mask[w] >> q & 1) {
                    const int I = fa.a[w][q], J = fa.b[w][q & 1];
                    if (I < 0 || J < 0 || I >= T || J >= T || I > J) { std::printf("pg_fuse_tasks T %d: wave %d product %d outside the triangle\n", T, w, q); ++wrong; }
                    else ++seen[I][J];
                }
        for (int I = 0; I < T; ++I)
            for (int J = I; J < T; ++J)
                if (seen[I][J] != 1) { std::printf("pg_fuse_tasks T %d: tile (%d, %d) formed %d times\n", T, I, J, seen[I][J]); ++wrong; }
    }
    return wrong;
}

int main(int argc, char **argv) {
    if (argc != 2) { std::printf("usage: pair_plan_main parent_decisions.txt\n"); return 2; }
    std::FILE *f = std::fopen(argv[1], "r");
    if (!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
    char line[1024];
    if (!std::fgets(line, sizeof line, f) || line[0] != '#') { std::printf("no header line\n"); return 2; }
    const std::vector<Case> grid = make_grid();
    std::vector<int64_t> lo, hi, h;
    int cases = 0;
    for (const Case &k : grid) {
        EnvGuard env(k.env);
        make_windows(k, lo, hi);
        const std::string got = format_row(k, decide(k, lo, hi, h));
        if (!std::fgets(line, sizeof line, f)) { fail(k, "the table ends early", cases); break; }
        line[strcspn(line, "\n")] = 0;
        if (got != line) {
            std::printf("want %s\n got %s\n", line, got.c_str());
            ++bad;
        }
        ++cases;
    }
    if (std::fgets(line, sizeof line, f)) { std::printf("the table has more lines than the grid\n"); ++bad; }
    std::fclose(f);
    bad += check_fuse_tasks();
    std::printf("%d cases, %d bad\n", cases, bad);
    return bad ? 1 : 0;
}
