// pg_ped_text (genomics_general_amd/csrc/pg_ped.cpp, the host route of the genoToPlink.py drop-in) on crafted blocks, built with
// -fsanitize=address,undefined by tests/test_plink_cpu.py and run as a program of its own: every text is copied into a heap buffer of
// exactly its size, so that a read behind its end is seen.
#include "../genomics_general_amd/csrc/pg_ped_core.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

namespace {

int failures = 0;

#define CHECK(x)                                                     \
    do {                                                             \
        if (!(x)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #x);            \
            ++failures;                                              \
        }                                                            \
    } while (0)

struct Result {
    pg_ped_block B;
    int rc;
    std::string sample(int q) const { return std::string(reinterpret_cast<const char *>(B.seq) + B.seq_off[q], (size_t)(B.seq_off[q + 1] - B.seq_off[q])); }
    std::string map() const { return std::string(reinterpret_cast<const char *>(B.map), (size_t)B.map_bytes); }
};

Result run(int fmt, int n_cols, const std::vector<int32_t> &sel, bool exact, const std::string &text, int threads = 1) {
    pg_ped_cfg cfg{fmt, (int32_t)sel.size(), n_cols, exact ? 1 : 0};
    char *heap = static_cast<char *>(malloc(text.size() ? text.size() : 1));
    memcpy(heap, text.data(), text.size());
    Result R;
    R.rc = pg_ped_text(&cfg, sel.data(), heap, (int64_t)text.size(), threads, &R.B);
    free(heap);
    return R;
}

}  // namespace

int main() {
    const std::vector<int32_t> ab{2, 3}, ba{3, 2}, a{2};
    {   // an empty block; '#' lines only
        Result R = run(PGP_F_PHASED, 4, ab, true, "");
        CHECK(R.rc == PG_OK && R.B.n_sites == 0 && R.B.n_runs == 0 && R.B.err_code == 0 && R.B.seq_bytes == 0 && R.B.map_bytes == 0);
        pg_ped_free(&R.B);
        R = run(PGP_F_PHASED, 4, ab, true, "# one\n#two\tx\n");
        CHECK(R.rc == PG_OK && R.B.n_sites == 0 && R.B.n_runs == 0 && R.B.err_code == 0);
        pg_ped_free(&R.B);
        pg_ped_free(&R.B);                                                       // (a second free finds nothing)
    }
    {   // ragged cells, a scaffold that comes back, a last line without a line feed, the cell at the very end of the buffer
        Result R = run(PGP_F_PHASED, 4, ab, true, "x1\t1\tG|G\tA|A\nx1\t2\tG\tA|C\nx2\t1\tA|C\tT|T\nx1\t3\tT|T\tC|");
        CHECK(R.rc == PG_OK && R.B.err_code == 0 && R.B.n_sites == 4 && R.B.n_runs == 3);
        CHECK(R.sample(0) == "G G A C T T " && R.sample(1) == "A A A C T T C ");
        CHECK(R.map() == "x1 1 0 1\nx1 2 0 2\nx2 1 0 1\nx1 3 0 3\n");
        CHECK(R.B.run_min[0] == 1 && R.B.run_min[1] == 3 && R.B.run_min[2] == 3 && R.B.run_min[5] == 2);
        CHECK(R.B.run_start[0] == 0 && R.B.run_start[1] == 2 && R.B.run_start[2] == 3 && R.B.run_name[2] == 24 && R.B.run_name[3] == 2);
        pg_ped_free(&R.B);
        R = run(PGP_F_CHARS, 4, ba, false, "x1 1 G|G A|A extra\n# no site\n x1\t2\tG\tA|C\n");
        CHECK(R.rc == PG_OK && R.B.err_code == 0 && R.sample(0) == "A | A A | C " && R.sample(1) == "G G ");
        pg_ped_free(&R.B);
    }
    {   // -f diplo; positions int() takes; a two-field line gives its position to the first sample
        Result R = run(PGP_F_DIPLO, 4, ab, true, "c\t007\tK\tN\nc\t+1_0\tW\tY\nc\t-0\tA\tS\n");
        CHECK(R.rc == PG_OK && R.B.err_code == 0 && R.sample(0) == "G T A T A A " && R.sample(1) == "N N C T C G ");
        CHECK(R.map() == "c 7 0 7\nc 10 0 10\nc 0 0 0\n");
        pg_ped_free(&R.B);
        R = run(PGP_F_PHASED, 4, a, false, "c\t1\tA/C\tT/T\nc\t14\nc\t3\tG/G\tT/T\n");
        CHECK(R.rc == PG_OK && R.B.err_code == 0 && R.sample(0) == "A 1 G " && R.B.run_min[0] == 2);
        pg_ped_free(&R.B);
    }
    {   // every stop, at its line
        struct { int fmt; bool exact; const char *text; int code; int64_t line; } stops[] = {
            {PGP_F_PHASED, true, "c\t1\tA/A\tA/A\n\nc\t2\tA/A\tA/A\n", PGP_E_COLS, 1},
            {PGP_F_PHASED, true, "c\t1\tA/A\tA/A\nc\n", PGP_E_COLS, 1},
            {PGP_F_PHASED, true, "c\t1x\tA/A\tA/A\n", PGP_E_POS, 0},
            {PGP_F_PHASED, true, "c\t1234567890123456789\tA/A\tA/A\n", PGP_E_DIGITS, 0},
            {PGP_F_PHASED, true, "# x\nc\t1\tA/A\n", PGP_E_COUNT, 1},
            {PGP_F_PHASED, true, "c\t1\tA/A\tA/A\tA/A\n", PGP_E_COUNT, 0},
            {PGP_F_PHASED, false, "c\t1\tA/A\tA/A\tA/A\nc\t2\tA/A\n", PGP_E_SHORT, 1},
            {PGP_F_DIPLO, true, "c\t1\tA\tZ\n", PGP_E_DIPLO, 0},
            {PGP_F_DIPLO, true, "c\t1\tA\tAC\n", PGP_E_DIPLO, 0},
            {PGP_F_PHASED, true, "c\t1\tA/A\tA/\xc3\x85\n", PGP_E_ASCII, 0},
        };
        for (const auto &s : stops) {
            Result R = run(s.fmt, 4, ab, s.exact, s.text);
            CHECK(R.rc == PG_OK && R.B.err_code == s.code && R.B.err_line == s.line && R.B.seq == nullptr);
            pg_ped_free(&R.B);
        }
    }
    {   // 9 000 lines over several threads' shares: runs that cross the shares, a minimum that drops in a later share; one thread
        // and eight give the same block
        std::string text;
        for (int i = 0; i < 9000; ++i) {
            char line[96];
            snprintf(line, sizeof line, "s%d\t%d\t%s\t%s\n", i / 3500, i + 1, i == 8000 ? "A" : "A|C", i % 7 == 0 ? "G|T|T" : "G|T");
            text += line;
            if (i % 1000 == 999) text += "# between\n";
        }
        Result one = run(PGP_F_PHASED, 4, ab, true, text, 1), many = run(PGP_F_PHASED, 4, ab, true, text, 8);
        CHECK(one.rc == PG_OK && many.rc == PG_OK && one.B.n_sites == 9000 && many.B.n_sites == 9000 && one.B.n_runs == 3 && many.B.n_runs == 3);
        CHECK(one.sample(0) == many.sample(0) && one.sample(1) == many.sample(1) && one.map() == many.map());
        CHECK(many.B.seq_off[1] == 2 * (2 * 7000 + 2000) && many.B.seq_off[2] - many.B.seq_off[1] == 4 * 9000);
        CHECK(memcmp(many.B.run_min, one.B.run_min, 6 * sizeof(int32_t)) == 0 && many.B.run_min[4] == 1 && many.B.run_min[0] == 3);
        CHECK(many.sample(0).substr(2 * 2 * 7000, 6) == "A A A " && many.B.run_start[2] == 7000);
        pg_ped_free(&one.B);
        pg_ped_free(&many.B);
    }
    {   // arguments the entry point refuses
        pg_ped_cfg cfg{PGP_F_PHASED, 1, 4, 1};
        pg_ped_block B;
        const int32_t bad = 4, good = 2;
        CHECK(pg_ped_text(&cfg, &bad, "x", 1, 1, &B) == PG_ERR_ARG && pg_ped_text(&cfg, &good, nullptr, 1, 1, &B) == PG_ERR_ARG);
        CHECK(pg_ped_text(nullptr, &good, "x", 1, 1, &B) == PG_ERR_ARG && pg_ped_text(&cfg, &good, "x", 1, 1, nullptr) == PG_ERR_ARG);
    }
    if (failures) return 1;
    printf("ok\n");
    return 0;
}
