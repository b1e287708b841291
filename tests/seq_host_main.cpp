// pg_seq_text (genomics_general_amd/csrc/pg_seq.cpp, the host route of the genoToSeq.py drop-in) on crafted blocks, as a program of its
// own for AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_seq_cpu.py builds and starts it; no GPU, no Python).  Every block is
// copied into a heap buffer of exactly its size, so that a read behind the text is a read behind the allocation.
#include "../include/popgen_hip.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

static int failures = 0;

#define EXPECT(cond)                                                       \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);   \
            ++failures;                                                    \
        }                                                                  \
    } while (0)

struct Sel {
    std::vector<int32_t> col, off, len;
};

static pg_seq_block run(const pg_seq_cfg &cfg, const Sel &s, const std::string &text, int *rc) {
    char *buf = static_cast<char *>(std::malloc(text.size() ? text.size() : 1));
    std::memcpy(buf, text.data(), text.size());
    pg_seq_block b;
    *rc = pg_seq_text(&cfg, s.col.data(), s.off.data(), s.len.data(), text.empty() ? nullptr : buf, (int64_t)text.size(), &b);
    std::free(buf);
    return b;
}

static std::string seq_of(const pg_seq_block &b, int q, int n_seq) {
    if (b.stride) return std::string(reinterpret_cast<const char *>(b.seq) + (int64_t)q * b.n_sites * b.stride, (size_t)(b.n_sites * b.stride));
    const int64_t *o = b.off + (int64_t)q * (b.n_sites + 1);
    (void)n_seq;
    return std::string(reinterpret_cast<const char *>(b.seq) + o[0], (size_t)(o[b.n_sites] - o[0]));
}

int main() {
    int rc;
    // two diploid samples split into four sequences
    const pg_seq_cfg split{4, 4, 1, 0, 1};
    const Sel s4{{2, 2, 3, 3}, {0, 2, 0, 2}, {3, 3, 3, 3}};
    // the same columns copied whole
    const pg_seq_cfg whole{4, 2, 0, 1, 1};
    const Sel s2{{2, 3}, {0, 0}, {0, 0}};

    {   // an empty block
        pg_seq_block b = run(split, s4, "", &rc);
        EXPECT(rc == 0 && b.n_sites == 0 && b.n_runs == 0 && b.err_line == -1 && b.seq_bytes == 0);
        pg_seq_free(&b);
    }
    {   // a cell at the very end of the buffer (no final line feed), a '#' line, a run that changes
        pg_seq_block b = run(split, s4, "c1\t5\tA|C\tG|T\n#x\nc1\t7\tN|N\tA|A\nc2\t1\tT|T\tC|G", &rc);
        EXPECT(rc == 0 && b.n_sites == 3 && b.n_runs == 2 && b.stride == 1 && b.err_line == -1);
        EXPECT(seq_of(b, 0, 4) == "ANT" && seq_of(b, 1, 4) == "CNT" && seq_of(b, 2, 4) == "GAC" && seq_of(b, 3, 4) == "TAG");
        EXPECT(b.pos[0] == 5 && b.pos[1] == 7 && b.pos[2] == 1 && b.run_start[0] == 0 && b.run_start[1] == 2 && b.run_name[3] == 2);
        pg_seq_free(&b);
    }
    {   // the last line has no cells: the sites in front of it are complete
        pg_seq_block b = run(split, s4, "c1\t5\tA|C\tG|T\nc1\t6", &rc);
        EXPECT(rc == 0 && b.n_sites == 1 && b.err_line == 1 && b.err_code == 1 && seq_of(b, 3, 4) == "T");
        pg_seq_free(&b);
    }
    {   // a line that ends behind its second tab; a blank line; only white space
        for (const char *t : {"c1\t5\t", "\n", " \t \n", "c1\t5\tA|C\t"}) {
            pg_seq_block b = run(split, s4, t, &rc);
            EXPECT(rc == 0 && b.n_sites == 0 && b.err_line == 0 && b.err_code == 1);
            pg_seq_free(&b);
        }
    }
    {   // a cell of another length under --splitPhased; a fifth field when every column is taken
        pg_seq_block b = run(split, s4, "c1\t5\tA|C\tG|T\nc1\t6\tA|C\tG\n", &rc);
        EXPECT(rc == 0 && b.n_sites == 1 && b.err_line == 1 && b.err_code == 3 && seq_of(b, 2, 4) == "G");
        pg_seq_free(&b);
        b = run(split, s4, "c1\t5\tA|C\tG|T\tA|A\n", &rc);
        EXPECT(rc == 0 && b.n_sites == 0 && b.err_code == 2);
        pg_seq_free(&b);
    }
    {   // cells copied whole: widths that differ give offsets; runs of spaces split as tabs do; N and n become gaps
        pg_seq_block b = run(whole, s2, "c1 5  AT\tn\nc1\t+6\tN/N \tG\n", &rc);
        EXPECT(rc == 0 && b.n_sites == 2 && b.stride == 0 && b.off != nullptr && b.err_line == -1);
        EXPECT(seq_of(b, 0, 2) == "AT-/-" && seq_of(b, 1, 2) == "-G" && b.pos[1] == 6);
        EXPECT(b.off[1] - b.off[0] == 2 && b.off[2] - b.off[1] == 3);
        pg_seq_free(&b);
        b = run(whole, s2, "c1\t5\tAT\tnn\nc1\t6\tNN\tGG\n", &rc);
        EXPECT(rc == 0 && b.stride == 2 && b.off == nullptr && seq_of(b, 1, 2) == "--GG");
        pg_seq_free(&b);
    }
    {   // positions: 18 digits are taken, 19 are not, nor is text; bytes that are not ASCII
        pg_seq_block b = run(whole, s2, "c1\t999999999999999999\tA\tC\nc1\t1000000000000000000\tA\tC\n", &rc);
        EXPECT(rc == 0 && b.n_sites == 1 && b.pos[0] == 999999999999999999ll && b.err_line == 1 && b.err_code == 4);
        pg_seq_free(&b);
        b = run(whole, s2, "c1\tx\tA\tC\n", &rc);
        EXPECT(rc == 0 && b.err_code == 4);
        pg_seq_free(&b);
        b = run(whole, s2, "c1\t5\tA\t\xc3\xa9\n", &rc);
        EXPECT(rc == 0 && b.err_code == 5);
        pg_seq_free(&b);
    }
    {   // tables that point outside the header are refused
        const Sel bad{{2, 4}, {0, 0}, {0, 0}};
        pg_seq_block b;
        EXPECT(pg_seq_text(&whole, bad.col.data(), bad.off.data(), bad.len.data(), "x", 1, &b) == PG_ERR_ARG);
        const Sel bad2{{2, 3, 3, 3}, {0, 2, 0, 4}, {3, 3, 3, 3}};
        EXPECT(pg_seq_text(&split, bad2.col.data(), bad2.off.data(), bad2.len.data(), "x", 1, &b) == PG_ERR_ARG);
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
