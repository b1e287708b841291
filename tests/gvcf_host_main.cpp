// pg_gvcf_text (genomics_general_amd/csrc/pg_gvcf.cpp, the host route of the genoToVCF.py drop-in) on crafted blocks, as a program of
// its own for AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_gvcf_cpu.py builds and starts it; no GPU, no Python).  Every
// block, every table and every output buffer is a heap allocation of exactly its size, so that a read or write behind it is one behind
// the allocation.
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

template <class T>
static T *exact(const std::vector<T> &v) {
    T *p = static_cast<T *>(std::malloc(v.size() ? v.size() * sizeof(T) : 1));
    if (!v.empty()) std::memcpy(p, v.data(), v.size() * sizeof(T));
    return p;
}

struct Ref {
    std::string names, seq;
    std::vector<int64_t> name_off{0}, len, off;
    std::vector<int32_t> table;
    uint32_t mask = 3;
    void add(const std::string &name, const std::string &s) {
        names += name;
        name_off.push_back((int64_t)names.size());
        off.push_back((int64_t)seq.size());
        len.push_back((int64_t)s.size());
        seq += s;
    }
};

struct Result {
    int rc = 0, err = 0;
    int64_t rows_len = 0, rows = 0, err_line = -1;
    std::string out;
};

// out_cap < 0: the room the header promises to be enough
static Result run(const pg_gvcf_cfg &cfg, const std::vector<int32_t> &sel, const std::vector<int32_t> &prev, Ref *R, const std::string &text,
                  int threads, int64_t out_cap = -1) {
    int64_t n_lines = 1;
    for (char ch : text) n_lines += ch == '\n' || ch == '\r';
    if (out_cap < 0) out_cap = 3 * (int64_t)text.size() + 40 * n_lines + 64;
    char *buf = exact(std::vector<char>(text.begin(), text.end()));
    char *out = static_cast<char *>(std::malloc(out_cap ? (size_t)out_cap : 1));
    int32_t *sel_p = exact(sel), *prev_p = exact(prev);
    char *names = nullptr;
    uint8_t *seq = nullptr;
    int64_t *name_off = nullptr, *len = nullptr, *off = nullptr;
    int32_t *table = nullptr;
    int32_t n_seq = 0;
    uint32_t mask = 3;
    if (R) {
        n_seq = (int32_t)R->len.size();
        while (R->mask + 1 < 2u * (uint32_t)n_seq) R->mask = R->mask * 2 + 1;
        R->table.assign((size_t)R->mask + 1, 0);
        mask = R->mask;
        names = exact(std::vector<char>(R->names.begin(), R->names.end()));
        seq = exact(std::vector<uint8_t>(R->seq.begin(), R->seq.end()));
        name_off = exact(R->name_off);
        len = exact(R->len);
        off = exact(R->off);
        table = exact(R->table);
        EXPECT(pg_gvcf_ref_table(names, name_off, n_seq, table, mask) == PG_OK);
    }
    Result r;
    r.rc = pg_gvcf_text(&cfg, sel_p, prev.empty() ? nullptr : prev_p, names, name_off, len, off, table, mask, n_seq, seq, text.empty() ? nullptr : buf,
                        (int64_t)text.size(), threads, out_cap ? out : nullptr, out_cap, &r.rows_len, &r.rows, &r.err_line, &r.err);
    if (r.rc == PG_OK && r.rows_len <= out_cap) r.out.assign(out, (size_t)r.rows_len);
    for (void *p : {(void *)buf, (void *)out, (void *)sel_p, (void *)prev_p, (void *)names, (void *)seq, (void *)name_off, (void *)len, (void *)off, (void *)table})
        std::free(p);
    return r;
}

int main() {
    const pg_gvcf_cfg plain{0, 2, 4, 0, 1};                      // phased, two output columns of a header of four fields, no -r, a file
    const std::vector<int32_t> ab{2, 3}, none;
    Result r = run(plain, ab, none, nullptr, "", 1);             // an empty block
    EXPECT(r.rc == PG_OK && r.rows == 0 && r.rows_len == 0 && r.err == 0 && r.err_line == -1);
    r = run(plain, ab, none, nullptr, "", 1, 0);                 // ... and no output buffer at all
    EXPECT(r.rc == PG_OK && r.rows_len == 0);

    r = run(plain, ab, none, nullptr, "c\t1\tA/A\tA/T\nc\t2", 1);                         // a last line without cells (and without a line feed)
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 1 && r.err_line == 1);
    EXPECT(r.out == "c\t1\t.\tA\tT\t.\t.\t.\tGT\t0/0\t0/1\n");
    r = run(plain, ab, none, nullptr, "c\t1\tA/A\tA/T\nc", 1);                            // ... of one field
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 1 && r.err_line == 1);
    r = run(plain, ab, none, nullptr, "c\t1\tA/A\tA/T\n\t \r\n", 1);                      // ... of blanks only
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 1 && r.err_line == 1);

    r = run(plain, ab, none, nullptr, "c\t1\tA/A\tT", 1);                                 // a cell at the very end of the buffer
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 0 && r.out == "c\t1\t.\tA\tT\t.\t.\t.\tGT\t0/0\t1\n");
    r = run(plain, ab, none, nullptr, "c\t1\tA/A\tT|", 1);                                // ... that ends in its phase character
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.out == "c\t1\t.\tA\tT\t.\t.\t.\tGT\t0/0\t1\n");
    r = run(plain, ab, none, nullptr, "c\t1\tA/A\tT|A|C|G|T|A|C|G|T|A|C|G|T|A|C|G|T", 1);  // 17 alleles: rejected
    EXPECT(r.rc == PG_OK && r.rows == 0 && r.err == 9 && r.err_line == 0);
    r = run(plain, ab, none, nullptr, "c\t1\tA/A\tT|A|C|G|T|A|C|G|T|A|C|G|T|A|C|G", 1);    // 16: the widest cell
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 0);

    const pg_gvcf_cfg diplo{1, 2, 4, 0, 0};
    r = run(diplo, ab, none, nullptr, "c\t5\tW\tN\r\nc\t6\tWW\tA\n", 1);                   // stdin: \r is whitespace; a diplo cell of two bytes
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 2 && r.err_line == 1 && r.out == "c\t5\t.\tT\tA\t.\t.\t.\tGT\t1/0\t./.\n");

    // a header that holds a name twice: the line too short for its last field takes the one before
    const pg_gvcf_cfg dup{0, 1, 5, 0, 1};
    r = run(dup, {4}, {-1, -1, -1, -1, 2}, nullptr, "c\t1\tA/A\tC/C\tT/T\nc\t2\tA/A\tC/C\nc\t3\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 3 && r.err == 0);
    EXPECT(r.out == "c\t1\t.\tT\t.\t.\t.\t.\tGT\t0/0\nc\t2\t.\tA\t.\t.\t.\t.\tGT\t0/0\nc\t3\t.\tN\t.\t.\t.\t.\tGT\t.\n");

    // -r: a position at the last base of the last sequence, one behind it, below 1, a scaffold that is not there
    Ref ref;
    ref.add("c", "ACGT");
    ref.add("longer_name", "TTg");
    const pg_gvcf_cfg with_ref{0, 2, 4, 1, 1};
    r = run(with_ref, ab, none, &ref, "longer_name\t3\tN/N\tA/N\nc\t4\tT/T\tT/T\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 2 && r.err == 0);
    EXPECT(r.out == "longer_name\t3\t.\tg\tA\t.\t.\t.\tGT\t./.\t./.\n" "c\t4\t.\tT\t.\t.\t.\t.\tGT\t0/0\t0/0\n");
    r = run(with_ref, ab, none, &ref, "longer_name\t4\tN/N\tA/N\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 0 && r.err == 5 && r.err_line == 0);
    r = run(with_ref, ab, none, &ref, "c\t1\tA/A\tA/A\nc\t0\tA/A\tA/A\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 6 && r.err_line == 1);
    r = run(with_ref, ab, none, &ref, "c\t-9223372036854775808\tA/A\tA/A\n", 1);
    EXPECT(r.rc == PG_OK && r.err == 8);
    r = run(with_ref, ab, none, &ref, "cc\t1\tA/A\tA/A\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 0 && r.err == 4 && r.err_line == 0);
    r = run(with_ref, ab, none, &ref, "longer_nam\t1\tA/A\tA/A\n", 1);
    EXPECT(r.rc == PG_OK && r.err == 4);

    // an output buffer one byte too small: nothing written, the size reported; with the byte: the rows
    const std::string two = "c\t1\tA/A\tA/T\nc\t2\tG/G\tG/G\n";
    const Result full = run(plain, ab, none, nullptr, two, 1);
    EXPECT(full.rc == PG_OK && full.rows == 2 && (int64_t)full.out.size() == full.rows_len);
    r = run(plain, ab, none, nullptr, two, 1, full.rows_len - 1);
    EXPECT(r.rc == PG_OK && r.rows_len == full.rows_len && r.out.empty());
    r = run(plain, ab, none, nullptr, two, 1, full.rows_len);
    EXPECT(r.rc == PG_OK && r.out == full.out);

    // many lines over several threads: the same rows, and the first stopping line in input order
    std::string many;
    for (int i = 0; i < 20000; ++i) many += "c\t" + std::to_string(i + 1) + "\t" + "ACGT"[i % 4] + "/" + "ACGT"[i % 3] + "\tN/" + "ACGT"[i % 4] + "\n";
    const Result one = run(plain, ab, none, nullptr, many, 1), four = run(plain, ab, none, nullptr, many, 4);
    EXPECT(one.rc == PG_OK && one.rows == 20000 && four.rows == 20000 && one.out == four.out);
    many.replace(many.find("\t15000\t") + 1, 5, "1500x");
    r = run(plain, ab, none, nullptr, many, 4);
    EXPECT(r.rc == PG_OK && r.err == 3 && r.err_line == 14999);
    EXPECT(r.out == one.out.substr(0, r.out.size()) && r.rows_len == (int64_t)r.out.size());

    // bad arguments are refused, not followed
    int64_t a = 0, b = 0, c = 0;
    int e = 0;
    EXPECT(pg_gvcf_text(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 0, nullptr, "x", 1, 1, nullptr, 0, &a, &b, &c, &e) == PG_ERR_ARG);
    const int32_t outside[2] = {2, 4};
    EXPECT(pg_gvcf_text(&plain, outside, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, 0, nullptr, "x", 1, 1, nullptr, 0, &a, &b, &c, &e) == PG_ERR_ARG);

    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
