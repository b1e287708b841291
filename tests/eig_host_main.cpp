// pg_eig_text (genomics_general_amd/csrc/pg_eig.cpp, the host route of the genoToEigenstrat.py drop-in) on crafted blocks, as a program
// of its own for AddressSanitizer / UndefinedBehaviorSanitizer (tests/test_eig_cpu.py builds and starts it; no GPU, no Python).  Every
// block, every table and every output buffer is a heap allocation of exactly its size, so that a read or write behind it is one behind
// the allocation.
#include "../include/popgen_hip.h"

#include <algorithm>
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

// a --chromFile: scaffolds and their labels; the last label is str(nullChrom)
struct Chrom {
    std::vector<std::string> names, labels{"22"};
    void add(const std::string &n, const std::string &l) {
        names.push_back(n);
        labels.insert(labels.end() - 1, l);
    }
};

// what --cumulativePos carries from block to block
struct Carry {
    pg_eig_state st{0, 0, -1, -1, 0};
    std::vector<int64_t> offsets;
    std::string scaf;
};

struct Result {
    int rc = 0, err = 0;
    int64_t geno_len = 0, snp_len = 0, rows = 0, sites = 0, err_line = -1;
    std::string geno, snp;
};

// caps < 0: room enough
static Result run(pg_eig_cfg cfg, const std::vector<int32_t> &sel, const std::vector<int32_t> &prev, const std::vector<int32_t> &next, const Chrom &ch,
                  Carry *carry, const std::string &text, int threads, int64_t geno_cap = -1, int64_t snp_cap = -1) {
    int64_t n_lines = 1;
    for (char c : text) n_lines += c == '\n' || c == '\r';
    if (geno_cap < 0) geno_cap = n_lines * (2 * cfg.n_sel + 1);
    if (snp_cap < 0) snp_cap = n_lines * 120;
    cfg.n_scaf = (int32_t)ch.names.size();
    std::string names, labels;
    std::vector<int64_t> name_off{0}, label_off{0};
    for (const auto &n : ch.names) { names += n; name_off.push_back((int64_t)names.size()); }
    for (const auto &l : ch.labels) { labels += l; label_off.push_back((int64_t)labels.size()); }
    uint32_t mask = 3;
    while (mask + 1 < 2u * (uint32_t)cfg.n_scaf) mask = mask * 2 + 1;
    std::vector<int32_t> table((size_t)mask + 1, 0), key;
    std::vector<std::string> keys = ch.names;
    if (std::find(keys.begin(), keys.end(), ch.labels.back()) == keys.end()) keys.push_back(ch.labels.back());
    for (const auto &l : ch.labels) {
        const auto it = std::find(keys.begin(), keys.end(), l);
        key.push_back(it == keys.end() ? -1 : (int32_t)(it - keys.begin()));
    }
    Carry fresh;
    Carry &C = carry ? *carry : fresh;
    if (C.offsets.empty()) C.offsets.assign(keys.size(), 0);
    char *buf = exact(std::vector<char>(text.begin(), text.end()));
    char *geno = static_cast<char *>(std::malloc(geno_cap ? (size_t)geno_cap : 1)), *snp = static_cast<char *>(std::malloc(snp_cap ? (size_t)snp_cap : 1));
    int32_t *sel_p = exact(sel), *prev_p = exact(prev), *next_p = exact(next), *table_p = exact(table), *key_p = exact(key);
    char *names_p = exact(std::vector<char>(names.begin(), names.end())), *labels_p = exact(std::vector<char>(labels.begin(), labels.end()));
    int64_t *name_off_p = exact(name_off), *label_off_p = exact(label_off), *off_p = exact(C.offsets);
    std::vector<char> scaf(std::max(text.size(), C.scaf.size()));          // exactly the room the header asks for
    std::copy(C.scaf.begin(), C.scaf.end(), scaf.begin());
    char *scaf_p = exact(scaf);
    EXPECT(pg_gvcf_ref_table(names_p, name_off_p, cfg.n_scaf, table_p, mask) == PG_OK);
    Result r;
    r.rc = pg_eig_text(&cfg, sel_p, prev.empty() ? nullptr : prev_p, next.empty() ? nullptr : next_p, names_p, name_off_p, table_p, mask, labels_p,
                       label_off_p, key_p, &C.st, off_p, scaf_p, text.empty() ? nullptr : buf, (int64_t)text.size(), threads,
                       geno_cap ? geno : nullptr, geno_cap, snp_cap ? snp : nullptr, snp_cap, &r.geno_len, &r.snp_len, &r.rows, &r.sites,
                       &r.err_line, &r.err);
    if (r.rc == PG_OK && r.geno_len <= geno_cap && r.snp_len <= snp_cap) {
        r.geno.assign(geno, (size_t)r.geno_len);
        r.snp.assign(snp, (size_t)r.snp_len);
        C.offsets.assign(off_p, off_p + C.offsets.size());
        if (cfg.cumulative && C.st.scaf_len >= 0) C.scaf.assign(scaf_p, (size_t)C.st.scaf_len);
    }
    for (void *p : {(void *)buf, (void *)geno, (void *)snp, (void *)sel_p, (void *)prev_p, (void *)next_p, (void *)table_p, (void *)key_p, (void *)names_p,
                    (void *)labels_p, (void *)name_off_p, (void *)label_off_p, (void *)off_p, (void *)scaf_p})
        std::free(p);
    return r;
}

int main() {
    const pg_eig_cfg plain{0, 2, 4, 1, 0, 0};                     // phased, two written columns of a header of four fields, a file
    const std::vector<int32_t> ab{2, 3}, none;
    const Chrom no_file;
    Result r = run(plain, ab, none, none, no_file, nullptr, "", 1);     // an empty block
    EXPECT(r.rc == PG_OK && r.rows == 0 && r.geno_len == 0 && r.snp_len == 0 && r.err == 0 && r.err_line == -1 && r.sites == 0);
    r = run(plain, ab, none, none, no_file, nullptr, "", 1, 0, 0);      // ... and no output buffer at all
    EXPECT(r.rc == PG_OK && r.geno_len == 0);

    r = run(plain, ab, none, none, no_file, nullptr, "c\t1\tA/A\tA/T\nc\t2", 1);                 // a last line without cells (and without a line feed)
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 0 && r.sites == 2);
    EXPECT(r.geno == "01\n" && r.snp == "0\t22\t0.0\t1\tA\tT\n");
    r = run(plain, ab, none, none, no_file, nullptr, "c\t1\tA/A\tA/T\nc", 1);                    // ... of one field
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 1 && r.err_line == 1 && r.sites == 1);
    r = run(plain, ab, none, none, no_file, nullptr, "c\t1\tA/A\tA/T\n\t \r\n", 1);              // ... of blanks only
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 1 && r.err_line == 1);
    r = run(plain, ab, none, none, no_file, nullptr, "c\t1\tA/A\tT", 1);                         // a cell at the very end of the buffer
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.geno == "01\n");
    r = run(plain, ab, none, none, no_file, nullptr, "c\t1\tA/A\tT|", 1);                        // ... that ends in its phase character
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.geno == "01\n");
    r = run(plain, ab, none, none, no_file, nullptr, "c\t1\tA/A\tT|A|C|G|T|A|C|G|T|A|C|G|T|A|C|G|T", 1);   // 17 alleles: rejected
    EXPECT(r.rc == PG_OK && r.rows == 0 && r.err == 9 && r.err_line == 0);
    r = run(plain, ab, none, none, no_file, nullptr, "c\t1\tT|T|T|T|T|T|T|T|T|T|T|T\tA|A|A|A|A|A|A|A|A|A|A|A|A|A|A|A", 1);   // 16: the widest cell; a count of two characters
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.geno == "120\n");
    r = run(plain, ab, none, none, no_file, nullptr, "c\t1\tA/A\tA/T\nc\t2\tA/C\n", 1);          // a kept site whose second sample has no cell
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 4 && r.err_line == 1 && r.geno == "01\n");
    r = run(plain, ab, none, none, no_file, nullptr, "#x\nc\t1\tA/A\tA/T\n#y\n\nc", 1);          // '#' lines are no sites
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 1 && r.err_line == 3 && r.sites == 1 && r.snp == "0\t22\t0.0\t1\tA\tT\n");

    pg_eig_cfg diplo = plain;
    diplo.in_fmt = 1;
    diplo.universal_newlines = 0;
    r = run(diplo, ab, none, none, no_file, nullptr, "c\t5\tW\tN\r\nc\t6\tWW\tA\n", 1);          // stdin: \r is whitespace; a diplo cell of two bytes
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 2 && r.err_line == 1 && r.geno == "19\n");

    // a header that holds a name twice (a b a): the line too short for its last field takes the one before, counted once
    pg_eig_cfg dup = plain;
    dup.n_cols = 5;
    dup.n_sel = 3;
    r = run(dup, {4, 3, 4}, {-1, -1, -1, -1, 2}, {-1, -1, 4, -1, -1}, no_file, nullptr, "c\t1\tC/C\tA/A\tT/T\nc\t2\tC/C\tA/C\nc\t3\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 2 && r.err == 0 && r.sites == 3);
    EXPECT(r.geno == "020\n010\n" && r.snp == "0\t22\t0.0\t1\tA\tT\n1\t22\t0.0\t2\tA\tC\n");

    // a --chromFile: the longest name, a prefix of it, an unlisted scaffold
    Chrom ch;
    ch.add("c", "1");
    ch.add("longer_name", "a_label");
    r = run(plain, ab, none, none, ch, nullptr, "longer_name\t3\tA/A\tA/T\nc\t4\tT/T\tT/A\nlonger_nam\t5\tA/C\tC/C\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 3 && r.snp == "0\ta_label\t0.0\t3\tA\tT\n1\t1\t0.0\t4\tA\tT\n2\t22\t0.0\t5\tA\tC\n");

    // --cumulativePos over two blocks: the scaffold's name, its label, the position and the offsets carried
    pg_eig_cfg cum = plain;
    cum.cumulative = 1;
    Carry carry;
    r = run(cum, ab, none, none, no_file, &carry, "a_long_scaffold_name\t2\tA/A\tA/T\na_long_scaffold_name\t9\tA/A\tA/T\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 2 && carry.st.sites == 2 && carry.st.pos == 9 && carry.scaf == "a_long_scaffold_name");
    r = run(cum, ab, none, none, no_file, &carry, "a_long_scaffold_name\t12\tA/A\tA/T\nb\t1\tA/A\tA/A\nb\t3\tC/C\tA/C\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 2 && r.snp == "2\t22\t0.0\t12\tA\tT\n4\t22\t0.0\t15\tA\tC\n" && carry.scaf == "b" && carry.st.sites == 5);
    Chrom bad;                                                   // a label that is no key: the run stops at the scaffold's first kept site
    bad.add("c", "c");
    bad.add("d", "7");
    Carry carry2;
    r = run(cum, ab, none, none, bad, &carry2, "c\t2\tA/A\tA/T\nd\t1\tA/A\tA/A\nd\t2\tA/A\tA/T\nd\t3\tA/A\tA/T\n", 1);
    EXPECT(r.rc == PG_OK && r.rows == 1 && r.err == 5 && r.err_line == 2 && r.geno == "01\n" && r.snp == "0\tc\t0.0\t2\tA\tT\n");

    // output buffers one byte too small: nothing written, the sizes reported, the state as it was; with the byte: the rows
    const std::string two = "c\t1\tA/A\tA/T\nc\t2\tG/G\tG/C\n";
    const Result full = run(plain, ab, none, none, no_file, nullptr, two, 1);
    EXPECT(full.rc == PG_OK && full.rows == 2 && (int64_t)full.geno.size() == full.geno_len && (int64_t)full.snp.size() == full.snp_len);
    Carry c3;
    r = run(plain, ab, none, none, no_file, &c3, two, 1, full.geno_len - 1, full.snp_len);
    EXPECT(r.rc == PG_OK && r.geno_len == full.geno_len && r.geno.empty() && c3.st.sites == 0);
    r = run(plain, ab, none, none, no_file, &c3, two, 1, full.geno_len, full.snp_len - 1);
    EXPECT(r.rc == PG_OK && r.snp_len == full.snp_len && r.snp.empty() && c3.st.sites == 0);
    r = run(plain, ab, none, none, no_file, &c3, two, 1, full.geno_len, full.snp_len);
    EXPECT(r.rc == PG_OK && r.geno == full.geno && r.snp == full.snp && c3.st.sites == 2);

    // many lines over several threads: the same rows, and the first stopping line in input order
    std::string many;
    for (int i = 0; i < 20000; ++i) many += "c\t" + std::to_string(i + 1) + "\t" + "ACGT"[i % 4] + "/" + "ACGT"[i % 3] + "\tN/" + "ACGT"[i % 4] + "\n";
    const Result one = run(plain, ab, none, none, no_file, nullptr, many, 1), four = run(plain, ab, none, none, no_file, nullptr, many, 4);
    EXPECT(one.rc == PG_OK && one.rows > 5000 && four.rows == one.rows && one.geno == four.geno && one.snp == four.snp);
    const Result cum1 = run(cum, ab, none, none, no_file, nullptr, many, 1), cum4 = run(cum, ab, none, none, no_file, nullptr, many, 4);
    EXPECT(cum1.snp == one.snp && cum4.snp == one.snp && cum4.geno == one.geno);
    many.replace(many.find("\t15000\t") + 1, 5, "1500x");
    r = run(plain, ab, none, none, no_file, nullptr, many, 4);
    EXPECT(r.rc == PG_OK && r.err == 3 && r.err_line == 14999 && r.sites == 14999);
    EXPECT(r.snp == one.snp.substr(0, r.snp.size()) && r.geno == one.geno.substr(0, r.geno.size()) && r.snp_len == (int64_t)r.snp.size());
    r = run(cum, ab, none, none, no_file, nullptr, many, 4);
    EXPECT(r.rc == PG_OK && r.err == 3 && r.err_line == 14999 && r.snp == one.snp.substr(0, r.snp.size()) && !r.snp.empty());

    // bad arguments are refused, not followed
    int64_t a = 0, b = 0, c = 0, d = 0, el = 0;
    int e = 0;
    pg_eig_state st{0, 0, -1, -1, 0};
    const int64_t loff[2] = {0, 2};
    EXPECT(pg_eig_text(nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 3, "22", loff, nullptr, &st, nullptr, nullptr, "x", 1, 1, nullptr, 0,
                       nullptr, 0, &a, &b, &c, &d, &el, &e) == PG_ERR_ARG);
    const int32_t outside[2] = {2, 4};
    EXPECT(pg_eig_text(&plain, outside, nullptr, nullptr, nullptr, nullptr, nullptr, 3, "22", loff, nullptr, &st, nullptr, nullptr, "x", 1, 1, nullptr, 0,
                       nullptr, 0, &a, &b, &c, &d, &el, &e) == PG_ERR_ARG);

    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
