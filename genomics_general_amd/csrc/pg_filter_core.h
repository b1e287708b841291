// `.geno` sites filtered the way filterGenotypes.py filters them: the per-cell and per-site halves of the drop-in as plain functions of
// one cell / one site, written once and compiled twice -- by hipcc into k_filt_lines (pg_filter_dev.hip: a wavefront per line, a lane
// per selected column) and by the host compiler into pg_filter_text (pg_filter.cpp: the host route, every spelling line.split()
// accepts) and tests/filter_emul.cpp.
//
// What they restate:
//   Genotype.__init__ / isMissing / as*                genomics.py:317-378
//   GenomeSite.asList / alleles / hets / nonMissing    genomics.py:465-575
//   siteTest                                           genomics.py:742-799
//   the per-line loop (include/exclude, thinning)      filterGenotypes.py:24-58
// A genotype follows the Genotype rules, not the alignment rules of the analyses: it is missing when any allele is not in ACGT, its
// A/C/G/T alleles are counted as bases even then, and a character outside ACGTN leaves it without any base.  Where the reference's
// worker raises (and the reference then waits forever), these functions return a PGF_E_* code; the driver stops with the line.
#pragma once
#include <stdint.h>

#include "../../include/popgen_hip.h"

#if defined(__HIPCC__)
#define PGF_HD __host__ __device__ inline
#else
#define PGF_HD inline
#endif

#define PGF_MAXA 16          // alleles of one genotype
#define PGF_MAXPOP PG_FILTER_MAXPOP
#define PGF_CELL_MAX 192     // bytes of one rendered cell (16 alleles as "'\x01', " ...)

enum { PGF_IN_PHASED = 0, PGF_IN_DIPLO = 1, PGF_IN_ALLELES = 2 };
enum { PGF_OUT_PHASED = 0, PGF_OUT_DIPLO = 1, PGF_OUT_BASES = 2, PGF_OUT_ALLELES = 3, PGF_OUT_RANDOM = 4, PGF_OUT_CODED = 5, PGF_OUT_COUNT = 6 };

// why a line stops the run (the reference's worker raises on it)
enum {
    PGF_E_COLS = 1,        // blank line / fewer fields than a selected column needs (IndexError)
    PGF_E_PLOIDY = 2,      // ploidy mismatch without --forcePloidy (Genotype.__init__)
    PGF_E_DIPLO_IN = 3,    // -if diplo: not one of DIPLOTYPES (haplo)
    PGF_E_DIPLO_OUT = 4,   // -of diplo: not a diploid pair of PAIRS (asDiplo)
    PGF_E_HWE = 5,         // --HWE with populations: a genotype other than N/N in a population at a variable site (inHWE)
    PGF_E_NFD = 6,         // --nearlyFixedDiff with one population: np.concatenate of nothing
    PGF_E_COUNT = 7,       // -of count at a site without any base (alleles[-1] of an empty list)
    PGF_E_ORDER = 8,       // --alleleOrder freq: an allele that is not among the site's alleles (list.index)
    PGF_E_POS = 9,         // --thinDist: a position int() does not take, or one beyond 18 significant digits
    PGF_E_CELL = 10,       // a genotype of more than PGF_MAXA alleles, or non-ASCII text
    PGF_E_POPSAMPLE = 11,  // a population names a sample that is not selected, and the line reaches that population's filters (KeyError)
};

// the option set (include/popgen_hip.h), by value into the kernels
typedef pg_filter_cfg PgfConfig;

struct PgfGeno {
    int32_t n;               // alleles
    char phase;
    uint8_t bad;             // a character outside ACGTN: no base at all (numAlleles all -999)
    uint8_t missing;         // isMissing: some allele not in ACGT
    uint8_t het;             // more than one distinct allele character (N included)
    char a[PGF_MAXA];
};

// per site (or per population) sums
struct PgfCounts {
    int32_t c[4];            // A C G T
    int32_t calls;           // genotypes without a missing allele
    int32_t hets;
    int32_t not_nn;          // genotypes other than the diploid N/N (whose diplotype "N" inHWE drops)
};

PGF_HD int pgf_base(char ch) { return ch == 'A' ? 0 : ch == 'C' ? 1 : ch == 'G' ? 2 : ch == 'T' ? 3 : ch == 'N' ? 4 : -1; }

// one cell -> its Genotype (genomics.py:320-351).  ploidy < 0: none given (the cell decides)
PGF_HD int pgf_classify(const uint8_t *s, int len, int in_fmt, int ploidy, int force, int p2m, PgfGeno *g) {
    for (int k = 0; k < len; ++k)
        if (s[k] >= 0x80) return PGF_E_CELL;
    int n = 0;
    g->phase = '/';
    if (in_fmt == PGF_IN_PHASED) {
        n = (len + 1) / 2;
        if (n > PGF_MAXA) return PGF_E_CELL;
        for (int k = 0; k < n; ++k) g->a[k] = (char)s[2 * k];
        if (len > 1 && (len & 1)) g->phase = (char)s[1];
    } else if (in_fmt == PGF_IN_ALLELES) {
        n = len;
        if (n > PGF_MAXA) return PGF_E_CELL;
        for (int k = 0; k < n; ++k) g->a[k] = (char)s[k];
    } else {
        // DIPLOTYPES -> PAIRS (genomics.py:14-15)
        if (len != 1) return PGF_E_DIPLO_IN;
        const char *P;
        switch (s[0]) {
        case 'A': P = "AA"; break;
        case 'C': P = "CC"; break;
        case 'G': P = "GG"; break;
        case 'K': P = "GT"; break;
        case 'M': P = "AC"; break;
        case 'N': P = "NN"; break;
        case 'S': P = "CG"; break;
        case 'R': P = "AG"; break;
        case 'T': P = "TT"; break;
        case 'W': P = "AT"; break;
        case 'Y': P = "CT"; break;
        default: return PGF_E_DIPLO_IN;
        }
        n = 2;
        g->a[0] = P[0];
        g->a[1] = P[1];
    }
    if (ploidy >= 0) {
        if (ploidy > PGF_MAXA) return PGF_E_CELL;
        if (ploidy != n) {
            if (!force) return PGF_E_PLOIDY;
            if (ploidy > n) {
                for (int k = n; k < ploidy; ++k) g->a[k] = 'N';
            } else {
                bool same = true;
                for (int k = 1; k < n; ++k) same = same && g->a[k] == g->a[0];
                const char f = same ? g->a[0] : 'N';
                for (int k = 0; k < ploidy; ++k) g->a[k] = f;
            }
            n = ploidy;
        }
    }
    if (p2m) {
        bool anyN = false;
        for (int k = 0; k < n; ++k) anyN = anyN || g->a[k] == 'N';
        if (anyN)
            for (int k = 0; k < n; ++k) g->a[k] = 'N';
    }
    g->n = n;
    bool bad = false, miss = false, het = false;
    for (int k = 0; k < n; ++k) {
        const int b = pgf_base(g->a[k]);
        bad = bad || b < 0;
        miss = miss || b < 0 || b == 4;
        het = het || g->a[k] != g->a[0];
    }
    g->bad = bad;
    g->missing = miss;
    g->het = het;
    return 0;
}

// the genotype's share of the sums (baseFreqs / nonMissing / hets)
PGF_HD void pgf_add(const PgfGeno &g, PgfCounts *c) {
    if (!g.bad)
        for (int k = 0; k < g.n; ++k) {
            const int b = pgf_base(g.a[k]);
            if (b >= 0 && b < 4) c->c[b] += 1;
        }
    c->calls += g.missing ? 0 : 1;
    c->hets += g.het ? 1 : 0;
    c->not_nn += (g.n == 2 && g.a[0] == 'N' && g.a[1] == 'N') ? 0 : 1;
}

// numpy's argsort of the present bases' counts (int64, 2 to 4 of them), which GenomeSite.alleles(byFreq=True) reverses: numpy's small-
// array sort is NOT stable, so its answer for every pattern of ties is tabulated (generated with numpy's np.argsort on every pattern;
// the key: for value k, the number of values below it in two bits k; the entry: the permutation, index k in two bits k)
static constexpr uint8_t PGF_ARGSORT2[16] = {0x04, 0x01, 0x01, 0x01, 0x04, 0x04, 0x01, 0x01, 0x04, 0x04, 0x04, 0x01, 0x04, 0x04, 0x04, 0x04};
static constexpr uint8_t PGF_ARGSORT3[64] = {0x24, 0x09, 0x09, 0x09, 0x18, 0x12, 0x06, 0x06, 0x18, 0x12, 0x12, 0x06, 0x18, 0x12, 0x12, 0x12, 0x24, 0x21, 0x09, 0x09, 0x24, 0x24, 0x09, 0x09, 0x18, 0x18, 0x12, 0x06, 0x18, 0x18, 0x12, 0x12, 0x24, 0x21, 0x21, 0x09, 0x24, 0x24, 0x21, 0x09, 0x24, 0x24, 0x24, 0x09, 0x18, 0x18, 0x18, 0x12, 0x24, 0x21, 0x21, 0x21, 0x24, 0x24, 0x21, 0x21, 0x24, 0x24, 0x24, 0x21, 0x24, 0x24, 0x24, 0x24};
static constexpr uint8_t PGF_ARGSORT4[256] = {0xe4, 0x39, 0x39, 0x39, 0x78, 0x1b, 0x1b, 0x1b, 0x78, 0x4b, 0x1b, 0x1b, 0x78, 0x4b, 0x4b, 0x1b, 0xb4, 0x8d, 0x2d, 0x2d, 0x9c, 0x93, 0x27, 0x27, 0x6c, 0x63, 0x1b, 0x1b, 0x6c, 0x63, 0x4b, 0x1b, 0xb4, 0x8d, 0x8d, 0x2d, 0x9c, 0x93, 0x87, 0x27, 0x9c, 0x93, 0x93, 0x27, 0x6c, 0x63, 0x63, 0x1b, 0xb4, 0x8d, 0x8d, 0x8d, 0x9c, 0x93, 0x87, 0x87, 0x9c, 0x93, 0x93, 0x87, 0x9c, 0x93, 0x93, 0x93, 0xe4, 0xc9, 0x39, 0x39, 0xd8, 0xd2, 0x36, 0x36, 0x78, 0x72, 0x1e, 0x1e, 0x78, 0x72, 0x4e, 0x1e, 0xe4, 0xe1, 0x39, 0x39, 0xe4, 0xe4, 0x39, 0x39, 0x78, 0x78, 0x1b, 0x1b, 0x78, 0x78, 0x4b, 0x1b, 0xb4, 0xb1, 0x8d, 0x2d, 0xb4, 0xb4, 0x8d, 0x2d, 0x9c, 0x9c, 0x93, 0x27, 0x6c, 0x6c, 0x63, 0x1b, 0xb4, 0xb1, 0x8d, 0x8d, 0xb4, 0xb4, 0x8d, 0x8d, 0x9c, 0x9c, 0x93, 0x87, 0x9c, 0x9c, 0x93, 0x93, 0xe4, 0xc9, 0xc9, 0x39, 0xd8, 0xd2, 0xc6, 0x36, 0xd8, 0xd2, 0xd2, 0x36, 0x78, 0x72, 0x72, 0x1e, 0xe4, 0xe1, 0xc9, 0x39, 0xe4, 0xe4, 0xc9, 0x39, 0xd8, 0xd8, 0xd2, 0x36, 0x78, 0x78, 0x72, 0x1e, 0xe4, 0xe1, 0xe1, 0x39, 0xe4, 0xe4, 0xe1, 0x39, 0xe4, 0xe4, 0xe4, 0x39, 0x78, 0x78, 0x78, 0x1b, 0xb4, 0xb1, 0xb1, 0x8d, 0xb4, 0xb4, 0xb1, 0x8d, 0xb4, 0xb4, 0xb4, 0x8d, 0x9c, 0x9c, 0x9c, 0x93, 0xe4, 0xc9, 0xc9, 0xc9, 0xd8, 0xd2, 0xc6, 0xc6, 0xd8, 0xd2, 0xd2, 0xc6, 0xd8, 0xd2, 0xd2, 0xd2, 0xe4, 0xe1, 0xc9, 0xc9, 0xe4, 0xe4, 0xc9, 0xc9, 0xd8, 0xd8, 0xd2, 0xc6, 0xd8, 0xd8, 0xd2, 0xd2, 0xe4, 0xe1, 0xe1, 0xc9, 0xe4, 0xe4, 0xe1, 0xc9, 0xe4, 0xe4, 0xe4, 0xc9, 0xd8, 0xd8, 0xd8, 0xd2, 0xe4, 0xe1, 0xe1, 0xe1, 0xe4, 0xe4, 0xe1, 0xe1, 0xe4, 0xe4, 0xe4, 0xe1, 0xe4, 0xe4, 0xe4, 0xe4};

// the site's alleles by frequency (GenomeSite.alleles(byFreq=True): alleles[argsort(counts)[::-1]] over the bases present).  Returns
// their number.
PGF_HD int pgf_order(const int32_t *c, int *order) {
    int b[4], m = 0;
    for (int k = 0; k < 4; ++k)
        if (c[k] > 0) b[m++] = k;
    if (m <= 1) {
        if (m == 1) order[0] = b[0];
        return m;
    }
    int key = 0;
    for (int i = 0; i < m; ++i) {
        int below = 0;
        for (int j = 0; j < m; ++j) below += c[b[j]] < c[b[i]];
        key |= below << (2 * i);
    }
    const int perm = m == 2 ? PGF_ARGSORT2[key] : m == 3 ? PGF_ARGSORT3[key] : PGF_ARGSORT4[key];
    for (int i = 0; i < m; ++i) order[m - 1 - i] = b[(perm >> (2 * i)) & 3];
    return m;
}

PGF_HD int pgf_n_alleles(const int32_t *c) { return (c[0] > 0) + (c[1] > 0) + (c[2] > 0) + (c[3] > 0); }

// the second largest of four values (sorted(...)[-2])
PGF_HD int32_t pgf_second_i(const int32_t *c) {
    int32_t a = c[0], b = c[1];
    int32_t hi = a > b ? a : b, lo = a > b ? b : a;
    for (int k = 2; k < 4; ++k) {
        if (c[k] > hi) { lo = hi; hi = c[k]; }
        else if (c[k] > lo) lo = c[k];
    }
    return lo;
}

// siteTest (genomics.py:742-799) on the sums: tot over the selected samples, pop[k] over population k.  1 pass, 0 fail, -PGF_E_* the
// reference raises
PGF_HD int pgf_site_test(const PgfConfig &cfg, const PgfCounts &tot, const PgfCounts *pop) {
    if (tot.calls < cfg.min_calls) return 0;
    const int nA = pgf_n_alleles(tot.c);
    if (!((double)cfg.min_alleles <= (double)nA && (double)nA <= cfg.max_alleles)) return 0;
    if (nA > 1) {
        if (cfg.min_var && pgf_second_i(tot.c) < cfg.min_var) return 0;
        if (cfg.has_max_het) {
            const double h = (double)tot.hets / (double)tot.calls;      // 0/0 NaN passes, x/0 inf fails (numpy's division)
            if (h > cfg.max_het) return 0;
        }
        const int32_t n = tot.c[0] + tot.c[1] + tot.c[2] + tot.c[3];
        if (cfg.min_freq != 0.0 || cfg.max_freq != 0.0) {
            double f[4];
            for (int k = 0; k < 4; ++k) f[k] = (double)tot.c[k] / (double)n;
            double hi = f[0] > f[1] ? f[0] : f[1], lo = f[0] > f[1] ? f[1] : f[0];
            for (int k = 2; k < 4; ++k) {
                if (f[k] > hi) { lo = hi; hi = f[k]; }
                else if (f[k] > lo) lo = f[k];
            }
            if (cfg.min_freq != 0.0 && !(cfg.min_freq <= lo)) return 0;
            if (cfg.max_freq != 0.0 && !(lo <= cfg.max_freq)) return 0;
        }
        // --HWE with populations: every population is tested (an empty one is all samples).  inHWE drops the "N" diplotypes and
        // passes when none is left; any other genotype stops the reference (asDiplo raises, or the undefined `unique` is reached)
        if (cfg.hwe && cfg.n_pops > 0)
            for (int k = 0; k < cfg.n_pops; ++k) {
                if ((cfg.pop_missing >> k) & 1) return -PGF_E_POPSAMPLE;
                if ((((cfg.pop_empty >> k) & 1) ? tot : pop[k]).not_nn) return -PGF_E_HWE;
            }
    }
    if (cfg.n_pops >= 1) {
        if (cfg.has_pop_calls)
            for (int k = 0; k < cfg.n_pops; ++k) {
                if ((cfg.pop_missing >> k) & 1) return -PGF_E_POPSAMPLE;
                if (pop[k].calls < cfg.pop_calls_min[k]) return 0;
            }
        if ((cfg.fixed || cfg.has_pop_alleles || cfg.has_nfd) && cfg.pop_missing) return -PGF_E_POPSAMPLE;
        if (cfg.fixed || cfg.has_pop_alleles) {
            if (cfg.fixed) {
                bool all_one = true;
                int u = 0;
                for (int k = 0; k < cfg.n_pops; ++k) {
                    const int32_t *c = ((cfg.pop_empty >> k) & 1) ? tot.c : pop[k].c;
                    all_one = all_one && pgf_n_alleles(c) == 1;
                    for (int b = 0; b < 4; ++b) u |= (c[b] > 0) << b;
                }
                const int nu = (u & 1) + ((u >> 1) & 1) + ((u >> 2) & 1) + ((u >> 3) & 1);
                if (!(all_one && nu > 1)) return 0;
            }
            if (cfg.has_pop_alleles)
                for (int k = 0; k < cfg.n_pops; ++k) {
                    const int na = pgf_n_alleles(((cfg.pop_empty >> k) & 1) ? tot.c : pop[k].c);
                    if (!(cfg.pop_alleles_min[k] <= na && na <= cfg.pop_alleles_max[k])) return 0;
                }
        }
        if (cfg.has_nfd) {
            if (cfg.n_pops < 2) return -PGF_E_NFD;
            bool any = false;
            for (int i = 0; i < cfg.n_pops && !any; ++i)
                for (int j = i + 1; j < cfg.n_pops && !any; ++j) {
                    const int32_t *ci = ((cfg.pop_empty >> i) & 1) ? tot.c : pop[i].c;
                    const int32_t *cj = ((cfg.pop_empty >> j) & 1) ? tot.c : pop[j].c;
                    const int32_t ni = ci[0] + ci[1] + ci[2] + ci[3], nj = cj[0] + cj[1] + cj[2] + cj[3];
                    if (!ni || !nj) continue;                        // a NaN frequency satisfies nothing
                    for (int b = 0; b < 4; ++b) {
                        double d = (double)ci[b] / (double)ni - (double)cj[b] / (double)nj;
                        d = d < 0 ? -d : d;
                        if (d >= cfg.nfd) any = true;
                    }
                }
            if (!any) return 0;
        }
    }
    return 1;
}

// Python's repr() of a one-character string of ASCII (never whitespace: line.split() took that)
PGF_HD int pgf_repr(char ch, char *o) {
    const uint8_t u = (uint8_t)ch;
    if (ch == '\'') { o[0] = '"'; o[1] = '\''; o[2] = '"'; return 3; }
    if (ch == '\\') { o[0] = '\''; o[1] = '\\'; o[2] = '\\'; o[3] = '\''; return 4; }
    if (u >= 0x20 && u < 0x7f) { o[0] = '\''; o[1] = ch; o[2] = '\''; return 3; }
    const char *hx = "0123456789abcdef";
    o[0] = '\''; o[1] = '\\'; o[2] = 'x'; o[3] = hx[u >> 4]; o[4] = hx[u & 15]; o[5] = '\'';
    return 6;
}

// rank of an allele in siteAlleles + ["N"] (asList's --alleleOrder freq key); -1: not there (list.index raises)
PGF_HD int pgf_rank(char ch, const int *order, int nA) {
    const int b = pgf_base(ch);
    for (int k = 0; k < nA; ++k)
        if (order[k] == b) return k;
    return b == 4 ? nA : -1;
}

// one output cell (GenomeSite.asList(samples, mode=out_fmt, alleleOrder) -> str) into o (PGF_CELL_MAX bytes); returns its length or
// -PGF_E_*.  order / nA: the site's alleles by frequency over the selected samples.
PGF_HD int pgf_render(const PgfConfig &cfg, const PgfGeno &g, const int *order, int nA, char *o) {
    const int n = g.n;
    int L = 0;
    switch (cfg.out_fmt) {
    case PGF_OUT_PHASED:
        for (int k = 0; k < n; ++k) {
            if (k) o[L++] = g.phase;
            o[L++] = g.a[k];
        }
        return L;
    case PGF_OUT_RANDOM:                                          // the reference draws one at random; the first is one of them
        if (n < 1) return -PGF_E_CELL;
        o[0] = g.a[0];
        return 1;
    case PGF_OUT_DIPLO: {
        if (n != 2) return -PGF_E_DIPLO_OUT;
        char x = g.a[0], y = g.a[1];
        if (y < x) { const char t = x; x = y; y = t; }
        const char *PAIRS = "AACCGGGTACNNCGAGTTATCT", *DIPLO = "ACGKMNSRTWY";
        for (int k = 0; k < 11; ++k)
            if (PAIRS[2 * k] == x && PAIRS[2 * k + 1] == y) { o[0] = DIPLO[k]; return 1; }
        return -PGF_E_DIPLO_OUT;
    }
    case PGF_OUT_CODED: {
        bool ok = true;
        int code[PGF_MAXA];
        for (int k = 0; k < n; ++k) {
            const int b = pgf_base(g.a[k]);
            code[k] = -1;
            for (int j = 0; j < nA; ++j)
                if (order[j] == b) code[k] = j;
            ok = ok && code[k] >= 0;
        }
        for (int k = 0; k < n; ++k) {
            if (k) o[L++] = g.phase;
            o[L++] = ok ? (char)('0' + code[k]) : '.';
        }
        return L;
    }
    case PGF_OUT_COUNT: {
        if (nA < 1) return -PGF_E_COUNT;
        if (g.missing) { o[0] = '-'; o[1] = '1'; return 2; }
        const int t = order[nA - 1];
        int m = 0;
        for (int k = 0; k < n; ++k) m += pgf_base(g.a[k]) == t;
        if (m >= 10) { o[L++] = (char)('0' + m / 10); }
        o[L++] = (char)('0' + m % 10);
        return L;
    }
    case PGF_OUT_BASES:
    case PGF_OUT_ALLELES: {
        char s[PGF_MAXA];
        for (int k = 0; k < n; ++k) s[k] = g.a[k];
        if (cfg.freq_order) {                                      // sorted(alleles, key=siteAlleles.index): stable
            int r[PGF_MAXA];
            for (int k = 0; k < n; ++k) {
                r[k] = pgf_rank(s[k], order, nA);
                if (r[k] < 0) return -PGF_E_ORDER;
            }
            for (int i = 1; i < n; ++i) {
                const int rv = r[i];
                const char sv = s[i];
                int j = i - 1;
                while (j >= 0 && r[j] > rv) { r[j + 1] = r[j]; s[j + 1] = s[j]; --j; }
                r[j + 1] = rv;
                s[j + 1] = sv;
            }
        }
        if (cfg.out_fmt == PGF_OUT_BASES) {
            for (int k = 0; k < n; ++k) {
                if (k) o[L++] = '\t';
                o[L++] = s[k];
            }
            return L;
        }
        if (cfg.freq_order) {
            for (int k = 0; k < n; ++k) o[L++] = s[k];
            return L;
        }
        o[L++] = '(';                                              // str(tuple)
        for (int k = 0; k < n; ++k) {
            if (k) { o[L++] = ','; o[L++] = ' '; }
            L += pgf_repr(s[k], o + L);
        }
        if (n == 1) o[L++] = ',';
        o[L++] = ')';
        return L;
    }
    }
    return -PGF_E_CELL;
}

// the thinning step of one line (filterGenotypes.py:41-47, 55): state lastScaf / lastPos of the pod.  same_scaf: the line's contig
// equals lastScaf (false at the pod's first line).  Returns whether thinning keeps the line; the caller applies siteTest after it and
// pgf_thin_commit when the line is written.
PGF_HD bool pgf_thin_keep(bool same_scaf, int64_t pos, int64_t *last_pos, int64_t thin) {
    if (!same_scaf) {
        *last_pos = pos;
        return false;
    }
    return !(pos - *last_pos < thin);
}

// int(token) for the regular spelling of a position: optional sign, digits (leading zeros kept by the row, not by the value: they
// do not count towards the 18 digits); returns 0 and *v, or PGF_E_POS
PGF_HD int pgf_parse_pos(const uint8_t *s, int len, int64_t *v) {
    int k = 0;
    bool neg = false;
    if (k < len && (s[k] == '+' || s[k] == '-')) { neg = s[k] == '-'; ++k; }
    if (k >= len) return PGF_E_POS;
    while (k < len - 1 && s[k] == '0') ++k;
    if (len - k > 18) return PGF_E_POS;
    int64_t x = 0;
    for (; k < len; ++k) {
        if (s[k] < '0' || s[k] > '9') return PGF_E_POS;
        x = x * 10 + (s[k] - '0');
    }
    *v = neg ? -x : x;
    return 0;
}
