"""The filterGenotypes.py golden cases (tests/golden/make_golden_filter.py writes their outputs with the unmodified reference):
(name, fixture, argv).  @G stands for tests/golden.  randomAllele output is random in the reference: its case is checked by
membership, not byte for byte."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))

P4 = ["-p", "pop0", "-p", "pop1", "-p", "pop2", "-p", "pop3", "--popsFile", "@G/abba_pops.txt"]

CASES = [
    ("c1_default", "c1", []),
    ("c1_var", "c1", ["--minAlleles", "2", "--minCalls", "6", "--threads", "2", "--noPrecomp", "--verbose"]),
    ("c1_thin_pod", "c1", ["--thinDist", "3", "--podSize", "100"]),
    ("c1_thin_pod7", "c1", ["--thinDist", "2", "--podSize", "7", "--minCalls", "0"]),
    ("c1_coded", "c1", ["-of", "coded", "--minAlleles", "2"]),
    ("c1_count", "c1", ["-of", "count", "--samples", "s0,s2,s5,s7"]),
    ("abba_fixed", "abba", P4 + ["--fixedDiffs"]),
    ("abba_popcalls", "abba", P4 + ["--minPopCalls", "3", "--minAlleles", "2"]),
    ("abba_popalleles", "abba", P4 + ["--minPopAlleles", "1", "2", "1", "2"]),
    ("abba_maxpopalleles", "abba", P4 + ["--maxPopAlleles", "1", "--excludeSamples", "s3,s9"]),
    ("abba_nfd", "abba", P4 + ["--nearlyFixedDiff", "0.75"]),
    ("abba_freq", "abba", ["--minFreq", "0.2", "--maxFreq", "0.4"]),
    ("abba_minvar_het", "abba", ["--minVarCount", "4", "--maxHet", "0.3"]),
    ("abba_hwe_nopops", "abba", ["--HWE", "0.05", "both", "--minAlleles", "2"]),
    ("abba_exclude_alleles", "abba", ["--excludeFile", "@G/abba_exclude.txt", "-of", "alleles"]),
    ("abba_bases_freq", "abba", ["-of", "bases", "--alleleOrder", "freq", "--ploidy", "2"]),
    ("abba_alleles_freq", "abba", ["-of", "alleles", "--alleleOrder", "freq", "--keepAllSamples", "-p", "x", "s1,s2"]),
    ("abba_diplo_in", "abba_diplo", ["-if", "diplo", "--minAlleles", "2", "--maxAlleles", "2"]),
    ("abba_diplo_out", "abba", ["-of", "diplo", "--include", "chr1"]),
    ("abba_pairs_in", "abba_pairs", ["-if", "alleles", "-of", "phased", "--maxHet", "0.5"]),
    ("abba_random", "abba", ["-of", "randomAllele", "--samples", "s0,s1,s2"]),
    ("haplo_default", "haplo", ["--minAlleles", "2"]),
    ("haplo_force", "haplo", ["--ploidy", "2", "--forcePloidy", "-of", "bases"]),
    ("mixed_ploidyfile", "mixed", ["--ploidyFile", "@G/mixed_ploidy.txt", "-of", "bases", "--minCalls", "3"]),
    ("mixed_force_p2m", "mixed", ["--ploidy", "2", "--forcePloidy", "--partialToMissing", "-of", "coded"]),
    ("multi_minalleles3", "multi", ["--minAlleles", "3", "-of", "count"]),
    ("multi_maxalleles", "multi", ["--maxAlleles", "2", "--minAlleles", "2", "-of", "alleles"]),
    ("sparse_include_pops", "sparse", ["--includeFile", "@G/sparse_include.txt", "--exclude", "chr2", "-p", "north", "-p", "south",
                                        "--popsFile", "@G/sparse_pops.txt", "--minPopCalls", "2", "--thinDist", "10", "--podSize", "500"]),
    ("sparse_include_list", "sparse", ["--include", "chr3", "chr2", "--noTest", "--thinDist", "50"]),
    ("holes_mincalls0", "holes", ["--minCalls", "0", "--maxHet", "0.5"]),
    ("holes_notest", "holes", ["--noTest", "-of", "coded"]),
    ("edge_default", "edge", []),
    ("edge_mincalls0_het", "edge", ["--minCalls", "0", "--maxHet", "0.5", "--podSize", "3", "--thinDist", "2"]),
    ("edge_notest_pod3", "edge", ["--noTest", "--podSize", "3", "--thinDist", "2"]),
    ("edge_alleles", "edge", ["-of", "alleles", "--minCalls", "0"]),
    ("edge_count", "edge", ["-of", "count", "--minAlleles", "2"]),
    ("edge_force", "edge", ["--ploidy", "2", "--forcePloidy", "--minCalls", "0", "-of", "coded"]),
]


def fixture_path(name):
    if name == "edge":
        return os.path.join(HERE, "filter", "edge.geno")
    return os.path.join(HERE, name + ".geno.gz")


def random_case(seed, n_samples=None, n_lines=None):
    """(text of a .geno file, argv) for seed: regular text of diploid / haploid cells with N, '|' and leading-zero positions, and an
    option set that never reaches a line the reference raises on"""
    import random
    R = random.Random(seed)
    n = n_samples or R.randint(2, 12)
    L = n_lines if n_lines is not None else R.randint(20, 400)
    names = ["i%d" % k for k in range(n)]
    bases = "ACGT"
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    scaf, pos = 0, 0
    hap = set(R.sample(range(n), R.randint(0, min(2, n)))) if R.random() < 0.3 else set()
    for _ in range(L):
        if R.random() < 0.02:
            scaf += 1
            pos = 0
        pos += R.randint(1, 6)
        p = ("0" * R.randint(1, 2) + str(pos)) if R.random() < 0.05 else str(pos)
        a, b = R.sample(bases, 2)
        cells = []
        for k in range(n):
            if k in hap:
                cells.append(R.choice([a, b, "N"]))
                continue
            x = R.choice([a, a, a, b, "N"]) if R.random() < 0.9 else R.choice(bases)
            y = R.choice([a, a, b, b, "N"])
            if R.random() < 0.05:
                x = y = "N"
            cells.append(x + R.choice("//|") + y)
        rows.append("\t".join(["sc%d" % scaf, p] + cells))
    text = "\n".join(rows) + "\n"
    argv = []
    if R.random() < 0.5:
        argv += ["--minCalls", str(R.randint(0 if R.random() < 0.3 else 1, n))]
    if R.random() < 0.4:
        argv += ["--minAlleles", str(R.randint(1, 3))]
    if R.random() < 0.2:
        argv += ["--maxAlleles", R.choice(["1", "2", "3", "inf"])]
    if R.random() < 0.3:
        argv += ["--minVarCount", str(R.randint(0, 4))]
    if R.random() < 0.3:
        argv += ["--maxHet", R.choice(["0", "0.25", "0.5", "1"])]
    if R.random() < 0.3:
        argv += ["--minFreq", R.choice(["0", "0.1", "0.25"])]
    if R.random() < 0.3:
        argv += ["--maxFreq", R.choice(["0.3", "0.5"])]
    pops = R.random() < 0.5 and n >= 4
    if pops:
        k = R.randint(2, min(4, n // 2))
        order = R.sample(names, n)
        for j in range(k):
            argv += ["-p", "P%d" % j, ",".join(order[j::k])]
        if R.random() < 0.4:
            argv += ["--minPopCalls", str(R.randint(0, 2))]
        if R.random() < 0.3:
            argv += ["--minPopAlleles", str(R.randint(1, 2))]
        if R.random() < 0.3:
            argv += ["--maxPopAlleles", str(R.randint(1, 2))]
        if R.random() < 0.2:
            argv += ["--fixedDiffs"]
        if R.random() < 0.3:
            argv += ["--nearlyFixedDiff", R.choice(["0", "0.5", "0.9"])]
    if R.random() < 0.4:
        argv += ["--thinDist", str(R.randint(1, 8)), "--podSize", str(R.randint(1, 60))]
    if R.random() < 0.2:
        argv += ["--include"] + ["sc%d" % j for j in range(0, scaf + 1, 2)]
    if R.random() < 0.2:
        argv += ["--exclude", "sc1"]
    if R.random() < 0.1:
        argv += ["--noTest"]
    fmt = R.choice(["phased", "phased", "coded", "alleles", "count", "bases", "randomAllele"])
    if fmt == "count" and ("--noTest" in argv or "0" == (argv[argv.index("--minCalls") + 1] if "--minCalls" in argv else "1")):
        fmt = "coded"
    if fmt == "bases":
        argv += ["--ploidy", "2", "--forcePloidy"]
    if fmt in ("bases", "alleles") and R.random() < 0.5:
        argv += ["--alleleOrder", "freq"]
    return text, argv + ["-of", fmt]
