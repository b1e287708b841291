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


# ---------------------------------------------------------------------------------------------------------------------------------
# edge_case: the shapes and edges where a filter goes wrong (random_case above stays as it is: the differential logs name its seeds)
# ---------------------------------------------------------------------------------------------------------------------------------
TIE_PATTERNS = {
    2: [(1, 1), (3, 3)],
    3: [(1, 1, 1), (2, 2, 1), (2, 1, 1), (1, 2, 2), (2, 1, 2), (1, 1, 2), (1, 2, 1), (3, 3, 3)],
    4: [(1, 1, 1, 1), (2, 2, 1, 1), (1, 1, 2, 2), (2, 1, 2, 1), (1, 2, 1, 2), (2, 1, 1, 2), (1, 2, 2, 1), (2, 2, 2, 1), (1, 2, 2, 2),
        (2, 1, 2, 2), (2, 2, 1, 2), (3, 1, 1, 1), (1, 3, 1, 1), (1, 1, 3, 1), (1, 1, 1, 3), (3, 2, 2, 1), (1, 2, 2, 3), (2, 3, 1, 2),
        (3, 3, 1, 2), (1, 3, 3, 2), (2, 1, 3, 3), (3, 1, 3, 2)],
}
ODD = "X-a?'\\*"          # characters outside ACGTN (a genotype holding one has no base at all)


def edge_case(seed, n_samples=None, n_lines=None, n_select=None, n_pops=None, n_listed=None, n_contigs=None, thin=None, pod=None,
              ploidy=None, over_limit=None, fmt=None, big_pos=None, shared=None, empty_pop=None, listing=None):
    """(text of a .geno file, argv, files) for seed, at the edges where the filter's rules or the device's loops go wrong:
    3- and 4-allele sites, sites whose present-allele counts tie in every pattern, haploid to 16-allele cells (--ploidyFile, @D/ploidy.txt
    in files), --forcePloidy / --partialToMissing, N and characters outside ACGTN, leading-zero and 18-digit positions, thresholds
    equal to an attainable ratio, permuted --samples / --excludeSamples / --keepAllSamples with shared and empty populations (up to 32),
    --include / --exclude lists of names that prefix each other.  argv and files name extra files as @D/<name>.

    Shape keywords pin what they name: n_select (samples picked by a permuted --samples), n_pops, n_listed (contigs listed in --include
    or --exclude), thin / pod (--thinDist / --podSize), ploidy ('none', 'file', 'force'), over_limit (a line number whose first selected
    cell gets 17 alleles -- past the drop-in's 16), fmt (-of), big_pos (18-digit positions), shared (populations that share samples,
    under --keepAllSamples or --samples), empty_pop (the last population names no sample), listing ('--include' / '--exclude').
    No option set reaches a line the reference raises on."""
    import random
    R = random.Random(seed)
    n = n_samples or R.choice([1, 2, 3, 5, 8, 12, 20, 33, 40])
    L = n_lines if n_lines is not None else R.randint(20, 250)
    names = ["e%d" % k for k in range(n)]
    argv, files = [], {}
    ploidy = ploidy or R.choice(["none", "none", "file", "force"])
    odd = R.random() < 0.3
    fmt = fmt or R.choice(["phased", "phased", "coded", "count", "alleles", "bases", "randomAllele"])
    freq_order = fmt in ("bases", "alleles") and R.random() < 0.6 and not odd
    if fmt == "bases" and ploidy == "none":
        ploidy = "force"
    if ploidy == "file":
        pl = {s: R.choice([1, 2, 2, 2, 3, 4, 6, 16]) for s in names}
        files["ploidy.txt"] = "".join("%s\t%d\n" % (s, pl[s]) for s in R.sample(names, n))
        argv += ["--ploidyFile", "@D/ploidy.txt"]
        force = R.random() < 0.4
        if force:
            argv += ["--forcePloidy"]
    elif ploidy == "force":
        pl = {s: 2 for s in names}
        argv += ["--ploidy", "2", "--forcePloidy"]
        force = True
    else:
        pl = {s: R.choice([1, 2, 2, 2, 3, 16]) if R.random() < 0.3 else 2 for s in names}
        force = False
    if R.random() < 0.25:
        argv += ["--partialToMissing"]
    in_alleles = R.random() < 0.15
    if in_alleles:
        argv += ["-if", "alleles"]
    n_contigs = n_contigs or R.choice([1, 3, 6])
    base_names = ["sc1", "sc10", "sc1x", "sc2", "sc11", "sc"]
    contigs = [base_names[k] if k < len(base_names) else "sc%d_%d" % (k, k) for k in range(n_contigs)]
    big = big_pos if big_pos is not None else R.random() < 0.15
    miss = R.choice([0.0, 0.02, 0.1, 0.3])
    patterns = [p for m in (2, 3, 4) for p in TIE_PATTERNS[m]]
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    ci, pos = 0, (10 ** 17 + R.randint(0, 10 ** 15)) if big else 0
    for i in range(L):
        if R.random() < (0.08 if n_contigs > 1 else 0.0):
            ci = (ci + 1) % n_contigs
        pos += R.choice([0, 1, 1, 2, 3, 7])
        p = str(pos)
        if R.random() < 0.05:
            p = "0" * R.randint(1, 3) + p
        m = R.choice([1, 2, 2, 3, 4])
        site = R.sample("ACGT", m)
        cells = []
        slots = None
        if R.random() < 0.25:                                      # counts in a tie pattern, scaled to the line's slots
            pat = R.choice(patterns)
            site = R.sample("ACGT", len(pat))
            slots = [b for b, c in zip(site, pat) for _ in range(c)]
            R.shuffle(slots)
        for s in names:
            k = pl[s]
            if force and R.random() < 0.15:
                k = R.choice([1, 2, 3])
            al = []
            for _ in range(k):
                if slots is not None:
                    al.append(slots.pop() if slots else "N")
                elif R.random() < miss:
                    al.append("N")
                else:
                    al.append(R.choice(site))
            if odd and R.random() < 0.03:
                al[R.randrange(k)] = R.choice(ODD)
            if R.random() < 0.03:
                al = ["N"] * k
            sep = "" if in_alleles else R.choice("/|")
            cells.append(sep.join(al))
        rows.append("\t".join([contigs[ci], p] + cells))
    argv_tail = []
    sel = list(names)
    if n_select is not None or R.random() < 0.3:
        k = n_select if n_select is not None else R.randint(1, n)
        sel = R.sample(names, k)                                   # picked from across the header, in another order
        argv += ["--samples", ",".join(sel)]
    ex = []
    if R.random() < 0.2 and len(sel) > 1:
        ex = R.sample(sel, R.randint(1, len(sel) - 1))
        argv += ["--excludeSamples", ",".join(ex)]
        sel = [s for s in sel if s not in ex]
    kp = n_pops if n_pops is not None else (R.choice([1, 2, 3, 5, 32]) if R.random() < 0.4 else 0)
    if kp:
        shared = "--samples" in argv or (shared if shared is not None else R.random() < 0.5)
        if shared and "--samples" not in argv:
            argv += ["--keepAllSamples"]
        pool = list(sel) if "--samples" in argv else list(names)
        empty = kp >= 2 and (empty_pop if empty_pop is not None else R.random() < 0.3)
        owned = []
        for j in range(kp):
            if shared:
                members = R.sample(pool, R.randint(1, len(pool)))
            else:                                                  # disjoint: the populations' samples are the selection
                members = pool[j::kp]
            if (empty and j == kp - 1) or not members:
                argv += ["-p", "P%d" % j]                         # an empty population: all samples where the reference says so
                continue
            owned += members
            argv += ["-p", "P%d" % j, ",".join(members)]
        if not shared:
            sel = [s for s in owned if s not in ex]
        if R.random() < 0.3:
            argv += ["--minPopCalls", str(R.randint(0, 2))]
        if R.random() < 0.25:
            argv += ["--minPopAlleles", str(R.randint(1, 2))]
        if R.random() < 0.25:
            argv += ["--maxPopAlleles", str(R.randint(1, 3))]
        if R.random() < 0.15:
            argv += ["--fixedDiffs"]
        if kp >= 2 and R.random() < 0.3:
            h1, h2 = R.randint(1, 8), R.randint(1, 8)
            argv += ["--nearlyFixedDiff", R.choice(["0.5", "1.0", repr(abs(R.randint(0, h1) / h1 - R.randint(0, h2) / h2))])]
    nh = 2 * max(1, len(sel))                                      # the haplotype count of a diploid, fully called line
    if R.random() < 0.4:
        argv += ["--minCalls", str(R.randint(0 if R.random() < 0.3 else 1, max(1, len(sel) // 2)))]
    if R.random() < 0.3:
        argv += ["--minAlleles", str(R.randint(1, 4))]
    if R.random() < 0.2:
        argv += ["--maxAlleles", R.choice(["2", "3", "4", "inf"])]
    if R.random() < 0.3:
        argv += ["--minVarCount", str(R.randint(1, 3))]
    if R.random() < 0.35:
        c = max(1, len(sel))
        argv += ["--maxHet", repr(R.randint(0, c) / c)]
    if R.random() < 0.35:
        argv += ["--minFreq", repr(R.randint(1, nh // 2) / nh)]
    if R.random() < 0.3:
        argv += ["--maxFreq", repr(R.randint(1, nh // 2) / nh)]
    if thin is not None or R.random() < 0.35:
        argv += ["--thinDist", str(thin if thin is not None else R.randint(1, 6))]
        argv += ["--podSize", str(pod if pod is not None else R.choice([1, 2, 3, 7, 64, 1000]))]
    elif pod is not None:
        argv += ["--podSize", str(pod)]
    nl = n_listed if n_listed is not None else (R.randint(1, 3) if R.random() < 0.3 else 0)
    if nl:
        listed = R.sample(contigs, min(nl, len(contigs)))
        listed += ["absent%d" % k for k in range(nl - len(listed))]
        R.shuffle(listed)
        argv += [listing or R.choice(["--include", "--exclude"])] + listed
    if R.random() < 0.08:
        argv += ["--noTest"]
    if fmt == "count" and ("--noTest" in argv or ("--minCalls" in argv and argv[argv.index("--minCalls") + 1] == "0")):
        fmt = "coded"
    argv_tail += ["-of", fmt]
    if freq_order:
        argv_tail += ["--alleleOrder", "freq"]
    if over_limit is not None and ploidy == "none":
        t = rows[over_limit - 1].split("\t")
        col = names.index(sel[0]) + 2 if sel else 2
        t[col] = "/".join(R.choice("ACGT") for _ in range(17))
        rows[over_limit - 1] = "\t".join(t)
    return "\n".join(rows) + "\n", argv + argv_tail, files


def edge_files(argv, files, directory):
    """write `files` into directory; argv with @D replaced by it"""
    for name, body in files.items():
        with open(os.path.join(directory, name), "w") as f:
            f.write(body)
    return [a.replace("@D", directory) for a in argv]
