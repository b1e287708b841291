"""The genoToEigenstrat.py golden cases (tests/golden/make_golden_eig.py writes their outputs with the unmodified reference):
(name, fixture, argv).  @G stands for tests/golden.  The fixtures are those of gvcf_cases.py and, under eig/:
  quirks.geno       a header that does not begin with '#'; counts that tie, three and four alleles, monomorphic and all-missing sites,
                    C/N and C/X, lower case, haploid and polyploid cells, positions 007, +1_0, 0 and -4, extra cells, a two-field
                    line, a '#' line, cells of ten alleles and more (a count of 11)
  ragged.geno       lines that end before the header does (a kept site the selected samples still have cells at)
  dup.geno          a header that holds a name twice
  cumul_a.geno      three scaffolds that end on kept sites, the first coming back        (--cumulativePos)
  cumul_b.geno      scaffolds that end and begin on sites that are not kept, one without any kept site
  diplo.geno        -f diplo with every letter
  header_only.geno  no site
  chrom.txt         a --chromFile: x1 twice (the later wins), blanks and tabs, a long label; chr3, x2, s2, sc* unlisted
  chrom_cumul.txt   a --chromFile whose labels are scaffold names of the file or the default nullChrom, as --cumulativePos needs"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))

CHROM = ["--chromFile", "@G/eig/chrom.txt"]
CHROM_CUMUL = ["--chromFile", "@G/eig/chrom_cumul.txt"]

CASES = [
    ("c1_phased", "c1", ["-f", "phased"]),
    ("c1_sel_unknown", "c1", ["-f", "phased", "-s", "s5,nobody,s0,s2"]),
    ("c1_chrom", "c1", ["-f", "phased"] + CHROM),
    ("abba_phased", "abba", ["-f", "phased"]),
    ("abba_null0", "abba", ["-f", "phased", "--nullChrom", "0", "-s", "s15,s3,s4,s9"]),
    ("abba_diplo", "abba_diplo", ["-f", "diplo"]),
    ("abba_diplo_sel_chrom", "abba_diplo", ["-f", "diplo", "-s", "s1,s2,s17"] + CHROM),
    ("haplo_phased", "haplo", ["-f", "phased"]),
    ("haplo_sel", "haplo", ["-f", "phased", "-s", "s4_B,s0_A"]),
    ("mixed_phased", "mixed", ["-f", "phased"]),
    ("mixed_cumul", "mixed", ["-f", "phased", "--cumulativePos"]),
    ("mixed_cumul_chrom", "mixed", ["-f", "phased", "--cumulativePos", "-s", "s9,s1,s2"] + CHROM_CUMUL),
    ("multi_phased", "multi", ["-f", "phased"]),
    ("multi_sel", "multi", ["-f", "phased", "-s", "s8,s7,s0"]),
    ("holes_phased", "holes", ["-f", "phased"]),
    ("sparse_phased", "sparse", ["-f", "phased"]),
    ("sparse_chrom", "sparse", ["-f", "phased", "--nullChrom", "-3"] + CHROM),
    ("sparse_cumul", "sparse", ["-f", "phased", "--cumulativePos", "--nullChrom", "0"]),
    ("edge_phased", "edge", ["-f", "phased"]),
    ("edge_sel_chrom", "edge", ["-f", "phased", "-s", "d,a"] + CHROM),
    ("extra_phased", "extra", ["-f", "phased"]),
    ("extra_sel_chrom", "extra", ["-f", "phased", "-s", "e,a"] + CHROM),
    ("quirks_phased", "quirks", ["-f", "phased"]),
    ("quirks_sel", "quirks", ["-f", "phased", "-s", "e,b,zz"]),
    ("quirks_chrom_null0", "quirks", ["-f", "phased", "--nullChrom", "0"] + CHROM),
    ("quirks_cumul", "quirks", ["-f", "phased", "--cumulativePos"]),
    ("ragged_sel", "ragged", ["-f", "phased", "-s", "a,b"]),
    ("dup_all", "dup", ["-f", "phased"]),
    ("dup_sel", "dup", ["-f", "phased", "-s", "c,a"]),
    ("gdup_all", "gdup", ["-f", "phased"]),
    ("cumul_a", "cumul_a", ["-f", "phased", "--cumulativePos"]),
    ("cumul_a_chrom", "cumul_a", ["-f", "phased", "--cumulativePos"] + CHROM_CUMUL),
    ("cumul_a_plain", "cumul_a", ["-f", "phased"] + CHROM_CUMUL),
    ("cumul_b", "cumul_b", ["-f", "phased", "--cumulativePos"]),
    ("cumul_b_chrom", "cumul_b", ["-f", "phased", "--cumulativePos", "-s", "b"] + CHROM_CUMUL),
    ("diplo_all", "diplo", ["-f", "diplo"]),
    ("diplo_sel_chrom", "diplo", ["-f", "diplo", "-s", "d,b"] + CHROM),
    ("header_only", "header_only", ["-f", "phased"]),
]

OUTPUTS = ("geno", "snp", "ind")

# what the device route hands to the host for the whole run
HOST_WHOLE = {"dup_all", "dup_sel", "gdup_all"} | {name for name, _, argv in CASES if "--cumulativePos" in argv}
# ... and the cases with a block that it hands back ('#' lines, irregular positions, short and long lines, cells of ten alleles) or
# without any block
HOST_BLOCKS = {"extra_phased", "extra_sel_chrom", "quirks_phased", "quirks_sel", "quirks_chrom_null0", "ragged_sel", "header_only"}
DEVICE = [name for name, _, _ in CASES if name not in HOST_WHOLE and name not in HOST_BLOCKS]


def fixture_path(name):
    if name == "edge":
        return os.path.join(HERE, "filter", "edge.geno")
    if name == "extra":
        return os.path.join(HERE, "gvcf", "extra.geno")
    if name == "gdup":
        return os.path.join(HERE, "gvcf", "dup.geno")
    if os.path.exists(os.path.join(HERE, "eig", name + ".geno")):
        return os.path.join(HERE, "eig", name + ".geno")
    return os.path.join(HERE, name + ".geno.gz")


def golden(name):
    """the three outputs of a case: {"geno": bytes, "snp": bytes, "ind": bytes}"""
    import gzip
    out = {}
    for kind in OUTPUTS:
        with gzip.open(os.path.join(HERE, "eig", "%s.%s.out.gz" % (name, kind)), "rb") as f:
            out[kind] = f.read()
    return out


def random_case(seed):
    """(text of a .geno file, argv, text of a --chromFile or None) for seed: filter_cases.random_case's file, read as phased or
    respelled as diplo, with a random selection of its samples, a --chromFile over some of its scaffolds, --nullChrom and -- where
    the reference survives it -- --cumulativePos"""
    import random
    from filter_cases import random_case as filter_random_case
    text, _ = filter_random_case(seed)
    R = random.Random(seed * 104729 + 3)
    lines = text.split("\n")
    names = lines[0].split("\t")[2:]
    fmt = R.choice(["phased", "phased", "phased", "diplo"])
    if fmt == "diplo":                                      # the cells respelled as one IUPAC letter (haploid cells doubled)
        table = {"AA": "A", "CC": "C", "GG": "G", "TT": "T", "GT": "K", "AC": "M", "NN": "N", "CG": "S", "AG": "R", "AT": "W", "CT": "Y"}
        for k in range(1, len(lines)):
            if not lines[k]:
                continue
            f = lines[k].split("\t")
            for j in range(2, len(f)):
                pair = f[j][::2]
                pair = pair * 2 if len(pair) == 1 else pair
                pair = "".join(sorted(pair))
                f[j] = table[pair] if pair in table else "N"
            lines[k] = "\t".join(f)
    argv = ["-f", fmt]
    if R.random() < 0.5:
        argv += ["-s", ",".join(R.choice(names + ["nobody"]) for _ in range(R.randint(1, len(names) + 1)))]
        if all(n == "nobody" for n in argv[-1].split(",")):
            argv[-1] = names[0]
    if R.random() < 0.4:
        argv += ["--nullChrom", str(R.choice([0, 1, 23, -1, 100]))]
    scafs = list(dict.fromkeys(ln.split("\t")[0] for ln in lines[1:] if ln and not ln.startswith("#")))
    chrom = None
    cumulative = R.random() < 0.35
    if R.random() < 0.6 and scafs:
        listed = [s for s in scafs if R.random() < 0.7] or scafs[:1]
        null = argv[argv.index("--nullChrom") + 1] if "--nullChrom" in argv else "22"
        rows = []
        for s in listed:
            # with --cumulativePos the reference survives only labels that are listed scaffolds or nullChrom
            label = R.choice(listed + [null]) if cumulative else R.choice(["1", "2", "X", "chrom_%s" % s, null])
            rows.append("%s%s%s\n" % (s, R.choice(["\t", " ", "  \t"]), label))
        if R.random() < 0.3:
            rows.append(rows[0].split()[0] + "\t" + (listed[0] if cumulative else "9") + "\n")     # a scaffold listed twice
        chrom = "".join(rows)
    if cumulative:
        argv += ["--cumulativePos"]
    return "\n".join(lines), argv, chrom
