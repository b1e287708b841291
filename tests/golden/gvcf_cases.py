"""The genoToVCF.py golden cases (tests/golden/make_golden_gvcf.py writes their outputs with the unmodified reference):
(name, fixture, argv).  @G stands for tests/golden.  gvcf/ref.fa (+ .fai), gvcf/ref_nofai.fa and gvcf/ref.fa.gz hold one set of
sequences for the fixtures' scaffolds: lower-case and n bases, text before the first record, blanks inside a sequence, a record name
given twice (the last wins) and chr3 in lower case only, so that its bases never match a site's alleles.  gvcf/extra.geno: sites whose
counts tie 2-, 3- and 4-way, all-missing sites, A/N beside a reference N / n, haploid and polyploid cells, a '#' line; gvcf/dup.geno: a
header that holds a name twice."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))

REF = ["-r", "@G/gvcf/ref.fa"]
REF_NOFAI = ["-r", "@G/gvcf/ref_nofai.fa"]
REF_GZ = ["-r", "@G/gvcf/ref.fa.gz"]

CASES = [
    ("c1_phased", "c1", ["-f", "phased"]),
    ("c1_sel_repeat", "c1", ["-f", "phased", "-s", "s5,s0,s2,s5"]),
    ("c1_ref", "c1", ["-f", "phased"] + REF),
    ("abba_phased", "abba", ["-f", "phased"]),
    ("abba_ref_nofai", "abba", ["-f", "phased"] + REF_NOFAI),
    ("abba_diplo", "abba_diplo", ["-f", "diplo"]),
    ("abba_diplo_ref_gz_sel", "abba_diplo", ["-f", "diplo", "-s", "s15,s3,s4,s9"] + REF_GZ),
    ("abba_pairs", "abba_pairs", ["-f", "pairs"]),
    ("abba_pairs_ref", "abba_pairs", ["-f", "pairs"] + REF),
    ("abba_read_as_pairs", "abba", ["-f", "pairs", "-s", "s0,s1"]),
    ("haplo_phased", "haplo", ["-f", "phased"]),
    ("haplo_pairs_ref", "haplo", ["-f", "pairs"] + REF),
    ("haplo_diplo", "haplo", ["-f", "diplo", "-s", "s4_B,s0_A"]),
    ("mixed_phased", "mixed", ["-f", "phased"]),
    ("mixed_ref_sel", "mixed", ["-f", "phased", "-s", "s9,s1,s2,s1"] + REF),
    ("multi_phased", "multi", ["-f", "phased"]),
    ("multi_ref", "multi", ["-f", "phased"] + REF),
    ("multi_sel", "multi", ["-f", "phased", "-s", "s8,s7,s0"]),
    ("holes_phased", "holes", ["-f", "phased"]),
    ("holes_ref", "holes", ["-f", "phased"] + REF_NOFAI),
    ("sparse_phased", "sparse", ["-f", "phased"]),
    ("sparse_ref", "sparse", ["-f", "phased"] + REF),
    ("edge_phased", "edge", ["-f", "phased"]),
    ("edge_ref", "edge", ["-f", "phased"] + REF),
    ("edge_sel", "edge", ["-f", "phased", "-s", "d,a"]),
    ("extra_phased", "extra", ["-f", "phased"]),
    ("extra_ref", "extra", ["-f", "phased"] + REF),
    ("extra_ref_gz_sel", "extra", ["-f", "phased", "-s", "e,a"] + REF_GZ),
    ("dup_all", "dup", ["-f", "phased"]),
    ("dup_sel_ref", "dup", ["-f", "phased", "-s", "a,c,a"] + REF),
]


def fixture_path(name):
    if name == "edge":
        return os.path.join(HERE, "filter", "edge.geno")
    if name in ("extra", "dup"):
        return os.path.join(HERE, "gvcf", name + ".geno")
    return os.path.join(HERE, name + ".geno.gz")


def random_case(seed):
    """(text of a .geno file, argv, text of a fasta or None) for seed: filter_cases.random_case's file, read in a random format with a
    random selection of its samples, and a fasta over its scaffolds long enough for every site"""
    import random
    from filter_cases import random_case as filter_random_case
    text, _ = filter_random_case(seed)
    R = random.Random(seed * 7919 + 1)
    lines = text.split("\n")
    names = lines[0].split("\t")[2:]
    fmt = R.choice(["phased", "phased", "pairs", "diplo"])
    if fmt != "phased":                                     # the cells respelled: pairs "AT", diplo one IUPAC letter (haploid cells doubled)
        table = {"AA": "A", "CC": "C", "GG": "G", "TT": "T", "GT": "K", "AC": "M", "NN": "N", "CG": "S", "AG": "R", "AT": "W", "CT": "Y"}
        for k in range(1, len(lines)):
            if not lines[k]:
                continue
            f = lines[k].split("\t")
            for j in range(2, len(f)):
                pair = f[j][::2]
                if fmt == "diplo":
                    pair = pair * 2 if len(pair) == 1 else pair
                    pair = "".join(sorted(pair))
                    f[j] = table[pair] if pair in table else "N"
                else:
                    f[j] = pair
            lines[k] = "\t".join(f)
    argv = ["-f", fmt]
    if R.random() < 0.5:
        argv += ["-s", ",".join(R.choice(names) for _ in range(R.randint(1, len(names) + 1)))]
    fasta = None
    if R.random() < 0.6:
        longest = {}
        for ln in lines[1:]:
            if ln:
                f = ln.split("\t")
                longest[f[0]] = max(longest.get(f[0], 0), int(f[1]))
        recs = []
        for scaf, n in longest.items():
            seq = "".join(R.choice("ACGTACGTACGTacgtNn") for _ in range(n))
            recs.append(">%s some text\n" % scaf + "\n".join(seq[k:k + 50] for k in range(0, n, 50)) + "\n")
        fasta = "".join(recs)
    return "\n".join(lines), argv, fasta
