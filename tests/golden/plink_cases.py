"""The genoToPlink.py golden cases (tests/golden/make_golden_plink.py writes their outputs with the unmodified reference):
(name, fixture, argv).  @P stands for the output prefix, @F for the name of the .fam file; a case without --prefix runs on a copy of
its fixture and takes the reference's default prefix (the input's name up to its last dot).  The fixtures are those of eig_cases.py
and, under plink/:
  trunc.geno        cells of unequal lengths within a run (zip() cuts them to the shortest, per sample and run), a cell of an even
                    length under phased, a scaffold that comes back
  haploid_col.geno  a haploid column among diploids
  quirks.geno       positions 007, +1_0, 0 and -4, a '#' line, a line with extra cells (taken under -s only), runs of blanks and tabs
  twofield.geno     a line of two fields: its position is the first sample's genotype
  nohash.geno       a header that does not begin with '#'
A file without sites is no case: the reference dies on it (tests/test_plink_cpu.py has it among the stops)."""
import os

HERE = os.path.dirname(os.path.abspath(__file__))

P = ["--prefix", "@P"]

CASES = [
    ("c1_phased", "c1", ["-f", "phased"] + P),
    ("c1_default_prefix", "c1", []),
    ("c1_sel_fam", "c1", ["-s", "s5", "s0", "s2", "--makeFAM"] + P),
    ("c1_pairs", "c1", ["-f", "pairs"] + P),
    ("c1_alleles_sel", "c1", ["-f", "alleles", "-s", "s7", "s1"] + P),
    ("abba_phased", "abba", ["-f", "phased", "--makeFAM"] + P),
    ("abba_sel_famprefix", "abba", P + ["-s", "s15", "s3", "s4", "s9", "--makeFAM", "--FAMprefix", "@F"]),
    ("abba_diplo", "abba_diplo", ["-f", "diplo"] + P),
    ("abba_diplo_sel", "abba_diplo", ["-f", "diplo", "-s", "s1", "s15", "s2", "--makeFAM"] + P),
    ("haplo_haplo", "haplo", ["-f", "haplo"] + P),
    ("haplo_phased_sel", "haplo", ["-f", "phased", "-s", "s4_B", "s0_A"] + P),
    ("mixed_phased", "mixed", P),
    ("mixed_sel", "mixed", ["-s", "s9", "s1", "s2"] + P),
    ("mixed_alleles", "mixed", ["-f", "alleles"] + P),
    ("multi_phased", "multi", P),
    ("multi_sel", "multi", ["-s", "s8", "s7", "s0", "--makeFAM"] + P),
    ("holes_phased", "holes", P),
    ("sparse_phased", "sparse", P),
    ("sparse_pairs", "sparse", ["-f", "pairs"] + P),
    ("edge_phased", "edge", P),
    ("edge_sel", "edge", ["-s", "d", "a"] + P),
    ("edge_haplo", "edge", ["-f", "haplo"] + P),
    ("extra_sel", "extra", ["-s", "e", "a"] + P),
    ("diplo_all", "diplo", ["-f", "diplo"] + P),
    ("diplo_sel", "diplo", ["-f", "diplo", "-s", "d", "b", "--makeFAM"] + P),
    ("trunc_phased", "trunc", P),
    ("trunc_alleles", "trunc", ["-f", "alleles"] + P),
    ("trunc_sel", "trunc", ["-s", "c", "a"] + P),
    ("haploid_col", "haploid_col", P + ["--makeFAM"]),
    ("quirks_sel", "quirks", ["-s", "c", "a"] + P),
    ("twofield_sel", "twofield", ["-s", "a"] + P),
    ("nohash", "nohash", P),
    ("nohash_default_prefix", "nohash", ["--makeFAM"]),
]

OUTPUTS = ("ped", "map", "fam")

# the cases with a block the device route hands back (cells of other lengths than the first site's, positions that are no plain
# decimals, lines of another field count or with blanks)
HOST_BLOCKS = {"extra_sel", "trunc_phased", "trunc_sel", "quirks_sel", "twofield_sel"}
# ... and the one whose first site holds a cell of five alleles, more than the device takes: the host's for the whole run
HOST_WHOLE = {"trunc_alleles"}
DEVICE = [name for name, _, _ in CASES if name not in HOST_BLOCKS and name not in HOST_WHOLE]


def fixture_path(name):
    if name == "edge":
        return os.path.join(HERE, "filter", "edge.geno")
    if name == "extra":
        return os.path.join(HERE, "gvcf", "extra.geno")
    if name == "diplo":
        return os.path.join(HERE, "eig", "diplo.geno")
    if os.path.exists(os.path.join(HERE, "plink", name + ".geno")):
        return os.path.join(HERE, "plink", name + ".geno")
    return os.path.join(HERE, name + ".geno.gz")


def golden(name):
    """the outputs of a case: {"ped": bytes, "map": bytes} and, with --makeFAM, "fam" """
    import gzip
    out = {}
    for kind in OUTPUTS:
        p = os.path.join(HERE, "plink", "%s.%s.out.gz" % (name, kind))
        if os.path.exists(p):
            with gzip.open(p, "rb") as f:
                out[kind] = f.read()
    return out


def command(argv, inp, tmp, tag="out"):
    """(arguments behind -g, {kind: path of the output}) of a case run on `inp` with its outputs in the directory tmp: the default
    prefix is the input's name up to its last dot, so such a case wants `inp` inside tmp"""
    prefix = os.path.join(tmp, tag) if "--prefix" in argv else inp.rsplit(".", 1)[0]
    fam = os.path.join(tmp, tag + "_fam_file")
    outs = {"ped": prefix + ".ped", "map": prefix + ".map"}
    if "--makeFAM" in argv:
        outs["fam"] = fam if "--FAMprefix" in argv else prefix + ".fam"
    return [prefix if a == "@P" else fam if a == "@F" else a for a in argv], outs


def random_case(seed):
    """(text of a .geno file, argv, whether the reference is expected to die) for seed: filter_cases.random_case's file with some of
    its scaffolds coming back, some cells shorter or longer than their column's, read in one of the five formats (respelled as one
    IUPAC letter for diplo), a random -s in an order of its own, --makeFAM; one case in eight carries a line the reference dies on (a
    position int() does not take, a line that ends early, an extra cell without -s, a blank line) or names a sample the header lacks"""
    import random
    from filter_cases import random_case as filter_random_case
    text, _ = filter_random_case(seed)
    R = random.Random(seed * 7919 + 11)
    lines = text.split("\n")[:-1]
    names = lines[0].split("\t")[2:]
    fmt = R.choice(["phased", "phased", "diplo", "haplo", "pairs", "alleles"])
    back = R.random() < 0.5
    ragged = R.random() < 0.4 and fmt != "diplo"
    table = {"AA": "A", "CC": "C", "GG": "G", "TT": "T", "GT": "K", "AC": "M", "NN": "N", "CG": "S", "AG": "R", "AT": "W", "CT": "Y"}
    for k in range(1, len(lines)):
        f = lines[k].split("\t")
        if back and f[0] in ("sc2", "sc4"):                        # a scaffold that comes back
            f[0] = "sc0"
        for j in range(2, len(f)):
            if fmt == "diplo":
                pair = f[j][::2]
                pair = "".join(sorted(pair * 2 if len(pair) == 1 else pair))
                f[j] = table.get(pair, "N")
            elif ragged and R.random() < 0.03:
                f[j] = R.choice([f[j][:1], f[j][:2], f[j] + "|" + f[j][:1], f[j] + "/"])
        lines[k] = "\t".join(f)
    if R.random() < 0.2:
        lines.insert(R.randint(1, len(lines)), "# no site")
    argv = ["-f", fmt]
    dies = False
    if R.random() < 0.5:
        argv += ["-s"] + R.sample(names, R.randint(1, len(names)))
    if R.random() < 0.125:
        dies = True
        at = R.randint(1, len(lines) - 1)
        how = R.randrange(5)
        f = lines[at].split("\t")
        if how == 0:
            f[1] = f[1] + "x"
        elif how == 1:
            f = f[:-1] if "-s" not in argv else f[:2 + min(names.index(n) for n in argv[argv.index("-s") + 1:])]
            if len(f) == 2 and "-s" in argv and argv[argv.index("-s") + 1:] == [names[0]]:
                f = f[:1]                                          # (two fields would give the position to the first sample)
        elif how == 2:
            if "-s" in argv:
                f = [f[0]]
            else:
                f.append("A/A")
        elif how == 3:
            f = []
        else:
            argv = [a for a in argv] + (["nobody"] if "-s" in argv else ["-s", names[0], "nobody"])
        lines[at] = "\t".join(f)
    if R.random() < 0.5:
        argv += ["--makeFAM"]
    return "\n".join(lines) + "\n", argv, dies
