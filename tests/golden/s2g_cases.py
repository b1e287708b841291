"""The seqToGeno.py golden cases (tests/golden/make_golden_s2g.py writes their outputs with the unmodified reference): (name, input,
argv, how).  `input` names a fixture; `how` says how the case is run for the golden: "file" (-s the file), "gz" (-s a gzipped copy),
"stdin" (no -s), "outgz" (-s the file, -g x.geno.gz: the golden is the output gunzipped), "stdout" (-s the file, no -g).  The tests
run every case every way.  The fixtures, under s2g/ (make_golden_s2g.py writes them from fixture_text()):
  wrapped.fa     descriptions behind the names, text before the first '>', lines wrapped at 60 with a short last line, blanks inside
                 sequences, an empty line inside a record, lower case / IUPAC / '-' / '*', sequences of unequal lengths (none shorter
                 than the first), a name held twice
  regular.fa     six sequences of 333 residues wrapped at 60, one ending exactly at a line's end: nothing irregular
  unwrapped.fa   four sequences of 150 residues, a line each
  tabs.fa        a tab inside a sequence (a character of it) and \\r\\n line ends (the reference's text-mode file turns them into \\n)
  single.phy     one sequential alignment
  inter.phy      one interleaved alignment whose continuation lines hold two words
  multi.phy      three alignments with their names in different orders and lengths of their own
and three of tests/golden/seq/*.out.gz, fasta and phylip as the reference's genoToSeq.py writes them."""
import gzip
import os
import random

HERE = os.path.dirname(os.path.abspath(__file__))

SEQ_INPUTS = {"seq_haplo_fasta": "haplo_cat_fasta", "seq_mixed_fasta": "mixed_ploidy_list", "seq_c1_phylip": "c1_cat_split_phylip"}

CASES = [
    ("wrapped_default", "wrapped.fa", [], "file"),
    ("wrapped_chrom", "wrapped.fa", ["-C", "chr7"], "stdin"),
    ("wrapped_contigs", "wrapped.fa", ["-M", "contigs", "-N", "ind9"], "file"),
    ("wrapped_sel", "wrapped.fa", ["-S", "s3", "s0", "s3", "dup"], "gz"),
    ("wrapped_contigs_sel", "wrapped.fa", ["-M", "contigs", "-S", "s4", "s1"], "file"),
    ("wrapped_p22", "wrapped.fa", ["-S", "s0", "s1", "s2", "s3", "-P", "2", "2"], "file"),
    ("wrapped_p121", "wrapped.fa", ["-S", "s0", "s1", "s2", "s3", "-P", "1", "2", "1"], "outgz"),
    ("regular_default", "regular.fa", [], "file"),
    ("regular_gz", "regular.fa", ["-C", "scaf_12"], "gz"),
    ("regular_stdin", "regular.fa", [], "stdin"),
    ("regular_outgz", "regular.fa", ["-f", "fasta"], "outgz"),
    ("regular_stdout", "regular.fa", ["-S", "r5", "r0"], "stdout"),
    ("regular_p222", "regular.fa", ["-P", "2", "2", "2"], "file"),
    ("regular_p1", "regular.fa", ["-P", "1", "1", "1", "1", "1", "1"], "file"),
    ("regular_p3", "regular.fa", ["-P", "3", "3"], "file"),
    ("regular_p1221", "regular.fa", ["-P", "1", "2", "2", "1"], "gz"),
    ("regular_contigs", "regular.fa", ["-M", "contigs"], "file"),
    ("regular_contigs_p2", "regular.fa", ["-M", "contigs", "-P", "2", "2", "2", "-N", "x"], "file"),
    ("unwrapped_default", "unwrapped.fa", [], "file"),
    ("unwrapped_p22", "unwrapped.fa", ["-P", "2", "2"], "stdin"),
    ("tabs_default", "tabs.fa", [], "file"),
    ("single_phylip", "single.phy", ["-f", "phylip"], "file"),
    ("single_phylip_contigs", "single.phy", ["-f", "phylip", "-M", "contigs", "-N", "me"], "stdin"),
    ("single_phylip_p2", "single.phy", ["-f", "phylip", "-P", "2", "2", "-S", "t3", "t1", "t0", "t2"], "file"),
    ("inter_phylip", "inter.phy", ["-f", "phylip", "-C", "aln"], "gz"),
    ("multi_phylip", "multi.phy", ["-f", "phylip"], "file"),
    ("multi_phylip_merge_sel", "multi.phy", ["-f", "phylip", "--merge", "-S", "m2", "m0", "-C", "chrM"], "file"),
    ("multi_phylip_contigs_ignored", "multi.phy", ["-f", "phylip", "-M", "contigs", "-N", "unused"], "outgz"),
    ("multi_phylip_p1", "multi.phy", ["-f", "phylip", "-P", "1", "1", "1"], "stdin"),
    ("seq_haplo_fasta", "seq_haplo_fasta", [], "file"),
    ("seq_mixed_fasta_contigs", "seq_mixed_fasta", ["-M", "contigs"], "gz"),
    ("seq_c1_phylip", "seq_c1_phylip", ["-f", "phylip"], "file"),
]

# the cases in which some block of the input is handed back to the host route's stripping (a blank, a tab, \r or a '>' inside a line,
# text before the first '>')
HOST_BLOCKS = {name for name, inp, _, _ in CASES if inp in ("wrapped.fa", "tabs.fa")}
# ... whose input the host route parses whole (phylip), the device emitting the lines
HOST_LOAD = {name for name, _, argv, _ in CASES if "phylip" in argv}
# ... and those the device takes whole
DEVICE = [name for name, _, _, _ in CASES if name not in HOST_BLOCKS and name not in HOST_LOAD]

# -P k for one k: held against the golden of the spelled-out list (the reference raises TypeError on it)
SINGLE_PLOIDY = [("regular.fa", ["-P", "2"], "regular_p222"), ("regular.fa", ["-P", "3"], "regular_p3"),
                 ("regular.fa", ["-M", "contigs", "-P", "2", "-N", "x"], "regular_contigs_p2")]


def _wrap(seq, width):
    return [seq[i:i + width] for i in range(0, len(seq), width)] or [""]


def fixture_text(name):
    R = random.Random(20261020)
    if name == "wrapped.fa":
        alpha = "ACGTacgtNnRYKMSW-*"
        lens = [130, 130, 180, 130, 150, 133]
        names = ["s0", "s1", "s2", "s3", "s4", "dup"]
        out = ["some text in front of the first record", "more of it"]
        for k, (n, ln) in enumerate(zip(names, lens)):
            seq = "".join(R.choice(alpha) for _ in range(ln))
            out.append(">%s description %d  of the record" % (n, k) if k % 2 == 0 else ">" + n)
            rows = _wrap(seq, 60)
            if k == 1:
                rows[1] = rows[1][:10] + " " + rows[1][10:30] + "  " + rows[1][30:]
            if k == 2:
                rows.insert(1, "")
            if k == 4:
                rows[0] = " " + rows[0] + " "
            out += rows
        out += [">dup second record of the name", "ACGT" * 50]
        return "\n".join(out) + "\n"
    if name == "regular.fa":
        out = []
        for k in range(6):
            seq = "".join(R.choice("ACGTN") for _ in range(333))
            out.append(">r%d" % k)
            out += _wrap(seq, 60) if k != 2 else _wrap(seq, 37)       # (r2 ends exactly at a line's end: 9 x 37)
        return "\n".join(out) + "\n"
    if name == "unwrapped.fa":
        return "".join(">u%d\n%s\n" % (k, "".join(R.choice("ACGT") for _ in range(150))) for k in range(4))
    if name == "tabs.fa":
        return ">a one\r\nACGT\tACGT\r\nAC\r\n>b\r\nACGTTACGTACGT\r\n>c\r\nAAAAACCCCCGG\r\n"
    if name == "single.phy":
        return " 4 70\n" + "".join("t%d   %s\n" % (k, "".join(R.choice("ACGT-N") for _ in range(70))) for k in range(4))
    if name == "inter.phy":
        seqs = ["".join(R.choice("ACGT") for _ in range(95)) for _ in range(3)]
        out = ["3 95"]
        for a in range(0, 95, 40):
            out += ["i%d %s" % (k, s[a:a + 40]) for k, s in enumerate(seqs)]
            out.append("")
        return "\n".join(out) + "\n"
    if name == "multi.phy":
        out = []
        for a, (ln, order) in enumerate([(50, [0, 1, 2]), (129, [2, 0, 1]), (7, [1, 2, 0])]):
            out.append(" 3 %d" % ln)
            out += ["m%d\t%s" % (k, "".join(R.choice("ACGTN") for _ in range(ln))) for k in order]
            out.append("")
        return "\n".join(out)
    raise KeyError(name)


FIXTURES = ["wrapped.fa", "regular.fa", "unwrapped.fa", "tabs.fa", "single.phy", "inter.phy", "multi.phy"]


def input_bytes(inp):
    """the bytes of a case's input"""
    if inp in SEQ_INPUTS:
        with gzip.open(os.path.join(HERE, "seq", SEQ_INPUTS[inp] + ".out.gz"), "rb") as f:
            return f.read()
    with open(os.path.join(HERE, "s2g", inp), "rb") as f:
        return f.read()


def golden(name):
    with gzip.open(os.path.join(HERE, "s2g", name + ".out.gz"), "rb") as f:
        return f.read()


def random_case(seed):
    """(text of a fasta or phylip file, argv) for seed: a handful of sequences of one length (now and then a longer later one, which
    is cut), wrapped at a random width or not at all, now and then with blanks, a description or text in front; a random mode, -C / -N,
    -S in an order of its own and a ploidy list that sums to the sequence count"""
    R = random.Random(seed * 104729 + 5)
    n = R.randint(1, 9)
    ln = R.choice([1, 2, 9, 10, 11, 63, 64, 99, 100, 127, 128, 129, 200, 300])
    names = ["q%d" % k for k in range(n)]
    lens = [ln + (R.randint(1, 5) if k and R.random() < 0.15 else 0) for k in range(n)]
    seqs = ["".join(R.choice("ACGTNacgt-") for _ in range(m)) for m in lens]
    phylip = R.random() < 0.25
    argv = []
    if phylip:
        argv += ["-f", "phylip"]
        n_aln = R.choice([1, 1, 2, 3])
        out = []
        for a in range(n_aln):
            order = list(range(n))
            R.shuffle(order)
            out.append("%d %d" % (n, ln))
            out += ["%s  %s" % (names[k], "".join(R.choice("ACGT") for _ in range(ln)) if a else seqs[k][:ln]) for k in order]
        text = "\n".join(out) + "\n"
        multi = n_aln > 1
    else:
        multi = False
        width = R.choice([0, 1, 7, 60, 61, 64])
        irregular = R.random() < 0.3
        out = ["junk"] if irregular and R.random() < 0.5 else []
        for k in range(n):
            out.append(">" + names[k] + (" about it" if R.random() < 0.3 else ""))
            rows = _wrap(seqs[k], width) if width else [seqs[k]]
            if irregular and R.random() < 0.5:
                j = R.randrange(len(rows))
                rows[j] = rows[j][:len(rows[j]) // 2] + " " + rows[j][len(rows[j]) // 2:]
            out += rows
        text = "\n".join(out) + ("\n" if R.random() < 0.9 else "")
    used = names
    if R.random() < 0.4:
        used = [R.choice(names) for _ in range(R.randint(1, n + 1))]
        argv += ["-S"] + used
    if R.random() < 0.4 and not multi:
        ploidy, left = [], len(used)
        while left:
            p = R.randint(1, min(left, 3))
            ploidy.append(p)
            left -= p
        argv += ["-P"] + [str(p) for p in ploidy]
    if R.random() < 0.3:
        argv += ["-M", "contigs"] + (["-N", "who"] if R.random() < 0.5 else [])
    if R.random() < 0.3:
        argv += ["-C", "chr" + str(seed)]
    if multi and R.random() < 0.5:
        argv += ["--merge"]
    return text, argv
