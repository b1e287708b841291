"""genoToSeq.py goldens: the fixture written for them, the command lines, and how a run's output is read back
(tests/golden/make_golden_seq.py runs the unmodified reference on them; tests/test_seq_cpu.py, tests/test_seq_emul.py and
tests/test_gpu_seq.py compare byte for byte).

{geno}: the case's fixture.  `out` says where the alignments go and what the golden tests/golden/seq/<name>.out.gz holds, gzipped:
  "stdout"  no -s: the standard output
  "file"    -s <tmp>/out: that file
  "gz"      -s <tmp>/out.gz: that file, gunzipped
  "gzflag"  -s <tmp>/out --gzip: <tmp>/out.gz, gunzipped
  "sep"     -s <tmp>/out --separateFiles: every file written, in the order of their names, as `== <name>` and its content
            (gunzipped when the name ends in .gz)"""
import gzip
import os

# cells the resident 4-bit codes do not keep (IUPAC codes, lower case, '-', '*'), a two-character cell, lines that begin with '#' in
# mid-file, scaffold and position fields of several widths
SEQ_FIXTURE = "seqmix"
SEQ_FIXTURE_HEADER = ["scaffold", "position", "ind1", "ind2", "x", "a_long_sample_name", "ind5"]


def seq_fixture_lines():
    """the data lines of seqmix.geno.gz: (scaffold, position, cells) or a comment line"""
    alphabet = ["A", "C", "G", "T", "N", "n", "R", "Y", "-", "*", "a", "k"]
    lines = []
    state = 20261019
    for scaf, n, step in (("sc1", 40, 7), ("scaffold_22", 35, 13), ("Z", 30, 101)):
        pos = 0
        for i in range(n):
            cells = []
            for k in range(5):
                state = (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
                cells.append(alphabet[(state >> 33) % len(alphabet)])
            state = (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
            pos += 1 + (state >> 40) % step
            if i % 11 == 5:
                cells[(i // 11) % 5] = "AT"                    # a two-character cell: two bytes of that sequence at this site
            lines.append((scaf, pos, cells))
            if scaf == "scaffold_22" and i in (0, 17):
                lines.append("#a comment in mid-file\tit has\tfields of its own")
    return lines


MIXED_PLOIDY = ["2", "1", "2", "2", "2", "2", "1", "2", "2", "1"]
HAPLO_WIN = ["-M", "windows", "--windType", "coordinate"]
SITES = ["-M", "windows", "--windType", "sites"]

SEQ_CASES = [
    # cat (-S keeps the goldens small where the case is not about the number of sequences)
    dict(name="multi_cat_unsplit_phased", fixture="multi", out="stdout", argv=["-g", "{geno}", "-S", "s0,s4"]),
    dict(name="c1_cat_split_phylip", fixture="c1", out="file", argv=["-g", "{geno}", "--splitPhased", "-f", "phylip", "-S", "s6,s1"]),
    dict(name="haplo_cat_fasta", fixture="haplo", out="stdout", argv=["-g", "{geno}", "-f", "fasta"]),
    dict(name="sparse_samples_reordered", fixture="sparse", out="file", argv=["-g", "{geno}", "--splitPhased", "-S", "s5,s2,s9", "-f", "phylip"]),
    dict(name="haplo_samples_repeated", fixture="haplo", out="file", argv=["-g", "{geno}", "-S", "s1_A,s0_B,s1_A"]),
    dict(name="diplo_samples_subset", fixture="abba_diplo", out="file", argv=["-g", "{geno}", "-S", "s3,s0"]),
    dict(name="seqmix_cat", fixture="seqmix", out="file", argv=["-g", "{geno}"]),
    dict(name="seqmix_ntogap_phylip", fixture="seqmix", out="file", argv=["-g", "{geno}", "--NtoGap", "-f", "phylip"]),
    dict(name="mixed_ploidy_list", fixture="mixed", out="file", argv=["-g", "{geno}", "--splitPhased", "-S", "s0,s1,s2", "--ploidy"] + MIXED_PLOIDY),
    dict(name="haplo_ploidy1_names_unchanged", fixture="haplo", out="file", argv=["-g", "{geno}", "--splitPhased", "--ploidy", "1", "-S", "s0_A,s1_B"]),
    dict(name="haplo_cat_seqnameformat_ignored", fixture="haplo", out="file",
         argv=["-g", "{geno}", "--seqNameFormat", "contig_position", "-f", "phylip", "-S", "s2_A,s2_B"]),
    dict(name="haplo_out_gz", fixture="haplo", out="gz", argv=["-g", "{geno}", "-S", "s4_B,s3_A"]),
    dict(name="seqmix_gzip_flag", fixture="seqmix", out="gzflag", argv=["-g", "{geno}", "-f", "phylip"]),
    # coordinate windows: a step below and above the size (above: the sites between two windows are in none)
    dict(name="haplo_coord_step_below", fixture="haplo", out="file", argv=["-g", "{geno}"] + HAPLO_WIN + ["--windSize", "900", "--stepSize", "600"]),
    dict(name="haplo_coord_step_above", fixture="haplo", out="stdout",
         argv=["-g", "{geno}", "-f", "phylip"] + HAPLO_WIN + ["--windSize", "700", "--stepSize", "1100", "--minSites", "100000"]),
    dict(name="mixed_coord_split", fixture="mixed", out="file",
         argv=["-g", "{geno}", "--splitPhased", "--ploidy"] + MIXED_PLOIDY + HAPLO_WIN + ["--windSize", "300", "--stepSize", "675"]),
    dict(name="abba_coord_split_phylip", fixture="abba", out="file",
         argv=["-g", "{geno}", "--splitPhased", "-f", "phylip"] + HAPLO_WIN + ["--windSize", "200", "--stepSize", "1950"]),
    # sites windows: an overlap, a --maxDist that cuts windows short, --minSites below --windSize
    dict(name="haplo_sites_maxdist_minsites", fixture="haplo", out="file",
         argv=["-g", "{geno}"] + SITES + ["--windSize", "100", "--overlap", "20", "--maxDist", "100", "--minSites", "30"]),
    dict(name="seqmix_sites_comments", fixture="seqmix", out="file",
         argv=["-g", "{geno}", "--NtoGap"] + SITES + ["--windSize", "12", "--overlap", "4", "--maxDist", "400", "--minSites", "5"]),
    dict(name="bigpos_sites_sep", fixture="bigpos", out="sep",
         argv=["-g", "{geno}", "--splitPhased"] + SITES + ["--windSize", "600", "--overlap", "100", "--maxDist", "100000", "--minSites", "200"]),
    # contigs
    dict(name="seqmix_contigs_phylip", fixture="seqmix", out="file", argv=["-g", "{geno}", "-M", "contigs", "-f", "phylip"]),
    dict(name="sparse_contigs_sep_gzip", fixture="sparse", out="sep", argv=["-g", "{geno}", "-M", "contigs", "--gzip", "-f", "phylip", "--splitPhased"]),
    # windows into separate files
    dict(name="haplo_windows_sep", fixture="haplo", out="sep", argv=["-g", "{geno}"] + HAPLO_WIN + ["--windSize", "2000", "--stepSize", "2000"]),
    dict(name="seqmix_windows_sep_gzip", fixture="seqmix", out="sep",
         argv=["-g", "{geno}", "--gzip", "-f", "phylip"] + SITES + ["--windSize", "20", "--overlap", "5", "--maxDist", "1000", "--minSites", "8"]),
]


def out_args(case, tmp):
    """the output flags of a case writing under the directory tmp"""
    stem = os.path.join(tmp, "out")
    return {"stdout": [], "file": ["-s", stem], "gz": ["-s", stem + ".gz"], "gzflag": ["-s", stem, "--gzip"],
            "sep": ["-s", stem, "--separateFiles"]}[case["out"]]


def read_output(case, tmp, stdout):
    """what the run left, as the bytes the golden holds"""
    kind = case["out"]
    if kind == "stdout":
        return stdout
    if kind == "file":
        with open(os.path.join(tmp, "out"), "rb") as f:
            return f.read()
    if kind in ("gz", "gzflag"):
        with gzip.open(os.path.join(tmp, "out.gz"), "rb") as f:
            return f.read()
    parts = []
    for name in sorted(os.listdir(tmp)):
        with (gzip.open if name.endswith(".gz") else open)(os.path.join(tmp, name), "rb") as f:
            parts.append(b"== " + name.encode() + b"\n" + f.read())
    return b"".join(parts)
