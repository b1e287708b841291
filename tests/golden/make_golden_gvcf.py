"""Golden outputs of the UNMODIFIED reference VCF_processing/genoToVCF.py on the existing fixtures, gvcf/extra.geno and gvcf/dup.geno.

    python tests/golden/make_golden_gvcf.py        (needs the reference tree; writes tests/golden/gvcf/<case>.out.gz)

It first writes the fasta the -r cases read (gvcf/ref.fa with its .fai, the copy gvcf/ref_nofai.fa without one, gvcf/ref.fa.gz): data
made here from a seed, not taken from anywhere.  Every case is a command line of the reference, run with the reference directory on
PYTHONPATH (the script imports genomics from there); tests/test_gvcf_cpu.py and tests/test_gpu_gvcf.py run the drop-in on the same
command line and compare the text byte for byte.
"""
import gzip
import os
import random
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.environ.get("GG_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "gvcf")

sys.path.insert(0, HERE)
from gvcf_cases import CASES, fixture_path  # noqa: E402

X1 = "ACgTaGGNnTCATcGN"          # x1: N under the A/N site at 8, n at 9, N under the all-missing site at 16


def write_fasta():
    R = random.Random(20261019)
    mixed = lambda n: "".join(R.choice("ACGT" * 10 + "acgt" * 2 + "Nn") for _ in range(n))      # noqa: E731
    seqs = [("chr1", mixed(8000)), ("x1", "T" * 16), ("chr2", mixed(5000)), ("chr3", "".join(R.choice("acgtn") for _ in range(2500))),
            ("s1", mixed(8)), ("s2", mixed(20)), ("x1", X1), ("x2", mixed(30))]
    recs = ["text in front of the first record\n"]
    for k, (name, seq) in enumerate(seqs):
        if name == "x1" and seq == X1:
            body = " ".join(seq[j:j + 4] for j in range(0, len(seq), 4)) + "\n"          # blanks inside the sequence
        else:
            body = "".join(seq[j:j + 60] + "\n" for j in range(0, len(seq), 60))
        recs.append(">%s%s\n%s" % (name, " record %d" % k if k % 2 else "", body))
    text = "".join(recs)
    for name in ("ref.fa", "ref_nofai.fa"):
        with open(os.path.join(OUT, name), "w") as f:
            f.write(text)
    with open(os.path.join(OUT, "ref.fa.gz"), "wb") as f:
        f.write(gzip.compress(text.encode(), mtime=0))
    final = dict(seqs)
    with open(os.path.join(OUT, "ref.fa.fai"), "w") as f:
        for name in dict.fromkeys(n for n, _ in seqs):
            f.write("%s\t%d\t0\t60\t61\n" % (name, len(final[name])))


def run(case):
    name, fixture, argv = case
    cmd = [sys.executable, os.path.join(REF_DIR, "VCF_processing", "genoToVCF.py"), "-g", fixture_path(fixture)] + [a.replace("@G", HERE) for a in argv]
    env = dict(os.environ, PYTHONPATH=REF_DIR)
    r = subprocess.run(cmd, cwd=REF_DIR, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (name, r.stderr.decode()[-2000:]))
    with open(os.path.join(OUT, name + ".out.gz"), "wb") as f:
        f.write(gzip.compress(r.stdout, mtime=0))
    return name, len(r.stdout)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    write_fasta()
    with ThreadPoolExecutor(max_workers=16) as ex:
        for name, n in ex.map(run, CASES):
            print(name, n)
