"""The genoToVCF.py drop-in against the UNMODIFIED reference on random files x random command lines (host route, CPU only).

    python tools/diff_reference_gvcf.py N SEED [--ref DIR] [--log profiles/gvcf/diff_reference_gvcf_<SEED>.log]

Case k is tests/golden/gvcf_cases.random_case(SEED * 100003 + k): a seeded `.geno` file (phased, pairs or diplo cells, haploid columns,
N, '|', leading-zero positions), a random -s selection with repeats, and for most cases a fasta over its scaffolds with lower-case and
n bases (-r, with a .fai for every second one).  The reference runs with its directory on PYTHONPATH.  Prints one line per differing case
and a summary; exit status 1 when any case differs."""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from gvcf_cases import random_case  # noqa: E402


def one(k, seed, ref, tmp):
    text, argv, fasta = random_case(seed * 100003 + k)
    d = os.path.join(tmp, "c%d" % k)
    os.makedirs(d)
    inp = os.path.join(d, "in.geno")
    with open(inp, "w") as f:
        f.write(text)
    if fasta is not None:
        fa = os.path.join(d, "ref.fa")
        with open(fa, "w") as f:
            f.write(fasta)
        if k % 2:
            with open(fa + ".fai", "w") as f:
                for rec in fasta.split(">")[1:]:
                    f.write("%s\t%d\n" % (rec.split()[0], len("".join(rec.split("\n")[1:]))))
        argv = argv + ["-r", fa]
    r = subprocess.run([sys.executable, os.path.join(ref, "VCF_processing", "genoToVCF.py"), "-g", inp] + argv, cwd=ref,
                       env=dict(os.environ, PYTHONPATH=ref), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    o = subprocess.run([sys.executable, os.path.join(ROOT, "VCF_processing", "genoToVCF.py"), "-g", inp] + argv, cwd=ROOT,
                       env=dict(os.environ, PG_GVCF_DEVICE="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    ok = r.returncode == 0 and o.returncode == 0 and r.stdout == o.stdout
    return k, ok, argv, r.stdout.count(b"\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("seed", type=int)
    ap.add_argument("--ref", default=os.environ.get("GG_REFERENCE", "/root/reference"))
    ap.add_argument("--jobs", type=int, default=16)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.jobs) as ex:
        res = list(ex.map(lambda k: one(k, a.seed, a.ref, tmp), range(a.n)))
        lines = ["case %d %s lines=%d %s" % (k, "same" if ok else "DIFFERS", rows, " ".join(x.replace(tmp, "@T") for x in argv))
                 for k, ok, argv, rows in res]
    bad = [r for r in res if not r[1]]
    lines.append("seed %d: %d cases, %d differ, %d lines written by the reference" % (a.seed, len(res), len(bad), sum(r[3] for r in res)))
    print("\n".join(ln for ln in lines if "DIFFERS" in ln or ln.startswith("seed")))
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
