"""The genoToEigenstrat.py drop-in against the UNMODIFIED reference on random files x random command lines (host route, CPU only).

    python tools/diff_reference_eig.py N SEED [--ref DIR] [--log profiles/eig/diff_reference_eig_<SEED>.log]

Case k is tests/golden/eig_cases.random_case(SEED * 100003 + k): a seeded `.geno` file (phased or diplo cells, haploid columns, N, '|',
leading-zero positions), a random -s selection with repeats and unknown names, --nullChrom, a --chromFile over some of its scaffolds
(blanks and tabs, a scaffold listed twice) and --cumulativePos with labels the reference survives.  Every second case runs the drop-in
in blocks of 2 000 bytes.  The reference runs with its directory on PYTHONPATH.  The three files are compared byte for byte.  Prints
one line per differing case and a summary; exit status 1 when any case differs."""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from eig_cases import OUTPUTS, random_case  # noqa: E402


def _outs(d, tag):
    return {k: os.path.join(d, "%s.%s" % (tag, k)) for k in OUTPUTS}


def _read(outs):
    got = {}
    for k, p in outs.items():
        if os.path.exists(p):
            with open(p, "rb") as f:
                got[k] = f.read()
    return got


def one(k, seed, ref, tmp):
    text, argv, chrom = random_case(seed * 100003 + k)
    d = os.path.join(tmp, "c%d" % k)
    os.makedirs(d)
    inp = os.path.join(d, "in.geno")
    with open(inp, "w") as f:
        f.write(text)
    if chrom is not None:
        with open(os.path.join(d, "chrom.txt"), "w") as f:
            f.write(chrom)
        argv = argv + ["--chromFile", os.path.join(d, "chrom.txt")]
    ro, oo = _outs(d, "ref"), _outs(d, "own")
    out_args = lambda o: ["--genoOutFile", o["geno"], "--snpOutFile", o["snp"], "--indOutFile", o["ind"]]      # noqa: E731
    r = subprocess.run([sys.executable, os.path.join(ref, "tools", "genoToEigenstrat.py"), "-g", inp] + argv + out_args(ro), cwd=ref,
                       env=dict(os.environ, PYTHONPATH=ref), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    env = dict(os.environ, PG_EIG_DEVICE="0")
    if k % 2:
        env["PG_STREAM_BYTES"] = "2000"
    o = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "genoToEigenstrat.py"), "-g", inp] + argv + out_args(oo), cwd=ROOT,
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    want, got = _read(ro), _read(oo)
    ok = r.returncode == 0 and o.returncode == 0 and len(want) == 3 and want == got and r.stdout == o.stdout
    return k, ok, argv, want.get("snp", b"").count(b"\n")


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
        lines = ["case %d %s rows=%d %s" % (k, "same" if ok else "DIFFERS", rows, " ".join(x.replace(tmp, "@T") for x in argv))
                 for k, ok, argv, rows in res]
    bad = [r for r in res if not r[1]]
    lines.append("seed %d: %d cases, %d differ, %d .snp rows written by the reference" % (a.seed, len(res), len(bad), sum(r[3] for r in res)))
    print("\n".join(ln for ln in lines if "DIFFERS" in ln or ln.startswith("seed")))
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
