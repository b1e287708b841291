"""The genoToPlink.py drop-in against the UNMODIFIED reference on random files x random command lines (host route, CPU only).

    python tools/diff_reference_plink.py N SEED [--ref DIR] [--log profiles/plink/diff_reference_plink_<SEED>.log]

Case k is tests/golden/plink_cases.random_case(SEED * 100003 + k): a seeded `.geno` file (haploid columns, N, '|', leading-zero
positions, scaffolds that come back, cells shorter and longer than their column's, a '#' line), one of the five formats, a random -s
in an order of its own, --makeFAM; one case in eight carries a line the reference dies on or a -s name the header lacks.  Every second
case runs the drop-in in blocks of 2 000 bytes.  The reference runs with its directory on PYTHONPATH.  Where it exits 0 the files must
be equal byte for byte (and stderr, the reference's progress lines, too); where it dies the drop-in must exit non-zero and leave no
file.  No case is left out.  Prints one line per differing case and a summary; exit status 1 when any case differs."""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from plink_cases import random_case  # noqa: E402


def _read(d):
    got = {}
    for name in sorted(os.listdir(d)):
        with open(os.path.join(d, name), "rb") as f:
            got[name] = f.read()
    return got


def one(k, seed, ref, tmp):
    text, argv, _ = random_case(seed * 100003 + k)
    d = os.path.join(tmp, "c%d" % k)
    os.makedirs(os.path.join(d, "ref"))
    os.makedirs(os.path.join(d, "own"))
    inp = os.path.join(d, "in.geno")
    with open(inp, "w") as f:
        f.write(text)
    r = subprocess.run([sys.executable, os.path.join(ref, "tools", "genoToPlink.py"), "-g", inp] + argv + ["--prefix", os.path.join(d, "ref", "o")],
                       cwd=ref, env=dict(os.environ, PYTHONPATH=ref), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    env = dict(os.environ, PG_PED_DEVICE="0")
    if k % 2:
        env["PG_STREAM_BYTES"] = "2000"
    o = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "genoToPlink.py"), "-g", inp] + argv + ["--prefix", os.path.join(d, "own", "o")],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=900)
    want, got = _read(os.path.join(d, "ref")), _read(os.path.join(d, "own"))
    if r.returncode == 0:
        ok = o.returncode == 0 and len(want) == (3 if "--makeFAM" in argv else 2) and want == got and r.stdout == o.stdout and r.stderr == o.stderr
    else:
        ok = o.returncode != 0 and got == {} and b"Traceback" not in o.stderr
    return k, ok, argv, r.returncode, o.returncode, want.get("o.map", b"").count(b"\n")


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
        lines = ["case %d %s reference=%d drop-in=%d sites=%d %s" % (k, "same" if ok else "DIFFERS", rr, ro, rows, " ".join(x.replace(tmp, "@T") for x in argv))
                 for k, ok, argv, rr, ro, rows in res]
    bad = [r for r in res if not r[1]]
    died = sum(1 for r in res if r[3] != 0)
    lines.append("seed %d: %d cases, %d differ, the reference died on %d, %d .map rows written by the reference"
                 % (a.seed, len(res), len(bad), died, sum(r[5] for r in res)))
    print("\n".join(ln for ln in lines if "DIFFERS" in ln or ln.startswith("seed")))
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
