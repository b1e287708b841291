"""The filterGenotypes.py drop-in against the UNMODIFIED reference on random files x random command lines (host route, CPU only).

    python tools/diff_reference_filter.py N SEED [--ref DIR] [--log profiles/filter/diff_reference_filter_<SEED>.log]

Case k is tests/golden/filter_cases.random_case(SEED * 100003 + k): a seeded `.geno` file and an option set that never reaches a line
the reference raises on.  Every reference run ends with its sleep(10), so the cases run in parallel.  -of randomAllele is compared
cell by cell as membership (the reference draws at random).  Prints one line per differing case and a summary; exit status 1 when any
case differs."""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from filter_cases import random_case  # noqa: E402


def same(ours, theirs, text, argv):
    if ours == theirs:
        return True
    if "randomAllele" not in argv:
        return False
    src = {}
    lines = text.split("\n")
    head = lines[0].split()
    for ln in lines[1:]:
        t = ln.split()
        if t:
            src[(t[0], t[1])] = dict(zip(head, t))
    a, b = ours.decode().split("\n"), theirs.decode().split("\n")
    if len(a) != len(b) or a[0] != b[0]:
        return False
    cols = a[0].split("\t")
    for x, y in zip(a[1:], b[1:]):
        xs, ys = x.split("\t"), y.split("\t")
        if xs[:2] != ys[:2]:
            return False
        row = src.get((xs[0], xs[1])) if xs[0] else None
        for c, v in zip(cols[2:], xs[2:]):
            if row is None or v not in row[c][::2]:
                return False
    return True


def one(k, seed, ref, tmp):
    text, argv = random_case(seed * 100003 + k)
    inp = os.path.join(tmp, "c%d.geno" % k)
    with open(inp, "w") as f:
        f.write(text)
    r = subprocess.run([sys.executable, os.path.join(ref, "filterGenotypes.py"), "-i", inp] + argv, cwd=ref, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, timeout=900)
    env = dict(os.environ, PG_FILTER_DEVICE="0")
    o = subprocess.run([sys.executable, os.path.join(ROOT, "filterGenotypes.py"), "-i", inp] + argv, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env, timeout=900)
    ok = r.returncode == 0 and o.returncode == 0 and same(o.stdout, r.stdout, text, argv)
    return k, ok, argv, len(r.stdout.split(b"\n")) - 2


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("seed", type=int)
    ap.add_argument("--ref", default=os.environ.get("GG_REFERENCE", "/root/reference"))
    ap.add_argument("--jobs", type=int, default=32)
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    lines = []
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.jobs) as ex:
        res = list(ex.map(lambda k: one(k, a.seed, a.ref, tmp), range(a.n)))
    bad = [r for r in res if not r[1]]
    for k, ok, argv, rows in res:
        lines.append("case %d %s rows=%d %s" % (k, "same" if ok else "DIFFERS", rows, " ".join(argv)))
    lines.append("seed %d: %d cases, %d differ, %d rows written by the reference" % (a.seed, a.n, len(bad), sum(r[3] for r in res)))
    print("\n".join(l for l in lines if "DIFFERS" in l or l.startswith("seed")))
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
