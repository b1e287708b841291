"""The filterGenotypes.py drop-in against the UNMODIFIED reference on random files x random command lines (host route, CPU only).

    python tools/diff_reference_filter.py N SEED [--generator random|edge] [--ref DIR]
                                          [--log profiles/filter/diff_reference_filter_<SEED>.log]

Case k is tests/golden/filter_cases.random_case(SEED * 100003 + k) (--generator random, the default) or edge_case(SEED * 100003 + k)
(--generator edge): a seeded `.geno` file and an option set.  Every reference run ends with its sleep(10), so the cases run in
parallel.  -of randomAllele is compared cell by cell as membership (the reference draws at random).

--generator edge also holds the reference against oracle/filter_oracle.py: a case is the same when the drop-in (host route), the
oracle and the reference agree.  Where the oracle names a line the reference raises on, the reference must still be running after
--hang seconds (its worker died; it waits forever) and the drop-in must stop naming that line.  Two hand-built --HWE cases with
populations of N/N genotypes follow the seeded ones.  Prints one line per differing case and a summary; exit status 1 when any case
differs."""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
sys.path.insert(0, ROOT)
from filter_cases import edge_case, edge_files, random_case  # noqa: E402

from oracle.filter_oracle import filter_reference  # noqa: E402

# --HWE with populations whose genotypes are N/N where the site varies: inHWE drops the "N" diplotypes and passes; the last line has a
# called genotype in P0 and stops the reference's worker (one line per pod, so the pods before it are written)
HWE_NN = ("#CHROM\tPOS\ta\tb\tc\td\n"
          "c\t1\tN/N\tN|N\tA/T\tT/T\n"
          "c\t2\tN/N\tN/N\tA/A\tA/A\n"
          "c\t3\tN/N\tN/N\tC/T\tC/C\n")
HAND = [(HWE_NN, ["--HWE", "0.05", "both", "-p", "P0", "a", "-p", "P1", "b", "--keepAllSamples", "--podSize", "1"], {}),
        (HWE_NN + "c\t4\tA/A\tN/N\tA/T\tT/T\n", ["--HWE", "0.05", "both", "-p", "P0", "a,b", "-s", "d,c,b,a", "--podSize", "1"], {})]


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


def one(k, seed, ref, tmp, generator="random", hang=40):
    if generator == "random":
        text, argv = random_case(seed * 100003 + k)
        files = {}
    else:
        text, argv, files = HAND[k - N_SEEDED[0]] if k >= N_SEEDED[0] else edge_case(seed * 100003 + k)
    d = os.path.join(tmp, "c%d" % k)
    os.makedirs(d)
    argv = edge_files(argv, files, d)
    inp = os.path.join(d, "in.geno")
    with open(inp, "w") as f:
        f.write(text)
    want = filter_reference(argv, text) if generator == "edge" else None
    raises = want is not None and want.error is not None
    try:
        r = subprocess.run([sys.executable, os.path.join(ref, "filterGenotypes.py"), "-i", inp] + argv, cwd=ref, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE, timeout=hang if raises else 900)
        hung = False
    except subprocess.TimeoutExpired:
        r, hung = None, True
    env = dict(os.environ, PG_FILTER_DEVICE="0")
    o = subprocess.run([sys.executable, os.path.join(ROOT, "filterGenotypes.py"), "-i", inp] + argv, cwd=ROOT, stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=env, timeout=900)
    if raises:
        ok = hung and o.returncode != 0 and ("line %d:" % want.error[0]).encode() in o.stderr
        return k, ok, argv, -1
    ok = not hung and r.returncode == 0 and o.returncode == 0
    if want is None:
        ok = ok and same(o.stdout, r.stdout, text, argv)
    else:                                   # (-of randomAllele: each cell among the genotype's alleles as the oracle lists them)
        ok = ok and want.setup_error is None and want.matches(r.stdout) and want.matches(o.stdout)
    return k, ok, argv, len(r.stdout.split(b"\n")) - 2 if r else -1


N_SEEDED = [0]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("seed", type=int)
    ap.add_argument("--ref", default=os.environ.get("GG_REFERENCE", "/root/reference"))
    ap.add_argument("--jobs", type=int, default=32)
    ap.add_argument("--generator", choices=("random", "edge"), default="random")
    ap.add_argument("--hang", type=int, default=40, help="seconds after which a reference run the oracle says raises counts as hung")
    ap.add_argument("--log", default=None)
    a = ap.parse_args()
    lines = []
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(a.jobs) as ex:
        N_SEEDED[0] = a.n
        total = a.n + (len(HAND) if a.generator == "edge" else 0)
        res = list(ex.map(lambda k: one(k, a.seed, a.ref, tmp, a.generator, a.hang), range(total)))
    bad = [r for r in res if not r[1]]
    for k, ok, argv, rows in res:
        lines.append("case %d %s %s %s" % (k, "same" if ok else "DIFFERS", "rows=%d" % rows if rows >= 0 else "raises-and-hangs",
                                           " ".join(x.replace(tmp, "@T") for x in argv)))
    lines.append("seed %d (%s): %d cases, %d differ, %d rows written by the reference" % (a.seed, a.generator, len(res), len(bad),
                                                                                        sum(max(r[3], 0) for r in res)))
    print("\n".join(l for l in lines if "DIFFERS" in l or l.startswith("seed")))
    if a.log:
        os.makedirs(os.path.dirname(a.log), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
