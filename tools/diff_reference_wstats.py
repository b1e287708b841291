#!/usr/bin/env python
"""Seeded random tables x command lines through the UNMODIFIED reference windowStats.py (under the `np.NaN = np.nan` shim) and through the
drop-in's host route (PG_WS_DEVICE=0), stdout compared byte for byte.

    python tools/diff_reference_wstats.py [--cases 240] [--seed 1] [--log profiles/wstats/diff_reference_wstats_SEED.log]

Needs the reference tree (GG_REFERENCE, default /root/reference) and no GPU.  Where the reference exits 0 the bytes must be equal.  Where
it dies with a traceback (a cell NumPy does not convert, min / max of a column without a value: the documented divergences) the drop-in
must stop with exit status 1 and have written exactly the reference's whole rows.  Anything else is a difference; the exit status is
their number."""
import argparse
import os
import random
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = os.environ.get("GG_REFERENCE", "/root/reference")
WRAP = ("import sys, runpy, numpy as np; np.NaN = np.nan; sys.path.insert(0, %r); "
        "sys.argv = sys.argv[1:]; runpy.run_path(sys.argv[0], run_name='__main__')" % REF)
STATS = ["mean", "median", "min", "max", "sd", "sum", "q5", "q10", "q25", "q75", "q90", "q95"]


def cell(R, nan_rate, odd_rate, junk_rate):
    x = R.random()
    if x < nan_rate:
        return R.choice(["nan", "NaN", "NAN"])
    if x < nan_rate + odd_rate:
        return R.choice(["inf", "-inf", "1_0", "12345678901234567", "1e400", "1e-400", "Infinity", "-nan", "1e23", ".5", "5.", "0.1e-22"])
    if x < nan_rate + odd_rate + junk_rate:
        return R.choice(["x", "NA", "1,5", "--"])
    kind = R.random()
    if kind < 0.3:
        return str(R.randint(-20, 200))
    if kind < 0.8:
        text = "%.*f" % (R.randint(0, 8), R.uniform(-50, 50))
        return text.lstrip("-") if float(text) == 0.0 else text     # (no -0.0: the sign of a zero min / median is NumPy's to choose)
    if kind < 0.9:
        return "%.*e" % (R.randint(0, 6), R.uniform(-1, 1) * 10.0 ** R.randint(-12, 12))
    return R.choice(["0", "1", "0.5", "2.5", "1e3", "07"])


def make_case(seed):
    R = random.Random(seed)
    n_cols = R.randint(1, 4)
    names = ["v%d" % k for k in range(n_cols)]
    nan_rate = R.choice([0.0, 0.02, 0.1, 0.5])
    odd_rate = R.choice([0.0, 0.0, 0.03])
    junk_rate = R.choice([0.0, 0.0, 0.0, 0.01])
    sep = R.choice(["\t", " ", "  \t"])
    rows = [sep.join(["scaffold", "position"] + names)]
    scafs = ["c%d" % k for k in range(R.randint(1, 3))]
    if len(scafs) > 1 and R.random() < 0.25:
        scafs.append(scafs[0])                              # a scaffold that comes back
    span = R.choice([200, 1000, 5000])
    for scaf in scafs:
        n = R.randint(1, R.choice([8, 40, 150]))
        for p in sorted(R.sample(range(1, span), min(n, span - 1))):
            rows.append(sep.join([scaf, str(p)] + [cell(R, nan_rate, odd_rate, junk_rate) for _ in range(n_cols)]))
            if R.random() < 0.01:
                rows.append("# a comment")
    argv = []
    wt = R.choice(["coordinate", "coordinate", "sites", "predefined"])
    coords = None
    if wt == "coordinate":
        w = R.choice([1, 10, 50, 100, 500])
        argv += ["-w", str(w)] + (["-s", str(R.choice([1, 5, 25, w, 2 * w]))] if R.random() < 0.5 else [])
        if R.random() < 0.5:
            argv = ["--windType", "coordinate"] + argv
    elif wt == "sites":
        w = R.choice([1, 3, 10, 40])
        argv += ["--windType", "sites", "-w", str(w)]
        if w > 1 and R.random() < 0.5:
            argv += ["-O", str(R.randint(1, w - 1))]
        elif R.random() < 0.4:
            argv += ["-D", str(R.choice([20, 100, 1000]))]
    else:
        lines = []
        for scaf in list(dict.fromkeys(scafs)) + (["zz"] if R.random() < 0.3 else []):
            at = 1
            for _ in range(R.randint(1, 5)):
                a = at + R.randint(0, span // 4)
                b = a + R.randint(0, span // 2)
                lines.append("%s %d %d" % (scaf, a, b))
                at = b + 1 if R.random() < 0.7 else a
        coords = "\n".join(lines) + "\n"
        argv += ["--windType", "predefined"]
    if R.random() < 0.5:
        m = R.choice([0, 1, 2, 5, 20])
        if not (wt == "predefined" and m == 0):
            argv += ["-m", str(m)]
    if R.random() < 0.7:
        pool = STATS if junk_rate or nan_rate >= 0.1 and R.random() < 0.3 else [s for s in STATS if nan_rate < 0.1 or s not in ("min", "max")]
        argv += ["--stats"] + [R.choice(pool) for _ in range(R.randint(1, 12))]
    if R.random() < 0.3:
        argv += ["--columns"] + [R.choice(names) for _ in range(R.randint(1, n_cols))]
    if R.random() < 0.1:
        argv += ["--writeFailedWindows"]
    return "\n".join(rows) + "\n", argv, coords


def run_case(seed):
    text, argv, coords = make_case(seed)
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, "t.tsv")
        with open(inp, "w") as f:
            f.write(text)
        if coords is not None:
            with open(os.path.join(tmp, "coords.txt"), "w") as f:
                f.write(coords)
            argv = argv + ["--windCoords", os.path.join(tmp, "coords.txt")]
        try:
            ref = subprocess.run([sys.executable, "-c", WRAP, os.path.join(REF, "windowStats.py"), "-i", inp] + argv, cwd=REF,
                                 stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
        except subprocess.TimeoutExpired:
            return seed, "skipped", "the reference does not end", argv
        env = dict(os.environ, PG_WS_DEVICE="0", PG_STREAM_BYTES=str(random.Random(seed).choice([200, 4000, 1 << 28])))
        got = subprocess.run([sys.executable, os.path.join(ROOT, "windowStats.py"), "-i", inp] + argv, cwd=ROOT, env=env,
                             stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=120)
    if ref.returncode == 0:
        if got.returncode == 0 and got.stdout == ref.stdout:
            return seed, "equal", "", argv
        return seed, "DIFFERENT", "exit %d, %d bytes against the reference's %d: %s" % (
            got.returncode, len(got.stdout), len(ref.stdout), got.stderr.decode()[-300:].strip()), argv
    # the reference died: its whole rows are what it wrote up to the last line feed
    whole = ref.stdout[:ref.stdout.rfind(b"\n") + 1]
    why = ref.stderr.decode().strip().splitlines()[-1][:120]
    if got.returncode == 1 and got.stdout in (whole, ref.stdout if b"\n" not in ref.stdout else whole):
        return seed, "both stop", why, argv
    return seed, "DIFFERENT", "the reference died (%s) behind %d bytes of whole rows; exit %d, %d bytes: %s" % (
        why, len(whole), got.returncode, len(got.stdout), got.stderr.decode()[-300:].strip()), argv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cases", type=int, default=240)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--log", default=None)
    args = ap.parse_args()
    if not os.path.exists(os.path.join(REF, "windowStats.py")):
        sys.exit("the reference tree is not at %s (GG_REFERENCE)" % REF)
    log = args.log or os.path.join(ROOT, "profiles", "wstats", "diff_reference_wstats_%d.log" % args.seed)
    os.makedirs(os.path.dirname(log), exist_ok=True)
    seeds = [args.seed * 100003 + k for k in range(args.cases)]
    with ThreadPoolExecutor(max_workers=min(16, len(os.sched_getaffinity(0)))) as ex:
        results = list(ex.map(run_case, seeds))
    import numpy
    tally = {}
    with open(log, "w") as f:
        f.write("windowStats.py: %d seeded cases from seed %d, reference under the np.NaN shim, NumPy %s, host route (PG_WS_DEVICE=0)\n"
                % (args.cases, args.seed, numpy.__version__))
        for seed, verdict, note, argv in results:
            tally[verdict] = tally.get(verdict, 0) + 1
            f.write("%d\t%s\t%s\t%s\n" % (seed, verdict, " ".join(argv), note))
        summary = ", ".join("%d %s" % (n, v) for v, n in sorted(tally.items()))
        f.write("total: %s\n" % summary)
    print(summary)
    return tally.get("DIFFERENT", 0)


if __name__ == "__main__":
    sys.exit(main())
