#!/usr/bin/env python
"""Regenerate tests/golden/paint/ by running the UNMODIFIED reference's distPaint.py on the `haplo` fixture of cases.py and on the
haploid fixtures of paint_cases.py (written here).  Only runs where the reference is (make_golden.py names the place and holds the
np.NaN shim); the fixtures and outputs it writes are committed.

    python tests/golden/make_golden_paint.py [case-name ...]
"""
import gzip
import io
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden import REF, WRAP  # noqa: E402
from paint_cases import PAINT_AUX_FILES, PAINT_CASES, PAINT_FIXTURES  # noqa: E402


def make_fixture(name):
    """haploid columns: every source population has its own allele frequency per site, a reference individual draws from its
    population's, a mosaic individual from the source of the block its position lies in"""
    p = PAINT_FIXTURES[name]
    rng = np.random.default_rng(p["seed"])
    names, src = [], []
    for prefix, n, s in p["groups"]:
        for k in range(n):
            names.append("%s%d" % (prefix, k))
            src.append(-1 if s is None else s)
    src = np.array(src)
    lines = []
    for sc, length in enumerate(p["scaf_len"]):
        pos = np.arange(2, length, p["step"]) + rng.integers(0, p["step"] - 1, size=len(np.arange(2, length, p["step"])))
        for x in pos:
            ref, alt = rng.choice(4, size=2, replace=False)
            freq = rng.choice([0.02, 0.2, 0.5, 0.8, 0.98], size=p["n_src"])
            blk = int(x) // p["block"]
            source = np.where(src >= 0, src, (blk + np.arange(len(src))) % p["n_src"])
            allele = np.where(rng.random(len(src)) < freq[source], alt, ref)
            cells = np.where(rng.random(len(src)) < p["miss"], "N", np.array(list("ACGT"))[allele])
            lines.append((sc, int(x), cells))
    order = list(range(len(names)))
    if p["names"] is not None:
        order = [names.index(nm) for nm in p["names"]]
    path = os.path.join(HERE, name + ".geno.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as raw:
        txt = io.TextIOWrapper(raw, newline="\n")
        txt.write("#CHROM\tPOS\t" + "\t".join(names[k] for k in order) + "\n")
        for sc, x, cells in lines:
            txt.write("chr%d\t%d\t" % (sc + 1, x) + "\t".join(cells[k] for k in order) + "\n")
        txt.flush()
    return path


def run_case(case):
    geno = os.path.join(HERE, case["fixture"] + ".geno.gz")
    out = os.path.join(HERE, "paint", case["name"] + ".out")
    target = out + ".gz" if case.get("gz") else out
    argv = [a.format(geno=geno, dir=HERE) for a in case["argv"]]
    cmd = [sys.executable, "-W", "ignore", "-c", WRAP, os.path.join(REF, "distPaint.py")] + argv + ["-o", target]
    r = subprocess.run(cmd, cwd=HERE, env=dict(os.environ, PYTHONHASHSEED="0"), timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if r.returncode != 0:
        sys.stderr.write(r.stderr.decode()[-2000:])
        raise SystemExit("reference failed on " + case["name"])
    if case.get("gz"):
        with gzip.open(target, "rb") as f, open(out, "wb") as g:
            g.write(f.read())
        os.remove(target)
    return out


def main():
    want = set(sys.argv[1:])
    os.makedirs(os.path.join(HERE, "paint"), exist_ok=True)
    for fn, txt in PAINT_AUX_FILES.items():
        with open(os.path.join(HERE, fn), "w") as f:
            f.write(txt)
    for name in PAINT_FIXTURES:
        if not want or any(c["fixture"] == name and c["name"] in want for c in PAINT_CASES):
            print("fixture", name, make_fixture(name))
    for case in PAINT_CASES:
        if want and case["name"] not in want:
            continue
        out = run_case(case)
        with open(out) as f:
            rows = f.read().splitlines()
        cells = [c for r in rows[1:] for c in r.split("\t")[-len(rows[0].split("\t")) + 5 + (rows[0].startswith("windowID")):]]
        print("golden", case["name"], len(rows), "lines; cells:", {c: cells.count(c) for c in sorted(set(cells))}, flush=True)


if __name__ == "__main__":
    main()
