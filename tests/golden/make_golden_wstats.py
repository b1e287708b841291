"""Fixtures and golden outputs of the UNMODIFIED reference windowStats.py.

    python tests/golden/make_golden_wstats.py     (needs the reference tree; writes tests/golden/wstats/*.tsv, coords.txt, <case>.out.gz)

Every case of wstats_cases.py is a command line of the reference, run with `np.NaN = np.nan` set first (the name NumPy 2 dropped; the
reference writes it for failed and empty windows) and the reference directory on the module path.  tests/test_wstats_cpu.py and
tests/test_gpu_wstats.py run the drop-in on the same command line and compare the output byte for byte.
"""
import gzip
import os
import random
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.environ.get("GG_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "wstats")
WRAP = ("import sys, runpy, numpy as np; np.NaN = np.nan; sys.path.insert(0, %r); "
        "sys.argv = sys.argv[1:]; runpy.run_path(sys.argv[0], run_name='__main__')" % REF_DIR)

sys.path.insert(0, HERE)
from wstats_cases import CASES, NUMPY_VERSION, fixture_path  # noqa: E402


def _cell(R):
    kind = R.random()
    if kind < 0.05:
        return R.choice(["nan", "NaN", "NAN"])
    if kind < 0.35:
        return str(R.randint(-50, 400))
    if kind < 0.75:
        return "%.*f" % (R.randint(1, 6), R.uniform(-3, 90))
    if kind < 0.85:
        return "%.3e" % R.uniform(-1e-4, 1e5)
    if kind < 0.9:
        return R.choice(["+", "-", ""]) + "%d.%03dE%+d" % (R.randint(0, 9), R.randint(0, 999), R.randint(-9, 9))
    return "0." + "0" * R.randint(0, 5) + str(R.randint(1, 999))


def main_table():
    R = random.Random(20240611)
    rows = ["scaffold\tposition\ta\tb\tc"]
    for scaf, n, span in (("c1", 70, 1000), ("c2", 45, 420)):
        pos = sorted(R.sample([p for p in range(1, span) if not 500 <= p < 760], n))       # (c1: no site in 500 .. 759)
        for p in pos:
            rows.append("\t".join([scaf, str(p)] + [_cell(R) for _ in range(3)]))
    return "\n".join(rows) + "\n"


QUIRKS = """scaffold position  u\tv
c1 3 1e3 07
c1   9\t\tinf   1_0
c1 12 -inf 1.
# a comment line 1 2 3
c1 17 .5 1e400
c1 21 2.5 infinity
c1 30 -nan 1234567890123456
c1 31 +nan 12345678901234567
c1 44 1e23 1e-23
c1 58 1e22 1e-22
c1 59 123456789012345e8 1e-400
c1 77 0.1 0.30000000000000004
c1 93 9007199254740993 -0.5
c1 101 1E+2 +7
c1 140 nan 3
c2 5 1.5 2.5
c2 6 Infinity -Infinity
c2 55 4 4.0000000000000001
c2 56 00012.50 1e0
c1 10 8 9
c1 20 10 11
c1 60 12 13.25
"""

BAD = """scaffold position a b
c1 10 1.5 2
c1 20 2.5 3
c1 30 3.5 nan
c1 45 1 1
c1 120 x 7
c1 130 3 oops
c1 210 4 4
c1 220 5 5
c1 230 6 6.5
c1 240 7 7
"""

ALLNAN = """scaffold position a b
c1 10 1.5 nan
c1 20 2.5 nan
c1 30 3.5 nan
c1 110 1 2
c1 120 nan 7
c1 130 3 nan
"""

DUP = """scaffold position a b a
c1 10 1 2 3
c1 20 4 5 6
c1 30 7 8 9.5
c1 150 1.25 2 nan
"""

COORDS = """c1 1 100
c1 101 250 named
c1 400 480
c1 500 700
c1 650 900
c9 1 100
c2 10 200
c2 150 420
"""


def write_fixtures():
    os.makedirs(OUT, exist_ok=True)
    main = main_table()
    files = {"main.tsv": main, "headerless.tsv": main.split("\n", 1)[1], "quirks.tsv": QUIRKS, "bad.tsv": BAD, "allnan.tsv": ALLNAN,
             "header_only.tsv": "scaffold\tposition\ta\tb\n", "dup.tsv": DUP, "coords.txt": COORDS}
    for name, text in files.items():
        with open(os.path.join(OUT, name), "w") as f:
            f.write(text)


def run(case):
    name, fixture, argv, through_stdin = case
    cmd = [sys.executable, "-c", WRAP, os.path.join(REF_DIR, "windowStats.py")] + [a.replace("@G", HERE) for a in argv]
    stdin = None
    if through_stdin:
        stdin = open(fixture_path(fixture), "rb")
    else:
        cmd += ["-i", fixture_path(fixture)]
    r = subprocess.run(cmd, cwd=REF_DIR, stdin=stdin, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if stdin:
        stdin.close()
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (name, r.stderr.decode()[-2000:]))
    with open(os.path.join(OUT, name + ".out.gz"), "wb") as f:
        f.write(gzip.compress(r.stdout, mtime=0))
    return name, len(r.stdout), r.stdout.count(b"\n")


if __name__ == "__main__":
    import numpy
    assert numpy.__version__ == NUMPY_VERSION, "wstats_cases.NUMPY_VERSION says %s" % NUMPY_VERSION
    write_fixtures()
    for case in CASES:
        print(*run(case))
