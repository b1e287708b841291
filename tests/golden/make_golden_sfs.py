#!/usr/bin/env python
"""Regenerate tests/golden/sfs/ by running the UNMODIFIED reference's sfs.py (/root/reference) on the fixtures of cases.py and on
freq.py goldens.  Only runs where the reference is (it does not travel to the GPU box); the outputs it writes are committed.

    python tests/golden/make_golden_sfs.py [case-name ...]
"""
import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
from sfs_cases import SFS_AUX_FILES, SFS_CASES  # noqa: E402

REF = "/root/reference"
WRAP = ("import sys, runpy, numpy as np; np.NaN = np.nan; sys.path.insert(0, %r); "
        "sys.argv = sys.argv[1:]; runpy.run_path(sys.argv[0], run_name='__main__')" % REF)


def run_case(case):
    out = os.path.join(HERE, "sfs", case["name"])
    shutil.rmtree(out, ignore_errors=True)
    os.makedirs(out)
    geno = os.path.join(HERE, case["fixture"] + ".geno.gz") if case.get("fixture") else ""
    argv = [a.format(geno=geno, dir=HERE, out=out) for a in case["argv"]]
    cmd = [sys.executable, "-c", WRAP, os.path.join(REF, "sfs.py")] + argv
    r = subprocess.run(cmd, cwd=out, env=dict(os.environ, PYTHONHASHSEED="0"), timeout=1200, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if case.get("fails"):
        assert r.returncode != 0 and not os.listdir(out), "the reference was expected to fail on " + case["name"]
        with open(os.path.join(out, "fails"), "w") as f:
            f.write(r.stderr.decode().strip().splitlines()[-1] + "\n")
        return ["fails"]
    if r.returncode != 0:
        sys.stderr.write(r.stderr.decode()[-2000:])
        raise SystemExit("reference failed on " + case["name"])
    if case.get("pipe"):
        with open(os.path.join(out, "stdout"), "wb") as f:
            f.write(r.stdout)
    return sorted(os.listdir(out))


def main():
    want = set(sys.argv[1:])
    for fn, txt in SFS_AUX_FILES.items():
        with open(os.path.join(HERE, fn), "w") as f:
            f.write(txt)
    for case in SFS_CASES:
        if want and case["name"] not in want:
            continue
        print("golden", case["name"], run_case(case), flush=True)


if __name__ == "__main__":
    main()
