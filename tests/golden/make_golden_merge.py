#!/usr/bin/env python
"""Regenerate tests/golden/merge/ by running the UNMODIFIED reference's mergeGeno.py on the fixtures of merge_cases.py (written here).
Only runs where the reference is (make_golden.py names the place); the fixtures and the outputs are committed.  The script is run as a
program of its own, not through make_golden.py's shim: it needs no NumPy name restored, and it never closes its output file -- under
runpy the file's last buffer is not written when the interpreter ends.  A case on which the reference fails stops the script.

    python tests/golden/make_golden_merge.py [case-name ...]
"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden import REF  # noqa: E402
from merge_cases import MERGE_CASES, out_args, read_output, write_fixtures  # noqa: E402

DIR = os.path.join(HERE, "merge")


def run_case(case):
    with tempfile.TemporaryDirectory() as tmp:
        argv = [a.format(dir=DIR) for a in case["argv"]] + out_args(case, tmp)
        cmd = [sys.executable, "-W", "ignore", os.path.join(REF, "mergeGeno.py")] + argv
        r = subprocess.run(cmd, cwd=tmp, env=dict(os.environ, PYTHONHASHSEED="0"), timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            sys.stderr.write(r.stderr.decode()[-2000:])
            raise SystemExit("reference failed on " + case["name"])
        data = read_output(case, tmp, r.stdout)
    if not data:
        raise SystemExit("reference wrote nothing on " + case["name"])
    out = os.path.join(DIR, case["name"] + ".out.gz")
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
        f.write(data)
    return out, data


def main():
    want = set(sys.argv[1:])
    write_fixtures(DIR)
    print("fixtures in", DIR)
    for case in MERGE_CASES:
        if want and case["name"] not in want:
            continue
        out, data = run_case(case)
        print("golden", case["name"], len(data), "bytes,", data.count(b"\n") - 1, "data lines", flush=True)


if __name__ == "__main__":
    main()
