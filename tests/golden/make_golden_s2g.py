#!/usr/bin/env python
"""Regenerate tests/golden/s2g/ by running the UNMODIFIED reference's seqToGeno.py on the fixtures of s2g_cases.py (written here from
fixture_text()) and on three of the goldens of make_golden_seq.py.  Only runs where the reference is (make_golden.py names the place
and holds the shim); the fixtures and the outputs are committed.  A case on which the reference fails stops the script.

    python tests/golden/make_golden_s2g.py [case-name ...]
"""
import gzip
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden import REF, WRAP  # noqa: E402
from s2g_cases import CASES, FIXTURES, fixture_text, input_bytes  # noqa: E402


def run_reference(data, argv, how, tmp):
    """(exit status, output bytes, stderr) of the reference on the input bytes `data`"""
    inp = os.path.join(tmp, "in.txt" + (".gz" if how == "gz" else ""))
    with open(inp, "wb") as f:
        f.write(gzip.compress(data, mtime=0) if how == "gz" else data)
    out = os.path.join(tmp, "out.geno" + (".gz" if how == "outgz" else ""))
    args = list(argv) + ([] if how == "stdin" else ["-s", inp]) + ([] if how == "stdout" else ["-g", out])
    cmd = [sys.executable, "-W", "ignore", "-c", WRAP, os.path.join(REF, "seqToGeno.py")] + args
    r = subprocess.run(cmd, cwd=tmp, env=dict(os.environ, PYTHONHASHSEED="0"), timeout=600, input=data if how == "stdin" else None,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if how == "stdout":
        got = r.stdout
    elif not os.path.exists(out):
        got = b""
    elif how == "outgz":
        try:
            with gzip.open(out, "rb") as f:
                got = f.read()
        except (EOFError, OSError):
            got = b""
    else:
        with open(out, "rb") as f:
            got = f.read()
    return r.returncode, got, r.stderr.decode(errors="replace")


def main():
    want = set(sys.argv[1:])
    os.makedirs(os.path.join(HERE, "s2g"), exist_ok=True)
    for name in FIXTURES:
        with open(os.path.join(HERE, "s2g", name), "wb") as f:
            f.write(fixture_text(name).encode("ascii"))
    for name, inp, argv, how in CASES:
        if want and name not in want:
            continue
        with tempfile.TemporaryDirectory() as tmp:
            rc, data, err = run_reference(input_bytes(inp), argv, how, tmp)
        if rc != 0 or not data:
            sys.stderr.write(err[-2000:])
            raise SystemExit("reference failed on " + name)
        with open(os.path.join(HERE, "s2g", name + ".out.gz"), "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
            f.write(data)
        print("golden", name, len(data), "bytes,", data.count(b"\n"), "lines", flush=True)


if __name__ == "__main__":
    main()
