#!/usr/bin/env python
"""Regenerate tests/golden/seq/ by running the UNMODIFIED reference's genoToSeq.py on the fixtures of cases.py and on the `seqmix`
fixture of seq_cases.py (written here).  Only runs where the reference is (make_golden.py names the place and holds the shim); the
fixture and the outputs it writes are committed.  A case on which the reference fails stops the script.

    python tests/golden/make_golden_seq.py [case-name ...]
"""
import gzip
import io
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, HERE)
from make_golden import REF, WRAP  # noqa: E402
from seq_cases import SEQ_CASES, SEQ_FIXTURE, SEQ_FIXTURE_HEADER, out_args, read_output, seq_fixture_lines  # noqa: E402


def make_fixture():
    path = os.path.join(HERE, SEQ_FIXTURE + ".geno.gz")
    with gzip.GzipFile(path, "wb", mtime=0) as raw:
        txt = io.TextIOWrapper(raw, newline="\n")
        txt.write("\t".join(SEQ_FIXTURE_HEADER) + "\n")
        for ln in seq_fixture_lines():
            txt.write(ln + "\n" if isinstance(ln, str) else "%s\t%d\t%s\n" % (ln[0], ln[1], "\t".join(ln[2])))
        txt.flush()
    return path


def run_case(case):
    geno = os.path.join(HERE, case["fixture"] + ".geno.gz")
    with tempfile.TemporaryDirectory() as tmp:
        argv = [a.format(geno=geno) for a in case["argv"]] + out_args(case, tmp)
        cmd = [sys.executable, "-W", "ignore", "-c", WRAP, os.path.join(REF, "genoToSeq.py")] + argv
        r = subprocess.run(cmd, cwd=tmp, env=dict(os.environ, PYTHONHASHSEED="0"), timeout=600, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        if r.returncode != 0:
            sys.stderr.write(r.stderr.decode()[-2000:])
            raise SystemExit("reference failed on " + case["name"])
        data = read_output(case, tmp, r.stdout)
    if not data:
        raise SystemExit("reference wrote nothing on " + case["name"])
    out = os.path.join(HERE, "seq", case["name"] + ".out.gz")
    with open(out, "wb") as raw, gzip.GzipFile(fileobj=raw, mode="wb", filename="", mtime=0) as f:
        f.write(data)
    return out, data


def main():
    want = set(sys.argv[1:])
    os.makedirs(os.path.join(HERE, "seq"), exist_ok=True)
    print("fixture", make_fixture())
    for case in SEQ_CASES:
        if want and case["name"] not in want:
            continue
        out, data = run_case(case)
        print("golden", case["name"], len(data), "bytes,", data.count(b">") + data.count(b"\n "), "alignment heads,",
              data.count(b"\n== ") + data.startswith(b"== "), "files", flush=True)


if __name__ == "__main__":
    main()
