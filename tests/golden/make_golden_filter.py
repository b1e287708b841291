"""Golden outputs of the UNMODIFIED reference filterGenotypes.py on the existing fixtures and one small edge file.

    python tests/golden/make_golden_filter.py        (needs the reference tree; writes tests/golden/filter/<case>.out.gz)

Every case is a command line of the reference; tests/test_filter_cpu.py and tests/test_gpu_filter.py run the drop-in on the same
command line and compare the text byte for byte.  The reference ends every run with sleep(10): the cases run in parallel.
Cases on which the reference hangs are not run here (tests/test_filter_cpu.py checks the drop-in's error exit on them).
"""
import os
import gzip
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.environ.get("GG_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "filter")

sys.path.insert(0, HERE)
from filter_cases import CASES, fixture_path  # noqa: E402


def run(case):
    name, fixture, argv = case
    cmd = [sys.executable, os.path.join(REF_DIR, "filterGenotypes.py"), "-i", fixture_path(fixture)] + [a.replace("@G", HERE) for a in argv]
    r = subprocess.run(cmd, cwd=REF_DIR, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (name, r.stderr.decode()[-2000:]))
    with open(os.path.join(OUT, name + ".out.gz"), "wb") as f:
        f.write(gzip.compress(r.stdout, mtime=0))
    return name, len(r.stdout)


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    with ThreadPoolExecutor(max_workers=min(len(CASES), 24)) as ex:
        for name, n in ex.map(run, CASES):
            print(name, n)
