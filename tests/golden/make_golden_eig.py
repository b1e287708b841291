"""Golden outputs of the UNMODIFIED reference tools/genoToEigenstrat.py on the existing fixtures and those under eig/.

    python tests/golden/make_golden_eig.py        (needs the reference tree; writes tests/golden/eig/<case>.{geno,snp,ind}.out.gz)

Every case is a command line of the reference, run with the reference directory on PYTHONPATH (the script imports genomics from
there); tests/test_eig_cpu.py and tests/test_gpu_eig.py run the drop-in on the same command line and compare the three files byte for
byte.
"""
import gzip
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.environ.get("GG_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "eig")

sys.path.insert(0, HERE)
from eig_cases import CASES, OUTPUTS, fixture_path  # noqa: E402


def run(case):
    name, fixture, argv = case
    with tempfile.TemporaryDirectory() as tmp:
        outs = {k: os.path.join(tmp, "out." + k) for k in OUTPUTS}
        cmd = [sys.executable, os.path.join(REF_DIR, "tools", "genoToEigenstrat.py"), "-g", fixture_path(fixture), "--genoOutFile", outs["geno"],
               "--snpOutFile", outs["snp"], "--indOutFile", outs["ind"]] + [a.replace("@G", HERE) for a in argv]
        env = dict(os.environ, PYTHONPATH=REF_DIR)
        r = subprocess.run(cmd, cwd=REF_DIR, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("%s: %s" % (name, r.stderr.decode()[-2000:]))
        sizes = []
        for k in OUTPUTS:
            with open(outs[k], "rb") as f:
                data = f.read()
            with open(os.path.join(OUT, "%s.%s.out.gz" % (name, k)), "wb") as f:
                f.write(gzip.compress(data, mtime=0))
            sizes.append(len(data))
    return name, sizes


if __name__ == "__main__":
    os.makedirs(OUT, exist_ok=True)
    with ThreadPoolExecutor(max_workers=16) as ex:
        for name, n in ex.map(run, CASES):
            print(name, n)
