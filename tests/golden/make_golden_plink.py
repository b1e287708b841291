"""Golden outputs of the UNMODIFIED reference tools/genoToPlink.py on the existing fixtures and those under plink/.

    python tests/golden/make_golden_plink.py        (needs the reference tree; writes tests/golden/plink/<case>.{ped,map,fam}.out.gz)

Every case is a command line of the reference, run with the reference directory on PYTHONPATH (the script imports genomics from
there); tests/test_plink_cpu.py and tests/test_gpu_plink.py run the drop-in on the same command line and compare the files byte for
byte.  A case on which the reference does not exit 0 is an error here: such inputs belong to the rejection and stop tests.
"""
import gzip
import os
import shutil
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
REF_DIR = os.environ.get("GG_REFERENCE", "/root/reference")
OUT = os.path.join(HERE, "plink")

sys.path.insert(0, HERE)
from plink_cases import CASES, command, fixture_path  # noqa: E402


def run(case):
    name, fixture, argv = case
    with tempfile.TemporaryDirectory() as tmp:
        inp = os.path.join(tmp, "in" + (".geno.gz" if fixture_path(fixture).endswith(".gz") else ".geno"))
        shutil.copy(fixture_path(fixture), inp)
        args, outs = command(argv, inp, tmp)
        cmd = [sys.executable, os.path.join(REF_DIR, "tools", "genoToPlink.py"), "-g", inp] + args
        r = subprocess.run(cmd, cwd=REF_DIR, env=dict(os.environ, PYTHONPATH=REF_DIR), stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=600)
        if r.returncode != 0:
            raise RuntimeError("%s: %s" % (name, r.stderr.decode()[-2000:]))
        sizes = []
        for k, p in outs.items():
            with open(p, "rb") as f:
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
