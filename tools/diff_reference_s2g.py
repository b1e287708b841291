"""The seqToGeno.py drop-in against the UNMODIFIED reference on random files x random command lines (host route, CPU only).

    python tools/diff_reference_s2g.py N SEED [--ref DIR] [--log profiles/s2g/diff_reference_s2g_<SEED>.log]

Case k is tests/golden/s2g_cases.random_case(SEED * 100003 + k): a seeded fasta or phylip file (one to nine sequences, wrapped at a
random width, now and then with blanks, descriptions, text in front, a longer later sequence, several alignments), a random mode,
-C / -N, -S in an order of its own, a ploidy list.  Every second case runs the drop-in in blocks of 2 000 bytes.  The reference runs
under the shim of tests/golden/make_golden.py.  Where it exits 0 the outputs must be equal byte for byte; where it dies the drop-in
must exit non-zero, and with status 1 (a short later sequence) must have written what the reference wrote.  A single -P k above 1, on which the reference raises TypeError, is the
README's stated divergence: such a case is counted apart.  No case is left out.
Prints one line per case and a summary; exit status 1 when any case differs."""
import argparse
import os
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
from s2g_cases import random_case  # noqa: E402


def one(k, seed, ref, wrap, tmp):
    text, argv = random_case(seed * 100003 + k)
    d = os.path.join(tmp, "c%d" % k)
    os.makedirs(d)
    inp = os.path.join(d, "in.txt")
    with open(inp, "w") as f:
        f.write(text)
    outs = {}
    for who, cmd, env in (("ref", [sys.executable, "-W", "ignore", "-c", wrap, os.path.join(ref, "seqToGeno.py")], {}),
                          ("own", [sys.executable, os.path.join(ROOT, "seqToGeno.py")],
                           dict({"PG_S2G_DEVICE": "0"}, **({"PG_STREAM_BYTES": "2000"} if k % 2 else {})))):
        out = os.path.join(d, who + ".geno")
        r = subprocess.run(cmd + argv + ["-s", inp, "-g", out], cwd=d, env=dict(os.environ, **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           timeout=900)
        data = None
        if os.path.exists(out):
            with open(out, "rb") as f:
                data = f.read()
        outs[who] = (r.returncode, data, r.stderr.decode(errors="replace"))
    (rc_r, d_r, err_r), (rc_o, d_o, _) = outs["ref"], outs["own"]
    single = "-P" in argv and (argv.index("-P") + 2 == len(argv) or argv[argv.index("-P") + 2].startswith("-")) and int(argv[argv.index("-P") + 1]) > 1
    if single and rc_r != 0 and "TypeError" in err_r:
        same = None                                            # (-P k: the reference raises TypeError, the drop-in takes k for every group)
    elif rc_r == 0:
        same = rc_o == 0 and d_o == d_r
    elif rc_o == 1:
        same = d_o == d_r                                      # (the rows before the line both stop on)
    else:
        same = rc_o == 2 and d_o is None
    return k, same, rc_r, rc_o, (d_r or b"").count(b"\n"), " ".join(argv)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("n", type=int)
    ap.add_argument("seed", type=int)
    ap.add_argument("--ref", default=os.environ.get("GG_REFERENCE", "/root/reference"))
    ap.add_argument("--log")
    a = ap.parse_args()
    wrap = ("import sys, runpy, numpy as np; np.NaN = np.nan; sys.path.insert(0, %r); sys.argv = sys.argv[1:]; "
            "runpy.run_path(sys.argv[0], run_name='__main__')" % a.ref)
    lines, differ, diverge, died, rows = [], 0, 0, 0, 0
    with tempfile.TemporaryDirectory() as tmp, ThreadPoolExecutor(max_workers=min(os.cpu_count() or 1, 16)) as ex:
        for k, same, rc_r, rc_o, n, argv in ex.map(lambda k: one(k, a.seed, a.ref, wrap, tmp), range(a.n)):
            differ += same is False
            diverge += same is None
            died += rc_r != 0
            rows += n
            lines.append("case %d %s reference=%d drop-in=%d lines=%d %s" % (k, "same" if same else "DIFFER" if same is False else "stated-divergence(-P k)", rc_r, rc_o, n, argv))
    lines.append("seed %d: %d cases, %d differ, %d are the stated divergence -P k (the reference raises TypeError), the reference died on %d in "
                 "all, %d lines written by the reference" % (a.seed, a.n, differ, diverge, died, rows))
    text = "\n".join(lines) + "\n"
    sys.stdout.write("\n".join(ln for ln in lines if "DIFFER" in ln or ln.startswith("seed")) + "\n")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write(text)
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
