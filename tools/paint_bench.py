#!/usr/bin/env python
"""Timings of the distPaint.py drop-in (profiles/paint/README.md holds the numbers and the commands).

  kernels    on one MI355X: k_paint's HIP-event time per batch from the engine's kernel timers, beside the pack and pair kernels' time
             for the same windows (the yardstick) and the called-count pass pg_paint adds (k_hap_called), both modes.  Synthetic
             resident rows: --windows x --sites-per-window sites of --n-ind haploid individuals, --pops reference populations of
             --pop-size (the first individuals).
  driver     on one MI355X: wall clock of distPaint.py on a bgzipped .geno file of --sites sites that this tool writes itself.
  reference  where the reference is (no GPU needed): wall clock of the reference's distPaint.py (--reference DIR, run with the np.NaN
             shim that tests/golden/make_golden.py uses) on the first --sites sites of the same file -- few enough to finish in about a minute.

One JSON line on stdout, and into --out when given.  Needs no file outside the tree (but the reference, for `reference`)."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def names_of(n):
    return ["i%04d" % k for k in range(n)]                    # (sorted order = file order)


def pop_args(n_pops, pop_size):
    nm = names_of(n_pops * pop_size)
    return [x for p in range(n_pops) for x in ("-p", "P%d" % p, ",".join(nm[p * pop_size:(p + 1) * pop_size]))]


def geno_chunks(n_sites, n_ind, n_pops, pop_size, chunk=50000, seed=99):
    """the file's text chunk by chunk (the same lines whatever n_sites): individual k draws its alleles from source k // pop_size
    (the individuals behind the reference populations: a mosaic changing source every 10 000 sites), 5 % missing calls"""
    yield ("#CHROM\tPOS\t" + "\t".join(names_of(n_ind)) + "\n").encode()
    letters = np.frombuffer(b"ACGTN", dtype=np.uint8)
    for c0 in range(0, n_sites, chunk):
        n = min(chunk, n_sites - c0)
        rng = np.random.default_rng([seed, c0])
        src = np.minimum(np.arange(n_ind) // pop_size, n_pops)
        src = np.where(src < n_pops, src, (np.arange(n_ind) + c0 // 10000) % n_pops)
        freq = rng.choice([0.05, 0.3, 0.7, 0.95], size=(n, n_pops))
        base = rng.integers(0, 4, size=(n, 1))
        allele = np.where(rng.random((n, n_ind)) < freq[:, src], (base + 1) % 4, base)
        allele[rng.random((n, n_ind)) < 0.05] = 4
        cells = np.full((n, 2 * n_ind), ord("\t"), dtype=np.uint8)
        cells[:, 0::2] = letters[allele]
        cells[:, -1] = ord("\n")
        yield b"".join(b"chr1\t%d\t" % (c0 + i + 1) + cells[i].tobytes() for i in range(n))


def write_geno(path, n_sites, args, bgzf):
    from genomics_general_amd import genoio
    t0 = time.perf_counter()
    if bgzf:
        w = genoio.BgzfWriter(path)
        for piece in geno_chunks(n_sites, args.n_ind, args.pops, args.pop_size):
            w.write(piece)
        w.close()
    else:
        import gzip
        with gzip.open(path, "wb", compresslevel=1) as f:
            for piece in geno_chunks(n_sites, args.n_ind, args.pops, args.pop_size):
                f.write(piece)
    return round(time.perf_counter() - t0, 2)


def kernels(args):
    from genomics_general_amd import _lib, synth
    from genomics_general_amd.engine import Engine
    from genomics_general_amd.samples import HapLayout, SampleData
    n = args.n_ind
    nm = names_of(n)
    lay = HapLayout(SampleData(indNames=list(nm), ploidyDict={x: 1 for x in nm}), nm, "haplo")
    total = args.windows * args.sites_per_window
    eng = Engine(0)
    eng.set_layout(lay)
    eng.reserve(total)
    # the generator's haplotypes 2 d, 2 d + 1 of n / 2 diploids in --pops populations: slot k takes haplotype k
    eng.synth_fill(0, total, 0, synth.SEED_DEFAULT, args.sites_per_window, n // 2, args.pops, np.arange(n, dtype=np.int32), args.var, args.miss)
    lo = np.arange(args.windows, dtype=np.int64) * args.sites_per_window
    hi = lo + args.sites_per_window
    refs = [list(range(p * args.pop_size, (p + 1) * args.pop_size)) for p in range(args.pops)]
    fam = {"pack": _lib.K_PACK, "pairC": _lib.K_PAIRWISE, "pairD": _lib.K_PAIRD, "called": _lib.K_PAINT_CALLED, "paint": _lib.K_PAINT}
    out = {"what": "kernels", "windows": args.windows, "sites_per_window": args.sites_per_window, "individuals": n, "pops": args.pops,
           "pop_size": args.pop_size, "min_sites": args.min_sites, "var_thr": args.var, "miss_thr": args.miss, "rounds": args.rounds}
    for mode, kw in (("test", dict(p_threshold=0.05)), ("delta", dict(delta_threshold=0.005))):
        ms = {k: [] for k in fam}
        wall = []
        for r in range(args.warmup + args.rounds):
            eng.kernel_time_reset()
            t0 = time.perf_counter()
            wb = eng.batch(lo, hi)
            res = wb.paint(refs, args.min_sites, noresult=-1, **kw)
            dt = time.perf_counter() - t0
            if r >= args.warmup:
                wall.append(dt * 1e3)
                for k, kid in fam.items():
                    ms[k].append(eng.kernel_time(kid)[0])
        med = {k: round(float(np.median(v)), 4) for k, v in ms.items()}
        yard = med["pack"] + med["pairC"] + med["pairD"]
        out[mode] = dict(ms=med, pack_plus_pair_ms=round(yard, 4), paint_over_pack_plus_pair=round(med["paint"] / yard, 4),
                         called_over_pack_plus_pair=round(med["called"] / yard, 4), call_wall_ms=round(float(np.median(wall)), 2),
                         assigned_share=round(float((res != -1).mean()), 4), host_finished_cells=int(wb.paint_host_cells.sum()))
    eng.close()
    return out


def driver(args):
    with tempfile.TemporaryDirectory() as tmp:
        geno = os.path.join(tmp, "paint.geno.gz")
        t_write = write_geno(geno, args.sites, args, bgzf=True)
        size = os.path.getsize(geno)
        cmd = [sys.executable, os.path.join(ROOT, "distPaint.py"), "-g", geno, "-w", str(args.sites_per_window), "-m", str(args.min_sites),
               "-o", os.path.join(tmp, "out.tsv")] + pop_args(args.pops, args.pop_size)
        walls = []
        for r in range(args.warmup + args.rounds):
            t0 = time.perf_counter()
            r_ = subprocess.run(cmd + (["--delta_threshold", "0.005"] if args.delta else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=ROOT)
            dt = time.perf_counter() - t0
            assert r_.returncode == 0, r_.stderr.decode()[-2000:]
            if r >= args.warmup:
                walls.append(dt)
        with open(os.path.join(tmp, "out.tsv")) as f:
            rows = f.read().splitlines()
        cells = [c for ln in rows[1:] for c in ln.split("\t")[5:]]
        wall = float(np.median(walls))
        return {"what": "driver", "sites": args.sites, "individuals": args.n_ind, "pops": args.pops, "pop_size": args.pop_size,
                "window_sites": args.sites_per_window, "mode": "delta" if args.delta else "test", "file_bytes": size, "write_file_s": t_write,
                "wall_s": round(wall, 3), "walls_s": [round(w, 3) for w in walls], "sites_per_s": round(args.sites / wall),
                "rows": len(rows) - 1, "assigned_share": round(sum(c != "-1" for c in cells) / max(len(cells), 1), 4)}


def reference(args):
    assert args.reference, "reference: give --reference DIR (where the reference's distPaint.py and genomics.py are)"
    ref = args.reference
    # np.NaN left NumPy 2; the reference uses it for failed windows: set in the child's interpreter, the reference's files stay as they are
    wrap = ("import sys, runpy, numpy as np; np.NaN = np.nan; sys.path.insert(0, %r); sys.argv = sys.argv[1:]; "
            "runpy.run_path(sys.argv[0], run_name='__main__')" % ref)
    with tempfile.TemporaryDirectory() as tmp:
        geno = os.path.join(tmp, "paint.geno.gz")
        write_geno(geno, args.sites, args, bgzf=False)
        cmd = [sys.executable, "-W", "ignore", "-c", wrap, os.path.join(ref, "distPaint.py"), "-g", geno, "-w", str(args.sites_per_window),
               "-m", str(args.min_sites), "-T", str(args.threads), "-o", os.path.join(tmp, "ref.tsv")] + pop_args(args.pops, args.pop_size)
        t0 = time.perf_counter()
        r_ = subprocess.run(cmd + (["--delta_threshold", "0.005"] if args.delta else []), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        wall = time.perf_counter() - t0
        assert r_.returncode == 0, r_.stderr.decode()[-2000:]
        with open(os.path.join(tmp, "ref.tsv")) as f:
            rows = f.read().splitlines()
        return {"what": "reference", "sites": args.sites, "individuals": args.n_ind, "pops": args.pops, "pop_size": args.pop_size,
                "window_sites": args.sites_per_window, "threads": args.threads, "mode": "delta" if args.delta else "test",
                "wall_s": round(wall, 2), "sites_per_s": round(args.sites / wall), "rows": len(rows) - 1}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("what", choices=("kernels", "driver", "reference"))
    ap.add_argument("--windows", type=int, default=2000)
    ap.add_argument("--sites-per-window", type=int, default=25000)
    ap.add_argument("--sites", type=int, default=1000000, help="driver / reference: sites of the file")
    ap.add_argument("--n-ind", type=int, default=400)
    ap.add_argument("--pops", type=int, default=4)
    ap.add_argument("--pop-size", type=int, default=50)
    ap.add_argument("--min-sites", type=int, default=100)
    ap.add_argument("--var", type=int, default=30000, help="kernels: synth var_thr")
    ap.add_argument("--miss", type=int, default=3000, help="kernels: synth miss_thr")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--delta", action="store_true", help="driver / reference: --delta_threshold 0.005 instead of the test")
    ap.add_argument("--threads", type=int, default=1, help="reference: -T")
    ap.add_argument("--reference", help="reference: the directory of the reference's scripts")
    ap.add_argument("--out", help="also write the JSON line into this file")
    args = ap.parse_args()
    res = {"kernels": kernels, "driver": driver, "reference": reference}[args.what](args)
    line = json.dumps(res)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
