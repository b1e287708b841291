#!/usr/bin/env python
"""Timings of the sfs.py drop-in on one MI355X (profiles/sfs/README.md holds the numbers and the commands).

  (1) the accumulation alone over resident synthetic rows (k_sfs_rows, HIP events) against k_site_counts alone over the same rows, in
      one process, alternating -- both read every row once;
  (2) the default table route (LDS tables + wave aggregation) against the forced global route (PG_SFS_LDS=0) on the same rows, alternating;
  (3) the whole driver on a bgzipped .geno file it writes itself, beside freq.py on the same file (wall clock of the two programs).

The shape is the north star's (200 diploids in 4 populations) cut down by --sites / --n-dip; the rows have no missing calls (--miss 0), or
no site of 400 haplotypes would be complete.  One JSON line on stdout.  Needs no reference and no file outside the tree."""
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
from genomics_general_amd import genoio, synth  # noqa: E402
from genomics_general_amd.engine import Engine  # noqa: E402
from genomics_general_amd.samples import HapLayout, SampleData  # noqa: E402


def layout_of(n_dip, n_pops):
    names = ["s%d" % d for d in range(n_dip)]
    per = n_dip // n_pops
    sd = SampleData(indNames=list(names), popNames=["pop%d" % k for k in range(n_pops)], popInds=[names[k * per:(k + 1) * per] for k in range(n_pops)])
    lay = HapLayout(sd, names, "phased")
    slot_gen = np.array([2 * names.index(nm) + k for nm in lay.ind_order for k in range(2)], dtype=np.int32)
    return names, lay, slot_gen


def med(xs):
    return round(float(np.median(xs)), 4)


def accumulation(args):
    names, lay, slot_gen = layout_of(args.n_dip, args.n_pops)
    eng = Engine(0)
    eng.set_layout(lay)
    eng.reserve(args.sites)
    eng.synth_fill(0, args.sites, 0, synth.SEED_DEFAULT, args.sites // 4 + 1, args.n_dip, args.n_pops, slot_gen, args.var, args.miss)
    P = args.n_pops
    ext = [2 * (args.n_dip // P) + 1] * P
    groups = [[k] for k in range(P)] + [[a, b] for a in range(P) for b in range(a + 1, P)]
    if args.quartet:
        groups.append(list(range(4)))
    out = {"sites": args.sites, "haplotypes": lay.n_hap, "pops": P, "row_bytes": eng.row_pitch // 2, "groups": len(groups), "var_thr": args.var, "miss_thr": args.miss}
    t_counts, t_sfs = {"default": [], "global": []}, {"default": [], "global": []}
    for r in range(args.warmup + args.rounds):
        for mode in ("default", "global"):
            os.environ["PG_SFS_LDS"] = "0" if mode == "global" else "1"
            cells, on_lds = eng.sfs_begin(ext, groups, 1)
            a = eng.time_site_counts(0, args.sites)
            b = eng.sfs_add_sites(0, args.sites, 0, list(range(P)), -1)
            n_cells = len(eng.sfs_read()[0])
            eng.sfs_end()
            if r >= args.warmup:
                t_counts[mode].append(a)
                t_sfs[mode].append(b)
            out["groups_on_lds_" + mode] = int(on_lds.sum())
    os.environ.pop("PG_SFS_LDS", None)
    out["touched_cells"] = n_cells
    out["k_site_counts_ms"] = med(t_counts["default"] + t_counts["global"])
    out["k_sfs_rows_ms_default"], out["k_sfs_rows_ms_global"] = med(t_sfs["default"]), med(t_sfs["global"])
    out["k_sfs_rows_ms_default_min"], out["k_sfs_rows_ms_global_min"] = round(min(t_sfs["default"]), 4), round(min(t_sfs["global"]), 4)
    out["ratio_sfs_over_site_counts"] = round(out["k_sfs_rows_ms_default"] / out["k_site_counts_ms"], 3)
    out["ratio_global_over_default"] = round(out["k_sfs_rows_ms_global"] / out["k_sfs_rows_ms_default"], 3)
    out["rows_GBps_default"] = round(args.sites * out["row_bytes"] / out["k_sfs_rows_ms_default"] / 1e6, 1)
    eng.close()
    return out


def write_bgzf_geno(path, n_sites, n_dip, n_pops, var, miss):
    names, lay, slot_gen = layout_of(n_dip, n_pops)
    sid, pos = synth.dense_sites(n_sites, 2)
    codes = synth.gen_codes(synth.SEED_DEFAULT, sid, pos, n_dip, n_pops, var_thr=var, miss_thr=miss)
    letters = np.frombuffer(b"NACNGNNNT", dtype=np.uint8)[codes]                 # one-hot code -> base
    cells = np.empty((n_sites, n_dip, 4), dtype=np.uint8)
    cells[:, :, 0], cells[:, :, 1], cells[:, :, 2], cells[:, :, 3] = letters[:, 0::2], ord("/"), letters[:, 1::2], ord("\t")
    cells[:, -1, 3] = ord("\n")
    body = cells.reshape(n_sites, -1)
    with genoio.BgzfWriter(path) as w:
        w.write(("#CHROM\tPOS\t" + "\t".join(names) + "\n").encode())
        for a in range(0, n_sites, 50000):
            w.write(b"".join(b"chr%d\t%d\t" % (s + 1, p) + row.tobytes() for s, p, row in zip(sid[a:a + 50000], pos[a:a + 50000], body[a:a + 50000])))
    return names


def drivers(args):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        geno = os.path.join(tmp, "bench.geno.gz")
        names = write_bgzf_geno(geno, args.file_sites, args.file_dip, 4, args.var, 0)
        per = args.file_dip // 4
        pops = []
        for k in range(4):
            pops += ["-p", "pop%d" % k, ",".join(names[k * per:(k + 1) * per])]
        out.update(file_sites=args.file_sites, file_diploids=args.file_dip, file_bytes=os.path.getsize(geno))
        cmds = {"sfs_py_s": [os.path.join(ROOT, "sfs.py"), "-i", geno, "--inputType", "genotypes", "--doPairs", "--pref", os.path.join(tmp, "o_")] + pops,
                "freq_py_s": [os.path.join(ROOT, "freq.py"), "-g", geno, "-o", os.path.join(tmp, "freq.tsv")] + pops}
        times = {k: [] for k in cmds}
        for r in range(3):
            for k, cmd in cmds.items():
                t0 = time.perf_counter()
                subprocess.run([sys.executable] + cmd, check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
                times[k].append(time.perf_counter() - t0)
        for k in cmds:
            out[k] = med(times[k])
            out[k + "_all"] = [round(x, 3) for x in times[k]]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=10_000_000, help="resident rows (the north star has 1e8)")
    ap.add_argument("--n-dip", type=int, default=200)
    ap.add_argument("--n-pops", type=int, default=4)
    ap.add_argument("--var", type=int, default=synth.VAR_THR, help="variable sites out of 65536 (default: 10 %%, monomorphic-dominated)")
    ap.add_argument("--miss", type=int, default=0, help="missing calls out of 65536")
    ap.add_argument("--quartet", action="store_true", help="add the 4-D spectrum (global route)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--file-sites", type=int, default=400_000)
    ap.add_argument("--file-dip", type=int, default=40)
    ap.add_argument("--no-drivers", action="store_true")
    ap.add_argument("--no-kernels", action="store_true")
    args = ap.parse_args()
    out = {}
    if not args.no_kernels:
        out.update(accumulation(args))
    if not args.no_drivers:
        out.update(drivers(args))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
