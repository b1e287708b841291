#!/usr/bin/env python
"""Measurements for the windowStats.py drop-in (profiles/wstats/README.md says which of them were taken, and where).

    python tools/wstats_bench.py --reference [--sites 20000]          the unmodified reference's sites/s on a head of the table (CPU)
    python tools/wstats_bench.py --device [--sites 2000000] [--reps 3] wall clock of the drop-in, device route and PG_WS_DEVICE=0, fresh
                                                                       processes alternating, median and range (needs an MI355X)
    python tools/wstats_bench.py --kernels [--sites 4000000]           k_ws_stats per tier (HIP events) against a device-to-device copy
                                                                       of the value store, in this process (needs an MI355X)
    python tools/wstats_bench.py --freq [--sites 2000000] [--reps 3]   the freq.py drop-in's wall clock on a .geno file of the same sites
                                                                       and about the same bytes as the table (needs an MI355X)
    python tools/wstats_bench.py --rocprof [--sites 2000000]           one device-route run under `rocprofv3 --kernel-trace --stats`, a run of
                                                                       its own: the kernels' calls and times from its statistics file

The table is seeded: --cols columns of decimals with 2 % nan, one scaffold, a site every 10 bases; coordinate windows of --window bases
(default 10 000: 1000 sites a window) and all twelve statistics.  One JSON line per leg on the standard output."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REF = os.environ.get("GG_REFERENCE", "/root/reference")
WRAP = ("import sys, runpy, numpy as np; np.NaN = np.nan; sys.path.insert(0, %r); "
        "sys.argv = sys.argv[1:]; runpy.run_path(sys.argv[0], run_name='__main__')" % REF)
ALL = ["mean", "median", "min", "max", "sd", "sum", "q5", "q10", "q25", "q75", "q90", "q95"]


def write_table(path, n_sites, n_cols, seed=1):
    rng = np.random.default_rng(seed)
    with open(path, "w") as f:
        f.write("\t".join(["scaffold", "position"] + ["v%d" % k for k in range(n_cols)]) + "\n")
        for at in range(0, n_sites, 100000):
            n = min(100000, n_sites - at)
            vals = np.round(rng.normal(30.0, 12.0, size=(n, n_cols)), 4)
            holes = rng.random((n, n_cols)) < 0.02
            rows = []
            for k in range(n):
                rows.append("chr1\t%d\t%s" % ((at + k) * 10 + 1, "\t".join("nan" if h else repr(float(v)) for v, h in zip(vals[k], holes[k]))))
            f.write("\n".join(rows) + "\n")
    return os.path.getsize(path)


def reference_leg(args, tmp):
    path = os.path.join(tmp, "head.tsv")
    size = write_table(path, args.sites, args.cols)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, "-c", WRAP, os.path.join(REF, "windowStats.py"), "-i", path, "-w", str(args.window), "--stats"] + ALL,
                       cwd=REF, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    ours = subprocess.run([sys.executable, os.path.join(ROOT, "windowStats.py"), "-i", path, "-w", str(args.window), "--stats"] + ALL,
                          env=dict(os.environ, PG_WS_DEVICE="0"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    return dict(leg="reference", sites=args.sites, cols=args.cols, bytes=size, seconds=round(dt, 3), sites_per_s=round(args.sites / dt),
                host_route_same_bytes=bool(ours.returncode == 0 and ours.stdout == r.stdout))


def device_leg(args, tmp):
    path = os.path.join(tmp, "table.tsv")
    size = write_table(path, args.sites, args.cols)
    argv = [sys.executable, os.path.join(ROOT, "windowStats.py"), "-i", path, "-w", str(args.window), "--stats"] + ALL
    times = {"device": [], "host": []}
    outs = {}
    for _ in range(args.reps):
        for name, env in (("device", {"PG_WS_DEVICE": "1"}), ("host", {"PG_WS_DEVICE": "0"})):
            t0 = time.perf_counter()
            r = subprocess.run(argv, env=dict(os.environ, PG_TIMING="1", **env), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
            times[name].append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            outs[name] = (r.stdout, [ln for ln in r.stderr.decode().splitlines() if ln.startswith("PG_TIMING wstats")][-1])
    res = dict(leg="device", sites=args.sites, cols=args.cols, bytes=size, window_sites=args.window // 10, reps=args.reps,
               same_bytes=outs["device"][0] == outs["host"][0], device_counters=outs["device"][1])
    for name, t in times.items():
        res[name + "_s"] = dict(median=round(statistics.median(t), 3), min=round(min(t), 3), max=round(max(t), 3))
    return res


def kernels_leg(args):
    from genomics_general_amd import wstats
    rng = np.random.default_rng(5)
    vals = rng.normal(30.0, 12.0, size=(args.cols, args.sites))
    vals[rng.random(vals.shape) < 0.02] = np.nan
    dev = wstats.Device.from_values(0, vals)
    res = dict(leg="kernels", sites=args.sites, cols=args.cols, store_bytes=int(vals.nbytes))
    try:
        copies = [dev.copy_ms() for _ in range(4)][1:]
        res["d2d_copy_ms"] = round(statistics.median(copies), 3)
        for name, per, lds in (("lds_1000", 1000, 8192), ("lds_8000", 8000, 8192), ("big_1000", 1000, 256), ("big_100000", 100000, 8192)):
            lo = np.arange(0, args.sites - per + 1, per, dtype=np.int64)
            runs = []
            for _ in range(4):
                _, _, _, tiers, ms = dev.stats(lo, lo + per, (1 << 12) - 1, lds)
                runs.append(ms)
            res[name] = dict(windows=int(len(lo)), ms=round(statistics.median(runs[1:]), 3), lds_cells=int(tiers[0]), big_cells=int(tiers[1]))
    finally:
        dev.close()
    return res


def freq_leg(args, tmp):
    """the yardstick: the freq.py drop-in over as many sites in about as many bytes (phased diploid cells of 4 bytes each)"""
    table = os.path.join(tmp, "table.tsv")
    size = write_table(table, min(args.sites, 100000), args.cols)
    line = size / min(args.sites, 100000)
    n_dip = max(2, int(round((line - 14) / 4)))
    names = ["s%d" % k for k in range(n_dip)]
    rng = np.random.default_rng(3)
    geno = os.path.join(tmp, "same.geno")
    cells = np.array(["A/A", "A/T", "T/T", "N/N"])
    with open(geno, "w") as f:
        f.write("\t".join(["#CHROM", "POS"] + names) + "\n")
        for at in range(0, args.sites, 100000):
            n = min(100000, args.sites - at)
            pick = cells[rng.integers(0, 4, size=(n, n_dip))]
            f.write("\n".join("chr1\t%d\t%s" % ((at + k) * 10 + 1, "\t".join(pick[k])) for k in range(n)) + "\n")
    half = n_dip // 2
    argv = [sys.executable, os.path.join(ROOT, "freq.py"), "-g", geno, "-f", "phased", "-o", os.path.join(tmp, "freq.out"),
            "-p", "A", ",".join(names[:half]), "-p", "B", ",".join(names[half:])]
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        r = subprocess.run(argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        times.append(time.perf_counter() - t0)
        assert r.returncode == 0, r.stderr.decode()[-2000:]
    return dict(leg="freq", sites=args.sites, diploids=n_dip, bytes=os.path.getsize(geno), table_bytes_per_site=round(line, 1), reps=args.reps,
                freq_s=dict(median=round(statistics.median(times), 3), min=round(min(times), 3), max=round(max(times), 3)))


def rocprof_leg(args, tmp):
    import csv
    import glob
    path = os.path.join(tmp, "table.tsv")
    size = write_table(path, args.sites, args.cols)
    out = os.path.join(tmp, "trace")
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "-d", out, "-o", "ws", "--", sys.executable, os.path.join(ROOT, "windowStats.py"), "-i", path,
           "-w", str(args.window), "-o", os.path.join(tmp, "out.csv"), "--stats"] + ALL
    r = subprocess.run(cmd, env=dict(os.environ, PG_WS_DEVICE="1"), stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    kernels = {}
    for stats_file in glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True):
        with open(stats_file) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                if any(k in name for k in ("k_ws_", "k_rows_scan", "k_inflate", "k_nl_")):
                    kernels[name.split("(")[0]] = dict(calls=int(row.get("Calls", 0)), total_ms=round(float(row.get("TotalDurationNs", 0)) / 1e6, 3))
    return dict(leg="rocprof", sites=args.sites, cols=args.cols, bytes=size, kernels=kernels)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--device", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--freq", action="store_true")
    ap.add_argument("--rocprof", action="store_true")
    ap.add_argument("--sites", type=int, default=None)
    ap.add_argument("--cols", type=int, default=4)
    ap.add_argument("--window", type=int, default=10000)
    ap.add_argument("--reps", type=int, default=3)
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        if args.reference:
            args.sites = args.sites or 20000
            print(json.dumps(reference_leg(args, tmp)), flush=True)
        if args.device:
            args.sites = args.sites or 2000000
            print(json.dumps(device_leg(args, tmp)), flush=True)
        if args.kernels:
            args.sites = args.sites or 4000000
            print(json.dumps(kernels_leg(args)), flush=True)
        if args.freq:
            args.sites = args.sites or 2000000
            print(json.dumps(freq_leg(args, tmp)), flush=True)
        if args.rocprof:
            args.sites = args.sites or 2000000
            print(json.dumps(rocprof_leg(args, tmp)), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
