"""Measurements of the genoToPlink.py drop-in (profiles/plink/README.md says where each number comes from).

    python tools/plink_bench.py --reference [--head 20000]       the UNMODIFIED reference's sites/s on a head of the file (CPU)
    python tools/plink_bench.py [--sites 300000] [--rounds 3]    on an MI355X: process wall clock, fresh processes, alternating
    python tools/plink_bench.py --kernels [--sites 300000]       on an MI355X: a rocprofv3 --kernel-trace --stats run of its own per command

The input is gvcf_bench.make_text's: --sites sites x --samples diploids, phased, bgzipped.  The runs on the same file are the device
route, the drop-in's own host route (PG_PED_DEVICE=0, 16 host threads) and the genoToSeq.py drop-in with --splitPhased in cat mode,
the yardstick: the same transpose with half the output bytes and no .map.  Every figure is a median of --rounds runs with its range;
PG_TIMING's line of the last round splits reading and writing.  --kernels leaves the kernels' total milliseconds as the profiler's
own table has them.  Results are merged into --out (profiles/plink/plink_bench.json)."""
import argparse
import csv
import glob
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from gvcf_bench import make_text  # noqa: E402

KERNELS = ("k_ped_lines", "k_ped_map", "k_ped_tile", "k_seq_lines", "k_seq_rows", "k_seq_tile", "k_rows_scan", "k_inflate")


def timed(cmd, env):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (" ".join(cmd), r.stderr.decode()[-2000:]))
    return dt, r.stderr.decode()


def summary(xs):
    return {"median_s": round(statistics.median(xs), 3), "min_s": round(min(xs), 3), "max_s": round(max(xs), 3), "runs": len(xs)}


def merge_json(path, section, value):
    data = {}
    if os.path.exists(path):
        with open(path) as f:
            data = json.load(f)
    data[section] = value
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def ped_cmd(script, inp, tmp, tag):
    return [sys.executable, script, "-g", inp, "-f", "phased", "--prefix", os.path.join(tmp, tag)]


def seq_cmd(inp, tmp, tag):
    return [sys.executable, os.path.join(ROOT, "genoToSeq.py"), "-g", inp, "-s", os.path.join(tmp, tag + ".fa"), "--splitPhased"]


def same_files(tmp, a, b):
    for k in ("ped", "map"):
        with open(os.path.join(tmp, "%s.%s" % (a, k)), "rb") as f, open(os.path.join(tmp, "%s.%s" % (b, k)), "rb") as g:
            if f.read() != g.read():
                return False
    return True


def kernel_ms(cmd, env, tmp, tag):
    """{kernel: [calls, total ms]} of one profiled run of cmd, from rocprofv3's kernel_stats table"""
    d = os.path.join(tmp, "prof_" + tag)
    timed(["rocprofv3", "--kernel-trace", "--stats", "-d", d, "-o", tag, "--output-format", "csv", "--"] + cmd, env)
    out = {}
    for path in glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True):
        with open(path) as f:
            for row in csv.DictReader(f):
                name = row.get("Name", "")
                for k in KERNELS:
                    if name.startswith(k) or name.startswith("void " + k) or ("::" + k) in name:
                        cur = out.setdefault(k, [0, 0.0])
                        cur[0] += int(row["Calls"])
                        cur[1] = round(cur[1] + float(row["TotalDurationNs"]) / 1e6, 3)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=300000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--head", type=int, default=20000)
    ap.add_argument("--ref", default=os.environ.get("GG_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "plink", "plink_bench.json"))
    a = ap.parse_args()
    from genomics_general_amd import genoio
    script = os.path.join(ROOT, "tools", "genoToPlink.py")
    with tempfile.TemporaryDirectory() as tmp:
        if a.reference:
            text = make_text(a.head, a.samples)
            inp = os.path.join(tmp, "head.geno")
            with open(inp, "wb") as f:
                f.write(text)
            t_ref, _ = timed(ped_cmd(os.path.join(a.ref, "tools", "genoToPlink.py"), inp, tmp, "r"), dict(os.environ, PYTHONPATH=a.ref))
            t_host, _ = timed(ped_cmd(script, inp, tmp, "h"), dict(os.environ, PG_PED_DEVICE="0"))
            merge_json(a.out, "reference", {"sites": a.head, "samples": a.samples, "text_bytes": len(text), "cpus": os.cpu_count(),
                                            "reference_s": round(t_ref, 2), "reference_sites_per_s": round(a.head / t_ref, 1),
                                            "host_route_s": round(t_host, 3), "host_route_sites_per_s": round(a.head / t_host, 1),
                                            "outputs_identical": same_files(tmp, "r", "h")})
            return 0
        text = make_text(a.sites, a.samples)
        inp = os.path.join(tmp, "in.geno.gz")
        with open(inp, "wb") as f:
            f.write(genoio.bgzf_compress(text))
        runs = {
            "ped_device": (ped_cmd(script, inp, tmp, "d"), {"PG_PED_DEVICE": "1"}),
            "ped_host_route": (ped_cmd(script, inp, tmp, "h"), {"PG_PED_DEVICE": "0", "PG_HOST_THREADS": "16"}),
            "seq_device_split_phased_cat": (seq_cmd(inp, tmp, "s"), {"PG_SEQ_DEVICE": "1"}),
        }
        if a.kernels:
            res = {k: kernel_ms(cmd, dict(os.environ, **extra), tmp, k) for k, (cmd, extra) in runs.items() if k != "ped_host_route"}
            merge_json(a.out, "kernel_trace_%d" % a.sites, {"sites": a.sites, "samples": a.samples, "calls_and_total_ms": res})
            return 0
        times = {k: [] for k in runs}
        timing = {}
        for _ in range(a.rounds):                              # alternating, each a fresh process
            for k, (cmd, extra) in runs.items():
                dt, err = timed(cmd, dict(os.environ, PG_TIMING="1", **extra))
                times[k].append(dt)
                timing[k] = [ln for ln in err.split("\n") if ln.startswith("PG_TIMING")][-1:]
        res = {k: summary(v) for k, v in times.items()}
        med = {k: v["median_s"] for k, v in res.items()}
        merge_json(a.out, "gpu_%d" % a.sites, {"sites": a.sites, "samples": a.samples, "text_bytes": len(text), "bgzf_bytes": os.path.getsize(inp),
                                               "ped_bytes": os.path.getsize(os.path.join(tmp, "d.ped")),
                                               "wall": res, "pg_timing": timing, "device_equals_host_route": same_files(tmp, "d", "h"),
                                               "host_route_over_device": round(med["ped_host_route"] / med["ped_device"], 2),
                                               "device_over_seq_device": round(med["ped_device"] / med["seq_device_split_phased_cat"], 2)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
