"""Measurements of the genoToEigenstrat.py drop-in (profiles/eig/README.md says where each number comes from).

    python tools/eig_bench.py --reference [--head 100000]      the UNMODIFIED reference's sites/s on a head of the file (CPU)
    python tools/eig_bench.py [--sites 300000] [--rounds 3]    on an MI355X: process wall clock, fresh processes, alternating

The input is gvcf_bench.make_text's: --sites sites x --samples diploids, phased, bgzipped (two alleles a site, 2 % missing cells), so
nearly every site is kept.  The runs on the same file are the device route, the drop-in's own host route (PG_EIG_DEVICE=0, 16 host
threads) and the genoToVCF.py drop-in to plain text, the yardstick of a per-line route through the same block slot.  Every figure is a
median of --rounds runs with its range; PG_TIMING's line of the last round splits block loop and start-up.  Results are merged into
--out (profiles/eig/eig_bench.json)."""
import argparse
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


def eig_cmd(script, inp, tmp, tag):
    return [sys.executable, script, "-g", inp, "-f", "phased", "--genoOutFile", os.path.join(tmp, tag + ".geno"), "--snpOutFile",
            os.path.join(tmp, tag + ".snp"), "--indOutFile", os.path.join(tmp, tag + ".ind")]


def same_files(tmp, a, b):
    for k in ("geno", "snp", "ind"):
        with open(os.path.join(tmp, "%s.%s" % (a, k)), "rb") as f, open(os.path.join(tmp, "%s.%s" % (b, k)), "rb") as g:
            if f.read() != g.read():
                return False
    return True


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=300000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--head", type=int, default=100000)
    ap.add_argument("--ref", default=os.environ.get("GG_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eig", "eig_bench.json"))
    a = ap.parse_args()
    from genomics_general_amd import genoio
    script = os.path.join(ROOT, "tools", "genoToEigenstrat.py")
    with tempfile.TemporaryDirectory() as tmp:
        if a.reference:
            text = make_text(a.head, a.samples)
            inp = os.path.join(tmp, "head.geno")
            with open(inp, "wb") as f:
                f.write(text)
            t_ref, _ = timed(eig_cmd(os.path.join(a.ref, "tools", "genoToEigenstrat.py"), inp, tmp, "r"), dict(os.environ, PYTHONPATH=a.ref))
            t_host, _ = timed(eig_cmd(script, inp, tmp, "h"), dict(os.environ, PG_EIG_DEVICE="0"))
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
            "eig_device": (eig_cmd(script, inp, tmp, "d"), {"PG_EIG_DEVICE": "1"}),
            "eig_host_route": (eig_cmd(script, inp, tmp, "h"), {"PG_EIG_DEVICE": "0", "PG_HOST_THREADS": "16"}),
            "gvcf_device_to_vcf": ([sys.executable, os.path.join(ROOT, "VCF_processing", "genoToVCF.py"), "-g", inp, "-f", "phased", "-o",
                                    os.path.join(tmp, "d.vcf")], {"PG_GVCF_DEVICE": "1"}),
        }
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
                                               "wall": res, "pg_timing": timing, "device_equals_host_route": same_files(tmp, "d", "h"),
                                               "host_route_over_device": round(med["eig_host_route"] / med["eig_device"], 2),
                                               "device_over_gvcf_device": round(med["eig_device"] / med["gvcf_device_to_vcf"], 2)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
