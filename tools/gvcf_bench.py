"""Measurements of the genoToVCF.py drop-in (profiles/gvcf/README.md says where each number comes from).

    python tools/gvcf_bench.py --reference [--head 100000]      the UNMODIFIED reference's sites/s on a head of the file (CPU)
    python tools/gvcf_bench.py [--sites 5000000] [--rounds 3]   on an MI355X: process wall clock, fresh processes, alternating

The input is seeded: --sites sites x --samples diploids, phased, bgzipped (two alleles a site, 2 % missing cells).  The device runs are
`.geno.gz -> .vcf.gz` and `.geno.gz -> .vcf`; the yardsticks on the same file are the drop-in's own host route (PG_GVCF_DEVICE=0) and the
filterGenotypes.py drop-in with --noTest -of coded, which moves nearly the same bytes through the same block slot.  Every figure is a
median of --rounds runs with its range.  Results are merged into profiles/gvcf/gvcf_bench.json."""
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
OUT = os.path.join(ROOT, "profiles", "gvcf", "gvcf_bench.json")


def make_text(sites, samples, seed=1):
    """the .geno text: header + sites lines of `samples` phased diploid cells"""
    rng = np.random.default_rng(seed)
    head = ("\t".join(["#CHROM", "POS"] + ["d%d" % k for k in range(samples)]) + "\n").encode()
    parts = [head]
    step = 200000
    for a in range(0, sites, step):
        n = min(step, sites - a)
        two = rng.integers(0, 4, size=(n, 2))
        two[:, 1] = (two[:, 0] + 1 + rng.integers(0, 3, size=n)) % 4
        pick = rng.random((n, samples, 2)) < rng.random((n, 1, 1)) * 0.5
        al = np.where(pick, two[:, None, 1:2], two[:, None, 0:1])
        ch = np.frombuffer(b"ACGT", dtype=np.uint8)[al]
        ch[rng.random((n, samples)) < 0.02] = ord("N")
        cells = np.empty((n, samples, 4), dtype=np.uint8)
        cells[:, :, 0] = ord("\t")
        cells[:, :, 1] = ch[:, :, 0]
        cells[:, :, 2] = ord("/")
        cells[:, :, 3] = ch[:, :, 1]
        body = cells.reshape(n, samples * 4)
        for k in range(n):
            parts.append(b"chr%d\t%d" % (1 + (a + k) * 4 // max(sites, 1), a + k + 1))
            parts.append(body[k].tobytes())
            parts.append(b"\n")
    return b"".join(parts)


def timed(cmd, env):
    t0 = time.perf_counter()
    r = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
    dt = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError("%s: %s" % (" ".join(cmd), r.stderr.decode()[-2000:]))
    return dt, r.stderr.decode()


def summary(xs):
    return {"median_s": round(statistics.median(xs), 3), "min_s": round(min(xs), 3), "max_s": round(max(xs), 3), "runs": len(xs)}


def merge_json(section, value):
    data = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            data = json.load(f)
    data[section] = value
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    with open(OUT, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=5000000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--head", type=int, default=100000)
    ap.add_argument("--ref", default=os.environ.get("GG_REFERENCE", "/root/reference"))
    a = ap.parse_args()
    from genomics_general_amd import genoio
    script = os.path.join(ROOT, "VCF_processing", "genoToVCF.py")
    with tempfile.TemporaryDirectory() as tmp:
        if a.reference:
            text = make_text(a.head, a.samples)
            inp = os.path.join(tmp, "head.geno")
            with open(inp, "wb") as f:
                f.write(text)
            out = os.path.join(tmp, "o.vcf")
            t_ref, _ = timed([sys.executable, os.path.join(a.ref, "VCF_processing", "genoToVCF.py"), "-g", inp, "-f", "phased", "-o", out],
                             dict(os.environ, PYTHONPATH=a.ref))
            with open(out, "rb") as f:
                want = f.read()
            t_host, _ = timed([sys.executable, script, "-g", inp, "-f", "phased", "-o", out], dict(os.environ, PG_GVCF_DEVICE="0"))
            with open(out, "rb") as f:
                same = f.read() == want
            merge_json("reference", {"sites": a.head, "samples": a.samples, "text_bytes": len(text), "cpus": os.cpu_count(),
                                     "reference_s": round(t_ref, 2), "reference_sites_per_s": round(a.head / t_ref, 1),
                                     "host_route_s": round(t_host, 3), "host_route_sites_per_s": round(a.head / t_host, 1),
                                     "outputs_identical": same})
            return 0
        text = make_text(a.sites, a.samples)
        inp = os.path.join(tmp, "in.geno.gz")
        with open(inp, "wb") as f:
            f.write(genoio.bgzf_compress(text))
        runs = {
            "gvcf_device_to_vcf_gz": ([sys.executable, script, "-g", inp, "-f", "phased", "-o", os.path.join(tmp, "d.vcf.gz")], {"PG_GVCF_DEVICE": "1"}),
            "gvcf_device_to_vcf": ([sys.executable, script, "-g", inp, "-f", "phased", "-o", os.path.join(tmp, "d.vcf")], {"PG_GVCF_DEVICE": "1"}),
            "gvcf_host_route_to_vcf": ([sys.executable, script, "-g", inp, "-f", "phased", "-o", os.path.join(tmp, "h.vcf")],
                                       {"PG_GVCF_DEVICE": "0", "PG_HOST_THREADS": "16"}),
            "filter_coded_device_to_geno_gz": ([sys.executable, os.path.join(ROOT, "filterGenotypes.py"), "-i", inp, "--noTest", "-of", "coded",
                                                "-o", os.path.join(tmp, "f.geno.gz")], {"PG_FILTER_DEVICE": "1"}),
        }
        times = {k: [] for k in runs}
        timing = {}
        for _ in range(a.rounds):                              # alternating, each a fresh process
            for k, (cmd, extra) in runs.items():
                dt, err = timed(cmd, dict(os.environ, PG_TIMING="1", **extra))
                times[k].append(dt)
                timing[k] = [ln for ln in err.split("\n") if ln.startswith("PG_TIMING")][-1:]
        with open(os.path.join(tmp, "d.vcf"), "rb") as f, open(os.path.join(tmp, "h.vcf"), "rb") as g:
            same = f.read() == g.read()
        res = {k: summary(v) for k, v in times.items()}
        med = {k: v["median_s"] for k, v in res.items()}
        merge_json("gpu", {"sites": a.sites, "samples": a.samples, "text_bytes": len(text), "bgzf_bytes": os.path.getsize(inp),
                           "wall": res, "pg_timing": timing, "device_equals_host_route": same,
                           "host_route_over_device_vcf": round(med["gvcf_host_route_to_vcf"] / med["gvcf_device_to_vcf"], 2),
                           "device_vcf_gz_over_filter_coded": round(med["gvcf_device_to_vcf_gz"] / med["filter_coded_device_to_geno_gz"], 2)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
