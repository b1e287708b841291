"""filterGenotypes.py drop-in: the device route against the host route on one synthetic bgzipped sample, and both against the
reference's measured rate.

    python tools/filter_bench.py [--sites N] [--samples 200] [--out profiles/filter/filter_bench.json]

Writes a `.geno.gz` of N sites x S diploids (fixed-width cells, 9-digit positions, ~5 % missing, ~30 % variable sites; --host-sites:
a second one of the first M of them for the host route, which is slower by orders of magnitude) to a scratch
directory, then runs `filterGenotypes.py --minAlleles 2 --minCalls S/2` as a child process per route and output (`-o x.geno.gz` and
plain): process wall-clock seconds (context creation included), the driver's own seconds after it (PG_TIMING filter_s), sites/s and
GB/s of input text.  The reference's rate is the one measured with one worker on 20 000 sites x 200 diploids (19 s of CPU, i.e.
about 1 000 sites/s per worker; its closing sleep(10) left out)."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REFERENCE_SITES_PER_S = 20000 / 19.0


def make_sample(path, n_sites, n_samples, seed=1):
    """the cells of one stretch of 200 000 random rows, repeated with new positions (the work per line is what counts here)"""
    from genomics_general_amd import genoio
    R = np.random.default_rng(seed)
    menu = np.frombuffer(b"A/A\tA/T\tT/T\tN/N\tC/C\tC/G\tG/G\tG|C\t", dtype=np.uint8).reshape(8, 4)
    head = ("\t".join(["#CHROM", "POS"] + ["s%d" % k for k in range(n_samples)]) + "\n").encode()
    step = min(200000, n_sites)
    var = R.random(step) < 0.3
    base = np.where(R.random(step) < 0.5, 0, 4)                       # A/T sites or C/G sites
    g = np.where(var[:, None], base[:, None] + R.integers(0, 3, (step, n_samples)), base[:, None] + np.where(base[:, None] == 0, 0, 2))
    g = np.where(R.random((step, n_samples)) < 0.05, 3, g)
    cells = menu[g].reshape(step, n_samples * 4)
    cells[:, -1] = 10
    chrom = np.frombuffer(b"chr1\t", dtype=np.uint8)[None, :].repeat(step, 0)
    tab = np.full((step, 1), 9, np.uint8)
    with open(path, "wb") as out:
        out.write(genoio.bgzf_compress(head, eof_marker=False))
        for a in range(0, n_sites, step):
            n = min(step, n_sites - a)
            pos = np.char.zfill((np.arange(a, a + n) + 1).astype(str), 9).astype("S9").view(np.uint8).reshape(n, 9)
            out.write(genoio.bgzf_compress(np.concatenate([chrom[:n], pos, tab[:n], cells[:n]], 1).tobytes(), eof_marker=False))
        out.write(genoio.bgzf_compress(b"", eof_marker=True))


def run(inp, out, device, n_samples):
    env = dict(os.environ, PG_TIMING="1", PG_FILTER_DEVICE="1" if device else "0")
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, "filterGenotypes.py"), "-i", inp, "-o", out, "--minAlleles", "2", "--minCalls",
                        str(n_samples // 2)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, cwd=ROOT)
    wall = time.perf_counter() - t0
    if r.returncode != 0:
        raise RuntimeError(r.stderr.decode()[-2000:])
    info = dict(kv.split("=", 1) for kv in re.search(r"PG_TIMING filter (.*)", r.stderr.decode()).group(1).split())
    return wall, info


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=2000000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--host-sites", type=int, default=None, help="the host route on the first N sites only (default: all)")
    ap.add_argument("--out", default=None)
    ap.add_argument("--dir", default=None, help="scratch directory (default: a temporary one)")
    ap.add_argument("--keep", action="store_true", help="keep the sample (for a rocprofv3 run of its own)")
    a = ap.parse_args()
    d = a.dir or tempfile.mkdtemp(prefix="filter_bench_")
    os.makedirs(d, exist_ok=True)
    inp = os.path.join(d, "sample.geno.gz")
    t0 = time.perf_counter()
    if not os.path.exists(inp):
        make_sample(inp, a.sites, a.samples)
    host_sites = min(a.host_sites or a.sites, a.sites)
    inp_host = inp
    if host_sites < a.sites:
        inp_host = os.path.join(d, "sample_host.geno.gz")
        if not os.path.exists(inp_host):
            make_sample(inp_host, host_sites, a.samples)
    gen_s = time.perf_counter() - t0
    text_bytes = None
    res = dict(sites=a.sites, host_sites=host_sites, samples=a.samples, sample_gz_bytes=os.path.getsize(inp), sample_s=round(gen_s, 2),
               reference_sites_per_s=round(REFERENCE_SITES_PER_S, 1), runs=[])
    outs = {}
    for device in (True, False):
        for gz in (True, False):
            o = os.path.join(d, "out_%s.geno%s" % ("dev" if device else "host", ".gz" if gz else ""))
            n = a.sites if device else host_sites
            wall, info = run(inp if device else inp_host, o, device, a.samples)
            if device:
                text_bytes = int(info["text_bytes"])
            fs = float(info["filter_s"])
            res["runs"].append(dict(route="device" if device else "host", output="geno.gz" if gz else "geno", wall_s=round(wall, 3),
                                    filter_s=round(fs, 3), sites=n, sites_per_s_wall=round(n / wall), sites_per_s_filter=round(n / fs),
                                    text_bytes=int(info["text_bytes"]), text_GB_per_s_wall=round(int(info["text_bytes"]) / wall / 1e9, 3), rows=int(info["rows"]),
                                    device_blocks=int(info.get("device_blocks", 0)), device_host_blocks=int(info.get("device_host_blocks", 0))))
            if not gz:
                with open(o, "rb") as f:
                    outs[device] = f.read()
    res["text_bytes"] = text_bytes
    dev_rows = outs[True].split(b"\n")
    host_rows = outs[False].split(b"\n")
    res["device_equals_host_on_common_lines"] = dev_rows[:len(host_rows) - 1] == host_rows[:-1]
    dev_gz = [r for r in res["runs"] if r["route"] == "device" and r["output"] == "geno.gz"][0]
    res["device_gz_vs_reference_x"] = round(dev_gz["sites_per_s_wall"] / REFERENCE_SITES_PER_S, 1)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")
    if not a.keep and not a.dir:
        for fn in os.listdir(d):
            os.remove(os.path.join(d, fn))
        os.rmdir(d)


if __name__ == "__main__":
    main()
