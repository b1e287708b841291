#!/usr/bin/env python
"""mergeGeno.py measured; the figures go into profiles/merge/merge_bench.json (profiles/merge/README.md says where each comes from).

    python tools/merge_bench.py [n_sites] [n_dip]               # on the GPU: three bgzipped files of n_sites x n_dip (5 000 000 x 70), each
                                                                # keeping 90 % of a shared list of sites
    python tools/merge_bench.py --reference [n_sites] [n_dip]   # where the reference is: the UNMODIFIED mergeGeno.py on three small files
                                                                # (20 000 x 70) over a .fai of 10^6 positions -- what it scales with

GPU mode: (1) the kernels' milliseconds from HIP events (pg_merge_dev_timing) of one run of `intersect` and one of `union` inside this
process; (2) the wall clock of fresh processes, alternating, three rounds: mergeGeno.py intersect, mergeGeno.py union, and -- the
yardstick for "the join costs about what a filter pass costs" -- the filterGenotypes.py drop-in over one file that holds the three
inputs' lines; (3) a device-to-device copy of as many bytes as each method's output holds: the floor of k_merge_emit.  The ratios
are written down, nothing is gated on them.  Each mode rewrites its own section of the JSON file."""
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from drivers_bench import REF                                                 # noqa: E402  (where the reference is)
OUT = os.path.join(ROOT, "profiles", "merge", "merge_bench.json")
CELLS = np.frombuffer(b"A/A\tA/T\tT/T\tN/N\tC/G\tG/G\tC/C\tT/A\t", dtype=np.uint8).reshape(8, 4)


def save(section, res):
    os.makedirs(os.path.dirname(OUT), exist_ok=True)
    doc = {}
    if os.path.exists(OUT):
        with open(OUT) as f:
            doc = json.load(f)
    doc[section] = res
    with open(OUT, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({section: res}))


def write_inputs(tmp, n_sites, n_dip, genome=None, n_files=3, keep=0.9, concat=False):
    """n_files plain `.geno` files under tmp, each keeping `keep` of a shared list of n_sites sites of one scaffold, and the .fai
    (genome: the scaffold's length, default the last site's position); concat: also one file that holds all their lines.  Returns
    (paths, fai, concat path or None, bytes of text)"""
    rng = np.random.default_rng(20261019)
    if genome is None:
        pos = np.cumsum(rng.integers(1, 4, size=n_sites))
        genome = int(pos[-1])
    else:
        pos = np.sort(rng.choice(np.arange(1, genome + 1), size=n_sites, replace=False))
    fai = os.path.join(tmp, "genome.fai")
    with open(fai, "w") as f:
        f.write("chr1\t%d\n" % genome)
    paths, total = [], 0
    cat = open(os.path.join(tmp, "concat.geno"), "wb") if concat else None
    for x in range(n_files):
        path = os.path.join(tmp, "in%d.geno" % x)
        header = ("#CHROM\tPOS\t" + "\t".join("f%ds%d" % (x, d) for d in range(n_dip)) + "\n").encode()
        with open(path, "wb") as f:
            f.write(header)
            if cat is not None and x == 0:
                cat.write(header)
            mine = pos[rng.random(n_sites) < keep]
            for a in range(0, len(mine), 100000):
                part = mine[a:a + 100000]
                body = CELLS[rng.integers(0, 8, size=(len(part), n_dip))].reshape(len(part), 4 * n_dip)
                body[:, -1] = 10
                text = b"".join(b"chr1\t%d\t" % p + row.tobytes() for p, row in zip(part.tolist(), body))
                f.write(text)
                if cat is not None:
                    cat.write(text)
        total += os.path.getsize(path)
        paths.append(path)
    if cat is not None:
        cat.close()
    return paths, fai, (os.path.join(tmp, "concat.geno") if concat else None), total


def bgzip(path):
    from genomics_general_amd import genoio
    with open(path, "rb") as f:
        data = f.read()
    with open(path + ".gz", "wb") as f:
        f.write(memoryview(genoio.bgzf_compress(data)))
    os.remove(path)
    return path + ".gz"


def wall(script, argv, env=None):
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, env=dict(os.environ, **(env or {})), stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s failed: %s" % (script, r.stderr.decode()[-800:]))
    return dt


def kernel_times(inputs, fai, method, out):
    """one run inside this process under PG_TIMING: the kernels' milliseconds (HIP events), the rounds, the output's bytes"""
    from genomics_general_amd import mergegeno
    os.environ.update(PG_TIMING="1", PG_MERGE_DEVICE="1")
    old = sys.stderr
    sys.stderr = open(os.devnull, "w")
    try:
        rc = mergegeno.main(sum([["-i", p] for p in inputs], []) + ["-f", fai, "--method", method, "-o", out])
    finally:
        sys.stderr.close()
        sys.stderr = old
    assert rc == 0
    info = dict(mergegeno.last_info)
    res = {k: round(float(info[k]), 3) for k in ("k_merge_keys_ms", "k_merge_lines_pos_ms", "k_merge_emit_ms", "total_s", "device_s", "read_s", "write_s")}
    res.update(rounds=info["rounds"], rounds_on_host=info["rounds_on_host"], lines_written=info["lines_written"], output_bytes=os.path.getsize(out))
    return res


def copy_floor_ms(n_bytes):
    """a device-to-device copy of n_bytes, HIP events, the median of five"""
    import torch
    a = torch.empty(n_bytes, dtype=torch.uint8, device="cuda")
    b = torch.empty_like(a)
    ms = []
    for rep in range(6):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        b.copy_(a)
        e1.record()
        torch.cuda.synchronize()
        if rep:
            ms.append(e0.elapsed_time(e1))
    return round(statistics.median(ms), 3)


def gpu_mode(n_sites, n_dip):
    tmp = tempfile.mkdtemp(prefix="pg_merge_bench_", dir=os.environ.get("PG_BENCH_TMP", "/tmp"))
    paths, fai, cat, n_text = write_inputs(tmp, n_sites, n_dip, concat=True)
    inputs = [bgzip(p) for p in paths]
    cat = bgzip(cat)
    res = {"sites": n_sites, "diploids": n_dip, "files": len(inputs), "text_bytes": n_text, "file_bytes": sum(os.path.getsize(p) for p in inputs)}
    out = os.path.join(tmp, "out.geno")
    res["kernels"] = {m: kernel_times(inputs, fai, m, out) for m in ("intersect", "union")}
    for m in ("intersect", "union"):
        k = res["kernels"][m]
        k["d2d_copy_of_output_ms"] = copy_floor_ms(k["output_bytes"])
        k["k_merge_emit_over_copy"] = round(k["k_merge_emit_ms"] / max(k["d2d_copy_of_output_ms"], 1e-9), 2)
    merge = sum([["-i", p] for p in inputs], []) + ["-f", fai, "-o", out]
    cmds = {
        "mergeGeno.py intersect": ("mergeGeno.py", merge + ["--method", "intersect"], {"PG_MERGE_DEVICE": "1"}),
        "mergeGeno.py union": ("mergeGeno.py", merge + ["--method", "union"], {"PG_MERGE_DEVICE": "1"}),
        "filterGenotypes.py (the three files' lines)": ("filterGenotypes.py", ["-i", cat, "-o", out + ".filtered", "--minCalls", "1"], {}),
    }
    runs = {k: [] for k in cmds}
    for rnd in range(3):
        for k, (script, argv, env) in cmds.items():
            runs[k].append(round(wall(script, argv, env), 3))
    res["wall_s"] = runs
    res["wall_median_s"] = {k: statistics.median(v) for k, v in runs.items()}
    filt = res["wall_median_s"]["filterGenotypes.py (the three files' lines)"]
    res["wall_over_filter"] = {k: round(v / filt, 2) for k, v in res["wall_median_s"].items()}
    for fn in os.listdir(tmp):
        os.remove(os.path.join(tmp, fn))
    os.rmdir(tmp)
    save("gpu", res)


def reference_mode(n_sites, n_dip, genome=1_000_000):
    """the unmodified mergeGeno.py on three small plain files over a .fai of `genome` positions: its time follows the positions it
    walks, not the lines it reads"""
    tmp = tempfile.mkdtemp(prefix="pg_merge_ref_")
    paths, fai, _, n_text = write_inputs(tmp, n_sites, n_dip, genome=genome)
    res = {"sites": n_sites, "diploids": n_dip, "genome_positions": genome, "text_bytes": n_text, "host_cpus": len(os.sched_getaffinity(0)), "runs": {}}
    for method in ("intersect", "union"):
        t = time.perf_counter()
        r = subprocess.run([sys.executable, "-W", "ignore", os.path.join(REF, "mergeGeno.py")] + sum([["-i", p] for p in paths], []) +
                           ["-f", fai, "--method", method, "-o", os.path.join(tmp, "o.geno")], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dt = time.perf_counter() - t
        res["runs"][method] = {"seconds": round(dt, 2), "positions_per_sec": round(genome / dt, 1), "rc": r.returncode}
    # the drop-in's host route on the same files, for scale (no device here)
    for method in ("intersect", "union"):
        dt = wall("mergeGeno.py", sum([["-i", p] for p in paths], []) + ["-f", fai, "--method", method, "-o", os.path.join(tmp, "o2.geno")],
                  {"PG_MERGE_DEVICE": "0"})
        res["runs"]["drop-in host route, " + method] = {"seconds": round(dt, 2)}
    for fn in os.listdir(tmp):
        os.remove(os.path.join(tmp, fn))
    os.rmdir(tmp)
    save("reference", res)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--reference" in sys.argv:
        reference_mode(int(args[0]) if args else 20_000, int(args[1]) if len(args) > 1 else 70)
    else:
        gpu_mode(int(args[0]) if args else 5_000_000, int(args[1]) if len(args) > 1 else 70)
