"""Measurements of the seqToGeno.py drop-in (profiles/s2g/README.md says where each number comes from).

    python tools/s2g_bench.py --reference [--head 20000]       the UNMODIFIED reference's sites/s on a head of the alignment (CPU)
    python tools/s2g_bench.py [--sites 300000] [--rounds 3]    on an MI355X: process wall clock, fresh processes, alternating
    python tools/s2g_bench.py --kernels [--sites 300000]       on an MI355X: a rocprofv3 --kernel-trace --stats run of its own per command

The input is the fasta that the genoToSeq.py drop-in writes with --splitPhased from gvcf_bench.make_text's file: --sites sites x
--samples diploids, so 2 x --samples sequences, joined again by -P 2.  The runs on it are the device route, the drop-in's own host
route (PG_S2G_DEVICE=0, 16 host threads) and the yardstick, the genoToSeq.py drop-in producing that fasta from the bgzipped `.geno`:
the same bytes, the other way.  Every figure is a median of --rounds runs with its range; PG_TIMING's line of the last round splits
loading and emitting.  --kernels leaves the kernels' total milliseconds as the profiler's own table has them.  Results are merged
into --out (profiles/s2g/s2g_bench.json)."""
import argparse
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import plink_bench  # noqa: E402
from gvcf_bench import make_text  # noqa: E402
from plink_bench import merge_json, summary, timed  # noqa: E402

plink_bench.KERNELS = ("k_s2g_lines", "k_s2g_gather", "k_s2g_heads", "k_s2g_tile", "k_seq_lines", "k_seq_rows", "k_seq_tile", "k_rows_scan",
                       "k_inflate", "k_deflate")


def s2g_cmd(script, fa, out):
    return [sys.executable, script, "-s", fa, "-g", out, "-P"] + ["2"]


def seq_cmd(geno, fa):
    return [sys.executable, os.path.join(ROOT, "genoToSeq.py"), "-g", geno, "-s", fa, "--splitPhased"]


def same(a, b):
    with open(a, "rb") as f, open(b, "rb") as g:
        return f.read() == g.read()


def make_inputs(tmp, sites, samples, device):
    """(the bgzipped .geno, the fasta genoToSeq.py --splitPhased writes from it)"""
    from genomics_general_amd import genoio
    text = make_text(sites, samples)
    geno = os.path.join(tmp, "in.geno.gz")
    with open(geno, "wb") as f:
        f.write(genoio.bgzf_compress(text))
    fa = os.path.join(tmp, "in.fa")
    timed(seq_cmd(geno, fa), dict(os.environ, PG_SEQ_DEVICE="1" if device else "0"))
    return geno, fa, len(text)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sites", type=int, default=300000)
    ap.add_argument("--samples", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reference", action="store_true")
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--head", type=int, default=20000)
    ap.add_argument("--ref", default=os.environ.get("GG_REFERENCE", "/root/reference"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "s2g", "s2g_bench.json"))
    a = ap.parse_args()
    script = os.path.join(ROOT, "seqToGeno.py")
    with tempfile.TemporaryDirectory() as tmp:
        if a.reference:
            _, fa, _ = make_inputs(tmp, a.head, a.samples, False)
            # (the reference's -P 2 dies under Python 3: the list is spelled out for it)
            ref_cmd = [sys.executable, os.path.join(a.ref, "seqToGeno.py"), "-s", fa, "-g", os.path.join(tmp, "r.geno"), "-P"] + ["2"] * a.samples
            t_ref, _ = timed(ref_cmd, dict(os.environ, PYTHONPATH=a.ref))
            t_host, _ = timed(s2g_cmd(script, fa, os.path.join(tmp, "h.geno")), dict(os.environ, PG_S2G_DEVICE="0"))
            merge_json(a.out, "reference", {"sites": a.head, "sequences": 2 * a.samples, "fasta_bytes": os.path.getsize(fa), "cpus": os.cpu_count(),
                                            "reference_s": round(t_ref, 2), "reference_sites_per_s": round(a.head / t_ref, 1),
                                            "host_route_s": round(t_host, 3), "host_route_sites_per_s": round(a.head / t_host, 1),
                                            "outputs_identical": same(os.path.join(tmp, "r.geno"), os.path.join(tmp, "h.geno"))})
            return 0
        geno, fa, geno_bytes = make_inputs(tmp, a.sites, a.samples, True)
        runs = {
            "s2g_device": (s2g_cmd(script, fa, os.path.join(tmp, "d.geno")), {"PG_S2G_DEVICE": "1"}),
            "s2g_host_route": (s2g_cmd(script, fa, os.path.join(tmp, "h.geno")), {"PG_S2G_DEVICE": "0", "PG_HOST_THREADS": "16"}),
            "seq_device_split_phased_cat": (seq_cmd(geno, os.path.join(tmp, "y.fa")), {"PG_SEQ_DEVICE": "1"}),
        }
        if a.kernels:
            res = {k: plink_bench.kernel_ms(cmd, dict(os.environ, **extra), tmp, k) for k, (cmd, extra) in runs.items() if k != "s2g_host_route"}
            merge_json(a.out, "kernel_trace_%d" % a.sites, {"sites": a.sites, "sequences": 2 * a.samples, "calls_and_total_ms": res})
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
        merge_json(a.out, "gpu_%d" % a.sites, {"sites": a.sites, "sequences": 2 * a.samples, "fasta_bytes": os.path.getsize(fa),
                                               "geno_text_bytes": geno_bytes, "out_bytes": os.path.getsize(os.path.join(tmp, "d.geno")),
                                               "wall": res, "pg_timing": timing,
                                               "device_equals_host_route": same(os.path.join(tmp, "d.geno"), os.path.join(tmp, "h.geno")),
                                               "host_route_over_device": round(med["s2g_host_route"] / med["s2g_device"], 2),
                                               "device_over_seq_device": round(med["s2g_device"] / med["seq_device_split_phased_cat"], 2)})
    return 0


if __name__ == "__main__":
    sys.exit(main())
