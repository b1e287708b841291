#!/usr/bin/env python
"""genoToSeq.py measured on the file shape tools/drivers_bench.py uses (5 000 000 sites x 200 diploids, bgzipped); the figures go into
profiles/seq/seq_bench.json (profiles/seq/README.md says where each comes from):

    python tools/seq_bench.py [n_sites] [n_dip]                 # on a GPU box
    python tools/seq_bench.py --reference [n_sites] [n_dip]     # where the reference is: the UNMODIFIED genoToSeq.py on a head of
                                                                # 100 000 sites, on the CPU

GPU mode: (1) k_seq_lines and k_seq_tile over one block of the text (PG_STREAM_BYTES of it, 256 MiB by default), timed by HIP events
(pg_seq_dev_timing), a warm-up and five repeats, with the bytes they read and write per second; next to them the device tokenizer over
the same block -- the wall time of its kernels and results behind the copies (pg_tokenize_stats), which bounds its parse kernel from
above: both read every byte of the text once.  (2) the wall clock of fresh processes, alternating, three rounds: genoToSeq.py
--splitPhased -M windows, genoToSeq.py --splitPhased (cat), freq.py.  Each mode rewrites its own half of the JSON file."""
import json
import os

os.environ.setdefault("PG_BGZF_ZLIB", "1")          # (the sample is what htslib's bgzip writes: see tools/drivers_bench.py)
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from drivers_bench import REF, driver_commands                                # noqa: E402  (where the reference is)
OUT = os.path.join(ROOT, "profiles", "seq", "seq_bench.json")


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


def kernel_times(geno, n_dip):
    """one block of the plain text through the device route and through the device tokenizer"""
    from genomics_general_amd import genoseq
    from genomics_general_amd.engine import Engine
    from genomics_general_amd.samples import HapLayout, SampleData
    block_bytes = int(os.environ.get("PG_STREAM_BYTES", str(256 << 20)))
    with open(geno, "rb") as f:
        header = f.readline()
        block = f.read(block_bytes)
        block = block[:block.rfind(b"\n") + 1]
    n_lines = block.count(b"\n")

    class A:
        splitPhased, ploidy, NtoGap = True, [2], False
    plan = genoseq.Plan(header.decode(), A, None)
    dev = genoseq.Device(plan, 0)
    assert dev.taken
    genoseq._lib.check(dev.L.pg_seq_dev_timing(dev.eng._h, 1))
    lines_ms, tile_ms = [], []
    for rep in range(6):
        b0 = dev.stats()
        chunk = dev.collect(dev.submit(block))[0]
        assert chunk is not None and chunk.n == n_lines
        b1 = dev.stats()
        if rep:
            lines_ms.append(b1[2] - b0[2])
            tile_ms.append(b1[3] - b0[3])
    n_seq = plan.cfg.n_seq
    dev.close()
    names = header.decode().split()[2:]
    e = Engine(0)
    e.set_layout(HapLayout(SampleData(indNames=list(names)), names, "phased"))
    e.reserve(n_lines + 1024)
    tok = []
    for rep in range(6):
        s0 = e.tokenize_stats()
        got = e.tokenize_text(block, 0, n_lines + 1, at_most=True)
        s1 = e.tokenize_stats()
        assert got is not None and got[0] == n_lines
        if rep:
            tok.append((s1["kernels_s"] - s0["kernels_s"]) * 1e3)
    e.close()
    lm, tm, km = statistics.median(lines_ms), statistics.median(tile_ms), statistics.median(tok)
    return {"block_text_bytes": len(block), "block_sites": n_lines, "sequences": n_seq, "matrix_bytes": n_seq * n_lines,
            "k_seq_lines_ms": [round(x, 3) for x in lines_ms], "k_seq_tile_ms": [round(x, 3) for x in tile_ms],
            "tokenizer_kernels_ms": [round(x, 3) for x in tok],
            "k_seq_lines_read_GBps": round(len(block) / lm / 1e6, 1),
            "k_seq_tile_read_GBps": round(len(block) / tm / 1e6, 1), "k_seq_tile_write_GBps": round(n_seq * n_lines / tm / 1e6, 1),
            "tokenizer_kernels_read_GBps": round(len(block) / km / 1e6, 1)}


def wall(script, argv):
    t = time.perf_counter()
    r = subprocess.run([sys.executable, os.path.join(ROOT, script)] + argv, env=dict(os.environ, PG_TIMING="1"), stdout=subprocess.DEVNULL,
                       stderr=subprocess.PIPE)
    dt = time.perf_counter() - t
    if r.returncode != 0:
        raise SystemExit("%s failed: %s" % (script, r.stderr.decode()[-800:]))
    return dt


def gpu_mode(n_sites, n_dip):
    import bgzip
    tmp = tempfile.mkdtemp(prefix="pg_seq_bench_", dir=os.environ.get("PG_BENCH_TMP", "/tmp"))
    geno = os.path.join(tmp, "sample.geno")
    subprocess.run([sys.executable, os.path.join(ROOT, "tools", "t2_write_sample.py"), geno, str(n_sites), str(n_dip)], stdout=subprocess.PIPE, check=True)
    res = {"sites": n_sites, "diploids": n_dip, "kernels": kernel_times(geno, n_dip)}
    n_in, n_gz = bgzip.bgzip_file(geno, geno + ".gz")
    os.remove(geno)
    res["text_bytes"], res["file_bytes"] = n_in, n_gz
    names = ["s%d" % d for d in range(n_dip)]
    out = os.path.join(tmp, "out")
    cmds = {
        "genoToSeq.py --splitPhased -M windows": ("genoToSeq.py", ["-g", geno + ".gz", "-s", out + ".win.fa", "--splitPhased", "-M", "windows",
                                                                   "--windType", "coordinate", "--windSize", "50000", "--stepSize", "50000"]),
        "genoToSeq.py --splitPhased (cat)": ("genoToSeq.py", ["-g", geno + ".gz", "-s", out + ".cat.fa", "--splitPhased"]),
        "freq.py": ("freq.py", driver_commands(geno + ".gz", out, names, 4, 50000)["freq.py"]),
    }
    runs = {k: [] for k in cmds}
    for rnd in range(3):
        for k, (script, argv) in cmds.items():
            dt = wall(script, argv)
            runs[k].append(round(dt, 3))
    res["wall_s"] = runs
    res["wall_median_s"] = {k: statistics.median(v) for k, v in runs.items()}
    res["sites_per_sec"] = {k: round(n_sites / statistics.median(v), 1) for k, v in runs.items()}
    for fn in os.listdir(tmp):
        os.remove(os.path.join(tmp, fn))
    os.rmdir(tmp)
    save("gpu", res)


def reference_mode(n_sites, n_dip):
    """the unmodified genoToSeq.py on a host-generated head of the file shape (np.NaN restored as tests/golden/make_golden.py does)"""
    tmp = tempfile.mkdtemp(prefix="pg_seq_ref_")
    rng = np.random.default_rng(1)
    geno = os.path.join(tmp, "ref.geno")
    letters = np.array(list(b"ACGT"), dtype=np.uint8)[rng.integers(0, 4, size=(n_sites, 1)) ^ (rng.random((n_sites, 2 * n_dip)) < 0.1)]
    letters[rng.random((n_sites, 2 * n_dip)) < 0.02] = ord("N")
    with open(geno, "wb") as f:
        f.write(("#CHROM\tPOS\t" + "\t".join("s%d" % d for d in range(n_dip)) + "\n").encode())
        for i in range(n_sites):
            row = letters[i]
            f.write(b"chr1\t%d\t" % (i + 1) + b"\t".join(bytes([row[2 * d]]) + b"/" + bytes([row[2 * d + 1]]) for d in range(n_dip)) + b"\n")
    shim = ("import sys, runpy, numpy as np; np.NaN = np.nan; sys.path.insert(0, %r); sys.argv = sys.argv[1:]; "
            "runpy.run_path(sys.argv[0], run_name='__main__')" % REF)
    res = {"sites": n_sites, "diploids": n_dip, "host_cpus": len(os.sched_getaffinity(0)), "runs": {}}
    for tag, extra in (("genoToSeq.py --splitPhased -M windows", ["-M", "windows", "--windType", "coordinate", "--windSize", "50000", "--stepSize", "50000"]),
                       ("genoToSeq.py --splitPhased (cat)", [])):
        t = time.perf_counter()
        r = subprocess.run([sys.executable, "-W", "ignore", "-c", shim, os.path.join(REF, "genoToSeq.py"), "-g", geno, "-s", os.path.join(tmp, "o.fa"),
                            "--splitPhased"] + extra, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        dt = time.perf_counter() - t
        res["runs"][tag] = {"seconds": round(dt, 2), "sites_per_sec": round(n_sites / dt, 1), "rc": r.returncode}
    for fn in os.listdir(tmp):
        os.remove(os.path.join(tmp, fn))
    os.rmdir(tmp)
    save("reference", res)


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    if "--reference" in sys.argv:
        reference_mode(int(args[0]) if args else 100_000, int(args[1]) if len(args) > 1 else 200)
    else:
        gpu_mode(int(args[0]) if args else 5_000_000, int(args[1]) if len(args) > 1 else 200)
