"""What the seqToGeno.py tests share: a run of the drop-in as a process of its own, inputs written plain, gzipped or as BGZF, and
seeded fasta files."""
import gzip
import os
import random
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
if GOLD not in sys.path:
    sys.path.insert(0, GOLD)


def write_input(data, source, tmp_path, tag="in"):
    """data as a plain file, a gzip file or bgzip's BGZF members; None for stdin"""
    if source == "stdin":
        return None
    p = str(tmp_path / (tag + ".txt" + ("" if source == "plain" else ".gz")))
    if source == "bgzf":
        from genomics_general_amd import genoio
        data = bytes(genoio.bgzf_compress(data, block=7000))
    elif source == "gz":
        data = gzip.compress(data, mtime=0)
    with open(p, "wb") as f:
        f.write(data)
    return p


def run(data, argv, tmp_path, source="plain", device=False, block=None, tile=None, out="file", tag="o", timeout=120, env=None):
    """(exit status, output bytes -- None when no file was written --, PG_TIMING's counters, stderr) of seqToGeno.py on the input
    bytes `data`.  out: "file", "gz" (-g x.geno.gz, gunzipped here) or "stdout" """
    e = dict(os.environ, PG_TIMING="1", PG_S2G_DEVICE="1" if device else "0")
    e.update(env or {})
    if block:
        e["PG_STREAM_BYTES"] = str(block)
    if tile:
        e["PG_S2G_TILE_SEQS"] = str(tile)
    inp = write_input(data, source, tmp_path, tag + "_in")
    path = str(tmp_path / (tag + ".geno" + (".gz" if out == "gz" else "")))
    cmd = [sys.executable, os.path.join(ROOT, "seqToGeno.py")] + list(argv) + ([] if inp is None else ["-s", inp]) + ([] if out == "stdout" else ["-g", path])
    r = subprocess.run(cmd, input=data if inp is None else None, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=e, timeout=timeout, cwd=ROOT)
    err = r.stderr.decode(errors="replace")
    info = {}
    m = re.search(r"PG_TIMING s2g (.*)", err)
    if m:
        info = dict(kv.split("=", 1) for kv in m.group(1).split())
    if out == "stdout":
        got = r.stdout
    elif not os.path.exists(path):
        got = None
    elif out == "gz":
        with gzip.open(path, "rb") as f:
            got = f.read()
    else:
        with open(path, "rb") as f:
            got = f.read()
    return r.returncode, got, info, err


def fasta(seed, n_seq, n_sites, width=60, alphabet="ACGTN", name="q%d", lengths=None):
    """a regular fasta file: n_seq sequences of n_sites residues (or of lengths[k]) wrapped at width (0: unwrapped)"""
    R = random.Random(seed)
    out = []
    for k in range(n_seq):
        s = "".join(R.choice(alphabet) for _ in range(lengths[k] if lengths else n_sites))
        out.append(">" + name % k)
        out += [s[i:i + width] for i in range(0, len(s), width)] if width else [s]
    return ("\n".join(out) + "\n").encode("ascii")


def expected(data, argv_groups=None, chrom="contig0"):
    """the lines of `samples` mode from a regular fasta text, made here independently of both routes: groups of consecutive
    sequences joined by '|' (argv_groups: their sizes; None: singles)"""
    recs = [r.split("\n", 1) for r in data.decode("ascii").split(">")[1:]]
    names = [r[0].split()[0] for r in recs]
    seqs = [r[1].replace("\n", "").replace(" ", "") for r in recs]
    sizes = argv_groups or [1] * len(seqs)
    groups, at = [], 0
    for p in sizes:
        groups.append(list(range(at, at + p)))
        at += p
    head = "#CHROM\tPOS\t" + "\t".join("_".join(names[k] for k in g) for g in groups) + "\n"
    n = min(len(s) for s in seqs)
    rows = [chrom + "\t" + str(x + 1) + "\t" + "\t".join("|".join(seqs[k][x] for k in g) for g in groups) + "\n" for x in range(len(seqs[0]) if len(seqs[0]) <= n else n)]
    return (head + "".join(rows)).encode("ascii")
