"""The genoToVCF.py drop-in's device route (pg_gvcf_dev_*: k_gvcf_lines) on an MI355X: every golden of the unmodified reference byte
for byte from gzip, plain and BGZF input (members inflated on the device), in one block and in many small ones; column counts at the
edges of the lanes' stride; a selection of 3 of 1 100 columns; pairs and diplo rows longer than their text; `.gz` output deflated on
the device; -r with a scaffold change inside a block and sites at the first and last base of a sequence; a double-tab line that hands
its block to the host.  Each run is a process of its own under a time limit; PG_TIMING's counters show where the blocks went."""
import gzip
import os
import random
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from gvcf_cases import CASES, fixture_path  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = ("edge", "extra", "dup")          # one BGZF member: the header line's read inflates it on the host
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def _run(inp, argv, out, device=True, block=None, timeout=120):
    env = dict(os.environ, PG_TIMING="1", PG_GVCF_DEVICE="1" if device else "0")
    if block:
        env["PG_STREAM_BYTES"] = str(block)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "VCF_processing", "genoToVCF.py"), "-g", inp, "-o", out] + [a.replace("@G", GOLD) for a in argv],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    info = {}
    m = re.search(r"PG_TIMING gvcf (.*)", r.stderr.decode())
    if m:
        for kv in m.group(1).split():
            k, v = kv.split("=", 1)
            info[k] = v
    with (gzip.open(out, "rb") if out.endswith(".gz") else open(out, "rb")) as f:
        return f.read(), info


def _golden(name):
    with gzip.open(os.path.join(GOLD, "gvcf", name + ".out.gz"), "rb") as f:
        return f.read()


def _source(fixture, source, tmp_path):
    """the fixture as it is, as plain text, or as bgzip's BGZF members (inflated on the device)"""
    from genomics_general_amd import genoio
    inp = fixture_path(fixture)
    if source == "gz":
        return inp
    with (gzip.open(inp, "rb") if inp.endswith(".gz") else open(inp, "rb")) as f:
        text = f.read()
    p = str(tmp_path / ("in.geno" + (".gz" if source == "bgzf" else "")))
    with open(p, "wb") as g:
        g.write(genoio.bgzf_compress(text, block=7000) if source == "bgzf" else text)
    return p


@pytest.mark.parametrize("name,fixture,argv", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("source,block", [("gz", None), ("plain", None), ("plain", 20000), ("bgzf", None), ("bgzf", 30000)])
def test_device_route_reproduces_the_reference(name, fixture, argv, source, block, tmp_path):
    got, info = _run(_source(fixture, source, tmp_path), argv, str(tmp_path / "o.vcf"), block=block)
    assert got == _golden(name)
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0, info
    if source == "bgzf" and fixture not in SMALL:
        assert int(info["blocks_inflated_on_device"]) >= 1, info


def _wide(path, n_cols, n_lines, seed, fmt="phased"):
    """n_lines sites of n_cols samples: counts that tie, three and four alleles, missing and half-missing cells, two scaffolds"""
    R = random.Random(seed)
    names = ["w%d" % k for k in range(n_cols)]
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    for i in range(n_lines):
        site = R.sample("ACGT", R.choice([1, 2, 2, 3, 4]))
        miss = R.choice([0.0, 0.1, 0.6, 1.0]) if i % 7 else 1.0
        cells = []
        for k in range(n_cols):
            a, b = ("N" if R.random() < miss else R.choice(site) for _ in range(2))
            if fmt == "phased":
                cells.append(a + R.choice("/|") + b)
            elif fmt == "pairs":
                cells.append(a + b)
            else:
                cells.append({"AA": "A", "CC": "C", "GG": "G", "TT": "T", "GT": "K", "AC": "M", "NN": "N", "CG": "S", "AG": "R", "AT": "W",
                              "CT": "Y"}.get("".join(sorted(a + b)), "N"))
        rows.append("\t".join(["u%d" % (i * 2 // n_lines), str(i + 1)] + cells))
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return names


@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 129, 1100])
def test_column_counts_at_the_edges_of_the_lane_stride(n_cols, tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, n_cols, 300, n_cols)
    want, _ = _run(inp, ["-f", "phased"], str(tmp_path / "h.vcf"), device=False)
    got, info = _run(inp, ["-f", "phased"], str(tmp_path / "d.vcf"))
    assert got == want and got.count(b"\n") == 303
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0, info


def test_three_of_1100_columns_in_reverse_order(tmp_path):
    inp = str(tmp_path / "w.geno")
    names = _wide(inp, 1100, 300, 5)
    argv = ["-f", "phased", "-s", ",".join([names[1099], names[64], names[0]])]
    want, _ = _run(inp, argv, str(tmp_path / "h.vcf"), device=False)
    got, info = _run(inp, argv, str(tmp_path / "d.vcf"))
    assert got == want and got.split(b"\n")[2].endswith(b"\tw1099\tw64\tw0")
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0, info


@pytest.mark.parametrize("fmt", ["pairs", "diplo"])
def test_rows_longer_than_their_text_stay_on_the_device(fmt, tmp_path):
    """cells of one or two bytes become three: the rows outgrow the buffer sized from the text, it grows, no host block"""
    inp = str(tmp_path / "w.geno")
    _wide(inp, 40, 3000, 11, fmt)
    want, _ = _run(inp, ["-f", fmt], str(tmp_path / "h.vcf"), device=False)
    got, info = _run(inp, ["-f", fmt], str(tmp_path / "d.vcf"))
    assert got == want and len(want) > os.path.getsize(inp) + 3000 * 32 + 4096
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0, info


@pytest.mark.parametrize("source", ["plain", "bgzf"])
def test_gz_output_deflated_on_the_device(source, tmp_path):
    name, fixture, argv = CASES[2]
    got, info = _run(_source(fixture, source, tmp_path), argv, str(tmp_path / "o.vcf.gz"), block=50000)
    assert got == _golden(name)
    with open(str(tmp_path / "o.vcf.gz"), "rb") as f:
        assert f.read().endswith(EOF_MEMBER)
    assert int(info["device_blocks"]) >= 2 and int(info["device_host_blocks"]) == 0, info


def test_reference_with_a_scaffold_change_inside_a_block(tmp_path):
    """two scaffolds in one block, sites at the first and at the last base of each sequence, lower-case and n bases"""
    R = random.Random(3)
    seqs = {"u0": "".join(R.choice("ACGTacgtNn") for _ in range(150)), "u1": "".join(R.choice("ACGTacgtNn") for _ in range(300))}
    fa = str(tmp_path / "r.fa")
    with open(fa, "w") as f:
        f.write("".join(">%s\n%s\n" % kv for kv in seqs.items()))
    inp = str(tmp_path / "w.geno")
    _wide(inp, 7, 300, 9)
    with open(inp) as f:
        lines = f.read().split("\n")
    assert lines[1].startswith("u0\t1\t") and lines[150].startswith("u0\t150\t") and lines[151].startswith("u1\t151\t") and lines[300].startswith("u1\t300\t")
    for k in range(151, 301):                               # u1's sites counted from its own first base
        f = lines[k].split("\t")
        f[1] = str((k - 150) * 2)
        lines[k] = "\t".join(f)
    lines[151] = "\t".join(["u1", "1"] + lines[151].split("\t")[2:])
    with open(inp, "w") as f:
        f.write("\n".join(lines))
    argv = ["-f", "phased", "-r", fa]
    want, _ = _run(inp, argv, str(tmp_path / "h.vcf"), device=False)
    got, info = _run(inp, argv, str(tmp_path / "d.vcf"))
    assert got == want
    rows = got.split(b"\n")[4:]                             # (behind ##fileformat, ##reference, ##FORMAT and #CHROM)
    assert rows[0].split(b"\t")[3] == seqs["u0"][0].encode() and rows[149].split(b"\t")[3] == seqs["u0"][149].encode()
    assert rows[150].split(b"\t")[3] == seqs["u1"][0].encode() and rows[299].split(b"\t")[:4] == [b"u1", b"300", b".", seqs["u1"][299].encode()]
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0, info


def test_a_double_tab_line_hands_its_block_to_the_host(tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, 5, 300, 21)
    with open(inp) as f:
        lines = f.read().split("\n")
    lines[200] = lines[200].replace("\t", "\t\t", 1)
    with open(inp, "w") as f:
        f.write("\n".join(lines))
    want, _ = _run(inp, ["-f", "phased"], str(tmp_path / "h.vcf"), device=False)
    got, info = _run(inp, ["-f", "phased"], str(tmp_path / "d.vcf"), block=4000)
    assert got == want and got.count(b"\n") == 303
    assert int(info["device_blocks"]) >= 2 and int(info["device_host_blocks"]) == 1, info
