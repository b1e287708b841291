"""The filterGenotypes.py drop-in's device route (pg_filter_dev_*: k_filt_lines, k_filt_thin) on an MI355X: every golden of the
unmodified reference byte for byte from gzip, plain and BGZF input (members inflated on the device), in one block and in many small
ones (pods and thinning across blocks), `.gz` output deflated on the device, rows longer than their text, the device
against the host route on seeded random files (one of more than 1 000 sample columns), and an irregular line that hands its block to the
host.  Each run is a process of its own under a time limit; PG_TIMING's counters show that the blocks were filtered on the device."""
import gzip
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from filter_cases import CASES, fixture_path, random_case  # noqa: E402

pytestmark = pytest.mark.gpu


def _run(inp, argv, out, device=True, block=None, timeout=180):
    env = dict(os.environ, PG_TIMING="1", PG_FILTER_DEVICE="1" if device else "0")
    if block:
        env["PG_STREAM_BYTES"] = str(block)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "filterGenotypes.py"), "-i", inp, "-o", out] + [a.replace("@G", GOLD) for a in argv],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    info = {}
    m = re.search(r"PG_TIMING filter (.*)", r.stderr.decode())
    if m:
        for kv in m.group(1).split():
            k, v = kv.split("=", 1)
            info[k] = v
    with (gzip.open(out, "rb") if out.endswith(".gz") else open(out, "rb")) as f:
        return f.read(), info


def _golden(name):
    with gzip.open(os.path.join(GOLD, "filter", name + ".out.gz"), "rb") as f:
        return f.read()


DET = [c for c in CASES if "randomAllele" not in c[2]]


def _source(fixture, source, tmp_path):
    """the fixture as it is (gzip), as plain text, or as bgzip's BGZF members (inflated on the device)"""
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


@pytest.mark.parametrize("name,fixture,argv", DET, ids=[c[0] for c in DET])
@pytest.mark.parametrize("source,block", [("gz", None), ("plain", None), ("plain", 20000), ("bgzf", None), ("bgzf", 30000)])
def test_device_route_reproduces_the_reference(name, fixture, argv, source, block, tmp_path):
    got, info = _run(_source(fixture, source, tmp_path), argv, str(tmp_path / "o.geno"), block=block)
    assert got == _golden(name)
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0, info
    if source == "bgzf" and "--thinDist" not in argv and fixture != "edge":    # (edge is one member: the header line's read inflates it)
        assert int(info["blocks_inflated_on_device"]) >= 1, info


@pytest.mark.parametrize("source", ["plain", "bgzf"])
def test_device_route_gz_output_deflated_on_the_device(source, tmp_path):
    name, fixture, argv = DET[0]
    got, info = _run(_source(fixture, source, tmp_path), argv, str(tmp_path / "o.geno.gz"), block=50000)
    assert got == _golden(name)
    with open(str(tmp_path / "o.geno.gz"), "rb") as f:
        assert f.read().endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))
    assert int(info["device_blocks"]) >= 2 and int(info["device_host_blocks"]) == 0, info


@pytest.mark.parametrize("argv", [["--ploidy", "2", "--forcePloidy", "-of", "alleles"], ["-of", "alleles"]])
def test_rows_longer_than_their_text_stay_on_the_device(argv, tmp_path):
    """haploid cells written as str(tuple) or padded to two alleles: rows several times their text grow the buffer, no host fallback"""
    names = ["h%d" % k for k in range(40)]
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    for i in range(3000):
        rows.append("\t".join(["c", str(i + 1)] + ["ACGT"[(i * 7 + k) % 4] if (i + k) % 3 else "A" for k in range(40)]))
    inp = str(tmp_path / "hap.geno")
    with open(inp, "w") as f:
        f.write("\n".join(rows) + "\n")
    want, _ = _run(inp, argv + ["--minCalls", "0"], str(tmp_path / "h.geno"), device=False)
    got, info = _run(inp, argv + ["--minCalls", "0"], str(tmp_path / "d.geno"))
    assert got == want and len(want) > 4 * os.path.getsize(inp) // 2
    assert int(info["device_host_blocks"]) == 0, info


def _random_pair(tmp_path, seed, **kw):
    text, argv = random_case(seed, **kw)
    inp = str(tmp_path / ("r%d.geno" % seed))
    with open(inp, "w") as f:
        f.write(text)
    return inp, argv, text


@pytest.mark.parametrize("seed", range(40))
def test_device_equals_host_on_random_files(seed, tmp_path):
    inp, argv, _ = _random_pair(tmp_path, seed)
    want, _ = _run(inp, argv, str(tmp_path / "h.geno"), device=False)
    got, info = _run(inp, argv, str(tmp_path / "d.geno"), block=3000)
    assert got == want
    assert int(info["device_host_blocks"]) == 0, info


def test_device_equals_host_on_a_wide_file(tmp_path):
    inp, argv, _ = _random_pair(tmp_path, 7001, n_samples=1200, n_lines=300)
    want, _ = _run(inp, argv, str(tmp_path / "h.geno"), device=False)
    got, info = _run(inp, argv, str(tmp_path / "d.geno"))
    assert got == want and len(want.split(b"\n")) > 2
    assert int(info["device_host_blocks"]) == 0, info


def test_irregular_line_hands_its_block_to_the_host(tmp_path):
    inp, argv, text = _random_pair(tmp_path, 7002, n_samples=6, n_lines=400)
    rows = text.split("\n")
    rows[200] = rows[200].replace("\t", "  ", 1)           # two spaces: line.split() takes it, the device does not
    with open(inp, "w") as f:
        f.write("\n".join(rows))
    want, _ = _run(inp, argv, str(tmp_path / "h.geno"), device=False)
    got, info = _run(inp, argv, str(tmp_path / "d.geno"), block=4000)
    assert got == want
    assert int(info["device_host_blocks"]) >= 1 and int(info["device_blocks"]) > int(info["device_host_blocks"]), info


@pytest.mark.parametrize("final_newline", [False, True])
def test_bgzf_input_whose_last_line_has_no_line_feed(final_newline, tmp_path):
    """four data lines in two BGZF members (the header and two lines, then two lines), the last line without its line feed: through the
    device route with the members inflated on the device, the rows are the host route's byte for byte and the unfinished line's block is
    the host's; with the line feed restored no block is.  (Whether a block of members ends in a line feed is read on the device once its
    line feeds are counted: pg_line_slot.h's tail_unknown)"""
    from genomics_general_amd import genoio
    head = "#CHROM\tPOS\ta\tb\tc\n"
    lines = ["c1\t%d\t%s\n" % (i + 1, cells) for i, cells in enumerate(("A/A\tA/T\tT/T", "A/A\tA/A\tA/A", "C/C\tC/G\tN/N", "G/T\tT/T\tG/G"))]
    text = (head + "".join(lines)).encode()
    if not final_newline:
        text = text[:-1]
    inp = str(tmp_path / "in.geno.gz")
    bz = genoio.bgzf_compress(text, block=len(head + lines[0] + lines[1]))
    assert len(genoio.bgzf_walk(bz)[0][0]) == 3                   # (two members of text, bgzip's empty last)
    with open(inp, "wb") as f:
        f.write(bz)
    argv = ["--minAlleles", "2"]
    want, _ = _run(inp, argv, str(tmp_path / "h.geno"), device=False)
    got, info = _run(inp, argv, str(tmp_path / "d.geno"))
    assert got == want and got.count(b"\n") == 4                  # (the header and lines 1, 3, 4: the host route ends the last line itself)
    assert int(info["blocks_inflated_on_device"]) >= 1 and int(info["device_blocks"]) >= 1, info
    if final_newline:
        assert int(info["device_host_blocks"]) == 0, info
    else:
        assert int(info["device_host_blocks"]) >= 1, info
