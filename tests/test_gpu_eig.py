"""The genoToEigenstrat.py drop-in's device route (pg_eig_dev_*: k_eig_lines, k_rows_scan) on an MI355X: every golden of the unmodified
reference the device takes, the three files byte for byte from gzip, plain and BGZF input (members inflated on the device), in one
block and in many small ones; then device against host route on seeded files of 300 lines: column counts at the edges of the lanes'
stride; line counts at the edges of the scan's 1 024 threads; three of 1 100 columns selected where only the others make the sites biallelic; .snp rows longer than their text; site indices
over many blocks; a scaffold change and an unlisted scaffold inside a block; a cell of ten alleles, a double tab and a '#' line that
each hand their block to the host; --cumulativePos and a repeated header name, the host's for the whole run.  Each run is a process
of its own under a time limit; PG_TIMING's counters show where the blocks went."""
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
from eig_cases import CASES, DEVICE, HOST_BLOCKS, HOST_WHOLE, OUTPUTS, fixture_path, golden  # noqa: E402

pytestmark = pytest.mark.gpu

SMALL = ("edge", "diplo", "cumul_a")      # one BGZF member: the header line's read inflates it on the host
BY_NAME = {c[0]: c for c in CASES}


def _run(inp, argv, tmp_path, tag, device=True, block=None, timeout=120):
    """the three files, PG_TIMING's counters and stderr"""
    env = dict(os.environ, PG_TIMING="1", PG_EIG_DEVICE="1" if device else "0")
    if block:
        env["PG_STREAM_BYTES"] = str(block)
    outs = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in OUTPUTS}
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "genoToEigenstrat.py"), "-g", inp, "--genoOutFile", outs["geno"], "--snpOutFile",
                        outs["snp"], "--indOutFile", outs["ind"]] + [a.replace("@G", GOLD) for a in argv],
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    info = {}
    m = re.search(r"PG_TIMING eig (.*)", r.stderr.decode())
    if m:
        for kv in m.group(1).split():
            k, v = kv.split("=", 1)
            info[k] = v
    got = {}
    for k, p in outs.items():
        with open(p, "rb") as f:
            got[k] = f.read()
    return got, info, r.stderr.decode()


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


@pytest.mark.parametrize("name", DEVICE)
@pytest.mark.parametrize("source,block", [("gz", None), ("plain", None), ("plain", 20000), ("bgzf", None), ("bgzf", 30000)])
def test_device_route_reproduces_the_reference(name, source, block, tmp_path):
    _, fixture, argv = BY_NAME[name]
    got, info, _ = _run(_source(fixture, source, tmp_path), argv, tmp_path, "d", block=block)
    assert got == golden(name)
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0 and int(info["blocks_redone_on_host"]) == 0, info
    if source == "bgzf" and fixture not in SMALL:
        assert int(info["blocks_inflated_on_device"]) >= 1, info


@pytest.mark.parametrize("name", sorted(HOST_BLOCKS | HOST_WHOLE))
def test_goldens_the_device_hands_back_come_out_the_same(name, tmp_path):
    _, fixture, argv = BY_NAME[name]
    got, info, err = _run(_source(fixture, "plain", tmp_path), argv, tmp_path, "d")
    assert got == golden(name)
    if name in HOST_WHOLE:
        assert "host threads do the job" in err and "device_blocks" not in info


def _wide(path, n_cols, n_lines, seed, fmt="phased", scaf=None):
    """n_lines sites of n_cols samples: counts that tie, one to four alleles, missing and half-missing cells, two scaffolds"""
    R = random.Random(seed)
    names = ["w%d" % k for k in range(n_cols)]
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    for i in range(n_lines):
        site = R.sample("ACGT", R.choice([1, 2, 2, 2, 3, 4]))
        miss = R.choice([0.0, 0.1, 0.6, 1.0]) if i % 7 else 1.0
        cells = []
        for k in range(n_cols):
            a, b = ("N" if R.random() < miss else R.choice(site) for _ in range(2))
            cells.append(a + R.choice("/|") + b)
        rows.append("\t".join([scaf(i) if scaf else "u%d" % (i * 2 // n_lines), str(i + 1)] + cells))
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return names


def _both(inp, argv, tmp_path, block=None):
    want, _, _ = _run(inp, argv, tmp_path, "h", device=False)
    got, info, err = _run(inp, argv, tmp_path, "d", block=block)
    assert got == want
    return got, info, err


@pytest.mark.parametrize("n_cols", [1, 63, 64, 65, 129, 1100])
def test_column_counts_at_the_edges_of_the_lane_stride(n_cols, tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, n_cols, 300, n_cols)
    got, info, _ = _both(inp, ["-f", "phased"], tmp_path)
    rows = got["geno"].split(b"\n")[:-1]
    assert 10 < len(rows) < 300 and all(len(r) == n_cols for r in rows) and got["snp"].count(b"\n") == len(rows)
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0, info


@pytest.mark.parametrize("n_lines", [1, 1023, 1024, 1025, 2049])
def test_line_counts_at_the_edges_of_the_scan_threads(n_lines, tmp_path):
    """one block whose lines k_rows_scan's 1 024 threads share out one each with threads to spare, one each exactly, and two and three
    each with the last threads left without: kept and dropped sites mixed, so that a line's rank is not its number and a wrong rank
    or place moves a row.  (The one line of the first case is all missing by _wide's rule for every seventh line: no site is kept,
    and the block still is the device's)"""
    inp = str(tmp_path / "w.geno")
    _wide(inp, 3, n_lines, 31)
    got, info, _ = _both(inp, ["-f", "phased"], tmp_path)
    kept = got["geno"].count(b"\n")
    assert (0 < kept < n_lines if n_lines > 1 else kept == 0) and got["snp"].count(b"\n") == kept, kept
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0, info


def test_three_of_1100_columns_where_the_others_alone_make_the_sites_biallelic(tmp_path):
    """the three selected samples carry one base at every site: counted over them alone no site would be kept"""
    inp = str(tmp_path / "w.geno")
    names = _wide(inp, 1100, 300, 5)
    sel = [names[1099], names[64], names[0]]
    with open(inp) as f:
        lines = f.read().split("\n")
    for k in range(1, 301):
        f = lines[k].split("\t")
        base = next((c for cell in f[2:] for c in cell[::2] if c != "N"), "N")
        for j in (2, 66, 1101):
            f[j] = base + "/" + base
        lines[k] = "\t".join(f)
    with open(inp, "w") as f:
        f.write("\n".join(lines))
    got, info, _ = _both(inp, ["-f", "phased", "-s", ",".join(sel)], tmp_path)
    rows = got["geno"].split(b"\n")[:-1]
    assert len(rows) > 30 and all(r in (b"000", b"222") for r in rows) and got["ind"] == b"w0  U  NA\nw64  U  NA\nw1099  U  NA\n"
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0, info


def test_snp_rows_longer_than_their_text_grow_the_buffer(tmp_path):
    """one diploid sample, het sites, chromosome labels of 40 bytes: a .snp row of some 60 bytes from a line of 15, more than the
    room the route sets out with (32 bytes a line and 256, an eighth and 4 096 on top)"""
    inp = str(tmp_path / "w.geno")
    with open(inp, "w") as f:
        f.write("#CHROM\tPOS\ta\n" + "".join("u%d\t%d\tA/T\n" % (i // 100, 100000 + i) for i in range(300)))
    chrom = str(tmp_path / "chrom.txt")
    with open(chrom, "w") as f:
        f.write("".join("u%d\t%s\n" % (k, (("label%d_" % k) * 6)[:40]) for k in range(3)))
    got, info, _ = _both(inp, ["-f", "phased", "--chromFile", chrom], tmp_path)
    assert got["geno"] == b"1\n" * 300 and len(got["snp"]) > 300 * 56 > (300 * 32 + 256) * 9 // 8 + 4096
    assert got["snp"].split(b"\n")[299] == b"299\t" + ("label2_" * 6)[:40].encode() + b"\t0.0\t100299\tA\tT"
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0, info


def test_site_indices_over_many_blocks_with_sites_not_kept_at_block_ends(tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, 9, 300, 17)
    got, info, _ = _both(inp, ["-f", "phased"], tmp_path, block=1500)
    index = [int(r.split(b"\t")[0]) for r in got["snp"].split(b"\n")[:-1]]
    assert index == sorted(set(index)) and index[-1] > 280 and len(index) < 250
    assert int(info["device_blocks"]) >= 8 and int(info["device_host_blocks"]) == 0 and int(info["blocks_redone_on_host"]) == 0, info


def test_a_scaffold_change_and_an_unlisted_scaffold_inside_one_block(tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, 7, 300, 9, scaf=lambda i: ("listed", "unlisted", "a_scaffold_with_a_name_of_more_than_sixty_four_bytes_" + "z" * 30)[i * 3 // 300])
    chrom = str(tmp_path / "chrom.txt")
    with open(chrom, "w") as f:
        f.write("listed 3\nliste 4\nlisted_ 5\na_scaffold_with_a_name_of_more_than_sixty_four_bytes_" + "z" * 30 + "\tlong\n")
    got, info, _ = _both(inp, ["-f", "phased", "--chromFile", chrom, "--nullChrom", "0"], tmp_path)
    labels = [r.split(b"\t")[1] for r in got["snp"].split(b"\n")[:-1]]
    assert sorted(set(labels)) == [b"0", b"3", b"long"] and labels == sorted(labels, key=[b"3", b"0", b"long"].index)
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0, info


def _spoil(inp, line, how):
    with open(inp) as f:
        lines = f.read().split("\n")
    lines[line:line + 1] = how(lines[line])
    with open(inp, "w") as f:
        f.write("\n".join(lines))


@pytest.mark.parametrize("what", ["ten_alleles", "double_tab", "hash_line"])
def test_a_line_the_device_does_not_take_hands_exactly_its_block_to_the_host(what, tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, 5, 300, 21)
    how = {"ten_alleles": lambda ln: ["\t".join(ln.split("\t")[:2] + ["/".join("A" * 10)] + ["C/C/C"] * 4)],
           "double_tab": lambda ln: [ln.replace("\t", "\t\t", 1)],
           "hash_line": lambda ln: [ln, "# no site"]}[what]
    _spoil(inp, 297, how)                                    # in the last block: the site indices behind a '#' line do not move
    got, info, _ = _both(inp, ["-f", "phased"], tmp_path, block=4000)
    assert got["snp"].count(b"\n") > 30                     # (kept sites in every block)
    if what == "ten_alleles":
        assert b"\n296\t22\t0.0\t297\tA\tC\n" in got["snp"] and b"\n100000\n" in got["geno"]
    assert int(info["device_blocks"]) >= 2 and int(info["device_host_blocks"]) == 1 and int(info["blocks_redone_on_host"]) == 0, info


def test_a_hash_line_in_the_middle_moves_the_index_of_the_blocks_behind_it(tmp_path):
    """the block after the one with the '#' line was given an index one too high: it is converted again, by the host route; the blocks
    behind it are the device's again"""
    inp = str(tmp_path / "w.geno")
    _wide(inp, 5, 300, 21)
    _spoil(inp, 100, lambda ln: [ln, "# no site"])
    got, info, _ = _both(inp, ["-f", "phased"], tmp_path, block=2000)
    assert int(info["device_host_blocks"]) == 1 and int(info["blocks_redone_on_host"]) == 1 and int(info["blocks_on_device"]) >= 2, info


def test_cumulative_positions_and_a_repeated_name_go_to_the_host_whole(tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, 5, 300, 23)
    got, info, err = _both(inp, ["-f", "phased", "--cumulativePos"], tmp_path)
    assert "--cumulativePos" in err and "host threads do the job" in err and "device_blocks" not in info and int(info["blocks_on_host"]) == 1
    _spoil(inp, 0, lambda ln: [ln.replace("w3", "w1")])
    got, info, err = _both(inp, ["-f", "phased"], tmp_path)
    assert "more than once" in err and "host threads do the job" in err and "device_blocks" not in info
    assert got["ind"] == b"w0  U  NA\nw1  U  NA\nw2  U  NA\nw1  U  NA\nw4  U  NA\n"
