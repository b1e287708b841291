"""The genoToPlink.py drop-in's device route (pg_ped_dev_*: k_ped_lines, k_ped_map, k_ped_tile) on an MI355X: every golden of the
unmodified reference the device takes, the files byte for byte from gzip, plain and BGZF input (members inflated on the device), in
one block and in many small ones; the goldens with blocks it hands back; then device against host route on seeded files of at most
300 lines: site counts at the tile's edge, sample counts at the edges of the lanes' stride and of the tile, three of 1 100 columns,
haploid and tetraploid columns among diploids, -f diplo with every letter, scaffold changes inside a block and at a block's end, .map
rows that outgrow their buffer, lines that hand their block back, a short cell that cuts the rows the device made before it.  Each run
is a process of its own under a time limit; PG_TIMING's counters show where the blocks went."""
import gzip
import os
import random
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from plink_cases import CASES, DEVICE, HOST_BLOCKS, HOST_WHOLE, command, fixture_path, golden  # noqa: E402

pytestmark = pytest.mark.gpu

BY_NAME = {c[0]: c for c in CASES}


def _run(inp, argv, tmp_path, tag, device=True, block=None, tile=None, timeout=120):
    """the files, PG_TIMING's counters and stderr"""
    env = dict(os.environ, PG_TIMING="1", PG_PED_DEVICE="1" if device else "0")
    if block:
        env["PG_STREAM_BYTES"] = str(block)
    if tile:
        env["PG_PED_TILE_SEQS"] = str(tile)
    args, outs = command(argv, inp, str(tmp_path), tag)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "genoToPlink.py"), "-g", inp] + args,
                       stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=timeout, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-3000:]
    info = {}
    m = re.search(r"PG_TIMING ped (.*)", r.stderr.decode())
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
    """a copy of the fixture as it is, as plain text, or as bgzip's BGZF members (inflated on the device); its text"""
    from genomics_general_amd import genoio
    inp = fixture_path(fixture)
    with (gzip.open(inp, "rb") if inp.endswith(".gz") else open(inp, "rb")) as f:
        text = f.read()
    if source == "gz":
        p = str(tmp_path / ("in.geno.gz" if inp.endswith(".gz") else "in.geno"))
        shutil.copy(inp, p)
        return p, text
    p = str(tmp_path / ("in.geno" + (".gz" if source == "bgzf" else "")))
    with open(p, "wb") as g:
        g.write(genoio.bgzf_compress(text, block=7000) if source == "bgzf" else text)
    return p, text


@pytest.mark.parametrize("name", DEVICE)
@pytest.mark.parametrize("source,block", [("gz", None), ("plain", None), ("plain", 20000), ("bgzf", None), ("bgzf", 30000)])
def test_device_route_reproduces_the_reference(name, source, block, tmp_path):
    _, fixture, argv = BY_NAME[name]
    inp, text = _source(fixture, source, tmp_path)
    got, info, _ = _run(inp, argv, tmp_path, "d", block=block)
    assert got == golden(name)
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0 and int(info["blocks_on_host"]) == 1, info
    if source == "bgzf" and len(text) > 3 * 7000:             # (of one or two members the reads of the first lines inflate all)
        assert int(info["blocks_inflated_on_device"]) >= 1, info


@pytest.mark.parametrize("name", sorted(HOST_BLOCKS | HOST_WHOLE))
def test_goldens_the_device_hands_back_come_out_the_same(name, tmp_path):
    _, fixture, argv = BY_NAME[name]
    inp, _ = _source(fixture, "plain", tmp_path)
    got, info, _ = _run(inp, argv, tmp_path, "d")
    assert got == golden(name)
    if name in HOST_WHOLE:
        assert "device_blocks" not in info
    else:
        assert int(info["device_host_blocks"]) >= 1, info


def _wide(path, n_cols, n_lines, seed, cell=None, scaf=None, pos=None):
    """n_lines sites of n_cols samples: diploid cells with '/' and '|', N, lower case and IUPAC letters, two scaffolds"""
    R = random.Random(seed)
    names = ["w%d" % k for k in range(n_cols)]
    rows = ["\t".join(["#CHROM", "POS"] + names)]
    for i in range(n_lines):
        cells = [cell(R, i, k) if cell else R.choice("ACGTNacgt*-") + R.choice("/|") + R.choice("ACGTNRYK") for k in range(n_cols)]
        rows.append("\t".join([scaf(i) if scaf else "u%d" % (i * 2 // n_lines), pos(i) if pos else str(i + 1)] + cells))
    with open(path, "w") as f:
        f.write("\n".join(rows) + "\n")
    return names


def _both(inp, argv, tmp_path, block=None, tile=None):
    want, _, _ = _run(inp, argv, tmp_path, "h", device=False)
    got, info, err = _run(inp, argv, tmp_path, "d", block=block, tile=tile)
    assert got == want
    return got, info, err


@pytest.mark.parametrize("n_sites", [127, 128, 129, 257])
def test_site_counts_at_the_edge_of_the_tile(n_sites, tmp_path):
    """the first site is the host's: the device's block holds n_sites of them"""
    inp = str(tmp_path / "w.geno")
    _wide(inp, 9, n_sites + 1, n_sites)
    got, info, _ = _both(inp, ["--prefix", "@P"], tmp_path)
    assert got["map"].count(b"\n") == n_sites + 1 and all(len(r) == 12 + 4 * (n_sites + 1) for r in got["ped"].split(b"\n")[:-1])
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0 and int(info["sites"]) == n_sites + 1, info


@pytest.mark.parametrize("n_sel", [1, 63, 64, 65, 129, 124])
def test_sample_counts_at_the_edges_of_the_lane_stride_and_of_the_tile(n_sel, tmp_path):
    """124 diploids: the LDS holds (65 536 - 16 x 126) // 516 = 123 of them beside the tab tables, the second tile one"""
    inp = str(tmp_path / "w.geno")
    _wide(inp, n_sel, 300, n_sel)
    got, info, _ = _both(inp, ["--prefix", "@P", "-f", "phased"], tmp_path)
    assert got["ped"].count(b"\n") == n_sel
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0, info
    if n_sel == 124:
        assert int(info["tile_seqs"]) == 123, info
    else:
        assert int(info["tile_seqs"]) == min(n_sel, (65536 - 16 * (n_sel + 2)) // 516), info


def test_sample_tiles_of_three_with_a_selection_in_another_order(tmp_path):
    inp = str(tmp_path / "w.geno")
    names = _wide(inp, 11, 300, 3)
    sel = [names[k] for k in (10, 0, 5, 4, 9, 1, 7)]
    got, info, _ = _both(inp, ["--prefix", "@P", "-s"] + sel + ["--makeFAM"], tmp_path, tile=3, block=5000)
    assert [r.split(b" ")[1].decode() for r in got["ped"].split(b"\n")[:-1]] == sel
    assert int(info["device_blocks"]) >= 2 and int(info["device_host_blocks"]) == 0 and int(info["tile_seqs"]) == 3, info


def test_three_of_1100_columns(tmp_path):
    inp = str(tmp_path / "w.geno")
    names = _wide(inp, 1100, 300, 5)
    sel = [names[1099], names[64], names[0]]
    got, info, _ = _both(inp, ["--prefix", "@P", "-s"] + sel, tmp_path)
    assert got["ped"].count(b"\n") == 3 and got["ped"].startswith(b"0 w1099 0 0 0 0 ")
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0, info


@pytest.mark.parametrize("fmt", ["phased", "alleles"])
def test_a_haploid_and_a_tetraploid_column_among_diploids(fmt, tmp_path):
    """131 sites in the device's block: a haploid's row of 262 bytes, a diploid's of 524 (786 under alleles, where its separator is
    an allele too) and a tetraploid's of 1 048 end inside a 16-byte store.  Under alleles the tetraploid is spelled as four
    characters: the seven of a|b|c|d are more alleles than the device takes"""
    inp = str(tmp_path / "w.geno")
    four = (lambda R: "|".join(R.choice("ACGT") for _ in range(4))) if fmt == "phased" else (lambda R: "".join(R.choice("ACGT") for _ in range(4)))

    def cell(R, i, k):
        return R.choice("ACGTN") if k == 2 else four(R) if k == 5 else R.choice("ACGTN") + R.choice("/|") + R.choice("ACGTN")

    _wide(inp, 7, 132, 11, cell=cell)
    got, info, _ = _both(inp, ["--prefix", "@P", "-f", fmt], tmp_path)
    per = {"phased": (2, 4, 8), "alleles": (2, 6, 8)}[fmt]
    rows = got["ped"].split(b"\n")[:-1]
    assert [len(r) - len(b"0 w0 0 0 0 0 ") + 1 for r in rows] == [132 * per[0 if k == 2 else 2 if k == 5 else 1] for k in range(7)]
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0, info


def test_diplo_with_every_letter(tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, 13, 300, 13, cell=lambda R, i, k: "ACGKMNSRTWY"[(i + k) % 11])
    got, info, _ = _both(inp, ["--prefix", "@P", "-f", "diplo"], tmp_path)
    assert got["ped"].split(b"\n")[0].startswith(b"0 w0 0 0 0 0 A A C C G G G T A C N N C G A G T T A T C T A A")
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0, info


def test_scaffold_changes_inside_a_block_and_exactly_at_a_block_boundary(tmp_path):
    """lines of 30 bytes in blocks of 1 500: behind the first site, the host's, a block holds 50 lines; the scaffold changes with
    the first line of the second and of the third block, at sites 120 and 130 inside a block; `one` comes back twice and goes on
    across three block ends"""
    inp = str(tmp_path / "w.geno")
    scaf = lambda i: "one" if i < 51 else "two" if i < 101 else "one" if i < 120 else "six" if i < 130 else "one"     # noqa: E731
    _wide(inp, 5, 300, 9, scaf=scaf, pos=lambda i: "%05d" % (i + 1000), cell=lambda R, i, k: R.choice("ACGT") + "|" + R.choice("ACGT"))
    with open(inp) as f:
        assert {len(ln) for ln in f.read().split("\n")[1:-1]} == {29}
    got, info, err = _both(inp, ["--prefix", "@P"], tmp_path, block=1500)
    assert [ln.split(b" ")[0] for ln in got["map"].split(b"\n")[:-1]] == [scaf(i).encode() for i in range(300)]
    assert err.count("scaffolds read into memory") == 5 and int(info["runs"]) == 5
    assert int(info["device_blocks"]) >= 6 and int(info["device_host_blocks"]) == 0, info


def test_map_rows_longer_than_their_room_grow_the_buffer(tmp_path):
    """18-digit positions with zeros in front and scaffold names of 60 bytes: a .map row of some 100 bytes, more than the room the
    route sets out with (32 bytes a line and 256, an eighth and 4 096 on top)"""
    inp = str(tmp_path / "w.geno")
    _wide(inp, 3, 300, 15, scaf=lambda i: ("scaffold_%d_" % (i // 100)) + "x" * 50, pos=lambda i: "00%d" % (10 ** 17 + i))
    got, info, _ = _both(inp, ["--prefix", "@P"], tmp_path)
    assert len(got["map"]) > 300 * 100 > (300 * 32 + 256) * 9 // 8 + 4096
    assert got["map"].split(b"\n")[299] == b"scaffold_2_" + b"x" * 50 + b" 100000000000000299 0 100000000000000299"
    assert int(info["device_blocks"]) == 1 and int(info["device_host_blocks"]) == 0, info


def _spoil(inp, line, how):
    with open(inp) as f:
        lines = f.read().split("\n")
    lines[line:line + 1] = how(lines[line])
    with open(inp, "w") as f:
        f.write("\n".join(lines))


@pytest.mark.parametrize("what", ["short_cell", "long_cell", "double_tab", "plus_position"])
def test_a_line_the_device_does_not_take_hands_exactly_its_block_to_the_host(what, tmp_path):
    inp = str(tmp_path / "w.geno")
    _wide(inp, 5, 300, 21)
    how = {"short_cell": lambda ln: ["\t".join(ln.split("\t")[:2] + ["A"] + ln.split("\t")[3:])],
           "long_cell": lambda ln: ["\t".join(ln.split("\t")[:2] + ["A/C/G"] + ln.split("\t")[3:])],
           "double_tab": lambda ln: [ln.replace("\t", "\t\t", 1)],
           "plus_position": lambda ln: [ln.replace("\t", "\t+", 1)]}[what]
    _spoil(inp, 297, how)
    got, info, _ = _both(inp, ["--prefix", "@P"], tmp_path, block=4000)
    assert got["map"].count(b"\n") == 300
    if what == "short_cell":
        assert got["ped"].split(b"\n")[0].count(b" ") == 6 + 449      # (the second scaffold's 150 sites: w0's alleles cut to one a site)
    assert int(info["device_blocks"]) >= 2 and int(info["device_host_blocks"]) == 1, info


def test_hash_lines_stay_on_the_device(tmp_path):
    """k_ped_lines marks them: no site, no .map row, the run goes on across them; one of them opens a block"""
    inp = str(tmp_path / "w.geno")
    _wide(inp, 5, 300, 21)
    for at in (200, 100, 99, 2):
        _spoil(inp, at, lambda ln: ["# no site\t1\tA/A", ln])
    got, info, _ = _both(inp, ["--prefix", "@P"], tmp_path, block=2000)
    assert got["map"].count(b"\n") == 300 and int(info["runs"]) == 2
    assert int(info["device_blocks"]) >= 4 and int(info["device_host_blocks"]) == 0, info


def test_a_short_cell_in_block_3_cuts_the_rows_of_device_blocks_1_and_2(tmp_path):
    """one scaffold; sample b's haploid cell at site 250 hands its block back and cuts b's alleles in the whole run to one a site"""
    rows = ["c\t%d\t%s\t%s\t%s" % (i + 1, "AC"[i % 2] + "|G", "T|" + "AC"[i % 2] if i != 250 else "G", "N|N") for i in range(300)]
    inp = str(tmp_path / "i.geno")
    with open(inp, "w") as f:
        f.write("#CHROM\tPOS\ta\tb\tc\n" + "\n".join(rows) + "\n")
    got, info, _ = _both(inp, ["--prefix", "@P"], tmp_path, block=1500)
    ped = got["ped"].split(b"\n")
    assert ped[1] == b"0 b 0 0 0 0 " + b" ".join(b"T" if i != 250 else b"G" for i in range(300))
    assert ped[0] == b"0 a 0 0 0 0 " + b" ".join(b"AC"[i % 2:i % 2 + 1] + b" G" for i in range(300)) and ped[2] == b"0 c 0 0 0 0" + b" N N" * 300
    assert int(info["device_host_blocks"]) == 1 and int(info["blocks_on_device"]) >= 2 and int(info["runs"]) == 1, info
