"""The seqToGeno.py drop-in's device route (pg_s2g_dev_*: k_s2g_lines, k_s2g_gather, k_s2g_tile) on an MI355X: every golden of the
unmodified reference from plain, gzip and BGZF input (members inflated on the device), in one block and in small ones -- the goldens
the device takes whole, those with blocks it hands back, the phylip ones whose lines it emits --, then device against host route
(and against lines made here) on seeded files at the smallest shapes that can go wrong: site counts at the tile's edge, positions
whose digits change inside a tile, haplotype counts at the edges of the lanes' stride and of the tile over several column tiles,
mixed ploidies, wrap widths, many short records as contigs, input blocks that cut inside a record, output ranges that end inside a
tile, a blank inside a sequence, BGZF in and out, a short later sequence.  Each run is a process of its own under a time limit;
PG_TIMING's counters show where the work went."""
import os
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from s2g_common import expected, fasta, run  # noqa: E402
from s2g_cases import CASES, DEVICE, HOST_BLOCKS, HOST_LOAD, SINGLE_PLOIDY, golden, input_bytes  # noqa: E402

pytestmark = pytest.mark.gpu

BY_NAME = {c[0]: c for c in CASES}


def _both(data, argv, tmp_path, status=0, **kw):
    """device and host route give the same status and bytes; the device's bytes and counters"""
    rc_h, host, _, err_h = run(data, argv, tmp_path, device=False, tag="h")
    rc_d, dev, info, err_d = run(data, argv, tmp_path, device=True, tag="d", **kw)
    assert rc_h == status, err_h[-2000:]
    assert rc_d == status, err_d[-2000:]
    assert dev == host
    return dev, info


@pytest.mark.parametrize("name", DEVICE)
@pytest.mark.parametrize("source,block", [("plain", None), ("plain", 3000), ("gz", None), ("bgzf", 9000)])
def test_device_route_reproduces_the_reference(name, source, block, tmp_path):
    _, inp, argv, _ = BY_NAME[name]
    data = input_bytes(inp)
    rc, got, info, err = run(data, argv, tmp_path, source=source, device=True, block=block)
    assert rc == 0, err[-2000:]
    assert got == golden(name)
    assert int(info["device_blocks"]) >= 1 and int(info["device_host_blocks"]) == 0 and int(info["out_ranges"]) >= 1, info
    if source == "bgzf" and len(data) > 3 * 7000:
        assert int(info["blocks_inflated_on_device"]) >= 1, info


@pytest.mark.parametrize("name", sorted(HOST_BLOCKS))
@pytest.mark.parametrize("block", [None, 700])
def test_blocks_handed_back_give_the_same_bytes(name, block, tmp_path):
    _, inp, argv, _ = BY_NAME[name]
    rc, got, info, err = run(input_bytes(inp), argv, tmp_path, device=True, block=block)
    assert rc == 0, err[-2000:]
    assert got == golden(name)
    assert int(info["device_host_blocks"]) >= 1, info


@pytest.mark.parametrize("name", sorted(HOST_LOAD))
def test_phylip_is_loaded_by_the_host_and_emitted_by_the_device(name, tmp_path):
    _, inp, argv, _ = BY_NAME[name]
    rc, got, info, err = run(input_bytes(inp), argv, tmp_path, device=True, block=5000)
    assert rc == 0, err[-2000:]
    assert got == golden(name)
    assert int(info["device_blocks"]) == 0 and int(info["out_ranges"]) >= 1, info


@pytest.mark.parametrize("inp,argv,gold", SINGLE_PLOIDY)
def test_single_ploidy_value(inp, argv, gold, tmp_path):
    rc, got, _, err = run(input_bytes(inp), argv, tmp_path, device=True)
    assert rc == 0, err[-2000:]
    assert got == golden(gold)


@pytest.mark.parametrize("n_sites", [1, 127, 128, 129, 257])
def test_sites_at_the_tile_edge(n_sites, tmp_path):
    data = fasta(n_sites, 5, n_sites)
    got, info = _both(data, ["-C", "c"], tmp_path)
    assert got == expected(data, chrom="c")
    assert int(info["device_host_blocks"]) == 0 and int(info["sites"]) == n_sites, info


def test_digits_change_inside_a_tile(tmp_path):
    data = fasta(11, 3, 10001)
    got, info = _both(data, [], tmp_path)
    assert got == expected(data)
    assert int(info["device_host_blocks"]) == 0, info


@pytest.mark.parametrize("n_hap,tile", [(63, None), (64, None), (65, None), (6, 5), (11, 5), (65, 7)])
def test_haplotypes_at_the_lane_stride_and_the_tile_edge(n_hap, tile, tmp_path):
    data = fasta(100 + n_hap, n_hap, 131, width=61)
    got, info = _both(data, [], tmp_path, tile=tile)
    assert got == expected(data)
    assert int(info["device_host_blocks"]) == 0, info
    if tile:
        assert int(info["tile_seqs"]) == tile, info


@pytest.mark.parametrize("tile", [None, 5])
def test_mixed_ploidies(tile, tmp_path):
    data = fasta(21, 14, 200)
    sizes = [1, 2, 4, 1, 4, 2]
    got, _ = _both(data, ["-P"] + [str(p) for p in sizes], tmp_path, tile=tile)
    assert got == expected(data, sizes)


@pytest.mark.parametrize("width", [1, 60, 61, 0])
def test_wrap_widths(width, tmp_path):
    data = fasta(31 + width, 4, 183, width=width)                # (183 = 3 x 61: every sequence ends exactly at a line's end at 61)
    got, info = _both(data, [], tmp_path, block=2000)
    assert got == expected(data)
    assert int(info["device_host_blocks"]) == 0, info


def test_many_short_records_as_contigs(tmp_path):
    data = fasta(41, 300, 3)
    got, info = _both(data, ["-M", "contigs", "-N", "me"], tmp_path)
    assert got.count(b"\n") == 901 and got.startswith(b"#CHROM\tPOS\tme\nq0\t1\t")
    assert int(info["device_host_blocks"]) == 0, info
    _both(data, ["-M", "contigs", "-P", "1", "2", "2", "1"] + ["1"] * 294, tmp_path)


def test_input_blocks_cut_inside_a_record_and_ranges_inside_a_tile(tmp_path):
    data = fasta(51, 7, 1500)
    got, info = _both(data, [], tmp_path, block=2000)
    assert got == expected(data)
    assert int(info["device_blocks"]) >= 4 and int(info["out_ranges"]) >= 4 and int(info["device_host_blocks"]) == 0, info


def test_a_blank_inside_a_sequence_hands_its_block_back(tmp_path):
    data = fasta(61, 5, 900)
    cut = data.index(b"\n", len(data) // 2) - 7
    data = data[:cut] + b" " + data[cut:]
    got, info = _both(data, [], tmp_path, block=1500)
    assert got == expected(data)
    assert int(info["device_host_blocks"]) >= 1 and int(info["device_blocks"]) > int(info["device_host_blocks"]), info


def test_bgzf_in_and_out(tmp_path):
    data = fasta(71, 6, 9000)
    rc, got, info, err = run(data, ["-P", "2"], tmp_path, source="bgzf", device=True, block=20000, out="gz")
    assert rc == 0, err[-2000:]
    assert got == expected(data, [2, 2, 2])
    assert int(info["blocks_inflated_on_device"]) >= 1 and int(info["device_host_blocks"]) == 0, info


def test_a_short_later_sequence_stops_both_routes_alike(tmp_path):
    data = fasta(81, 4, 0, lengths=[300, 300, 170, 300])
    got, _ = _both(data, [], tmp_path, status=1)
    assert got.count(b"\n") == 171
    assert got == expected(data)
