"""k_vcf_cells, k_vcf_heads and k_rows_scan (csrc/pg_vcf_dev.hip, pg_line_slot.hip) where their lanes, steps and blocks turn over: the
files of tests/vcf_cell_cases.py through parseVCF's device route and its host route, both held byte for byte against a model that
knows the calls from the generator (tests/test_vcf_cell_cases.py shows on the CPU that the emulated device path takes every regular
set whole: so here no block may go to the host -- a fault in the tab scan would otherwise hide behind the hand-over, which costs
only speed and changes no byte).

What a red case stands on:

LANES   the 64-lane trips over the selected samples (`s0 += 64`): 1, 2, 63, 64, 65, 128, 129 selected; the last lane of a trip and
        the first of the next one (`s + 1 == n_sel`: line feed against separator); on the indel lines `run`, which carries the bytes
        of a trip's cells into the next one (the wave scan of the cells' sizes; k_vcf_cells<0> leaves their total in rlen); -s in
        reversed and scattered order (tabs[col - 1] read out of order from LDS); ploidy 1 on every third sample (cell_off strides of 2
        and 4 across the 64th lane); --addRefTrack, --outSep and --missing on pl_129.  blocks_3000: a few lines a block (the files of 63 columns and
        more), every block's lines at another place of the slot
ALIGN   the `valid` mask at the section's start (`rel < cells_off`) and at its end (`rel + 16 > line_len`): all 16 places of cells_off
        in its 16-byte word; sections of 3 bytes and 1 byte, where both masks cut the same word -- or, at places 14 and 15, the two
        words of the 3 bytes; the last column without a tab (`c < n_tabs ? tabs[c] : line_len`) as the only column.  bgzf_700: the
        text inflated on the device, lines at other places of the slot
STEPS   the 1024-byte step of the tab scan (`g0 += 1024`, lane * 16): sections ending one byte before, on and one byte behind the
        first and the second step (a second or third trip for 1 .. 16 bytes), a tab in the last byte of a step and in the first of
        the next (`n_tabs += total` between trips: the ranks of the tabs go on where the step before left them)
EXTRA   the loop's early exit (`n_tabs < n_cols`) with the n_cols-th tab as the last byte of the first step and the first of the
        second; the blank rule's column index (`r + popc(tm below j) < n_cols`): a blank behind the named columns in the word of
        their last tab, 3000 bytes behind it, a column of one blank; a trailing tab (`n_tabs > n_cols`); a byte >= 0x80 (no blank
        for bytes_blank, a cell piece nobody reads)
HOSTLINES  what the scan must hand over, and only that block: a blank at the end of the last named column, 0x0b and 0x1f inside a
        cell, an empty column (`b <= a`), a column fewer than the header (`n_tabs < n_cols - 1`); blank_r*: a blank in a column
        that is not selected -- only the scan sees it -- at every place of a 16-byte word, in the word that holds cells_off
WAVES   waves_per_block 4, 2, 2, 1, 1 (3840, 3841, 7680, 7681, 14000 columns: `tabs = sh_tabs + wave * n_cols`, the dynamic LDS
        of a block); 1, 2, 3, 4, 5, 9 lines: a last block partly empty (`i >= n_lines`); column 0 (starts at cells_off), the last
        column (ends at line_len); 14001 columns stay on the host
ROOM    k_rows_scan's overflow bit: a complex row longer than its line inside out_cap stays on the device; 304 KB of rows for a
        room of 20 KB raise PG_ST_OVERFLOW, k_vcf_cells<1> writes nothing (`status[0] != 0`) and the block goes to the host
SCAN    k_vcf_heads' blocks of 256 lines (255, 256, 257) and k_rows_scan's stretch of lines per thread (1023, 1024 -> 1; 1025 -> 2;
        2049 -> 3), lines without a row (rlen == 0: comment lines, lines --minQual drops) at every place of a stretch"""
import pytest

import vcf_cell_cases as VC
from test_gpu_vcf import _run

from genomics_general_amd import genoio

pytestmark = pytest.mark.gpu
ONE_BLOCK = str(1 << 27)


def _both_routes(case, tmp_path, monkeypatch, form="plain", stream=ONE_BLOCK):
    """the case's file through the device route and the host route: (device bytes, host bytes, the device run's info)"""
    text = case["head"] + case["body"]
    if form == "plain":
        path = str(tmp_path / "in.vcf")
        data = text
    else:
        path = str(tmp_path / "in.vcf.gz")
        data = genoio.bgzf_compress(text, 6, int(form.split("_")[1])).tobytes()
    with open(path, "wb") as f:
        f.write(data)
    argv = VC.argv_of(case, tmp_path)
    env = {"PG_STREAM_BYTES": stream}
    dev, info = _run(path, str(tmp_path / "dev.geno"), argv, env, monkeypatch)
    host, _ = _run(path, str(tmp_path / "host.geno"), argv, env, monkeypatch, device="0")
    return dev, host, info


def _difference(got, want):
    k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    row = want.count(b"\n", 0, k)
    return "first difference in row %d, at byte %d of %d / %d: %r != %r" % (row, k, len(got), len(want), got[max(k - 40, 0):k + 40],
                                                                           want[max(k - 40, 0):k + 40])


def _all_on_the_device(case, tmp_path, monkeypatch, form="plain", stream=ONE_BLOCK):
    want = VC.header_row(case) + VC.expected(case)
    dev, host, info = _both_routes(case, tmp_path, monkeypatch, form, stream)
    assert host == want, _difference(host, want)
    assert dev == want, _difference(dev, want)
    # every block the device was given came back as rows: no line of these files is one it may hand over
    assert info["blocks_parsed_on_device"] >= 1 and info["stats"] == (info["blocks_parsed_on_device"], 0), info
    return info


@pytest.mark.parametrize("form", ["one_block", "blocks_3000"])
@pytest.mark.parametrize("name", VC.LANES)
def test_lanes_counts_of_selected_samples_around_the_64_lane_trips(name, form, tmp_path, monkeypatch):
    case = VC.lanes(name)
    info = _all_on_the_device(case, tmp_path, monkeypatch, stream=ONE_BLOCK if form == "one_block" else "3000")
    if form == "one_block":
        assert info["blocks"] == 1, info
    elif len(case["body"]) > 9000:
        assert info["blocks"] >= 3, info


@pytest.mark.parametrize("form", ["plain", "bgzf_700"])
@pytest.mark.parametrize("name", VC.ALIGN)
def test_align_sections_at_every_place_of_a_16_byte_word(name, form, tmp_path, monkeypatch):
    _all_on_the_device(VC.align(name), tmp_path, monkeypatch, form)


@pytest.mark.parametrize("form", ["plain", "bgzf_700"])
@pytest.mark.parametrize("B", VC.STEPS)
def test_steps_sections_and_tabs_on_both_sides_of_a_1024_byte_step(B, form, tmp_path, monkeypatch):
    """(the ranges of tests/vcf_cell_cases.py are not trimmed: every S in [B - 24, B + 24] at all 16 residues)"""
    _all_on_the_device(VC.steps(B), tmp_path, monkeypatch, form)


@pytest.mark.parametrize("name", VC.EXTRA)
def test_extra_columns_behind_the_named_ones_stay_on_the_device(name, tmp_path, monkeypatch):
    _all_on_the_device(VC.extra(name), tmp_path, monkeypatch)


@pytest.mark.parametrize("name", VC.HOSTLINES)
def test_hostlines_hand_exactly_their_block_over(name, tmp_path, monkeypatch):
    case = VC.hostline(name)
    if case["raises"]:                                            # a named column missing: both routes end with the host parser's words
        from genomics_general_amd._lib import PopgenError
        for dev in ("1", "0"):
            path = str(tmp_path / "in.vcf")
            with open(path, "wb") as f:
                f.write(case["head"] + case["body"])
            with pytest.raises(PopgenError, match=case["raises"]):
                _run(path, str(tmp_path / "x.geno"), VC.argv_of(case, tmp_path), case["env"], monkeypatch, device=dev)
        return
    dev, host, info = _both_routes(case, tmp_path, monkeypatch, stream=case["env"]["PG_STREAM_BYTES"])
    assert dev == host, _difference(dev, host)
    # (all other lines are the model's: the planted line's row is the host parser's business)
    at = VC.planted_line(case)
    before = VC.header_row(case) + VC.model(case["truth"][:at], case["sel"], case["sep"], case["missing"])
    behind = VC.model(case["truth"][at + 1:], case["sel"], case["sep"], case["missing"])
    assert dev.startswith(before) and dev.endswith(behind) and dev.count(b"\n") == before.count(b"\n") + 1 + behind.count(b"\n")
    blocks, host_blocks = info["stats"]
    assert host_blocks == 1 and blocks >= 3, info


@pytest.mark.parametrize("name", VC.ROOM)
def test_room_rows_longer_than_the_text_inside_and_beyond_the_output(name, tmp_path, monkeypatch):
    case = VC.room(name)
    if name == "fits":
        _all_on_the_device(case, tmp_path, monkeypatch)
        return
    want = VC.header_row(case) + VC.expected(case)
    dev, host, info = _both_routes(case, tmp_path, monkeypatch)
    assert host == want, _difference(host, want)
    assert dev == want, _difference(dev, want)
    assert info["stats"] == (1, 1), info                           # the overflow bit: the one block went to the host


@pytest.mark.parametrize("n_lines", VC.WAVES_LINES)
@pytest.mark.parametrize("n_cols", VC.WAVES_COLS)
def test_waves_every_block_shape_with_a_last_block_partly_empty(n_cols, n_lines, tmp_path, monkeypatch):
    _all_on_the_device(VC.waves(n_cols, n_lines), tmp_path, monkeypatch)


def test_waves_one_column_too_many_stays_on_the_host(tmp_path, monkeypatch):
    case = VC.waves(VC.WAVES_TOO_MANY, 3)
    want = VC.header_row(case) + VC.expected(case)
    dev, host, info = _both_routes(case, tmp_path, monkeypatch)
    assert dev == want and host == want
    assert info["blocks_parsed_on_device"] == 0 and "sample columns" in info.get("device_parser_not_taken", ""), info


@pytest.mark.parametrize("n_lines", VC.SCAN)
def test_scan_line_counts_around_the_blocks_of_heads_and_the_stretches_of_the_scan(n_lines, tmp_path, monkeypatch):
    info = _all_on_the_device(VC.scan(n_lines), tmp_path, monkeypatch)
    assert info["blocks"] == 1, info
