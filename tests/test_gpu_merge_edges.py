"""k_merge_keys and k_merge_emit (csrc/pg_merge_dev.hip) where their 64-byte steps and the probes of the .fai table turn over, with
k_merge_stop / k_merge_lines / k_merge_pos / k_rows_scan at their block and stretch sizes: the files of tests/merge_edge_cases.py
through mergeGeno's device route, byte for byte against the plain-Python model (tests/merge_model.py).  tests/merge_emul.cpp restates
the kernels serially, byte by byte, so the CPU suite sees no fault in how a wave divides a line; tests/test_merge_edge_cases.py shows
on the CPU that the emulated device takes every regular case whole -- so here no round may go to the host, where a fault in the keys
would otherwise hide (a round handed back costs only speed and changes no byte).

What a red case stands on:

NAMES   k_merge_keys: the first tab at byte 1, 62 .. 65, 127 .. 129 (`t0` found in the first, second, third step), the second tab a
        step behind the first (`ntab == 1`) and both in a later step (`m2` there); the hash sum and the name compare
        (`k += 64`) for two and three trips, against a second name of the same length that differs in its last byte.  k_merge_emit:
        the head copy (`k < hl`) and the .fai name (`k < nn`) beyond one trip, under all three methods
TWINS   the probe `at = (at + 1) & F.mask`: past an entry of the same length that differs in a byte of the second trip (a) or in byte
        0 (b), from the last slot to slot 0 (c), onto an empty slot behind an entry of the same length (d: PGM_STOP_SCAF, the file
        stops there)
WIDTH   tab counts summed over 1, 2, 3 and 4 steps (32 .. 92 fields), tabs on both sides of every seam, lines of 63 .. 193 bytes
        (`in = k < n` in a step's last, first and second lane); a file whose head is its whole line
SEAMS   `before = line[k - 1]` read by lane 0 of a later step (a double tab across bytes 63|64 and 127|128), `k == n - 1` in a step's
        last and first lane (a trailing tab), a blank in a step's last and first lane: the round goes to the host and the bytes are
        the host route's; the regular twin, one byte apart, stays on the device
DUMMY   the dummy run `k % per` beyond one trip and with per = 1, 2, 4, 22, 64, 65, at an output offset off the 64-byte grid; --missing
        of 65 bytes is not the device's
CELLS   a file's cells copied at an output offset `w` the parts in front left anywhere, for 63 .. 300 bytes, every tab turned into a comma
DIGITS  positions rendered with 1 to 6 digits, the count changing inside a round and with a round's last position
LINES   1 .. 1025 lines a file: the 4 lines a block of k_merge_keys / k_merge_emit, the 256 threads of k_merge_stop / k_merge_lines,
        k_rows_scan's stretch of 1 and 2 slots a thread
Every second case of NAMES, WIDTH, CELLS and DUMMY runs once more with three of its longest lines a file and round: the seams of the
rounds (take_block's remainder copy, k_merge_nl's shift) between wide lines."""
import pytest

import merge_edge_cases as MC
from merge_common import run_main

from genomics_general_amd import mergegeno

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _device_route(monkeypatch):
    monkeypatch.setenv("PG_MERGE_DEVICE", "1")


@pytest.fixture(scope="module")
def store(tmp_path_factory):
    return MC.Store(tmp_path_factory.mktemp("merge_edges"))


def _difference(got, want):
    k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    return "first difference in line %d, at byte %d of %d / %d: %r != %r" % (want.count(b"\n", 0, k), k, len(got), len(want),
                                                                            got[max(k - 40, 0):k + 40], want[max(k - 40, 0):k + 40])


def _run(argv, monkeypatch, stream, device="1"):
    monkeypatch.setenv("PG_MERGE_DEVICE", device)
    if stream:
        monkeypatch.setenv("PG_STREAM_BYTES", str(stream))
    rc, out, err = run_main(argv)
    assert rc == 0, err
    return out, dict(mergegeno.last_info)


def _whole_on_the_device(name, store, monkeypatch, stream):
    argv, facts, want = store.get(name)
    out, info = _run(argv, monkeypatch, stream)
    assert out == want, _difference(out, want)
    assert info["rounds_on_host"] == 0 and info["rounds_on_device"] == info["rounds"] >= 1, info
    assert info["stopped_files"] == facts["stopped_files"], info
    assert info["rounds"] >= facts.get("rounds_at_least", 1), info
    return info


def _regular(cases):
    return [n for n, _ in cases if not n.endswith("defect") and n != MC.MISSING_TOO_LONG]


@pytest.mark.parametrize("name", _regular(MC.NAMES))
def test_names_tabs_around_the_64_byte_steps(name, store, monkeypatch):
    _whole_on_the_device(name, store, monkeypatch, None)


@pytest.mark.parametrize("name", _regular(MC.TWINS))
def test_twins_probe_chains_of_the_fai_table(name, store, monkeypatch):
    _whole_on_the_device(name, store, monkeypatch, None)


@pytest.mark.parametrize("name", _regular(MC.WIDTH))
def test_width_lines_and_tab_counts_of_one_to_four_steps(name, store, monkeypatch):
    _whole_on_the_device(name, store, monkeypatch, None)


@pytest.mark.parametrize("name", _regular(MC.DUMMY))
def test_dummy_runs_around_64_bytes_off_the_grid(name, store, monkeypatch):
    _whole_on_the_device(name, store, monkeypatch, None)


@pytest.mark.parametrize("name", _regular(MC.CELLS))
def test_cells_parts_of_63_to_300_bytes_in_every_file_position(name, store, monkeypatch):
    _whole_on_the_device(name, store, monkeypatch, None)


@pytest.mark.parametrize("name", _regular(MC.DIGITS))
def test_digits_positions_of_one_to_six_digits(name, store, monkeypatch):
    _whole_on_the_device(name, store, monkeypatch, store.get(name)[1]["stream"])


@pytest.mark.parametrize("name", _regular(MC.LINES))
def test_lines_counts_around_the_blocks_and_the_scans_stretches(name, store, monkeypatch):
    info = _whole_on_the_device(name, store, monkeypatch, None)
    assert info["rounds"] == 1, info


@pytest.mark.parametrize("name", [n for _, n, _ in MC.streamed()])
def test_a_few_wide_lines_a_file_and_round(name, store, monkeypatch):
    info = _whole_on_the_device(name, store, monkeypatch, store.get(name)[1]["few_lines_stream"])
    assert info["rounds"] > 3, info


@pytest.mark.parametrize("name", [n for n, _ in MC.SEAMS if n.endswith("defect")])
def test_seams_a_defect_on_a_seam_hands_its_round_to_the_host(name, store, monkeypatch):
    argv, facts, want = store.get(name)
    out, info = _run(argv, monkeypatch, facts["stream"])
    assert out == want, _difference(out, want)
    assert info["rounds_on_host"] >= 1 and info["rounds_on_device"] >= 1, info
    host, _ = _run(argv, monkeypatch, facts["stream"], device="0")
    assert out == host, _difference(out, host)


@pytest.mark.parametrize("name", [n for n, _ in MC.SEAMS if n.endswith("twin")])
def test_seams_the_regular_twin_stays_on_the_device(name, store, monkeypatch):
    info = _whole_on_the_device(name, store, monkeypatch, store.get(name)[1]["stream"])
    assert info["rounds"] > 3, info


def test_a_missing_of_65_bytes_is_not_the_devices(store, monkeypatch):
    argv, facts, want = store.get(MC.MISSING_TOO_LONG)
    out, info = _run(argv, monkeypatch, None)
    assert out == want, _difference(out, want)
    assert info["rounds_on_device"] == 0 and info["rounds"] >= 1, info
