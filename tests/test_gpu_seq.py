"""The genoToSeq.py drop-in's device route (pg_seq_dev_*: k_seq_lines, k_seq_tile) on an MI355X: every golden of the unmodified
reference byte for byte (some from BGZF input whose members are inflated on the device, some in blocks that windows span) with no block
handed back; the kernels against NumPy on seeded random text over the tile edges, the pad columns untouched; a block with an irregular
line goes to the host route; positions across 2^31."""
import os

import numpy as np
import pytest

from seq_common import CASE_IDS, SEQ_CASES, fixture_text, golden, random_geno, run_case, run_main
from test_seq_emul import _regular, numpy_matrix, plan_for, selection

from genomics_general_amd import genoio, genoseq

pytestmark = pytest.mark.gpu

# members of 5000 bytes of text under PG_STREAM_BYTES=20000 (genoio.BgzfFile.read_span hands out 64 KiB of text at least: fixtures of
# several blocks of that size)
BGZF = ("abba_coord_split_phylip", "c1_cat_split_phylip")
SMALL = ("haplo_sites_maxdist_minsites", "mixed_coord_split")                  # blocks of 3000 bytes


@pytest.fixture(autouse=True)
def _device_route(monkeypatch):
    monkeypatch.setenv("PG_SEQ_DEVICE", "1")


@pytest.mark.parametrize("case", SEQ_CASES, ids=CASE_IDS)
def test_seq_device_reproduces_the_reference(case, tmp_path, monkeypatch):
    geno = None
    if case["name"] in BGZF:
        geno = str(tmp_path / "in.geno.gz")
        with open(geno, "wb") as f:
            f.write(genoio.bgzf_compress(fixture_text(case["fixture"]), block=5000))
        monkeypatch.setenv("PG_STREAM_BYTES", "20000")
    elif case["name"] in SMALL:
        monkeypatch.setenv("PG_STREAM_BYTES", "3000")
    assert run_case(case, tmp_path, geno=geno) == golden(case["name"])
    info = genoseq.last_info
    assert info["blocks"] >= 1 and info["device_blocks"] + info["device_host_blocks"] >= info["blocks"]
    if case["name"] in BGZF:
        assert info["blocks_inflated_on_device"] == info["blocks"] > 1
    if case["name"] in SMALL:
        assert info["blocks"] > 10
    if _regular(case):
        assert info["device_host_blocks"] == 0 and info["blocks_on_device"] == info["blocks"]
    else:                       # cells of several characters copied whole are the host route's by rule (k_seq_lines takes one character)
        assert info["device_host_blocks"] == info["blocks"]


@pytest.fixture(scope="module")
def device():
    class A:
        splitPhased, ploidy, NtoGap = True, [2], False
    d = genoseq.Device(genoseq.Plan("#CHROM\tPOS\ts0\n", A, None), 0)
    yield d
    d.close()


LINES = (1, 127, 128, 129, 257)


@pytest.mark.parametrize("n_seq", [1, 63, 64, 65, 130])
@pytest.mark.parametrize("kind", ["identity", "reversed", "repeated"])
def test_seq_kernels_equal_numpy(device, n_seq, kind):
    for n_kept in LINES:
        seed = n_seq * 1000 + n_kept
        rng = np.random.default_rng(seed)
        ploidies = [int(p) for p in rng.integers(1, 4, size=n_seq)]
        comments = (0, n_kept // 2 + 1, n_kept + 2) if n_kept > 1 else (0, 2)
        header, text, sites = random_geno(seed, n_kept + len(comments), ploidies, comments=comments)
        sel = selection(kind, ploidies, n_seq, rng)
        for n_to_gap, tile_seqs in ((False, 0), (True, 64)):
            device.configure(plan_for(header, ploidies, sel, n_to_gap), tile_seqs)
            assert device.taken
            chunk, pos, starts, names, text_back, n_lines = device.collect(device.submit(text.encode()), padded=True)
            assert chunk is not None and chunk.n == n_kept and n_lines == n_kept + len(comments)
            assert chunk.mat.shape[1] % 128 == 0
            assert np.array_equal(chunk.mat[:, :n_kept], numpy_matrix(sites, sel, True, n_to_gap))
            assert not chunk.mat[:, n_kept:].any()                                    # the pad columns are as the memset left them
            assert [int(p) for p in pos] == [p for _, p, _ in sites]
            run_rows = [k for k in range(n_kept) if k == 0 or sites[k][0] != sites[k - 1][0]]
            assert [int(a) for a in starts] == run_rows and names == [sites[k][0] for k in run_rows]


def test_seq_positions_across_2_31(device):
    ploidies = [2, 2, 1]
    header, text, sites = random_geno(5, 200, ploidies, base_pos=2 ** 31 - 300)
    assert sites[0][1] < 2 ** 31 < max(p for _, p, _ in sites)
    sel = [(0, 0), (0, 2), (1, 0), (1, 2), (2, 0)]
    device.configure(plan_for(header, ploidies, sel, False), 0)
    chunk, pos, starts, names, _, _ = device.collect(device.submit(text.encode()))
    assert pos.dtype == np.int64 and [int(p) for p in pos] == [p for _, p, _ in sites]
    assert np.array_equal(chunk.mat, numpy_matrix(sites, sel, True, False))


def test_seq_irregular_line_goes_to_the_host_route(device, tmp_path, monkeypatch):
    ploidies = [2, 1, 3, 2, 2]
    header, text, sites = random_geno(91, 300, ploidies, irregular=120)
    sel = [(c, 2 * h) for c, p in enumerate(ploidies) for h in range(p)]
    device.configure(plan_for(header, ploidies, sel, False), 0)
    chunk, _, _, _, text_back, line = device.collect(device.submit(text.encode()))
    assert chunk is None and line == 120 and text_back == text.encode()
    inp = str(tmp_path / "i.geno")
    with open(inp, "w") as f:
        f.write(header + text)
    argv = ["-g", inp, "--splitPhased", "--ploidy"] + [str(p) for p in ploidies] + ["-f", "phylip"]
    rc, dev_out, err = run_main(argv)
    assert rc == 0, err
    assert genoseq.last_info["device_blocks"] == 1 and genoseq.last_info["device_host_blocks"] == 1 and genoseq.last_info["blocks_on_host"] == 1
    monkeypatch.setenv("PG_SEQ_DEVICE", "0")
    rc, host_out, err = run_main(argv)
    assert rc == 0 and dev_out == host_out
    assert [ln.split(b"   ")[1] for ln in host_out.splitlines()[1:]] == [bytes(r) for r in numpy_matrix(sites, sel, True, False)]


@pytest.mark.parametrize("final_newline", [False, True])
def test_seq_bgzf_input_whose_last_line_has_no_line_feed(final_newline, device, tmp_path, monkeypatch):
    """four data lines in two BGZF members (the header and two lines, then two lines), the last line without its line feed: through the
    device route with the members inflated on the device, the output is the host route's byte for byte and the unfinished line's block
    is the host's; with the line feed restored no block is.  Then the same lines as ONE block of members handed to the device as it
    is: whether it ends in a line feed is read on the device once its line feeds are counted (pg_line_slot.h's tail_unknown), and
    without one the block comes back as the host's, its text with it"""
    ploidies = [2, 2, 1]
    header, text, sites = random_geno(17, 4, ploidies)
    lines = text.splitlines(keepends=True)
    whole = (header + text).encode()
    if not final_newline:
        whole = whole[:-1]
    inp = str(tmp_path / "in.geno.gz")
    bz = genoio.bgzf_compress(whole, block=len(header + lines[0] + lines[1]))
    assert len(genoio.bgzf_walk(bz)[0][0]) == 3                   # (two members of text, bgzip's empty last)
    with open(inp, "wb") as f:
        f.write(bz)
    argv = ["-g", inp, "--splitPhased", "--ploidy"] + [str(p) for p in ploidies] + ["-f", "fasta"]
    rc, dev_out, err = run_main(argv)
    assert rc == 0, err
    info = dict(genoseq.last_info)
    monkeypatch.setenv("PG_SEQ_DEVICE", "0")
    rc, host_out, err = run_main(argv)
    assert rc == 0 and dev_out == host_out and len(host_out) > 0
    assert info["blocks_inflated_on_device"] >= 1 and info["device_blocks"] >= 1, info
    if final_newline:
        assert info["device_host_blocks"] == 0, info
    else:
        assert info["device_host_blocks"] >= 1, info
    # one block of members, as genoio.BgzfFile.read_span would hand it out if it did not cut behind the last line feed
    body = whole[len(header):]
    bz = genoio.bgzf_compress(body, block=(len(body) + 1) // 2)
    tab, used, n_text = genoio.bgzf_walk(bz)
    assert n_text == len(body) and len(tab[0]) == 3
    comp = np.frombuffer(bz, dtype=np.uint8)[:used]
    sel = [(c, 2 * h) for c, p in enumerate(ploidies) for h in range(p)]
    device.configure(plan_for(header, ploidies, sel, False), 0)
    before = device.stats()[1]
    chunk, pos, _, _, text_back, line = device.collect(device.submit(genoio.BgzfSpan(b"", comp, tab, n_text, lines[0].encode()[:-1])))
    if final_newline:
        assert chunk is not None and np.array_equal(chunk.mat, numpy_matrix(sites, sel, True, False)) and device.stats()[1] == before
        assert [int(p) for p in pos] == [p for _, p, _ in sites]
    else:
        assert chunk is None and line == 0 and text_back == body and device.stats()[1] == before + 1
