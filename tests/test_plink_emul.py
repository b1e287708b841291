"""The device route's functions (csrc/pg_ped_core.h), walked on the host with 64 emulated lanes and emulated tiles by
tests/plink_emul.cpp in the device's place inside the genoToPlink.py driver: its blocks, their matrices and their hand-backs as the
device gets them.  Every golden of the unmodified reference the device takes through it, byte for byte, in one block and in many; the
goldens with lines or cells the device does not take (their blocks handed back); 120 seeded random files against the host route; a
run whose shortest cell comes in the block behind one the device made."""
import ctypes as C
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from plink_cases import CASES, DEVICE, HOST_BLOCKS, HOST_WHOLE, command, fixture_path, golden, random_case  # noqa: E402

from genomics_general_amd import genoplink  # noqa: E402

BY_NAME = {c[0]: c for c in CASES}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("plink_emul") / "libplink_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "plink_emul.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pgp_emul_tile_seqs.restype = C.c_int
    L.pgp_emul_tile_seqs.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
    L.pgp_emul_block.restype = C.c_int
    L.pgp_emul_block.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64,
                                 C.c_void_p, C.c_void_p] + [C.POINTER(C.c_int64)] * 4
    return L


class _Stats:
    blocks = 0
    handed_back = 0
    sites = 0
    refused = 0


def _emul_device(L):
    vp = lambda a: C.c_void_p(a.ctypes.data)                               # noqa: E731

    class EmulDevice:
        """genoplink._Device's interface over the emulator"""

        def __init__(self, plan, device, sel_len, tile_seqs=0):
            self.plan = plan
            self.sel_len = np.ascontiguousarray(sel_len, dtype=np.int32)
            self.tq = L.pgp_emul_tile_seqs(C.c_void_p(C.addressof(plan.cfg)), vp(self.sel_len), int(tile_seqs))
            self.taken = self.tq > 0
            _Stats.refused += not self.taken
            self.w = 2 * genoplink.alleles(plan.cfg.fmt, self.sel_len)
            self.woff = np.cumsum(self.w) - self.w

        def tile_seqs(self):
            return self.tq

        def submit(self, text):
            buf = bytes(text)
            p = self.plan
            _Stats.blocks += 1
            lines = buf.count(b"\n")
            out_cap, map_cap = int(self.w.sum()) * (lines + 128), 2 * len(buf) + 8 * lines + 64
            out, mp = np.full(out_cap, 0xdd, dtype=np.uint8), np.empty(map_cap, dtype=np.uint8)
            run, start = np.empty(lines + 1, dtype=np.uint8), np.empty(lines + 1, dtype=np.int64)
            ns, ml, hl, pitch = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
            rc = L.pgp_emul_block(C.c_void_p(C.addressof(p.cfg)), vp(p.sel_col), vp(self.sel_len), self.tq, buf, len(buf), vp(out), out_cap,
                                  vp(mp), map_cap, vp(run), vp(start), C.byref(ns), C.byref(ml), C.byref(hl), C.byref(pitch))
            assert rc >= 0, rc
            if rc == 1:
                _Stats.handed_back += 1
                return (None, buf, lines)
            n = ns.value
            _Stats.sites += n
            # nothing is stored behind a sample's last site: the bytes up to the next sample's row keep their fill
            for q in range(len(self.w)):
                a, b = int(self.woff[q]) * pitch.value + n * int(self.w[q]), (int(self.woff[q]) + int(self.w[q])) * pitch.value
                assert (out[a:b] == 0xdd).all()
            blk = genoplink.matrix_block(self.sel_len, self.w, self.woff, pitch.value, out, mp[:ml.value].tobytes(), run[:n], start[:n],
                                         lambda a, k: buf[a:a + k])
            return (blk, None, lines)

        def collect(self, ticket):
            return ticket

        def pinned(self):
            return None

        def stats(self):
            return _Stats.blocks, _Stats.handed_back

        def close(self):
            pass

    return EmulDevice


@pytest.fixture
def on_emul(emul, monkeypatch):
    monkeypatch.setattr(genoplink, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_PED_DEVICE", "1")
    monkeypatch.setenv("PG_BGZF_DEVICE", "0")                 # (no device here)
    _Stats.blocks = _Stats.handed_back = _Stats.sites = 0
    return _Stats


def _main(inp, argv, tmp_path, tag):
    """the outputs, or the exit status the driver ends with"""
    args, outs = command(argv, inp, str(tmp_path), tag)
    for p in outs.values():
        if os.path.exists(p):
            os.remove(p)
    try:
        rc = genoplink.main(["-g", inp] + args)
    except SystemExit as exc:
        assert not any(os.path.exists(p) for p in outs.values())
        return exc.code
    assert rc == 0
    got = {}
    for k, p in outs.items():
        with open(p, "rb") as f:
            got[k] = f.read()
    return got


def _copy(fixture, tmp_path):
    inp = str(tmp_path / ("in.geno.gz" if fixture_path(fixture).endswith(".gz") else "in.geno"))
    shutil.copy(fixture_path(fixture), inp)
    return inp


@pytest.mark.parametrize("name", DEVICE)
@pytest.mark.parametrize("block,tile", [(None, 0), (9000, 3)])
def test_device_functions_give_the_reference_files(name, block, tile, on_emul, tmp_path, monkeypatch):
    _, fixture, argv = BY_NAME[name]
    if block:
        monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    monkeypatch.setenv("PG_PED_TILE_SEQS", str(tile))
    assert _main(_copy(fixture, tmp_path), argv + ["--device", "0"], tmp_path, "d") == golden(name)
    assert on_emul.blocks >= 1 and on_emul.handed_back == 0 and on_emul.sites >= 1
    assert genoplink.last_info["blocks_on_host"] == 1      # (the lines up to the first site)


@pytest.mark.parametrize("name", sorted(HOST_BLOCKS | HOST_WHOLE))
def test_goldens_with_lines_the_device_does_not_take_hand_their_blocks_back(name, on_emul, tmp_path, monkeypatch):
    _, fixture, argv = BY_NAME[name]
    monkeypatch.setenv("PG_STREAM_BYTES", "30")
    assert _main(_copy(fixture, tmp_path), argv + ["--device", "0"], tmp_path, "d") == golden(name)
    if name in HOST_WHOLE:
        assert on_emul.blocks == 0 and genoplink.last_info["blocks_on_host"] == genoplink.last_info["blocks"] >= 2
    else:
        assert on_emul.blocks >= on_emul.handed_back >= 1


@pytest.mark.parametrize("seed", range(120))
def test_device_functions_equal_the_host_route_on_random_files(seed, emul, tmp_path, monkeypatch):
    text, argv, dies = random_case(seed + 9000)
    inp = str(tmp_path / "r.geno")
    with open(inp, "w") as f:
        f.write(text)
    argv = argv + ["--prefix", "@P"]
    monkeypatch.setenv("PG_PED_DEVICE", "0")
    want = _main(inp, argv, tmp_path, "h")
    assert isinstance(want, int) == dies and want != 0
    monkeypatch.setattr(genoplink, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_PED_DEVICE", "1")
    monkeypatch.setenv("PG_STREAM_BYTES", str(1000 + 97 * (seed % 13)))
    monkeypatch.setenv("PG_PED_TILE_SEQS", str(seed % 4))
    _Stats.blocks = _Stats.handed_back = _Stats.sites = _Stats.refused = 0
    assert _main(inp, argv + ["--device", "0"], tmp_path, "d") == want
    assert _Stats.blocks >= 1 or dies or _Stats.refused == 1     # (refused: a first site with a cell the device does not take)


def test_a_short_cell_cuts_the_rows_of_the_device_blocks_before_it(on_emul, tmp_path, monkeypatch):
    """one scaffold, 300 diploid sites in blocks of some 40 lines; the haploid cell of sample b at site 250 hands its block back and
    cuts b's alleles in every block of the run, the device's included, to one a site"""
    rows = ["c\t%d\t%s\t%s\t%s" % (i + 1, "AC"[i % 2] + "|G", "T|" + "AC"[i % 2] if i != 250 else "G", "N|N") for i in range(300)]
    inp = str(tmp_path / "i.geno")
    with open(inp, "w") as f:
        f.write("#CHROM\tPOS\ta\tb\tc\n" + "\n".join(rows) + "\n")
    monkeypatch.setenv("PG_STREAM_BYTES", "600")
    got = _main(inp, ["--prefix", "@P", "--device", "0"], tmp_path, "d")
    info = dict(genoplink.last_info)
    ped = got["ped"].split(b"\n")
    assert ped[1] == b"0 b 0 0 0 0 " + b" ".join(b"T" if i != 250 else b"G" for i in range(300))
    assert ped[0] == b"0 a 0 0 0 0 " + b" ".join(b"AC"[i % 2:i % 2 + 1] + b" G" for i in range(300)) and ped[2] == b"0 c 0 0 0 0" + b" N N" * 300
    assert on_emul.handed_back == 1 and info["blocks_on_device"] >= 5 and info["blocks_on_host"] == 2 and info["runs"] == 1
    monkeypatch.setenv("PG_PED_DEVICE", "0")
    assert got == _main(inp, ["--prefix", "@P"], tmp_path, "h")
