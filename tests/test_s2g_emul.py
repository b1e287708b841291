"""The device route's functions (csrc/pg_s2g_core.h), walked on the host with 64 emulated lanes and emulated tiles by
tests/s2g_emul.cpp in the device's place inside the seqToGeno.py driver: line classification, the lines' places in the store, the
closed-form line start and the template fill.  Every golden of the unmodified reference through it, byte for byte, in one block and
in many, with several tile widths; 120 seeded random files against the host route; the line-start formula against a running sum for
every x up to 10^5 + 1 and against exact integers at 10^9 +- 1 and 10^18 - 1."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from s2g_common import GOLD  # noqa: E402,F401
from s2g_cases import CASES, DEVICE, HOST_BLOCKS, HOST_LOAD, golden, input_bytes, random_case  # noqa: E402

from genomics_general_amd import seqgeno  # noqa: E402

BY_NAME = {c[0]: c for c in CASES}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("s2g_emul") / "libs2g_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "s2g_emul.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pgs_emul_tile_seqs.restype = C.c_int
    L.pgs_emul_tile_seqs.argtypes = [C.c_int, C.c_int]
    L.pgs_emul_block.restype = C.c_int
    L.pgs_emul_block.argtypes = [C.c_char_p, C.c_int64, C.c_int, C.c_void_p, C.c_int64, C.c_void_p] + [C.POINTER(C.c_int64)] * 3
    L.pgs_emul_emit.restype = C.c_int
    L.pgs_emul_emit.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_char_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                C.c_void_p, C.c_int64, C.c_void_p, C.c_int64]
    L.pgs_emul_digit_sum_mismatch.restype = C.c_int64
    L.pgs_emul_digit_sum_mismatch.argtypes = [C.c_int64]
    L.pgs_emul_digit_sum.restype = C.c_uint64
    L.pgs_emul_digit_sum.argtypes = [C.c_uint64]
    L.pgs_emul_line_start.restype = C.c_uint64
    L.pgs_emul_line_start.argtypes = [C.c_uint64, C.c_uint64]
    return L


class _Stats:
    blocks = 0
    handed_back = 0
    ranges = 0


def _emul_device(L):
    vp = lambda a: C.c_void_p(a.ctypes.data)                               # noqa: E731

    class EmulDevice:
        """seqgeno._Device's interface over the emulator; the store is a host array that begins at a multiple of 16"""

        def __init__(self, device, hint):
            self.cap = 0
            self._room(max(hint, 1))

        def _room(self, need):
            if need + 64 <= self.cap:
                return
            raw = np.full(2 * need + 64 + 80, 0xcc, dtype=np.uint8)
            lead = (-raw.ctypes.data) % 16
            fresh = raw[lead:lead + 2 * need + 64]
            if self.cap:
                fresh[:self.cap] = self.store
            self.raw, self.store, self.cap = raw, fresh, len(fresh)

        def pinned(self):
            return None

        def submit(self, block):
            return bytes(block)

        def parse(self, ticket, base, is_open):
            self.base, self.is_open = base, is_open

        def collect(self, buf, rec, n_threads):
            _Stats.blocks += 1
            self._room(self.base + len(buf))
            heads = np.empty(3 * (buf.count(b"\n") + 1), dtype=np.int64)
            nr, nh, hl = C.c_int64(), C.c_int64(), C.c_int64()
            rc = L.pgs_emul_block(buf, len(buf), int(self.is_open), vp(self.store), self.base, vp(heads), C.byref(nr), C.byref(nh), C.byref(hl))
            assert rc >= 0 and self.base == rec.total
            if rc == 1:
                _Stats.handed_back += 1
                self.put(self.base, rec.host_block(buf, n_threads))
                return
            for a, k, before in heads[:3 * nh.value].reshape(-1, 3):
                rec.head(buf[int(a) + 1:int(a) + int(k)], rec.total + int(before))
            rec.total += nr.value
            assert (self.store[rec.total:rec.total + 16] == 0xcc).all()    # (nothing is stored behind the last residue)

        def put(self, off, arr):
            self._room(off + len(arr))
            self.store[off:off + len(arr)] = arr

        def get(self, n):
            return self.store[:n].copy()

        def plan(self, part, total, tile_seqs):
            self.part, self.total = part, total
            self.tq = L.pgs_emul_tile_seqs(part.n_haps, int(tile_seqs))
            self.name_off = np.concatenate([[0], np.cumsum([len(n) for n in part.names])]).astype(np.int64)
            self.offs = np.ascontiguousarray(np.concatenate(part.hap_off), dtype=np.int64)
            for (name, n, offs) in part.segs:
                assert all(0 <= o and o + n <= total for o in offs)
            return self.tq

        def emit(self, pieces, size, gz_rows):
            _Stats.ranges += 1
            part = self.part
            out = np.full(size + 32, 0xdd, dtype=np.uint8)
            seg = np.asarray([p[0] for p in pieces], dtype=np.int32)
            x0 = np.asarray([p[1] for p in pieces], dtype=np.int64)
            x1 = np.asarray([p[2] for p in pieces], dtype=np.int64)
            rc = L.pgs_emul_emit(vp(self.store), vp(part.tmpl), len(part.tmpl), part.n_haps, b"".join(part.names), vp(self.name_off), vp(self.offs),
                                 self.tq, vp(seg), vp(x0), vp(x1), len(pieces), vp(out), size)
            assert rc == 0
            assert (out[size:] == 0xdd).all()
            return out[:size]

        def stats(self):
            return _Stats.blocks, _Stats.handed_back, _Stats.ranges

        def close(self):
            pass

    return EmulDevice


def _main(data, argv, tmp_path, tag):
    """the output, or the exit status the driver ends with and what it wrote"""
    inp, out = str(tmp_path / (tag + ".in")), str(tmp_path / (tag + ".geno"))
    with open(inp, "wb") as f:
        f.write(data)
    if os.path.exists(out):
        os.remove(out)
    try:
        rc = seqgeno.main(list(argv) + ["-s", inp, "-g", out])
    except SystemExit as exc:
        rc = exc.code
    got = None
    if os.path.exists(out):
        with open(out, "rb") as f:
            got = f.read()
    return rc, got


@pytest.fixture
def on_emul(emul, monkeypatch):
    monkeypatch.setattr(seqgeno, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_S2G_DEVICE", "1")
    monkeypatch.setenv("PG_BGZF_DEVICE", "0")
    _Stats.blocks = _Stats.handed_back = _Stats.ranges = 0
    return _Stats


@pytest.mark.parametrize("name", [c[0] for c in CASES])
@pytest.mark.parametrize("block,tile", [(None, 0), (3000, 3), (900, 1)])
def test_device_functions_give_the_reference_bytes(name, block, tile, on_emul, tmp_path, monkeypatch):
    _, inp, argv, _ = BY_NAME[name]
    if block:
        monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    monkeypatch.setenv("PG_S2G_TILE_SEQS", str(tile))
    assert _main(input_bytes(inp), argv, tmp_path, "d") == (0, golden(name))
    assert on_emul.ranges >= 1
    if name in DEVICE:
        assert on_emul.blocks >= 1 and on_emul.handed_back == 0
    elif name in HOST_BLOCKS:
        assert on_emul.handed_back >= 1
    else:
        assert name in HOST_LOAD and on_emul.blocks == 0


@pytest.mark.parametrize("seed", range(120))
def test_device_functions_equal_the_host_route_on_random_files(seed, emul, tmp_path, monkeypatch):
    text, argv = random_case(seed + 500)
    monkeypatch.setenv("PG_S2G_DEVICE", "0")
    want = _main(text.encode("ascii"), argv, tmp_path, "h")
    assert want[0] in (0, 1, 2)
    monkeypatch.setattr(seqgeno, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_S2G_DEVICE", "1")
    monkeypatch.setenv("PG_STREAM_BYTES", str(300 + 97 * (seed % 13)))
    monkeypatch.setenv("PG_S2G_TILE_SEQS", str(seed % 4))
    _Stats.blocks = _Stats.handed_back = _Stats.ranges = 0
    assert _main(text.encode("ascii"), argv, tmp_path, "d") == want
    assert want[0] == 2 or _Stats.ranges >= 1 or want[1].count(b"\n") == 1


def test_line_start_is_the_running_sum(emul):
    assert emul.pgs_emul_digit_sum_mismatch(100001) == -1
    exact = lambda x: sum((min(x, 10 ** d - 1) - 10 ** (d - 1) + 1) * d for d in range(1, len(str(x)) + 1)) if x else 0   # noqa: E731
    for x in (0, 1, 9, 10, 10 ** 9 - 1, 10 ** 9, 10 ** 9 + 1, 10 ** 18 - 1):
        assert emul.pgs_emul_digit_sum(x) == exact(x) == seqgeno.digit_sum(x), x
    for x, fixed in ((10 ** 9 + 1, 807), (10 ** 9 - 1, 3), (12345, 40002)):
        assert emul.pgs_emul_line_start(x, fixed) == x * fixed + exact(x) == seqgeno.line_start(x, fixed)
