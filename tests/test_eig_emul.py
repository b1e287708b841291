"""The device route's per-site / per-cell functions (csrc/pg_eig_core.h), walked on the host with 64 emulated lanes by
tests/eig_emul.cpp in the device's place inside the genoToEigenstrat.py driver: its blocks, their first site indices and their
hand-backs as the device gets them.  Every golden of the unmodified reference the device takes through it, byte for byte, in one block
and in many; the goldens with irregular lines (their blocks handed back); 120 seeded random files against the host route; a '#' line
in the middle moves the index of the block behind it."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from eig_cases import CASES, DEVICE, HOST_BLOCKS, OUTPUTS, fixture_path, golden, random_case  # noqa: E402

from genomics_general_amd import genoeig  # noqa: E402

BY_NAME = {c[0]: c for c in CASES}


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("eig_emul") / "libeig_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "eig_emul.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pge_emul_block.restype = C.c_int
    L.pge_emul_block.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_char_p, C.c_void_p, C.c_int64,
                                 C.c_char_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                 C.POINTER(C.c_int64)]
    return L


class _Stats:
    blocks = 0
    handed_back = 0


def _emul_device(L):
    class EmulDevice:
        """genoeig._Device's interface over the emulator"""

        def __init__(self, plan, device):
            self.plan = plan
            self.taken = 1 if plan.cfg.n_cols >= 3 and plan.cfg.n_sel >= 1 and not plan.cfg.cumulative else 0

        def submit(self, text, first_site):
            buf = bytes(text)
            p = self.plan
            _Stats.blocks += 1
            lines = buf.count(b"\n")
            cap = (lines + 1) * (40 + p.max_label) + 64
            geno, snp = np.empty((lines + 1) * (p.cfg.n_sel + 1), dtype=np.uint8), np.empty(cap, dtype=np.uint8)
            nr, sl, hl = C.c_int64(), C.c_int64(), C.c_int64()
            vp = lambda a: C.c_void_p(a.ctypes.data)                           # noqa: E731
            rc = L.pge_emul_block(C.c_void_p(C.addressof(p.cfg)), vp(p.sel_col), p.names, vp(p.name_off), vp(p.table), p.mask, p.labels,
                                  vp(p.label_off), first_site, buf, len(buf), vp(geno), vp(snp), cap, C.byref(nr), C.byref(sl), C.byref(hl))
            assert rc >= 0, rc
            if rc == 1:
                _Stats.handed_back += 1
                result = (None, None, buf, lines)
            else:
                result = (geno[:nr.value * (p.cfg.n_sel + 1)].tobytes(), snp[:sl.value].tobytes(), None, lines)
            return (result, buf), first_site, lines

        def collect(self, ticket, as_text=False):
            result, buf = ticket
            return (None, None, buf, result[3]) if as_text else result

        def pinned(self):
            return None

        def stats(self):
            return _Stats.blocks, _Stats.handed_back

        def close(self):
            pass

    return EmulDevice


@pytest.fixture
def on_emul(emul, monkeypatch):
    monkeypatch.setattr(genoeig, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_EIG_DEVICE", "1")
    monkeypatch.setenv("PG_BGZF_DEVICE", "0")                 # (no device here)
    _Stats.blocks = _Stats.handed_back = 0
    return _Stats


def _main(inp, argv, tmp_path, tag):
    outs = {k: str(tmp_path / ("%s.%s" % (tag, k))) for k in OUTPUTS}
    rc = genoeig.genoeig_main(["-g", inp, "--genoOutFile", outs["geno"], "--snpOutFile", outs["snp"], "--indOutFile", outs["ind"]]
                              + [a.replace("@G", GOLD) for a in argv])
    assert rc == 0
    got = {}
    for k, p in outs.items():
        with open(p, "rb") as f:
            got[k] = f.read()
    return got


@pytest.mark.parametrize("name", DEVICE)
@pytest.mark.parametrize("block", [None, 9000])
def test_device_functions_give_the_reference_rows(name, block, on_emul, tmp_path, monkeypatch):
    _, fixture, argv = BY_NAME[name]
    if block:
        monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    assert _main(fixture_path(fixture), argv + ["--device", "0"], tmp_path, "d") == golden(name)
    assert on_emul.blocks >= 1 and on_emul.handed_back == 0 and genoeig.last_info["blocks_redone_on_host"] == 0


@pytest.mark.parametrize("name", sorted(HOST_BLOCKS - {"header_only"}))
def test_goldens_with_irregular_lines_hand_their_blocks_back(name, on_emul, tmp_path, monkeypatch):
    _, fixture, argv = BY_NAME[name]
    monkeypatch.setenv("PG_STREAM_BYTES", "100")
    assert _main(fixture_path(fixture), argv + ["--device", "0"], tmp_path, "d") == golden(name)
    assert on_emul.blocks >= on_emul.handed_back >= 1


@pytest.mark.parametrize("seed", range(120))
def test_device_functions_equal_the_host_route_on_random_files(seed, emul, tmp_path, monkeypatch):
    text, argv, chrom = random_case(seed + 7000)
    argv = [a for a in argv if a != "--cumulativePos"]
    inp = str(tmp_path / "r.geno")
    with open(inp, "w") as f:
        f.write(text)
    if chrom is not None:
        with open(str(tmp_path / "chrom.txt"), "w") as f:
            f.write(chrom)
        argv = argv + ["--chromFile", str(tmp_path / "chrom.txt")]
    monkeypatch.setenv("PG_EIG_DEVICE", "0")
    want = _main(inp, argv, tmp_path, "h")
    monkeypatch.setattr(genoeig, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_EIG_DEVICE", "1")
    monkeypatch.setenv("PG_STREAM_BYTES", str(1000 + 97 * (seed % 13)))
    _Stats.blocks = _Stats.handed_back = 0
    assert _main(inp, argv + ["--device", "0"], tmp_path, "d") == want
    assert want["snp"].count(b"\n") >= 1 and _Stats.blocks >= 1 and _Stats.handed_back == 0


def test_a_hash_line_moves_the_index_of_the_block_behind_it(on_emul, tmp_path, monkeypatch):
    text, argv, _ = random_case(7077)
    argv = [a for a in argv if a != "--cumulativePos"]
    rows = text.split("\n")
    rows[12:12] = ["# no site"]
    inp = str(tmp_path / "i.geno")
    with open(inp, "w") as f:
        f.write("\n".join(rows))
    monkeypatch.setenv("PG_STREAM_BYTES", "600")
    got = _main(inp, argv + ["--device", "0"], tmp_path, "d")
    info = dict(genoeig.last_info)
    monkeypatch.setenv("PG_EIG_DEVICE", "0")
    assert got == _main(inp, argv, tmp_path, "h")
    assert on_emul.handed_back == 1 and info["blocks_redone_on_host"] == 1 and info["blocks_on_device"] >= 2
