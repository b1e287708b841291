"""The device route's per-site / per-cell functions (csrc/pg_gvcf_core.h), walked on the host by tests/gvcf_emul.cpp in the device's
place inside the genoToVCF.py driver: its blocks and hand-backs as the device gets them.  Every golden of the unmodified reference
through it, byte for byte, in one block and in many; 200 seeded random files (with a random fasta) against the host route; a block with
one irregular line ends in the host route's rows."""
import ctypes as C
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from gvcf_cases import CASES, fixture_path, random_case  # noqa: E402

from genomics_general_amd import genovcf  # noqa: E402


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("gvcf_emul") / "libgvcf_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "gvcf_emul.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pgg_emul_block.restype = C.c_int
    L.pgg_emul_block.argtypes = [C.c_void_p, C.c_void_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int32,
                                 C.c_void_p, C.c_char_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    return L


class _Stats:
    blocks = 0
    handed_back = 0


def _emul_device(L):
    class EmulDevice:
        """genovcf._Device's interface over the emulator"""

        def __init__(self, plan, device, gz_rows=False):
            self.plan = plan
            self.taken = 1 if plan.cfg.n_cols >= 3 and plan.cfg.n_sel >= 1 else 0

        def submit(self, text):
            buf = bytes(text)
            _Stats.blocks += 1
            cap = 3 * len(buf) + 40 * (buf.count(b"\n") + 1) + 64
            out = np.empty(cap, dtype=np.uint8)
            n, hl = C.c_int64(), C.c_int64()
            rc = L.pgg_emul_block(C.c_void_p(C.addressof(self.plan.cfg)), C.c_void_p(self.plan.sel_col.ctypes.data), *self.plan.ref_args(), buf,
                                  len(buf), out.ctypes.data_as(C.c_void_p), cap, C.byref(n), C.byref(hl))
            assert rc >= 0, rc
            lines = buf.count(b"\n")
            if rc == 1:
                _Stats.handed_back += 1
                return None, None, buf, lines
            return out[:n.value].tobytes(), None, None, lines

        def collect(self, ticket):
            return ticket

        def stats(self):
            return _Stats.blocks, _Stats.handed_back

        def close(self):
            pass

    return EmulDevice


@pytest.fixture
def on_emul(emul, monkeypatch):
    monkeypatch.setattr(genovcf, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_GVCF_DEVICE", "1")
    monkeypatch.setenv("PG_BGZF_DEVICE", "0")                 # (no device here)
    _Stats.blocks = _Stats.handed_back = 0
    return _Stats


def _golden(name):
    with gzip.open(os.path.join(GOLD, "gvcf", name + ".out.gz"), "rb") as f:
        return f.read()


@pytest.mark.parametrize("name,fixture,argv", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("block", [None, 9000])
def test_device_functions_give_the_reference_rows(name, fixture, argv, block, on_emul, tmp_path, monkeypatch):
    if block:
        monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    out = str(tmp_path / "o.vcf")
    assert genovcf.genovcf_main(["-g", fixture_path(fixture), "-o", out, "--device", "0"] + [a.replace("@G", GOLD) for a in argv]) == 0
    with open(out, "rb") as f:
        assert f.read() == _golden(name)
    assert on_emul.blocks >= 1 and on_emul.handed_back == 0


@pytest.mark.parametrize("seed", range(200))
def test_device_functions_equal_the_host_route_on_random_files(seed, emul, tmp_path, monkeypatch):
    text, argv, fasta = random_case(seed + 5000)
    inp = str(tmp_path / "r.geno")
    with open(inp, "w") as f:
        f.write(text)
    if fasta is not None:
        with open(str(tmp_path / "r.fa"), "w") as f:
            f.write(fasta)
        argv = argv + ["-r", str(tmp_path / "r.fa")]
    monkeypatch.setenv("PG_GVCF_DEVICE", "0")
    assert genovcf.genovcf_main(["-g", inp, "-o", str(tmp_path / "h.vcf")] + argv) == 0
    monkeypatch.setattr(genovcf, "_Device", _emul_device(emul))
    monkeypatch.setenv("PG_GVCF_DEVICE", "1")
    monkeypatch.setenv("PG_STREAM_BYTES", str(1000 + 97 * (seed % 13)))
    _Stats.blocks = _Stats.handed_back = 0
    assert genovcf.genovcf_main(["-g", inp, "-o", str(tmp_path / "d.vcf"), "--device", "0"] + argv) == 0
    with open(str(tmp_path / "h.vcf"), "rb") as f, open(str(tmp_path / "d.vcf"), "rb") as g:
        want = f.read()
        assert g.read() == want and want.count(b"\n") > 10
    assert _Stats.blocks >= 1 and _Stats.handed_back == 0


@pytest.mark.parametrize("what,old,new", [("spaces", "\t", "  "), ("empty field", "\t", "\t\t"), ("signed position", "\t", "\t+")])
def test_irregular_line_is_handed_to_the_host_route(what, old, new, on_emul, tmp_path, monkeypatch):
    text, argv, _ = random_case(77)
    rows = text.split("\n")
    rows[12] = rows[12].replace(old, new, 1)
    inp = str(tmp_path / "i.geno")
    with open(inp, "w", newline="") as f:
        f.write("\n".join(rows))
    monkeypatch.setenv("PG_STREAM_BYTES", "600")
    assert genovcf.genovcf_main(["-g", inp, "-o", str(tmp_path / "d.vcf"), "--device", "0"] + argv) == 0
    handed, blocks = on_emul.handed_back, on_emul.blocks
    monkeypatch.setenv("PG_GVCF_DEVICE", "0")
    assert genovcf.genovcf_main(["-g", inp, "-o", str(tmp_path / "h.vcf")] + argv) == 0
    with open(str(tmp_path / "h.vcf"), "rb") as f, open(str(tmp_path / "d.vcf"), "rb") as g:
        assert g.read() == f.read()
    assert handed == 1 and blocks > 2
