"""The device route's per-line functions and the kernels' arithmetic (csrc/pg_merge_core.h), walked on the host by tests/merge_emul.cpp
in the device's place inside the mergeGeno.py driver: its regions, rounds and hand-backs as the device gets them.  Every golden of the
unmodified reference through it, byte for byte, in one round and in many; no round handed back for the regular cases; random files
against the plain-Python model."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from merge_common import CASE_IDS, MERGE_CASES, ROOT, dense_files, golden, many_rounds_stream, random_files, run_case, run_main

import merge_model
from genomics_general_amd import _lib, mergegeno


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("merge_emul") / "libmerge_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-shared", "-fPIC", os.path.join(ROOT, "tests", "merge_emul.cpp"), "-o", so])
    L = C.CDLL(so)
    L.pgm_emul_config.restype = C.c_void_p
    L.pgm_emul_config.argtypes = [C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgm_emul_free.argtypes = [C.c_void_p]
    L.pgm_emul_submit.argtypes = [C.c_void_p, C.c_int, C.c_char_p, C.c_int64]
    L.pgm_emul_keys.argtypes = [C.c_void_p, C.c_void_p]
    L.pgm_emul_merge.argtypes = [C.c_void_p, C.c_int, C.c_int32, C.c_int64, C.c_int32, C.c_int64, C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    L.pgm_emul_rows.argtypes = [C.c_void_p, C.c_void_p]
    L.pgm_emul_advance.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pgm_emul_text.restype = C.c_int64
    L.pgm_emul_text.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
    return L


class _Stats:
    devices = 0
    not_taken = 0


def _emul_device(E):
    class EmulDevice:
        """mergegeno.Device's interface over the emulator"""

        def __init__(self, cfg, sep, missing, fai, n_cols, device, gz_rows=False):
            self.L = _lib.lib()                                # (pg_merge_plan: plain host code)
            self.nf = cfg.n_files
            self.n_cols = np.ascontiguousarray(n_cols, dtype=np.int32)
            self.h = E.pgm_emul_config(C.addressof(cfg), sep, missing, fai.blob, fai.name_off.ctypes.data, fai.lens.ctypes.data, self.n_cols.ctypes.data)
            self.taken = bool(self.h)
            self.gz_rows = False
            _Stats.devices += 1
            _Stats.not_taken += not self.taken

        def submit(self, f, block):
            block = bytes(block)
            assert E.pgm_emul_submit(self.h, f, block, len(block)) == 0

        def keys(self):
            info = np.zeros((self.nf, 8), dtype=np.int64)
            assert E.pgm_emul_keys(self.h, info.ctypes.data) == 0
            return info

        def merge(self, dense, frm, hor):
            done = np.zeros((self.nf, 4), dtype=np.int64)
            nb, nr = C.c_int64(), C.c_int64()
            rc = E.pgm_emul_merge(self.h, int(dense), frm[0], frm[1], hor[0], hor[1], done.ctypes.data, C.byref(nb), C.byref(nr))
            assert rc == 0, rc
            out = np.empty(max(nb.value, 1), dtype=np.uint8)[:nb.value]
            E.pgm_emul_rows(self.h, out.ctypes.data)
            return out.tobytes(), None, nr.value, done

        def advance(self, done, prevs):
            ps = np.ascontiguousarray([p[0] for p in prevs], dtype=np.int32)
            pp = np.ascontiguousarray([p[1] for p in prevs], dtype=np.int64)
            done = np.ascontiguousarray(done, dtype=np.int64)
            assert E.pgm_emul_advance(self.h, done.ctypes.data, ps.ctypes.data, pp.ctypes.data) == 0

        def text(self, f, n):
            assert E.pgm_emul_text(self.h, f, None) == n
            out = np.empty(max(n, 1), dtype=np.uint8)[:n]
            E.pgm_emul_text(self.h, f, out.ctypes.data)
            return out.tobytes()

        def pinned(self):
            return None

        def stats(self):
            return 0, 0.0, 0.0, 0.0

        def close(self):
            if self.h:
                E.pgm_emul_free(self.h)
                self.h = None

    return EmulDevice


@pytest.fixture
def on_emul(emul, monkeypatch):
    monkeypatch.setattr(mergegeno, "Device", _emul_device(emul))
    monkeypatch.setenv("PG_MERGE_DEVICE", "1")
    monkeypatch.setenv("PG_BGZF_DEVICE", "0")                 # (no device here: the inputs are inflated by the host)
    _Stats.devices = _Stats.not_taken = 0
    return _Stats


@pytest.mark.parametrize("case", MERGE_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("stream", [None, "small"])
def test_device_functions_give_the_reference_bytes(case, stream, on_emul, tmp_path, monkeypatch):
    if stream:
        monkeypatch.setenv("PG_STREAM_BYTES", str(many_rounds_stream(case)))
    out, _ = run_case(case, tmp_path)
    assert out == golden(case["name"])
    info = mergegeno.last_info
    assert on_emul.devices == 1 and info["rounds"] >= 1
    if case.get("host"):
        assert info["rounds_on_host"] >= 1
    else:
        assert info["rounds_on_host"] == 0 and on_emul.not_taken == 0 and info["rounds_on_device"] == info["rounds"]
    if stream:
        assert info["rounds"] > 10


@pytest.mark.parametrize("seed,kind", [(1, "zero"), (2, "range"), (3, "scaffold"), (4, "repeat"), (5, "back"), (6, "plus"), (7, None), (8, None)])
@pytest.mark.parametrize("method", ["intersect", "union", "all"])
def test_device_functions_equal_the_model_on_random_files(seed, kind, method, on_emul, tmp_path, monkeypatch):
    paths, fai = random_files(seed, 150, 3, str(tmp_path), scaffolds=3, n_fai=5, stop=(seed % 3, kind) if kind else None, bare_file=seed % 4,
                              long_tails=((0, 70), (1, 300)))
    argv = sum([["-i", p] for p in paths], []) + ["-f", fai, "--method", method]
    monkeypatch.setenv("PG_STREAM_BYTES", "900")
    rc, out, err = run_main(argv)
    assert rc == 0, err
    assert out == merge_model.merge_argv(argv)
    assert mergegeno.last_info["rounds_on_host"] == 0 and mergegeno.last_info["rounds"] >= 3
    assert mergegeno.last_info["stopped_files"] == (1 if kind else 0)


def test_a_dense_method_over_files_beyond_the_stream_size_takes_few_rounds(on_emul, tmp_path, monkeypatch):
    argv, stream, bound = dense_files(str(tmp_path))
    monkeypatch.setenv("PG_STREAM_BYTES", str(stream))
    rc, out, err = run_main(argv)
    assert rc == 0, err
    assert out == merge_model.merge_argv(argv)
    info = mergegeno.last_info
    assert info["blocks"] >= 6 and info["rounds_on_host"] == 0
    assert info["rounds"] <= bound(info["blocks"]), info


def test_a_round_with_an_irregular_line_is_the_host_routes(on_emul, tmp_path, monkeypatch):
    case = [c for c in MERGE_CASES if c["name"] == "spaced_union"][0]
    monkeypatch.setenv("PG_STREAM_BYTES", "300")
    dev_out, _ = run_case(case, tmp_path / "a")
    info = dict(mergegeno.last_info)
    assert info["rounds_on_host"] >= 1 and info["rounds_on_device"] >= 1            # (both routes took rounds of this run)
    monkeypatch.setenv("PG_MERGE_DEVICE", "0")
    host_out, _ = run_case(case, tmp_path / "b")
    assert dev_out == host_out == golden(case["name"])
