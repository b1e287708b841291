"""The mergeGeno.py drop-in's host route (genomics_general_amd/mergegeno.py + pg_merge_text) and the plain-Python model
(tests/merge_model.py) against the outputs of the UNMODIFIED reference mergeGeno.py (tests/golden/make_golden_merge.py): byte for byte,
in one round and in many; the rejected inputs; a stopped file's warning; the planning of the rounds (csrc/pg_merge_plan.h) under a
sanitizer, as a program of its own."""
import gzip
import os
import subprocess
import sys

import pytest

from merge_common import CASE_IDS, MERGE, MERGE_CASES, ROOT, case_argv, dense_files, golden, many_rounds_stream, random_files, run_case, run_main

import merge_model
from genomics_general_amd import mergegeno


@pytest.fixture(autouse=True)
def host_route(monkeypatch):
    monkeypatch.setenv("PG_MERGE_DEVICE", "0")


@pytest.mark.parametrize("case", MERGE_CASES, ids=CASE_IDS)
def test_model_equals_the_reference(case):
    assert merge_model.merge_argv(case_argv(case)) == golden(case["name"])


@pytest.mark.parametrize("case", MERGE_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("stream", [None, "small"])
def test_host_route_equals_the_reference(case, stream, tmp_path, monkeypatch):
    if stream:
        monkeypatch.setenv("PG_STREAM_BYTES", str(many_rounds_stream(case)))
    out, _ = run_case(case, tmp_path)
    assert out == golden(case["name"])
    info = mergegeno.last_info
    assert info["rounds_on_host"] == info["rounds"] >= 1 and info["rounds_on_device"] == 0
    assert info["lines_written"] == golden(case["name"]).count(b"\n") - 1
    if stream:
        assert info["rounds"] > 10


def test_the_script_runs_as_a_program(tmp_path):
    case = MERGE_CASES[0]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "mergeGeno.py")] + case_argv(case), stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       env=dict(os.environ, PG_MERGE_DEVICE="0"))
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == golden(case["name"])


def test_gz_output_is_gzip(tmp_path):
    case = [c for c in MERGE_CASES if c["out"] == "gz"][0]
    out, _ = run_case(case, tmp_path)
    with open(str(tmp_path / "o" / "out.gz"), "rb") as f:
        assert gzip.decompress(f.read()) == out == golden(case["name"])


def _write(path, text):
    with open(path, "wb") as f:
        f.write(text)
    return str(path)


def _reject(argv, word):
    rc, out, err = run_main(argv)
    assert rc == 2, (rc, err)
    assert err.startswith("mergeGeno.py: ") and err.count("\n") == 1 and word in err, err


def test_rejected_inputs(tmp_path):
    good = os.path.join(MERGE, "s1.geno.gz")
    fai = os.path.join(MERGE, "small.fai")
    _reject(["-i", good, "-f", _write(tmp_path / "a.fai", b"c1\t60\nc2\n")], "fewer than two fields")
    _reject(["-i", good, "-f", _write(tmp_path / "b.fai", b"c1\tsixty\n")], "not an integer")
    _reject(["-i", good, "-f", _write(tmp_path / "c.fai", b"c1\t60\nc2\t30\nc1\t10\n")], "twice")
    _reject(["-i", good, "-f", _write(tmp_path / "d.fai", b"c1\t1234567890123456789\n")], "18 digits")
    _reject(["-i", good, "-f", fai, "--outputOnly", "2"], "--outputOnly")
    _reject(["-i", good, "-f", fai, "--outputOnly", "0"], "--outputOnly")
    _reject(["-i", good, "-i", _write(tmp_path / "empty.geno", b""), "-f", fai], "empty")
    _reject(["-i", good, "-i", _write(tmp_path / "latin.geno", "#CHROM\tPOS\tx\nc1\t3\té\n".encode("latin-1")), "-f", fai, "--method", "union"], "ASCII")
    _reject(["-i", _write(tmp_path / "hdr.geno", "#CHROM\tPOS\té\n".encode("utf-8")), "-f", fai], "ASCII")
    _reject(["-i", good, "-i", _write(tmp_path / "long.geno", b"#CHROM\tPOS\tx\nc1\t1234567890123456789\tA\n"), "-f", fai, "--method", "union"], "18 digits")
    _reject(sum([["-i", good] for _ in range(33)], []) + ["-f", fai], "32")


STOP_WORDS = {"stop_zero": "plain decimal", "stop_range": "outside", "stop_scaffold": "not in the .fai", "stop_repeat": "behind",
              "stop_blank": "fewer than two fields"}


@pytest.mark.parametrize("case", [c for c in MERGE_CASES if c["name"].startswith("stop_")], ids=lambda c: c["name"])
def test_a_stopped_file_gives_its_warning(case, tmp_path):
    out, err = run_case(case, tmp_path)
    fixture = case["name"].rsplit("_", 1)[0]
    word = STOP_WORDS[fixture]
    warnings = [ln for ln in err.splitlines() if "warning" in ln]
    assert len(warnings) == 1 and fixture + ".geno.gz stops at line" in warnings[0] and word in warnings[0], err
    # the line number is the file's own, the header counted
    with gzip.open(os.path.join(MERGE, fixture + ".geno.gz"), "rt") as f:
        lines = f.read().split("\n")
    n = int(warnings[0].split("stops at line ")[1].split(":")[0])
    s2 = gzip.open(os.path.join(MERGE, "s2.geno.gz"), "rt").read().split("\n")
    assert lines[:n - 1] == s2[:n - 1] and lines[n - 1] != s2[n - 1]
    assert mergegeno.last_info["stopped_files"] == 1


@pytest.mark.parametrize("seed,kind", [(1, "zero"), (2, "range"), (3, "scaffold"), (4, "repeat"), (5, "back"), (6, "plus"), (7, None)])
@pytest.mark.parametrize("method", ["intersect", "union", "all"])
def test_host_route_equals_the_model_on_random_files(seed, kind, method, tmp_path, monkeypatch):
    paths, fai = random_files(seed, 150, 3, str(tmp_path), scaffolds=3, n_fai=5, stop=(seed % 3, kind) if kind else None, bare_file=seed % 4)
    argv = sum([["-i", p] for p in paths], []) + ["-f", fai, "--method", method]
    monkeypatch.setenv("PG_STREAM_BYTES", "900")
    rc, out, err = run_main(argv)
    assert rc == 0, err
    assert out == merge_model.merge_argv(argv)
    assert mergegeno.last_info["stopped_files"] == (1 if kind else 0)


def test_a_dense_method_over_files_beyond_the_stream_size_takes_few_rounds(tmp_path, monkeypatch):
    argv, stream, bound = dense_files(str(tmp_path))
    monkeypatch.setenv("PG_STREAM_BYTES", str(stream))
    rc, out, err = run_main(argv)
    assert rc == 0, err
    assert out == merge_model.merge_argv(argv) and out.count(b"\n") == 20001
    info = mergegeno.last_info
    assert info["blocks"] >= 6                               # (the files exceed the stream size several times)
    assert info["rounds"] <= bound(info["blocks"]), info


def test_round_planning_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "merge_plan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tests", "merge_plan_main.cpp"), "-o", exe])
    r = subprocess.run([exe, "400"], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, r.stdout.decode()[-2000:] + r.stderr.decode()[-2000:]
    assert b"ok" in r.stdout
