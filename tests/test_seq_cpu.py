"""The genoToSeq.py drop-in (genomics_general_amd/genoseq.py + pg_seq_text, the host route) against the outputs of the UNMODIFIED
reference genoToSeq.py (tests/golden/make_golden_seq.py): byte for byte, from gzipped, plain and stdin input and with blocks that
windows span; the cases on which the reference dies with a traceback end with status 2 and a message; the host route against itself
over block sizes on seeded random files; pg_seq_text under AddressSanitizer in a program of its own (tests/seq_host_main.cpp)."""
import os
import subprocess
import sys

import numpy as np
import pytest

from seq_common import CASE_IDS, GOLD, ROOT, SEQ_CASES, fixture_text, golden, random_geno, run_case, run_main

from genomics_general_amd import genoseq


@pytest.fixture(autouse=True)
def _host_route(monkeypatch):
    monkeypatch.setenv("PG_SEQ_DEVICE", "0")


@pytest.mark.parametrize("case", SEQ_CASES, ids=CASE_IDS)
@pytest.mark.parametrize("source", ["gz", "plain", "stdin"])
def test_seq_reproduces_the_reference(case, source, tmp_path):
    assert run_case(case, tmp_path, source) == golden(case["name"])


@pytest.mark.parametrize("case", SEQ_CASES, ids=CASE_IDS)
def test_seq_windows_span_blocks(case, tmp_path, monkeypatch):
    monkeypatch.setenv("PG_STREAM_BYTES", "3000")
    assert run_case(case, tmp_path) == golden(case["name"])
    assert genoseq.last_info["blocks"] > 1 or case["fixture"] == "seqmix"


def test_seq_wrapper_reads_stdin_and_writes_stdout():
    case = SEQ_CASES[CASE_IDS.index("haplo_coord_step_above")]
    argv = [a for a in case["argv"] if a not in ("-g", "{geno}")]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "genoToSeq.py")] + argv, input=fixture_text(case["fixture"]), stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, env=dict(os.environ, PG_SEQ_DEVICE="0"), timeout=120, cwd=ROOT)
    assert r.returncode == 0, r.stderr
    assert r.stdout == golden(case["name"])


HAPLO = os.path.join(GOLD, "haplo.geno.gz")
SPARSE = os.path.join(GOLD, "sparse.geno.gz")
COORD = ["-M", "windows", "--windType", "coordinate", "--windSize", "1000", "--stepSize", "1000"]
SITES = ["-M", "windows", "--windType", "sites", "--windSize", "100", "--overlap", "0", "--maxDist", "1000"]

REJECTED = [
    ("seqnameformat_windows", ["-g", HAPLO, "--seqNameFormat", "contig"] + COORD, "seqNameFormat"),
    ("seqnameformat_contigs", ["-g", HAPLO, "--seqNameFormat", "sample_contig", "-M", "contigs"], "seqNameFormat"),
    ("samples_windows", ["-g", HAPLO, "-S", "s0_A"] + COORD, "-S"),
    ("samples_contigs", ["-g", HAPLO, "-S", "s0_A", "-M", "contigs"], "-S"),
    ("sites_without_maxdist", ["-g", HAPLO, "-M", "windows", "--windSize", "100", "--overlap", "0"], "--maxDist"),
    ("sites_without_overlap", ["-g", HAPLO, "-M", "windows", "--windSize", "100", "--maxDist", "1000"], "--overlap"),
    ("coordinate_without_size", ["-g", HAPLO, "-M", "windows", "--windType", "coordinate", "--stepSize", "100"], "--windSize"),
    ("coordinate_without_step", ["-g", HAPLO, "-M", "windows", "--windType", "coordinate", "--windSize", "100"], "--stepSize"),
    ("separate_without_s", ["-g", HAPLO, "--separateFiles"] + COORD, "-s"),
    ("sample_not_in_header", ["-g", HAPLO, "-S", "s0_A,nobody"], "nobody"),
    ("haplotype_not_in_header", ["-g", SPARSE, "--splitPhased", "-S", "s1", "--ploidy", "3"] + ["2"] * 11, "s1_C"),
    ("cell_not_2p_minus_1", ["-g", HAPLO, "--splitPhased"], "line 2"),
    # sparse has a stretch of 1706 positions without a site on chr1: a window of 500 there is empty
    ("empty_coordinate_window", ["-g", SPARSE, "-M", "windows", "--windType", "coordinate", "--windSize", "500", "--stepSize", "500"], "holds no site"),
]


@pytest.mark.parametrize("name,argv,word", REJECTED, ids=[r[0] for r in REJECTED])
def test_seq_rejects_what_the_reference_dies_on(name, argv, word):
    rc, out, err = run_main(argv)
    assert rc == 2
    assert err.startswith("genoToSeq.py: ") and err.count("\n") == 1 and word in err, err


def test_seq_empty_window_comes_after_the_windows_before_it(tmp_path):
    """the reference writes the windows in front of the empty one, then dies: so does the drop-in, and names scaffold and limits"""
    rc, out, err = run_main(["-g", SPARSE, "-M", "windows", "--windType", "coordinate", "--windSize", "500", "--stepSize", "500"])
    assert rc == 2 and "chr1:" in err
    assert out.count(b">s0\n") >= 1
    first = int(err.split("chr1:")[1].split("-")[0])
    assert out.count(b">s0\n") == (first - 1) // 500


def test_seq_line_with_fewer_fields(tmp_path):
    text = fixture_text("haplo").split(b"\n")
    text[40] = b"\t".join(text[40].split(b"\t")[:-1])
    p = str(tmp_path / "short.geno")
    with open(p, "wb") as f:
        f.write(b"\n".join(text))
    for mode in ([], ["-M", "contigs"], ["-S", "s0_A"]):
        rc, out, err = run_main(["-g", p] + mode)
        assert rc == 2 and "line 41:" in err and "fewer fields" in err, err


def test_seq_multi_rank_launch_leaves_the_job_to_rank_0(tmp_path, monkeypatch):
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")
    out = str(tmp_path / "x.fa")
    rc, so, err = run_main(["-g", HAPLO, "-s", out])
    assert rc == 0 and so == b"" and not os.path.exists(out)


def _seq_bytes(chunk, n_seq):
    return [chunk.slice(q, 0, chunk.n) for q in range(n_seq)]


@pytest.mark.parametrize("seed,split", [(1, True), (2, False), (3, True)])
def test_seq_host_route_over_block_sizes(seed, split):
    """pg_seq_text on the whole text against blocks of one to three lines: the same bytes, positions and scaffold runs"""
    rng = np.random.default_rng(seed)
    ploidies = [int(p) for p in rng.integers(1, 4, size=7)]
    header, text, _ = random_geno(seed, 300, ploidies, comments=(0, 57, 299))

    class A:
        splitPhased, ploidy, NtoGap = split, ploidies, bool(seed & 1)
    plan = genoseq.Plan(header, A, None)
    whole, pos, starts, names, err, _, n_lines = genoseq.host_seq(plan, text.encode())
    assert err == 0 and n_lines == 300 and whole.n == 297
    lines = text.encode().splitlines(keepends=True)
    sites = genoseq.Sites()
    k = 0
    while k < len(lines):
        step = int(rng.integers(1, 4))
        c, p, s, nm, e, _, _ = genoseq.host_seq(plan, b"".join(lines[k:k + step]))
        assert e == 0
        sites.append(c, p, s, nm)
        k += step
    assert np.array_equal(sites.pos, pos)
    assert sites.run_starts == [int(x) for x in starts] and sites.run_names == names
    for q in range(plan.cfg.n_seq):
        assert b"".join(sites.pieces(q, 0, whole.n)) == _seq_bytes(whole, plan.cfg.n_seq)[q]
        assert b"".join(sites.pieces(q, 10, 200)) == b"".join(genoseq.Sites.pieces(_one(whole), q, 10, 200))


def _one(chunk):
    s = genoseq.Sites()
    s.chunks = [chunk]
    return s


def test_seq_host_program_under_asan(tmp_path):
    """tests/seq_host_main.cpp: pg_seq_text on crafted blocks (empty block, a last line without cells, a cell at the very end of the
    buffer ...) under AddressSanitizer and UndefinedBehaviorSanitizer, in a program of its own"""
    exe = str(tmp_path / "seq_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "seq_host_main.cpp"),
                           os.path.join(ROOT, "genomics_general_amd", "csrc", "pg_seq.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert b"ok" in r.stdout
