"""The genoToPlink.py drop-in (genomics_general_amd/genoplink.py + pg_ped_text, the host route) against the outputs of the UNMODIFIED
reference tools/genoToPlink.py (tests/golden/make_golden_plink.py): the files byte for byte from gzipped, plain and stdin input, in one
block and in blocks of 3 000 bytes; the rejections (status 2) and the stops at a line (status 1), each with one message and no output
file left behind; the stderr lines; pg_ped_text under ASan and UBSan in a program of its own."""
import gzip
import os
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from plink_cases import CASES, command, fixture_path, golden  # noqa: E402

SCRIPT = os.path.join(ROOT, "tools", "genoToPlink.py")
BY_NAME = {c[0]: c for c in CASES}


def _read(outs):
    got = {}
    for k, p in outs.items():
        if os.path.exists(p):
            with open(p, "rb") as f:
                got[k] = f.read()
    return got


def _script(argv, text=None, block=None):
    env = dict(os.environ, PG_PED_DEVICE="0")
    if block:
        env["PG_STREAM_BYTES"] = str(block)
    return subprocess.run([sys.executable, SCRIPT] + argv, input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120, cwd=ROOT)


def _text(fixture):
    inp = fixture_path(fixture)
    with (gzip.open(inp, "rb") if inp.endswith(".gz") else open(inp, "rb")) as f:
        return f.read()


@pytest.fixture(autouse=True)
def _host_route(monkeypatch):
    monkeypatch.setenv("PG_PED_DEVICE", "0")


# (without -g the reference needs --prefix: the cases on the default prefix have no stdin form)
SOURCES = [(c, s) for c in CASES for s in ("gz", "plain", "stdin") if s != "stdin" or "--prefix" in c[2]]


@pytest.mark.parametrize("case,source", SOURCES, ids=["%s-%s" % (c[0], s) for c, s in SOURCES])
@pytest.mark.parametrize("block", [None, 3000], ids=["one_block", "blocks_of_3000"])
def test_plink_reproduces_the_reference(case, source, block, tmp_path, monkeypatch):
    from genomics_general_amd import genoplink
    name, fixture, argv = case
    text = _text(fixture)
    if source == "stdin":
        args, outs = command(argv, "", str(tmp_path))
        r = _script(args, text, block)
        assert r.returncode == 0, r.stderr
        assert r.stdout == b""
        assert _read(outs) == golden(name)
        return
    inp = str(tmp_path / ("in.geno" if source == "plain" else "in.geno.gz"))
    if (source == "plain") == fixture_path(fixture).endswith(".gz"):       # the other form of the fixture
        with open(inp, "wb") as g:
            g.write(text if source == "plain" else gzip.compress(text))
    else:
        shutil.copy(fixture_path(fixture), inp)
    if block:
        monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    args, outs = command(argv, inp, str(tmp_path))
    assert genoplink.main(["-g", inp] + args) == 0
    assert _read(outs) == golden(name)
    assert sorted(p for p in os.listdir(str(tmp_path)) if p != os.path.basename(inp)) == sorted(os.path.basename(p) for p in outs.values())
    if block and len(text) > 10 * block:
        assert genoplink.last_info["blocks"] > 5 and genoplink.last_info["blocks_on_host"] == genoplink.last_info["blocks"]


def _geno(tmp_path, body, head="#CHROM\tPOS\ta\tb\n"):
    p = str(tmp_path / "t.geno")
    with open(p, "wb") as f:
        f.write((head + body).encode("utf-8") if isinstance(body, str) else head.encode() + body)
    return p


def _left_behind(tmp_path):
    return sorted(p for p in os.listdir(str(tmp_path)) if p != "t.geno")


def test_truncation_checked_by_hand(tmp_path):
    """the issue's example: G|G then G in x1, A|C in x2, T|T in x1 again -- the cut is per sample and per run, never per file; under
    -f alleles every character of the shortest cell stays, the separator included"""
    inp = _geno(tmp_path, "x1\t1\tG|G\tA|A\nx1\t2\tG\tA|C\nx2\t1\tA|C\tT|T\nx1\t3\tT|T\tC|C\n")
    r = _script(["-g", inp, "--prefix", str(tmp_path / "o")])
    assert r.returncode == 0, r.stderr
    with open(str(tmp_path / "o.ped"), "rb") as f:
        assert f.read() == b"0 a 0 0 0 0 G G A C T T\n0 b 0 0 0 0 A A A C T T C C\n"
    with open(str(tmp_path / "o.map"), "rb") as f:
        assert f.read() == b"x1 1 0 1\nx1 2 0 2\nx2 1 0 1\nx1 3 0 3\n"
    r = _script(["-g", inp, "--prefix", str(tmp_path / "o"), "-f", "alleles", "-s", "b"])
    assert r.returncode == 0, r.stderr
    with open(str(tmp_path / "o.ped"), "rb") as f:
        assert f.read() == b"0 b 0 0 0 0 A | A A | C T | T C | C\n"


def test_every_spelling_split_takes(tmp_path):
    """runs of blanks and tabs, \\r\\n, a lone \\r, leading blanks, a '#' line that is no site, int() of the position; on stdin a \\r
    is whitespace inside the line"""
    body = "c \t 07\tA/A   T/A\r\n  c\t+1_0\tC/C\tC/T\rc\t-3\tG/G\tG/G\n#c\t4\tA/A\tA/T\nd 12 A/A T/T\n"
    inp = _geno(tmp_path, body, head="CHROM POS  a\tb\n")
    r = _script(["-g", inp, "--prefix", str(tmp_path / "o")])
    assert r.returncode == 0, r.stderr
    with open(str(tmp_path / "o.ped"), "rb") as f:
        assert f.read() == b"0 a 0 0 0 0 A A C C G G A A\n0 b 0 0 0 0 T A C T G G T T\n"
    with open(str(tmp_path / "o.map"), "rb") as f:
        assert f.read() == b"c 7 0 7\nc 10 0 10\nc -3 0 -3\nd 12 0 12\n"
    r = _script(["--prefix", str(tmp_path / "p")], b"#CHROM\tPOS\ta\tb\nc\t1\tA/A\r\tT/A\nc\t2\tA/T\tT/T\r\n")
    assert r.returncode == 0, r.stderr
    with open(str(tmp_path / "p.ped"), "rb") as f:
        assert f.read() == b"0 a 0 0 0 0 A A A T\n0 b 0 0 0 0 T A T T\n"


REJECTED = [
    ("no_input_and_no_prefix", None, [], b"--prefix"),
    ("sample_the_header_lacks", "c\t1\tA/A\tA/C\n", ["-s", "a", "nobody"], b"nobody"),
    ("sample_twice_in_s", "c\t1\tA/A\tA/C\n", ["-s", "b", "a", "b"], b"twice"),
    ("sample_twice_in_the_header", "c\t1\tA/A\tA/C\tA/A\n", [], b"more than once"),
    ("selected_sample_twice_in_the_header", "c\t1\tA/A\tA/C\tA/A\n", ["-s", "a"], b"more than once"),
    ("header_without_samples", "c\t1\n", [], b"no sample"),
    ("header_not_ascii", "c\t1\tA/A\tA/A\n", [], b"line 1"),
]


@pytest.mark.parametrize("name,body,argv,message", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_with_one_message_status_2_and_no_output_file(name, body, argv, message, tmp_path):
    head = {"sample_twice_in_the_header": "#CHROM\tPOS\ta\tb\ta\n", "selected_sample_twice_in_the_header": "#CHROM\tPOS\ta\tb\ta\n",
            "header_without_samples": "#CHROM\tPOS\n", "header_not_ascii": "#CHROM\tPOS\tå\tb\n"}.get(name, "#CHROM\tPOS\ta\tb\n")
    if body is None:
        r = subprocess.run([sys.executable, SCRIPT], input=b"#CHROM\tPOS\ta\nc\t1\tA/A\n", stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                           env=dict(os.environ, PG_PED_DEVICE="0"), timeout=120, cwd=str(tmp_path))
    else:
        r = _script(["-g", _geno(tmp_path, body, head), "--prefix", str(tmp_path / "o"), "--makeFAM"] + argv)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert message in r.stderr and b"Traceback" not in r.stderr
    assert len([ln for ln in r.stderr.split(b"\n") if ln.startswith(b"genoToPlink.py:")]) == 1
    assert _left_behind(tmp_path) == []


def test_a_repeated_header_name_that_is_not_used_is_no_obstacle(tmp_path):
    inp = _geno(tmp_path, "c\t1\tA/A\tA/C\tT/T\n", head="#CHROM\tPOS\ta\tb\ta\n")
    r = _script(["-g", inp, "--prefix", str(tmp_path / "o"), "-s", "b"])
    assert r.returncode == 0, r.stderr
    with open(str(tmp_path / "o.ped"), "rb") as f:
        assert f.read() == b"0 b 0 0 0 0 A C\n"


# (name, golden case, data lines in front of the inserted line, the inserted line, what the message names)
STOPS = [
    ("blank_line", "edge_phased", 5, "", b"blank"),
    ("one_field_line", "edge_phased", 7, "s2", b"one field"),
    ("position_int_does_not_take", "edge_phased", 9, "s2\t3x\tA/A\tA/T\tA/A\tA", b"position"),
    ("position_of_19_digits", "edge_phased", 3, "s1\t1234567890123456789\tA/A\tA/T\tA/A\tA", b"18 digits"),
    ("fewer_cells_than_the_header", "edge_phased", 4, "s1\t9\tA/A\tA/T\tA/A", b"number of genotypes"),
    ("more_cells_than_the_header", "edge_phased", 4, "s1\t9\tA/A\tA/T\tA/A\tA\tA", b"number of genotypes"),
    ("line_ends_before_a_selected_column", "edge_sel", 6, "s2\t9\tA/A\tA/T\tA/A", b"-s"),
    ("diplo_cell_outside_the_table", "diplo_all", 3, "x1\t9\tA\tZ\tA\tA", b"diplo"),
    ("diplo_cell_of_two_letters", "diplo_sel", 2, "x1\t9\tA\tAC\tA\tA", b"diplo"),
    ("not_ascii", "edge_phased", 8, "s2\t9\tA/A\tA/Å\tA/A\tA", b"ASCII"),
    ("stop_in_a_long_file", "multi_sel", 2000, "chr2\t1.5\tA/A", b"position"),
]


@pytest.mark.parametrize("block", [None, 60], ids=["one_block", "small_blocks"])
@pytest.mark.parametrize("name,case,k,bad,word", STOPS, ids=[s[0] for s in STOPS])
def test_stopped_at_the_line_with_status_1_and_no_output_file(name, case, k, bad, word, block, tmp_path):
    _, fixture, argv = BY_NAME[case]
    lines = _text(fixture).decode().split("\n")
    assert not any(ln.startswith("#") for ln in lines[1:k + 1])
    inp = str(tmp_path / "t.geno")
    with open(inp, "wb") as f:
        f.write("\n".join(lines[:k + 1] + [bad] + lines[k + 1:]).encode("utf-8"))
    args, _ = command(argv + ["--makeFAM"], inp, str(tmp_path))
    r = _script(["-g", inp] + args, block=block)
    assert r.returncode == 1 and b"Traceback" not in r.stderr, (r.returncode, r.stderr)
    assert ("%s line %d:" % (inp, k + 2)).encode() in r.stderr and word in r.stderr, r.stderr
    assert len([ln for ln in r.stderr.split(b"\n") if ln.startswith(b"genoToPlink.py:")]) == 1
    assert _left_behind(tmp_path) == []


@pytest.mark.parametrize("body", ["", "# no site\n#c\t1\tA/A\tA/A\n"], ids=["header_only", "hash_lines_only"])
def test_a_file_without_sites_stops_as_the_reference_does(body, tmp_path):
    """the unmodified script raises TypeError at the end of such an input (addSite on the site None) and writes nothing"""
    r = _script(["-g", _geno(tmp_path, body), "--prefix", str(tmp_path / "o"), "--makeFAM"])
    assert r.returncode == 1 and b"no site" in r.stderr and b"Traceback" not in r.stderr, (r.returncode, r.stderr)
    assert _left_behind(tmp_path) == []


def test_the_reference_stderr_lines(tmp_path):
    inp = _geno(tmp_path, "x1\t1\tG|G\tA|A\nx2\t1\tA|C\tT|T\nx1\t3\tT|T\tC|C\n")
    r = _script(["-g", inp, "--prefix", str(tmp_path / "o"), "--makeFAM"])
    assert r.returncode == 0, r.stderr
    assert r.stderr == (b"1 scaffolds read into memory\n2 scaffolds read into memory\n3 scaffolds read into memory\nWriting PED file...\n"
                        b"Writing MAP file...\nWriting FAM file...\n")
    r = _script(["-g", inp, "--prefix", str(tmp_path / "o")])
    assert r.returncode == 0 and b"FAM" not in r.stderr


def test_fam_prefix_names_the_file_exactly_and_the_default_prefix_cuts_at_the_last_dot(tmp_path):
    inp = str(tmp_path / "x.y.geno.gz")
    with open(inp, "wb") as f:
        f.write(gzip.compress(b"#CHROM\tPOS\ta\tb\nc\t1\tA/A\tA/C\n"))
    r = _script(["-g", inp, "--makeFAM", "--FAMprefix", str(tmp_path / "fam_as_named")])
    assert r.returncode == 0, r.stderr
    assert sorted(os.listdir(str(tmp_path))) == ["fam_as_named", "x.y.geno.gz", "x.y.geno.map", "x.y.geno.ped"]
    with open(str(tmp_path / "fam_as_named"), "rb") as f:
        assert f.read() == b"0 a 0 0 0 0\n0 b 0 0 0 0\n"


def test_help_lists_the_reference_flags():
    r = subprocess.run([sys.executable, SCRIPT, "-h"], stdout=subprocess.PIPE, timeout=120, cwd=ROOT)
    assert r.returncode == 0
    for flag in ("--genoFile", "--genoFormat", "--prefix", "--makeFAM", "--FAMprefix", "--samples", "haplo,diplo,pairs,alleles,phased"):
        assert flag.encode() in r.stdout, flag


def test_plink_host_program_under_asan(tmp_path):
    """tests/plink_host_main.cpp: pg_ped_text on crafted blocks (an empty block, '#' lines only, a last line without a line feed, a
    cell at the very end of the buffer, ragged cells, a two-field line, runs that cross the threads' shares, every stop) under
    AddressSanitizer and UndefinedBehaviorSanitizer, in a program of its own"""
    exe = str(tmp_path / "plink_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "plink_host_main.cpp"),
                           os.path.join(ROOT, "genomics_general_amd", "csrc", "pg_ped.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert b"ok" in r.stdout
