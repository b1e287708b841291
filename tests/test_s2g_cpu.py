"""The seqToGeno.py drop-in's host route (pg_s2g_strip, pg_s2g_text; PG_S2G_DEVICE=0): every golden of the unmodified reference from
gzip, plain and stdin input, in one block and in blocks of 3 000 bytes, to a file, a .gz file and the standard output; every
rejection (exit status 2, one message, no file) and the stop at a short sequence (status 1, the rows before it); -P k against the
golden of the spelled-out list; genoToSeq.py then seqToGeno.py gives a .geno file's cells back; the host functions under ASan and
UBSan in a program of its own."""
import gzip
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from s2g_common import GOLD, expected, fasta, run  # noqa: E402
from s2g_cases import CASES, SINGLE_PLOIDY, golden, input_bytes  # noqa: E402


@pytest.mark.parametrize("name,inp,argv,how", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("source,block,out", [("gz", None, "file"), ("plain", None, "gz"), ("plain", 3000, "file"), ("stdin", None, "stdout"),
                                              ("stdin", 3000, "file")])
def test_host_route_reproduces_the_reference(name, inp, argv, how, source, block, out, tmp_path):
    rc, got, info, err = run(input_bytes(inp), argv, tmp_path, source=source, block=block, out=out)
    assert rc == 0, err[-2000:]
    assert got == golden(name)
    assert int(info["device_blocks"]) == 0 and int(info["out_ranges"]) >= 1, info


@pytest.mark.parametrize("inp,argv,gold", SINGLE_PLOIDY)
def test_single_ploidy_value_means_it_for_every_group(inp, argv, gold, tmp_path):
    rc, got, _, err = run(input_bytes(inp), argv, tmp_path)
    assert rc == 0, err[-2000:]
    assert got == golden(gold)


FA = b">a x\nACGT\nAC\n>b\nACGTTT\n>c\nAAAAAA\n>d\nCCCCCCC\n"
PHY = b"2 4\nx ACGT\ny AAAA\n"
MULTI = b"2 4\nx ACGT\ny AAAA\n2 3\ny CCC\nx GGG\n"
REJECTED = [
    ("no sequences", b"no record here\n", []),
    ("empty input", b"", []),
    ("no sequences in phylip", b"just words\n", ["-f", "phylip"]),
    ("record without a line feed", b">a\nACGT\n>b", []),
    ("empty name", b">\nACGT\n", []),
    ("blank name", b"> \nACGT\n", []),
    ("absent -S", FA, ["-S", "a", "nobody"]),
    ("absent -S in multi", MULTI, ["-f", "phylip", "-S", "x", "z"]),
    ("ploidies that do not sum", FA, ["-P", "2", "1"]),
    ("ploidy that does not divide", FA, ["-P", "3"]),
    ("ploidy of zero", FA, ["-P", "0", "4"]),
    ("random phase", FA, ["-P", "2", "2", "--randomPhase"]),
    ("multi with ploidy", MULTI, ["-f", "phylip", "-P", "2"]),
    ("phylip line of one word", b"2 8\nx ACGT\ny AAAA\nACGT\nAAAA\n", ["-f", "phylip"]),
    ("phylip with fewer names", b"3 4\nx ACGT\ny AAAA\n", ["-f", "phylip"]),
    ("multi with unequal counts", b"2 4\nx ACGT\ny AAAA\n1 3\ny CCC\n", ["-f", "phylip"]),
    ("not ASCII", ">a\nAC\xc3\xa9T\n".encode("latin-1"), []),
    ("not ASCII in phylip", "1 3\nx A\xe9C\n".encode("latin-1"), ["-f", "phylip"]),
    ("not ASCII in -C", FA, ["-C", "café"]),
]


@pytest.mark.parametrize("why,data,argv", REJECTED, ids=[r[0] for r in REJECTED])
@pytest.mark.parametrize("source", ["plain", "stdin"])
def test_rejections_leave_no_file(why, data, argv, source, tmp_path):
    rc, got, _, err = run(data, argv, tmp_path, source=source)
    assert rc == 2, (rc, err)
    assert got is None
    lines = [ln for ln in err.splitlines() if ln.strip()]
    assert len(lines) == 1 and lines[0].startswith("seqToGeno.py: "), err


def test_a_short_later_sequence_stops_at_its_line(tmp_path):
    data = fasta(3, 4, 0, lengths=[50, 50, 20, 19])
    rc, got, _, err = run(data, ["-C", "z"], tmp_path)
    assert rc == 1
    assert got == expected(data, chrom="z") and got.count(b"\n") == 20
    lines = [ln for ln in err.splitlines() if ln.startswith("seqToGeno.py: ")]
    assert len(lines) == 1 and "site 20" in lines[0] and "q3" in lines[0], err
    # a group is as long as its shortest member; a longer later sequence is cut
    rc, got, _, err = run(data, ["-P", "1", "1", "2"], tmp_path)
    assert rc == 1 and got.count(b"\n") == 20 and "q2_q3" in err, err
    rc, got, _, err = run(fasta(4, 3, 0, lengths=[30, 31, 40]), [], tmp_path)
    assert rc == 0 and got.count(b"\n") == 31, err
    # multi-phylip: the alignments before it whole, its rows up to there
    rc, got, _, err = run(b"2 3\nx ACG\ny TTT\n2 3\nx ACG\ny TT\n2 3\nx ACG\ny TTT\n", ["-f", "phylip"], tmp_path)
    assert rc == 1 and got == b"#CHROM\tPOS\tx\ty\ncontig00\t1\tA\tT\ncontig00\t2\tC\tT\ncontig00\t3\tG\tT\ncontig01\t1\tA\tT\ncontig01\t2\tC\tT\n", (got, err)


def _cells(path):
    with gzip.open(path, "rb") as f:
        lines = f.read().decode().split("\n")[1:-1]
    return [ln.split("\t")[2:] for ln in lines if not ln.startswith("#")]


@pytest.mark.parametrize("fixture,phased", [("haplo", False), ("c1", True), ("multi", True), ("sparse", True)])
def test_genotoseq_then_seqtogeno_gives_the_cells_back(fixture, phased, tmp_path):
    geno = os.path.join(GOLD, fixture + ".geno.gz")
    want = _cells(geno)
    fa = str(tmp_path / "seqs.fa")
    env = dict(os.environ, PG_SEQ_DEVICE="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "genoToSeq.py"), "-g", geno, "-s", fa, "-f", "fasta"] + (["--splitPhased"] if phased else []),
                       env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300, cwd=ROOT)
    assert r.returncode == 0, r.stderr.decode()[-2000:]
    with open(fa, "rb") as f:
        data = f.read()
    rc, got, _, err = run(data, ["-P", "2"] if phased else [], tmp_path)
    assert rc == 0, err[-2000:]
    rows = [ln.split("\t")[2:] for ln in got.decode().split("\n")[1:-1]]
    if phased:
        want = [["|".join(c[::2]) for c in row] for row in want]
    assert rows == want


def test_s2g_host_program_under_asan(tmp_path):
    """pg_s2g_strip / pg_s2g_text (csrc/pg_s2g.cpp, no GPU context) on crafted inputs in heap buffers of exactly their size, under
    AddressSanitizer and UndefinedBehaviorSanitizer, in a program of its own"""
    exe = str(tmp_path / "s2g_host")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "s2g_host_main.cpp"),
                           os.path.join(ROOT, "genomics_general_amd", "csrc", "pg_s2g.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=300)
    assert r.returncode == 0 and b"s2g host ok" in r.stdout, r.stdout.decode()[-3000:]
