"""The genoToVCF.py drop-in (genomics_general_amd/genovcf.py + pg_gvcf_text, the host route) against the outputs of the UNMODIFIED
reference VCF_processing/genoToVCF.py (tests/golden/make_golden_gvcf.py): byte for byte from gzipped, plain and stdin input, in one
block and in blocks of 3 000 bytes; the rejections and the stops at a line (status, message, the rows written before); the spellings
split() takes; pg_gvcf_text under ASan and UBSan in a program of its own."""
import gzip
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from gvcf_cases import CASES, fixture_path  # noqa: E402

SCRIPT = os.path.join(ROOT, "VCF_processing", "genoToVCF.py")
HEAD = ('##fileformat=VCFv4.2\n##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n'
        "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t")


def _argv(argv):
    return [a.replace("@G", GOLD) for a in argv]


def _golden(name):
    with gzip.open(os.path.join(GOLD, "gvcf", name + ".out.gz"), "rb") as f:
        return f.read()


def _script(argv, text=None, block=None):
    env = dict(os.environ, PG_GVCF_DEVICE="0")
    if block:
        env["PG_STREAM_BYTES"] = str(block)
    return subprocess.run([sys.executable, SCRIPT] + argv, input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120, cwd=ROOT)


@pytest.fixture(autouse=True)
def _host_route(monkeypatch):
    monkeypatch.setenv("PG_GVCF_DEVICE", "0")


@pytest.mark.parametrize("name,fixture,argv", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("block", [None, 3000], ids=["one_block", "blocks_of_3000"])
@pytest.mark.parametrize("source", ["gz", "plain", "stdin"])
def test_gvcf_reproduces_the_reference(name, fixture, argv, source, block, tmp_path, monkeypatch):
    from genomics_general_amd import genovcf
    inp = fixture_path(fixture)
    with (gzip.open(inp, "rb") if inp.endswith(".gz") else open(inp, "rb")) as f:
        text = f.read()
    if source == "stdin":
        r = _script(_argv(argv), text, block)
        assert r.returncode == 0, r.stderr
        assert r.stdout == _golden(name)
        return
    if source == "plain" and inp.endswith(".gz"):
        inp = str(tmp_path / "in.geno")
        with open(inp, "wb") as g:
            g.write(text)
    if block:
        monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    out = str(tmp_path / "out.vcf")
    assert genovcf.genovcf_main(["-g", inp, "-o", out] + _argv(argv)) == 0
    with open(out, "rb") as f:
        assert f.read() == _golden(name)
    if block and len(text) > 10 * block:
        assert genovcf.last_info["blocks"] > 5 and genovcf.last_info["blocks_on_host"] == genovcf.last_info["blocks"]


def test_gz_output_is_bgzf_of_the_same_text(tmp_path):
    from genomics_general_amd import genovcf
    name, fixture, argv = CASES[2]
    out = str(tmp_path / "out.vcf.gz")
    assert genovcf.genovcf_main(["-g", fixture_path(fixture), "-o", out] + _argv(argv)) == 0
    with open(out, "rb") as f:
        raw = f.read()
    assert raw.endswith(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))     # BGZF end-of-file member
    assert gzip.decompress(raw) == _golden(name)


def test_missing_fai_warns_and_writes_no_contig_lines(tmp_path):
    name, fixture, argv = CASES[4]
    r = _script(["-g", fixture_path(fixture)] + _argv(argv))
    assert r.returncode == 0 and b"WARNING: Could not parse fai file" in r.stderr
    assert b"##contig" not in r.stdout and b"##reference=file:ref_nofai.fa\n" in r.stdout
    r = _script(["-g", fixture_path("extra")] + _argv(CASES[26][2]))
    assert b"WARNING" not in r.stderr and r.stdout.count(b"##contig=<ID=") == 7 and b"##contig=<ID=x1,length=16>\n" in r.stdout


def _geno(tmp_path, body, head="#CHROM\tPOS\ta\tb\n"):
    p = str(tmp_path / "t.geno")
    with open(p, "wb") as f:
        f.write((head + body).encode("utf-8") if isinstance(body, str) else head.encode() + body)
    return p


def _fasta(tmp_path, text=">c desc\nACgT\nnNAC\n", fai=None):
    p = str(tmp_path / "r.fa")
    with open(p, "w") as f:
        f.write(text)
    if fai is not None:
        with open(p + ".fai", "w") as f:
            f.write(fai)
    return p


def test_quirks_checked_by_hand(tmp_path):
    """the issue's quirks: N/N alone, with a reference, A/N beside a reference n, haploid and polyploid cells, the fasta's base verbatim,
    a reference base among the alleles moved to the front"""
    inp = _geno(tmp_path, "c\t1\tN/N\tN/N\nc\t5\tA/N\tN/N\nc\t3\tA\tT|T|G\nc\t4\tA/A\tT/A\nc\t6\tN/N\tN/N\n")
    r = _script(["-g", inp, "-f", "phased"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == HEAD + "a\tb\n" + ("c\t1\t.\tN\t.\t.\t.\t.\tGT\t0/0\t0/0\nc\t5\t.\tA\t.\t.\t.\t.\tGT\t./.\t./.\n"
                                                  "c\t3\t.\tT\tG,A\t.\t.\t.\tGT\t2\t0|0|1\nc\t4\t.\tA\tT\t.\t.\t.\tGT\t0/0\t1/0\n"
                                                  "c\t6\t.\tN\t.\t.\t.\t.\tGT\t0/0\t0/0\n")
    r = _script(["-g", inp, "-f", "phased", "-r", _fasta(tmp_path)])
    assert r.returncode == 0, r.stderr
    rows = r.stdout.decode().split("\n")
    assert rows[1] == "##reference=file:r.fa"
    assert rows[4:] == ["c\t1\t.\tA\tN\t.\t.\t.\tGT\t1/1\t1/1", "c\t5\t.\tn\tA\t.\t.\t.\tGT\t./.\t./.", "c\t3\t.\tg\tT,G,A\t.\t.\t.\tGT\t3\t1|1|2",
                        "c\t4\t.\tT\tA\t.\t.\t.\tGT\t1/1\t0/1", "c\t6\t.\tN\t.\t.\t.\t.\tGT\t0/0\t0/0", ""]
    inp = _geno(tmp_path, "c\t6\tA/N\tN/N\n")
    r = _script(["-g", inp, "-f", "phased", "-r", _fasta(tmp_path)])
    assert r.stdout.decode().split("\n")[4] == "c\t6\t.\tN\tA\t.\t.\t.\tGT\t1/0\t0/0"


def test_every_spelling_split_takes(tmp_path):
    """runs of blanks and tabs, \\r\\n, a lone \\r, leading blanks, extra cells, a '#' line, a line of two fields (its position is
    the first sample's cell), positions with a sign, zeros and underscores; the header whatever it begins with"""
    body = "c \t 07\tA/A   T/A\r\n  c\t+1_0\tC/C\tC/T\textra\rc\t-3\tG/G\tG/G\n#c\t4\tA/A\tA/A\n #c\t5\tA/A\tA/T\nc 12\n"
    inp = _geno(tmp_path, body, head="CHROM POS  a\tb\n")
    r = _script(["-g", inp, "-f", "phased", "-s", "a"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode() == HEAD + "a\n" + ("c\t7\t.\tA\t.\t.\t.\t.\tGT\t0/0\nc\t10\t.\tC\t.\t.\t.\t.\tGT\t0/0\nc\t-3\t.\tG\t.\t.\t.\t.\tGT\t0/0\n"
                                               "#c\t5\t.\tA\t.\t.\t.\t.\tGT\t0/0\nc\t12\t.\tN\t.\t.\t.\t.\tGT\t.\n")
    # stdin has no universal newlines: a \r is whitespace inside the line
    r = _script(["-f", "phased"], b"#CHROM\tPOS\ta\tb\nc\t1\tA/A\r\tT/T\nc\t2\tA/T\tT/T\r\n")
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().split("\n")[3:] == ["c\t1\t.\tT\tA\t.\t.\t.\tGT\t1/1\t0/0", "c\t2\t.\tT\tA\t.\t.\t.\tGT\t1/0\t0/0", ""]


def test_a_name_the_header_holds_twice_takes_its_last_cell_present(tmp_path):
    inp = _geno(tmp_path, "c\t1\tA/A\tC/C\tT/T\nc\t2\tA/A\tC/C\n", head="#CHROM\tPOS\ta\tb\ta\n")
    r = _script(["-g", inp, "-f", "phased", "-s", "a"])
    assert r.returncode == 0, r.stderr
    assert r.stdout.decode().split("\n")[3:] == ["c\t1\t.\tT\t.\t.\t.\t.\tGT\t0/0", "c\t2\t.\tA\t.\t.\t.\t.\tGT\t0/0", ""]


def test_fasta_rules(tmp_path):
    """text before the first record ignored, the name the first word, blanks and line feeds removed, the last of two records wins"""
    fa = _fasta(tmp_path, "junk\n>c first\nTTTT\n>d\nGG GG\n>c\tsecond\nAC GT\r\nac\n")
    inp = _geno(tmp_path, "c\t1\tN/N\tN/N\nc\t6\tN/N\tN/N\nd\t4\tN/N\tN/N\n")
    r = _script(["-g", inp, "-f", "phased", "-r", fa])
    assert r.returncode == 0, r.stderr
    assert [x.split("\t")[3] for x in r.stdout.decode().split("\n")[4:7]] == ["A", "c", "G"]


REJECTED = [
    ("no_format", "c\t1\tA/A\tA/A\n", [], None, b"-f"),
    ("sample_not_in_header", "c\t1\tA/A\tA/A\n", ["-f", "phased", "-s", "a,z"], None, b"sample z"),
    ("fai_short_line", "c\t1\tA/A\tA/A\n", ["-f", "phased", "-r", "@FA"], "c\t8\nd\n", b".fai line 2"),
    ("not_ascii", "c\t1\tA/A\tA/Å\n", ["-f", "phased"], None, b"line 2"),
    ("header_not_ascii", None, ["-f", "phased"], None, b"line 1"),
    ("position_of_19_digits", "c\t1\tA/A\tA/A\nc\t1234567890123456789\tA/A\tA/A\n", ["-f", "phased"], None, b"line 3"),
]


@pytest.mark.parametrize("name,body,argv,fai,message", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_with_one_message_and_status_2(name, body, argv, fai, message, tmp_path):
    inp = _geno(tmp_path, body) if body is not None else _geno(tmp_path, "c\t1\tA/A\tA/A\n", head="#CHROM\tPOS\tå\tb\n")
    argv = [_fasta(tmp_path, fai=fai) if a == "@FA" else a for a in argv]
    r = _script(["-g", inp] + argv)
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert message in r.stderr and b"Traceback" not in r.stderr
    assert len([ln for ln in r.stderr.split(b"\n") if ln.startswith(b"genoToVCF.py:")]) == 1


STOPS = [
    ("diplo_cell_outside_the_table", "c\t1\tA\tW\nc\t2\tA\tZ\nc\t3\tA\tA\n", ["-f", "diplo"], 3, 1),
    ("fewer_cells_than_selected", "c\t1\tA/A\tT/T\nc\t2\tA/A\nc\t3\tA/A\tA/A\n", ["-f", "phased"], 3, 1),
    ("blank_line", "c\t1\tA/A\tT/T\n\nc\t3\tA/A\tA/A\n", ["-f", "phased"], 3, 1),
    ("position_int_does_not_take", "c\t1\tA/A\tT/T\nc\t2\tA/A\tT/T\nc\t3x\tA/A\tA/A\n", ["-f", "phased"], 4, 2),
    ("scaffold_the_fasta_lacks", "c\t1\tA/A\tT/T\nz\t2\tA/A\tT/T\n", ["-f", "phased", "-r", "@FA"], 3, 1),
    ("position_beyond_the_sequence", "c\t8\tA/A\tT/T\nc\t9\tA/A\tT/T\n", ["-f", "phased", "-r", "@FA"], 3, 1),
    ("position_below_1", "c\t1\tA/A\tT/T\nc\t0\tA/A\tT/T\n", ["-f", "phased", "-r", "@FA"], 3, 1),
]


@pytest.mark.parametrize("block", [None, 12], ids=["one_block", "a_line_a_block"])
@pytest.mark.parametrize("name,body,argv,line,rows", STOPS, ids=[s[0] for s in STOPS])
def test_stopped_at_the_line_with_the_rows_before_it_written(name, body, argv, line, rows, block, tmp_path):
    inp = _geno(tmp_path, body)
    argv = [_fasta(tmp_path) if a == "@FA" else a for a in argv]
    r = _script(["-g", inp] + argv, block=block)
    assert r.returncode not in (0, 2) and b"Traceback" not in r.stderr, (r.returncode, r.stderr)
    assert ("%s line %d:" % (inp, line)).encode() in r.stderr, r.stderr
    sites = [ln for ln in r.stdout.split(b"\n") if ln and not ln.startswith(b"#")]
    assert len(sites) == rows and sites[0].startswith(b"c\t")


def test_help_lists_the_reference_flags():
    r = subprocess.run([sys.executable, SCRIPT, "-h"], stdout=subprocess.PIPE, timeout=120, cwd=ROOT)
    assert r.returncode == 0
    for flag in ("--genoFile", "--genoFormat", "--outFile", "--reference", "--samples", "phased,diplo,pairs"):
        assert flag.encode() in r.stdout, flag


def test_gvcf_host_program_under_asan(tmp_path):
    """tests/gvcf_host_main.cpp: pg_gvcf_text on crafted blocks (an empty block, a last line without cells, a cell at the very end of
    the buffer, a position at the last base of the last sequence, an output buffer one byte too small) under AddressSanitizer and
    UndefinedBehaviorSanitizer, in a program of its own"""
    exe = str(tmp_path / "gvcf_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "gvcf_host_main.cpp"),
                           os.path.join(ROOT, "genomics_general_amd", "csrc", "pg_gvcf.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert b"ok" in r.stdout
