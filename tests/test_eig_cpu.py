"""The genoToEigenstrat.py drop-in (genomics_general_amd/genoeig.py + pg_eig_text, the host route) against the outputs of the
UNMODIFIED reference tools/genoToEigenstrat.py (tests/golden/make_golden_eig.py): the three files byte for byte from gzipped, plain and
stdin input, in one block and in blocks of 3 000 bytes; the rejections (status 2, one message, no output file) and the stops at a line
(status 1, the rows before it the golden's prefix, no .ind); the `lines done...` line; pg_eig_text under ASan and UBSan in a program of
its own."""
import gzip
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from eig_cases import CASES, OUTPUTS, fixture_path, golden  # noqa: E402

SCRIPT = os.path.join(ROOT, "tools", "genoToEigenstrat.py")
BY_NAME = {c[0]: c for c in CASES}


def _argv(argv):
    return [a.replace("@G", GOLD) for a in argv]


def _outs(tmp_path):
    return {k: str(tmp_path / ("out." + k)) for k in OUTPUTS}


def _out_args(outs):
    return ["--genoOutFile", outs["geno"], "--snpOutFile", outs["snp"], "--indOutFile", outs["ind"]]


def _read(outs):
    got = {}
    for k, p in outs.items():
        if os.path.exists(p):
            with open(p, "rb") as f:
                got[k] = f.read()
    return got


def _script(argv, text=None, block=None):
    env = dict(os.environ, PG_EIG_DEVICE="0")
    if block:
        env["PG_STREAM_BYTES"] = str(block)
    return subprocess.run([sys.executable, SCRIPT] + argv, input=text, stdout=subprocess.PIPE, stderr=subprocess.PIPE, env=env, timeout=120, cwd=ROOT)


def _text(fixture):
    inp = fixture_path(fixture)
    with (gzip.open(inp, "rb") if inp.endswith(".gz") else open(inp, "rb")) as f:
        return f.read()


@pytest.fixture(autouse=True)
def _host_route(monkeypatch):
    monkeypatch.setenv("PG_EIG_DEVICE", "0")


@pytest.mark.parametrize("name,fixture,argv", CASES, ids=[c[0] for c in CASES])
@pytest.mark.parametrize("block", [None, 3000], ids=["one_block", "blocks_of_3000"])
@pytest.mark.parametrize("source", ["gz", "plain", "stdin"])
def test_eig_reproduces_the_reference(name, fixture, argv, source, block, tmp_path, monkeypatch):
    from genomics_general_amd import genoeig
    inp = fixture_path(fixture)
    text = _text(fixture)
    outs = _outs(tmp_path)
    if source == "stdin":
        r = _script(_out_args(outs) + _argv(argv), text, block)
        assert r.returncode == 0, r.stderr
        assert r.stdout == b""
        assert _read(outs) == golden(name)
        return
    if (source == "plain") == inp.endswith(".gz"):           # the other form of the fixture
        inp = str(tmp_path / ("in.geno" if source == "plain" else "in.geno.gz"))
        with open(inp, "wb") as g:
            g.write(text if source == "plain" else gzip.compress(text))
    if block:
        monkeypatch.setenv("PG_STREAM_BYTES", str(block))
    assert genoeig.genoeig_main(["-g", inp] + _out_args(outs) + _argv(argv)) == 0
    assert _read(outs) == golden(name)
    if block and len(text) > 10 * block:
        assert genoeig.last_info["blocks"] > 5 and genoeig.last_info["blocks_on_host"] == genoeig.last_info["blocks"]


def test_cumulative_positions_cross_block_ends():
    """mixed_cumul in blocks of 3 000 bytes (above) carries the scaffold, its label, the last position and the offsets over some forty
    block ends: the golden's positions on chr2 lie behind the last kept position of chr1"""
    snp = golden("mixed_cumul")["snp"].decode().split("\n")[:-1]
    plain = golden("mixed_phased")["snp"].decode().split("\n")[:-1]
    assert len(snp) == len(plain) and snp != plain
    shift = {int(a.split("\t")[3]) - int(b.split("\t")[3]) for a, b in zip(snp, plain)}
    assert len(shift) == 2 and 0 in shift


def _geno(tmp_path, body, head="#CHROM\tPOS\ta\tb\n"):
    p = str(tmp_path / "t.geno")
    with open(p, "wb") as f:
        f.write((head + body).encode("utf-8") if isinstance(body, str) else head.encode() + body)
    return p


def test_quirks_checked_by_hand(tmp_path):
    """the issue's observed behaviours: alleles counted over all samples, -s in file order with an unknown name, the tie's
    alphabetically first base counted, C/N and C/X read as 9, the index over all sites, int() of the position"""
    inp = _geno(tmp_path, "c\t007\tA/A\tA/A\tC/C\nc\t2\tA/A\tA/A\tA/A\nc\t+1_0\tC/N\tC/X\tT/T\nc\t4\tA/C\tN/N\tN/N\nc\t5\tA/A/T\tT\tA\n",
                head="#CHROM\tPOS\ta\tb\tc\n")
    outs = _outs(tmp_path)
    r = _script(["-g", inp, "-f", "phased", "-s", "b,zz,a"] + _out_args(outs))
    assert r.returncode == 0, r.stderr
    got = _read(outs)
    assert got["geno"] == b"00\n99\n19\n11\n"              # site 0: C counted, a and b have none; site 2: C the rarer; site 3: the tie counts A
    assert got["snp"] == b"0\t22\t0.0\t7\tA\tC\n2\t22\t0.0\t10\tC\tT\n3\t22\t0.0\t4\tA\tC\n4\t22\t0.0\t5\tA\tT\n"
    assert got["ind"] == b"a  U  NA\nb  U  NA\n"


def test_every_spelling_split_takes(tmp_path):
    """runs of blanks and tabs, \\r\\n, a lone \\r, leading blanks, a '#' line that is no site, a line of two fields; on stdin a \\r is
    whitespace inside the line"""
    body = "c \t 07\tA/A   T/A\r\n  c\t+1_0\tC/C\tC/T\textra\rc\t-3\tG/G\tG/G\n#c\t4\tA/A\tA/T\n #c\t5\tA/A\tA/T\nc 12\n"
    inp = _geno(tmp_path, body, head="CHROM POS  a\tb\n")
    outs = _outs(tmp_path)
    r = _script(["-g", inp, "-f", "phased"] + _out_args(outs))
    assert r.returncode == 0, r.stderr
    got = _read(outs)
    assert got["geno"] == b"01\n01\n01\n"
    assert got["snp"] == b"0\t22\t0.0\t7\tA\tT\n1\t22\t0.0\t10\tC\tT\n3\t22\t0.0\t5\tA\tT\n"
    r = _script(["-f", "phased"] + _out_args(outs), b"#CHROM\tPOS\ta\tb\nc\t1\tA/A\r\tT/A\nc\t2\tA/T\tT/T\r\n")
    assert r.returncode == 0, r.stderr
    assert _read(outs)["geno"] == b"01\n10\n"


REJECTED = [
    ("no_format", "c\t1\tA/A\tA/C\n", [], b"-f"),
    ("paired", "c\t1\tA/A\tA/C\n", ["-f", "paired"], b"paired"),
    ("samples_match_no_name", "c\t1\tA/A\tA/C\n", ["-f", "phased", "-s", "x,y"], b"-s"),
    ("chrom_file_line_of_three_fields", "c\t1\tA/A\tA/C\n", ["-f", "phased", "--chromFile", "@CHROM"], b"line 2"),
    ("not_ascii", "c\t1\tA/A\tA/C\nc\t2\tA/A\tA/Å\n", ["-f", "phased"], b"line 3"),
    ("header_not_ascii", None, ["-f", "phased"], b"line 1"),
    ("header_without_samples", "", ["-f", "phased"], b"no sample"),
    ("position_of_19_digits", "c\t1\tA/A\tA/C\nc\t1234567890123456789\tA/A\tA/A\n", ["-f", "phased"], b"line 3"),
    ("genotype_of_17_alleles", "c\t1\tA/A\tA/C\nc\t2\tA/A\t" + "/".join("A" * 17) + "\n", ["-f", "phased"], b"line 3"),
]


@pytest.mark.parametrize("name,body,argv,message", REJECTED, ids=[r[0] for r in REJECTED])
def test_rejected_with_one_message_status_2_and_no_output_file(name, body, argv, message, tmp_path):
    if name == "header_without_samples":
        inp = _geno(tmp_path, "c\t1\n", head="#CHROM\tPOS\n")
    elif body is None:
        inp = _geno(tmp_path, "c\t1\tA/A\tA/A\n", head="#CHROM\tPOS\tå\tb\n")
    else:
        inp = _geno(tmp_path, body)
    chrom = str(tmp_path / "chrom.txt")
    with open(chrom, "w") as f:
        f.write("c 1\nd 2 3\n")
    outs = _outs(tmp_path)
    r = _script(["-g", inp] + [chrom if a == "@CHROM" else a for a in argv] + _out_args(outs))
    assert r.returncode == 2, (r.returncode, r.stderr)
    assert message in r.stderr and b"Traceback" not in r.stderr
    assert len([ln for ln in r.stderr.split(b"\n") if ln.startswith(b"genoToEigenstrat.py:")]) == 1
    assert _read(outs) == {}


# (name, golden case, data lines in front of the inserted line, the inserted line)
STOPS = [
    ("diplo_cell_outside_the_table", "diplo_all", 3, "x1\t9\tA\tZ\tA\tA"),
    ("blank_line", "edge_phased", 5, ""),
    ("one_field_line", "edge_phased", 7, "s2"),
    ("position_int_does_not_take", "edge_phased", 9, "s2\t3x\tA/A\tA/T\tA/A\tA"),
    ("kept_site_without_a_selected_cell", "edge_phased", 4, "s1\t9\tA/A\tA/T"),
    ("stop_in_a_long_file", "multi_sel", 2000, "chr2\t1.5\tA/A"),
]


@pytest.mark.parametrize("block", [None, 60], ids=["one_block", "small_blocks"])
@pytest.mark.parametrize("name,case,k,bad", STOPS, ids=[s[0] for s in STOPS])
def test_stopped_at_the_line_with_the_golden_prefix_written(name, case, k, bad, block, tmp_path):
    _, fixture, argv = BY_NAME[case]
    lines = _text(fixture).decode().split("\n")
    assert not any(ln.startswith("#") for ln in lines[1:k + 1])
    inp = str(tmp_path / "t.geno")
    with open(inp, "w") as f:
        f.write("\n".join(lines[:k + 1] + [bad] + lines[k + 1:]))
    outs = _outs(tmp_path)
    r = _script(["-g", inp] + _argv(argv) + _out_args(outs), block=block)
    assert r.returncode == 1 and b"Traceback" not in r.stderr, (r.returncode, r.stderr)
    assert ("%s line %d:" % (inp, k + 2)).encode() in r.stderr, r.stderr
    gold = golden(case)
    rows = [ln for ln in gold["snp"].split(b"\n")[:-1] if int(ln.split(b"\t")[0]) < k]
    got = _read(outs)
    assert "ind" not in got
    assert got["snp"] == b"".join(ln + b"\n" for ln in rows)
    assert got["geno"] == b"".join(ln + b"\n" for ln in gold["geno"].split(b"\n")[:len(rows)])
    assert 0 < len(rows) < gold["snp"].count(b"\n")


@pytest.mark.parametrize("block", [None, 30], ids=["one_block", "small_blocks"])
def test_cumulative_offset_of_a_label_that_is_no_key_stops_and_names_it(block, tmp_path):
    """genoToEigenstrat.py:44: the offsets are keyed by the --chromFile's scaffold names; sc2's label 7 is none of them"""
    chrom = str(tmp_path / "chrom.txt")
    with open(chrom, "w") as f:
        f.write("sc1 sc1\nsc2 7\n")
    outs = _outs(tmp_path)
    inp = fixture_path("cumul_a")
    r = _script(["-g", inp, "-f", "phased", "--cumulativePos", "--chromFile", chrom] + _out_args(outs), block=block)
    assert r.returncode == 1 and b"Traceback" not in r.stderr, (r.returncode, r.stderr)
    assert ("%s line 5:" % inp).encode() in r.stderr and b"label 7 of scaffold sc2" in r.stderr
    gold = golden("cumul_a_chrom")
    got = _read(outs)
    assert "ind" not in got
    assert got["snp"] == b"".join(ln + b"\n" for ln in gold["snp"].split(b"\n")[:2]) and got["snp"].startswith(b"0\tsc1\t0.0\t2\t")
    assert got["geno"] == b"".join(ln + b"\n" for ln in gold["geno"].split(b"\n")[:2])


def test_lines_done_goes_to_stdout_after_every_100000th_site(tmp_path):
    inp = str(tmp_path / "big.geno")
    with open(inp, "w") as f:
        f.write("#CHROM\tPOS\ta\n" + "".join("c\t%d\t%s\n" % (i + 1, ("A/A", "A/T", "N/N")[i % 3]) for i in range(100001)))
    outs = _outs(tmp_path)
    r = _script(["-g", inp, "-f", "phased"] + _out_args(outs))
    assert r.returncode == 0, r.stderr
    assert r.stdout == b"100000 lines done...\n"
    got = _read(outs)
    assert got["geno"].count(b"\n") == got["snp"].count(b"\n") == 33334 and got["snp"].endswith(b"100000\t22\t0.0\t100001\tA\tT\n")


def test_help_lists_the_reference_flags():
    r = subprocess.run([sys.executable, SCRIPT, "-h"], stdout=subprocess.PIPE, timeout=120, cwd=ROOT)
    assert r.returncode == 0
    for flag in ("--genoFile", "--genoFormat", "--genoOutFile", "--snpOutFile", "--indOutFile", "--samples", "--chromFile", "--cumulativePos",
                 "--nullChrom", "phased,diplo,paired"):
        assert flag.encode() in r.stdout, flag


def test_eig_host_program_under_asan(tmp_path):
    """tests/eig_host_main.cpp: pg_eig_text on crafted blocks (an empty block, a last line without cells, a cell at the very end of the
    buffer, a repeated name on a short line, --cumulativePos carried over two blocks, output buffers one byte too small) under
    AddressSanitizer and UndefinedBehaviorSanitizer, in a program of its own"""
    exe = str(tmp_path / "eig_host_main")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-static-libasan", "-static-libubsan", os.path.join(ROOT, "tests", "eig_host_main.cpp"),
                           os.path.join(ROOT, "genomics_general_amd", "csrc", "pg_eig.cpp"),
                           os.path.join(ROOT, "genomics_general_amd", "csrc", "pg_gvcf.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    assert r.returncode == 0, (r.returncode, r.stdout.decode()[-2000:], r.stderr.decode()[-3000:])
    assert b"ok" in r.stdout
