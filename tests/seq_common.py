"""What the genoToSeq.py tests share (test_seq_cpu.py, test_seq_emul.py, test_gpu_seq.py): the goldens, one run of the driver inside
the test's process with its standard streams caught, seeded random `.geno` text."""
import gzip
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, GOLD)
from seq_cases import SEQ_CASES, out_args, read_output  # noqa: E402

from genomics_general_amd import genoio, genoseq  # noqa: E402

CASE_IDS = [c["name"] for c in SEQ_CASES]


def golden(name):
    with gzip.open(os.path.join(GOLD, "seq", name + ".out.gz"), "rb") as f:
        return f.read()


def fixture_text(name):
    with gzip.open(os.path.join(GOLD, name + ".geno.gz"), "rb") as f:
        return f.read()


class _Out:
    def __init__(self):
        self.buffer = io.BytesIO()

    def write(self, s):
        self.buffer.write(s.encode())

    def flush(self):
        pass


class _In:
    def __init__(self, data):
        self.f = io.BytesIO(data)

    def read(self, n=-1):
        return self.f.read(n)


def run_main(argv, stdin=None):
    """genoseq.main(argv) with the standard streams caught: (exit status, stdout bytes, stderr text)"""
    old = sys.stdout, sys.stderr, genoio.STDIN
    sys.stdout, sys.stderr = _Out(), io.StringIO()
    if stdin is not None:
        genoio.STDIN = _In(stdin)
    try:
        try:
            rc = genoseq.main(argv)
        except SystemExit as exc:
            rc = exc.code
        return rc, sys.stdout.buffer.getvalue(), sys.stderr.getvalue()
    finally:
        sys.stdout, sys.stderr, genoio.STDIN = old


def run_case(case, tmp_path, source="gz", geno=None):
    """one golden case through the driver: the bytes its golden holds.  source: "gz" the committed fixture, "plain" its text in a
    file, "stdin" its text on the standard input; geno: another file that holds the fixture (BGZF)"""
    tmp = str(tmp_path / "o")
    os.makedirs(tmp)
    path = geno or os.path.join(GOLD, case["fixture"] + ".geno.gz")
    stdin = None
    if source == "plain":
        path = str(tmp_path / "in.geno")
        with open(path, "wb") as f:
            f.write(fixture_text(case["fixture"]))
    elif source == "stdin":
        stdin = fixture_text(case["fixture"])
    argv = [a.format(geno=path) for a in case["argv"]] + out_args(case, tmp)
    if source == "stdin":
        k = argv.index("-g")
        del argv[k:k + 2]
    rc, out, err = run_main(argv, stdin)
    assert rc == 0, err
    return read_output(case, tmp, out)


def random_geno(seed, n_lines, ploidies, comments=(), irregular=None, base_pos=0):
    """seeded random `.geno` text of mixed ploidies (the header's samples s0 ..): scaffold and position fields of varying width,
    '#' lines at the line indices `comments`, at line `irregular` two spaces between two fields.  Returns (header, data text,
    the sites' cells as a list of lists of str)"""
    rng = np.random.default_rng(seed)
    header = "#CHROM\tPOS\t" + "\t".join("s%d" % k for k in range(len(ploidies))) + "\n"
    alphabet = np.array(list("ACGTNn-*RY"))
    scafs = ["c", "chr10", "scaffold_0123", "Q"]
    lines, sites = [], []
    pos, scaf = base_pos, 0
    for i in range(n_lines):
        if i in comments:
            lines.append("#skipped\tline %d" % i)
            continue
        if rng.random() < 0.02 and scaf < len(scafs) - 1:
            scaf += 1
            pos = base_pos
        pos += int(rng.integers(1, 10 ** int(rng.integers(1, 5))))
        cells = ["|".join(alphabet[rng.integers(0, len(alphabet), size=p)]) for p in ploidies]
        sep = "  " if i == irregular else "\t"
        lines.append(scafs[scaf] + "\t" + str(pos) + sep + "\t".join(cells))
        sites.append((scafs[scaf], pos, cells))
    return header, "\n".join(lines) + "\n", sites
