"""What the mergeGeno.py tests share (test_merge_cpu.py, test_merge_emul.py, test_gpu_merge.py): the goldens, one run of the driver
inside the test's process with its standard streams caught, seeded random files."""
import gzip
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
MERGE = os.path.join(GOLD, "merge")
sys.path.insert(0, GOLD)
from merge_cases import MERGE_CASES, out_args, read_output  # noqa: E402

from genomics_general_amd import mergegeno  # noqa: E402

CASE_IDS = [c["name"] for c in MERGE_CASES]


def golden(name):
    with gzip.open(os.path.join(MERGE, name + ".out.gz"), "rb") as f:
        return f.read()


class _Out:
    def __init__(self):
        self.buffer = io.BytesIO()

    def write(self, s):
        self.buffer.write(s.encode())

    def flush(self):
        pass


def run_main(argv):
    """mergegeno.main(argv) with the standard streams caught: (exit status, stdout bytes, stderr text)"""
    old = sys.stdout, sys.stderr
    sys.stdout, sys.stderr = _Out(), io.StringIO()
    try:
        try:
            rc = mergegeno.main(argv)
        except SystemExit as exc:
            rc = exc.code
        return rc, sys.stdout.buffer.getvalue(), sys.stderr.getvalue()
    finally:
        sys.stdout, sys.stderr = old


def case_argv(case, directory=MERGE):
    return [a.format(dir=directory) for a in case["argv"]]


def run_case(case, tmp_path, directory=MERGE):
    """one golden case through the driver: (the bytes its golden holds, stderr)"""
    tmp = str(tmp_path / "o")
    os.makedirs(tmp)
    rc, out, err = run_main(case_argv(case, directory) + out_args(case, tmp))
    assert rc == 0, err
    return read_output(case, tmp, out), err


def many_rounds_stream(case):
    """PG_STREAM_BYTES under which a golden case takes more than 10 rounds: a few lines a file and round (the fixtures on small.fai hold
    about 40 lines of 10 - 14 bytes, the others 240 and more of about 20)"""
    return 60 if "small.fai" in " ".join(case["argv"]) else 700


def dense_files(directory, n_pos=20000):
    """two files that hold the even and the odd positions of one scaffold of n_pos positions: with --method all every position is
    written, and the files exceed a PG_STREAM_BYTES of 40 000 several times.  Returns (argv, upper bound on the rounds given the blocks
    read).  The bound: a dense round ends at the horizon (then a file is consumed whole and read further: at most one round a block
    read), at the scaffold's end (once), or after its output budget -- stream / (bytes of a line no file adds to) positions, and such a
    line is below 64 bytes here: at most n_pos / (stream // 64) rounds"""
    fai = os.path.join(directory, "dense.fai")
    with open(fai, "w") as f:
        f.write("chr\t%d\n" % n_pos)
    paths = []
    for x in range(2):
        path = os.path.join(directory, "dense_%d.geno" % x)
        with open(path, "w") as f:
            f.write("#CHROM\tPOS\ts%d\n" % x + "".join("chr\t%d\t%s\n" % (p, "AT"[x]) for p in range(1 + x, n_pos + 1, 2)))
        paths.append(path)
    stream = 40000
    bound = lambda blocks: blocks + 1 + n_pos // (stream // 64) + 1          # noqa: E731
    return sum([["-i", p] for p in paths], []) + ["-f", fai, "--method", "all"], stream, bound


def random_files(seed, n_sites, n_files, directory, scaffolds=2, n_fai=None, big=False, stop=None, long_tails=(), bare_file=None, keep=0.7,
                 report=None):
    """seeded random inputs under `directory`: a .fai of `n_fai` names (default: the scaffolds used) and n_files plain `.geno` files that
    each keep a site of the shared list with probability `keep`; cells of 1 - 5 characters.  big: scaffold 0 is 3e9 long and its sites
    lie across 2^31.  stop: (file, kind) -- one stopping line in the second half of that file.  long_tails: (file, bytes) -- one line of
    that file gets a cell of that many bytes.  bare_file: that file has two header fields only.  One site is the last position of its
    scaffold.  report: a dict that gets stopped = whether the stopping line was put in.  Returns (paths, fai path)"""
    rng = np.random.default_rng(seed)
    n_fai = n_fai or scaffolds
    used = sorted(rng.choice(n_fai, size=scaffolds, replace=False).tolist())
    names = ["sc%d_%s" % (k, "x" * int(rng.integers(0, 9))) for k in range(n_fai)]
    lens = [int(rng.integers(50, 400)) for _ in range(n_fai)]
    if big:
        lens[used[0]] = 3 * 10 ** 9
    per = [n_sites // scaffolds + (1 if k < n_sites % scaffolds else 0) for k in range(scaffolds)]
    sites = []
    for k, s in enumerate(used):
        n = min(per[k], lens[s])
        if big and k == 0:
            pos = sorted(set(int(p) for p in rng.integers(2 ** 31 - 200, 2 ** 31 + 200, size=n)))
        else:
            pos = sorted(rng.choice(np.arange(1, lens[s] + 1), size=n, replace=False).tolist())
            if pos:
                pos[-1] = lens[s]                              # a position equal to the scaffold's length
        sites += [(s, int(p)) for p in pos]
    fai = os.path.join(directory, "r%d.fai" % seed)
    with open(fai, "w") as f:
        for nm, ln in zip(names, lens):
            f.write("%s\t%d\n" % (nm, ln))
    letters = np.array(list("ACGTN/|-*acgt."))
    paths = []
    for x in range(n_files):
        n_samples = 0 if x == bare_file else int(rng.integers(1, 4))
        lines = []
        for s, p in sites:
            if rng.random() >= keep:
                continue
            cells = ["".join(letters[rng.integers(0, len(letters), size=int(rng.integers(1, 6)))]) for _ in range(n_samples)]
            lines.append([names[s], str(p)] + cells)
        for fx, nbytes in long_tails:
            if fx == x and lines and n_samples:
                lines[len(lines) // 3][2] = "".join(letters[rng.integers(0, len(letters), size=nbytes)])
        text = ["\t".join(ln) for ln in lines]
        if stop is not None and stop[0] == x and len(text) >= 2:
            at = len(text) // 2 + int(rng.integers(0, max(len(text) // 2, 1)))
            at = min(max(at, 1), len(text) - 1)
            before = lines[at - 1]
            bad = {"zero": [before[0], "0" + before[1]], "range": [before[0], str(10 ** 10)], "scaffold": ["nowhere", "1"],
                   "repeat": before[:2], "back": [lines[0][0], lines[0][1]], "plus": [before[0], "+" + before[1]]}[stop[1]]
            text.insert(at, "\t".join(bad + ["A"] * n_samples))
            if report is not None:
                report["stopped"] = True
        path = os.path.join(directory, "r%d_%d.geno" % (seed, x))
        with open(path, "w") as f:
            f.write("\t".join(["#CHROM", "POS"] + ["f%ds%d" % (x, k) for k in range(n_samples)]) + "\n" + "".join(t + "\n" for t in text))
        paths.append(path)
    return paths, fai
