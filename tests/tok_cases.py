"""The case table of the device tokenizer's tests (csrc/pg_tokenize.hip), shared by tests/test_host.py (no GPU: the table against
the host tokenizer, the routes it reaches) and tests/test_gpu_tokenize.py (the kernels against the table).

A case is drawn, not parsed: build(spec) draws one-hot codes [lines][file haplotypes] and a spelling for every cell, writes the
`.geno` lines from them and returns the text together with what a tokenizer must make of it -- the drawn codes gathered through
HapLayout.col_slot, the drawn positions, the runs of equal drawn scaffold names.  No parser takes part in the expectation.

Spelling: A C G T are 1 2 4 8 and every other byte is 0, so a zero is spelt with the bytes 33 .. 255 in turn (all of them occur
across the table, tests/test_host.py checks it); phased cells take their separators from '/' and '|'; a diplo cell is one
character of the reference's table (genomics.py:14-15: the IUPAC codes of two bases), every other byte standing for N; cells are
separated by one blank, mostly a tab, now and then another of the five blanks the tokenizers know.

Which kernel takes a case is decided by pg_plan_tok (csrc/pg_tok_plan.h); plan() asks tests/tok_plan_main.cpp, and the cases that sit
on a boundary of that decision take their column counts from it."""
import functools
import os
import subprocess
import tempfile
from types import SimpleNamespace

import numpy as np

from genomics_general_amd.samples import HapLayout, SampleData

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

COLS = (1, 2, 63, 64, 65, 128, 129, 192, 193, 200, 256, 257, 300, 600)        # file sample columns
LINES = (1, 15, 16, 17, 63, 64, 65)                                          # a wavefront takes 16 lines, a block 64
SEAM_COLS = (2, 65, 200)
SEAM_LINES = (255, 256, 257, 513)                                            # k_tok_heads takes 256 lines per block
FAMILIES = ("phased2", "phased12", "pairs123", "haplo", "diplo")
LAYOUTS = ("all", "shuf")
FMT = {"phased2": "phased", "phased12": "phased", "pairs123": "pairs", "haplo": "haplo", "diplo": "diplo",
       "phasedwide": "phased", "pairswide": "pairs", "unwanted7": "phased"}
BLANKS = np.array([9, 32, 11, 12, 13], dtype=np.uint8)

BASES = np.frombuffer(b"ACGT", dtype=np.uint8)
ZERO_BYTES = np.array([b for b in range(33, 256) if b not in b"ACGT"], dtype=np.uint8)
# genomics.py:14-15: a diplo character and the two bases it stands for (every other byte: N N)
DIPLO = {"A": "AA", "C": "CC", "G": "GG", "K": "GT", "M": "AC", "N": "NN", "S": "CG", "R": "AG", "T": "TT", "W": "AT", "Y": "CT"}
CODE = {"A": 1, "C": 2, "G": 4, "T": 8, "N": 0}
DIPLO_CODES = np.zeros((256, 2), dtype=np.int8)
for _ch, _pair in DIPLO.items():
    DIPLO_CODES[ord(_ch)] = [CODE[_pair[0]], CODE[_pair[1]]]
DIPLO_CALLED = np.frombuffer(b"ACGKMSRTWY", dtype=np.uint8)
DIPLO_ZERO = np.array([b for b in range(33, 256) if b not in b"ACGKMSRTWY"], dtype=np.uint8)


def spec(name, family, ploidy, n_lines, layout="all", seed=0, unwanted=(), names=None, pos_text=None):
    """ploidy: alleles per file column (what the cell widths follow); unwanted: columns no layout asks for; names / pos_text: the
    scaffold name and the position's spelling of every line (drawn when None)"""
    return SimpleNamespace(name=name, family=family, fmt=FMT[family], ploidy=tuple(int(p) for p in ploidy), n_lines=int(n_lines), layout=layout,
                           seed=int(seed), unwanted=tuple(unwanted), names=names, pos_text=pos_text)


def _ploidies(family, n_cols, rng):
    if family in ("phased2", "diplo"):
        return [2] * n_cols
    if family == "haplo":
        return [1] * n_cols
    pool = {"phased12": (1, 2), "pairs123": (1, 2, 3), "phasedwide": (1, 2, 3, 26), "pairswide": (1, 2, 3, 4, 5)}[family]
    pl = rng.choice(pool, size=n_cols)
    k = min(n_cols, len(pool))
    pl[rng.permutation(n_cols)[:k]] = pool[::-1][:k]          # (every ploidy of the pool where the columns allow it, the widest first)
    return pl.tolist()


def _zero_and_forced(rng, n):
    """which of n wanted cells are missing (12 %, at least one) and four cells that take A C G T: from five cells on a case holds
    all four codes and zeros and at least 80 % of its cells are called"""
    if n < 5:
        return rng.random(n) < 0.12, None
    nz = max(1, int(round(0.12 * n)))
    perm = rng.permutation(n)
    zero = np.zeros(n, dtype=bool)
    zero[perm[:nz]] = True
    return zero, perm[nz:nz + 4]


def build(sp):
    rng = np.random.default_rng(sp.seed)
    fmt, L = sp.fmt, sp.n_lines
    pl = np.asarray(sp.ploidy, dtype=np.int64)
    n_cols = len(pl)
    # the layout: which columns are wanted, in which order their samples take their slots
    order = np.arange(n_cols)
    if sp.layout == "shuf":
        order = rng.permutation(n_cols)[n_cols // 3:]
    order = [int(c) for c in order if c not in sp.unwanted]
    col_names = ["s%d" % c for c in range(n_cols)]
    sd = SampleData(indNames=[col_names[c] for c in order], ploidyDict={col_names[c]: int(pl[c]) for c in order})
    lay = HapLayout(sd, col_names, fmt)
    # cells: widths and where they begin behind the line's head
    width = 2 * pl - 1 if fmt == "phased" else (pl if fmt == "pairs" else np.ones(n_cols, dtype=np.int64))
    off = np.concatenate([[0], np.cumsum(width + 1)[:-1]])
    cells_w = int(off[-1] + width[-1])
    hap_off = np.concatenate([[0], np.cumsum(pl)])
    n_fh = int(hap_off[-1])
    col_of = np.repeat(np.arange(n_cols), pl)
    k_of = np.arange(n_fh) - hap_off[col_of]
    wanted_col = np.zeros(n_cols, dtype=bool)
    wanted_col[order] = True
    block = np.empty((L, cells_w), dtype=np.uint8)
    if fmt == "diplo":
        chars = rng.choice(DIPLO_CALLED, size=(L, n_cols))
        miss = rng.random((L, n_cols)) < 0.12
        wi = np.flatnonzero(np.broadcast_to(wanted_col, (L, n_cols)).ravel())
        zero, forced = _zero_and_forced(rng, len(wi))
        flat, mflat = chars.reshape(-1), miss.reshape(-1)
        mflat[wi] = zero
        if forced is not None:
            flat[wi[forced]] = BASES
        nm = int(mflat.sum())
        flat[mflat] = DIPLO_ZERO[(sp.seed * 31 + np.arange(nm)) % len(DIPLO_ZERO)]
        codes = DIPLO_CODES[chars].reshape(L, n_fh)
        block[:, off] = chars
        allele_bytes = chars
    else:
        codes = (1 << rng.integers(0, 4, size=(L, n_fh))).astype(np.int8)
        miss = rng.random((L, n_fh)) < 0.12
        wi = np.flatnonzero(np.broadcast_to(wanted_col[col_of], (L, n_fh)).ravel())
        zero, forced = _zero_and_forced(rng, len(wi))
        miss.reshape(-1)[wi] = zero
        if forced is not None:
            codes.reshape(-1)[wi[forced]] = [1, 2, 4, 8]
        codes[miss] = 0
        chars = np.empty((L, n_fh), dtype=np.uint8)
        for b, ch in zip((1, 2, 4, 8), BASES):
            chars[codes == b] = ch
        z = codes == 0
        chars[z] = ZERO_BYTES[(sp.seed * 31 + np.arange(int(z.sum()))) % len(ZERO_BYTES)]
        step = 2 if fmt == "phased" else 1
        block[:, off[col_of] + step * k_of] = chars
        if fmt == "phased":
            inner = (off[col_of] + 2 * k_of + 1)[k_of + 1 < pl[col_of]]
            block[:, inner] = rng.choice(np.frombuffer(b"/|", dtype=np.uint8), size=(L, len(inner)))
        allele_bytes = chars
    if n_cols > 1:
        block[:, off[1:] - 1] = rng.choice(BLANKS, p=[0.8, 0.05, 0.05, 0.05, 0.05], size=(L, n_cols - 1))
    # heads: scaffold name and position of every line
    if sp.names is not None:
        names = list(sp.names)
    else:
        cuts = sorted(set(rng.integers(1, L, size=int(rng.integers(0, 3))).tolist())) if L > 1 else []
        run_of = np.searchsorted(np.asarray(cuts, dtype=np.int64), np.arange(L), side="right")
        names = ["sc%d" % (r + 1) for r in run_of]
    assert len(names) == L
    starts = [i for i in range(L) if i == 0 or names[i] != names[i - 1]]
    if sp.pos_text is not None:
        pos_text = list(sp.pos_text)
    else:
        steps = rng.integers(1, 60, size=L)
        pos_text, at = [], 0
        for i in range(L):
            at = int(steps[i]) if i in starts else at + int(steps[i])
            pos_text.append(str(at))
    pos = np.array([int(t) for t in pos_text], dtype=np.int64)
    lines, line_at, cells_at, at = [], [], [], 0
    for i in range(L):
        head = names[i].encode() + b"\t" + pos_text[i].encode() + b"\t"
        line_at.append(at)
        cells_at.append(at + len(head))
        lines.append(head + block[i].tobytes() + b"\n")
        at += len(lines[-1])
    # what the rows must hold: the drawn codes at the slots of the layout
    rows = np.zeros((L, lay.n_hap), dtype=np.int8)
    has = lay.col_slot >= 0
    src = hap_off[:n_cols, None] + np.arange(lay.max_ploidy)[None, :]
    rows[:, lay.col_slot[has]] = codes[:, src[has]]
    return SimpleNamespace(spec=sp, name=sp.name, text=b"".join(lines), lay=lay, rows=rows, pos=pos, run_starts=np.asarray(starts, dtype=np.int64),
                           run_names=[names[i] for i in starts], n_lines=L, n_cols=n_cols, width=width, off=off, line_at=line_at,
                           cells_at=cells_at, allele_bytes=allele_bytes, widest=int(width.max()), wanted_col=wanted_col)


# ---- the table --------------------------------------------------------------------------------------------------------------------
def _seed(*parts):
    s = 0
    for p in parts:
        s = (s * 1000003 + (sum(p.encode()) if isinstance(p, str) else int(p)) + 17) % (1 << 31)
    return s


def grid_spec(family, layout, n_cols, n_lines, tag="", **kw):
    seed = _seed(family, layout, n_cols, n_lines, tag)
    pl = _ploidies(family, n_cols, np.random.default_rng(seed + 1))
    return spec("%s-%s-c%d-l%d%s" % (family, layout, n_cols, n_lines, tag), family, pl, n_lines, layout, seed, **kw)


def grid(lines=LINES, cols=COLS, families=FAMILIES, layouts=LAYOUTS):
    """every column count x line count x format x layout"""
    return [grid_spec(f, lay, c, n) for f in families for lay in layouts for c in cols for n in lines]


def reduced():
    """the table of the forced forms' processes: all column counts and formats, 1, 17 and 65 lines"""
    return grid(lines=(1, 17, 65))


def _seam_names(variant, L):
    """scaffold names of L lines around the 256-line seams of k_tok_heads"""
    if variant == "none":                    # a change far from the seam, none across it
        return ["chr1" if i < 7 else "chr2" for i in range(L)]
    if variant == "around":                  # a change between the rows 254 | 255, 255 | 256 and 256 | 257 (and at 511 | 512 | 513)
        cut = [c for c in (255, 256, 257, 511, 512) if c < L]
        return ["chr%d" % (1 + sum(i >= c for c in cut)) for i in range(L)]
    a, b = ("chr1", "chr10") if variant == "prefix_up" else ("chr10", "chr1")      # names that begin with each other, across the seams
    return [(a, b, a)[(i >= 256) + (i >= 512)] for i in range(L)]


def seam():
    out, k = [], 0
    for c in SEAM_COLS:
        for n in SEAM_LINES:
            for variant in ("around", "none", "prefix_up", "prefix_down"):
                out.append(grid_spec(FAMILIES[k % 5], LAYOUTS[k % 2], c, n, "-" + variant, names=_seam_names(variant, n)))
                k += 1
    return out


def _fit_name(n, alt):
    return "s" + "a" * (n - 2) + ("b" if alt else "a") if n > 1 else "s"


def heads():
    out = []
    # scaffold + position + their two blanks of 63, 64 and 65 bytes (k_tok_heads holds 64 bytes of a line in LDS; beyond them it
    # reads the text), of 80 bytes with names that differ behind byte 64, and of 10: every length behind every other, names of
    # one length that differ in their last byte, names that begin with each other
    lens = (63, 64, 65, 80, 10)
    seq = [a for p in lens for q in lens for a in (p, q)] + [63, 63, 64, 64, 65, 65, 80, 80, 10, 10]
    names, pos_text = [], []
    for i, n in enumerate(seq):
        pos_text.append(str(1000 + i))
        names.append(_fit_name(n - 2 - 4, alt=i % 2 == 1 and i >= 2 * len(lens) ** 2))
    for family, c in (("phased2", 3), ("haplo", 1), ("pairs123", 65)):
        out.append(grid_spec(family, "all", c, len(seq), "-prefix", names=names, pos_text=pos_text))
    # positions as the reference's int() reads them
    pos_text = ["0", "1", str(2 ** 31 - 1), str(2 ** 31), str(10 ** 17), "+5", "999999999999999999", "7"]
    for family, c in (("phased2", 2), ("diplo", 65)):
        out.append(grid_spec(family, "all", c, len(pos_text), "-positions", names=["chrP"] * len(pos_text), pos_text=pos_text))
    # one-column haplo lines of five bytes: every head load runs past its line and, on the last line, past the text
    for n in (1, 17, 300):
        out.append(grid_spec("haplo", "all", 1, n, "-short", names=["a"] * n, pos_text=[str(i % 9 + 1) for i in range(n)]))
    return out


def general():
    """k_tok_cells' wide-cell branch: phased ploidy 3 and 26 beside 1 and 2, pairs ploidy 4 and 5, narrow wanted cells beside one
    unwanted cell of seven characters (which needs a second column: 2 columns stand where the others have 1)"""
    out = []
    for c in (1, 64, 65, 300):
        for n in (1, 16, 17, 65):
            for lay in LAYOUTS:
                out.append(grid_spec("phasedwide", lay, c, n))
                out.append(grid_spec("pairswide", lay, c, n))
            cu = max(c, 2)
            sp = grid_spec("phased2", "all", cu, n, "-unwanted7")
            wide = _seed(c, n) % cu
            pl = list(sp.ploidy)
            pl[wide] = 4
            out.append(spec("unwanted7-all-c%d-l%d" % (cu, n), "unwanted7", pl, n, "all", sp.seed, unwanted=(wide,)))
    return out


# ---- the plan, asked of tests/tok_plan_main.cpp ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def plan_exe():
    d = tempfile.mkdtemp(prefix="tok_plan_")
    exe = os.path.join(d, "tok_plan_main")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", os.path.join(ROOT, "tests", "tok_plan_main.cpp"), "-o", exe])
    return exe


def plan(shapes, switches=None, exe=None):
    """[(n_cols, max_ploidy, S, widest)] -> [(route, nit, lds bytes)] under the switches {name: value} (and no other PG_TOK_* switch)"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("PG_TOK_")}
    env.update(switches or {})
    out = []
    for k in range(0, len(shapes), 2000):
        r = subprocess.run([exe or plan_exe()] + ["%d:%d:%d:%d" % tuple(s) for s in shapes[k:k + 2000]], env=env, stdout=subprocess.PIPE,
                           stderr=subprocess.PIPE)
        assert r.returncode == 0, (r.returncode, r.stderr.decode()[-2000:])
        for ln in r.stdout.decode().splitlines():
            f = ln.split()
            out.append((f[4], int(f[5]), int(f[6])))
    assert len(out) == len(shapes)
    return out


def shape_of(case):
    lay = case.lay
    return (case.n_cols, lay.max_ploidy, (lay.n_hap + 15) // 16 * 16, case.widest)


def _s16(n):
    return (n + 15) // 16 * 16


@functools.lru_cache(maxsize=None)
def size_edges():
    """(the haplo column count from which k_tok_cells3's LDS no longer fits while k_tok_cells' does, the last diploid phased column
    count of the second form, the first of k_tok_parse), found by walking the plan function"""
    hap = plan([(n, 1, _s16(n), 1) for n in range(2900, 3100)])
    first_cells = 2900 + [r[0] for r in hap].index("CELLS")
    dip = plan([(n, 2, _s16(2 * n), 3) for n in range(2100, 2300)])
    first_parse = 2100 + [r[0] for r in dip].index("PARSE")
    assert hap[first_cells - 2900 - 1][0] == "CELLS3" and dip[first_parse - 2100 - 1][0] != "PARSE"
    return first_cells, first_parse - 1, first_parse


def by_size():
    """layouts that change the route by their size alone (column counts from the plan function; the shuffled layout wants two
    thirds of its columns: with half as many columns again k_tok_cells' table is as large as the first k_tok_parse layout's and its
    rows hold as many slots)"""
    first_cells, last_second, first_parse = size_edges()
    return [grid_spec("haplo", "all", first_cells, 17, "-lds3"), grid_spec("haplo", "all", first_cells - 1, 17, "-lds3"),
            grid_spec("phased2", "all", last_second, 70, "-lds"), grid_spec("phased2", "all", first_parse, 70, "-lds"),
            grid_spec("phased2", "shuf", 3 * first_parse // 2 + 8, 17, "-lds")]


def regular():
    return grid() + seam() + heads() + general() + by_size()


# ---- refusals: a regular text and twins of it with one defect each ---------------------------------------------------------------------
def refusal_bases():
    """a base per route: k_tok_cells3<DIPLO | PHASED | PAIRS, 0 .. 4>, k_tok_cells (wide wanted cell, wide unwanted column),
    k_tok_parse; 33 lines: rows 0, 15, 16 and 32 are the first and the last of a wavefront's lines and the first of the next's"""
    first_parse = size_edges()[2]
    return [grid_spec("haplo", "all", 64, 33, "-ref"), grid_spec("phased2", "shuf", 65, 33, "-ref"), grid_spec("diplo", "all", 129, 33, "-ref"),
            grid_spec("pairs123", "shuf", 200, 33, "-ref"), grid_spec("phased12", "all", 300, 33, "-ref"),
            grid_spec("phasedwide", "shuf", 65, 33, "-ref"), [s for s in general() if s.name == "unwanted7-all-c65-l17"][0],
            grid_spec("phased2", "all", first_parse, 33, "-ref")]


DEFECTS = ("short", "tabtab", "blank", "nosep")


def twins(case):
    """[(label, kind, column or -1, text)]: the case's text with one defect.  short: a cell one character short; tabtab: a doubled tab behind a cell;
    blank: a blank in place of a character of a cell; nosep (not the last column): a letter in place of the blank behind a cell --
    the last two keep the line's length, so only the cell kernels can see them.  At column 0, 63, 64 and the last, in rows 0, 15,
    16 and the last; a position of 19 digits and a `#` line besides"""
    t, L, n_cols = case.text, case.n_lines, case.n_cols
    rng = np.random.default_rng(case.spec.seed + 5)
    out = []
    for c in sorted({0, 63, 64, n_cols - 1} & set(range(n_cols))):
        for r in sorted({0, 15, 16, L - 1} & set(range(L))):
            a = case.cells_at[r] + int(case.off[c])
            w = int(case.width[c])
            k = int(rng.integers(0, w))
            for d in DEFECTS:
                if d == "short":
                    x = t[:a + k] + t[a + k + 1:]
                elif d == "tabtab":
                    x = t[:a + w] + b"\t" + t[a + w:]
                elif d == "blank":
                    x = t[:a + k] + (b" ", b"\t")[(r + c) % 2] + t[a + k + 1:]
                elif c + 1 < n_cols:
                    x = t[:a + w] + b"A" + t[a + w + 1:]
                else:
                    continue
                out.append(("%s-c%d-r%d" % (d, c, r), d, c, x))
    for r in sorted({0, 16 % L}):
        a, e = case.line_at[r], case.cells_at[r]
        head = t[a:e].split(b"\t")
        out.append(("pos19-r%d" % r, "pos19", -1, t[:a] + head[0] + b"\t1234567890123456789\t" + t[e:]))
        out.append(("comment-r%d" % r, "comment", -1, t[:a] + b"#" + t[a + 1:]))
        out.append(("comment-line-r%d" % r, "comment-line", -1, t[:a] + b"# a comment\n" + t[a:]))
    return out


def is_regular(text, n_cols):
    """the regularity rule of the device tokenizer (csrc/pg_tokenize.hip's header), spelt out on its own: every line is scaffold,
    blanks, a position of at most 18 digits with an optional sign, blanks, then n_cols cells of the first line's widths with ONE
    blank between them; no `#` line, no empty line"""
    to_tab = bytes.maketrans(b" \r\v\f", b"\t\t\t\t")
    widths = None
    if not text.endswith(b"\n"):
        return False
    for ln in text[:-1].translate(to_tab).split(b"\n"):
        ln = ln.lstrip(b"\t")
        if not ln or ln[:1] == b"#":
            return False
        scaffold, _, rest = ln.partition(b"\t")
        num, _, rest = rest.lstrip(b"\t").partition(b"\t")
        num = num[1:] if num[:1] in (b"+", b"-") else num
        if not num.isdigit() or len(num) > 18:
            return False
        w = [len(x) for x in rest.lstrip(b"\t").split(b"\t")]
        if len(w) != n_cols or min(w) < 1 or (widths is not None and w != widths):
            return False
        widths = w
    return True


# ---- a case on the device (tests/test_gpu_tokenize.py and the processes it starts) -----------------------------------------------------
SENTINEL = 8


def check_on_device(e, c, row_offset=37, behind=9, text=None, set_layout=True):
    """c's text through Engine.tokenize_text into rows row_offset .. of a reservation filled with a sentinel: the rows, positions
    and runs are the case's, the rows in front of and behind them still hold the sentinel"""
    L, H = c.n_lines, c.lay.n_hap
    if set_layout:
        e.set_layout(c.lay)
        e.reserve(row_offset + L + behind + 1)
    e.upload(np.full((row_offset + L + behind, H), SENTINEL, dtype=np.int8), 0)
    got = e.tokenize_text(c.text if text is None else text, row_offset=row_offset, n_rows=L)
    assert got is not None, "%s: a regular text refused by the device tokenizer" % c.name
    n, pos, run_starts, run_names = got
    assert n == L, (c.name, n, L)
    rows = e.download(0, row_offset + L + behind)
    diff = np.argwhere(rows[row_offset:row_offset + L] != c.rows)
    assert len(diff) == 0, "%s: %d cells differ, the first at row %d slot %d: %d for %d" % (
        c.name, len(diff), diff[0][0], diff[0][1], rows[row_offset + diff[0][0], diff[0][1]], c.rows[diff[0][0], diff[0][1]])
    assert np.array_equal(pos, c.pos), c.name
    assert np.array_equal(run_starts, c.run_starts) and list(run_names) == c.run_names, (c.name, run_starts, run_names)
    assert (rows[:row_offset] == SENTINEL).all(), "%s: rows in front of the block were written" % c.name
    assert (rows[row_offset + L:] == SENTINEL).all(), "%s: rows behind the block were written" % c.name
