"""Seeded VCF files for the parseVCF drop-in's device route -- k_vcf_heads / k_vcf_cells / k_rows_scan of csrc/pg_vcf_dev.hip -- at the
sizes where the cell kernel's lanes, steps and blocks turn over.  A generator that writes regular VCF lines and keeps what it knows of
each (chrom, pos, allele strings, per sample the allele indices or "missing" and the phase character), a model that makes the expected
`.geno` rows from that knowledge alone (neither parser is asked), and the geometry of the kernel's tab scan worked out from the text.
No GPU and no native library.  tests/test_vcf_cell_cases.py shows on the CPU that the cases contain what they are built for;
tests/test_gpu_vcf_cells.py runs the device over them.

LANES      40 lines, every 4th an indel line: 1, 2, 63, 64, 65, 128, 129 columns all selected; 200 columns with -s naming 63, 64, 65,
           129 of them in reversed header order and scattered; 65 and 129 columns with ploidy 1 on every third sample
STEPS      for B in 1024, 2048: every section length S in [B - 24, B + 24] x all 16 residues of (ls + cells_off), one line each
ALIGN      three section shapes (3 columns GT:DP; one diploid column, 3 bytes; one haploid column, 1 byte) x all 16 residues
EXTRA      lines with more columns than the header names (blanks among them, a trailing tab, the n_cols-th tab on both sides of the
           first 1024-byte step), a byte >= 0x80 in a cell piece nobody reads
HOSTLINES  one line the device hands over in the middle of a file of several blocks
WAVES      3840, 3841, 7680, 7681, 14000 columns x 1, 2, 3, 4, 5, 9 lines; 14001 columns stay on the host
ROOM       a row longer than its line inside the output's room, and one far beyond it
SCAN       255 .. 2049 lines of 3 columns with comment lines and lines --minQual drops in between

The scan of a line: 16-byte words from the aligned address below cells_off, 1024 bytes a step.  With b = the residue of the block's
first byte, A = (b + ls + cells_off) % 16 is the section's place in its first word; the scan walks A + S bytes, and a byte at section
offset d has walk offset A + d."""
import functools

import numpy as np

HEAD9 = "#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT"
MIN_QUAL = 30                                      # (the sets that drop lines run with --minQual 30: QUAL 10 is dropped, 50 kept)
BASES = "ACGT"


# ---- generator -------------------------------------------------------------------------------------------------------------------
def sample_names(n):
    return ["s%d" % k for k in range(n)]


def make_line(rng, pos, n_cols, indel=False, ploidy=None, fmt="GT:DP", miss=0.10, pad=0, qual=50, alleles=None, calls=None,
              chrom="chr1", high_byte=False, missing_at=()):
    """one regular data line (str, latin-1) and what is known of it.  pad: bytes of a third piece of the first cell that FORMAT does
    not name (`0/1:12:7777`): the sample section grows, the row does not change.  calls: a fixed (indices, phase) for every sample"""
    if alleles is None:
        if indel:
            alleles = [["A", "ACG"], ["ACG", "A"], ["A", "ACGT", "C"], ["GT", "G", "GTTT"]][int(rng.integers(0, 4))]
        else:
            ref = int(rng.integers(0, 4))
            alleles = [BASES[ref], BASES[(ref + 1 + int(rng.integers(0, 3))) % 4]]
            if rng.random() < 0.2:
                alleles.append([x for x in BASES if x not in alleles][0])
    n_all = len(alleles)
    a = rng.integers(0, n_all, size=(n_cols, 2))
    phased = rng.random(n_cols) < 0.3
    missing = rng.random(n_cols) < miss
    dp = rng.integers(0, 100, size=n_cols)
    with_dp = ":" in fmt
    cells, known = [], []
    for c in range(n_cols):
        pl = 2 if ploidy is None else ploidy[c]
        ph = "|" if (phased[c] and pl == 2) else "/"
        if calls is not None:
            idx, ph = calls
            idx = tuple(idx[:pl])
        elif missing[c] or c in missing_at:
            idx = (None,) * pl
        else:
            idx = tuple(int(x) for x in a[c, :pl])
        cell = ph.join("." if i is None else str(i) for i in idx)
        if with_dp:
            cell += ":%d" % dp[c]
            if high_byte and c == n_cols // 2:
                cell += "\xe9"                              # a byte >= 0x80 in the DP piece: nobody reads it without --gtf
        known.append((idx, ph))
        cells.append(cell)
    if pad:
        assert with_dp
        cells[0] += ":" + "7" * (pad - 1)
    line = "\t".join([chrom, str(pos), ".", alleles[0], ",".join(alleles[1:]), str(qual), "PASS", ".", fmt] + cells)
    return line, dict(chrom=chrom, pos=pos, alleles=alleles, calls=known, kept=qual >= MIN_QUAL, indel=indel)


def comment_of(n):
    """a line the parsers skip that takes n >= 1 bytes of the block, line feed included"""
    return "" if n == 1 else "#" + "x" * (n - 2)


class Writer:
    """lines with the truth beside them (None beside a comment line) and the block offset of the next line"""

    def __init__(self):
        self.lines, self.truth, self.at = [], [], 0

    def add(self, line, truth=None):
        self.lines.append(line)
        self.truth.append(truth)
        self.at += len(line) + 1

    def add_at_residue(self, line, truth, needed):
        """the line placed so that (ls + cells_off) % 16 is one of `needed`: as it comes where that holds, else behind a comment line of
        the right length; returns the residue taken"""
        co = cells_off_of(line)
        r = (self.at + co) % 16
        if r not in needed:
            want = min(needed, key=lambda x: (x - r) % 16)
            n = (want - r) % 16
            self.add(comment_of(n if n > 1 else 17))
            r = (self.at + co) % 16
            assert r == want
        self.add(line, truth)
        return r


def finish(name, w, n_cols, argv=(), sel=None, ploidy=None, sep="\t", missing="N", add_ref=False, env=None, **more):
    names = sample_names(n_cols)
    sel = list(range(n_cols)) if sel is None else list(sel)
    argv = list(argv)
    if sel != list(range(n_cols)):
        argv += ["-s", ",".join(names[c] for c in sel)]
    ploidy_file = None
    if ploidy is not None:
        ploidy_file = "".join("%s %d\n" % (names[c], ploidy[c]) for c in range(n_cols) if ploidy[c] != 2)
        argv += ["--ploidyFile", "{ploidy}"]
    if sep != "\t":
        argv += ["--outSep", sep]
    if missing != "N":
        argv += ["--missing", missing]
    if add_ref:
        argv += ["--addRefTrack"]
    head = ("##fileformat=VCFv4.2\n" + HEAD9 + "\t" + "\t".join(names) + "\n").encode()
    body = ("\n".join(w.lines) + "\n").encode("latin-1")
    case = dict(name=name, names=names, head=head, body=body, lines=w.lines, truth=w.truth, argv=argv, sel=sel, sep=sep, missing=missing,
                add_ref=add_ref, ploidy_file=ploidy_file, n_cols=n_cols, env=dict(env or {}))
    case.update(more)
    return case


def argv_of(case, tmp_dir):
    """the case's arguments, its ploidy file written into tmp_dir"""
    import os
    path = os.path.join(str(tmp_dir), "ploidy.txt")
    if case["ploidy_file"] is not None:
        with open(path, "w") as f:
            f.write(case["ploidy_file"])
    return [a.format(ploidy=path) for a in case["argv"]]


# ---- model -----------------------------------------------------------------------------------------------------------------------
def model(truth, selected_columns, sep, missing, add_ref=False):
    """the `.geno` rows of the kept lines: chrom sep pos [sep REF], then per selected sample -- in the order of -s -- the allele strings
    joined by the phase character, the missing character once per allele of a missing call; a line feed"""
    rows = []
    for t in truth:
        if t is None or not t["kept"]:
            continue
        al = t["alleles"]
        parts = [t["chrom"], str(t["pos"])] + ([al[0]] if add_ref else [])
        for c in selected_columns:
            idx, phase = t["calls"][c]
            parts.append(phase.join(missing if i is None else al[i] for i in idx))
        rows.append(sep.join(parts) + "\n")
    return "".join(rows).encode("latin-1")


def expected(case):
    return model(case["truth"], case["sel"], case["sep"], case["missing"], case["add_ref"])


def header_row(case):
    names = case["names"]
    return (case["sep"].join(["#CHROM", "POS"] + (["REF"] if case["add_ref"] else []) + [names[c] for c in case["sel"]]) + "\n").encode()


# ---- geometry --------------------------------------------------------------------------------------------------------------------
def cells_off_of(line):
    """the offset behind the ninth tab"""
    at = -1
    for _ in range(9):
        at = line.index("\t", at + 1)
    return at + 1


def geometry(lines):
    """per data line (comment and empty lines: None): ls = its offset in the block, cells_off, S = line_len - cells_off, tabs = the
    section offsets of the tabs behind cells_off"""
    out, at = [], 0
    for ln in lines:
        if ln == "" or ln.startswith("#"):
            out.append(None)
        else:
            co = cells_off_of(ln)
            sec = ln[co:]
            out.append(dict(ls=at, cells_off=co, S=len(sec), tabs=[k for k, ch in enumerate(sec) if ch == "\t"]))
        at += len(ln) + 1
    return out


def A_of(g, b):
    """the section's first byte in its 16-byte word, the block's first byte at residue b"""
    return (b + g["ls"] + g["cells_off"]) % 16


def walk_tabs(g, b):
    """the walk offsets of the section's tabs"""
    a = A_of(g, b)
    return [a + d for d in g["tabs"]]


def wpb_of(n_vcf_samples):
    """lines (wavefronts) per block of k_vcf_cells: the tab positions of 4, 2 or 1 lines in 60 KiB of LDS, 4 bytes a column"""
    per = n_vcf_samples * 4
    return 4 if per * 4 <= 60 * 1024 else (2 if per * 2 <= 60 * 1024 else 1)


def out_cap_of(case):
    """the room the device route gives a block's rows: text + n_lines * (plain_cells + 64) + 4096"""
    calls = next(t for t in case["truth"] if t is not None)["calls"]
    plain = sum(2 * len(calls[c][0]) for c in case["sel"])
    return len(case["body"]) + len(case["lines"]) * (plain + 64) + 4096


# ---- the case sets ---------------------------------------------------------------------------------------------------------------
def _plain_file(seed, n_cols, n_lines, indel_every, ploidy=None, indel_at=None, missing_at=()):
    rng = np.random.default_rng(seed)
    w = Writer()
    for k in range(n_lines):
        indel = (k % indel_every == indel_every - 1) if indel_at is None else k == indel_at
        w.add(*make_line(rng, 1000 + 3 * k, n_cols, indel=indel, ploidy=ploidy, missing_at=missing_at if k == 0 else ()))
    return rng, w


LANES_ALL = [1, 2, 63, 64, 65, 128, 129]
LANES_SEL = [63, 64, 65, 129]
LANES_PL = [65, 129]
LANES = (["all_%d" % n for n in LANES_ALL] + ["%s_%d" % (how, n) for n in LANES_SEL for how in ("rev", "scat")] +
         ["pl_%d" % n for n in LANES_PL])


@functools.lru_cache(maxsize=None)
def lanes(name):
    how, n = name.split("_")
    n = int(n)
    if how == "all":
        _, w = _plain_file(8100 + n, n, 40, 4)
        return finish("lanes_" + name, w, n)
    if how in ("rev", "scat"):
        rng, w = _plain_file(8300 + n + (500 if how == "scat" else 0), 200, 40, 4)
        pick = rng.choice(200, size=n, replace=False)
        sel = sorted(int(x) for x in pick)[::-1] if how == "rev" else [int(x) for x in pick]
        return finish("lanes_" + name, w, 200, sel=sel)
    ploidy = [1 if c % 3 == 2 else 2 for c in range(n)]          # cell_off strides of 2 and 4 mixed across the 64th lane
    _, w = _plain_file(8700 + n, n, 40, 4, ploidy=ploidy)
    if n == 129:
        return finish("lanes_" + name, w, n, ploidy=ploidy, sep=",", missing="?", add_ref=True)
    return finish("lanes_" + name, w, n, ploidy=ploidy)


ALIGN = ["cols3", "dip1", "hap1"]


def _fill_residues(w, make, rounds=1):
    """lines of make() until (ls + cells_off) % 16 has taken each of its 16 values `rounds` times: as they fall while that serves, else
    behind a comment line of the right length -- and behind a comment line four lines as they fall, so that at least four lines in
    five stay data lines"""
    need = {r: rounds for r in range(16)}
    free = 0
    while need:
        line, t = make()
        r = (w.at + cells_off_of(line)) % 16
        if r in need:
            w.add(line, t)
        elif free > 0:
            w.add(line, t)
            free -= 1
        else:
            r = w.add_at_residue(line, t, set(need))
            free = 4
        if r in need:
            need[r] -= 1
            if not need[r]:
                del need[r]


def _fill_shapes(w, rng, shapes, n_cols, tails=None):
    """for every section length in `shapes` a line at each of the 16 residues of (ls + cells_off): a line is drawn, the shape it takes is
    one that still wants the residue it falls on (its first cell padded to that length); a comment line only where none does"""
    needed = {s: set(range(16)) for s in shapes}
    k = 0
    while needed:
        state = rng.bit_generator.state
        line, _ = make_line(rng, 100 + k, n_cols, indel=k % 5 == 4)
        co = cells_off_of(line)
        s0, r = len(line) - co, (w.at + co) % 16
        S = next((s for s in needed if r in needed[s]), next(iter(needed)))
        assert s0 <= S
        rng.bit_generator.state = state                         # the same line again, its first cell padded to S bytes of section
        line, t = make_line(rng, 100 + k, n_cols, indel=k % 5 == 4, pad=S - s0)
        assert len(line) - co == S
        t["shape"] = S
        if tails:
            line += tails[k % len(tails)]
        needed[S].discard(w.add_at_residue(line, t, needed[S]))
        if not needed[S]:
            del needed[S]
        k += 1


@functools.lru_cache(maxsize=None)
def align(name):
    """every residue of (ls + cells_off) three times over, a comment line where the lines do not fall so by themselves"""
    rng = np.random.default_rng({"cols3": 8801, "dip1": 8802, "hap1": 8803}[name])
    n_cols, fmt, ploidy = {"cols3": (3, "GT:DP", None), "dip1": (1, "GT", None), "hap1": (1, "GT", [1])}[name]
    w = Writer()
    k = [0]

    def make():
        k[0] += 1
        return make_line(rng, 100 + 7 * k[0], n_cols, indel=k[0] % 5 == 4, ploidy=ploidy, fmt=fmt, miss=0.15)
    _fill_residues(w, make, rounds=3)
    want_s = {"cols3": None, "dip1": 3, "hap1": 1}[name]
    return finish("align_" + name, w, n_cols, argv=["--ploidy", "1"] if name == "hap1" else [], section_bytes=want_s)


STEPS = [1024, 2048]
STEPS_SPAN = 24
STEPS_COLS = {1024: 140, 2048: 285}                 # at most 7 bytes a column (`0/1:12` + tab): below B - 24 before the padding


@functools.lru_cache(maxsize=None)
def steps(B):
    rng = np.random.default_rng(8900 + B)
    w = Writer()
    _fill_shapes(w, rng, list(range(B - STEPS_SPAN, B + STEPS_SPAN + 1)), STEPS_COLS[B])
    return finish("steps_%d" % B, w, STEPS_COLS[B])


EXTRA = ["misc", "exit"]
EXTRA_EXIT_COLS = 140
EXTRA_KINDS = ["space_near", "space_far", "trailing_tab", "high_byte", "plain", "two_extra"]


@functools.lru_cache(maxsize=None)
def extra(name):
    """lines with more columns than the header names: rows from the named columns, nothing handed over"""
    rng = np.random.default_rng({"misc": 9001, "exit": 9002}[name])
    w = Writer()
    if name == "misc":
        n_cols = 5
        k = [0]
        for kind in EXTRA_KINDS:
            def make():
                k[0] += 1
                line, t = make_line(rng, 100 + 3 * k[0], n_cols, indel=k[0] % 4 == 3, high_byte=kind == "high_byte")
                if kind == "space_near":
                    line += "\tx y"                             # the space two bytes behind the tab that ends the last named column
                elif kind == "space_far":
                    line += "\t" + "x" * 2999 + " y"            # 3000 bytes behind it: in a later step of the scan
                elif kind == "trailing_tab":
                    line += "\t"
                elif kind == "two_extra":
                    line += "\t0/1:3\t \t"
                t["kind"] = kind
                return line, t
            _fill_residues(w, make)
        return finish("extra_misc", w, n_cols)
    # the n_cols-th tab at section offset D: walk offset A + D = 1023 or 1024 for every A
    _fill_shapes(w, rng, list(range(1024 - 16, 1024 + 1)), EXTRA_EXIT_COLS, tails=["\t0/1:7", "\tx y\tz", "\t", "\t0/0:1\t \t1/1"])
    return finish("extra_exit", w, EXTRA_EXIT_COLS)


HOST_COLS = 8
HOST_LINES = 60
HOST_AT = 30
HOSTLINES = (["space_end_last", "vtab_in_cell", "x1f_in_cell", "empty_col", "col_fewer"] + ["blank_r%d" % r for r in range(16)])
HOST_STREAM_BYTES = "500"


@functools.lru_cache(maxsize=None)
def hostline(name):
    """one line only the host reads, in the middle of a file of several blocks.  Every planted line is one the host parser reads
    without complaint whichever way it splits at the blank -- a blank inside a cell is followed by a whole genotype (`0/1`) -- or
    one it stops at in words of its own (a named column missing: case["raises"])."""
    rng = np.random.default_rng(9100 + HOSTLINES.index(name))
    w = Writer()
    sel = None
    for k in range(HOST_LINES):
        line, t = make_line(rng, 100 + 3 * k, HOST_COLS, indel=k % 6 == 5)
        if k == HOST_AT:
            f = line.split("\t")
            if name == "space_end_last":
                f[-1] += " "
            elif name == "vtab_in_cell":
                f[9 + 4] += ":7\x0b0/1"
            elif name == "x1f_in_cell":
                f[9 + 2] += ":7\x1f0/1"
            elif name == "empty_col":
                f[9 + 3] = ""
            elif name == "col_fewer":
                f = f[:-1]
            else:
                # the blank at section offset 3, (ls + cells_off) % 16 = r: its place in the scan's words runs through all 16 with r.  The
                # first column is not selected: only the tab scan sees the blank
                f[9] = "0/1\x0b0/1"
                sel = list(range(1, HOST_COLS))
                line = "\t".join(f)
                w.add_at_residue(line, t, {int(name[7:])})
                continue
            line = "\t".join(f)
        w.add(line, t)
    # (str.split() finds one column fewer than the header names in these two: the host parser ends the run with that message)
    raises = "fewer columns" if name in ("empty_col", "col_fewer") else None
    return finish("host_" + name, w, HOST_COLS, sel=sel, env={"PG_STREAM_BYTES": HOST_STREAM_BYTES}, raises=raises)


def planted_line(case):
    """the index (in the block of the whole body) of the line only the host reads"""
    hits = [i for i, ln in enumerate(case["lines"]) if not ln.startswith("#") and ln and
            ("\x0b" in ln or "\x1f" in ln or " " in ln or "\t\t" in ln or ln.count("\t") != 8 + case["n_cols"])]
    assert len(hits) == 1
    return hits[0]


WAVES_COLS = [3840, 3841, 7680, 7681, 14000]
WAVES_LINES = [1, 2, 3, 4, 5, 9]
WAVES_TOO_MANY = 14001


@functools.lru_cache(maxsize=8)
def waves(n_cols, n_lines):
    _, w = _plain_file(9200 + n_cols % 1000 + n_lines, n_cols, n_lines, 0, indel_at=n_lines // 2, missing_at=(1,))
    # column 0 starts at cells_off, the last column ends at line_len and not at a tab
    sel = [n_cols - 1, 0, n_cols // 2, 64, 1, n_cols - 2]
    return finish("waves_%d_%d" % (n_cols, n_lines), w, n_cols, sel=sel)


ROOM = ["fits", "overflows"]
ROOM_ALT = {"fits": 40, "overflows": 3000}


@functools.lru_cache(maxsize=None)
def room(name):
    rng = np.random.default_rng(9300)
    w = Writer()
    for k in range(20):
        if k == 7:
            w.add(*make_line(rng, 1000 + 3 * k, 50, indel=True, alleles=["A", "A" + "C" * ROOM_ALT[name]], calls=((1, 1), "/")))
        else:
            w.add(*make_line(rng, 1000 + 3 * k, 50))
    return finish("room_" + name, w, 50)


SCAN = [255, 256, 257, 1023, 1024, 1025, 2049]


@functools.lru_cache(maxsize=None)
def scan(n_lines):
    """n_lines lines in all: two in thirteen have no row (a comment line, a line --minQual drops), side by side, so that over the
    file they stand at every place of a stretch of 1, 2 or 3 lines of k_rows_scan"""
    rng = np.random.default_rng(9400 + n_lines)
    w = Writer()
    for k in range(n_lines):
        if k % 13 == 5:
            w.add(comment_of(2 + k % 9))
        else:
            w.add(*make_line(rng, 100 + 2 * k, 3, indel=k % 7 == 6, qual=10 if k % 13 == 6 else 50))
    return finish("scan_%d" % n_lines, w, 3, argv=["--minQual", str(MIN_QUAL)])


def regular_cases():
    """(id, builder) of every set the device takes whole"""
    out = [("lanes_" + n, functools.partial(lanes, n)) for n in LANES]
    out += [("align_" + n, functools.partial(align, n)) for n in ALIGN]
    out += [("steps_%d" % B, functools.partial(steps, B)) for B in STEPS]
    out += [("extra_" + n, functools.partial(extra, n)) for n in EXTRA]
    out += [("waves_%d_%d" % (c, n), functools.partial(waves, c, n)) for c in WAVES_COLS for n in WAVES_LINES]
    out += [("room_fits", functools.partial(room, "fits"))]
    out += [("scan_%d" % n, functools.partial(scan, n)) for n in SCAN]
    return out
