"""Seeded `.geno` files for the mergeGeno.py drop-in's device route -- the kernels of csrc/pg_merge_dev.hip -- at the sizes where the
64-byte steps of k_merge_keys and k_merge_emit and the probes of the .fai table turn over.  A generator that writes the files and keeps
what it knows of them: per line its length, the offsets of its first two tabs and its number of 64-byte steps; per file the bytes it
adds to a written line; where it applies the .fai table's slots and the chain a name walks.  No GPU, no native library and nothing of
the engine: the expected bytes are tests/merge_model.py's.  tests/test_merge_edge_cases.py shows on the CPU that the cases contain
what they are built for; tests/test_gpu_merge_edges.py runs the device over them.

NAMES   scaffold names of 1, 62, 63, 64, 65, 127, 128, 129 bytes (the first tab stands there); names of 60 and 124 bytes with positions
        of 2, 3 and 4 digits (the second tab at 63, 64, 65 and 127, 128, 129); a second name of the same length and starting slot that
        differs in its last byte; intersect, union and all (sites no file holds: the head rendered from the .fai)
TWINS   .fai name sets found by a seeded search with a port of pgm_hash and the table build: (a) (b) two names of one length on one
        starting slot that differ in one byte behind the first step / in byte 0, (c) a chain from the last slot to slot 0, (d) a line
        whose name is in no slot but passes an entry of its length: the stopping line
WIDTH   lines of 63 .. 193 bytes made of 30 to 90 one-character cells; one file with all the lengths in turn; a bare file
SEAMS   one irregular line whose defect stands on a step's seam, and its regular twin
DUMMY   dummy-cell runs of (header cells, --missing bytes) around 64 bytes, behind another file's part; --missing of 65 bytes
CELLS   a held file's part of 63 .. 300 bytes in each of three file positions, --outSep ,
DIGITS  one scaffold of 100 010 positions under --method all
LINES   files of 1 .. 1025 lines"""
import os
import zlib

import numpy as np

LETTERS = "ACGTN/|-*acgt."
NAME_CHARS = "abcdefghijklmnopqrstuvwxyzABCDEFGHIJKLMNOPQRSTUVWXYZ0123456789_"
M32 = 0xFFFFFFFF


# ---- the name hash and the .fai table of csrc/pg_merge_core.h / pg_merge_dev_config, in Python ------------------------------------
def hash_byte(b, k):
    x = ((b + 1) * 0x9E3779B1 + k * 0x85EBCA6B) & M32
    x ^= x >> 15
    x = (x * 0x2C1B3C6D) & M32
    x ^= x >> 12
    return x


def hash_end(total, length):
    x = (total + length * 0xC2B2AE35) & M32
    x ^= x >> 16
    x = (x * 0x7FEB352D) & M32
    x ^= x >> 15
    return x


def name_hash(name):
    total = 0
    for k, b in enumerate(name):
        total = (total + hash_byte(b, k)) & M32
    return hash_end(total, len(name) & M32)


def table_size(n_fai):
    size = 4
    while size < 2 * n_fai:
        size <<= 1
    return size


def build_table(names, hash_fn=name_hash):
    """the open-addressed table over the .fai's names (bytes): size 4, doubled while below 2 x n_fai, linear probing in .fai order"""
    size = table_size(len(names))
    table = [-1] * size
    for s, name in enumerate(names):
        at = hash_fn(name) & (size - 1)
        while table[at] >= 0:
            at = (at + 1) & (size - 1)
        table[at] = s
    return table


def chain(table, names, name, hash_fn=name_hash):
    """(the slots a look-up of `name` visits, the index it finds or -1)"""
    mask = len(table) - 1
    at = hash_fn(name) & mask
    slots = []
    while True:
        slots.append(at)
        e = table[at]
        if e < 0:
            return slots, -1
        if names[e] == name:
            return slots, e
        at = (at + 1) & mask


# ---- writing a case and what is known of it ----------------------------------------------------------------------------------------
def _rng(tag):
    return np.random.default_rng(zlib.crc32(tag.encode()))


def _word(rng, n, chars=NAME_CHARS):
    return "".join(chars[int(k)] for k in rng.integers(0, len(chars), size=n))


def _cell(rng, lo=1, hi=5):
    return _word(rng, int(rng.integers(lo, hi + 1)), LETTERS)


def geometry(line):
    """of one data line without its line feed: length, the first two tabs, the tab count, the 64-byte steps of k_merge_keys"""
    tabs = [k for k, c in enumerate(line) if c == "\t"]
    return dict(n=len(line), t0=tabs[0] if tabs else None, t1=tabs[1] if len(tabs) > 1 else None, ntab=len(tabs), steps=(len(line) + 63) // 64)


def _finish(directory, tag, fai_rows, files, method, missing="N", out_sep="\t", cut=None, **more):
    """writes the .fai (name, length) and the files (sample names, data lines); returns (argv, facts).  cut: {file: line} -- from that
    line on the file gives nothing (a stopping line).  facts: lines[f] = the geometry of every data line; held[f] =
    {(scaffold name, position): bytes the file adds to the written line}; n_cells[f]; what the caller adds"""
    fai = os.path.join(directory, tag + ".fai")
    with open(fai, "w") as f:
        f.write("".join("%s\t%d\n" % row for row in fai_rows))
    paths, lines_geo, held, n_cells, longest = [], [], [], [], 0
    for x, (samples, lines) in enumerate(files):
        path = os.path.join(directory, "%s_%d.geno" % (tag, x))
        with open(path, "w") as f:
            f.write("\t".join(["#CHROM", "POS"] + list(samples)) + "\n" + "".join(ln + "\n" for ln in lines))
        paths.append(path)
        geo = [geometry(ln) for ln in lines]
        mine = {}
        for k, (ln, g) in enumerate(zip(lines, geo)):
            if cut and x in cut and k >= cut[x]:
                break
            fields = ln.split("\t")
            mine[(fields[0], int(fields[1]))] = g["n"] - (g["t1"] if samples else g["n"])
        lines_geo.append(geo)
        held.append(mine)
        n_cells.append(len(samples))
        longest = max([longest] + [g["n"] + 1 for g in geo])
    argv = sum([["-i", p] for p in paths], []) + ["-f", fai, "--method", method]
    if missing != "N":
        argv += ["--missing", missing]
    if out_sep != "\t":
        argv += ["--outSep", out_sep]
    facts = dict(lines=lines_geo, held=held, n_cells=n_cells, missing_len=len(missing), out_sep=out_sep, fai=[r[0] for r in fai_rows],
                 stopped_files=0, handed_back=False, device_takes=True, parts_known=True, stream=None,
                 few_lines_stream=len(files) * 3 * longest)       # PG_STREAM_BYTES of three of the longest lines a file
    facts.update(more)
    return argv, facts


def written_parts(facts, want):
    """per written line of the model's bytes: (scaffold name, bytes of the head, [(output offset, bytes, dummy?) per file], the line's
    length without its line feed) -- from what the generator knows of the files"""
    sep = facts["out_sep"]
    rows = []
    for line in want.decode().split("\n")[1:-1]:
        name, pos = line.split(sep)[:2]
        w = len(name) + 1 + len(pos)
        parts = []
        for mine, cells in zip(facts["held"], facts["n_cells"]):
            n = mine.get((name, int(pos)))
            dummy = n is None
            n = cells * (1 + facts["missing_len"]) if dummy else n
            parts.append((w, n, dummy))
            w += n
        rows.append((name, len(name) + 1 + len(pos), parts, len(line)))
    return rows


def _random_lines(rng, sites, n_samples, keep, lo=1, hi=5):
    return ["\t".join([s, str(p)] + [_cell(rng, lo, hi) for _ in range(n_samples)]) for s, p in sites if rng.random() < keep]


# ---- NAMES -------------------------------------------------------------------------------------------------------------------------
NAME_LENS = (1, 62, 63, 64, 65, 127, 128, 129)
SECOND_TAB = {60: (63, 64, 65), 124: (127, 128, 129)}         # name bytes: where the second tab stands with 2, 3, 4 digits
METHODS = ("intersect", "union", "all")


def names(length, method, directory):
    tag = "names_%d_%s" % (length, method)
    rng = _rng(tag)
    main = _word(rng, length)
    twin = next(t for t in (main[:-1] + c for c in NAME_CHARS)      # the same starting slot: a look-up of the twin passes `main`
                if t != main and name_hash(t.encode()) & 7 == name_hash(main.encode()) & 7)
    if length in SECOND_TAB:
        n_pos = 1100
        pos = sorted(set([10, 11, 57, 98, 99, 100, 101, 500, 998, 999, 1000, 1001, 1100] + rng.integers(10, 1100, size=12).tolist()))
    else:
        n_pos = 30
        pos = sorted(set(rng.choice(np.arange(1, n_pos), size=14, replace=False).tolist() + [n_pos]))
    fai = [(main, n_pos), ("mid", 25), (twin, n_pos)]
    sites = [(main, p) for p in pos] + [("mid", p) for p in (1, 7, 25)] + [(twin, p) for p in pos]
    n_files = 2 + (NAME_LENS + tuple(SECOND_TAB)).index(length) % 2
    files = []
    for x in range(n_files):
        n_samples = int(rng.integers(1, 4))
        files.append((["n%ds%d" % (x, k) for k in range(n_samples)], _random_lines(rng, sites, n_samples, 0.8)))
    steps = {1: {1}, 60: {2}, 62: {2}, 63: {2}, 64: {2}, 65: {2}, 124: {3}, 127: {3}, 128: {3}, 129: {3}}[length]
    return _finish(directory, tag, fai, files, method, want_t0=length, want_t1=set(SECOND_TAB.get(length, ())), want_steps=steps)


NAMES = [("names_%d_%s" % (n, m), (lambda d, n=n, m=m: names(n, m, d))) for n in NAME_LENS + tuple(SECOND_TAB) for m in METHODS]


# ---- TWINS -------------------------------------------------------------------------------------------------------------------------
def _twins_search(kind):
    """the .fai names of the set, the name the files' sites use, and for (d) the name of the stopping line (in no slot)"""
    rng = _rng("twins_" + kind)
    for _ in range(100000):
        if kind in ("a", "b"):
            base = _word(rng, 70)
            at = 66 if kind == "a" else 0
            other = base[:at] + NAME_CHARS[(NAME_CHARS.index(base[at]) + 1 + int(rng.integers(0, 60))) % len(NAME_CHARS)] + base[at + 1:]
            fai = [base, "t2", other]
            if other != base and name_hash(base.encode()) & 7 == name_hash(other.encode()) & 7:
                return fai, other, None
        elif kind == "c":
            first, second = _word(rng, 68), _word(rng, 68)
            fai = [first, second, "t3"]
            table = build_table([n.encode() for n in fai])
            if name_hash(first.encode()) & 7 == 7 and name_hash(second.encode()) & 7 == 7 and table[0] == 1:
                return fai, second, None
        else:
            base = _word(rng, 70)
            ghost = base[:66] + ("q" if base[66] != "q" else "r") + base[67:]
            fai = [base, "t2"]
            table = build_table([n.encode() for n in fai])
            slots, found = chain(table, [n.encode() for n in fai], ghost.encode())
            if found < 0 and len(slots) == 2 and table[slots[0]] == 0:
                return fai, base, ghost
    raise AssertionError("no name set found for TWINS (%s)" % kind)


def twins(kind, method, directory):
    tag = "twins_%s_%s" % (kind, method)
    rng = _rng(tag)
    fai_names, wanted, ghost = _twins_search(kind)
    n_pos = 40
    fai = [(n, n_pos) for n in fai_names]
    pos = sorted(rng.choice(np.arange(1, n_pos + 1), size=20, replace=False).tolist())
    sites = [(n, p) for n in fai_names for p in (pos if n == wanted else pos[::4])]
    files = []
    for x in range(2):
        n_samples = 1 + x
        files.append((["t%ds%d" % (x, k) for k in range(n_samples)], _random_lines(rng, sites, n_samples, 0.8)))
    cut = None
    if ghost is not None:                                         # the stopping line, in the second half of file 0
        lines = files[0][1]
        at = len(lines) // 2 + 2
        lines.insert(at, "\t".join([ghost, "1", "A"]))
        cut = {0: at}
    names_b = [n.encode() for n in fai_names]
    table = build_table(names_b)
    slots, found = chain(table, names_b, (ghost or wanted).encode())
    return _finish(directory, tag, fai, files, method, cut=cut, kind=kind, table=table, wanted=wanted, ghost=ghost, chain=slots, found=found,
                   stopped_files=1 if ghost else 0)


TWINS = [("twins_%s_%s" % (k, m), (lambda d, k=k, m=m: twins(k, m, d))) for k in "abcd" for m in ("union", "all")]


# ---- WIDTH -------------------------------------------------------------------------------------------------------------------------
WIDTHS = (63, 64, 65, 127, 128, 129, 191, 192, 193)


def _wide_line(rng, name, pos, n_samples):
    return "\t".join([name, str(pos)] + [_cell(rng, 1, 1) for _ in range(n_samples)])


def width(w, directory):
    """file 0: every line w bytes, of 30 / 60 / 90 one-character cells behind a head of 3 .. 13 bytes (positions of one digit)"""
    tag = "width_%d" % w
    rng = _rng(tag)
    n_samples = 30 * ((w + 1) // 64)
    name_len = w - 2 * n_samples - 2
    scaf = []
    while len(scaf) < 3:
        s = _word(rng, name_len)
        if s not in scaf:
            scaf.append(s)
    sites = [(s, p) for s in scaf for p in range(1, 10)]
    wide = [_wide_line(rng, s, p, n_samples) for s, p in sites if rng.random() < 0.8]
    other = [_wide_line(rng, s, p, 35) for s, p in sites if rng.random() < 0.7]
    files = [(["w%d" % k for k in range(n_samples)], wide), (["v%d" % k for k in range(35)], other)]
    return _finish(directory, tag, [(s, 9) for s in scaf], files, "union", want_n={w}, want_steps={(w + 63) // 64}, wide_file=0)


def width_turn(directory):
    """one file of 30 cells whose lines are 63, 63, 64, 64, 65, 65 bytes, then 127 .. 129, then 191 .. 193, and all of that once more"""
    tag = "width_turn"
    rng = _rng(tag)
    scaf = [_word(rng, n) for n in (1, 65, 129, 1, 65, 129)]
    scaf[3] = "b" if scaf[0] != "b" else "c"
    sites = [(s, p) for s in scaf for p in (4, 7, 40, 70, 100, 200)]
    files = [(["w%d" % k for k in range(30)], [_wide_line(rng, s, p, 30) for s, p in sites]),
             (["v0", "v1"], _random_lines(rng, sites, 2, 0.7))]
    return _finish(directory, tag, [(s, 200) for s in scaf], files, "union", want_n=set(WIDTHS), want_steps={1, 2, 3, 4}, wide_file=0)


def width_bare(directory):
    """a file of two header fields (its head is its whole line) in front of one of 129-byte lines"""
    tag = "width_bare"
    rng = _rng(tag)
    scaf = [_word(rng, 7), _word(rng, 7)]
    sites = [(s, p) for s in scaf for p in range(1, 10)]
    bare = ["%s\t%d" % (s, p) for s, p in sites if rng.random() < 0.7]
    wide = [_wide_line(rng, s, p, 60) for s, p in sites if rng.random() < 0.8]
    files = [([], bare), (["w%d" % k for k in range(60)], wide)]
    return _finish(directory, tag, [(s, 9) for s in scaf], files, "union", want_n={129}, want_steps={3}, wide_file=1)


WIDTH = [("width_%d" % w, (lambda d, w=w: width(w, d))) for w in WIDTHS] + [("width_turn", width_turn), ("width_bare", width_bare)]


# ---- SEAMS -------------------------------------------------------------------------------------------------------------------------
SEAM_DEFECTS = (("dtab", 64), ("dtab", 128), ("trail", 63), ("trail", 64), ("trail", 128), ("blank", 63), ("blank", 64))
SEAM_POS = 45                                                  # the position of the special line, of 60: two digits


def seams(kind, d, defect, directory):
    """file 1 holds one special line (position 45 of 60): its byte d is a letter of a cell of two or three characters in the regular
    twin and the defect in the other case.  dtab: byte d - 1 is a tab, the defect a second tab at d.  trail: the line is d + 1 bytes,
    the defect a tab as its last byte.  blank: bytes d - 1 and d + 1 are letters of the same cell, the defect a space at d"""
    tag = "seams_%s_%d_%s" % (kind, d, "defect" if defect else "twin")
    rng = _rng("seams_%s_%d" % (kind, d))                      # (the twin's files are the defect's but for one byte)
    target = d if kind == "dtab" else d - 1                    # bytes in front of the special cell, the last a tab
    name = "sm_" if (target - 7) % 2 == 0 else "sm_x"          # `name <tab> 45 <tab>` is 7 or 8 bytes
    head = "%s\t%d\t" % (name, SEAM_POS)
    m = (target - len(head)) // 2
    front = head + "".join(_cell(rng, 1, 1) + "\t" for _ in range(m))
    assert len(front) == target
    if kind == "trail":
        n_samples, special = m + 1, front + "GT"
    else:
        n_samples = max(70, m + 6)
        cell = "GT" if kind == "dtab" else "GTC"
        special = front + "\t".join([cell] + [_cell(rng, 1, 1) for _ in range(n_samples - m - 1)])
    if defect:
        special = special[:d] + ("\t" if kind != "blank" else " ") + special[d + 1:]
    sites = [(name, p) for p in range(1, 61)]
    lines, at = [], None
    for s, p in sites:
        if p == SEAM_POS:
            at = len(lines)
            lines.append(special)
        elif rng.random() < 0.85:
            lines.append(_wide_line(rng, s, p, n_samples))
    files = [(["a0", "a1", "a2"], _random_lines(rng, sites, 3, 0.8)), (["s%d" % k for k in range(n_samples)], lines)]
    argv, facts = _finish(directory, tag, [(name, 60)], files, "union", seam=(kind, d), special=(1, at), special_line=special,
                          handed_back=defect, parts_known=not defect)     # (what the defect line adds is str.split()'s business)
    facts["stream"] = facts["few_lines_stream"] + 2 * facts["few_lines_stream"] // 6       # four of the longest lines a file
    return argv, facts


SEAMS = [("seams_%s_%d_%s" % (k, d, "defect" if x else "twin"), (lambda dr, k=k, d=d, x=x: seams(k, d, x, dr)))
         for k, d in SEAM_DEFECTS for x in (True, False)]


# ---- DUMMY -------------------------------------------------------------------------------------------------------------------------
DUMMY_RUNS = ((63, 0), (64, 0), (65, 0), (31, 1), (32, 1), (33, 1), (16, 3), (17, 3), (1, 63), (1, 64), (2, 64), (3, 21))
MISSING_CHARS = "".join(chr(c) for c in range(48, 123))       # digits, letters, : ; < = > ? @ [ \ ] ^ _ `: no blank, no comma


def missing_of(n):
    """a --missing of n bytes, no two neighbours alike"""
    return {1: "N", 3: "./."}.get(n, "".join(MISSING_CHARS[(7 * k + 3) % len(MISSING_CHARS)] for k in range(n)))


def dummy(cells, mlen, method, directory):
    """file 1 has `cells` header cells and holds half the sites; file 0 stands in front with two samples"""
    tag = "dummy_%d_%d_%s" % (cells, mlen, method)
    rng = _rng(tag)
    scaf = ["dm_" + _word(rng, 3), "dm_" + _word(rng, 6)]
    sites = [(s, p) for s in scaf for p in range(1, 26)]
    files = [(["a0", "a1"], _random_lines(rng, sites, 2, 0.8)),
             (["d%d" % k for k in range(cells)], [_wide_line(rng, s, p, cells) for s, p in sites if rng.random() < 0.5])]
    takes = mlen <= 64
    return _finish(directory, tag, [(s, 25) for s in scaf], files, method, missing=missing_of(mlen), dummy_run=cells * (1 + mlen), dummy_file=1,
                   device_takes=takes, handed_back=not takes)


DUMMY = ([("dummy_%d_%d_%s" % (c, n, m), (lambda d, c=c, n=n, m=m: dummy(c, n, m, d))) for c, n in DUMMY_RUNS for m in ("union", "all")]
         + [("dummy_2_65_union", lambda d: dummy(2, 65, "union", d))])
MISSING_TOO_LONG = "dummy_2_65_union"


# ---- CELLS -------------------------------------------------------------------------------------------------------------------------
PART_BYTES = (63, 64, 65, 129, 300)


def cells(part, shape, g, directory):
    """three files; file g adds `part` bytes to a line it holds: one cell of part - 1 bytes, or part // 2 cells of one character (one
    of two where part is odd)"""
    tag = "cells_%d_%s_%d" % (part, shape, g)
    rng = _rng(tag)
    scaf = ["ce" + _word(rng, 4), "ce" + _word(rng, 9)]
    sites = [(s, p) for s in scaf for p in range(1, 16)]
    files = []
    for x in range(3):
        if x != g:
            files.append((["c%ds%d" % (x, k) for k in range(2)], _random_lines(rng, sites, 2, 0.7)))
        elif shape == "long":
            files.append((["c%dlong" % x], _random_lines(rng, sites, 1, 0.7, part - 1, part - 1)))
        else:
            n = part // 2
            lines = ["\t".join([s, str(p), _cell(rng, 1 + part % 2, 1 + part % 2)] + [_cell(rng, 1, 1) for _ in range(n - 1)])
                     for s, p in sites if rng.random() < 0.7]
            files.append((["c%ds%d" % (x, k) for k in range(n)], lines))
    return _finish(directory, tag, [(s, 15) for s in scaf], files, "union", out_sep=",", part=part, part_file=g)


CELLS = [("cells_%d_%s_%d" % (p, s, g), (lambda d, p=p, s=s, g=g: cells(p, s, g, d))) for p in PART_BYTES for s in ("long", "short") for g in range(3)]


# ---- DIGITS ------------------------------------------------------------------------------------------------------------------------
DIGITS_LEN = 100010
DIGITS_ROUND = 1000                                            # positions a round of the small stream covers


def digits(small, directory):
    """two files hold sites at the changes of the digit count and at the scaffold's end; --method all writes all 100 010 positions.
    small: the output budget of a round is DIGITS_ROUND lines no file adds to (pgm_fixed_bytes: the name, a separator, 18 digits, a
    line feed, every file's dummy cells), so that rounds end on 1000, 10000 and 100000, the first position of a digit count, and the
    round in front of each holds the change inside"""
    tag = "digits_%s" % ("rounds" if small else "default")
    rng = _rng("digits")
    edges = sorted(set(p + k for p in (10, 100, 1000, 10000, 100000) for k in (-2, -1, 0, 1)) | {1, 5, DIGITS_LEN - 1, DIGITS_LEN})
    sites = [("chr", p) for p in edges]
    files = [(["g0"], _random_lines(rng, sites, 1, 0.6)), (["h0", "h1"], _random_lines(rng, sites, 2, 0.6))]
    argv, facts = _finish(directory, tag, [("chr", DIGITS_LEN)], files, "all")
    fixed = len("chr") + 1 + 18 + 1 + 3 * 2
    if small:
        facts["stream"] = fixed * DIGITS_ROUND
        facts["rounds_at_least"] = DIGITS_LEN // DIGITS_ROUND
    return argv, facts


DIGITS = [("digits_default", lambda d: digits(False, d)), ("digits_rounds", lambda d: digits(True, d))]


# ---- LINES -------------------------------------------------------------------------------------------------------------------------
LINE_COUNTS = (1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025)


def lines(n, directory):
    tag = "lines_%d" % n
    rng = _rng(tag)
    sites = [("ln", int(p)) for p in sorted(rng.choice(np.arange(1, 1101), size=n, replace=False).tolist())]
    files = [(["a0"], _random_lines(rng, sites, 1, 2.0)), (["b0", "b1"], _random_lines(rng, sites, 2, 2.0))]
    return _finish(directory, tag, [("ln", 1100)], files, "union", n_lines=n)


LINES = [("lines_%d" % n, (lambda d, n=n: lines(n, d))) for n in LINE_COUNTS]

SETS = dict(NAMES=NAMES, TWINS=TWINS, WIDTH=WIDTH, SEAMS=SEAMS, DUMMY=DUMMY, CELLS=CELLS, DIGITS=DIGITS, LINES=LINES)
ALL = [(set_name, name, build) for set_name, cases in SETS.items() for name, build in cases]
STREAMED_SETS = ("NAMES", "WIDTH", "CELLS", "DUMMY")          # every second case of these also runs with a few lines a file and round


def streamed():
    return [(s, n, b) for s in STREAMED_SETS for k, (n, b) in enumerate(SETS[s]) if k % 2 == 1 and n != MISSING_TOO_LONG]


class Store:
    """every case built once under a directory of its own: (argv, facts, the model's bytes)"""

    def __init__(self, root):
        self.root, self.done = str(root), {}
        self.builders = {name: build for _, name, build in ALL}

    def get(self, name):
        if name not in self.done:
            import merge_model
            directory = os.path.join(self.root, name)
            os.makedirs(directory)
            argv, facts = self.builders[name](directory)
            self.done[name] = (argv, facts, merge_model.merge_argv(argv))
        return self.done[name]
