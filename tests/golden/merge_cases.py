"""mergeGeno.py goldens: the fixtures written for them, the command lines, and how a run's output is read back
(tests/golden/make_golden_merge.py runs the unmodified reference on them; tests/test_merge_cpu.py, tests/test_merge_emul.py and
tests/test_gpu_merge.py compare byte for byte).

A fixture is a `.geno.gz` under tests/golden/merge/; {dir} in a command line is that directory.  `out`: "stdout" (no -o), "file"
(-o <tmp>/out) or "gz" (-o <tmp>/out.gz, gunzipped); the golden tests/golden/merge/<name>.out.gz holds those bytes, gzipped.  `host`: the
case holds a line outside the regular spelling, or a separator of more than one byte: its rounds are the host route's on every route."""
import gzip
import os

# scaffolds of the .fai files; `empty` is one no file has a line of, `tiny` has one position
FAI = {"main": [("c1", 700), ("empty", 40), ("scaffold_2", 1500), ("tiny", 1), ("Z", 900)],
       "small": [("c1", 60), ("c2", 30)]}


def _rng(state):
    while True:
        state = (state * 6364136223846793005 + 1442695040888963407) % (1 << 64)
        yield state >> 33


def _sites(fai, keep_of, seed):
    """the shared list of sites of a .fai, about one position in `keep_of`"""
    r = _rng(seed)
    return [(s, p) for s, n in FAI[fai] if s != "empty" for p in range(1, n + 1) if next(r) % keep_of == 0]


def _lines(sites, samples, seed, keep=70):
    """the data lines of a file: `keep` per cent of the sites, one cell a sample"""
    r = _rng(seed)
    alphabet = ["A/A", "A/T", "T/T", "N/N", "C/G", "G/G", "A", "ACGT/-"]
    out = []
    for s, p in sites:
        if next(r) % 100 >= keep:
            for _ in samples:
                next(r)
            continue
        out.append("%s\t%d\t%s" % (s, p, "\t".join(alphabet[next(r) % len(alphabet)] for _ in samples)) if samples else "%s\t%d" % (s, p))
    return out


def _insert(lines, at, new):
    return lines[:at] + new + lines[at:]


def fixtures():
    """name -> (header fields, data lines)"""
    main = _sites("main", 9, 11)
    small = _sites("small", 2, 5)
    fx = {}
    fx["a"] = (["#CHROM", "POS", "a1", "a2", "a3"], _lines(main, ["a1", "a2", "a3"], 1))
    fx["b"] = (["scaffold", "position", "b1", "b2"], _lines(main, ["b1", "b2"], 2))
    fx["c"] = (["#CHROM", "POS", "c1", "c2", "c3", "c4"], _lines(main, ["c1"] * 4, 3))
    fx["d"] = (["#CHROM", "POS", "d1"], _lines(main, ["d1"], 4, keep=85))
    fx["e"] = (["#CHROM", "POS", "e1", "e2"], _lines(main, ["e1", "e2"], 5, keep=85))
    fx["nosamples"] = (["#CHROM", "POS"], _lines(main, [], 6))
    fx["headeronly"] = (["#CHROM", "POS", "h1", "h2"], [])
    s1 = _lines(small, ["p", "q"], 7, keep=80)
    s2 = _lines(small, ["r"], 8, keep=80)
    fx["s1"] = (["#CHROM", "POS", "p", "q"], s1)
    fx["s2"] = (["#CHROM", "POS", "r"], s2)
    half = len(s2) // 2 + 2
    pos_of = lambda ln: int(ln.split("\t")[1])          # noqa: E731
    # the stopping lines, each in the second half of its file and followed by lines the file would otherwise give
    fx["stop_zero"] = fx["s2"][0], _insert(s2, half, ["c1\t0%d\tT/T" % (pos_of(s2[half]) - 1 if s2[half].startswith("c1") else 3)])
    fx["stop_range"] = fx["s2"][0], _insert(s2, len(s2) - 2, ["c2\t31\tA/A"])
    fx["stop_scaffold"] = fx["s2"][0], _insert(s2, half, ["c9\t5\tA/A"])
    fx["stop_repeat"] = fx["s2"][0], _insert(s2, half, [s2[half - 1]])
    fx["stop_blank"] = fx["s2"][0], _insert(s2, half, [""])
    # ragged lines: a cell too few, cells too many
    rag = list(s1)
    rag[3] = rag[3].rsplit("\t", 1)[0]
    rag[7] = rag[7] + "\textra\tcells"
    fx["ragged"] = fx["s1"][0], rag
    # spellings split() takes and the device does not: a double tab, trailing spaces, spaces between fields
    odd = list(s1)
    odd[2] = odd[2].replace("\t", "\t\t", 1)
    odd[5] = odd[5] + "  "
    odd[9] = odd[9].replace("\t", " ")
    fx["spaced"] = fx["s1"][0], odd
    return fx


def _in(*names):
    argv = []
    for n in names:
        argv += ["-i", "{dir}/%s.geno.gz" % n]
    return argv


M, S = ["-f", "{dir}/main.fai"], ["-f", "{dir}/small.fai"]
MERGE_CASES = [
    dict(name="intersect_three", out="stdout", argv=_in("a", "b", "c") + M),
    dict(name="union_three", out="file", argv=_in("a", "b", "c") + M + ["--method", "union"]),
    dict(name="all_two_small", out="file", argv=_in("s1", "s2") + S + ["--method", "all"]),
    dict(name="union_min2_five", out="file", argv=_in("a", "b", "c", "d", "e") + M + ["--method", "union", "--unionMin", "2"]),
    dict(name="union_min0_small", out="file", argv=_in("s1", "s2") + S + ["--method", "union", "--unionMin", "0"]),
    dict(name="union_first1", out="file", argv=_in("b", "a", "d") + M + ["--method", "union", "--mustIncludeFirst", "1"]),
    dict(name="all_first1_small", out="file", argv=_in("s2", "s1") + S + ["--method", "all", "--mustIncludeFirst", "1"]),
    dict(name="union_only2", out="file", argv=_in("a", "b", "c") + M + ["--method", "union", "--outputOnly", "2"]),
    dict(name="union_only21", out="file", argv=_in("a", "b") + M + ["--method", "union", "--outputOnly", "2", "1"]),
    dict(name="intersect_only_twice", out="file", argv=_in("a", "b", "c") + M + ["--outputOnly", "3", "1", "3"]),
    dict(name="union_missing_dots", out="file", argv=_in("a", "b", "c") + M + ["--method", "union", "--missing", "./."]),
    dict(name="union_missing_empty", out="file", argv=_in("a", "b") + M + ["--method", "union", "--missing", ""]),
    dict(name="union_sep_comma", out="file", argv=_in("a", "b", "c") + M + ["--method", "union", "--outSep", ","]),
    dict(name="union_sep_two", out="file", host=True, argv=_in("a", "b") + M + ["--method", "union", "--outSep", "::"]),
    dict(name="stop_zero_union", out="file", argv=_in("s1", "stop_zero") + S + ["--method", "union"]),
    dict(name="stop_range_union", out="file", argv=_in("s1", "stop_range") + S + ["--method", "union"]),
    dict(name="stop_scaffold_intersect", out="file", argv=_in("s1", "stop_scaffold") + S),
    dict(name="stop_repeat_all", out="file", argv=_in("stop_repeat", "s1") + S + ["--method", "all"]),
    dict(name="stop_blank_union", out="file", host=True, argv=_in("s1", "stop_blank") + S + ["--method", "union"]),
    dict(name="ragged_union", out="file", host=True, argv=_in("ragged", "s2") + S + ["--method", "union"]),
    dict(name="spaced_union", out="file", host=True, argv=_in("s2", "spaced") + S + ["--method", "union"]),
    dict(name="nosamples_union", out="file", argv=_in("a", "nosamples", "b") + M + ["--method", "union"]),
    dict(name="headeronly_union", out="file", argv=_in("a", "headeronly", "b") + M + ["--method", "union"]),
    dict(name="headeronly_intersect", out="stdout", argv=_in("a", "headeronly") + M),
    dict(name="union_five_gz", out="gz", argv=_in("a", "b", "c", "d", "e") + M + ["--method", "union"]),
    dict(name="intersect_two", out="file", argv=_in("d", "e") + M),
]


def write_fixtures(directory):
    os.makedirs(directory, exist_ok=True)
    for name, scafs in FAI.items():
        with open(os.path.join(directory, name + ".fai"), "w") as f:
            for k, (s, n) in enumerate(scafs):
                f.write("%s\t%d\t%d\t60\t61\n" % (s, n, 7 + 1000 * k))
    for name, (header, lines) in fixtures().items():
        with gzip.GzipFile(os.path.join(directory, name + ".geno.gz"), "wb", mtime=0) as raw:
            raw.write(("\t".join(header) + "\n" + "".join(ln + "\n" for ln in lines)).encode())


def out_args(case, tmp):
    stem = os.path.join(tmp, "out")
    return {"stdout": [], "file": ["-o", stem], "gz": ["-o", stem + ".gz"]}[case["out"]]


def read_output(case, tmp, stdout):
    if case["out"] == "stdout":
        return stdout
    if case["out"] == "file":
        with open(os.path.join(tmp, "out"), "rb") as f:
            return f.read()
    with gzip.open(os.path.join(tmp, "out.gz"), "rb") as f:
        return f.read()
