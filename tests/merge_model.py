"""What mergeGeno.py computes, written from the drop-in's rules and not from the reference's walk: per file the longest prefix of lines
whose sites are valid and increasing, then a join of the files' sites by a dictionary.  Slow by design and for small inputs only; it
stands in for the reference wherever the reference is not at hand.  tests/test_merge_cpu.py holds it against every golden of the
unmodified reference."""
import gzip


def _text(path):
    with (gzip.open(path, "rt") if path.endswith(".gz") else open(path, "rt")) as f:
        return f.read()


def _contribution(text, index, lengths):
    """(header fields, {site: cells}) of one file: its lines up to the first that is no site or does not lie behind the one before"""
    lines = text.split("\n")
    if lines and lines[-1] == "":
        lines.pop()
    header = lines[0].split() if lines else []
    sites, last = {}, None
    for line in lines[1:]:
        fields = line.split()
        if len(fields) < 2 or fields[0] not in index:
            break
        number = fields[1]
        if not (number.isascii() and number.isdigit()) or number[0] == "0":
            break
        site = (index[fields[0]], int(number))
        if site[1] > lengths[site[0]] or (last is not None and site <= last):
            break
        sites[site] = fields[2:]
        last = site
    return header, sites


def merge(inputs, fai, method="intersect", union_min=1, must_first=0, out_sep="\t", missing="N", output_only=None):
    """the bytes the reference writes for these options"""
    scaffolds = [ln.split()[:2] for ln in _text(fai).splitlines()]
    names = [s[0] for s in scaffolds]
    lengths = [int(s[1]) for s in scaffolds]
    index = {name: k for k, name in enumerate(names)}
    files = [_contribution(_text(p), index, lengths) for p in inputs]
    n = len(files)
    shown = set(k - 1 for k in output_only) if output_only else set(range(n))
    order = [k - 1 for k in output_only] if output_only else list(range(n))
    enough = max(union_min, must_first)

    def wanted(held):
        if not all(held[:max(must_first, 0)]):
            return False
        if method == "intersect":
            return all(held)
        return method == "all" or sum(held) >= enough

    if wanted([False] * n):                                   # sites no file holds are written: every position is a candidate
        candidates = ((k, p) for k in range(len(names)) for p in range(1, lengths[k] + 1))
    else:
        candidates = sorted(set(site for _, sites in files for site in sites))
    out = [out_sep.join(files[0][0][:2]) + out_sep + out_sep.join(out_sep.join(files[x][0][2:]) for x in order) + "\n"]
    for site in candidates:
        held = [site in sites for _, sites in files]
        if not wanted(held):
            continue
        fields = [names[site[0]], str(site[1])]
        for x, (header, sites) in enumerate(files):
            if x in shown:
                fields += sites[site] if held[x] else [missing] * max(len(header) - 2, 0)
        out.append(out_sep.join(fields) + "\n")
    return "".join(out).encode()


def merge_argv(argv):
    """the same from a command line of the drop-in (the options the goldens use)"""
    import argparse
    ap = argparse.ArgumentParser()
    ap.add_argument("-i", action="append")
    ap.add_argument("-f")
    ap.add_argument("-o")
    ap.add_argument("--method", default="intersect")
    ap.add_argument("--unionMin", type=int, default=1)
    ap.add_argument("--mustIncludeFirst", type=int, default=0)
    ap.add_argument("--outSep", default="\t")
    ap.add_argument("--missing", default="N")
    ap.add_argument("--outputOnly", type=int, nargs="+")
    a = ap.parse_args(argv)
    return merge(a.i, a.f, a.method, a.unionMin, a.mustIncludeFirst, a.outSep, a.missing, a.outputOnly)
