"""Drop-in for the reference's seqToGeno.py: a fasta or phylip alignment (a whole-genome alignment, simulated sequences, what
genoToSeq.py writes) as `.geno` sites -- the transpose back from sequences to site-major text, with the lines' own text (scaffold,
position, tabs, '|') generated on the way.

Two stages meet in a residue store: the sequences' characters side by side, feeds and blanks gone, with a table of where each begins
and how long it is.  Stage 1 loads it: fasta text goes through the device route's text slot in blocks of whole lines (pg_s2g_dev_*:
k_s2g_lines, k_s2g_gather), a block with an irregular line (a blank, a tab, \\r, a second '>', text in front of the first record)
through the host route's stripping (pg_s2g_strip) and to the same place; phylip input, line-structured and small in practice, is
parsed here into the store.  Stage 2 emits: the output is a list of segments (a scaffold name, a number of sites, per haplotype its
store offset) that share one row template, and a line's start is a closed form of its site, so ranges of sites sized to
PG_STREAM_BYTES are written by k_s2g_tile (device) or pg_s2g_text (host threads; PG_S2G_DEVICE=0) one after the other.  The rules
both routes share live in csrc/pg_s2g_core.h.

The reference reads everything before it writes, so every rejection (exit status 2, one message) leaves no output file.  A later
sequence shorter than the first stops the run at that line as the reference's IndexError does: the rows before it are written, one
message, exit status 1.  Divergences: `-P k` with one k above 1 (the reference raises TypeError under Python 3) means k for every
group; --randomPhase and multi-phylip input with a ploidy above 1 (the reference always dies) are rejected.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib, devroute, dist, genoio

ENGINE_EPILOG = ("MI355X engine: fasta blocks of regular lines (head lines, sequence lines without blanks, tabs or \\r, ASCII) are "
                 "gathered into a residue store on the device, every other block is stripped by host threads and uploaded; phylip "
                 "input is parsed on the host.  The lines are written by the device in ranges of sites.  Under WORLD_SIZE > 1 rank 0 "
                 "does the whole job.  Environment: PG_S2G_DEVICE=0 host threads only; PG_BGZF_DEVICE=0 bgzip members inflated by host "
                 "threads; PG_DEFLATE_DEVICE=0 -g x.gz rows deflated by host threads; PG_STREAM_BYTES bytes per input block and "
                 "output range (default 256 MiB); PG_SCRATCH_GIB the device's budget for the store; PG_S2G_TILE_SEQS haplotypes per "
                 "tile; PG_HOST_THREADS host threads; PG_TIMING=1 blocks and times on stderr.")

MAX_HAPS = 32768                                           # PGS_MAX_HAPS
MAX_NAME = 4096                                            # PGS_MAX_NAME
last_info = {}


class Usage(devroute.Usage):
    """(no output file is left)"""
    prog = "seqToGeno.py"


class Stop(devroute.Stop):
    prog = "seqToGeno.py"


def make_parser():
    ap = argparse.ArgumentParser(prog="seqToGeno.py", epilog=ENGINE_EPILOG)
    ap.add_argument("-s", "--seqFile", help="Input sequence file", action="store", required=False)
    ap.add_argument("-g", "--genoFile", help="Output geno file", action="store", required=False)
    ap.add_argument("-f", "--format", help="Sequence file format", action="store", required=False, choices=("phylip", "fasta"), default="fasta")
    ap.add_argument("-M", "--mode", help="Output mode for separate sequences", action="store", choices=("samples", "contigs"), required=False,
                    default="samples")
    ap.add_argument("-C", "--chrom", help="Name for chromosome or contig if sequences are samples", action="store", required=False,
                    default="contig0")
    ap.add_argument("-N", "--name", help="Name for sample if sequences are contigs", action="store", required=False, default="sample0")
    ap.add_argument("-S", "--sequences", help="Sequences to output", action="store", nargs="+", type=str)
    ap.add_argument("--merge", help="For multi-phylip input, do not increment scaffold numbers", action="store_true")
    ap.add_argument("-P", "--ploidy", help="Ploidy for joining sequences", action="store", nargs="+", type=int, default=[1])
    ap.add_argument("--randomPhase", help="Randomize phase for fused sequences", action="store_true")
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


def _vp(a):
    return C.c_void_p(a.ctypes.data if a.size else 0)


_threads = devroute.host_threads


def digit_sum(x):
    """pgs_digit_sum: the digits of 1 .. x together"""
    d = len(str(x))
    return (x + 1) * d - (10 ** d - 1) // 9


def line_start(x, fixed):
    """pgs_line_start: where line x of a segment begins, counted from its line 0"""
    return x * fixed + digit_sum(x)


def universal(buf):
    """the reference's text-mode file (and its stdin): \\r\\n and a lone \\r end a line"""
    return buf.replace(b"\r\n", b"\n").replace(b"\r", b"\n") if b"\r" in buf else buf


def strip(text, dst, n_threads=0):
    """pg_s2g_strip: text without its line feeds and blanks into the uint8 array dst; the bytes written"""
    return int(_lib.lib().pg_s2g_strip(text, len(text), _vp(dst), _threads(n_threads))) if len(text) else 0


# ---- stage 1: the store ---------------------------------------------------------------------------------------------------------
class Records:
    """the fasta records seen so far: their names and where each begins in the store; `total` residues stand there"""

    def __init__(self, shown):
        self.names, self.starts, self.total, self.shown = [], [], 0, shown

    @property
    def open(self):
        return bool(self.names)

    def head(self, line, at):
        """a record's first line (behind its '>') opens a record whose residues begin at `at`"""
        words = line.decode("ascii").split()
        if not words:
            raise Usage("%s: record %d has no name (the reference raises IndexError)" % (self.shown, len(self.names) + 1))
        self.names.append(words[0])
        self.starts.append(at)

    def lengths(self):
        return np.diff(np.asarray(self.starts + [self.total], dtype=np.int64))

    def host_block(self, buf, n_threads=0):
        """parseFasta on a block of whole lines (genomics.py:2256-2261): the block's residues as a uint8 array; the records it opens
        are noted at their places behind self.total, which moves on"""
        buf = universal(bytes(buf))
        if not buf.isascii():
            raise Usage("%s: text that is not ASCII is not supported" % self.shown)
        out = np.empty(max(len(buf), 1), dtype=np.uint8)
        n = 0
        pieces = buf.split(b">")
        if self.open and pieces[0]:                        # (text before the first '>' is ignored)
            n += strip(pieces[0], out, n_threads)
        for piece in pieces[1:]:
            nl = piece.find(b"\n")
            if nl < 0:
                raise Usage("%s: record %d ends without a line feed (the reference raises ValueError)" % (self.shown, len(self.names) + 1))
            self.head(piece[:nl], self.total + n)
            if len(piece) > nl + 1:
                n += strip(piece[nl:], out[n:], n_threads)
        self.total += n
        return out[:n]


class HostStore:
    """the residue store in host memory"""

    def __init__(self):
        self.buf = np.empty(1 << 16, dtype=np.uint8)
        self.n = 0

    def append(self, arr):
        need = self.n + len(arr)
        if need > len(self.buf):
            grown = np.empty(need + need // 2 + 4096, dtype=np.uint8)
            grown[:self.n] = self.buf[:self.n]
            self.buf = grown
        self.buf[self.n:need] = arr
        self.n = need


class _Device(devroute.SlotDevice):
    """the device route: the store in device memory, a fasta block's kernels queued while the next block is on its way"""

    def __init__(self, device, hint):
        super().__init__(device, "s2g")
        _lib.check(self.L.pg_s2g_dev_begin(self.eng._h, int(hint)))

    def submit(self, block):
        """the block into the next slot (its copy, or its members' inflation, queued); the ticket parse and collect take"""
        return self.load(block)

    def parse(self, ticket, base, is_open):
        _lib.check(self.L.pg_s2g_dev_parse(self.eng._h, ticket[0], int(base), int(bool(is_open))))

    def collect(self, ticket, rec, n_threads):
        """the block's records into rec; a block the device hands back is stripped here and uploaded to the same place"""
        s, keep = ticket
        nr, nh, hl, nl = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pg_s2g_dev_collect(self.eng._h, s, C.byref(nr), C.byref(nh), C.byref(hl), C.byref(nl)))
        plain = isinstance(keep, bytes)
        total = len(keep) if plain else len(keep[0])
        if not total:
            return
        if hl.value >= 0:
            base = rec.total
            arr = rec.host_block(keep if plain else self.text(s, 0, total), n_threads)
            self.put(base, arr)
            return
        heads = np.empty(3 * max(nh.value, 1), dtype=np.int64)[:3 * nh.value]
        if nh.value:
            _lib.check(self.L.pg_s2g_dev_heads(self.eng._h, s, _vp(heads), nh.value))
        for a, k, before in heads.reshape(-1, 3):
            a, k = int(a), int(k)
            rec.head(keep[a + 1:a + k] if plain else self.text(s, a + 1, k - 1), rec.total + int(before))
        rec.total += nr.value

    def put(self, off, arr):
        arr = np.ascontiguousarray(arr, dtype=np.uint8)
        _lib.check(self.L.pg_s2g_dev_put(self.eng._h, int(off), _vp(arr), len(arr)))

    def get(self, n):
        return devroute.fetch(lambda h, dst, m: self.L.pg_s2g_dev_get(h, 0, m, dst), self.eng._h, n)

    def plan(self, part, total, tile_seqs):
        """the part's template and segments to the device; the haplotypes a tile of k_s2g_tile takes"""
        name_off = np.concatenate([[0], np.cumsum([len(n) for n in part.names])]).astype(np.int64)
        sites = np.asarray([s[1] for s in part.segs], dtype=np.int64)
        offs = np.ascontiguousarray(np.concatenate(part.hap_off), dtype=np.int64)
        tq = C.c_int()
        _lib.check(self.L.pg_s2g_dev_plan(self.eng._h, _vp(part.tmpl), len(part.tmpl), part.n_haps, b"".join(part.names), _vp(name_off),
                                          len(part.names), _vp(sites), _vp(offs), int(total), int(tile_seqs), C.byref(tq)))
        return tq.value

    def emit(self, pieces, size, gz_rows):
        """the lines of the pieces (segment, x0, x1), `size` bytes: the rows, or -- gz_rows -- their BGZF members"""
        seg = np.asarray([p[0] for p in pieces], dtype=np.int32)
        x0 = np.asarray([p[1] for p in pieces], dtype=np.int64)
        x1 = np.asarray([p[2] for p in pieces], dtype=np.int64)
        bl = C.c_int64()
        _lib.check(self.L.pg_s2g_dev_emit(self.eng._h, _vp(seg), _vp(x0), _vp(x1), len(pieces), size, int(gz_rows), C.byref(bl)))
        return devroute.fetch(self.L.pg_s2g_dev_rows, self.eng._h, bl.value if gz_rows else size, int(gz_rows))

    def stats(self):
        b, h, r = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pg_s2g_dev_stats(self.eng._h, C.byref(b), C.byref(h), C.byref(r)))
        return b.value, h.value, r.value


def parse_phylip(text, shown):
    """parsePhylip (genomics.py:2265-2283) on the file's text: [(names, [sequence bytes, ...]), ...], an entry per alignment"""
    parts = [ln.strip().split() for ln in text.strip().split("\n")]
    parts = [p for p in parts if p]
    heads, counts = [], []
    for x, p in enumerate(parts):
        try:
            int(p[1])
            n = int(p[0])
        except (ValueError, IndexError):
            continue
        heads.append(x)
        counts.append(n)
    heads.append(len(parts))
    out = []
    for i, n in enumerate(counts):
        a, b = heads[i] + 1, heads[i + 1]
        if n > b - a:
            raise Usage("%s: alignment %d announces %d sequences and holds %d lines" % (shown, i + 1, n, b - a))
        for y in range(a, b):
            if len(parts[y]) < 2:
                raise Usage("%s: alignment %d: a line of one word, '%s' (the reference raises IndexError; interleaved files whose "
                            "continuation lines lack the name are not supported)" % (shown, i + 1, parts[y][0][:40]))
        names = [parts[a + j][0] for j in range(n)]
        seqs = ["".join(parts[y][1] for y in range(a + j, b, n)).encode("ascii") for j in range(n)]
        out.append((names, seqs))
    return out


# ---- the plan: header, template, segments ---------------------------------------------------------------------------------------
class Part:
    """segments that share a row template.  tmpl: int32 per byte of a line's body, -1 - literal or a haplotype's index; segs:
    [(scaffold name, sites, [store offset per haplotype])]"""

    def __init__(self, tmpl, segs):
        self.tmpl, self.segs = np.asarray(tmpl, dtype=np.int32), segs
        self.n_haps = int((self.tmpl >= 0).sum())
        self.names = [s[0].encode("ascii") for s in segs]
        self.hap_off = [np.asarray(s[2], dtype=np.int64) for s in segs]


class Plan:
    """header: the output's first line; parts: the segments, one part but for -M contigs with unequal ploidies (a part per stretch
    of one ploidy); stop: None, or the message of the line the run stops on behind the last segment's sites"""

    def __init__(self, header, parts, stop):
        self.header, self.parts, self.stop = header, parts, stop


def groups_of(n, ploidy):
    """haploToPhased's groups of consecutive sequences (genomics.py:413-430); a single value k stands for k, k, ..."""
    if max(ploidy) <= 1:
        return [[k] for k in range(n)]
    if len(ploidy) == 1:
        if n % ploidy[0]:
            raise Usage("-P %d: the number of sequences, %d, is not divisible by it" % (ploidy[0], n))
        ploidy = ploidy * (n // ploidy[0])
    elif sum(ploidy) != n:
        raise Usage("-P: the ploidies sum to %d, the sequences are %d" % (sum(ploidy), n))
    out, at = [], 0
    for p in ploidy:
        out.append(list(range(at, at + p)))
        at += p
    return out


def template(groups):
    t = []
    for g, grp in enumerate(groups):
        for k in range(len(grp)):
            t.append(len(t) // 2)
            t.append(-1 - ord("|" if k + 1 < len(grp) else "\t" if g + 1 < len(groups) else "\n"))
    return t


def select(names, wanted):
    out = []
    for w in wanted:
        if w not in names:
            raise Usage("-S: sequence %s is not in the input (the reference raises ValueError)" % w)
        out.append(names.index(w))
    return out


def make_plan(args, alignments, shown):
    """alignments: [(names, starts, lengths)] with the sequences' places in the store -- one entry, or the alignments of a
    multi-phylip file"""
    ploidy = list(args.ploidy)
    if len(alignments) == 1:
        names, starts, lens = alignments[0]
        idx = select(names, args.sequences) if args.sequences is not None else list(range(len(names)))
        names = list(args.sequences) if args.sequences is not None else names
        if not idx:
            raise Usage("%s holds no sequence" % shown)
        groups = groups_of(len(idx), ploidy)
        gnames = ["_".join(names[k] for k in g) for g in groups]
        glen = [min(int(lens[idx[k]]) for k in g) for g in groups]
        goff = [[int(starts[idx[k]]) for k in g] for g in groups]
        if args.mode == "samples":
            header = "#CHROM\tPOS\t" + "\t".join(gnames) + "\n"
            n = min(glen)
            stop = None
            if n < glen[0]:
                stop = "%s: site %d: sequence %s ends there, the first holds %d (the reference raises IndexError)" % (
                    shown, n + 1, gnames[glen.index(n)], glen[0])
            return Plan(header, [Part(template(groups), [(args.chrom, n, [o for g in goff for o in g])])], stop)
        header = "#CHROM\tPOS\t" + args.name + "\n"
        parts, g = [], 0
        while g < len(groups):                             # (a row template per ploidy)
            e = g
            while e < len(groups) and len(groups[e]) == len(groups[g]):
                e += 1
            parts.append(Part(template([list(range(len(groups[g])))]), [(gnames[k], glen[k], goff[k]) for k in range(g, e)]))
            g = e
        return Plan(header, parts, None)
    if max(ploidy) > 1:
        raise Usage("multi-phylip input with a ploidy above 1 is not supported (the reference always dies there)")
    if len({len(a[0]) for a in alignments}) != 1:
        raise Usage("%s: for multi phylip, all alignments must have same number of sequences" % shown)
    names = list(args.sequences) if args.sequences else alignments[0][0]
    if not names:
        raise Usage("%s holds no sequence" % shown)
    header = "#CHROM\tPOS\t" + "\t".join(names) + "\n"
    segs, stop = [], None
    for i, (anames, starts, lens) in enumerate(alignments):
        idx = select(anames, names)
        ln = [int(lens[k]) for k in idx]
        n = min(ln)
        segs.append((args.chrom if args.merge else args.chrom + str(i), n, [int(starts[k]) for k in idx]))
        if n < ln[0]:
            stop = "%s: alignment %d, site %d: sequence %s ends there, the first holds %d (the reference raises IndexError)" % (
                shown, i + 1, n + 1, names[ln.index(n)], ln[0])
            break
    return Plan(header, [Part(template([[k] for k in range(len(names))]), segs)], stop)


# ---- stage 2: the lines ---------------------------------------------------------------------------------------------------------
def ranges(part, target):
    """the output in ranges of about `target` bytes: lists of pieces (segment, x0, x1) and their bytes"""
    pieces, size = [], 0
    for s, (name, n, _) in enumerate(part.segs):
        fixed = len(name) + 2 + len(part.tmpl)
        x = 0
        while x < n:
            room = max(target - size, 0)
            take = min(n - x, max(room // (fixed + len(str(x + 1)) + 1), 1))
            nbytes = line_start(x + take, fixed) - line_start(x, fixed)
            pieces.append((s, x, x + take))
            size += nbytes
            x += take
            if size >= target or len(pieces) >= 65536:
                yield pieces, size
                pieces, size = [], 0
    if pieces:
        yield pieces, size


def host_emit(part, store, pieces, size, n_threads):
    names, hap_off, tmpl = part.names, part.hap_off, part.tmpl
    out = np.empty(max(size, 1), dtype=np.uint8)[:size]
    L = _lib.lib()
    at = 0
    for s, x0, x1 in pieces:
        fixed = len(names[s]) + 2 + len(tmpl)
        n = line_start(x1, fixed) - line_start(x0, fixed)
        got = L.pg_s2g_text(_vp(store), names[s], len(names[s]), C.c_void_p(hap_off[s].ctypes.data), _vp(tmpl), len(tmpl), x0, x1,
                            C.c_void_p(out[at:].ctypes.data if n else 0), n, n_threads)
        if got != n:
            raise RuntimeError("pg_s2g_text: %d bytes for %d" % (got, n))
        at += n
    return out


def main(argv=None):
    t0 = time.perf_counter()
    args = make_parser().parse_args(argv)
    world = dist.world_from_env()
    if world.size > 1 and world.rank != 0:                 # rank 0 does the whole job
        return 0
    shown = args.seqFile or "<stdin>"
    if args.randomPhase:
        raise Usage("--randomPhase is not supported (the reference dies at len() of a zip)")
    if min(args.ploidy) < 1:
        raise Usage("-P: a ploidy below 1")
    for opt, vals in (("-C", [args.chrom]), ("-N", [args.name]), ("-S", args.sequences or [])):
        for v in vals:
            if not v.isascii():
                raise Usage("%s: text that is not ASCII is not supported" % opt)
            if len(v) > MAX_NAME:
                raise Usage("%s: a name of more than %d bytes is not supported" % (opt, MAX_NAME))
    n_threads = int(os.environ.get("PG_HOST_THREADS", "0"))
    block_bytes = max(int(os.environ.get("PG_STREAM_BYTES", str(256 << 20))), 1)
    budget = int(float(os.environ.get("PG_SCRATCH_GIB", "48")) * (1 << 30))
    info = dict(blocks=0, text_bytes=0, blocks_inflated_on_device=0, device_blocks=0, device_host_blocks=0, out_ranges=0, sites=0, tile_seqs=0)

    reader = genoio.BlockReader(args.seqFile)
    dev = None
    if os.environ.get("PG_S2G_DEVICE", "1") != "0":
        size = reader.input_size()
        if size > budget:
            sys.stderr.write("seqToGeno.py: the input's %d bytes exceed the device's scratch budget (PG_SCRATCH_GIB): host threads do the "
                             "job\n" % size)
        else:
            dev = _Device(args.device if args.device is not None else dist.device_for(world), max(size, 0) if reader.mm is not None else 0)
    store = None if dev is not None else HostStore()
    t_ctx = time.perf_counter()
    out = None
    try:
        def to_host(n):
            """the run goes on on the host route: the device's store comes back"""
            nonlocal dev, store
            sys.stderr.write("seqToGeno.py: the sequences exceed the device's scratch budget (PG_SCRATCH_GIB): host threads do the job\n")
            store = HostStore()
            store.append(dev.get(n))
            dev.close()
            dev = None

        if args.format == "fasta":
            rec = Records(shown)
            spans = dev is not None and isinstance(getattr(reader, "f", None), genoio.BgzfFile) and os.environ.get("PG_BGZF_DEVICE", "1") != "0"
            pending, upper = None, 0
            for blk in devroute.read_ahead(devroute.blocks(reader, block_bytes, dev.pinned() if spans else None, info), "pg-s2g-read"):
                if not len(blk):
                    break
                info["blocks"] += 1
                if devroute.is_span(blk):
                    info["blocks_inflated_on_device"] += 1
                upper += len(blk)
                if dev is not None and upper > budget:
                    if pending is not None:
                        dev.collect(pending, rec, n_threads)
                        pending = None
                    to_host(rec.total)
                if dev is None:
                    store.append(rec.host_block(blk, n_threads))
                    continue
                ticket = dev.submit(blk)                   # (the copy of this block beside the kernels of the one before)
                if pending is not None:
                    dev.collect(pending, rec, n_threads)
                dev.parse(ticket, rec.total, rec.open)
                pending = ticket
            if pending is not None:
                dev.collect(pending, rec, n_threads)
            alignments = [(rec.names, rec.starts, rec.lengths())]
        else:
            data = universal(bytes(reader.read_block(None)))
            info["blocks"], info["text_bytes"] = 1, len(data)
            if not data.isascii():
                raise Usage("%s: text that is not ASCII is not supported" % shown)
            alignments, chunks, at = [], [], 0
            for names, seqs in parse_phylip(data.decode("ascii"), shown):
                lens = [len(s) for s in seqs]
                starts = list(at + np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.int64)) if seqs else []
                alignments.append((names, starts, lens))
                chunks += seqs
                at += sum(lens)
            arr = np.frombuffer(b"".join(chunks), dtype=np.uint8)
            if dev is not None and len(arr) > budget:
                to_host(0)
            if dev is not None:
                dev.put(0, arr)
            else:
                store.append(arr)
        if not alignments or not alignments[0][0]:
            raise Usage("%s holds no sequence" % shown)
        total = int(sum(int(np.sum(a[2])) for a in alignments))
        plan = make_plan(args, alignments, shown)
        if max(p.n_haps for p in plan.parts) > MAX_HAPS:
            raise Usage("more than %d sequences a line are not supported" % MAX_HAPS)
        if any(len(n) > MAX_NAME for p in plan.parts for n in p.names):
            raise Usage("a scaffold name of more than %d bytes is not supported" % MAX_NAME)
        t_load = time.perf_counter()
        gz_rows = (dev is not None and bool(args.genoFile and args.genoFile.endswith(".gz"))
                   and os.environ.get("PG_DEFLATE_DEVICE", "1") != "0")
        out = devroute.open_rows(args.genoFile)
        out.write(plan.header.encode("ascii"))
        for part in plan.parts:
            if dev is not None:
                info["tile_seqs"] = dev.plan(part, total, int(os.environ.get("PG_S2G_TILE_SEQS", "0")))
            for pieces, size in ranges(part, block_bytes):
                info["sites"] += sum(x1 - x0 for _, x0, x1 in pieces)
                if dev is None:
                    out.write(memoryview(host_emit(part, store.buf, pieces, size, _threads(n_threads))))
                    info["out_ranges"] += 1
                    continue
                rows = dev.emit(pieces, size, gz_rows)
                if gz_rows:
                    out.write_members(rows)
                else:
                    out.write(memoryview(rows))
        if dev is not None:
            info["device_blocks"], info["device_host_blocks"], info["out_ranges"] = dev.stats()
        devroute.close_rows(out, True)
        out = None
        info["load_s"] = t_load - t_ctx
        info["emit_s"] = time.perf_counter() - t_load
    finally:
        if out is not None:
            devroute.close_rows(out, False)
        if dev is not None:
            dev.close()
        reader.close()
    info["total_s"] = time.perf_counter() - t0
    devroute.report(last_info, info, "s2g")
    if plan.stop:
        raise Stop(plan.stop)
    return 0
