"""Drop-in for the reference's genoToSeq.py: a `.geno` file, or every window or contig of it, as sequence alignments (fasta / phylip).

The work is a byte transpose -- site-major text in, sequence-major text out -- done on the text itself: the reference copies a cell's
characters verbatim (IUPAC codes, `-`, `*`, lower case), which the resident 4-bit rows do not keep.  The per-line and per-cell rules
live in csrc/pg_seq_core.h and run on the device (pg_seq_dev_*: k_seq_lines, k_seq_tile) for blocks of the regular spelling, on the
host (pg_seq_text) for everything else and under PG_SEQ_DEVICE=0.  The names and the selection follow genomics.py:448-453
(makeHaploidNames), 1884-1967 (parseGenoLine, GenoFileReader, parseGenoFile) and 1790-1793 (seqDict); the windows are those of
genomics_general_amd/windows.py (slidingCoordWindows / slidingSitesWindows restated), cut from the positions and scaffold runs of the
blocks; the host keeps, per output sequence, the bytes of the sites no window has left behind yet.  Where the reference dies with a
traceback this driver ends with one message and exit status 2.  Bgzipped input crosses PCIe as its members (k_inflate writes the text
into the tokenizer's slot); `-s x.gz` and `--gzip` outputs are BGZF (gzip-compatible).
"""
import argparse
import ctypes as C
import os
import string
import time

import numpy as np

from . import _lib, devroute, dist, genoio, windows

ERRORS = {
    1: "the line has fewer fields than the header (the reference raises on it)",
    2: "the line has more fields than the header (the reference's addSite asserts)",
    3: "--splitPhased: a genotype is not 2 * ploidy - 1 characters long (the reference asserts, or shifts the sequences against "
       "each other)",
    4: "the position is not an integer of up to 18 digits",
    5: "text that is not ASCII is not supported",
}

ENGINE_EPILOG = ("MI355X engine: blocks of the regular spelling (single tabs, the header's field count, ASCII, cells of 2 * ploidy - 1 "
                 "characters under --splitPhased and of one character otherwise) are transposed on the device, every other block on the "
                 "host.  Under WORLD_SIZE > 1 rank 0 does the whole job.  Environment: PG_SEQ_DEVICE=0 host only; PG_BGZF_DEVICE=0 "
                 "bgzip members inflated by host threads; PG_STREAM_BYTES text bytes per block (default 256 MiB); PG_TIMING=1 blocks "
                 "and times on stderr.")

last_info = {}


class Usage(devroute.Usage):
    prog = "genoToSeq.py"


class SeqCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_cols", "n_seq", "split", "n_to_gap", "exact_cols")]


class SeqBlock(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in ("n_sites", "n_runs", "stride", "seq_bytes")]
                + [(n, C.c_void_p) for n in ("seq", "off", "pos", "run_start", "run_name")]
                + [("err_line", C.c_int64), ("err_code", C.c_int32)])


def make_parser():
    ap = argparse.ArgumentParser(prog="genoToSeq.py", epilog=ENGINE_EPILOG)
    ap.add_argument("-g", "--genoFile", help="Input geno file", action="store", required=False)
    ap.add_argument("-s", "--seqFile", help="Output sequence file", action="store", required=False)
    ap.add_argument("-f", "--format", help="Sequence file format", action="store", required=False, choices=("phylip", "fasta"), default="fasta")
    ap.add_argument("-M", "--mode", help="Output mode for different contigs", action="store", choices=("cat", "windows", "contigs"), default="cat")
    ap.add_argument("-S", "--samples", help="Name of sample(s)", action="store", required=False)
    ap.add_argument("--NtoGap", help="Convert 'N' or 'n' to '-'", action="store_true")
    ap.add_argument("--seqNameFormat", help="Format for sequence names", action="store", required=False,
                    choices=("sample", "contig", "sample_contig", "contig_position", "sample_contig_position"), default="sample")
    ap.add_argument("--splitPhased", help="Split phased genotypes into two (or more, see --ploidy) sequences per sample", action="store_true")
    ap.add_argument("--ploidy", help="Ploidy for each individual. Only necessary when splitting phased sequences", action="store", nargs="+",
                    type=int, default=[2])
    ap.add_argument("--separateFiles", help="Output windows or contigs as separate files", action="store_true")
    ap.add_argument("--gzip", help="gzip output file(s)", action="store_true")
    ap.add_argument("--windType", help="FOR WINDOWS: type of windows to make", action="store", choices=("sites", "coordinate"), default="sites")
    ap.add_argument("--windSize", help="FOR WINDOWS: Window size in bases", type=int, action="store")
    ap.add_argument("--minSites", help="FOR WINDOWS: Minumum sites per window", type=int, action="store")
    ap.add_argument("--stepSize", help="FOR WINDOWS: Step size for coordinate sliding window", type=int, action="store")
    ap.add_argument("--overlap", help="FOR WINDOWS: Overlap for sites sliding window", type=int, action="store")
    ap.add_argument("--maxDist", help="FOR WINDOWS: Maximum span distance for sites window", type=int, action="store")
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


def haploid_names(names, ploidy):
    """makeHaploidNames (genomics.py:448-453): the names and, per name, its sample's place in `names` and its haplotype"""
    ploidy = list(ploidy)
    if len(ploidy) == 1:
        ploidy = ploidy * len(names)
    if any(p < 1 for p in ploidy):
        raise Usage("--ploidy must be 1 or more")
    if all(p == 1 for p in ploidy):
        return list(names), [(k, 0, 1) for k in range(len(names))]
    pd = dict(zip(names, ploidy))
    if any(n not in pd for n in names):
        raise Usage("--ploidy needs one value, or one per sample (the reference raises KeyError)")
    if max(pd.values()) > 26:
        raise Usage("--ploidy above 26 leaves haplotypes without a name")
    return ([n + "_" + letter for n in names for letter in string.ascii_uppercase[:pd[n]]],
            [(k, h, pd[n]) for k, n in enumerate(names) for h in range(pd[n])])


class Plan:
    """the output sequences' names and the selection tables pg_seq_text / pg_seq_dev_config take"""

    def __init__(self, header, args, samples):
        fields = header.split()
        hdr = fields[2:]
        if args.splitPhased:
            names, slots = haploid_names(hdr, args.ploidy)
            cols = [(2 + k, 2 * h, 2 * p - 1) for k, h, p in slots]
        else:
            names, cols = list(hdr), [(2 + k, 0, 0) for k in range(len(hdr))]
        if samples:
            want = haploid_names(samples, args.ploidy)[0] if args.splitPhased else list(samples)
            place = {n: k for k, n in enumerate(names)}            # (dict(zip(names, GTs)): of a name given twice the last column)
            for n in want:
                if n not in place:
                    raise Usage("sequence %s (-S) is not in the header%s" % (n, " as --ploidy names its haplotypes" if args.splitPhased else ""))
            sel = [cols[place[n]] for n in want]
            names = want
        else:
            sel = cols
        if not names:
            raise Usage("the header names no sample")
        first = {}
        for k, n in enumerate(names):                               # seqDict (genomics.py:1790-1793): names.index() finds the first
            first.setdefault(n, k)
        sel = [sel[first[n]] for n in names]
        self.names = names
        self.cfg = SeqCfg(len(fields), len(names), int(args.splitPhased), int(args.NtoGap), int(not samples))
        self.sel_col = np.ascontiguousarray([c for c, _, _ in sel], dtype=np.int32)
        self.sel_off = np.ascontiguousarray([o for _, o, _ in sel], dtype=np.int32)
        self.sel_len = np.ascontiguousarray([w for _, _, w in sel], dtype=np.int32)

    def args(self):
        vp = devroute.vp
        return (C.c_void_p(C.addressof(self.cfg)), vp(self.sel_col), vp(self.sel_off), vp(self.sel_len))


class Chunk:
    """the sites of one block: every sequence's bytes, by a stride (a matrix, one row a sequence) or by offsets"""

    def __init__(self, n, mat=None, stride=0, seq=None, off=None):
        self.n, self.mat, self.stride, self.seq, self.off = n, mat, stride, seq, off

    def slice(self, q, a, b):
        if self.mat is not None:
            return self.mat[q, a * self.stride:b * self.stride].tobytes()
        return self.seq[self.off[q, a]:self.off[q, b]]


def host_seq(plan, text):
    """pg_seq_text on a block of lines: (chunk, positions, run starts, run names, error code, error line, lines)"""
    L = _lib.lib()
    buf = text if isinstance(text, bytes) else bytes(text)
    if b"\r" in buf:                                                # the reference's text-mode file: \r\n and a lone \r end a line
        buf = buf.replace(b"\r\n", b"\n").replace(b"\r", b"\n")
    blk = SeqBlock()
    _lib.check(L.pg_seq_text(*plan.args(), buf, len(buf), C.byref(blk)))
    try:
        n, nq = blk.n_sites, plan.cfg.n_seq
        take = lambda p, count, dt: np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), shape=(max(count, 1),))[:count].copy()   # noqa: E731
        pos = take(blk.pos, n, C.c_int64)
        starts = take(blk.run_start, blk.n_runs, C.c_int64)
        where = take(blk.run_name, 2 * blk.n_runs, C.c_int64).reshape(-1, 2)
        names = [buf[a:a + k].decode("ascii") for a, k in where]
        seq = C.string_at(blk.seq, blk.seq_bytes) if blk.seq_bytes else b""
        if blk.stride:
            chunk = Chunk(n, mat=np.frombuffer(seq, dtype=np.uint8).reshape(nq, n * blk.stride), stride=blk.stride)
        else:
            chunk = Chunk(n, seq=seq, off=take(blk.off, nq * (n + 1), C.c_int64).reshape(nq, n + 1))
        n_lines = buf.count(b"\n") + (0 if buf.endswith(b"\n") or not buf else 1)
        return chunk, pos, starts, names, blk.err_code, blk.err_line, n_lines
    finally:
        L.pg_seq_free(C.byref(blk))


class Device(devroute.SlotDevice):
    """the device route (devroute.SlotDevice): one block transposed while the next is submitted"""

    def __init__(self, plan, device, tile_seqs=0):
        super().__init__(device, "seq")
        self.configure(plan, tile_seqs)

    def configure(self, plan, tile_seqs=0):
        """the option set of the blocks submitted from now on; tile_seqs: output sequences per tile of k_seq_tile (0: as many as
        the LDS holds)"""
        self.plan = plan
        taken = C.c_int()
        _lib.check(self.L.pg_seq_dev_config(self.eng._h, *plan.args(), int(tile_seqs), C.byref(taken)))
        self.taken = bool(taken.value)

    # submit(block): devroute.SlotDevice's

    def collect(self, ticket, padded=False):
        """(chunk, positions, run starts, run names, None, lines), or -- the block is the host's -- (None, ..., its text, the line the
        device does not take).  padded: the chunk's matrix keeps the device's pitch (the tests look at the pad columns)"""
        s = ticket[0]
        ns, hl, nl, pitch = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pg_seq_dev_collect(self.eng._h, s, C.byref(ns), C.byref(hl), C.byref(nl), C.byref(pitch)))
        if hl.value >= 0:
            return None, None, None, None, self.host_text(ticket), hl.value
        n, nq = ns.value, self.plan.cfg.n_seq
        width = pitch.value if padded else n
        mat = self.eng.pinned.empty((nq, max(width, 1)), np.uint8)[:, :width]
        if not mat.flags["C_CONTIGUOUS"]:
            mat = np.ascontiguousarray(mat)
        pos, run, start = np.empty(n, dtype=np.int64), np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.int64)
        vp = devroute.vp
        if n:
            _lib.check(self.L.pg_seq_dev_rows(self.eng._h, s, 0, nq, vp(mat), width, width))
            _lib.check(self.L.pg_seq_dev_meta(self.eng._h, s, vp(pos), vp(run), vp(start)))
        starts = np.flatnonzero(run)
        text_at = self.text_at(ticket)
        names = [devroute.field_at(text_at, int(a)).decode("ascii") for a in start[starts]]
        return Chunk(n, mat=mat, stride=1), pos, starts, names, None, nl.value

    def stats(self):
        """SlotDevice's two counts, and the milliseconds of k_seq_lines and of k_seq_tile"""
        b, h, lm, tm = C.c_int64(), C.c_int64(), C.c_double(), C.c_double()
        _lib.check(self.L.pg_seq_dev_stats(self.eng._h, C.byref(b), C.byref(h), C.byref(lm), C.byref(tm)))
        return b.value, h.value, lm.value, tm.value


class Sites:
    """the sites no window has left behind: their chunks, positions and scaffold runs (rows count from the first kept site)"""

    def __init__(self):
        self.chunks, self.skip = [], 0               # skip: rows of the first chunk that are gone
        self.pos = np.zeros(0, dtype=np.int64)
        self.run_starts, self.run_names = [], []
        self.last_name = None                        # the scaffold of the last site seen

    def append(self, chunk, pos, starts, names):
        n0 = len(self.pos)
        for a, name in zip(starts, names):
            if int(a) == 0 and name == self.last_name:
                if n0 == 0 and not self.run_starts:  # the run goes on, none of its rows was kept
                    self.run_starts.append(0)
                    self.run_names.append(name)
                continue
            self.run_starts.append(n0 + int(a))
            self.run_names.append(name)
        if names:
            self.last_name = names[-1]
        if chunk.n:
            self.chunks.append(chunk)
            self.pos = np.concatenate([self.pos, pos])

    def drop(self, keep_from):
        if keep_from <= 0:
            return
        self.pos = self.pos[keep_from:]
        k = 0
        while k + 1 < len(self.run_starts) and self.run_starts[k + 1] <= keep_from:
            k += 1
        self.run_starts = [max(a - keep_from, 0) for a in self.run_starts[k:]]
        self.run_names = self.run_names[k:]
        if not len(self.pos):
            self.run_starts, self.run_names = [], []
        gone = self.skip + keep_from
        while self.chunks and gone >= self.chunks[0].n:
            gone -= self.chunks.pop(0).n
        self.skip = gone

    def pieces(self, q, lo, hi):
        """the bytes of sequence q over rows [lo, hi), chunk by chunk"""
        a, b = lo + self.skip, hi + self.skip
        at = 0
        for c in self.chunks:
            if at >= b:
                break
            if at + c.n > a:
                yield c.slice(q, max(a - at, 0), min(b - at, c.n))
            at += c.n


def alignment(fmt, names, seqs):
    """makeAlnString (genomics.py:2232-2251) on bytes"""
    out = []
    if fmt == "phylip":
        out.append(b" %d %d" % (len(names), max(len(s) for s in seqs)))
        for n, s in zip(names, seqs):
            out.append(n + b"   " + s)
    else:
        for n, s in zip(names, seqs):
            out.append(b">" + n)
            out.append(s)
    return b"\n".join(out) + b"\n"


def _open_bin(path):
    if path is not None and path.endswith(".gz") and os.environ.get("PG_OUT_GZIP_MODULE"):
        import gzip
        return gzip.open(path, "wb")
    return devroute.open_rows(path)


def _check_args(args):
    windowed = args.mode in ("windows", "contigs")
    if args.separateFiles and not args.seqFile:
        raise Usage("--separateFiles needs -s, the stem of the files' names")
    if args.separateFiles and not windowed:
        raise Usage("--separateFiles applies to -M windows and -M contigs (in cat mode the reference has no file to write to)")
    if not windowed:
        return
    if args.seqNameFormat != "sample":
        raise Usage("--seqNameFormat %s: the reference looks the new names up among the samples and raises KeyError; only `sample` "
                    "works in %s mode" % (args.seqNameFormat, args.mode))
    if args.samples:
        raise Usage("-S in %s mode: the reference takes it for the header line and stops at an assertion" % args.mode)
    if args.mode == "contigs":
        return
    if args.windSize is None or args.windSize < 1:
        raise Usage("-M windows needs --windSize (1 or more)")
    if args.windType == "coordinate":
        if args.stepSize is None or args.stepSize < 1:
            raise Usage("--windType coordinate needs --windSize and --stepSize")
    else:
        if args.maxDist is None:
            raise Usage("--windType sites needs --maxDist (the reference compares a distance with None and raises TypeError)")
        if args.overlap is None:
            raise Usage("--windType sites needs --overlap (the reference's trim asserts)")
        if args.overlap < 0 or args.overlap >= args.windSize:
            raise Usage("--overlap must be 0 or more and below --windSize (the reference never ends otherwise)")


def main(argv=None):
    t0 = time.perf_counter()
    args = make_parser().parse_args(argv)
    world = dist.world_from_env()
    if world.size > 1 and world.rank != 0:                 # rank 0 does the whole job
        return 0
    _check_args(args)
    if args.genoFile is None:
        from .cli import _spool_stdin
        args.genoFile = _spool_stdin()
    reader = genoio.BlockReader(args.genoFile)
    try:
        header = reader.read_header().decode("ascii")
    except UnicodeDecodeError:
        raise Usage("line 1: " + ERRORS[5])
    samples = args.samples.split(",") if args.samples else None
    plan = Plan(header, args, samples)
    names = [n.encode("ascii") for n in plan.names]
    windowed = args.mode in ("windows", "contigs")
    ext = (".fa" if args.format == "fasta" else ".phy") + (".gz" if args.gzip else "")

    stream = None
    if windowed:
        if args.mode == "contigs":
            stream = windows.CoordWindowStream(10 ** 7, 10 ** 7)
        elif args.windType == "coordinate":
            stream = windows.CoordWindowStream(args.windSize, args.stepSize)
        else:
            stream = windows.SitesWindowStream(args.windSize, args.overlap, args.maxDist, args.minSites)
    coord = isinstance(stream, windows.CoordWindowStream)

    out = None
    if not args.separateFiles:
        path = args.seqFile
        if path and args.gzip and not path.endswith(".gz"):
            path += ".gz"
        out = _open_bin(path)

    use_device = os.environ.get("PG_SEQ_DEVICE", "1") != "0"
    dev = None
    if use_device:
        dev_index = args.device if args.device is not None else dist.device_for(world)
        dev = Device(plan, dev_index)
        if not dev.taken:
            dev.close()
            dev = None
    block_bytes = int(os.environ.get("PG_STREAM_BYTES", str(256 << 20)))
    info = dict(blocks=0, blocks_on_device=0, blocks_on_host=0, sites=0, alignments=0, text_bytes=0, blocks_inflated_on_device=0,
                collect_s=0.0, host_s=0.0, window_s=0.0, write_s=0.0)
    sites = Sites()
    lines_done = [1]                                       # lines of the file in front of the block in hand (the header is one)

    def write_windows(final):
        t_a = time.perf_counter()
        try:
            T, keep_from = stream.feed(np.asarray(sites.run_starts, dtype=np.int64), sites.run_names, sites.pos, final)
        except ValueError as exc:
            raise Usage(str(exc))
        info["window_s"] += time.perf_counter() - t_a
        t_a = time.perf_counter()
        for k in range(T.n):
            lo, hi = int(T.lo[k]), int(T.hi[k])
            if hi <= lo:
                raise Usage("window %s:%d-%d holds no site: the reference stops here at min() of no positions, after the windows "
                            "before it" % (T.scaffold[k], T.start[k], T.end[k]))
            text = alignment(args.format, names, [b"".join(sites.pieces(q, lo, hi)) for q in range(len(names))])
            if args.separateFiles:
                name = args.seqFile + "." + T.scaffold[k]
                if args.mode == "windows":
                    name += "_%d_%d" % (int(sites.pos[lo]), int(sites.pos[hi - 1]))
                f = _open_bin(name + ext) if args.gzip else open(name + ext, "wb")
                f.write(text)
                f.close()
            else:
                out.write(text)
            info["alignments"] += 1
        info["write_s"] += time.perf_counter() - t_a
        sites.drop(keep_from)

    def finish(result):
        chunk, pos, starts, run_names, text, at = result
        if chunk is None:
            t_a = time.perf_counter()
            chunk, pos, starts, run_names, err, err_line, n_lines = host_seq(plan, text)
            info["host_s"] += time.perf_counter() - t_a
            info["blocks_on_host"] += 1
        else:
            err, n_lines = 0, at
            info["blocks_on_device"] += 1
        info["sites"] += chunk.n
        sites.append(chunk, pos, starts, run_names)
        if err:
            raise Usage("line %d: %s" % (lines_done[0] + err_line + 1, ERRORS.get(err, "error %d" % err)))
        lines_done[0] += n_lines
        if stream is not None:
            write_windows(False)

    def collect(ticket):
        t_a = time.perf_counter()
        r = dev.collect(ticket)
        info["collect_s"] += time.perf_counter() - t_a
        return r

    ok = False
    try:
        spans = (dev is not None and isinstance(getattr(reader, "f", None), genoio.BgzfFile) and os.environ.get("PG_BGZF_DEVICE", "1") != "0")
        blocks = devroute.read_ahead(devroute.blocks(reader, block_bytes, dev.pinned() if spans else None, info), "pg-seq-read")
        devroute.run_blocks(blocks, dev, info, finish, lambda text, n_lines: finish((None, None, None, None, text, 0)), collect=collect)
        if stream is not None:
            write_windows(True)
        else:                                              # cat: one alignment of everything
            t_a = time.perf_counter()
            n = len(sites.pos)
            if n == 0:
                raise Usage("the file holds no site (the reference stops at max() of no sequence lengths)")
            if args.format == "phylip":
                lens = [sum(len(p) for p in sites.pieces(q, 0, n)) for q in range(len(names))]
                out.write(b" %d %d\n" % (len(names), max(lens)))
            for q, name in enumerate(names):
                out.write((name + b"   ") if args.format == "phylip" else (b">" + name + b"\n"))
                for p in sites.pieces(q, 0, n):
                    out.write(p)
                out.write(b"\n")
            info["alignments"] += 1
            info["write_s"] += time.perf_counter() - t_a
        ok = True
    finally:
        if dev is not None:
            info["device_blocks"], info["device_host_blocks"], info["k_seq_lines_ms"], info["k_seq_tile_ms"] = dev.stats()
            dev.close()
        if out is not None:
            devroute.close_rows(out, ok)
        last_info.clear()
        last_info.update(info)
    info["total_s"] = time.perf_counter() - t0
    devroute.report(last_info, info, "genoToSeq")
    return 0
