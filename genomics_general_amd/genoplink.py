"""Drop-in for the reference's tools/genoToPlink.py: a `.geno` file written as PLINK .ped / .map (and .fam) files -- a row per sample
with the alleles of every site, a line per site.

The work is a byte transpose in which a cell expands into its alleles, each followed by a blank.  The per-cell rules live in
csrc/pg_ped_core.h and run on the device (pg_ped_dev_*: k_ped_lines, k_ped_map, k_ped_tile) for blocks of the regular spelling whose
cells are as long as those of the file's first site, on host threads (pg_ped_text) for everything else and under PG_PED_DEVICE=0.
The reference zips the cells of one sample within one run of a scaffold (genomics.py:390-396), which cuts every one of them to the
run's shortest: each block keeps, per run and sample, the shortest cell it saw and bytes rendered at that length; the cut to the
whole run's shortest -- a prefix of every site's bytes -- is applied when the .ped is written, so a block rendered on the device can
still be cut by a later one.  Header, names and selection follow genomics.py:1914-1945 and 2176-2223.  The reference writes nothing
before everything is read, so neither does this driver: the .ped lives in host memory until the input ends, and every failure leaves
no output file -- a command line or a header the drop-in does not take ends with one message and exit status 2, a line the reference
dies on with one message naming it and exit status 1.  Divergence: a name given twice by -s, or held twice by the header among the
samples used, is rejected (the reference then writes that sample's alleles twice over, run by run).  Bgzipped input crosses PCIe as
its members, inflated by k_inflate into the route's text slot.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib, devroute, dist, genoio

FMT = {"phased": 0, "diplo": 1, "haplo": 2, "pairs": 2, "alleles": 2}
DEV_ALLELES = 4                                            # PG_PED_DEV_ALLELES: alleles of a cell the device takes
ERRORS = {
    1: "a blank line or a line of one field (the reference raises IndexError)",
    2: "-f diplo: a genotype that is not one of A C G K M N S R T W Y (the reference raises KeyError)",
    3: "the position is not an integer (the reference raises ValueError)",
    4: "the line does not hold the header's number of genotypes (the reference's addSite asserts)",
    5: "the line ends before the genotype of a sample -s names (the reference raises KeyError)",
    7: "text that is not ASCII is not supported",
    8: "a position of more than 18 digits is not supported",
}

ENGINE_EPILOG = ("MI355X engine: blocks of the regular spelling (single tabs, the header's field count, ASCII, positions as plain "
                 "decimals) whose genotypes are as long as those of the file's first site -- at most %d alleles each, an odd length "
                 "under phased -- are converted on the device, every other block on host threads.  The PED rows stay in host memory "
                 "until the input ends.  Under WORLD_SIZE > 1 rank 0 does the whole job.  Environment: PG_PED_DEVICE=0 host threads "
                 "only; PG_BGZF_DEVICE=0 bgzip members inflated by host threads; PG_STREAM_BYTES text bytes per block (default 256 "
                 "MiB); PG_HOST_THREADS host threads; PG_TIMING=1 blocks and times on stderr." % DEV_ALLELES)

last_info = {}


class Usage(devroute.Usage):
    prog = "genoToPlink.py"


class Stop(devroute.Stop):
    prog = "genoToPlink.py"


class PedCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("fmt", "n_sel", "n_cols", "exact_cols")]


class PedBlock(C.Structure):
    _fields_ = ([(n, C.c_int64) for n in ("n_sites", "n_runs", "seq_bytes", "map_bytes")]
                + [(n, C.c_void_p) for n in ("seq", "seq_off", "run_start", "run_name", "run_min", "map")]
                + [("err_line", C.c_int64), ("err_code", C.c_int32)])


def make_parser():
    ap = argparse.ArgumentParser(prog="genoToPlink.py", epilog=ENGINE_EPILOG)
    ap.add_argument("-g", "--genoFile", help="Input vcf file", action="store")
    ap.add_argument("-f", "--genoFormat", action="store", choices=["haplo", "diplo", "pairs", "alleles", "phased"], default="phased",
                    help="Genotype format [otherwise will be inferred (slower)]")
    ap.add_argument("--prefix", help="Output file prefix for PED and MAP files", action="store")
    ap.add_argument("--makeFAM", help="Make FAM file (assumes all unrelated)", action="store_true")
    ap.add_argument("--FAMprefix", help="Output file prefix for FAM file", action="store")
    ap.add_argument("-s", "--samples", help="sample names", nargs="+", action="store")
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


_vp = devroute.vp


def alleles(fmt, m):
    """pgp_alleles on an array of cell lengths"""
    m = np.asarray(m, dtype=np.int64)
    return (m + 1) // 2 if fmt == 0 else np.full_like(m, 2) if fmt == 1 else m


class Plan:
    """the option set and the selected columns in the forms pg_ped_text / pg_ped_dev_config take"""

    def __init__(self, fmt, n_cols, sel_col, exact):
        self.cfg = PedCfg(fmt, len(sel_col), n_cols, int(exact))
        self.sel_col = np.ascontiguousarray(sel_col, dtype=np.int32)


class Block:
    """the sites of one block.  Run r of the block (names[r], run_n[r] sites) holds, for sample q, run_n[r] x wid[r, q] bytes at
    data[off[r, q]:] -- every site's alleles, each followed by a blank --; mins[r, q] is the shortest cell seen"""

    def __init__(self, names, run_n, mins, wid, off, data, map_rows):
        self.names, self.run_n, self.mins, self.wid, self.off, self.data, self.map = names, run_n, mins, wid, off, data, map_rows

    @property
    def n(self):
        return int(self.run_n.sum())


def host_ped(plan, text, n_threads=0):
    """pg_ped_text on a block of lines ended by \\n: (block, error code, line index in the block)"""
    L = _lib.lib()
    buf = text if isinstance(text, bytes) else bytes(text)
    n_threads = devroute.host_threads(n_threads)
    blk = PedBlock()
    _lib.check(L.pg_ped_text(C.c_void_p(C.addressof(plan.cfg)), _vp(plan.sel_col), buf, len(buf), n_threads, C.byref(blk)))
    try:
        if blk.err_code:
            return None, blk.err_code, blk.err_line
        nr, nq = blk.n_runs, plan.cfg.n_sel
        take = lambda p, count, dt: np.ctypeslib.as_array(C.cast(p, C.POINTER(dt)), shape=(max(count, 1),))[:count].copy()   # noqa: E731
        starts = take(blk.run_start, nr, C.c_int64)
        where = take(blk.run_name, 2 * nr, C.c_int64).reshape(-1, 2)
        names = [buf[a:a + k] for a, k in where]
        run_n = np.diff(np.concatenate([starts, [blk.n_sites]])).astype(np.int64)
        mins = take(blk.run_min, nr * nq, C.c_int32).reshape(nr, nq).astype(np.int64)
        wid = 2 * alleles(plan.cfg.fmt, mins)
        seq_off = take(blk.seq_off, nq + 1, C.c_int64)
        sizes = run_n[:, None] * wid
        off = seq_off[None, :nq] + np.cumsum(sizes, axis=0) - sizes
        data = np.frombuffer(C.string_at(blk.seq, blk.seq_bytes) if blk.seq_bytes else b"", dtype=np.uint8)
        map_rows = C.string_at(blk.map, blk.map_bytes) if blk.map_bytes else b""
        return Block(names, run_n, mins, wid, off, data, map_rows), 0, -1
    finally:
        L.pg_ped_free(C.byref(blk))


def matrix_block(sel_len, w, woff, pitch, data, map_rows, run, start, text_at):
    """the block of a device matrix: sample q's w[q] bytes a site begin at woff[q] x pitch; run / start: per site 1 where it opens a
    run, where its line begins in the text; text_at(a, k): the text's bytes [a, a + k)"""
    starts = np.flatnonzero(run)
    names = [devroute.field_at(text_at, int(a)) for a in start[starts]]
    nr, nq, n = len(starts), len(w), len(run)
    run_n = np.diff(np.concatenate([starts, [n]])).astype(np.int64)
    mins = np.broadcast_to(np.asarray(sel_len, dtype=np.int64), (nr, nq))
    wid = np.broadcast_to(w, (nr, nq))
    off = woff[None, :] * pitch + starts[:, None].astype(np.int64) * w[None, :]
    return Block(names, run_n, mins, wid, off, data, map_rows)


class _Device(devroute.SlotDevice):
    """the device route (devroute.SlotDevice): one block transposed while the next is submitted"""

    def __init__(self, plan, device, sel_len, tile_seqs=0):
        super().__init__(device, "ped")
        self.plan = plan
        self.sel_len = np.ascontiguousarray(sel_len, dtype=np.int32)
        taken = C.c_int()
        _lib.check(self.L.pg_ped_dev_config(self.eng._h, C.c_void_p(C.addressof(plan.cfg)), _vp(plan.sel_col), _vp(self.sel_len), int(tile_seqs),
                                            C.byref(taken)))
        self.taken = bool(taken.value)
        self.w = 2 * alleles(plan.cfg.fmt, self.sel_len)
        self.woff = np.cumsum(self.w) - self.w

    # submit(block): devroute.SlotDevice's

    def tile_seqs(self):
        t = C.c_int()
        _lib.check(self.L.pg_ped_dev_tile_seqs(self.eng._h, C.byref(t)))
        return t.value

    def collect(self, ticket):
        """(block, None, lines), or -- the block is the host's -- (None, its text, lines)"""
        s = ticket[0]
        ns, ml, hl, nl, pitch = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pg_ped_dev_collect(self.eng._h, s, C.byref(ns), C.byref(ml), C.byref(hl), C.byref(nl), C.byref(pitch)))
        if hl.value >= 0:
            return None, self.host_text(ticket), nl.value
        n = ns.value
        # (the matrix up to the last sample's last site, into pageable memory: the rows stay until the input ends, and page-locking
        # them cost more than the faster copy gave back, 0.09 s on 240 MB)
        data = devroute.fetch(self.L.pg_ped_dev_rows, self.eng._h, int(self.woff[-1]) * pitch.value + n * int(self.w[-1]) if n else 0, s, 0)
        map_rows = devroute.fetch(self.L.pg_ped_dev_rows, self.eng._h, ml.value, s, 1).tobytes()
        run, start = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.int64)
        if n:
            _lib.check(self.L.pg_ped_dev_meta(self.eng._h, s, _vp(run), _vp(start)))
        return matrix_block(self.sel_len, self.w, self.woff, pitch.value, data, map_rows, run, start, self.text_at(ticket)), None, nl.value


def first_site_lengths(line, plan):
    """the selected cells' lengths at the file's first site (the device's widths), None when the line is not the header's fields"""
    f = line.split()
    if len(f) != plan.cfg.n_cols:
        return None
    return [len(f[c]) for c in plan.sel_col]


def join_runs(blocks):
    """the file's runs: [name, [(block, run of the block), ...]] -- a block's first run goes on with the run before it when the
    scaffold is the same"""
    runs = []
    for b in blocks:
        for r, name in enumerate(b.names):
            if r == 0 and runs and runs[-1][0] == name:
                runs[-1][1].append((b, r))
            else:
                runs.append([name, [(b, r)]])
    return runs


def write_ped(f, names, runs, fmt):
    """tools/genoToPlink.py:61-64: a row per sample, every site's alleles cut to what the run's shortest cell of the sample gives"""
    final = [2 * alleles(fmt, np.min([b.mins[r] for b, r in segs], axis=0)) for _, segs in runs]
    for q, name in enumerate(names):
        f.write(b"0 " + name + b" 0 0 0 0 ")
        pieces = []
        for (_, segs), fin in zip(runs, final):
            keep = int(fin[q])
            for b, r in segs:
                n, w, o = int(b.run_n[r]), int(b.wid[r, q]), int(b.off[r, q])
                arr = b.data[o:o + n * w]
                if keep < w:
                    arr = arr.reshape(n, w)[:, :keep].reshape(-1)
                if len(arr):
                    pieces.append(arr)
        if pieces:
            pieces[-1] = pieces[-1][:-1]                       # (the row's last blank)
        for p in pieces:
            f.write(memoryview(np.ascontiguousarray(p)))
        f.write(b"\n")


def main(argv=None):
    t0 = time.perf_counter()
    args = make_parser().parse_args(argv)
    world = dist.world_from_env()
    if world.size > 1 and world.rank != 0:                 # rank 0 does the whole job
        return 0
    if not args.genoFile and args.prefix is None:
        raise Usage("without -g the input is the standard input: --prefix is needed (the reference stops at an assertion)")
    prefix = args.prefix if args.prefix else args.genoFile.rsplit(".", 1)[0]
    shown = args.genoFile or "<stdin>"
    universal = args.genoFile is not None                  # (a file in text mode; stdin keeps its \r inside the line)
    fmt = FMT[args.genoFormat]

    reader = genoio.BlockReader(args.genoFile)
    headers, carry = devroute.geno_header(reader, universal, shown, Usage)
    all_names = headers[2:]
    if not all_names:
        raise Usage("%s line 1: the header names no sample" % shown)
    if args.samples is not None:
        if not all(s.isascii() for s in args.samples):
            raise Usage("-s: " + ERRORS[7])
        for s in args.samples:
            if s not in all_names:
                raise Usage("-s: sample %s is not in the header (the reference raises KeyError at the first site)" % s)
        if len(set(args.samples)) != len(args.samples):
            raise Usage("-s names a sample twice (the reference then writes its alleles twice over, run by run; this is not followed)")
        used = list(args.samples)
    else:
        used = all_names
    for n in used:
        if all_names.count(n) > 1:
            raise Usage("%s line 1: the header holds sample %s more than once (the reference then writes its alleles twice over, run "
                        "by run; this is not followed)" % (shown, n))
    plan = Plan(fmt, len(headers), [2 + all_names.index(n) for n in used], args.samples is None)
    names = [n.encode("ascii") for n in used]

    n_threads = int(os.environ.get("PG_HOST_THREADS", "0"))
    block_bytes = int(os.environ.get("PG_STREAM_BYTES", str(256 << 20)))
    info = dict(blocks=0, blocks_on_device=0, blocks_on_host=0, sites=0, text_bytes=0, blocks_inflated_on_device=0)
    t_ctx = time.perf_counter()
    blocks_done = []
    lines_done = [1]                                       # lines of the file in front of the block in hand (the header is one)

    def finish(result):
        blk, text, n_lines = result
        if blk is None:
            buf = bytes(text)
            if universal and b"\r" in buf:                 # the reference's text-mode file: \r\n and a lone \r end a line
                buf = buf.replace(b"\r\n", b"\n").replace(b"\r", b"\n")
            blk, err, at = host_ped(plan, buf, n_threads)
            info["blocks_on_host"] += 1
            if err:
                raise Stop("%s line %d: %s" % (shown, lines_done[0] + at + 1, ERRORS.get(err, "error %d" % err)))
            n_lines = buf.count(b"\n") + (0 if buf.endswith(b"\n") or not buf else 1)
        else:
            info["blocks_on_device"] += 1
        info["sites"] += blk.n
        blocks_done.append(blk)
        lines_done[0] += n_lines

    def host(text, n_lines=0):              # (finish counts the lines itself, behind the \r rule)
        finish((None, text, 0))

    # the lines up to the file's first site: their block is the host's, the site's cells set the widths the device is given
    peek = [carry] if carry else []
    first = None
    while first is None and not carry:
        line = reader.read_header()
        if not line:
            break
        peek.append(line)
        info["text_bytes"] += len(line)
        if not line.startswith(b"#"):
            first = line
    dev = None
    if os.environ.get("PG_PED_DEVICE", "1") != "0" and first is not None and first.isascii() and b"\r" not in first:
        lens = first_site_lengths(first, plan)
        if lens is not None:
            dev = _Device(plan, args.device if args.device is not None else dist.device_for(world), lens,
                          int(os.environ.get("PG_PED_TILE_SEQS", "0")))
            if not dev.taken:
                dev.close()
                dev = None
            else:
                info["tile_seqs"] = dev.tile_seqs()
    try:
        if peek:
            info["blocks"] += 1
            host(b"".join(peek))
        spans = (dev is not None and isinstance(getattr(reader, "f", None), genoio.BgzfFile) and os.environ.get("PG_BGZF_DEVICE", "1") != "0")
        blocks = devroute.read_ahead(devroute.blocks(reader, block_bytes, dev.pinned() if spans else None, info), "pg-ped-read")
        devroute.run_blocks(blocks, dev, info, finish, host)
        if dev is not None:
            info["device_blocks"], info["device_host_blocks"] = dev.stats()
        _write(args, prefix, names, fmt, blocks_done, shown, info, t0, t_ctx)
    finally:
        t_close = time.perf_counter()
        if dev is not None:
            dev.close()
    info["close_s"] = time.perf_counter() - t_close
    devroute.report(last_info, info, "ped")
    return 0


def _write(args, prefix, names, fmt, blocks_done, shown, info, t0, t_ctx):
    """tools/genoToPlink.py:56-79: the files, once everything is read"""
    runs = join_runs(blocks_done)
    if not runs:
        raise Stop("%s: the file holds no site (the reference raises TypeError at the end of the input)" % shown)
    for k in range(len(runs)):
        sys.stderr.write("%d scaffolds read into memory\n" % (k + 1))
    t_read = time.perf_counter()
    sys.stderr.write("Writing PED file...\n")
    with open(prefix + ".ped", "wb") as f:
        write_ped(f, names, runs, fmt)
    sys.stderr.write("Writing MAP file...\n")
    with open(prefix + ".map", "wb") as f:
        for b in blocks_done:
            f.write(b.map)
    if args.makeFAM:
        sys.stderr.write("Writing FAM file...\n")
        with open(args.FAMprefix if args.FAMprefix else prefix + ".fam", "wb") as f:
            f.write(b"".join(b"0 " + n + b" 0 0 0 0\n" for n in names))
    info["runs"] = len(runs)
    info["total_s"] = time.perf_counter() - t0
    info["read_s"] = t_read - t_ctx
    info["write_s"] = time.perf_counter() - t_read
