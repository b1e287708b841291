"""Drop-in for the reference's VCF_processing/genoToVCF.py: `.geno` sites written as VCF rows -- REF and ALT from the selected samples'
base counts (or a reference fasta), every genotype coded against them.

The per-site and per-cell rules live in csrc/pg_gvcf_core.h and run on the device (pg_gvcf_dev_*: k_gvcf_lines) for blocks of the
regular spelling, on host threads (pg_gvcf_text) for everything else and under PG_GVCF_DEVICE=0.  Header, sample selection, .fai and
fasta handling follow genoToVCF.py:37-79 and parseFasta (genomics.py:2256-2261).  Where the reference dies with a traceback this driver
stops with one message: before any output with exit status 2 (no -f, a -s name the header lacks, a .fai line of fewer than two fields,
text that is not ASCII), at the line otherwise -- the rows before it written.  Divergences: with -r a position below 1 stops the run
(Python's negative index gives the reference a base from the sequence's end); -o x.gz is BGZF.  Bgzipped input crosses PCIe as its
members, inflated by k_inflate into the route's text slot; `-o x.gz` rows are deflated where they lie (k_deflate).
"""
import argparse
import ctypes as C
import os
import re
import sys
import time

import numpy as np

from . import _lib, devroute, dist, genoio

IN_FMT = {"phased": 0, "diplo": 1, "pairs": 2}
ERRORS = {
    1: "the line has fewer cells than the selected samples need, or fewer than two fields (the reference raises KeyError / IndexError)",
    2: "-f diplo: a genotype that is not one of A C G K M N S R T W Y (the reference raises KeyError)",
    3: "the position is not an integer (the reference raises ValueError)",
    4: "-r: the fasta holds no sequence of the line's scaffold (the reference raises KeyError)",
    5: "-r: the position lies beyond the scaffold's sequence (the reference raises IndexError)",
    6: "-r: a position below 1 (the reference takes a base counted from the sequence's end; this is not followed)",
    7: "text that is not ASCII is not supported",
    8: "a position of more than 18 digits is not supported",
    9: "a genotype of more than 16 alleles is not supported",
}
REJECTED = (7, 8, 9)                                   # exit status 2, as for an input the drop-in does not take

ENGINE_EPILOG = ("MI355X engine: blocks of the regular spelling (single tabs, the header's field count, ASCII, positions as plain "
                 "decimals) are converted on the device, every other block on host threads.  Under WORLD_SIZE > 1 rank 0 does the whole "
                 "job.  Environment: PG_GVCF_DEVICE=0 host threads only, =1 the device whatever the input's size; PG_BGZF_DEVICE=0 bgzip "
                 "members inflated by host threads; PG_DEFLATE_DEVICE=0 -o x.gz rows deflated by host threads; PG_STREAM_BYTES text "
                 "bytes per block (default 256 MiB); PG_SCRATCH_GIB the device's budget for the fasta's sequences; PG_HOST_THREADS host "
                 "threads; PG_TIMING=1 blocks and times on stderr.")

last_info = {}


class Usage(devroute.Usage):
    prog = "genoToVCF.py"


class GvcfCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_fmt", "n_sel", "n_cols", "has_ref", "universal_newlines")]


def make_parser():
    ap = argparse.ArgumentParser(prog="genoToVCF.py", epilog=ENGINE_EPILOG)
    ap.add_argument("-g", "--genoFile", help="Input vcf file", action="store")
    ap.add_argument("-f", "--genoFormat", help="Genotype format [otherwise will be inferred (slower)]", action="store",
                    choices=["phased", "diplo", "pairs"])
    ap.add_argument("-o", "--outFile", help="Output vcf file", action="store")
    ap.add_argument("-r", "--reference", help="Reference fasta", action="store")
    ap.add_argument("-s", "--samples", help="Samples to include (separated by commas)", action="store")
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


_WORD = re.compile(rb"[^ \t\n\r\x0b\x0c\x1c-\x1f]+")


def parse_fasta(path):
    """parseFasta(ref.read()) of a file read in text mode: ({name: (offset, length)}, the sequences side by side)"""
    if path.endswith(".gz"):
        import gzip
        with gzip.open(path, "rb") as f:
            raw = f.read()
    else:
        with open(path, "rb") as f:
            raw = f.read()
    if not raw.isascii():
        raise Usage("%s: %s" % (path, ERRORS[7]))
    if b"\r" in raw:
        raw = raw.replace(b"\r\n", b"\n").replace(b"\r", b"\n")
    where, pieces, at = {}, [], 0
    for k, rec in enumerate(raw.split(b">")[1:]):
        m = _WORD.search(rec)
        if m is None:
            raise Usage("%s: record %d has no name (the reference raises IndexError)" % (path, k + 1))
        nl = rec.find(b"\n")
        if nl < 0:
            raise Usage("%s: record %d has no line feed behind its name (the reference raises ValueError)" % (path, k + 1))
        seq = rec[nl:].replace(b"\n", b"").replace(b" ", b"")
        where[m.group()] = (at, len(seq))              # of two records with one name the last wins
        pieces.append(seq)
        at += len(seq)
    return where, b"".join(pieces)


class _Plan:
    """the option set and the fasta in the forms pg_gvcf_text / pg_gvcf_dev_config take"""

    def __init__(self, cfg, sel_col, prev_same, where, seq):
        self.cfg = cfg
        self.sel_col = np.ascontiguousarray(sel_col if len(sel_col) else [0], dtype=np.int32)
        self.prev_same = np.ascontiguousarray(prev_same if len(prev_same) else [-1], dtype=np.int32)
        names = list(where)
        self.n_seq = len(names)
        self.names = b"".join(names)
        self.name_off = np.zeros(self.n_seq + 1, dtype=np.int64)
        np.cumsum([len(n) for n in names], out=self.name_off[1:])
        self.seq_off = np.ascontiguousarray([where[n][0] for n in names] or [0], dtype=np.int64)
        self.seq_len = np.ascontiguousarray([where[n][1] for n in names] or [0], dtype=np.int64)
        self.seq = np.frombuffer(seq if seq else b"\0", dtype=np.uint8)
        self.seq_bytes = len(seq)
        size = 4
        while size < 2 * self.n_seq:
            size <<= 1
        self.mask = size - 1
        self.table = np.empty(size, dtype=np.int32)
        _lib.check(_lib.lib().pg_gvcf_ref_table(self.names, C.c_void_p(self.name_off.ctypes.data), self.n_seq,
                                               C.c_void_p(self.table.ctypes.data), self.mask))

    def ref_args(self):
        vp = devroute.vp
        return (self.names, vp(self.name_off), vp(self.seq_len), vp(self.seq_off), vp(self.table), self.mask, self.n_seq, vp(self.seq))


def host_gvcf(plan, text, n_threads=0):
    """pg_gvcf_text on a block of lines: (rows, error code, line index in the block)"""
    L = _lib.lib()
    buf = text if isinstance(text, bytes) else bytes(text)
    n_threads, vp = devroute.host_threads(n_threads), devroute.vp
    cap = 3 * len(buf) + 40 * (buf.count(b"\n") + buf.count(b"\r") + 1) + 64
    while True:
        out = np.empty(cap, dtype=np.uint8)
        rows_len, n_rows, err_line, err_code = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        _lib.check(L.pg_gvcf_text(C.c_void_p(C.addressof(plan.cfg)), vp(plan.sel_col), vp(plan.prev_same), *plan.ref_args(), buf, len(buf),
                                  n_threads, vp(out), cap, C.byref(rows_len), C.byref(n_rows), C.byref(err_line), C.byref(err_code)))
        if rows_len.value <= cap:
            return out[:rows_len.value].tobytes(), err_code.value, err_line.value
        cap = rows_len.value


class _Device(devroute.SlotDevice):
    """the device route (devroute.SlotDevice): one block converted while the next is submitted; gz_rows: the rows leave the device as
    BGZF members (k_deflate)"""

    def __init__(self, plan, device, gz_rows=False):
        super().__init__(device, "gvcf")
        taken = C.c_int()
        _lib.check(self.L.pg_gvcf_dev_config(self.eng._h, C.c_void_p(C.addressof(plan.cfg)), C.c_void_p(plan.sel_col.ctypes.data),
                                             *plan.ref_args(), plan.seq_bytes, C.byref(taken)))
        self.taken = taken.value
        _lib.check(self.L.pg_gvcf_dev_set_output(self.eng._h, int(bool(gz_rows))))

    # submit(block): devroute.SlotDevice's

    def collect(self, ticket):
        """(rows, members, text, lines): the rows as text or as BGZF members; rows and members None: the block is the host's, `text` its
        text"""
        s = ticket[0]
        rl, nr, hl, bl, nl = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pg_gvcf_dev_collect(self.eng._h, s, C.byref(rl), C.byref(nr), C.byref(hl), C.byref(bl), C.byref(nl)))
        if hl.value >= 0:
            return None, None, self.host_text(ticket), nl.value
        if bl.value:
            return None, (devroute.fetch(self.L.pg_gvcf_dev_rows_bgzf, self.eng._h, bl.value, s).tobytes(), nr.value), None, nl.value
        return devroute.fetch(self.L.pg_gvcf_dev_rows, self.eng._h, rl.value, s).tobytes(), None, None, nl.value


def genovcf_main(argv=None):
    t0 = time.perf_counter()
    args = make_parser().parse_args(argv)
    world = dist.world_from_env()
    if world.size > 1 and world.rank != 0:                 # rank 0 does the whole job
        return 0
    if not args.genoFormat:
        raise Usage("-f phased|diplo|pairs is needed (the reference raises ValueError at the first site)")
    shown = args.genoFile or "<stdin>"
    universal = args.genoFile is not None                  # (a file in text mode; stdin keeps its \r inside the line)

    scafs_lengths, where, seq = None, {}, b""
    if args.reference:
        sys.stderr.write("Parsing reference. This could take a while...\n")
        try:
            with open(args.reference + ".fai", "rt") as fai:
                scafs_lengths = [line.split()[:2] for line in fai]
        except Exception:
            sys.stderr.write("WARNING: Could not parse fai file, vcf header will not contain contig entries...\n")
            scafs_lengths = None
        where, seq = parse_fasta(args.reference)
        if where and scafs_lengths:
            for k, sl in enumerate(scafs_lengths):
                if len(sl) < 2:
                    raise Usage("%s.fai line %d: fewer than two fields (the reference raises IndexError)" % (args.reference, k + 1))
                if not (sl[0] + sl[1]).isascii():
                    raise Usage("%s.fai line %d: %s" % (args.reference, k + 1, ERRORS[7]))

    reader = genoio.BlockReader(args.genoFile)
    headers, carry = devroute.geno_header(reader, universal, shown, Usage)
    all_names = headers[2:]
    names_to_use = args.samples.split(",") if args.samples else all_names
    if not all(n.isascii() for n in names_to_use):
        raise Usage("-s: " + ERRORS[7])
    last_col = {n: k + 2 for k, n in enumerate(all_names)}     # a name the header holds twice: its last field
    for n in names_to_use:
        if n not in last_col:
            raise Usage("-s: sample %s is not in the header (the reference raises KeyError at the first site)" % n)
    if not names_to_use:
        raise Usage("%s line 1: the header names no sample (the reference stops at an assertion at the first site)" % shown)
    prev_same, seen = [-1] * len(headers), {}
    for k, n in enumerate(all_names):
        prev_same[k + 2] = seen.get(n, -1)
        seen[n] = k + 2

    cfg = GvcfCfg()
    cfg.in_fmt = IN_FMT[args.genoFormat]
    cfg.n_sel = len(names_to_use)
    cfg.n_cols = len(headers)
    cfg.has_ref = int(bool(where))
    cfg.universal_newlines = int(universal)
    plan = _Plan(cfg, [last_col[n] for n in names_to_use], prev_same, where, seq)

    out = devroute.open_rows(args.outFile)
    ok = False
    try:
        top = ["##fileformat=VCFv4.2\n"]
        if where:
            top.append("##reference=file:{}\n".format(args.reference.split("/")[-1]))
            if scafs_lengths:
                top += ["##contig=<ID={},length={}>\n".format(sl[0], sl[1]) for sl in scafs_lengths]
        top.append('##FORMAT=<ID=GT,Number=1,Type=String,Description="Genotype">\n')
        top.append("#CHROM\tPOS\tID\tREF\tALT\tQUAL\tFILTER\tINFO\tFORMAT\t" + "\t".join(names_to_use) + "\n")
        out.write("".join(top).encode("ascii"))
        sys.stderr.write("Converting...\n")
        rc = _run(args, reader, out, plan, carry, shown, world, t0)
        ok = rc == 0
        return rc
    finally:
        devroute.close_rows(out, ok)


def _run(args, reader, out, plan, carry, shown, world, t0):
    cfg = plan.cfg
    use_device = os.environ.get("PG_GVCF_DEVICE", "1") != "0"
    dev = None
    gz_out = bool(args.outFile and args.outFile.endswith(".gz"))
    if use_device:
        dev_index = args.device if args.device is not None else dist.device_for(world)
        dev = _Device(plan, dev_index, gz_rows=gz_out and os.environ.get("PG_DEFLATE_DEVICE", "1") != "0")
        if dev.taken != 1:
            if dev.taken < 0:
                sys.stderr.write("genoToVCF.py: the fasta's %d bytes of sequence exceed the device's scratch budget (PG_SCRATCH_GIB): "
                                 "host threads do the job\n" % plan.seq_bytes)
            dev.close()
            dev = None
    block_bytes = int(os.environ.get("PG_STREAM_BYTES", str(256 << 20)))
    n_threads = int(os.environ.get("PG_HOST_THREADS", "0"))
    info = dict(blocks=0, blocks_on_device=0, blocks_on_host=0, rows=0, text_bytes=0, blocks_inflated_on_device=0)
    t_ctx = time.perf_counter()
    done = [1]                              # lines of the file in front of the block in hand (the header is one)

    def finish(result):
        """a block's result -> out; returns an exit code or None"""
        rows, members, text, n_lines = result
        if members is not None:
            out.write_members(members[0])
            info["blocks_on_device"] += 1
            info["rows"] += members[1]
        else:
            if rows is None:
                rows, err, at = host_gvcf(plan, text, n_threads)
                info["blocks_on_host"] += 1
                if err:
                    out.write(rows)
                    sys.stderr.write("genoToVCF.py: %s line %d: %s\n" % (shown, done[0] + at + 1, ERRORS.get(err, "error %d" % err)))
                    return 2 if err in REJECTED else 1
            else:
                info["blocks_on_device"] += 1
            out.write(rows)
            info["rows"] += rows.count(b"\n")
        done[0] += n_lines
        return None

    spans = (dev is not None and not carry and isinstance(getattr(reader, "f", None), genoio.BgzfFile)
             and os.environ.get("PG_BGZF_DEVICE", "1") != "0")
    blocks = devroute.read_ahead(devroute.blocks(reader, block_bytes, dev.pinned() if spans else None, info), "pg-gvcf-read")
    rc = devroute.run_blocks(blocks, dev, info, finish, lambda text, n_lines: finish((None, None, text, n_lines)),
                             universal=bool(cfg.universal_newlines), carry=carry)
    if rc:
        return rc
    if dev is not None:
        info["device_blocks"], info["device_host_blocks"] = dev.stats()
        dev.close()
    info["total_s"] = time.perf_counter() - t0
    info["gvcf_s"] = time.perf_counter() - t_ctx
    devroute.report(last_info, info, "gvcf")
    return 0


def main():
    return genovcf_main()
