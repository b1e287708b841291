"""Drop-in for the reference's mergeGeno.py: `.geno` files joined by site.

The reference walks every position of every scaffold of the `.fai` and compares strings against one pending line per file
(mergeGeno.py:57-88); its cost is the genome's length.  Here the work is a sorted join of text files: every line gets a key (the
scaffold's line in the `.fai`, the position), the keys are matched, bytes are copied.  Every input keeps a block of lines resident; a
ROUND writes the sites up to a horizon -- the smallest last key among the files that may still bring lines -- and carries the rest
(csrc/pg_merge_plan.h).  The per-line rules are csrc/pg_merge_core.h and run on the device (pg_merge_dev_*: k_merge_keys,
k_merge_lines / k_merge_pos, k_merge_emit) for lines of the regular spelling and a one-byte --outSep, on the host (pg_merge_text) for a
round that holds any other line and under PG_MERGE_DEVICE=0.  Bgzipped input crosses PCIe as its members (k_inflate); `-o x.gz` is BGZF
(gzip-compatible), its members made by k_deflate on the device route.

Kept quirks: a file gives only the longest prefix of its lines whose sites are valid and increasing -- the first other line (`03`, a
position beyond the scaffold, an unknown scaffold, a site again, a blank line) STOPS it, one warning on stderr; the header's sample names
follow --outputOnly's order while the cells stay in file order.  Where the reference raises or misbehaves silently this driver ends
with one message and exit status 2.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib, devroute, dist, genoio

MAX_FILES = 32
METHODS = {"intersect": 0, "union": 1, "all": 2}
STOPS = {
    2: "the position is no plain decimal number (the reference compares it with str(position))",
    3: "the position lies outside 1 .. the scaffold's length",
    4: "the scaffold is not in the .fai",
    5: "the site does not lie behind the site of the line before",
    6: "the line has fewer than two fields",
}
ERRORS = {7: "text that is not ASCII is not supported", 8: "a position of more than 18 digits is not supported"}

ENGINE_EPILOG = ("MI355X engine: rounds whose lines are of the regular spelling (fields split by single tabs, no other whitespace, the "
                 "header's field count, ASCII) are joined on the device when --outSep is one byte, every other round on the host.  Under "
                 "WORLD_SIZE > 1 rank 0 does the whole job.  Environment: PG_MERGE_DEVICE=0 host only, =1 the device even for small "
                 "inputs; PG_BGZF_DEVICE=0 bgzip members inflated by host threads; PG_DEFLATE_DEVICE=0 -o x.gz deflated by host threads; "
                 "PG_STREAM_BYTES text bytes resident per round, shared among the files, and as many bytes of output lines no file adds "
                 "to (default 256 MiB); PG_TIMING=1 rounds and times on stderr.")
SMALL_INPUT = 4 << 20                # bytes of input files below which the host route is taken unless PG_MERGE_DEVICE=1

last_info = {}


class Usage(devroute.Usage):
    prog = "mergeGeno.py"


class MergeCfg(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("n_files", "method", "union_min", "must_first")] + [("out_mask", C.c_uint32)]
                + [(n, C.c_int32) for n in ("sep_len", "missing_len", "n_fai")])


class MergeInput(C.Structure):
    _fields_ = [("text", C.c_char_p), ("len", C.c_int64), ("open", C.c_int32), ("n_cols", C.c_int32), ("prev_scaf", C.c_int32),
                ("prev_pos", C.c_int64), ("stop", C.c_int32), ("stop_line", C.c_int64), ("lines_done", C.c_int64), ("bytes_done", C.c_int64)]


class MergeResult(C.Structure):
    _fields_ = [("out", C.c_void_p), ("out_len", C.c_int64), ("rows", C.c_int64), ("from_scaf", C.c_int32), ("hor_scaf", C.c_int32),
                ("from_pos", C.c_int64), ("hor_pos", C.c_int64), ("last", C.c_int32), ("stalled", C.c_int32), ("err_code", C.c_int32),
                ("err_file", C.c_int32), ("err_line", C.c_int64)]


def make_parser():
    ap = argparse.ArgumentParser(prog="mergeGeno.py", epilog=ENGINE_EPILOG)
    ap.add_argument("-i", "--inputFile", help="a .geno file, plain or gzipped (give -i once per file)", action="append", required=True)
    ap.add_argument("-f", "--fai", help="the .fai of the genome: scaffold names and lengths, in the order of the output", action="store", required=True)
    ap.add_argument("-o", "--outputFile", help="where the joined .geno goes (.gz: gzipped); the standard output without it", action="store")
    ap.add_argument("--method", help="which sites are written: those every file holds, those enough files hold, or every position", action="store", choices=("intersect", "union", "all"), default="intersect")
    ap.add_argument("--unionMin", help="--method union: files that must hold a site for it to be written", action="store", type=int, default=1)
    ap.add_argument("--mustIncludeFirst", help="a site is written only if each of the first n files holds it", action="store", type=int, default=0)
    ap.add_argument("--outSep", help="what stands between the fields of an output line", action="store", default="\t")
    ap.add_argument("--missing", help="the cell written for each sample of a file that lacks the site", action="store", default="N")
    ap.add_argument("--outputOnly", help="numbers (from 1) of the files whose samples are written", action="store", type=int, nargs="+")
    ap.add_argument("--verbose", help="accepted; no per-position lines are written", action="store_true")
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


def read_fai(path):
    """the scaffolds' names and lengths, in the file's order (mergeGeno.py:35)"""
    names, lens, seen = [], [], set()
    with open(path, "rb") as f:
        for k, ln in enumerate(f.read().splitlines()):
            fields = ln.split()
            if len(fields) < 2:
                raise Usage("%s line %d: fewer than two fields (the reference raises ValueError)" % (path, k + 1))
            try:
                name = fields[0].decode("ascii")
                digits = fields[1].decode("ascii")
                length = int(digits)
            except (UnicodeDecodeError, ValueError):
                raise Usage("%s line %d: the name is not ASCII or the length is not an integer" % (path, k + 1))
            if len(digits.lstrip("+-").lstrip("0")) > 18:
                raise Usage("%s line %d: a length of more than 18 digits is not supported" % (path, k + 1))
            if name in seen:
                raise Usage("%s line %d: scaffold %s is listed twice (the reference's second visit could restart a stopped file)" % (path, k + 1, name))
            seen.add(name)
            names.append(fields[0])
            lens.append(length)
    return names, lens


class Fai:
    def __init__(self, names, lens):
        self.n = len(names)
        self.blob = b"".join(names)
        self.name_off = np.zeros(self.n + 1, dtype=np.int64)
        if self.n:
            self.name_off[1:] = np.cumsum([len(x) for x in names])
        self.lens = np.ascontiguousarray(lens, dtype=np.int64).reshape(-1)
        self.max_name = max([len(x) for x in names], default=0)
        self.names = names


class _File:
    """one input: its reader, the fields of its header, and what the rounds know of it"""

    def __init__(self, k, path):
        self.k, self.path = k, path
        self.reader = genoio.BlockReader(path)
        head = self.reader.read_header()
        if not head:
            raise Usage("%s is empty: no header line" % path)
        try:
            self.header = head.decode("ascii").split()
        except UnicodeDecodeError:
            raise Usage("%s line 1: %s" % (path, ERRORS[7]))
        self.n_cols = len(self.header)
        self.open, self.stopped = True, False
        self.resident = 0                  # bytes of its resident lines
        self.lines_before = 0              # data lines in front of them
        self.prev = (-1, 0)                # the key of the last line consumed
        self.carry = b""                   # host route: the resident lines
        self.blocks = None


def header_line(files, output_idx, sep):
    """the first file's first two header fields, then one piece per --outputOnly number in that option's order (the cells keep the
    files' order): a file's sample names joined, an empty piece for a file without samples; the pieces joined once more, so that a
    separator stands behind POS even when no name follows"""
    names = [sep.join(files[x].header[2:]) for x in output_idx]
    return sep.join(files[0].header[:2]) + sep + sep.join(names) + "\n"


class Device:
    """the device route: every file's region on the device, a round's keys, join and output (pg_merge_dev_*)"""

    def __init__(self, cfg, sep, missing, fai, n_cols, device, gz_rows=False):
        from .engine import Engine
        self.eng = Engine(device)
        self.L = _lib.lib()
        self.nf = cfg.n_files
        taken = C.c_int()
        self.n_cols = np.ascontiguousarray(n_cols, dtype=np.int32)
        _lib.check(self.L.pg_merge_dev_config(self.eng._h, C.addressof(cfg), sep, missing, fai.blob, fai.name_off.ctypes.data, fai.lens.ctypes.data,
                                              self.n_cols.ctypes.data, C.byref(taken)))
        self.taken = bool(taken.value)
        self.gz_rows = bool(gz_rows) and self.taken
        if self.taken:
            _lib.check(self.L.pg_merge_dev_set_output(self.eng._h, int(self.gz_rows)))
            if os.environ.get("PG_TIMING"):
                _lib.check(self.L.pg_merge_dev_timing(self.eng._h, 1))

    def submit(self, f, block):
        if isinstance(block, genoio.BgzfSpan):
            args, _comp = devroute.span_args(block)
            _lib.check(self.L.pg_merge_dev_submit_bgzf(self.eng._h, f, *args))
        else:
            _lib.check(self.L.pg_merge_dev_submit(self.eng._h, f, block, len(block)))

    def keys(self):
        info = np.zeros((self.nf, 8), dtype=np.int64)
        _lib.check(self.L.pg_merge_dev_keys(self.eng._h, info.ctypes.data))
        return info

    def merge(self, dense, frm, hor):
        """(text or None, BGZF members or None, rows, lines and bytes consumed per file)"""
        done = np.zeros((self.nf, 4), dtype=np.int64)
        nb, nr, nz = C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pg_merge_dev_merge(self.eng._h, int(dense), frm[0], frm[1], hor[0], hor[1], done.ctypes.data, C.byref(nb), C.byref(nr),
                                             C.byref(nz)))
        bgzf = bool(self.gz_rows and nz.value)
        n = nz.value if bgzf else nb.value
        out = devroute.fetch(self.L.pg_merge_dev_rows, self.eng._h, n, int(bgzf))
        return (None, out.tobytes(), nr.value, done) if bgzf else (out.tobytes(), None, nr.value, done)

    def advance(self, done, prevs):
        ps = np.ascontiguousarray([p[0] for p in prevs], dtype=np.int32)
        pp = np.ascontiguousarray([p[1] for p in prevs], dtype=np.int64)
        done = np.ascontiguousarray(done, dtype=np.int64)
        _lib.check(self.L.pg_merge_dev_advance(self.eng._h, done.ctypes.data, ps.ctypes.data, pp.ctypes.data))

    def text(self, f, n):
        return devroute.fetch(self.L.pg_merge_dev_text, self.eng._h, n, f).tobytes()

    def pinned(self):
        return self.eng.pinned.empty

    def stats(self):
        r, a, b, c = C.c_int64(), C.c_double(), C.c_double(), C.c_double()
        if not self.taken:
            return 0, 0.0, 0.0, 0.0
        _lib.check(self.L.pg_merge_dev_stats(self.eng._h, C.byref(r), C.byref(a), C.byref(b), C.byref(c)))
        return r.value, a.value, b.value, c.value

    def close(self):
        self.eng.close()


def host_round(cfg, sep, missing, fai, files, texts, frm, out_cap, info):
    """pg_merge_text over the files' resident lines: (the written lines, rows, horizon, last, stalled); the files' prev, lines_before and
    stop state are brought up to date, done[f] = (lines, bytes) consumed"""
    L = _lib.lib()
    ins = (MergeInput * len(files))()
    for f, t in zip(files, texts):
        I = ins[f.k]
        I.text, I.len, I.open, I.n_cols = t, len(t), int(f.open), f.n_cols
        I.prev_scaf, I.prev_pos = f.prev
    res = MergeResult()
    res.from_scaf, res.from_pos = frm
    _lib.check(L.pg_merge_text(C.addressof(cfg), sep, missing, fai.blob, fai.name_off.ctypes.data, fai.lens.ctypes.data, C.addressof(ins), out_cap,
                               C.addressof(res)))
    try:
        if res.err_code:
            f = files[res.err_file]
            raise Usage("%s line %d: %s" % (f.path, f.lines_before + res.err_line + 2, ERRORS.get(res.err_code, "error %d" % res.err_code)))
        out = C.string_at(res.out, res.out_len) if res.out_len else b""
        done = []
        for f in files:
            I = ins[f.k]
            if I.stop:
                note_stop(f, I.stop, I.stop_line, info)
            f.prev = (I.prev_scaf, I.prev_pos)
            done.append((I.lines_done, I.bytes_done))
        return out, res.rows, (res.hor_scaf, res.hor_pos), bool(res.last), bool(res.stalled), done
    finally:
        L.pg_merge_free(C.addressof(res))


def note_stop(f, why, line, info):
    """the file gives nothing from this line on: one warning, one more stopped file in info"""
    if f.stopped:
        return
    f.stopped, f.open = True, False
    info["stopped_files"] += 1
    sys.stderr.write("mergeGeno.py: warning: %s stops at line %d: %s; this line and everything behind it is left out (as the reference "
                     "leaves it out)\n" % (f.path, f.lines_before + line + 2, STOPS.get(int(why), "reason %d" % why)))


def main(argv=None):
    t0 = time.perf_counter()
    args = make_parser().parse_args(argv)
    world = dist.world_from_env()
    if world.size > 1 and world.rank != 0:                 # rank 0 does the whole job
        return 0
    nf = len(args.inputFile)
    if nf > MAX_FILES:
        raise Usage("more than %d input files are not supported" % MAX_FILES)
    output_idx = [i - 1 for i in args.outputOnly] if args.outputOnly else list(range(nf))
    if any(x < 0 or x >= nf for x in output_idx):
        raise Usage("--outputOnly takes file numbers 1 .. %d" % nf)
    try:
        sep, missing = args.outSep.encode("ascii"), args.missing.encode("ascii")
    except UnicodeEncodeError:
        raise Usage("--outSep and --missing must be ASCII")
    fai = Fai(*read_fai(args.fai))
    files = [_File(k, p) for k, p in enumerate(args.inputFile)]

    clamp = lambda v: max(-1, min(int(v), MAX_FILES + 1))   # noqa: E731  (beyond the files' number every value acts alike)
    cfg = MergeCfg(nf, METHODS[args.method], clamp(max(args.unionMin, args.mustIncludeFirst)), clamp(args.mustIncludeFirst),
                   sum(1 << x for x in set(output_idx)), len(sep), len(missing), fai.n)

    gz_out = bool(args.outputFile and args.outputFile.endswith(".gz"))
    out = devroute.open_rows(args.outputFile)
    info = dict(rounds=0, rounds_on_device=0, rounds_on_host=0, blocks=0, blocks_inflated_on_device=0, lines_written=0, stopped_files=0,
                rounds_deflated_on_device=0, text_bytes=0, read_s=0.0, device_s=0.0, host_s=0.0, write_s=0.0)
    dev = None
    ok = False
    try:
        out.write(header_line(files, output_idx, args.outSep).encode("ascii"))
        want = os.environ.get("PG_MERGE_DEVICE", "")
        sizes = sum(os.path.getsize(p) for p in args.inputFile)
        if fai.n and (want == "1" or (want != "0" and sizes >= SMALL_INPUT)):
            dev_index = args.device if args.device is not None else dist.device_for(world)
            dev = Device(cfg, sep, missing, fai, [f.n_cols for f in files], dev_index,
                         gz_rows=gz_out and os.environ.get("PG_DEFLATE_DEVICE", "1") != "0")
            if not dev.taken:
                dev.close()
                dev = None
        stream_bytes = int(os.environ.get("PG_STREAM_BYTES", str(256 << 20)))
        share = max(stream_bytes // nf, 1)
        spans_ok = dev is not None and os.environ.get("PG_BGZF_DEVICE", "1") != "0"
        for f in files:
            spans = spans_ok and isinstance(getattr(f.reader, "f", None), genoio.BgzfFile)
            f.blocks = devroute.blocks(f.reader, share, dev.pinned() if spans else None, info)

        def to_host():
            """the rest of the job is the host route's (a carriage return: the reference's text mode ends a line there)"""
            nonlocal dev
            for f in files:
                f.carry = dev.text(f.k, f.resident).replace(b"\r\n", b"\n").replace(b"\r", b"\n")
                f.resident = len(f.carry)
            dev.close()
            dev = None

        def top_up(force=False):
            t_a = time.perf_counter()
            for f in files:
                while f.open and (f.resident < share or force):
                    blk = next(f.blocks)
                    if not len(blk):
                        f.open = False
                        break
                    info["blocks"] += 1
                    if isinstance(blk, genoio.BgzfSpan):
                        info["blocks_inflated_on_device"] += 1
                    else:
                        if not blk.endswith(b"\n"):
                            blk += b"\n"
                        if b"\r" in blk:
                            if dev is not None:
                                to_host()
                            blk = blk.replace(b"\r\n", b"\n").replace(b"\r", b"\n")
                    if dev is not None:
                        dev.submit(f.k, blk)
                    else:
                        f.carry += bytes(blk)
                    f.resident += len(blk)
                    if force:
                        break
            info["read_s"] += time.perf_counter() - t_a

        def write(text, members, rows):
            t_a = time.perf_counter()
            if members is not None:
                out.write_members(members)
                info["rounds_deflated_on_device"] += 1
            elif text:
                out.write(text)
            info["lines_written"] += rows
            info["write_s"] += time.perf_counter() - t_a

        def consumed(done):
            for f, (n_lines, n_bytes) in zip(files, [tuple(d[:2]) for d in done]):
                f.lines_before += int(n_lines)
                f.resident -= int(n_bytes)
                if dev is None:
                    f.carry = f.carry[int(n_bytes):]

        frm = (0, 0)
        last = fai.n == 0
        force = False
        while not last:
            top_up(force)
            force = False
            if dev is not None:
                t_a = time.perf_counter()
                keys = dev.keys()
                if keys[:, 6].any():                       # a line outside the regular spelling: the round is the host route's
                    texts = [dev.text(f.k, f.resident) for f in files]
                    info["device_s"] += time.perf_counter() - t_a
                    if any(b"\r" in t for t in texts):
                        to_host()
                        continue
                    t_a = time.perf_counter()
                    text, rows, hor, last, stalled, done = host_round(cfg, sep, missing, fai, files, texts, frm, stream_bytes, info)
                    dev.advance(done, [f.prev for f in files])
                    info["host_s"] += time.perf_counter() - t_a
                    if stalled:
                        force = True
                        continue
                    info["rounds"] += 1
                    info["rounds_on_host"] += 1
                    write(text, None, rows)
                    consumed(done)
                    frm = hor
                    continue
                for f in files:
                    if keys[f.k, 4]:
                        note_stop(f, keys[f.k, 4], keys[f.k, 5], info)
                opened = np.ascontiguousarray([int(f.open) for f in files], dtype=np.int32)
                rnd = np.zeros(8, dtype=np.int64)
                _lib.check(dev.L.pg_merge_plan(C.addressof(cfg), fai.lens.ctypes.data, dev.n_cols.ctypes.data, fai.max_name, keys.ctypes.data,
                                               opened.ctypes.data, stream_bytes, frm[0], frm[1], rnd.ctypes.data))
                if rnd[4]:
                    force = True
                    continue
                text, members, rows, done = dev.merge(bool(rnd[6]), (int(rnd[0]), int(rnd[1])), (int(rnd[2]), int(rnd[3])))
                for f in files:
                    f.prev = (int(done[f.k, 2]), int(done[f.k, 3]))
                info["device_s"] += time.perf_counter() - t_a
                info["rounds"] += 1
                info["rounds_on_device"] += 1
                write(text, members, rows)
                consumed(done)
                frm = (int(rnd[2]), int(rnd[3]))
                last = bool(rnd[5])
            else:
                t_a = time.perf_counter()
                text, rows, hor, last, stalled, done = host_round(cfg, sep, missing, fai, files, [f.carry for f in files], frm, stream_bytes, info)
                info["host_s"] += time.perf_counter() - t_a
                if stalled:
                    force = True
                    continue
                info["rounds"] += 1
                info["rounds_on_host"] += 1
                write(text, None, rows)
                consumed(done)
                frm = hor
        ok = True
    finally:
        if dev is not None:
            info["device_rounds"], info["k_merge_keys_ms"], info["k_merge_lines_pos_ms"], info["k_merge_emit_ms"] = dev.stats()
            dev.close()
        for f in files:
            f.reader.close()
        devroute.close_rows(out, ok)
        info["total_s"] = time.perf_counter() - t0
        last_info.clear()
        last_info.update(info)
    devroute.report(last_info, info, "mergeGeno")
    return 0
