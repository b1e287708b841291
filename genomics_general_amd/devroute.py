"""What the drivers of the per-line device routes share (parseVCF: vcf.py, filterGenotypes: filtergeno.py, genoToSeq: genoseq.py,
mergeGeno: mergegeno.py, genoToVCF: genovcf.py, genoToEigenstrat: genoeig.py, genoToPlink: genoplink.py, seqToGeno: seqgeno.py): a
bgzipped block's arguments for the library, the fetch of a result into host memory, the input in blocks read ahead by a thread, the
block pipeline -- submit block k+1, then collect and finish block k (run_blocks) --, the two text slots a route alternates between
(csrc/pg_line_slot.h: submit, parse, collect), and the drivers' small change: their exits, a .geno header, the rows' output file, the
PG_TIMING line."""
import ctypes as C
import os
import queue
import sys
import threading

import numpy as np

from . import _lib


class _Exit(SystemExit):
    prog, status = "", 0

    def __init__(self, msg):
        sys.stderr.write(self.prog + ": " + msg + "\n")
        super().__init__(self.status)


class Usage(_Exit):
    """a command line or an input the drop-in (`prog`, set by each driver's subclass) does not take: one line on stderr, exit status 2"""
    status = 2


class Stop(_Exit):
    """a line the reference dies on: one line on stderr, exit status 1"""
    status = 1


def host_threads(n=0):
    """n, or -- 0 -- the CPUs this process may use, 64 at the most"""
    return n or min(len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1), 64)


def vp(a):
    return C.c_void_p(a.ctypes.data)


def geno_header(reader, universal, shown, Usage):
    """the fields of a .geno file's header line and, universal (a file in text mode), what stood behind a \\r in it: the header ends
    where the text-mode file ends it, the rest is the first block's"""
    head = reader.read_header()
    carry = b""
    if universal and b"\r" in head:
        head, _, carry = head.partition(b"\r")
        carry = carry[1:] if carry.startswith(b"\n") else carry
    if not head:
        raise Usage("%s is empty: no header line" % shown)
    if not head.isascii():
        raise Usage("%s line 1: text that is not ASCII is not supported" % shown)
    return head.decode("ascii").split(), carry


def open_rows(path):
    """where the rows go: a BGZF file (x.gz), a file, or the standard output"""
    if not path:
        return sys.stdout.buffer
    if path.endswith(".gz"):
        from .genoio import BgzfWriter
        return BgzfWriter(path)
    return open(path, "wb")


def close_rows(out, ok):
    """the end of open_rows' output; not ok: a .gz begun is aborted"""
    if out is sys.stdout.buffer:
        out.flush()
    elif ok or not hasattr(out, "abort"):
        out.close()
    else:
        out.abort()


def report(last_info, info, name):
    """a run's counters and times into the driver's last_info and, under PG_TIMING, on stderr"""
    last_info.clear()
    last_info.update(info)
    if os.environ.get("PG_TIMING"):
        sys.stderr.write("PG_TIMING %s %s\n" % (name, " ".join("%s=%s" % kv for kv in sorted(info.items()))))


def is_span(block):
    """a genoio.BgzfSpan (members still deflated), not text"""
    return hasattr(block, "tab")


def span_args(span):
    """a genoio.BgzfSpan as the library's entry points take it -- (comp, comp_len, in_off, in_len, out_len, crc, n_members, head,
    head_len, text_len) -- and what must stay alive while the device reads the members"""
    in_off, in_len, out_len, crc = span.tab
    vp = lambda a: C.c_void_p(a.ctypes.data if a.size else 0)               # noqa: E731
    comp = np.frombuffer(span.comp, dtype=np.uint8)
    head = bytes(span.head)
    return (vp(comp), comp.size, vp(in_off), vp(in_len), vp(out_len), vp(crc), len(in_off), head, len(head), len(span)), comp


def fetch(fn, handle, n, *lead):
    """n bytes of a result: fn(handle, *lead, destination, n) into a new uint8 array"""
    out = np.empty(max(n, 1), dtype=np.uint8)[:n]
    _lib.check(fn(handle, *lead, C.c_void_p(out.ctypes.data), n))
    return out


def blocks(reader, block_bytes, spans, info):
    """the input in blocks of whole lines: bytes, or -- spans: a bgzipped input the device takes as it is -- genoio.BgzfSpan (members
    still deflated, inflated on the device into the route's own text slot); an empty block at the end"""
    if spans:
        reader.spans = True
        reader.f.alloc = spans                  # (the members land in page-locked memory)
    while True:
        blk = reader.read_block(block_bytes)
        if not is_span(blk):
            blk = bytes(blk)
        info["text_bytes"] += len(blk)
        yield blk
        if not len(blk):
            return


def read_ahead(blocks, name, depth=2):
    """the blocks of an iterator, produced by a thread (`name`) `depth` blocks ahead of the consumer (the reading and inflating of the
    next blocks beside the work on this one).  A consumer that stops early sets `stop` and empties the queue until the thread has
    ended: the thread looks at `stop` while it waits for room, and its last put -- the end marker, or an exception -- is freed by
    that emptying"""
    q = queue.Queue(depth)
    stop = threading.Event()
    done = object()

    def run():
        try:
            for body in blocks:
                while not stop.is_set():
                    try:
                        q.put(body, timeout=0.1)
                        break
                    except queue.Full:
                        pass
                if stop.is_set():
                    break
            q.put(done)
        except BaseException as exc:
            q.put(exc)

    th = threading.Thread(target=run, name=name, daemon=True)
    th.start()
    try:
        while True:
            body = q.get()
            if isinstance(body, BaseException):
                raise body
            if body is done:
                return
            yield body
    finally:
        stop.set()
        while th.is_alive():
            try:
                q.get_nowait()
            except queue.Empty:
                pass
            th.join(0.05)


def run_blocks(blocks, dev, info, finish, host, submit=None, collect=None, universal=False, carry=b"", cut=None):
    """The block pipeline of a per-line driver: block k+1 is submitted before block k is collected and finished, so that its copy (or
    its members' inflation) runs beside the kernels of the block before; the last block is collected when the input has ended.

    blocks: read_ahead(blocks(...)), ended by an empty block; dev None: every block is the host's.  submit(block) -> ticket and
    collect(ticket) -> result are the device's own unless the driver gives closures; finish(result) and host(text, n_lines) ->
    None, or an exit code that ends the run (they may raise as well); the block on the device is collected and finished before a
    block goes to host().  A span is submitted as it is.  Text
    has `carry` joined in front; universal: from the first \\r on the rest of the input is the host's, in one piece (a text-mode
    file ends lines there, which only the host route does).  cut(data, lines_before, eof) -> (data, carry) holds the tail of a
    block back for the next one.  Counts info["blocks"] and info["blocks_inflated_on_device"]; returns the exit code, or 0."""
    if dev is not None:
        submit, collect = submit or dev.submit, collect or dev.collect
    pending = None                          # the ticket of the block on the device
    lines = 0                              # text lines handled so far (kept for cut only)
    try:
        for blk in blocks:
            eof = not len(blk)
            rest = False
            if is_span(blk):
                if eof:
                    break
                info["blocks_inflated_on_device"] += 1
                data = blk
            else:
                data = carry + blk if carry else blk
                carry = b""
                if not data:
                    break
                if universal and b"\r" in data:
                    data += b"".join(blocks)
                    rest = eof = True
                if cut is not None:
                    data, carry = cut(data, lines, eof)
                    if not data:
                        continue
            info["blocks"] += 1
            if dev is not None and not rest:
                ticket = submit(data)
                rc = finish(collect(pending)) if pending is not None else None
                pending = ticket
                if cut is not None and not is_span(data):
                    lines += count_lines(data)
            else:
                rc = finish(collect(pending)) if pending is not None else None
                pending = None
                if not rc:
                    n = count_lines(data)
                    lines += n
                    rc = host(data, n)
            if rc:
                return rc
            if eof:
                break
        return (finish(collect(pending)) if pending is not None else None) or 0
    finally:
        if hasattr(blocks, "close"):
            blocks.close()                  # (an early end: read_ahead's thread ends with it)


def count_lines(data):
    """the lines of a block of text that is not empty; the last need not end in a line feed"""
    return data.count(b"\n") + (0 if data.endswith(b"\n") else 1)


def field_at(text_at, a):
    """the field that begins at offset a of a text -- a line's scaffold name, at the line's start --: the bytes up to the first tab,
    read in growing pieces; text_at(a, k): the text's bytes [a, a + k)"""
    k = 64
    while True:
        piece = text_at(a, k)
        if b"\t" in piece:
            return piece[:piece.index(b"\t")]
        k *= 4


class SlotDevice:
    """a route over the tokenizer's two text slots: one block on the device while the next is submitted.  A block is text, or a
    genoio.BgzfSpan whose members cross PCIe deflated (k_inflate writes the text into the slot).  `route` names the library's entry
    points: pg_<route>_dev_submit, _submit_bgzf, _parse, _collect, _text, _stats ..."""

    def __init__(self, device, route):
        from .engine import Engine
        self.eng = Engine(device)
        self.L = _lib.lib()
        self.route = route
        self.slot = 0

    def fn(self, name):
        return getattr(self.L, "pg_%s_dev_%s" % (self.route, name))

    def load(self, block, *tail):
        """the block into the next slot by the route's entry point for text or for a span (`tail`: the route's own arguments behind
        the block's), its copy queued; the ticket collect takes: (slot, the text -- or (span, its bytes) --, kept alive)"""
        s = self.slot
        self.slot ^= 1
        if is_span(block):
            args, comp = span_args(block)
            _lib.check(self.fn("submit_bgzf")(self.eng._h, s, *args, *tail))
            return (s, (block, comp))
        keep = block if isinstance(block, bytes) else bytes(block)
        _lib.check(self.fn("submit")(self.eng._h, s, keep, len(keep), *tail))
        return (s, keep)

    def submit(self, block, *tail, parse_tail=()):
        """load, and the block's kernels queued (`parse_tail`: the route's own arguments of its parse)"""
        ticket = self.load(block, *tail)
        _lib.check(self.fn("parse")(self.eng._h, ticket[0], *parse_tail))
        return ticket

    def text(self, s, off, n):
        """the bytes [off, off + n) of slot s's text.  pg_ped / pg_seq / pg_s2g_dev_text take (slot, offset, length, destination);
        pg_filter / pg_gvcf / pg_eig_dev_text take (slot, destination, length) and give the text from its start"""
        text = self.fn("text")
        if len(text.argtypes) == 5:
            out = np.empty(max(n, 1), dtype=np.uint8)[:n]
            _lib.check(text(self.eng._h, s, off, n, C.c_void_p(out.ctypes.data)))
            return out.tobytes()
        assert off == 0
        return fetch(text, self.eng._h, n, s).tobytes()

    def text_at(self, ticket):
        """text_at(a, k) -- the bytes [a, a + k) -- over a ticket's text: the kept bytes, or the slot's text for a span"""
        s, keep = ticket
        if isinstance(keep, bytes):
            return lambda a, k: keep[a:a + k]
        total = len(keep[0])
        return lambda a, k: self.text(s, a, min(k, total - a))

    def host_text(self, ticket):
        """the text of a block that is the host's: the kept bytes, or the slot's text fetched back for a span"""
        s, keep = ticket
        return keep if isinstance(keep, bytes) else self.text(s, 0, len(keep[0]))

    def stats(self):
        """(blocks submitted, blocks handed back to the host)"""
        b, h = C.c_int64(), C.c_int64()
        _lib.check(self.fn("stats")(self.eng._h, C.byref(b), C.byref(h)))
        return b.value, h.value

    def pinned(self):
        return self.eng.pinned.empty

    def close(self):
        self.eng.close()
