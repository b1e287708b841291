"""What the drivers of the per-line device routes share (parseVCF: vcf.py, filterGenotypes: filtergeno.py, genoToSeq: genoseq.py,
mergeGeno: mergegeno.py): a bgzipped block's arguments for the library, the fetch of a result into host memory, the input in blocks
read ahead by a thread, and the two text slots a route alternates between (csrc/pg_line_slot.h: submit, parse, collect)."""
import ctypes as C
import queue
import threading

import numpy as np

from . import _lib


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


class SlotDevice:
    """a route over the tokenizer's two text slots: one block on the device while the next is submitted.  A block is text, or a
    genoio.BgzfSpan whose members cross PCIe deflated (k_inflate writes the text into the slot)"""

    def __init__(self, device):
        from .engine import Engine
        self.eng = Engine(device)
        self.L = _lib.lib()
        self.slot = 0

    def _submit(self, block, submit_text, submit_bgzf, parse, *tail):
        """the block into the next slot by the route's entry point for text or for a span (`tail`: the route's own arguments behind
        the block's), its kernels queued; the ticket collect takes: (slot, the text -- or (span, its bytes) --, kept alive)"""
        s = self.slot
        self.slot ^= 1
        if is_span(block):
            args, comp = span_args(block)
            _lib.check(submit_bgzf(self.eng._h, s, *args, *tail))
            keep = (block, comp)
        else:
            keep = block if isinstance(block, bytes) else bytes(block)
            _lib.check(submit_text(self.eng._h, s, keep, len(keep), *tail))
        _lib.check(parse(self.eng._h, s))
        return (s, keep)

    def pinned(self):
        return self.eng.pinned.empty

    def close(self):
        self.eng.close()
