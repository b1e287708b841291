"""Test infrastructure: DEFLATE streams (RFC 1951) written by hand, and a walker that tells what a stream is made of.

Every stream the suite gave the decoders (k_inflate, its lockstep emulation, pg_fast_inflate.h) came out of zlib, and zlib's dialect
is a small part of the format: short codes, code-length runs that stop at the end of the literal / length lengths, a window of
32 506 bytes, length 258 only as symbol 285.  Other writers (libdeflate, which today's bgzip is built on) use the rest.  The writer
here puts any legal -- or deliberately illegal -- choice on the wire; `crafted_streams()` is the corpus all tests share.

The reference for BYTES is always zlib (`zlib_accepts` / `zlib_refuses`): a stream goes to the project's decoders only after zlib
has accepted it to the last bit, or refused it.  `walk()` is a plain table-free decoder for stating FACTS about a stream (which
symbols, which code lengths, which runs in the header), not a reference for bytes.  No product code is used here."""
import random
import struct
import zlib

LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
LEN_EXTRA = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289,
             16385, 24577]
DIST_EXTRA = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]
CL_ORDER = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
FIXED_LL = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
FIXED_D = [5] * 32
MAX_TEXT = 65280                   # text of a BGZF member
MAX_STREAM = 65536 - 26            # its deflate stream


def canonical(lens):
    """code lengths -> the codes of RFC 1951 3.2.2 (as written: most significant bit first); None for an unused symbol"""
    count = [0] * 17
    for n in lens:
        count[n] += 1
    count[0] = 0
    code, nxt = 0, [0] * 17
    for n in range(1, 17):
        code = (code + count[n - 1]) << 1
        nxt[n] = code
    codes = []
    for n in lens:
        if n:
            codes.append(nxt[n])
            nxt[n] += 1
        else:
            codes.append(None)
    return codes


def kraft(lens, unit=15):
    """the sum of 2^-length over the used symbols, in units of 2^-unit (a complete code: 1 << unit)"""
    return sum(1 << (unit - n) for n in lens if n)


def complete_lengths(budget, k, unit=15):
    """k code lengths of at most `unit` bits whose Kraft sum is exactly `budget` (in units of 2^-unit), longest first"""
    parts = [unit - b for b in range(unit + 1) if (budget >> b) & 1]          # the binary digits of the budget: one code each
    assert budget > 0 and len(parts) <= k <= budget, (budget, k)
    while len(parts) < k:                                                       # split the shortest code that can still be split
        n = min(p for p in parts)
        assert n < unit
        parts.remove(n)
        parts += [n + 1, n + 1]
    return sorted(parts, reverse=True)


def _rev(v, n):
    r = 0
    for _ in range(n):
        r = (r << 1) | (v & 1)
        v >>= 1
    return r


def length_symbol(length, as_284=False):
    """(symbol - 257, extra bits' value) of a match length; as_284: 258 written as symbol 284 with extra 31 (legal, and never zlib's)"""
    if length == 258 and not as_284:
        return 28, 0
    s = max(k for k in range(28) if LEN_BASE[k] <= length)
    assert length - LEN_BASE[s] < (1 << LEN_EXTRA[s]), length
    return s, length - LEN_BASE[s]


def dist_symbol(dist):
    s = max(k for k in range(30) if DIST_BASE[k] <= dist)
    assert dist - DIST_BASE[s] < (1 << DIST_EXTRA[s]), dist
    return s, dist - DIST_BASE[s]


def expand(tokens, out):
    """the text the tokens stand for, appended to the bytearray `out` (whose content is the window); raw tokens add nothing"""
    for t in tokens:
        if isinstance(t, int):
            out.append(t)
        elif isinstance(t[0], int):
            n, d = t[0], t[1]
            assert 1 <= d <= len(out), (d, len(out))
            for _ in range(n):
                out.append(out[-d])
    return out


def rle_lengths(seq):
    """the code lengths of a dynamic header as (symbol, extra) of the code-length alphabet: zero runs as 17 / 18, repeats as 16 --
    over the WHOLE sequence (literal / length lengths and distance lengths as one), so that runs cross from one into the other"""
    ops, k, n = [], 0, len(seq)
    while k < n:
        run = 1
        while k + run < n and seq[k + run] == seq[k]:
            run += 1
        if seq[k] == 0 and run >= 3:
            r = min(run, 138)
            ops.append((17, r - 3) if r <= 10 else (18, r - 11))
            k += r
        elif seq[k] != 0 and run >= 4:
            ops.append((seq[k], 0))
            r = min(run - 1, 6)
            ops.append((16, r - 3))
            k += 1 + r
        else:
            ops.append((seq[k], 0))
            k += 1
    return ops


def code_length_code(used):
    """a complete code of at most 7 bits over the symbols in `used` (of the 19 of the code-length alphabet)"""
    used = sorted(set(used))
    if len(used) == 1:                                        # (a complete code needs two symbols)
        used.append(0 if used[0] else 1)
    lens = [0] * 19
    for s, n in zip(used, complete_lengths(1 << 7, len(used), 7)):
        lens[s] = n
    return lens


class Stream:
    """a raw DEFLATE stream under construction: bits least significant first, Huffman codes most significant first"""

    def __init__(self):
        self.buf = bytearray()
        self.acc = 0                     # the bits that do not fill a byte yet
        self.n = 0                       # bits written
        self.text = bytearray()          # what the blocks so far inflate to

    def bits(self, v, n):
        assert 0 <= v < (1 << n) or n == 0
        k = self.n & 7
        self.acc |= v << k
        self.n += n
        k += n
        while k >= 8:
            self.buf.append(self.acc & 255)
            self.acc >>= 8
            k -= 8

    def code(self, c, n):
        self.bits(_rev(c & ((1 << n) - 1), n), n)            # (masked: an over-subscribed set has codes that do not fit)

    def phase(self):
        return self.n & 7

    def bytes(self):
        return bytes(self.buf) + (bytes([self.acc]) if self.n & 7 else b"")

    # ---- blocks ----
    def stored(self, final, data, pad_bit=0, len_field=None, nlen_field=None):
        self.bits(final | (0 << 1), 3)
        while self.n & 7:
            self.bits(pad_bit, 1)
        n = len(data) if len_field is None else len_field
        self.bits(n, 16)
        self.bits((n ^ 0xFFFF) if nlen_field is None else nlen_field, 16)
        for b in data:
            self.bits(b, 8)
        self.text += data
        return self

    def _tokens(self, tokens, ll_lens, d_lens):
        """tokens: int = a literal; (length, distance[, "284"]); ("sym", s) = literal / length symbol s as it is; ("dsym", s) = a
        distance symbol as it is; ("raw", value, n) = n bits as they are.  The end-of-block code follows unless a token is ("noeob",)"""
        ll, dd = canonical(ll_lens), canonical(d_lens)
        eob = True
        for t in tokens:
            if isinstance(t, int):
                self.code(ll[t], ll_lens[t])
            elif t[0] == "sym":
                self.code(ll[t[1]], ll_lens[t[1]])
            elif t[0] == "dsym":
                self.code(dd[t[1]], d_lens[t[1]])
            elif t[0] == "raw":
                self.bits(t[1], t[2])
            elif t[0] == "noeob":
                eob = False
            else:
                ls, le = length_symbol(t[0], len(t) > 2 and t[2] == "284")
                ds, de = dist_symbol(t[1])
                self.code(ll[257 + ls], ll_lens[257 + ls])
                self.bits(le, LEN_EXTRA[ls])
                self.code(dd[ds], d_lens[ds])
                self.bits(de, DIST_EXTRA[ds])
        if eob:
            self.code(ll[256], ll_lens[256])
        expand([t for t in tokens if isinstance(t, int) or isinstance(t[0], int)], self.text)

    def fixed(self, final, tokens):
        self.bits(final | (1 << 1), 3)
        self._tokens(tokens, FIXED_LL, FIXED_D)
        return self

    def dynamic(self, final, tokens, ll_lens, d_lens, hlit=None, hdist=None, cl_lens=None, ops=None, hlit_field=None, hdist_field=None,
                body=True):
        """hlit / hdist default to the last used symbol (at least 257 / 1).  For illegal headers: cl_lens (the code-length code's
        lengths), ops (the header's (symbol, extra) list), the raw 5-bit fields, body=False (nothing behind the header)"""
        ll_lens = list(ll_lens) + [0] * (288 - len(ll_lens))
        d_lens = list(d_lens) + [0] * (32 - len(d_lens))
        if hlit is None:
            hlit = max([257] + [s + 1 for s in range(286) if ll_lens[s]])
        if hdist is None:
            hdist = max([1] + [s + 1 for s in range(30) if d_lens[s]])
        if ops is None:
            ops = rle_lengths(ll_lens[:hlit] + d_lens[:hdist])          # ONE sequence: its runs cross the boundary
        if cl_lens is None:
            cl_lens = code_length_code([s for s, _ in ops])
        cl = canonical(cl_lens)
        hclen = max([4] + [k + 1 for k in range(19) if cl_lens[CL_ORDER[k]]])
        self.bits(final | (2 << 1), 3)
        self.bits(hlit - 257 if hlit_field is None else hlit_field, 5)
        self.bits(hdist - 1 if hdist_field is None else hdist_field, 5)
        self.bits(hclen - 4, 4)
        for k in range(hclen):
            self.bits(cl_lens[CL_ORDER[k]], 3)
        for s, extra in ops:
            self.code(cl[s], cl_lens[s])
            if s >= 16:
                self.bits(extra, (2, 3, 7)[s - 16])
        if body:
            self._tokens(tokens, ll_lens, d_lens)
        return self


def wrap_member(raw, text):
    """a BGZF member around a raw stream"""
    total = 18 + len(raw) + 8
    assert total <= 65536, total
    return (b"\x1f\x8b\x08\x04\0\0\0\0\0\xff\x06\x00BC\x02\x00" + struct.pack("<H", total - 1) + raw +
            struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text)))


def wrap_gzip(raw, text):
    """a gzip file of one member around a raw stream"""
    return b"\x1f\x8b\x08\x00\0\0\0\0\0\xff" + raw + struct.pack("<II", zlib.crc32(text) & 0xFFFFFFFF, len(text))


# ---- zlib, the reference for bytes ----
def zlib_accepts(raw):
    """the text, after asserting that zlib takes the stream to its last byte and sees its end"""
    d = zlib.decompressobj(-15)
    text = d.decompress(raw)
    assert d.eof and d.unused_data == b"" and d.unconsumed_tail == b""
    return text


def zlib_refuses(raw, truncated=False):
    """asserts that zlib refuses the stream: zlib.error while it decodes, or -- a stream that merely ends too early is no error to a
    decompressobj, which waits for more -- no end of stream, and zlib.error from the one-shot call"""
    d = zlib.decompressobj(-15)
    if truncated:
        d.decompress(raw)
        assert not d.eof
    else:
        try:
            d.decompress(raw)
        except zlib.error:
            pass
        else:
            raise AssertionError("zlib accepted a stream that was meant to be illegal")
    try:
        zlib.decompress(raw, wbits=-15)
    except zlib.error:
        return
    raise AssertionError("zlib accepted a stream that was meant to be illegal")


# ---- the walker ----
class _Bits:
    def __init__(self, raw):
        self.raw = raw
        self.at = 0
        self.end = len(raw) * 8

    def take(self, n):
        if self.at + n > self.end:
            raise ValueError("the stream ends inside a block")
        r = (int.from_bytes(self.raw[self.at >> 3:(self.at >> 3) + 4], "little") >> (self.at & 7)) & ((1 << n) - 1)
        self.at += n
        return r

    def symbol(self, table):
        code = n = 0
        while n < 15:
            code = (code << 1) | self.take(1)
            n += 1
            s = table.get((n, code))
            if s is not None:
                return s
        raise ValueError("no code")


def _table(lens):
    return {(n, c): s for s, (n, c) in enumerate(zip(lens, canonical(lens))) if n}


def walk(raw):
    """per block: {"type": "stored" | "fixed" | "dynamic", "final", "ll_lens", "d_lens", "cl_lens", "hlit", "hdist", "ops" (the
    header's code-length symbols as (symbol, first position, positions covered)), "tokens" (literals as ints, matches as (length,
    distance, length symbol, distance symbol)), "data" (stored)}"""
    b, blocks = _Bits(raw), []
    while True:
        final, kind = b.take(1), b.take(2)
        blk = {"final": final, "type": ("stored", "fixed", "dynamic")[kind], "ll_lens": None, "d_lens": None, "cl_lens": None, "ops": [],
               "tokens": [], "data": b""}
        blocks.append(blk)
        if kind == 0:
            blk["pad"] = b.take(-b.at % 8)
            n, nn = b.take(16), b.take(16)
            if n ^ 0xFFFF != nn:
                raise ValueError("stored block: LEN / NLEN")
            blk["data"] = bytes(b.take(8) for _ in range(n))
        else:
            if kind == 1:
                ll_lens, d_lens = FIXED_LL, FIXED_D
            else:
                hlit, hdist, hclen = b.take(5) + 257, b.take(5) + 1, b.take(4) + 4
                cl_lens = [0] * 19
                for k in range(hclen):
                    cl_lens[CL_ORDER[k]] = b.take(3)
                cl, seq = _table(cl_lens), []
                while len(seq) < hlit + hdist:
                    s = b.symbol(cl)
                    at = len(seq)
                    if s < 16:
                        seq.append(s)
                    elif s == 16:
                        seq += [seq[-1]] * (3 + b.take(2))
                    elif s == 17:
                        seq += [0] * (3 + b.take(3))
                    else:
                        seq += [0] * (11 + b.take(7))
                    blk["ops"].append((s, at, len(seq) - at))
                if len(seq) != hlit + hdist:
                    raise ValueError("a run past the code lengths")
                ll_lens, d_lens = seq[:hlit], seq[hlit:]
                blk.update(cl_lens=cl_lens, hlit=hlit, hdist=hdist)
            blk.update(ll_lens=list(ll_lens), d_lens=list(d_lens))
            ll, dd = _table(ll_lens), _table(d_lens)
            toks = blk["tokens"]
            while True:
                s = b.symbol(ll)
                if s < 256:
                    toks.append(s)
                elif s == 256:
                    break
                else:
                    n = LEN_BASE[s - 257] + b.take(LEN_EXTRA[s - 257])
                    ds = b.symbol(dd)
                    toks.append((n, DIST_BASE[ds] + b.take(DIST_EXTRA[ds]), s, ds))
        if final:
            return blocks


def walked_text(blocks):
    out = bytearray()
    for blk in blocks:
        out += blk["data"]
        expand([t if isinstance(t, int) else t[:2] for t in blk["tokens"]], out)
    return bytes(out)


# ---- the corpus ----
def _lit(rng, n, alphabet=None, lf=0.02):
    """n random literals; some of them line feeds (the decoder lists those)"""
    alphabet = alphabet or range(256)
    return [10 if (10 in alphabet and rng.random() < lf) else rng.choice(alphabet) for _ in range(n)]


def _place(n, lens_for):
    """a list of n code lengths from {symbol: length}"""
    out = [0] * n
    for s, v in lens_for.items():
        out[s] = v
    return out


LL_ALL = [8] * 226 + [9] * 60                                  # all 286 symbols: 226 / 256 + 60 / 512 = 1


def _all_symbols(rng):
    """group b: every length and every distance symbol, extra bits all zero and all ones, under a distance code of up to 15 bits"""
    ll = list(LL_ALL)
    rng.shuffle(ll)
    dl = list(range(1, 11)) + [14] * 12 + [15] * 8
    rng.shuffle(dl)
    matches = []
    for ds in range(30):
        for de in (0, (1 << DIST_EXTRA[ds]) - 1):
            for ls in range(29):
                for le in (0, (1 << LEN_EXTRA[ls]) - 1):
                    n = LEN_BASE[ls] + le
                    matches.append((n, DIST_BASE[ds] + de) if n < 258 or ls == 28 else (258, DIST_BASE[ds] + de, "284"))
    matches += [(258, 32768), (258, 32768, "284"), (3, 32768), (258, 24577)]
    rng.shuffle(matches)
    out, k = [], 0
    while k < len(matches):
        toks = _lit(rng, 33000)
        size = len(toks)
        while k < len(matches) and size + matches[k][0] <= MAX_TEXT:
            toks.append(matches[k])
            size += matches[k][0]
            k += 1
            if k % 7 == 0:                                     # a literal now and then, so that the matches do not only copy matches
                toks.append(rng.randrange(256))
                size += 1
        out.append(("b%d_every_length_and_distance_symbol" % len(out), Stream().dynamic(1, toks, ll, dl)))
    return out


def _boundary_runs(rng):
    """group c: a symbol-16 run, and a symbol-18 run, that start in the literal / length lengths and end in the distance lengths.
    What the format allows: a 16 run repeats a literal / length length as distance lengths, so with hdist = 1 it would need three
    literal / length codes of one bit (over-subscribed); an 18 run over position 256 would leave no end-of-block code, so hlit = 257
    cannot have one.  Hence: 16 runs for hlit 257 and 286 with hdist 30, 18 runs for hlit 286 with hdist 30 and 1 (there it ends with
    the only distance length), and for hlit 257 with hdist 1 a 16 run that ends AT the boundary."""
    out = []
    for hlit, hdist, kind in ((257, 30, 16), (286, 30, 16), (286, 30, 18), (286, 1, 18), (257, 1, 16)):
        if kind == 16 and hdist == 30:
            if hlit == 257:
                ll, v = [9] + [8] * 252 + [9] + [8] * 3, 8     # 255 eights, two nines; eights at 254 .. 256, a nine in front
            else:
                ll, v = [9] * 57 + [8] * 226 + [9] * 3, 9      # 226 eights, 60 nines; nines at 283 .. 285, an eight in front
            # length hlit - 3 is written as itself, the six repeats of ONE symbol 16 cover hlit - 2 .. hlit + 3
            dl = [v] * 4 + complete_lengths((1 << 15) - 4 * (1 << (15 - v)), 26)
            span = (hlit - 2, hlit + 3)
        elif kind == 18 and hdist == 30:
            ll = complete_lengths(1 << 15, 272)[::-1] + [0] * 14                   # symbols 272 .. 285 unused
            dl = [0] * 4 + complete_lengths(1 << 15, 26)
            span = (hlit - 2, hlit + 3)
        elif kind == 18:
            ll = complete_lengths(1 << 15, 270)[::-1] + [0] * 16
            dl = [0]                                                                # no distance code: literals only
            span = (hlit - 2, hlit)
        else:
            ll = [9] + [8] * 248 + [9] + [8] * 7                                    # eights at 250 .. 256: one as itself, six repeats
            dl = [0]
            span = (hlit - 6, hlit - 1)
        assert kraft(ll) == 1 << 15 and (kraft(dl) in (0, 1 << 15)), (hlit, hdist, kind)
        toks = _lit(rng, 400)
        lsyms = [s for s in range(29) if hlit > 257 + s and ll[257 + s]]
        dsyms = [s for s in range(len(dl)) if dl[s] and DIST_BASE[s] <= 400]
        if lsyms and dsyms:
            for _ in range(60):
                toks.append((LEN_BASE[rng.choice(lsyms)], DIST_BASE[rng.choice(dsyms)]))
                toks += _lit(rng, 3)
        out.append(("c_run_of_%d_hlit_%d_hdist_%d" % (kind, hlit, hdist), Stream().dynamic(1, toks, ll, dl, hlit=hlit, hdist=hdist), (kind, span)))
    return out


def _ring_sweep(rng):
    """group e: near and far sources right behind the overshoot of a 258-byte match and across flushes of the decoder's 4 KiB ring.
    k_inflate copies a match in steps of 64 lanes, so a 258-byte match writes 320 ring slots: the 62 behind its end hold what was
    4096 .. 4035 bytes in front of the new position.  It reads sources up to 3776 bytes back from the ring (3770 .. 3781: both sides
    of that switch) and the rest from the text it has flushed; 4030 .. 4040 are the distances at which a ring read WOULD see the
    overshoot (a switch at 4035 or beyond fails here), 4095 .. 4097 the ring's size."""
    out = []
    for dist in list(range(3770, 3782)) + list(range(4030, 4041)) + [4095, 4096, 4097]:
        toks = _lit(rng, 6000)
        for n in (258, 258, 3, 64, 65, 128, 129, 192, 193, 256, 257, 258):
            toks.append((258, rng.randrange(1, 300)))
            toks.append((n, dist))
        out.append(("e_ring_distance_%d" % dist, Stream().fixed(1, toks)))
    return out


def _block_mix(phase):
    """group f: the block types one after the other; the first stored block's header starts at bit `phase` of its byte, which the
    number of nine-bit literals in the first block sets; pad bits of one"""
    ll2 = _place(286, {**{c: 7 for c in range(64, 190)}, 256: 7, 277: 8, 285: 8})                # 127 / 128 + 2 / 256
    for k in range(8):
        rng = random.Random(6000 + phase)
        s = Stream()
        s.fixed(0, _lit(rng, 40) + [200] * k)
        s.fixed(0, [66, 67, (4, 2)])
        s.dynamic(0, [65] * 3 + [(258, 1), 66] + _lit(rng, 70, range(64, 190)) + [(70, 65)], ll2, [1] + [0] * 11 + [1])    # both overlap themselves
        s.fixed(0, [(30, 200), 10, (5, 1)])                                                     # reaches into the block before
        if s.phase() == phase:
            break
    else:
        raise AssertionError("no phase %d" % phase)
    s.stored(0, b"", 1)
    s.stored(0, bytes(_lit(rng, 3000 + phase)), 1)
    s.stored(0, b"")
    s.fixed(0, [(258, 3000), (200, 2999 + phase)])                                            # only matches, into the stored bytes
    s.dynamic(0, _lit(rng, 500, range(60, 99)), _place(257, dict(zip(list(range(60, 99)) + [256], complete_lengths(1 << 15, 40)))), [0])
    s.stored(1, b"")
    return s


def crafted_streams():
    """-> (legal, illegal).  legal: {"name", "group", "raw", "text", ...}; illegal: {"name", "raw", "out_len", "truncated"}.
    Deterministic; every text at most 65 280 bytes, every stream at most 65 536 - 26."""
    rng = random.Random(1951)
    legal = []

    def add(group, name, s, **more):
        legal.append(dict(name=name, group=group, raw=s.bytes(), text=bytes(s.text), **more))

    # a. a literal / length code of lengths 1, 2 ... 14, 15, 15 over 15 literals and the end-of-block code (15 bits); no distance code
    syms = [10, 9] + list(range(65, 78))
    rng.shuffle(syms)
    ll = _place(257, dict(zip(syms, range(1, 16))))
    ll[256] = 15
    toks = [s for s in syms for _ in range(20)] + [rng.choice(syms[:6]) for _ in range(4700)]
    rng.shuffle(toks)
    add("a", "a_codes_of_1_to_15_bits", Stream().dynamic(1, toks, ll, [0], hdist=1))
    # b
    for name, s in _all_symbols(rng):
        add("b", name, s)
    # c
    for name, s, run in _boundary_runs(rng):
        add("c", name, s, run=run)
    # d. distance-code edge cases
    ll = _place(286, {**{c: 7 for c in range(32, 32 + 124)}, 10: 7, 256: 7, 285: 7, 257: 7})       # 128 codes of 7 bits
    add("d", "d_one_bit_distance_code_on_symbol_29", Stream().dynamic(1, _lit(rng, 24600, list(range(32, 156)) + [10]) + [(258, 24582), 65, (3, 24577)],
                                                                      ll, [0] * 29 + [1]))
    add("d", "d_one_bit_distance_code_on_symbol_0", Stream().dynamic(1, _lit(rng, 50, list(range(32, 156)) + [10]) + [(258, 1), 65, (3, 1)], ll, [1]))
    add("d", "d_only_the_end_of_block_code", Stream().dynamic(1, [], _place(257, {256: 1}), [0]))
    # e
    for name, s in _ring_sweep(rng):
        add("e", name, s)
    # f
    for phase in range(8):
        add("f", "f_block_mix_phase_%d" % phase, _block_mix(phase))
    # g. 300 blocks of 1 .. 40 bytes: stored, fixed, dynamic in turn
    s = Stream()
    ll = _place(257, dict(zip(list(range(65, 65 + 31)) + [256], [5] * 32)))
    for k in range(300):
        n = rng.randrange(1, 41)
        final = int(k == 299)
        if k % 3 == 0:
            s.stored(final, bytes(_lit(rng, n)), k & 1)
        elif k % 3 == 1:
            s.fixed(final, _lit(rng, n))
        else:
            s.dynamic(final, _lit(rng, n, range(65, 96), 0), ll, [0])
    add("g", "g_300_short_blocks", s)
    # h. the distance equals the position
    add("h", "h_distance_equals_position", Stream().fixed(1, [65, (3, 1)]))

    illegal = []

    def bad(name, s, out_len=8, truncated=False, raw=None):
        illegal.append(dict(name=name, raw=s.bytes() if raw is None else raw, out_len=out_len, truncated=truncated))

    ok_ll, ok_d = _place(257, {65: 1, 256: 1}), [0]
    bad("oversubscribed_literal_length_code", Stream().dynamic(1, [65] * 8, _place(257, {65: 1, 66: 1, 256: 1}), [0]))
    bad("oversubscribed_distance_code", Stream().dynamic(1, [65] * 8, ok_ll, [1, 1, 1]))
    bad("oversubscribed_code_length_code", Stream().dynamic(1, [65] * 8, ok_ll, ok_d, cl_lens=_place(19, {0: 1, 1: 1, 18: 1, 17: 2})))
    bad("incomplete_literal_length_code", Stream().dynamic(1, [65] * 8, _place(257, {65: 2, 66: 2, 256: 2}), [0]))
    bad("incomplete_distance_code_of_two_symbols", Stream().dynamic(1, [65] * 8, ok_ll, [2, 2]))
    bad("code_length_code_with_a_single_symbol", Stream().dynamic(1, [], [1] * 257, [1], cl_lens=_place(19, {1: 1}), ops=[(1, 0)] * 258, body=False))
    bad("symbol_16_as_the_first_length", Stream().dynamic(1, [], ok_ll, ok_d, cl_lens=_place(19, {16: 2, 0: 2, 1: 2, 18: 2}),
                                                           ops=[(16, 3), (18, 127), (18, 90), (1, 0), (0, 0)], body=False))
    bad("a_run_past_the_code_lengths", Stream().dynamic(1, [], ok_ll, ok_d, cl_lens=_place(19, {0: 2, 1: 2, 18: 1}),
                                                         ops=[(18, 54), (1, 0), (18, 127), (18, 41), (1, 0), (18, 0)], body=False))
    ll286 = LL_ALL
    bad("hlit_287", Stream().dynamic(1, [65] * 8, ll286 + [0], [1], hlit=287, hlit_field=30, ops=rle_lengths(ll286 + [0, 1])))
    bad("hdist_31", Stream().dynamic(1, [65] * 8, ok_ll, [5] * 31 + [0], hdist=31, hdist_field=30, ops=rle_lengths(ok_ll + [5] * 31)))
    bad("no_code_for_the_end_of_block", Stream().dynamic(1, [65] * 8 + [("noeob",)], _place(257, {65: 1, 66: 1}), [0]))
    bad("unassigned_pattern_of_a_one_bit_distance_code", Stream().dynamic(1, [65] * 5 + [("sym", 257), ("raw", 1, 1)] + [65] * 3,
                                                                          _place(258, {65: 2, 256: 2, 257: 1}), [1]), out_len=11)
    bad("fixed_block_with_length_symbol_286", Stream().fixed(1, [65] * 5 + [("sym", 286), ("raw", 0, 5)] + [65] * 3), out_len=11)
    bad("fixed_block_with_distance_symbol_30", Stream().fixed(1, [65] * 5 + [("sym", 257), ("dsym", 30)] + [65] * 3), out_len=11)
    far = Stream()
    far.bits(1 | (1 << 1), 3)
    far._tokens([65, ("sym", 257), ("dsym", 1)], FIXED_LL, FIXED_D)
    bad("distance_greater_than_the_position", far, out_len=4)
    bad("stored_block_with_nlen_off_by_one", Stream().stored(1, b"ABCDEFGH", 0, nlen_field=(8 ^ 0xFFFF) ^ 1))
    bad("stored_len_past_the_member", Stream().stored(1, b"ABCDEFGH", 0, len_field=100), out_len=100, truncated=True)
    for m in legal:
        assert len(m["text"]) <= MAX_TEXT and len(m["raw"]) <= MAX_STREAM, (m["name"], len(m["text"]), len(m["raw"]))
    return legal, illegal


_checked = None


def checked_streams():
    """crafted_streams() after zlib has spoken: every legal stream accepted to its last bit with the text the writer meant, every
    illegal one refused.  Made once per process and shared; nobody changes it."""
    global _checked
    if _checked is None:
        legal, illegal = crafted_streams()
        for m in legal:
            assert zlib_accepts(m["raw"]) == m["text"], m["name"]
        for m in illegal:
            zlib_refuses(m["raw"], m["truncated"])
        _checked = (legal, illegal)
    return _checked


ILLEGAL_NAMES = ["oversubscribed_literal_length_code", "oversubscribed_distance_code", "oversubscribed_code_length_code",
                 "incomplete_literal_length_code", "incomplete_distance_code_of_two_symbols", "code_length_code_with_a_single_symbol",
                 "symbol_16_as_the_first_length", "a_run_past_the_code_lengths", "hlit_287", "hdist_31", "no_code_for_the_end_of_block",
                 "unassigned_pattern_of_a_one_bit_distance_code", "fixed_block_with_length_symbol_286", "fixed_block_with_distance_symbol_30",
                 "distance_greater_than_the_position", "stored_block_with_nlen_off_by_one", "stored_len_past_the_member"]


# ---- texts for the COMPRESSORS: frequencies that make an unrestricted Huffman code deeper than the format allows ----
def huffman_depth(freqs):
    """the length of the longest code of an unrestricted Huffman code over the non-zero frequencies (heapq; ties: the shallower tree
    first, so the depth is the smallest any Huffman tree of these frequencies has)"""
    import heapq
    heap = [(f, 0) for f in freqs if f]
    if len(heap) < 2:
        return len(heap)
    heapq.heapify(heap)
    while len(heap) > 1:
        a, b = heapq.heappop(heap), heapq.heappop(heap)
        heapq.heappush(heap, (a[0] + b[0], max(a[1], b[1]) + 1))
    return heap[0][1]


def _without_repeated_4_grams(counts, rng):
    """the symbols of {symbol: count} in an order in which no four bytes in a row occur twice: a match finder whose shortest match
    is four bytes finds nothing, so the tokens of the text are its bytes and their frequencies are `counts` exactly"""
    pool = [s for s, c in counts.items() for _ in range(c)]
    rng.shuffle(pool)
    out, seen = bytearray(), set()
    while pool:
        for _ in range(400):
            gram = bytes(out[-3:]) + bytes([pool[-1]])
            if len(gram) < 4 or gram not in seen:
                break
            k = rng.randrange(len(pool))
            pool[k], pool[-1] = pool[-1], pool[k]
        else:
            raise AssertionError("no order without a repeated 4-gram")
        if len(gram) == 4:
            seen.add(gram)
        out.append(pool.pop())
    return bytes(out)


SKEWED_NAMES = ["fibonacci_22_symbols", "fibonacci_24_symbols", "fibonacci_tail_without_matches", "code_length_fibonacci"]
_skewed = None


def skewed_texts():
    """the texts of _make_skewed_texts(), made once per process"""
    global _skewed
    if _skewed is None:
        _skewed = _make_skewed_texts()
        assert [t[0] for t in _skewed] == SKEWED_NAMES
    return _skewed


def _make_skewed_texts():
    """-> [(name, kind, text)]; kind "ll": the literal / length code needs limiting to 15 bits, "cl": the code-length code to 7.
      * fibonacci_22_symbols (65 280 bytes), fibonacci_24_symbols (200 000 bytes): byte frequencies in Fibonacci proportion, shuffled.
        A match finder absorbs most of such a text, so what frequencies the TOKENS have is up to it;
      * fibonacci_tail_without_matches (65 280 bytes): fifteen bytes with frequencies 1, 2, 3, 5 ... 987 (with the end-of-block
        code's 1: a Fibonacci chain of sixteen, sum 2583) and 24 bytes with 2612 or 2613 each, ordered without a repeated 4-gram: no
        matches, the sixteen form a subtree 15 deep that has to be merged at least once more, whatever the ties: a depth of 20;
      * code_length_fibonacci (16 383 bytes): 140 bytes with frequencies 2^(14 - L), L being 6, 7, 9 ... 14 for 34, 55, 5, 21, 13, 8, 3
        and 2 (the end-of-block code among them) symbols -- a dyadic distribution, so those ARE the code lengths --, ordered without a
        repeated 4-gram and without four equal lengths in a row: the header's symbols have frequencies 1, 1, 2, 3, 5, 8, 13, 21, 34,
        55 (one run of zeros, the one distance length, eight lengths): a code-length code 9 deep."""
    rng = random.Random(1952)
    fib = [1, 1]
    while len(fib) < 24:
        fib.append(fib[-1] + fib[-2])
    out = []
    for n_sym, size in ((22, 65280), (24, 200000)):
        syms = rng.sample(range(256), n_sym)
        counts = [max(1, f * size // sum(fib[:n_sym])) for f in fib[:n_sym]]
        counts[-1] += size - sum(counts)
        text = [s for s, c in zip(syms, counts) for _ in range(c)]
        rng.shuffle(text)
        out.append(("fibonacci_%d_symbols" % n_sym, "ll", bytes(text)))
    syms = rng.sample(range(256), 39)
    counts = dict(zip(syms[:15], fib[1:16]))
    rest = 65280 - sum(fib[1:16])
    for k, s in enumerate(syms[15:]):
        counts[s] = rest // 24 + (1 if k < rest % 24 else 0)
    assert huffman_depth(list(counts.values()) + [1]) == 20
    out.append(("fibonacci_tail_without_matches", "ll", _without_repeated_4_grams(counts, rng)))
    n_of = {6: 34, 7: 55, 9: 5, 10: 21, 11: 13, 12: 8, 13: 3, 14: 2}
    assert sum(n << (15 - L) for L, n in n_of.items()) == 1 << 15
    lens = [L for L, n in n_of.items() for _ in range(n - (L == 14))]           # (one of the two 14s is the end-of-block code's)
    while True:
        rng.shuffle(lens)
        if all(len(set(lens[k:k + 4])) > 1 for k in range(len(lens) - 3)):
            break
    out.append(("code_length_fibonacci", "cl", _without_repeated_4_grams({s: 1 << (14 - L) for s, L in enumerate(lens)}, rng)))
    return out


def dynamic_block_facts(raw):
    """what a compressor made of a member: asserts a single dynamic block whose codes respect the format's limits (15 bits; 7 for
    the code-length code) and are complete (Kraft sum exactly 1; a distance code that no match uses is one unused code of one bit);
    -> the unrestricted Huffman depths of the frequencies it coded: {"ll", "d", "cl"}, and the longest lengths it emitted"""
    blocks = walk(raw)
    assert len(blocks) == 1 and blocks[0]["type"] == "dynamic", [b["type"] for b in blocks]
    b = blocks[0]
    f_ll, f_d, f_cl = [0] * 286, [0] * 30, [0] * 19
    f_ll[256] = 1
    for t in b["tokens"]:
        if isinstance(t, int):
            f_ll[t] += 1
        else:
            f_ll[t[2]] += 1
            f_d[t[3]] += 1
    for s, _, _ in b["ops"]:
        f_cl[s] += 1
    assert max(b["ll_lens"]) <= 15 and max(b["d_lens"]) <= 15 and max(b["cl_lens"]) <= 7
    assert kraft(b["ll_lens"]) == 1 << 15, "the literal / length code is not complete"
    assert kraft(b["d_lens"]) == 1 << 15 or (sum(f_d) == 0 and [n for n in b["d_lens"] if n] == [1]), "the distance code is not complete"
    assert kraft(b["cl_lens"], 7) == 1 << 7, "the code-length code is not complete"
    # (every symbol that occurs has a code: the walk would have failed otherwise, and zlib has inflated the member before)
    return {"ll": huffman_depth(f_ll), "d": huffman_depth(f_d), "cl": huffman_depth(f_cl),
            "max_ll": max(b["ll_lens"]), "max_d": max(b["d_lens"]), "max_cl": max(b["cl_lens"]), "matches": sum(f_d)}
