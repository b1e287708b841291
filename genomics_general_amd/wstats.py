"""Drop-in for the reference's windowStats.py: a table of per-site numbers (scaffold, position, then numeric columns) summarised per
window and column -- mean, median, min, max, sd, sum and quantiles over the non-nan values, as NumPy 2.2 computes them, to the last bit.

The input goes through the device a block of whole lines at a time (devroute.SlotDevice over pg_ws_dev_*: a text slot of
csrc/pg_line_slot.h; bgzip members cross PCIe deflated and k_inflate writes their text into the slot).  k_ws_lines takes a wavefront per
line: '#' lines marked, the fields cut at whitespace runs by ballots, lanes strided over the selected columns converting decimal text to
float64 with pg_ws_core.h's cell rule, the position read, a scaffold change noted; a scan places the sites, and the values land in the
value store [column][site], resident on the device.  A block with a line outside the regular spelling (another field count than the
header's, a cell or position of another spelling, a carriage return, text that is not ASCII) is handed back, parsed by host threads
(pg_ws_text; such cells through float(), which is what NumPy's cast of a string does) and its doubles uploaded to the same place.
k_ws_stats then computes every window's statistics over the store (a workgroup per window and column, a sort in LDS up to
PG_WS_LDS_VALS values, a radix select over global memory beyond).  Positions, scaffold runs, the statistics, the counts and the flags
come back; the windows (windows.py, the reference's own generators), `mid`, round(sd, 6) and the text are the host's.
PG_WS_DEVICE=0 parses and computes on host threads (pg_ws_text, pg_ws_stats_host) and needs no GPU.

Where the reference dies with a traceback this driver stops with one message: with exit status 2 before any output (the assertions of
windowStats.py:56-79, `--windType predefined -m 0`, a --columns name the header lacks, a header without value columns, text that is
not ASCII, a position of more than 18 digits, selected columns beyond PG_SCRATCH_GIB), with exit status 1 behind the rows that were
whole (a cell NumPy does not convert or min / max of a column without a value, in the first window in output order that has enough
sites; a position int() does not take or a line with too few -- without --columns: not exactly the header's -- fields, where the line
is read).  --include / --exclude, -o and gzipped input, which are Python-2 lines in the reference, work.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib, devroute, dist, genoio, windows

STATS = ("mean", "median", "min", "max", "sd", "sum", "q5", "q10", "q25", "q75", "q90", "q95")     # PG_WS_MEAN ... (pg_ws_core.h)
SD = STATS.index("sd")
LDS_DEFAULT = 8192                                     # PG_WS_LDS_DEFAULT

ENGINE_EPILOG = ("MI355X engine: blocks of the regular spelling are parsed on the device (k_ws_lines), every other block on host threads; the "
                 "selected columns of the whole file are held on the device and every window's statistics are computed there "
                 "(k_ws_stats); windows, mid, round(sd, 6) and the text are the host's.  "
                 "Under WORLD_SIZE > 1 rank 0 does the whole job.  Environment: PG_WS_DEVICE=0 host threads only (no GPU needed); "
                 "PG_WS_LDS_VALS values of a window and column sorted in LDS (default and most 8192; more go through a radix select); "
                 "PG_SCRATCH_GIB the budget the selected columns must fit (default 48); PG_STREAM_BYTES text bytes per block (default "
                 "256 MiB); PG_BGZF_DEVICE=0 bgzip members inflated by host threads; PG_HOST_THREADS host threads; PG_TIMING=1 counters "
                 "and times on stderr.")

last_info = {}


class Usage(devroute.Usage):
    prog = "windowStats.py"


class Stop(devroute.Stop):
    prog = "windowStats.py"


def make_parser():
    ap = argparse.ArgumentParser(prog="windowStats.py", epilog=ENGINE_EPILOG)
    ap.add_argument("--windType", help="Type of windows to make", action="store", choices=("sites", "coordinate", "predefined"),
                    default="coordinate")
    ap.add_argument("-w", "--windSize", help="Window size in bases", type=int, action="store", required=False, metavar="sites")
    ap.add_argument("-s", "--stepSize", help="Step size for sliding window", type=int, action="store", required=False, metavar="sites")
    ap.add_argument("-m", "--minSites", help="Minumum good sites per window", type=int, action="store", required=False, metavar="sites",
                    default=1)
    ap.add_argument("-O", "--overlap", help="Overlap for sites sliding window", type=int, action="store", required=False, metavar="sites")
    ap.add_argument("-D", "--maxDist", help="Maximum span distance for sites window", type=int, action="store", required=False)
    ap.add_argument("--windCoords", help="Window coordinates file (scaffold start end)", required=False)
    ap.add_argument("--stats", help="Which statistics to compute", action="store", nargs="+", choices=STATS,
                    default=("mean", "median", "min", "max", "sd", "sum"))
    ap.add_argument("-i", "--inFile", help="Input genotypes file", required=False)
    ap.add_argument("-o", "--outFile", help="Results file", required=False)
    ap.add_argument("--headers", help="Headers text (separated by spaces) if no header in input", nargs="+", action="store")
    ap.add_argument("--columns", help="Columns to analyse, separated by spaces", required=False, nargs="+")
    ap.add_argument("--exclude", help="File of scaffolds to exclude", required=False)
    ap.add_argument("--include", help="File of scaffolds to analyse", required=False)
    ap.add_argument("--verbose", help="Verbose output", action="store_true")
    ap.add_argument("--writeFailedWindows", help="Write output even for windows with too few sites.", action="store_true")
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


_vp = devroute.vp


def _window_params(args):
    """windowStats.py:56-82: the assertions, as one message each"""
    wt = args.windType
    if wt == "coordinate":
        if not args.windSize:
            raise Usage("Window size must be provided.")
        if args.overlap:
            raise Usage("Overlap does not apply to coordinate windows. Use --stepSize instead.")
        if args.maxDist:
            raise Usage("Maximum distance only applies to sites windows.")
    elif wt == "sites":
        if not args.windSize:
            raise Usage("Window size (number of sites) must be provided.")
        if args.stepSize:
            raise Usage("Step size only applies to coordinate windows. Use --overlap instead.")
    else:
        if not args.windCoords:
            raise Usage("Please provide a file of window coordinates.")
        if args.overlap:
            raise Usage("Overlap does not apply for predefined windows.")
        if args.maxDist:
            raise Usage("Maximum does not apply for predefined windows.")
        if args.stepSize:
            raise Usage("Step size does not apply for predefined windows.")
        if args.include:
            raise Usage("You cannot only include specific scaffolds if using predefined windows.")
        if args.exclude:
            raise Usage("You cannot exclude specific scaffolds if using predefined windows.")
        if not args.minSites:
            raise Usage("--windType predefined -m 0: there is no window size to stand in for it (the reference raises NameError)")
    return args.minSites if args.minSites else args.windSize


def _read_coords(path):
    """windowStats.py:79: (scaffold, int(start), int(end)) of every line's first three fields"""
    coords = []
    with open(path, "rt") as wc:
        for k, line in enumerate(wc):
            f = line.split()[:3]
            try:
                if len(f) != 3:
                    raise ValueError
                coords.append((f[0], int(f[1]), int(f[2])))
            except ValueError:
                raise Usage("%s line %d: a scaffold and two integers are needed (the reference raises ValueError)" % (path, k + 1))
    return coords


def _scaf_list(path):
    with open(path, "rt") as f:
        return [line.rstrip() for line in f.readlines()]


class Table:
    """the parsed input: the selected columns [column][site], positions, scaffold runs, the cells NumPy does not convert, and where
    and why the reading stopped"""

    def __init__(self, n_sel):
        self.n_sel = n_sel
        self.vals, self.pos = [], []
        self.run_starts, self.run_names = [], []
        self.bad = {}                                      # site -> (selected column, the cell's text): the first bad cell of the site
        self.n_sites = 0
        self.stop = None                                   # (exit status, message)
        self.lines = 1                                     # lines of the file in front of the block in hand
        self.host_cells = 0


def parse_block(tab, text, sel_col, n_names, exact, shown, n_threads=0, dev=None):
    """pg_ws_text over a block of whole lines; the irregular cells through float(), the irregular positions through int().  dev: the
    block's doubles are uploaded behind the store's sites instead of kept"""
    L = _lib.lib()
    buf = np.frombuffer(text, dtype=np.uint8)
    n_sel = len(sel_col)
    cap = text.count(b"\n") + 1
    cap_irr = 1024
    while True:
        vals = np.empty((n_sel, cap), dtype=np.float64)
        pos = np.empty(cap, dtype=np.int64)
        soff, slen, new_run = np.empty(cap, dtype=np.int64), np.empty(cap, dtype=np.int32), np.empty(cap, dtype=np.uint8)
        irr = np.empty((cap_irr, 4), dtype=np.int64)
        ns, ni, nl, el, es, ec = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        rc = L.pg_ws_text(C.c_void_p(buf.ctypes.data if len(buf) else 0), len(buf), n_sel, _vp(sel_col), n_names, int(exact),
                          devroute.host_threads(n_threads), cap, _vp(vals), cap, _vp(pos), _vp(soff), _vp(slen), _vp(new_run), cap_irr,
                          _vp(irr), C.byref(ns), C.byref(ni), C.byref(nl), C.byref(ec), C.byref(el), C.byref(es))
        if rc != 0:
            raise RuntimeError("pg_ws_text: bad arguments")
        if ni.value <= cap_irr:
            break
        cap_irr = ni.value
    n = ns.value
    site0 = tab.n_sites
    stop = None
    for s, k, off, ln in irr[:ni.value].tolist():
        cell = text[off:off + ln].decode("ascii")
        if stop is not None and s >= stop[0]:
            continue
        if k < 0:
            try:
                digits = cell.strip().lstrip("+-").replace("_", "")
                value = int(cell)
                if len(digits.lstrip("0")) > 18:
                    stop = (s, 2, "a position of more than 18 digits is not supported")
                    continue
                pos[s] = value
            except ValueError:
                stop = (s, 1, "the position %r is not an integer (the reference raises ValueError)" % cell)
        else:
            tab.host_cells += 1
            try:
                vals[k, s] = float(cell)
            except ValueError:
                tab.bad.setdefault(site0 + s, (k, cell))
    err_line = el.value
    if stop is not None:
        # the line of site stop[0]: count the lines that are sites
        n = stop[0]
        at, line = 0, 0
        seen = -1
        while True:
            if text[at:at + 1] != b"#":
                seen += 1
                if seen == n:
                    break
            at = text.index(b"\n", at) + 1
            line += 1
        tab.stop = (stop[1], "%s line %d: %s" % (shown, tab.lines + line + 1, stop[2]))
    elif ec.value:
        why = {1: "fewer fields than the selected columns need (the reference raises IndexError, KeyError or an assertion)",
               2: "more value fields than the header names (the reference stops at an assertion)",
               7: "text that is not ASCII is not supported"}[ec.value]
        tab.stop = (2 if ec.value == 7 else 1, "%s line %d: %s" % (shown, tab.lines + err_line + 1, why))
    for s in [k for k in tab.bad if k >= site0 + n]:
        del tab.bad[s]
    starts = np.flatnonzero(new_run[:n])
    for s in starts.tolist():
        name = text[soff[s]:soff[s] + slen[s]].decode("ascii")
        if tab.run_names and tab.run_names[-1] == name and s == 0:
            continue                                        # the run goes on across the seam of two blocks
        tab.run_starts.append(site0 + s)
        tab.run_names.append(name)
    if dev is not None:
        dev.put(tab.n_sites, vals[:, :n])
    else:
        tab.vals.append(vals[:, :n])
    tab.pos.append(pos[:n])
    tab.n_sites += n
    tab.lines += nl.value


def host_block(tab, blk, sel_col, n_names, exact, shown, universal, n_threads, dev=None):
    """a block through the host parser: a text-mode file's line ends first, text that is not ASCII rejected"""
    if universal and b"\r" in blk:                        # a file in text mode: \r\n and a lone \r end a line
        blk = blk.replace(b"\r\n", b"\n").replace(b"\r", b"\n")
    if not blk.isascii():
        # (a '#' line that is not ASCII is rejected as well)
        at = next(k for k, ch in enumerate(blk) if ch >= 128)
        raise Usage("%s line %d: text that is not ASCII is not supported" % (shown, tab.lines + blk.count(b"\n", 0, at) + 1))
    parse_block(tab, blk, sel_col, n_names, exact, shown, n_threads, dev)


def device_block(tab, blk, dev, info):
    """a block through k_ws_lines; returns its text when the device hands it to the host route, else None"""
    n_lines = C.c_int64()
    if devroute.is_span(blk):
        info["blocks_inflated_on_device"] += 1
    ticket = dev.slot.submit(blk, parse_tail=(tab.n_sites, C.byref(n_lines)))
    ns, hl, nl = C.c_int64(), C.c_int64(), C.c_int64()
    _lib.check(dev.L.pg_ws_dev_collect(dev.h, ticket[0], C.byref(ns), C.byref(hl), C.byref(nl)))
    if hl.value >= 0:
        return dev.slot.host_text(ticket)
    n = ns.value
    dev.take(tab.n_sites + n)
    pos, runf = np.empty(max(n, 1), dtype=np.int64), np.empty(max(n, 1), dtype=np.uint8)
    soff, slen = np.empty(max(n, 1), dtype=np.int64), np.empty(max(n, 1), dtype=np.int32)
    _lib.check(dev.L.pg_ws_dev_meta(dev.h, ticket[0], n, _vp(pos), _vp(runf), _vp(soff), _vp(slen)))
    text_at = dev.slot.text_at(ticket)
    for s_ in np.flatnonzero(runf[:n]).tolist():
        name = bytes(text_at(int(soff[s_]), int(slen[s_]))).decode("ascii")
        if tab.run_names and tab.run_names[-1] == name and s_ == 0:
            continue                                        # the run goes on across the seam of two blocks
        tab.run_starts.append(tab.n_sites + s_)
        tab.run_names.append(name)
    tab.pos.append(pos[:n])
    tab.n_sites += n
    tab.lines += nl.value
    return None


def read_table(reader, carry, sel_col, n_names, exact, shown, universal, info, dev=None):
    """the whole input, a block of PG_STREAM_BYTES at a time: through k_ws_lines into the device's store (dev), the blocks it hands
    back and everything under PG_WS_DEVICE=0 through parse_block"""
    tab = Table(len(sel_col))
    block_bytes = int(os.environ.get("PG_STREAM_BYTES", str(256 << 20)))
    n_threads = int(os.environ.get("PG_HOST_THREADS", "0"))
    budget = float(os.environ.get("PG_SCRATCH_GIB", "48")) * (1 << 30)
    spans = (dev is not None and dev.parses and not carry and isinstance(getattr(reader, "f", None), genoio.BgzfFile)
             and os.environ.get("PG_BGZF_DEVICE", "1") != "0")
    first = True
    for blk in devroute.blocks(reader, block_bytes, dev.slot.pinned() if spans else None, info):
        if first and not devroute.is_span(blk):
            blk = carry + blk
        first = False
        if not len(blk):
            break
        info["blocks"] += 1
        try:
            if dev is not None and dev.parses:
                blk = device_block(tab, blk, dev, info)
            if blk is not None:
                host_block(tab, bytes(blk), sel_col, n_names, exact, shown, universal, n_threads, dev)
        except _lib.PopgenError as exc:
            if "PG_SCRATCH_GIB" in str(exc):
                raise Usage("%s: %s" % (shown, exc))
            raise
        if dev is None and tab.n_sites * len(sel_col) * 8.0 > budget:
            raise Usage("%s: %d selected columns of more than %d sites do not fit the budget of the value store (PG_SCRATCH_GIB = %s)"
                        % (shown, len(sel_col), tab.n_sites - 1, os.environ.get("PG_SCRATCH_GIB", "48")))
        if tab.stop is not None:
            break
    if tab.stop is not None and tab.stop[0] == 2:
        raise Usage(tab.stop[1])
    if dev is None:
        tab.values = np.ascontiguousarray(np.concatenate(tab.vals, axis=1)) if tab.vals else np.zeros((len(sel_col), 0))
    tab.positions = np.concatenate(tab.pos) if tab.pos else np.zeros(0, dtype=np.int64)
    tab.vals = tab.pos = None
    return tab


def find_windows(args, tab, minSites, include, exclude, coords):
    """the windows the reference's generator yields over the table -- of a table that stops early, those it had yielded by then
    (windows.*Stream: the windows that are certain once the rows so far have been read)"""
    final = tab.stop is None
    rs = np.asarray(tab.run_starts, dtype=np.int64)
    try:
        if args.windType == "coordinate":
            st = windows.CoordWindowStream(args.windSize, args.stepSize if args.stepSize else args.windSize, include, exclude)
        elif args.windType == "sites":
            st = windows.SitesWindowStream(args.windSize, args.overlap if args.overlap else 0,
                                           args.maxDist if args.maxDist else np.inf, minSites, include, exclude)
        else:
            st = windows.PredefinedWindowStream(coords)
        T, _ = st.feed(rs, tab.run_names, tab.positions, final)
    except ValueError as exc:
        raise Usage(str(exc))
    return T


def window_mid(positions, lo, hi):
    """GenoWindow.midPos (genomics.py:1795-1797): int(round(sum / len)) in Python's exact integers, nan without sites"""
    n = len(lo)
    if n == 0:
        return []
    small = len(positions) == 0 or (int(np.abs(positions).max()) < (1 << 31) and len(positions) < (1 << 31))
    if small:
        csum = np.concatenate([[0], np.cumsum(positions, dtype=np.int64)])
        tot = (csum[hi] - csum[lo]).tolist()
    else:
        plist = positions.tolist()
        tot = [sum(plist[a:b]) for a, b in zip(lo.tolist(), hi.tolist())]
    return [int(round(t / s)) if s > 0 else float("nan") for t, s in zip(tot, (hi - lo).tolist())]


def host_stats(values, lo, hi, mask, n_threads=0):
    """pg_ws_stats_host: (out[n_win][n_cols][12], cnt, flag)"""
    n_cols, pitch = values.shape
    n_win = len(lo)
    out = np.zeros((n_win, n_cols, len(STATS)), dtype=np.float64)
    cnt = np.zeros((n_win, n_cols), dtype=np.int64)
    flag = np.zeros((n_win, n_cols), dtype=np.uint8)
    lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
    rc = _lib.lib().pg_ws_stats_host(_vp(values), pitch, n_cols, _vp(lo), _vp(hi), n_win, mask, devroute.host_threads(n_threads), _vp(out),
                                     _vp(cnt), _vp(flag))
    if rc != 0:
        raise RuntimeError("pg_ws_stats_host: bad arguments")
    return out, cnt, flag


class Device:
    """the value store on the device, k_ws_lines into it (a devroute.SlotDevice over the route's entry points) and k_ws_stats over it"""

    def __init__(self, device, n_cols, n_fields=0, sel_field=None):
        self.slot = devroute.SlotDevice(device, "ws")
        self.eng = self.slot.eng
        self.L, self.h = self.eng._L, self.eng._h
        self.n_cols = n_cols
        self.parses = False
        try:
            _lib.check(self.L.pg_ws_reserve(self.h, n_cols, 0))
            if sel_field is not None:
                taken = C.c_int()
                sel_field = np.ascontiguousarray(sel_field, dtype=np.int32)
                _lib.check(self.L.pg_ws_dev_config(self.h, n_fields, n_cols, _vp(sel_field), C.byref(taken)))
                self.parses = taken.value == 1
        except BaseException:
            self.close()
            raise

    @classmethod
    def from_values(cls, device, values):
        """a store filled from host memory (tools/wstats_bench.py's kernel leg)"""
        dev = cls(device, values.shape[0])
        try:
            dev.put(0, values)
        except BaseException:
            dev.close()
            raise
        return dev

    def take(self, n_sites):
        """the store holds n_sites sites from now on (those a block's kernels wrote, or room for a host block's)"""
        _lib.check(self.L.pg_ws_reserve(self.h, self.n_cols, int(n_sites)))

    def put(self, site0, values):
        """values[column][site] behind site0"""
        n = values.shape[1]
        self.take(site0 + n)
        for c in range(self.n_cols):
            col = np.ascontiguousarray(values[c])
            _lib.check(self.L.pg_ws_put(self.h, c, int(site0), _vp(col), n))

    def stats(self, lo, hi, mask, lds_vals):
        n_win = len(lo)
        out = np.zeros((n_win, self.n_cols, len(STATS)), dtype=np.float64)
        cnt = np.zeros((n_win, self.n_cols), dtype=np.int64)
        flag = np.zeros((n_win, self.n_cols), dtype=np.uint8)
        tiers = np.zeros(2, dtype=np.int64)
        ms = C.c_double()
        lo, hi = np.ascontiguousarray(lo, dtype=np.int64), np.ascontiguousarray(hi, dtype=np.int64)
        _lib.check(self.L.pg_ws_stats(self.h, _vp(lo), _vp(hi), n_win, mask, lds_vals, _vp(out), _vp(cnt), _vp(flag), _vp(tiers), C.byref(ms)))
        return out, cnt, flag, tiers, ms.value

    def copy_ms(self):
        ms = C.c_double()
        _lib.check(self.L.pg_ws_copy_time(self.h, C.byref(ms)))
        return ms.value

    def close(self):
        self.L.pg_ws_end(self.h)
        self.eng.close()


def _fmt(x):
    return repr(x)                                         # str(np.float64): the shortest digits that read back, `nan`, `inf`


def wstats_main(argv=None):
    t0 = time.perf_counter()
    args = make_parser().parse_args(argv)
    world = dist.world_from_env()
    if world.size > 1 and world.rank != 0:                 # rank 0 does the whole job
        return 0
    minSites = _window_params(args)
    coords = _read_coords(args.windCoords) if args.windType == "predefined" else None
    shown = args.inFile or "<stdin>"
    universal = args.inFile is not None

    exclude = include = None
    if args.exclude:
        exclude = _scaf_list(args.exclude)
        sys.stderr.write("%d scaffolds will be excluded.\n" % len(exclude))
    if args.include:
        include = _scaf_list(args.include)
        sys.stderr.write("%d scaffolds will be analysed.\n" % len(include))

    reader = genoio.BlockReader(args.inFile)
    carry = b""
    if args.headers:
        header = " ".join(args.headers)
        if not header.isascii():
            raise Usage("--headers: text that is not ASCII is not supported")
        fields = header.split()
    else:
        fields, carry = devroute.geno_header(reader, universal, shown, Usage)
    names = fields[2:]
    if not names:
        raise Usage("%s: the header names no value column (the reference fails at the first window)" % shown)
    if args.columns:
        for name in args.columns:
            if name not in names:
                raise Usage("--columns: %s is not in the header (the reference raises KeyError)" % name)
        out_names = list(args.columns)
        sel_col = [len(names) - 1 - names[::-1].index(n) for n in out_names]      # a name the header holds twice: its last cell
        exact = False
    else:
        out_names = list(names)
        sel_col = [names.index(n) for n in names]          # (seqDict looks a name up with list.index: the first of two)
        exact = True
    sel_col = np.ascontiguousarray(sel_col, dtype=np.int32)
    stats = list(args.stats)
    mask = 0
    for s in stats:
        mask |= 1 << STATS.index(s)
    stat_idx = np.asarray([STATS.index(s) for s in stats], dtype=np.int64)

    info = dict(blocks=0, text_bytes=0, sites=0, windows=0, windows_computed=0, device_cells=0, device_lds_cells=0, device_big_cells=0,
                device_blocks=0, device_host_blocks=0, blocks_inflated_on_device=0, host_cells=0, cells_through_float=0, kernel_ms=0.0)
    use_device = os.environ.get("PG_WS_DEVICE", "1") != "0"
    dev = None
    if use_device:
        dev = Device(args.device if args.device is not None else dist.device_for(world), len(sel_col), len(names) + 2, sel_col + 2)
    try:
        return _run(args, world, t0, reader, carry, sel_col, names, out_names, exact, shown, universal, info, stats, mask, stat_idx,
                    minSites, include, exclude, coords, dev)
    finally:
        if dev is not None:
            dev.close()


def _run(args, world, t0, reader, carry, sel_col, names, out_names, exact, shown, universal, info, stats, mask, stat_idx, minSites,
         include, exclude, coords, dev):
    use_device = dev is not None
    tab = read_table(reader, carry, sel_col, len(names), exact, shown, universal, info, dev)
    info["sites"], info["cells_through_float"] = tab.n_sites, tab.host_cells
    if dev is not None:
        info["device_blocks"], info["device_host_blocks"] = dev.slot.stats()
    T = find_windows(args, tab, minSites, include, exclude, coords)
    n_win = T.n
    dup = np.asarray(getattr(T, "dup", np.zeros(n_win, dtype=bool)), dtype=bool)
    lo, hi = T.lo.copy(), T.hi.copy()
    sites = hi - lo
    enough = (sites >= minSites) & ~dup

    # the first window, in output order, that has enough sites and holds a cell NumPy does not convert: the reference dies there
    stop_at, stop_msg = n_win, None
    if tab.bad:
        bad_sites = np.asarray(sorted(tab.bad), dtype=np.int64)
        first_bad = np.searchsorted(bad_sites, lo, side="left")
        holds = enough & (first_bad < len(bad_sites)) & (bad_sites[np.minimum(first_bad, len(bad_sites) - 1)] < hi)
        if holds.any():
            stop_at = int(np.argmax(holds))
            s = int(bad_sites[first_bad[stop_at]])
            k, cell = tab.bad[s]
            stop_msg = ("%s: window %d (%s %s-%s), column %s: the cell %r is not a number (the reference raises ValueError)"
                        % (shown, stop_at + 1, T.scaffold[stop_at], T.start[stop_at], T.end[stop_at], out_names[k], cell))

    todo = np.flatnonzero(enough[:stop_at])
    n_threads = int(os.environ.get("PG_HOST_THREADS", "0"))
    n_sel = len(sel_col)
    if len(todo):
        if use_device:
            lds_vals = int(os.environ.get("PG_WS_LDS_VALS", str(LDS_DEFAULT)))
            if not 1 <= lds_vals <= LDS_DEFAULT:
                raise Usage("PG_WS_LDS_VALS=%d: 1 .. %d values fit the piece in LDS" % (lds_vals, LDS_DEFAULT))
            out, cnt, flag, tiers, ms = dev.stats(lo[todo], hi[todo], mask, lds_vals)
            info["device_cells"] = int(len(todo)) * n_sel
            info["device_lds_cells"], info["device_big_cells"], info["kernel_ms"] = int(tiers[0]), int(tiers[1]), round(ms, 3)
        else:
            out, cnt, flag = host_stats(tab.values, lo[todo], hi[todo], mask, n_threads)
            info["host_cells"] = int(len(todo)) * n_sel
        if flag.any():                                     # min / max of a column without a value: the reference dies there
            row = int(np.argmax(flag.any(axis=1)))
            w = int(todo[row])
            k = int(np.argmax(flag[row]))
            stop_at = w
            stop_msg = ("%s: window %d (%s %s-%s), column %s: min / max of a column without a value (the reference raises ValueError)"
                        % (shown, w + 1, T.scaffold[w], T.start[w], T.end[w], out_names[k]))
            out = out[:row]
            todo = todo[:row]
        with np.errstate(all="ignore"):
            out[:, :, SD] = np.round(out[:, :, SD], 6)     # round(np.float64, 6): times 1e6, rint, over 1e6
        cells = out[:, :, stat_idx].reshape(len(todo), n_sel * len(stats))
    else:
        cells = np.zeros((0, n_sel * len(stats)))
    info["windows"], info["windows_computed"] = n_win, int(len(todo))

    mid = window_mid(tab.positions, lo, hi)
    failed = ",".join(["nan"] * (n_sel * len(stats)))
    rows_of = dict(zip(todo.tolist(), range(len(todo))))
    cell_rows = cells.tolist()
    sink = devroute.open_rows(args.outFile)
    ok = False
    try:
        parts = ["scaffold,start,end,mid,sites"]
        n_written = min(stop_at, n_win)
        if tab.stop is None and stop_msg is None:
            n_written = n_win
        prev = None
        if n_written > 0 or stop_msg is not None:          # the header row is finished when the first window arrives
            parts.append("".join("," + ",".join(name + "_" + s for s in stats) for name in out_names) + "\n")
        for w in range(n_written):
            if dup[w] and prev is not None:                # the generator yields its last window once more behind a skipped scaffold
                row = prev
            else:
                head = "%s,%s,%s,%s,%d," % (T.scaffold[w], T.start[w], T.end[w], mid[w], sites[w])
                k = rows_of.get(w)
                row = head + (failed if k is None else ",".join(_fmt(x) for x in cell_rows[k])) + "\n"
            parts.append(row)
            prev = row
            if (w + 1) % 100 == 0:
                sys.stderr.write(str(w + 1) + " windows analysed...\n")
                sink.write("".join(parts).encode("ascii"))
                parts = []
        sink.write("".join(parts).encode("ascii"))
        ok = True
    finally:
        devroute.close_rows(sink, ok)
    info["total_s"] = round(time.perf_counter() - t0, 4)
    devroute.report(last_info, info, "wstats")
    if stop_msg is not None:
        raise Stop(stop_msg)
    if tab.stop is not None:
        raise Stop(tab.stop[1])
    return 0


def main(argv=None):
    return wstats_main(argv)
