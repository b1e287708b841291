"""Drop-in for the reference's tools/genoToEigenstrat.py: the biallelic sites of a `.geno` file written as EIGENSTRAT .geno / .snp /
.ind files -- a site's alleles from the base counts of ALL samples of the file, the rarer one counted in the selected samples.

The per-site and per-cell rules live in csrc/pg_eig_core.h and run on the device (pg_eig_dev_*: k_eig_lines) for blocks of the regular
spelling, on host threads (pg_eig_text) for everything else, for --cumulativePos, for a header with a repeated name and under
PG_EIG_DEVICE=0.  Header, sample selection and --chromFile follow genoToEigenstrat.py:18-45.  Where the reference dies with a traceback
this driver stops with one message: before any output file is opened with exit status 2 (no -f, -f paired, a header without samples, a
--chromFile line that is not two fields, a header that is not ASCII; a line that is not ASCII, a position of more than 18 digits or a
genotype of more than 16 alleles removes the two files begun), at the line otherwise -- the rows before it written, no .ind file.
Divergence: a -s that matches no header name is rejected (the reference then writes every sample, sorted by name, and an empty .ind).
Bgzipped input crosses PCIe as its members, inflated by k_inflate into the route's text slot.
"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

from . import _lib, devroute, dist, genoio

IN_FMT = {"phased": 0, "diplo": 1}
ERRORS = {
    1: "a blank line or a line of one field (the reference raises IndexError)",
    2: "-f diplo: a genotype that is not one of A C G K M N S R T W Y (the reference raises KeyError)",
    3: "the position is not an integer (the reference raises ValueError)",
    4: "a biallelic site at which a selected sample has no cell (the reference raises KeyError)",
    5: "--cumulativePos: no offset is kept under the scaffold's chromosome label (the reference raises KeyError)",
    7: "text that is not ASCII is not supported",
    8: "a position of more than 18 digits is not supported",
    9: "a genotype of more than 16 alleles is not supported",
}
REJECTED = (7, 8, 9)                                   # exit status 2, as for an input the drop-in does not take
MAX_SCAF, MAX_LABEL = 1 << 22, 255                     # PG_EIG_MAX_SCAF, PG_EIG_MAX_LABEL: what the device route takes of a --chromFile

ENGINE_EPILOG = ("MI355X engine: blocks of the regular spelling (single tabs, the header's field count, ASCII, positions as plain "
                 "decimals, genotypes of at most nine alleles, no '#' line) are converted on the device, every other block on host "
                 "threads; --cumulativePos, a header with a repeated name and a --chromFile of more than 2^22 scaffolds or a label of "
                 "more than 255 bytes on host threads throughout.  Under WORLD_SIZE > 1 rank 0 does the whole job.  Environment: "
                 "PG_EIG_DEVICE=0 host threads only, =1 the device whatever the input's size; PG_BGZF_DEVICE=0 bgzip members inflated "
                 "by host threads; PG_STREAM_BYTES text bytes per block (default 256 MiB); PG_HOST_THREADS host threads; PG_TIMING=1 "
                 "blocks and times on stderr.")

last_info = {}


class Usage(devroute.Usage):
    prog = "genoToEigenstrat.py"


class EigCfg(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("in_fmt", "n_sel", "n_cols", "universal_newlines", "cumulative", "n_scaf")]


class EigState(C.Structure):
    _fields_ = [("sites", C.c_int64), ("pos", C.c_int64), ("scaf_len", C.c_int64), ("entry", C.c_int32), ("pad", C.c_int32)]


def make_parser():
    ap = argparse.ArgumentParser(prog="genoToEigenstrat.py", epilog=ENGINE_EPILOG)
    ap.add_argument("-g", "--genoFile", help="Input vcf file", action="store")
    ap.add_argument("-f", "--genoFormat", help="Genotype format [otherwise will be inferred (slower)]", action="store",
                    choices=["phased", "diplo", "paired"])
    ap.add_argument("--genoOutFile", help="Output Eigenstrat geno file", action="store", required=True)
    ap.add_argument("--snpOutFile", help="Output Eigenstrat snp file", action="store", required=True)
    ap.add_argument("--indOutFile", help="Output Eigenstrat ind file", action="store", required=True)
    ap.add_argument("-s", "--samples", help="sample names (separated by commas)", action="store")
    ap.add_argument("--chromFile", help="Input chromosome number file", action="store")
    ap.add_argument("--cumulativePos", help="For chroms with multiple scafs, add positions to previous scaf", action="store_true")
    ap.add_argument("--nullChrom", help="Chrom_for_unknown_scafs", action="store", type=int, default=22)
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


_vp = devroute.vp


class _Plan:
    """the option set, the header's tables and the --chromFile in the forms pg_eig_text / pg_eig_dev_config take, and what one block
    hands the next (the sites done; with --cumulativePos the scaffold, its label, the last position, the offsets)"""

    def __init__(self, cfg, sel_col, prev_same, next_same, repeats, chrom, null_label):
        self.cfg = cfg
        self.sel_col = np.ascontiguousarray(sel_col if len(sel_col) else [0], dtype=np.int32)
        self.repeats = repeats
        self.prev_same = np.ascontiguousarray(prev_same, dtype=np.int32)
        self.next_same = np.ascontiguousarray(next_same, dtype=np.int32)
        names = list(chrom)
        self.n_scaf = len(names)
        self.names = b"".join(names)
        self.name_off = np.zeros(self.n_scaf + 1, dtype=np.int64)
        np.cumsum([len(n) for n in names], out=self.name_off[1:])
        labels = [chrom[n] for n in names] + [null_label]
        self.labels = b"".join(labels)
        self.label_off = np.zeros(self.n_scaf + 2, dtype=np.int64)
        np.cumsum([len(x) for x in labels], out=self.label_off[1:])
        self.max_label = max(len(x) for x in labels)
        slot = {}
        for key in names + [null_label]:                   # chromOffset: the file's scaffold names and str(nullChrom)
            slot.setdefault(key, len(slot))
        self.label_key = np.ascontiguousarray([slot.get(x, -1) for x in labels], dtype=np.int32)
        self.offsets = np.zeros(len(slot), dtype=np.int64)
        size = 4
        while size < 2 * self.n_scaf:
            size <<= 1
        self.mask = size - 1
        self.table = np.empty(size, dtype=np.int32)
        _lib.check(_lib.lib().pg_gvcf_ref_table(self.names, _vp(self.name_off), self.n_scaf, _vp(self.table), self.mask))
        self.state = EigState(0, 0, -1, -1, 0)
        self.scaf = b""

    def same_args(self):
        return (_vp(self.prev_same), _vp(self.next_same)) if self.repeats else (None, None)


def host_eig(plan, text, n_threads=0):
    """pg_eig_text on a block of lines: (.geno rows, .snp rows, error code, line index in the block, sites walked); the plan's state
    moves on"""
    L = _lib.lib()
    buf = text if isinstance(text, bytes) else bytes(text)
    n_threads = devroute.host_threads(n_threads)
    n_lines = buf.count(b"\n") + buf.count(b"\r") + 1
    gcap, scap = n_lines * (plan.cfg.n_sel + 1) + 64, n_lines * (40 + plan.max_label) + 64
    scaf = C.create_string_buffer(max(len(buf), len(plan.scaf), 1))
    C.memmove(scaf, plan.scaf, len(plan.scaf))
    while True:
        geno, snp = np.empty(gcap, dtype=np.uint8), np.empty(scap, dtype=np.uint8)
        gl, sl, nr, ns, el, ec = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        _lib.check(L.pg_eig_text(C.c_void_p(C.addressof(plan.cfg)), _vp(plan.sel_col), *plan.same_args(), plan.names, _vp(plan.name_off),
                                 _vp(plan.table), plan.mask, plan.labels, _vp(plan.label_off), _vp(plan.label_key),
                                 C.c_void_p(C.addressof(plan.state)), _vp(plan.offsets), C.cast(scaf, C.c_void_p), buf, len(buf), n_threads,
                                 _vp(geno), gcap, _vp(snp), scap, C.byref(gl), C.byref(sl), C.byref(nr), C.byref(ns), C.byref(el),
                                 C.byref(ec)))
        if gl.value <= gcap and sl.value <= scap:
            if plan.cfg.cumulative and plan.state.scaf_len >= 0:
                plan.scaf = scaf.raw[:plan.state.scaf_len]
            return geno[:gl.value].tobytes(), snp[:sl.value].tobytes(), ec.value, el.value, ns.value
        gcap, scap = max(gcap, gl.value), max(scap, sl.value)


class _Device(devroute.SlotDevice):
    """the device route (devroute.SlotDevice): one block converted while the next is submitted"""

    def __init__(self, plan, device):
        super().__init__(device, "eig")
        self.n_sel = plan.cfg.n_sel
        taken = C.c_int()
        _lib.check(self.L.pg_eig_dev_config(self.eng._h, C.c_void_p(C.addressof(plan.cfg)), _vp(plan.sel_col), plan.names, _vp(plan.name_off),
                                            _vp(plan.table), plan.mask, plan.labels, _vp(plan.label_off), C.byref(taken)))
        self.taken = taken.value

    def submit(self, block, first_site):
        """the ticket, the site index the block was given and the number of its lines"""
        n_lines = C.c_int64()
        ticket = super().submit(block, parse_tail=(first_site, C.byref(n_lines)))
        return ticket, first_site, n_lines.value

    def collect(self, ticket, as_text=False):
        """(.geno rows, .snp rows, text, lines): rows None: the block is the host's (or, as_text, the caller's wish), `text` its text"""
        s = ticket[0]
        sl, nr, hl, nl = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pg_eig_dev_collect(self.eng._h, s, C.byref(sl), C.byref(nr), C.byref(hl), C.byref(nl)))
        if hl.value >= 0 or as_text:
            return None, None, self.host_text(ticket), nl.value
        geno = devroute.fetch(self.L.pg_eig_dev_rows, self.eng._h, nr.value * (self.n_sel + 1), s, 0).tobytes()
        return geno, devroute.fetch(self.L.pg_eig_dev_rows, self.eng._h, sl.value, s, 1).tobytes(), None, nl.value


def read_chrom_file(path):
    """dict(line.split() for line in chromFile) of a file read in text mode, as bytes: of two lines for one scaffold the later wins"""
    with open(path, "rb") as f:
        raw = f.read()
    if not raw.isascii():
        raise Usage("%s: %s" % (path, ERRORS[7]))
    chrom = {}
    for k, line in enumerate(raw.decode("ascii").splitlines(True) if b"\r" not in raw else
                             raw.replace(b"\r\n", b"\n").replace(b"\r", b"\n").decode("ascii").splitlines(True)):
        parts = line.split()
        if len(parts) != 2:
            raise Usage("%s line %d: %d fields where a scaffold and its chromosome are needed (the reference raises ValueError)"
                        % (path, k + 1, len(parts)))
        chrom[parts[0].encode("ascii")] = parts[1].encode("ascii")
    return chrom


def genoeig_main(argv=None):
    t0 = time.perf_counter()
    args = make_parser().parse_args(argv)
    world = dist.world_from_env()
    if world.size > 1 and world.rank != 0:                 # rank 0 does the whole job
        return 0
    if not args.genoFormat:
        raise Usage("-f phased|diplo is needed (the reference raises ValueError at the first site)")
    if args.genoFormat == "paired":
        raise Usage("-f paired: the reference offers the choice and raises ValueError on it at the first site; use phased or diplo")
    shown = args.genoFile or "<stdin>"
    universal = args.genoFile is not None                  # (a file in text mode; stdin keeps its \r inside the line)
    chrom = read_chrom_file(args.chromFile) if args.chromFile else {}

    reader = genoio.BlockReader(args.genoFile)
    headers, carry = devroute.geno_header(reader, universal, shown, Usage)
    all_names = headers[2:]
    if not all_names:
        raise Usage("%s line 1: the header names no sample (the reference stops at an assertion at the first site)" % shown)
    if args.samples is not None:
        if not args.samples.isascii():
            raise Usage("-s: " + ERRORS[7])
        wanted = set(args.samples.split(","))
        names_to_use = [n for n in all_names if n in wanted]   # in file order; a name the header lacks is ignored
        if not names_to_use:
            raise Usage("-s: none of the samples is in the header (the reference then writes every sample, sorted by name, and an "
                        "empty .ind file; this is not followed)")
    else:
        names_to_use = all_names
    last_col = {n: k + 2 for k, n in enumerate(all_names)}     # a name the header holds twice: its last field
    prev_same, next_same, seen = [-1] * len(headers), [-1] * len(headers), {}
    for k, n in enumerate(all_names):
        prev_same[k + 2] = seen.get(n, -1)
        if n in seen:
            next_same[seen[n]] = k + 2
        seen[n] = k + 2
    repeats = len(seen) != len(all_names)

    cfg = EigCfg()
    cfg.in_fmt = IN_FMT[args.genoFormat]
    cfg.n_sel = len(names_to_use)
    cfg.n_cols = len(headers)
    cfg.universal_newlines = int(universal)
    cfg.cumulative = int(bool(args.cumulativePos))
    cfg.n_scaf = len(chrom)
    plan = _Plan(cfg, [last_col[n] for n in names_to_use], prev_same, next_same, repeats, chrom, str(args.nullChrom).encode("ascii"))

    with open(args.genoOutFile, "wb") as geno_out, open(args.snpOutFile, "wb") as snp_out:
        rc = _run(args, reader, geno_out, snp_out, plan, carry, shown, world, t0)
    if rc:
        if rc == 2:                                        # an input the drop-in does not take leaves no file behind
            for path in (args.genoOutFile, args.snpOutFile):
                if os.path.isfile(path) and not os.path.islink(path):
                    os.remove(path)
        return rc
    with open(args.indOutFile, "wb") as ind:
        ind.write("".join(n + "  U  NA\n" for n in names_to_use).encode("ascii"))
    return 0


def _run(args, reader, geno_out, snp_out, plan, carry, shown, world, t0):
    cfg = plan.cfg
    use_device = os.environ.get("PG_EIG_DEVICE", "1") != "0"
    why_host = None
    if use_device:
        if cfg.cumulative:
            why_host = "--cumulativePos is a walk over the scaffold changes in file order"
        elif plan.repeats:
            why_host = "the header holds a sample name more than once"
        elif plan.n_scaf > MAX_SCAF or plan.max_label > MAX_LABEL:
            why_host = "the --chromFile holds more than %d scaffolds or a label of more than %d bytes" % (MAX_SCAF, MAX_LABEL)
        if why_host:
            sys.stderr.write("genoToEigenstrat.py: %s: host threads do the job\n" % why_host)
    dev = None
    if use_device and not why_host:
        dev = _Device(plan, args.device if args.device is not None else dist.device_for(world))
        if dev.taken != 1:
            dev.close()
            dev = None
    block_bytes = int(os.environ.get("PG_STREAM_BYTES", str(256 << 20)))
    n_threads = int(os.environ.get("PG_HOST_THREADS", "0"))
    info = dict(blocks=0, blocks_on_device=0, blocks_on_host=0, blocks_redone_on_host=0, rows=0, sites=0, text_bytes=0,
                blocks_inflated_on_device=0)
    t_ctx = time.perf_counter()
    done = [1]                              # lines of the file in front of the block in hand (the header is one)

    def said(before, now):
        for m in range(before // 100000 + 1, now // 100000 + 1):
            print(m * 100000, "lines done...")

    def finish(result):
        """a block's result -> the two files; returns an exit code or None"""
        geno, snp, text, n_lines = result
        before = plan.state.sites
        if geno is None:
            geno, snp, err, at, n_sites = host_eig(plan, text, n_threads)
            info["blocks_on_host"] += 1
            geno_out.write(geno)
            snp_out.write(snp)
            said(before, before + n_sites)
            if err:
                sys.stdout.flush()
                sys.stderr.write("genoToEigenstrat.py: %s line %d: %s\n" % (shown, done[0] + at + 1, _worded(plan, err, text, at)))
                return 2 if err in REJECTED else 1
        else:
            info["blocks_on_device"] += 1
            geno_out.write(geno)
            snp_out.write(snp)
            plan.state.sites += n_lines     # (a block the device takes holds no '#' line)
            said(before, plan.state.sites)
        info["rows"] += snp.count(b"\n")
        done[0] += n_lines
        return None

    flying = [None]                         # the block on the device: (ticket, the site index it was given, its lines)

    def submit(blk):
        flying[0] = dev.submit(blk, plan.state.sites + (flying[0][2] if flying[0] is not None else 0))
        return flying[0]

    def collect(block):
        ticket, first, _ = block
        if block is flying[0]:
            flying[0] = None
        stale = first != plan.state.sites   # the block before held '#' lines: the index this one was given is not its own
        if stale:
            info["blocks_redone_on_host"] += 1
        return dev.collect(ticket, as_text=stale)

    spans = (dev is not None and not carry and isinstance(getattr(reader, "f", None), genoio.BgzfFile)
             and os.environ.get("PG_BGZF_DEVICE", "1") != "0")
    blocks = devroute.read_ahead(devroute.blocks(reader, block_bytes, dev.pinned() if spans else None, info), "pg-eig-read")
    rc = devroute.run_blocks(blocks, dev, info, finish, lambda text, n_lines: finish((None, None, text, n_lines)), submit=submit,
                             collect=collect, universal=bool(cfg.universal_newlines), carry=carry)
    if rc:
        return rc
    if dev is not None:
        info["device_blocks"], info["device_host_blocks"] = dev.stats()
        dev.close()
    sys.stdout.flush()
    info["sites"] = plan.state.sites
    info["total_s"] = time.perf_counter() - t0
    info["eig_s"] = time.perf_counter() - t_ctx
    devroute.report(last_info, info, "eig")
    return 0


def _worded(plan, err, text, at):
    """the message of a stop; the --cumulativePos KeyError names the label and the scaffold"""
    msg = ERRORS.get(err, "error %d" % err)
    if err == 5:
        lines = text.replace(b"\r\n", b"\n").replace(b"\r", b"\n").split(b"\n") if plan.cfg.universal_newlines else text.split(b"\n")
        scaf = lines[at].split()[0]
        label = dict(zip(_names(plan), _labels(plan))).get(scaf, _labels(plan)[-1])
        msg += ": label %s of scaffold %s" % (label.decode("ascii"), scaf.decode("ascii"))
    return msg


def _names(plan):
    return [plan.names[plan.name_off[k]:plan.name_off[k + 1]] for k in range(plan.n_scaf)]


def _labels(plan):
    return [plan.labels[plan.label_off[k]:plan.label_off[k + 1]] for k in range(plan.n_scaf + 1)]


def main():
    return genoeig_main()
