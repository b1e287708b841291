"""Drop-in for the reference's filterGenotypes.py: `.geno` sites filtered by siteTest, include / exclude lists and per-pod thinning,
written in any of its output formats.

The per-cell and per-site rules live in csrc/pg_filter_core.h and run on the device (pg_filter_dev_*: k_filt_lines, k_filt_thin) for
blocks of the regular spelling, on host threads (pg_filter_text) for everything else and under PG_FILTER_DEVICE=0.  Sample and
population setup follows filterGenotypes.py:188-327 line for line.  Where the reference's worker raises and the reference then waits
forever (a ploidy mismatch, -of diplo of a non-pair, --HWE with populations, a blank line ...), this driver stops with a non-zero exit
and names the line.  Divergences: -of randomAllele writes the genotype's first allele (the reference draws one); -o x.gz is BGZF.
Bgzipped input crosses PCIe as its members, inflated by k_inflate into the filter's own text slot; `-o x.gz` rows are deflated where
they lie (k_deflate).
"""
import argparse
import ctypes as C
import os
import string
import sys
import time

import numpy as np

from . import _lib, devroute, dist, genoio

IN_FMT = {"phased": 0, "diplo": 1, "alleles": 2}
OUT_FMT = {"phased": 0, "diplo": 1, "bases": 2, "alleles": 3, "randomAllele": 4, "coded": 5, "count": 6}
MAXPOP = 32
ERRORS = {
    1: "the line has fewer fields than the selected samples need (the reference's worker raises IndexError here and never ends)",
    2: "a genotype's ploidy does not match --ploidy / --ploidyFile and --forcePloidy is not set (the reference's worker raises here "
       "and never ends)",
    3: "-if diplo: a genotype that is not one of A C G K M N S R T W Y (the reference's worker raises here and never ends)",
    4: "-of diplo: a genotype that is not a diploid pair of A/C/G/T/N the reference knows (the reference's worker raises here and never ends)",
    5: "--HWE with populations: a population holds a genotype other than N/N at a variable site, where the reference's HWE test "
       "calls an undefined function; its worker dies and it never ends (no test is invented here)",
    6: "--nearlyFixedDiff needs two populations or more (the reference's worker raises here and never ends)",
    7: "-of count at a site without any called base (the reference's worker raises here and never ends)",
    8: "--alleleOrder freq: a genotype holds an allele that is not among the site's alleles (the reference's worker raises here and "
       "never ends)",
    9: "--thinDist: the position is not an integer of up to 18 significant digits",
    10: "a genotype of more than 16 alleles, or text that is not ASCII, is not supported",
    11: "a population names a sample that is not among the selected samples, and the line reaches the population filters (the "
        "reference's worker raises KeyError here and never ends)",
}

ENGINE_EPILOG = ("MI355X engine: blocks of the regular spelling (single tabs, the header's field count, ASCII) are filtered on the "
                 "device, every other block on host threads.  Under WORLD_SIZE > 1 rank 0 does the whole job.  Environment: "
                 "PG_FILTER_DEVICE=0 host threads only; PG_BGZF_DEVICE=0 bgzip members inflated by host threads; PG_DEFLATE_DEVICE=0 "
                 "-o x.gz rows deflated by host threads; PG_STREAM_BYTES text bytes per block (default 256 MiB); PG_HOST_THREADS "
                 "host threads; PG_TIMING=1 blocks and times on stderr.")

last_info = {}


class FilterCfg(C.Structure):
    _fields_ = ([(n, C.c_int32) for n in ("in_fmt", "out_fmt", "freq_order", "force_ploidy", "partial_to_missing", "no_test", "n_sel",
                                          "n_pops", "n_cols", "n_contigs", "contig_mode", "min_calls", "min_alleles", "min_var",
                                          "has_max_het", "hwe", "fixed", "has_pop_calls", "has_pop_alleles", "has_nfd")]
                + [(n, C.c_double) for n in ("max_alleles", "max_het", "min_freq", "max_freq", "nfd")]
                + [("thin_dist", C.c_int64), ("pod_size", C.c_int64)]
                + [(n, C.c_int32 * MAXPOP) for n in ("pop_calls_min", "pop_alleles_min", "pop_alleles_max")]
                + [("pop_empty", C.c_uint32), ("pop_missing", C.c_uint32), ("universal_newlines", C.c_int32)])


def make_parser():
    ap = argparse.ArgumentParser(prog="filterGenotypes.py", epilog=ENGINE_EPILOG)
    ap.add_argument("-i", "--infile", help="Input vcf file", action="store", required=False)
    ap.add_argument("-o", "--outfile", help="Output csv file", action="store")
    ap.add_argument("-t", "--threads", help="Analysis threads", type=int, action="store", default=1)
    ap.add_argument("--verbose", help="Verbose output.", action="store_true")
    ap.add_argument("-if", "--inputGenoFormat", help="Genotype format [otherwise will be inferred (slower)]", action="store",
                    choices=["phased", "diplo", "alleles"], default="phased")
    ap.add_argument("-of", "--outputGenoFormat", action="store", default="phased",
                    choices=("phased", "diplo", "bases", "alleles", "randomAllele", "coded", "count"), help="Genotype format for output")
    ap.add_argument("--alleleOrder", action="store", default=None, choices=("freq",),
                    help="Order sample alleles by frequency when outputting 'bases' or 'alleles'")
    ap.add_argument("-s", "--samples", help="sample names (separated by commas)", action="store")
    ap.add_argument("--excludeSamples", help="sample names (separated by commas)", action="store")
    ap.add_argument("-p", "--pop", help="Pop name and optionally sample names (separated by commas)", action="append", nargs="+",
                    metavar=("popName", "[samples]"))
    ap.add_argument("--popsFile", help="Optional file of sample names and populations", action="store", required=False)
    ap.add_argument("--keepAllSamples", help="Keep all samples (not just specified populations)", action="store_true")
    ap.add_argument("--ploidy", help="Ploidy for each sample", action="store", type=int, nargs="+")
    ap.add_argument("--ploidyFile", help="File with samples names and ploidy as columns", action="store")
    ap.add_argument("--forcePloidy", help="Force genotypes to specified ploidy", action="store_true")
    ap.add_argument("--partialToMissing", help="Set partially missing genotypes to completely missing", action="store_true")
    ap.add_argument("--include", help="include contigs", nargs="+", action="store")
    ap.add_argument("--includeFile", help="File of contigs (one per line)", action="store")
    ap.add_argument("--exclude", help="exclude contigs", nargs="+", action="store")
    ap.add_argument("--excludeFile", help="File of contigs (one per line)", action="store")
    ap.add_argument("--minCalls", help="Minimum number of good genotype calls", type=int, action="store", default=1, metavar="integer")
    ap.add_argument("--minAlleles", help="Minimum number of alleles at a site", type=int, action="store", default=1, metavar="integer")
    ap.add_argument("--maxAlleles", help="Maximum number of alleles at a site", type=float, action="store", default="inf",
                    metavar="integer or 'inf'")
    ap.add_argument("--minVarCount", help="Minimum number of instances for rare vaiants", type=int, action="store", default=None,
                    metavar="integer")
    ap.add_argument("--maxHet", help="Maximum proportion of heterozygous genotypes", type=float, action="store", default=None,
                    metavar="proportion")
    ap.add_argument("--minFreq", help="Minimum variant frequency", type=float, action="store", default=None, metavar="freqency")
    ap.add_argument("--maxFreq", help="Maximum variant frequency", type=float, action="store", default=None, metavar="frequency")
    ap.add_argument("--HWE", help="Hardy-Weinberg equalibrium test P-value and side", action="store", nargs=2,
                    metavar=("P-value", "'top'/'bottom'/'both'"))
    ap.add_argument("--minPopCalls", help="Minimum number of good genotype calls per pop", nargs="+", action="store", type=int)
    ap.add_argument("--minPopAlleles", help="Minimum number of alleles per site per pop", nargs="+", action="store", type=int)
    ap.add_argument("--maxPopAlleles", help="Maximum number of alleles per site per pop", nargs="+", action="store", type=int)
    ap.add_argument("--fixedDiffs", help="Only variants where differences are fixed between pops", action="store_true")
    ap.add_argument("--nearlyFixedDiff", help="Only variants where frequency diff between any pops is > x", action="store", type=float)
    ap.add_argument("--thinDist", help="Allowed distance between sites for thinning", type=int, action="store", metavar="integer")
    ap.add_argument("--podSize", help="Lines to analyse in each thread simultaneously", type=int, action="store", default=10000)
    ap.add_argument("--noPrecomp", help="Do not use precomputed genotypes shortcut", action="store_true")
    ap.add_argument("--noTest", help="Output all lines (for debugging mostly)", action="store_true")
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


def _die(msg):
    sys.stderr.write("filterGenotypes.py: %s\n" % msg)
    return 1


class _Plan:
    """the option set in the forms pg_filter_text / pg_filter_dev_config take"""

    def __init__(self, cfg, sel_col, sel_ploidy, sel_popmask, contigs, contig_flags):
        self.cfg = cfg
        self.sel_col = np.ascontiguousarray(sel_col, dtype=np.int32)
        self.sel_ploidy = np.ascontiguousarray(sel_ploidy, dtype=np.int32)
        self.sel_popmask = np.ascontiguousarray(sel_popmask, dtype=np.uint32)
        self.contigs = contigs
        self.contig_flags = np.ascontiguousarray(contig_flags if len(contig_flags) else [0], dtype=np.uint8)

    def args(self):
        vp = devroute.vp
        return (C.c_void_p(C.addressof(self.cfg)), vp(self.sel_col), vp(self.sel_ploidy), vp(self.sel_popmask), self.contigs, len(self.contigs),
                vp(self.contig_flags))


def host_filter(plan, text, first_line, n_threads=0):
    """pg_filter_text on a block of data lines: (rows, error code, line index in the block)"""
    L = _lib.lib()
    rows_p, rows_len, n_rows, err_line, err_code = C.c_void_p(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
    buf = text if isinstance(text, bytes) else bytes(text)
    _lib.check(L.pg_filter_text(*plan.args(), buf, len(buf), first_line, n_threads, C.byref(rows_p), C.byref(rows_len), C.byref(n_rows),
                                C.byref(err_line), C.byref(err_code)))
    try:
        rows = C.string_at(rows_p, rows_len.value) if rows_len.value else b""
    finally:
        L.pg_filter_free(rows_p)
    return rows, err_code.value, err_line.value


class _Device(devroute.SlotDevice):
    """the device route (devroute.SlotDevice): one block filtered while the next is submitted; gz_rows: the rows leave the device as
    BGZF members (k_deflate)"""

    def __init__(self, plan, device, gz_rows=False):
        super().__init__(device, "filter")
        taken = C.c_int()
        _lib.check(self.L.pg_filter_dev_config(self.eng._h, *plan.args(), C.byref(taken)))
        self.taken = bool(taken.value)
        _lib.check(self.L.pg_filter_dev_set_output(self.eng._h, int(bool(gz_rows))))

    # submit(block, first_line): devroute.SlotDevice's

    def collect(self, ticket):
        """(rows, members, text, lines): the rows as text or as BGZF members; rows and members None: the block is the host's, `text` its
        text"""
        s = ticket[0]
        rl, nr, hl, bl, nl = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64(), C.c_int64()
        _lib.check(self.L.pg_filter_dev_collect(self.eng._h, s, C.byref(rl), C.byref(nr), C.byref(hl), C.byref(bl), C.byref(nl)))
        if hl.value >= 0:
            return None, None, self.host_text(ticket), nl.value
        if bl.value:
            return None, (devroute.fetch(self.L.pg_filter_dev_rows_bgzf, self.eng._h, bl.value, s).tobytes(), nr.value), None, nl.value
        return devroute.fetch(self.L.pg_filter_dev_rows, self.eng._h, rl.value, s).tobytes(), None, None, nl.value


def filter_main(argv=None):
    t0 = time.perf_counter()
    args = make_parser().parse_args(argv)
    world = dist.world_from_env()
    if world.size > 1 and world.rank != 0:                 # rank 0 does the whole job (sharding is not done)
        return 0

    include = args.include if args.include else []
    exclude = args.exclude if args.exclude else []
    if args.includeFile:
        with open(args.includeFile, "r") as f:
            include += f.read().split()
    if args.excludeFile:
        with open(args.excludeFile, "r") as f:
            exclude += f.read().split()
    if len(include) >= 1:
        include = list(dict.fromkeys(include))
        sys.stderr.write("\nIncluding {} contigs.\n".format(len(include)))
    else:
        include = []
    if len(exclude) >= 1:
        exclude = list(dict.fromkeys(exclude))
        sys.stderr.write("\nExcluding {} contigs.\n".format(len(exclude)))
    else:
        exclude = []

    HWE_P = float(args.HWE[0]) if args.HWE else None
    popDict, popNames = {}, []
    minPopCallsDict = minPopAllelesDict = maxPopAllelesDict = None
    if args.pop:
        for pop in args.pop:
            popNames.append(pop[0])
            popDict[pop[0]] = [] if len(pop) == 1 else pop[1].split(",")
        if args.popsFile:
            with open(args.popsFile, "rt") as pf:
                for line in pf:
                    ind, pop = line.split()
                    if pop in popDict and ind not in popDict[pop]:
                        popDict[pop].append(ind)
        if args.minPopCalls:
            minPopCalls = args.minPopCalls
            if len(minPopCalls) == 1:
                minPopCalls = minPopCalls * len(popNames)
            assert len(minPopCalls) == len(popNames)
            minPopCallsDict = dict(zip(popNames, minPopCalls))
        if args.minPopAlleles:
            minPopAlleles = args.minPopAlleles
            if len(minPopAlleles) == 1:
                minPopAlleles = minPopAlleles * len(popNames)
            assert len(minPopAlleles) == len(popNames)
            minPopAllelesDict = dict(zip(popNames, minPopAlleles))
            if args.maxPopAlleles is None:
                maxPopAllelesDict = dict(zip(popNames, [4] * len(popNames)))
        if args.maxPopAlleles:
            maxPopAlleles = args.maxPopAlleles
            if len(maxPopAlleles) == 1:
                maxPopAlleles = maxPopAlleles * len(popNames)
            assert len(maxPopAlleles) == len(popNames)
            maxPopAllelesDict = dict(zip(popNames, maxPopAlleles))
            if args.minPopAlleles is None:
                minPopAllelesDict = dict(zip(popNames, [0] * len(popNames)))
    popNames = list(popDict.keys())                         # (a name given twice is one population, as in the reference's dict)

    reader = genoio.BlockReader(args.infile)
    head = reader.read_header().decode("utf-8")
    headers = head.split()
    allSamples = headers[2:]
    samples = args.samples.split(",") if args.samples else None
    exSamples = args.excludeSamples.split(",") if args.excludeSamples else []
    if samples is not None:
        for sample in samples:
            assert sample in allSamples, "Sample name not in header: " + sample
    elif args.pop and not args.keepAllSamples:
        samples = [i for j in popDict.values() for i in j]
        assert len(set(samples)) == len(samples), "Populations cannot share the same sample"
    else:
        samples = allSamples
    samples = [s for s in samples if s not in exSamples]
    if args.minCalls:
        assert args.minCalls <= len(samples), "Minimum calls is greater than number of specified samples."
    for popName in popNames:
        popDict[popName] = [s for s in popDict[popName] if s not in exSamples]
        for sample in popDict[popName]:
            assert sample in allSamples, "Sample name not in header: " + sample
    if args.ploidy is not None:
        ploidy = args.ploidy if len(args.ploidy) != 1 else args.ploidy * len(samples)
        assert len(ploidy) == len(samples), "Incorrect number of ploidy values supplied."
        ploidyDict = dict(zip(samples, ploidy))
    elif args.ploidyFile is not None:
        with open(args.ploidyFile, "rt") as pf:
            ploidyDict = dict([[s[0], int(s[1])] for s in [ln.split() for ln in pf]])
    else:
        ploidyDict = dict(zip(samples, [None] * len(samples)))

    out = devroute.open_rows(args.outfile)
    ok = False
    try:
        if args.outputGenoFormat != "bases":
            out.write(("\t".join(headers[0:2] + samples) + "\n").encode("utf-8"))
        else:
            assert args.ploidy is not None or args.ploidyFile, "Ploidy must be specified."
            outSamples = [sample + "_" + letter for sample in samples for letter in string.ascii_uppercase[:ploidyDict[sample]]]
            out.write(("\t".join(headers[0:2] + outSamples) + "\n").encode("utf-8"))
        rc = _run(args, reader, out, headers, samples, popNames, popDict, ploidyDict, include, exclude, HWE_P, minPopCallsDict,
                  minPopAllelesDict, maxPopAllelesDict, world, t0)
        ok = rc == 0
        return rc
    finally:
        devroute.close_rows(out, ok)


def _run(args, reader, out, headers, samples, popNames, popDict, ploidyDict, include, exclude, HWE_P, minPopCallsDict, minPopAllelesDict,
         maxPopAllelesDict, world, t0):
    if len(popNames) > MAXPOP:
        return _die("more than %d populations are not supported" % MAXPOP)
    sel_col = [headers.index(s) for s in samples]
    sel_ploidy = []
    for s in samples:
        if s not in ploidyDict:
            return _die("no ploidy for sample %s (the reference's worker raises KeyError and never ends)" % s)
        sel_ploidy.append(-1 if ploidyDict[s] is None else int(ploidyDict[s]))
    sel_popmask = [sum(1 << k for k, p in enumerate(popNames) if s in popDict[p]) for s in samples]
    cfg = FilterCfg()
    cfg.in_fmt = IN_FMT[args.inputGenoFormat]
    cfg.out_fmt = OUT_FMT[args.outputGenoFormat]
    cfg.freq_order = int(args.alleleOrder == "freq")
    cfg.force_ploidy = int(args.forcePloidy)
    cfg.partial_to_missing = int(args.partialToMissing)
    cfg.no_test = int(args.noTest)
    cfg.n_sel = len(samples)
    cfg.n_pops = len(popNames)
    cfg.n_cols = len(headers)
    cfg.min_calls = args.minCalls
    cfg.min_alleles = args.minAlleles
    cfg.max_alleles = args.maxAlleles
    cfg.min_var = args.minVarCount or 0
    cfg.has_max_het = int(args.maxHet is not None)
    cfg.max_het = args.maxHet if args.maxHet is not None else 0.0
    cfg.min_freq = args.minFreq or 0.0
    cfg.max_freq = args.maxFreq or 0.0
    cfg.hwe = int(bool(HWE_P))
    cfg.fixed = int(args.fixedDiffs)
    cfg.has_pop_calls = int(bool(minPopCallsDict))
    cfg.has_pop_alleles = int(bool(minPopAllelesDict or maxPopAllelesDict))
    cfg.has_nfd = int(args.nearlyFixedDiff is not None)
    cfg.nfd = args.nearlyFixedDiff if args.nearlyFixedDiff is not None else 0.0
    for k, p in enumerate(popNames):
        if minPopCallsDict:
            cfg.pop_calls_min[k] = minPopCallsDict[p]
        if cfg.has_pop_alleles:
            cfg.pop_alleles_min[k] = minPopAllelesDict[p]
            cfg.pop_alleles_max[k] = maxPopAllelesDict[p]
        if not popDict[p]:
            cfg.pop_empty |= 1 << k
        if any(x not in samples for x in popDict[p]):               # (an error only where a line reaches the population filters)
            cfg.pop_missing |= 1 << k
    cfg.universal_newlines = int(args.infile is not None)            # (a file in text mode; stdin keeps its \r inside the line)
    thin = args.thinDist or 0
    pod = abs(args.podSize)
    if pod == 0:
        return _die("--podSize 0: the reference divides the line count by it and stops")
    cfg.thin_dist = thin
    cfg.pod_size = max(pod, 1)
    names = list(dict.fromkeys(include + exclude))
    cfg.n_contigs = len(names)
    cfg.contig_mode = (1 if include else 0) | (2 if exclude else 0)
    contigs = b"".join(n.encode("utf-8") + b"\0" for n in names)
    flags = [(1 if n in include else 0) | (2 if n in exclude else 0) for n in names]
    plan = _Plan(cfg, sel_col, sel_ploidy, sel_popmask, contigs, flags)

    use_device = os.environ.get("PG_FILTER_DEVICE", "1") != "0"
    dev = None
    gz_out = bool(args.outfile and args.outfile.endswith(".gz"))
    if use_device:
        dev_index = args.device if args.device is not None else dist.device_for(world)
        dev = _Device(plan, dev_index, gz_rows=gz_out and os.environ.get("PG_DEFLATE_DEVICE", "1") != "0")
        if not dev.taken:
            dev.close()
            dev = None
    block_bytes = int(os.environ.get("PG_STREAM_BYTES", str(256 << 20)))
    n_threads = int(os.environ.get("PG_HOST_THREADS", "0"))
    info = dict(blocks=0, blocks_on_device=0, blocks_on_host=0, rows=0, text_bytes=0, blocks_inflated_on_device=0)
    t_ctx = time.perf_counter()
    done = [0]                              # data lines of the blocks written so far

    def finish(result):
        """a block's result -> out; returns an exit code or None"""
        rows, members, text, n_lines = result
        first = done[0]
        if members is not None:
            out.write_members(members[0])
            info["blocks_on_device"] += 1
            info["rows"] += members[1]
        else:
            if rows is None:
                rows, err, at = host_filter(plan, text, first, n_threads)
                info["blocks_on_host"] += 1
                if err:
                    out.write(rows)
                    return _die("line %d: %s" % (2 + first + at, ERRORS.get(err, "error %d" % err)))
            else:
                info["blocks_on_device"] += 1
            out.write(rows)
            info["rows"] += rows.count(b"\n")
        done[0] += n_lines
        return None

    # bgzip's members go to the device as they are, unless thinning has to cut the text at pods (then the library's host threads
    # inflate them) or PG_BGZF_DEVICE=0
    spans = (dev is not None and not thin and isinstance(getattr(reader, "f", None), genoio.BgzfFile)
             and os.environ.get("PG_BGZF_DEVICE", "1") != "0")
    first = [0]                             # data lines of the text handed on so far: the line index the device is given

    def submit(block):
        ticket = dev.submit(block, first[0])
        if not devroute.is_span(block):
            first[0] += devroute.count_lines(block)
        return ticket

    def host(text, n_lines):
        first[0] += n_lines
        return finish((None, None, text, n_lines))

    def whole_pods(data, lines_before, eof):
        """--thinDist: whole pods per block, the lines after the last pod boundary wait for the next block (a rest that is the
        host's in one piece has its pods counted there)"""
        if eof:
            return data, b""
        nl = np.flatnonzero(np.frombuffer(data, dtype=np.uint8) == 10)
        take = ((lines_before + len(nl)) // pod) * pod - lines_before
        if take <= 0:
            return b"", data
        at = int(nl[take - 1]) + 1
        return data[:at], data[at:]

    blocks = devroute.read_ahead(devroute.blocks(reader, block_bytes, dev.pinned() if spans else None, info), "pg-filter-read")
    rc = devroute.run_blocks(blocks, dev, info, finish, host, submit=submit, universal=bool(cfg.universal_newlines),
                             cut=whole_pods if thin else None)
    if rc:
        return rc
    if dev is not None:
        info["device_blocks"], info["device_host_blocks"] = dev.stats()
        dev.close()
    info["total_s"] = time.perf_counter() - t0
    info["filter_s"] = time.perf_counter() - t_ctx
    devroute.report(last_info, info, "filter")
    return 0


def main():
    return filter_main()
