"""Drop-in for the reference's sfs.py: 1-D to 4-D joint site-frequency spectra from genotypes or from a freq.py table, counted on
the device (csrc/pg_sfs.hip: k_sfs_rows / k_sfs_base / k_sfs_target, read out by k_sfs_compact).

The host side here: the populations and spectrum groups of the command line (sfs.py:284-415), the regions (genomics.Intervals), the
per-block membership lists the kernels evaluate, the parser of the table inputs, and the reference's sparse output: SparseFS.asChains
walks nested dicts in insertion order, so at every nesting level the keys appear in the order in which their prefix was first touched --
reproduced from the lowest line ordinal per cell (`first`).

Divergences (README.md): --subsample / --subsampleIndividuals, --header and non-default --scafCol / --posCol / --firstSampleCol are
rejected; negative counts in a table are an error; --verbose prints no per-site lines."""
import argparse
import gzip
import itertools
import os
import sys

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
MAX_IN = 32                 # SFS_MAX_IN of pg_sfs.hip


class SfsError(SystemExit):
    """a command line or an input the drop-in does not take: one line on stderr, exit status 2"""

    def __init__(self, msg):
        sys.stderr.write("sfs.py: " + msg + "\n")
        super().__init__(2)


# ---- command line -> populations and groups ---------------------------------------------------------------
def fs_groups(inPopNames, FSpops=None, doPairs=False, doTrios=False, doQuartets=False):
    """the spectra to make, as lists of population names (sfs.py:410-415)"""
    if FSpops:
        return [list(g) for g in FSpops]
    groups = [[p] for p in inPopNames]
    for on, k in ((doPairs, 2), (doTrios, 3), (doQuartets, 4)):
        if on:
            groups += [list(c) for c in itertools.combinations(inPopNames, k)]
    return groups


def ingroup(popNames, polarized=False, outgroup=None):
    """(ingroup names, outgroup or None): the outgroup -- --outgroup, or the last population with --polarized -- leaves the ingroup
    list wherever it stands (sfs.py:369-376)"""
    if polarized or outgroup:
        out = outgroup if outgroup else popNames[-1]
        return [p for p in popNames if p != out], out
    return list(popNames), None


REJECTED = {
    "subsample": "--subsample is not supported: the reference draws per site from NumPy's global random stream, which is not reproduced",
    "subsampleIndividuals": "--subsampleIndividuals is not supported: the reference draws per site from Python's global random stream, "
                            "which is not reproduced",
    "header": "--header is not supported: the input must carry its header line",
    "scafCol": "--scafCol other than 0 is not supported",
    "posCol": "--posCol other than 1 is not supported",
    "firstSampleCol": "--firstSampleCol other than 2 is not supported",
}


def check_supported(args):
    """None, or the message for the first flag of the reference's command line that the drop-in rejects"""
    if args.subsample is not None:
        return REJECTED["subsample"]
    if args.subsampleIndividuals:
        return REJECTED["subsampleIndividuals"]
    if args.header:
        return REJECTED["header"]
    for name, default in (("scafCol", 0), ("posCol", 1), ("firstSampleCol", 2)):
        if getattr(args, name) != default:
            return REJECTED[name]
    return None


def make_parser():
    ap = argparse.ArgumentParser(prog="sfs.py")
    ap.add_argument("-i", "--inputFile", help="Input file")
    ap.add_argument("--inputType", choices=("genotypes", "baseCounts", "targetCounts"), default="targetCounts")
    ap.add_argument("--scafCol", type=int, default=0)
    ap.add_argument("--posCol", type=int, default=1)
    ap.add_argument("--firstSampleCol", type=int, default=2)
    ap.add_argument("--header")
    ap.add_argument("--genoFormat", choices=("phased", "diplo", "alleles"), default="phased")
    ap.add_argument("-p", "--pop", action="append", nargs="+", metavar=("popName", "[samples]"))
    ap.add_argument("--popsFile")
    ap.add_argument("--ploidy", type=int, nargs="+")
    ap.add_argument("--ploidyFile")
    ap.add_argument("--FSpops", action="append", type=str, nargs="+")
    ap.add_argument("--doPairs", action="store_true")
    ap.add_argument("--doTrios", action="store_true")
    ap.add_argument("--doQuartets", action="store_true")
    ap.add_argument("--subsample", nargs="+", type=int)
    ap.add_argument("--subsampleIndividuals", action="store_true")
    ap.add_argument("--pref", default="")
    ap.add_argument("--suff", default=".sfs")
    ap.add_argument("--pipe", action="store_true")
    ap.add_argument("--polarized", action="store_true")
    ap.add_argument("--outgroup")
    ap.add_argument("--include", nargs="+")
    ap.add_argument("--includeFile")
    ap.add_argument("--exclude", nargs="+")
    ap.add_argument("--excludeFile")
    ap.add_argument("--regions", nargs="+")
    ap.add_argument("--regionsFile")
    ap.add_argument("-R", "--report", default=100000, help="accepted for compatibility")
    ap.add_argument("--verbose", action="store_true", help="accepted; the per-site lines on stderr are not written")
    ap.add_argument("--seed", type=int, default=42, help="accepted for compatibility")
    ap.add_argument("--device", type=int, default=None, help="GPU index (MI355X engine)")
    return ap


# ---- regions (genomics.parseRegionText / Intervals, genomics.py:2323-2378) ---------------------------------------
def parse_region_text(text):
    sp = text.split(":")
    ori = "+" if len(sp) < 3 or sp[2] == "" else sp[2]
    if ori not in "+-":
        raise ValueError("Incorrect region specification")
    try:
        ft = [int(x) for x in sp[1].split("-")]
        if len(ft) == 1:
            ft.append(None)
        if ft[1] is not None and ft[0] > ft[1]:
            ft = ft[::-1]
        return sp[0], ft[0], ft[1]
    except (ValueError, IndexError):
        return sp[0], None, None


def intervals_from(regions=None, regions_file=None):
    """(chroms, starts, ends) with both ends inclusive.  A region without coordinates makes the reference raise (np.inf into an
    integer array): an error here too."""
    if regions:
        tuples = [parse_region_text(r) for r in regions]
    else:
        with open(regions_file, "rt") as f:
            tuples = [tuple(ln.split()) for ln in f]
    chroms, starts, ends = [], [], []
    for t in tuples:
        if len(t) < 1:
            raise ValueError("a region without a name")
        start = t[1] if len(t) > 1 and t[1] is not None else None
        end = t[2] if len(t) > 2 and t[2] is not None else start
        if end is None:
            raise OverflowError("region %r has no coordinates: cannot convert float infinity to integer" % (t[0],))
        chroms.append(t[0])
        starts.append(int(start))
        ends.append(int(end))
    for v in starts + ends:
        if not I64_MIN <= v <= I64_MAX:
            raise OverflowError("region coordinate %d does not fit 64 bits" % v)
    return chroms, np.array(starts, dtype=np.int64), np.array(ends, dtype=np.int64)


class Membership:
    """which sites count, and for which intervals: --include / --exclude by scaffold name, then the regions.  lists(run_names) gives
    the per-run (start, end, interval id) lists the kernels evaluate per site; None when every site counts once."""

    def __init__(self, include=None, exclude=None, intervals=None):
        self.include = set(include) if include else None
        self.exclude = set(exclude) if exclude else None
        self.n_intervals = 1
        self.by_chrom = None
        if intervals is not None:
            chroms, starts, ends = intervals
            self.n_intervals = len(chroms)
            self.by_chrom = {}
            for k, ch in enumerate(chroms):
                self.by_chrom.setdefault(ch, []).append(k)
            self.by_chrom = {ch: (starts[ks], ends[ks], np.array(ks, dtype=np.int32)) for ch, ks in self.by_chrom.items()}
        self.active = bool(self.include or self.exclude or self.by_chrom is not None)

    def lists(self, run_names):
        if not self.active:
            return None
        off, st, en, ids = [0], [], [], []
        for nm in run_names:
            if (self.include and nm not in self.include) or (self.exclude and nm in self.exclude):
                pass
            elif self.by_chrom is None:
                st.append(np.array([I64_MIN], dtype=np.int64))
                en.append(np.array([I64_MAX], dtype=np.int64))
                ids.append(np.zeros(1, dtype=np.int32))
            elif nm in self.by_chrom:
                s, e, k = self.by_chrom[nm]
                st.append(s)
                en.append(e)
                ids.append(k)
            off.append(sum(len(x) for x in st))
        cat = lambda xs, dt: np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros(0, dtype=dt), dtype=dt)      # noqa: E731
        return np.array(off, dtype=np.int32), cat(st, np.int64), cat(en, np.int64), cat(ids, np.int32)


# ---- the sparse output ---------------------------------------------------------------------------------------
def merge_partials(parts):
    """parts: (digits int64 [n][nd], first uint64 [n], counts uint64 [n][NI]) of one spectrum, read out at different times (the
    extents of a table input grow): one such triple with every cell once -- counts summed, first the minimum"""
    parts = [p for p in parts if len(p[0])]
    if not parts:
        return None
    if len(parts) == 1:
        return parts[0]
    digits = np.concatenate([p[0] for p in parts])
    first = np.concatenate([p[1] for p in parts])
    counts = np.concatenate([p[2] for p in parts])
    uniq, inv = np.unique(digits, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    f = np.full(len(uniq), np.iinfo(np.uint64).max, dtype=np.uint64)
    np.minimum.at(f, inv, first)
    c = np.zeros((len(uniq), counts.shape[1]), dtype=np.uint64)
    np.add.at(c, inv, counts)
    return uniq, f, c


def order_rows(digits, first):
    """the order SparseFS.asChains gives the cells: at every level the keys in order of the first line that touched their prefix"""
    n, nd = digits.shape
    keys = []
    for d in range(nd - 1):
        _, inv = np.unique(digits[:, :d + 1], axis=0, return_inverse=True)
        inv = inv.reshape(-1)
        m = np.full(int(inv.max()) + 1 if n else 0, np.iinfo(np.uint64).max, dtype=np.uint64)
        np.minimum.at(m, inv, first)
        keys.append(m[inv])
    keys.append(first)
    return np.lexsort(keys[::-1])


def spectrum_text(part):
    """the file sfs.py writes for one spectrum (sfs.py:499-505): a row per touched cell, tab separated; "\\n" alone when none"""
    if part is None or len(part[0]) == 0:
        return "\n"
    digits, first, counts = part
    order = order_rows(digits, first)
    table = np.concatenate([digits[order].astype(np.int64), counts[order].astype(np.int64)], axis=1)
    return "\n".join("\t".join(map(str, row)) for row in table.tolist()) + "\n"


# ---- the device session ----------------------------------------------------------------------------------------
class Accumulator:
    """the spectra of one run on an engine: begins a device session when the extents are known, restarts it with larger extents
    when a table block needs them (the touched cells read so far become a host-side partial), and merges at the end"""

    def __init__(self, eng, groups_idx, n_intervals):
        self.eng, self.groups, self.NI = eng, groups_idx, n_intervals
        self.ext = None
        self.parts = [[] for _ in groups_idx]
        self.restarts = 0
        self.on_lds = None

    def _begin(self, ext):
        self.cells, self.on_lds = self.eng.sfs_begin(ext, self.groups, self.NI)
        self.ext = list(ext)

    def ensure(self, need):
        """extents of at least `need` (max count + 1 per ingroup population)"""
        need = [int(x) for x in need]
        if self.ext is None:
            self._begin(need)
            return
        if all(n <= e for n, e in zip(need, self.ext)):
            return
        old = self.ext
        self.flush()
        grown = [max(n, 2 * e) if n > e else e for n, e in zip(need, old)]
        exact = [max(n, e) for n, e in zip(need, old)]
        self.restarts += 1
        try:
            self._begin(grown)
        except Exception:
            self._begin(exact)                       # doubled extents beyond the scratch budget: what is needed, no more

    def flush(self):
        if self.ext is None:
            return
        cell, first, counts = self.eng.sfs_read()
        self.eng.sfs_end()
        bases = np.concatenate([[0], np.cumsum(self.cells)]).astype(np.int64)
        g_of = np.searchsorted(bases, cell, side="right") - 1
        for g, pops in enumerate(self.groups):
            sel = g_of == g
            if not sel.any():
                continue
            local = cell[sel] - bases[g]
            digits = np.stack(np.unravel_index(local, tuple(self.ext[p] for p in pops)), axis=1).astype(np.int64)
            self.parts[g].append((digits, first[sel], counts[sel]))
        self.ext = None

    def finish(self):
        self.flush()
        return [merge_partials(p) for p in self.parts]


# ---- table inputs ----------------------------------------------------------------------------------------------
def open_table(path):
    if not path:
        return sys.stdin
    return gzip.open(path, "rt") if path.endswith(".gz") else open(path, "rt")


def table_blocks(f, names, in_names, out_name, base_counts, block_bytes):
    """per block of lines: (scaffold run names, run index per row, positions, values).  values: int32 [n][n_in] target counts, or
    int32 [n][n_in (+1 with an outgroup)][4] base counts (cells `a,c,g,t` through float then int, sfs.py:466)."""
    col = {nm: k for k, nm in enumerate(names)}                 # (dict(zip(names, GTs)): the last column of a repeated name)
    want = list(in_names) + ([out_name] if out_name else [])
    for nm in want:
        if nm not in col:
            raise KeyError("population %r is not a column of the input" % nm)
    idx = [col[nm] + 2 for nm in want]
    while True:
        lines = f.readlines(block_bytes)
        if not lines:
            return
        run_names, row_run, pos, vals = [], [], [], []
        for ln in lines:
            if ln[0] == "#":
                continue
            fld = ln.split()
            if not run_names or fld[0] != run_names[-1]:
                run_names.append(fld[0])
            row_run.append(len(run_names) - 1)
            pos.append(int(fld[1]))
            if base_counts:
                cells = [[int(float(x)) for x in fld[k].split(",")] for k in idx]
                if any(len(c) != 4 for c in cells):
                    raise ValueError("a baseCounts cell does not hold four counts: line %r" % ln[:60])
                vals.append(cells)
            else:
                vals.append([int(fld[k]) for k in idx])
        if not vals:
            continue
        v = np.array(vals, dtype=np.int64)
        if v.min() < 0:
            raise ValueError("negative counts in the input table")
        if v.max() >= 2 ** 31:
            raise ValueError("counts beyond 2^31 in the input table")
        yield run_names, np.array(row_run, dtype=np.int32), np.array(pos, dtype=np.int64), np.ascontiguousarray(v, dtype=np.int32)


# ---- the driver ------------------------------------------------------------------------------------------------
def main(argv=None):
    import time as _time
    from . import dist, genoio
    from .cli import _SiteIngest
    from .engine import Engine
    from .samples import HapLayout, SampleData
    t_begin = _time.perf_counter()
    args = make_parser().parse_args(argv)
    msg = check_supported(args)
    if msg:
        raise SfsError(msg)
    include = list(args.include or [])
    exclude = list(args.exclude or [])
    if args.includeFile:
        with open(args.includeFile, "rt") as f:
            include += f.read().split()
    if args.excludeFile:
        with open(args.excludeFile, "rt") as f:
            exclude += f.read().split()
    intervals = None
    if args.regions or args.regionsFile:
        try:
            intervals = intervals_from(args.regions, None if args.regions else args.regionsFile)
        except (ValueError, OverflowError) as exc:
            raise SfsError("bad regions: %s" % exc)
        sys.stderr.write("Recording SFS for {} intervals\n".format(len(intervals[0])))
    member = Membership(include, exclude, intervals)
    genotypes = args.inputType == "genotypes"

    if genotypes:
        reader = genoio.open_input(args.inputFile)
        headerInds = reader.read_header().decode("utf-8", "replace").split()[2:]
        popNames, popDict = [], {}
        if args.pop or args.FSpops:
            for pop in args.pop or []:
                popNames.append(pop[0])
                popDict[pop[0]] = [] if len(pop) == 1 else pop[1].split(",")
            for pop in [p for pops in args.FSpops or [] for p in pops]:
                if pop not in popNames:
                    popNames.append(pop)
                    popDict[pop] = []
            if args.popsFile:
                with open(args.popsFile, "rt") as pf:
                    for line in pf:
                        ind, pop = line.split()
                        if pop in popDict and ind not in popDict[pop]:
                            popDict[pop].append(ind)
        else:
            popNames, popDict = ["all"], {"all": list(headerInds)}
        for p in popNames:
            assert len(popDict[p]) >= 1, "Population {} has no samples".format(p)
        allSamples = [s for p in popDict for s in popDict[p]]
        if args.ploidy is not None:
            ploidy = args.ploidy if len(args.ploidy) != 1 else args.ploidy * len(allSamples)
            assert len(ploidy) == len(allSamples), "Incorrect number of ploidy values supplied."
            ploidyDict = dict(zip(allSamples, ploidy))
        elif args.ploidyFile is not None:
            with open(args.ploidyFile, "rt") as pf:
                ploidyDict = dict([[s[0], int(s[1])] for s in [ln.split() for ln in pf]])
        else:
            ploidyDict = dict(zip(allSamples, [2] * len(allSamples)))
        names = headerInds
    else:
        table = open_table(args.inputFile)
        names = table.readline().split()[2:]
        if args.pop or args.FSpops:
            popNames = [pop[0] for pop in args.pop or []]
            for pop in [p for pops in args.FSpops or [] for p in pops]:
                if pop not in popNames:
                    popNames.append(pop)
        else:
            popNames = list(names)
    sys.stderr.write("\nPopulations:\n" + " ".join(popNames) + "\n")
    if args.inputType != "targetCounts" and not (args.polarized or args.outgroup):
        sys.stderr.write("\nNo outgroup provided. Minor allele frequency will be used.\n")
    if args.inputType in ("genotypes", "baseCounts"):
        inPopNames, outgroup = ingroup(popNames, args.polarized, args.outgroup)
        if outgroup:
            sys.stderr.write("\nFrequencies will be polarized assuming outgroup is {}\n".format(outgroup))
    else:
        inPopNames, outgroup = list(popNames), None
    groups = fs_groups(inPopNames, args.FSpops, args.doPairs, args.doTrios, args.doQuartets)
    for g in groups:
        if not 1 <= len(g) <= 4:
            raise SfsError("a spectrum takes one to four populations, not %d (%s)" % (len(g), " ".join(g)))
        for p in g:
            if p not in inPopNames:
                raise KeyError(p)                        # (popTargetCountsDict[pop], sfs.py:494)
    if not 1 <= len(inPopNames) <= MAX_IN:
        raise SfsError("1 to %d ingroup populations are supported, not %d" % (MAX_IN, len(inPopNames)))
    groups_idx = [[inPopNames.index(p) for p in g] for g in groups]

    # Multi-GPU: rank 0 does the job, the others take part in the closing exchanges only (the unsharded branch of freq.py)
    world = dist.world_from_env()
    eng = Engine(args.device if args.device is not None else dist.device_for(world))
    layout = None
    if genotypes:
        sampleData = SampleData(popNames=popNames, popInds=[popDict[p] for p in popNames], ploidyDict=ploidyDict)
        layout = HapLayout(sampleData, names, "pairs" if args.genoFormat == "alleles" else args.genoFormat)
        eng.set_layout(layout)
    comm = dist.make_comm(eng, world)
    if world.size > 1 and world.rank > 0:
        dist.gather_bytes(comm, b"")
        comm.close()
        return 0
    acc = Accumulator(eng, groups_idx, member.n_intervals)
    stats = {"device_tokenizer": 0, "bgzf_blocks_inflated_on_device": 0, "host_tokenized_blocks": 0, "blocks": 0, "sites": 0,
             "wait_for_block_s": 0.0, "tokenize_s": 0.0, "parse_s": 0.0, "accumulate_s": 0.0, "kernel_ms": 0.0, "read_s": 0.0, "write_s": 0.0}

    def lap(key, t0):
        t1 = _time.perf_counter()
        stats[key] += t1 - t0
        return t1

    ordinal = 0
    if genotypes:
        pop_of = {p: k for k, p in enumerate(popNames)}
        in_pops = [pop_of[p] for p in inPopNames]
        out_pop = pop_of[outgroup] if outgroup else -1
        nHap = [sum(ploidyDict[s] for s in popDict[p]) for p in inPopNames]
        acc.ensure([n + 1 for n in nHap])
        ing = _SiteIngest(reader, eng, layout, False)
        stats["device_tokenizer"] = int(ing.on_device)
        cur, lists = None, None
        for data, run_of_row, a, b in ing.blocks(stats, lap):
            if data is not cur:
                cur, lists = data, member.lists(data.run_names)
            t0 = _time.perf_counter()
            lo_, hi_ = (a, b) if data.gt is None else (0, b - a)     # tokenised on the device: the block's rows are resident
            if data.gt is not None:
                ing.load(data.gt[a:b])
            rows = None
            if lists is not None:
                rows = lists + (np.ascontiguousarray(run_of_row[a:b], dtype=np.int32), np.ascontiguousarray(data.pos[a:b], dtype=np.int64))
            stats["kernel_ms"] += eng.sfs_add_sites(lo_, hi_, ordinal + a, in_pops, out_pop, rows)
            lap("accumulate_s", t0)
            if b == data.n_sites:
                ordinal += data.n_sites
        reader.close()
    else:
        base_counts = args.inputType == "baseCounts"
        block_bytes = int(os.environ.get("PG_STREAM_BYTES", 1 << 30))
        n_in = len(inPopNames)
        t0 = _time.perf_counter()
        blocks = table_blocks(table, names, inPopNames, outgroup, base_counts, block_bytes)
        while True:
            try:
                run_names, row_run, pos, vals = next(blocks)
            except StopIteration:
                break
            except (ValueError, KeyError, IndexError) as exc:      # negative counts, a missing column, a line that does not parse
                raise SfsError("bad input table: %s" % exc)
            t0 = lap("parse_s", t0)
            stats["blocks"] += 1
            stats["sites"] += len(pos)
            lists = member.lists(run_names)
            rows = lists + (row_run, pos) if lists is not None else None
            # the extents a block needs: its largest count per ingroup population (base counts: over the four bases, a bound)
            acc.ensure(vals[:, :n_in].reshape(len(vals), n_in, -1).max(axis=(0, 2)) + 1)
            if base_counts:
                stats["kernel_ms"] += eng.sfs_add_base_counts(vals, ordinal, list(range(n_in)), n_in if outgroup else -1, rows)
            else:
                stats["kernel_ms"] += eng.sfs_add_target_counts(vals, ordinal, rows)
            ordinal += len(pos)
            t0 = lap("accumulate_s", t0)
        if table is not sys.stdin:
            table.close()
        if acc.ext is None and not any(acc.parts):
            acc.ensure([1] * n_in)                       # an input without a site: empty spectra
    t0 = _time.perf_counter()
    parts = acc.finish()
    stats["extent_restarts"] = acc.restarts
    t0 = lap("read_s", t0)
    texts = [spectrum_text(p) for p in parts]
    if args.pipe:
        for text in texts:
            sys.stdout.write(text)
        sys.stdout.flush()
    else:
        for g, text in zip(groups, texts):
            with open(args.pref + "_".join(g) + args.suff, "w") as out:
                out.write(text)
    lap("write_s", t0)
    if os.environ.get("PG_TIMING"):
        import json
        stats["total_s"] = _time.perf_counter() - t_begin
        sys.stderr.write("PG_TIMING " + json.dumps(dict({k: (round(v, 4) if isinstance(v, float) else v) for k, v in stats.items()}, rank=world.rank)) + "\n")
    if world.size > 1:
        dist.gather_bytes(comm, b"")
        comm.close()
    eng.close()
    return 0
