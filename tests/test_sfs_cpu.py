"""Host side of the sfs.py drop-in (genomics_general_amd/sfs.py), no GPU: the spectrum groups of a command line, the reference's
first-appearance row order and text against a literal nested-dict model, the merge of partial read-outs, the rejected flags, the
regions, and the target allele's tie rule (the device function, called on the host) against np.argsort."""
import ctypes as C
import itertools

import numpy as np
import pytest

from genomics_general_amd import _lib, sfs

U64_MAX = np.iinfo(np.uint64).max


# ---- groups ------------------------------------------------------------------------------------------------
def test_groups_of_singles_pairs_trios_quartets_in_the_reference_order():
    pops = ["a", "b", "c", "d"]
    assert sfs.fs_groups(pops) == [["a"], ["b"], ["c"], ["d"]]
    g = sfs.fs_groups(pops, doPairs=True, doTrios=True, doQuartets=True)
    want = [[p] for p in pops] + [list(c) for k in (2, 3, 4) for c in itertools.combinations(pops, k)]
    assert g == want and len(g) == 4 + 6 + 4 + 1
    assert sfs.fs_groups(pops, doQuartets=True)[-1] == pops
    assert sfs.fs_groups(pops, doTrios=True)[4:] == [["a", "b", "c"], ["a", "b", "d"], ["a", "c", "d"], ["b", "c", "d"]]


def test_explicit_fspops_replace_every_default_group():
    assert sfs.fs_groups(["a", "b", "c"], FSpops=[["c", "a"], ["b"]], doPairs=True) == [["c", "a"], ["b"]]


def test_outgroup_leaves_the_ingroup_wherever_it_stands():
    pops = ["a", "b", "c", "d"]
    assert sfs.ingroup(pops) == (pops, None)
    assert sfs.ingroup(pops, polarized=True) == (["a", "b", "c"], "d")
    assert sfs.ingroup(pops, outgroup="b") == (["a", "c", "d"], "b")
    assert sfs.ingroup(pops, polarized=True, outgroup="a") == (["b", "c", "d"], "a")
    inn, out = sfs.ingroup(pops, outgroup="b")
    assert sfs.fs_groups(inn, doPairs=True) == [["a"], ["c"], ["d"], ["a", "c"], ["a", "d"], ["c", "d"]]
    assert sfs.fs_groups(inn, doQuartets=True) == [["a"], ["c"], ["d"]]          # three ingroup populations: no quartet


# ---- order and text ------------------------------------------------------------------------------------------
def dict_model_text(nd, n_intervals, events):
    """the reference's SparseFS as plain nested dicts: events = (key tuple, addValue vector) in input order"""
    root = {}
    for key, add in events:
        d = root
        for k in key[:-1]:
            d = d.setdefault(k, {})
        if key[-1] not in d:
            d[key[-1]] = [0] * n_intervals
        d[key[-1]] = [x + y for x, y in zip(d[key[-1]], add)]

    def chains(d, depth, chain):
        for k in d:
            if depth == nd - 1:
                yield chain + [k] + d[k]
            else:
                yield from chains(d[k], depth + 1, chain + [k])
    return "\n".join("\t".join(str(x) for x in row) for row in chains(root, 0, [])) + "\n"


def cells_of(nd, n_intervals, events):
    """what the device hands back for those events: per touched cell its first event index and summed counts, shuffled"""
    first, counts = {}, {}
    for i, (key, add) in enumerate(events):
        first.setdefault(key, i)
        counts[key] = [x + y for x, y in zip(counts.get(key, [0] * n_intervals), add)]
    keys = list(first)
    return (np.array(keys, dtype=np.int64).reshape(len(keys), nd), np.array([first[k] for k in keys], dtype=np.uint64),
            np.array([counts[k] for k in keys], dtype=np.uint64).reshape(len(keys), n_intervals))


@pytest.mark.parametrize("nd", [1, 2, 3, 4])
@pytest.mark.parametrize("n_intervals", [1, 3])
def test_rows_come_in_first_appearance_order_at_every_level(nd, n_intervals):
    rng = np.random.default_rng(100 * nd + n_intervals)
    events = []
    for _ in range(400):
        key = tuple(int(x) for x in rng.integers(0, 4, size=nd))
        add = [int(x) for x in rng.integers(0, 2, size=n_intervals)]
        if sum(add) == 0:                                       # (a site in no interval is skipped)
            add[int(rng.integers(0, n_intervals))] = 1
        events.append((key, add))
    digits, first, counts = cells_of(nd, n_intervals, events)
    perm = rng.permutation(len(digits))                         # the read-out's order means nothing
    got = sfs.spectrum_text((digits[perm], first[perm], counts[perm]))
    assert got == dict_model_text(nd, n_intervals, events)


def test_rows_touched_by_one_interval_carry_zeros_for_the_others():
    events = [((2, 1), [0, 1, 0]), ((0, 0), [1, 1, 0]), ((2, 1), [0, 1, 0]), ((2, 0), [0, 0, 1])]
    want = "2\t1\t0\t2\t0\n2\t0\t0\t0\t1\n0\t0\t1\t1\t0\n"
    assert dict_model_text(2, 3, events) == want and sfs.spectrum_text(cells_of(2, 3, events)) == want


def test_an_empty_spectrum_is_one_newline():
    assert sfs.spectrum_text(None) == "\n"
    assert sfs.spectrum_text((np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.uint64), np.zeros((0, 1), dtype=np.uint64))) == "\n"
    assert dict_model_text(2, 1, []) == "\n"


def test_a_late_cell_under_an_early_prefix_stays_with_its_prefix():
    events = [((1, 0), [1]), ((0, 0), [1]), ((1, 5), [1]), ((0, 2), [1]), ((1, 0), [1])]
    assert sfs.spectrum_text(cells_of(2, 1, events)) == "1\t0\t2\n1\t5\t1\n0\t0\t1\n0\t2\t1\n"


# ---- merge ---------------------------------------------------------------------------------------------------
def test_partials_merge_by_summing_counts_and_keeping_the_lowest_first():
    rng = np.random.default_rng(5)
    events = [(tuple(int(x) for x in rng.integers(0, 5, size=2)), [1, int(rng.integers(0, 2))]) for _ in range(300)]
    cuts = [0, 70, 71, 200, 300]
    parts = []
    for a, b in zip(cuts[:-1], cuts[1:]):
        d, f, c = cells_of(2, 2, events[a:b])
        parts.append((d, f + np.uint64(a), c))
    parts.insert(2, (np.zeros((0, 2), dtype=np.int64), np.zeros(0, dtype=np.uint64), np.zeros((0, 2), dtype=np.uint64)))
    merged = sfs.merge_partials(parts)
    d, f, c = cells_of(2, 2, events)
    want = {tuple(k): (int(ff), [int(x) for x in cc]) for k, ff, cc in zip(d.tolist(), f, c)}
    got = {tuple(k): (int(ff), [int(x) for x in cc]) for k, ff, cc in zip(merged[0].tolist(), merged[1], merged[2])}
    assert got == want and len(merged[0]) == len(want)
    assert sfs.spectrum_text(merged) == dict_model_text(2, 2, events)
    assert sfs.merge_partials([]) is None and sfs.merge_partials(parts[2:3]) is None


class ModelEngine:
    """the device session as dense NumPy tables (target counts only)"""

    def sfs_begin(self, ext, groups, n_intervals=1):
        self.ext, self.groups = list(ext), groups
        self.count = [np.zeros([ext[p] for p in g] + [n_intervals], dtype=np.uint64) for g in groups]
        self.first = [np.full([ext[p] for p in g], U64_MAX, dtype=np.uint64) for g in groups]
        return np.array([f.size for f in self.first], dtype=np.int64), np.ones(len(groups), dtype=bool)

    def sfs_add_target_counts(self, tc, ord0, members=None):
        for i, row in enumerate(tc):
            assert all(0 <= row[p] < self.ext[p] for p in range(len(self.ext)))
            for g, pops in enumerate(self.groups):
                key = tuple(int(row[p]) for p in pops)
                self.count[g][key][0] += np.uint64(1)
                self.first[g][key] = min(self.first[g][key], np.uint64(ord0 + i))
        return 0.0

    def sfs_read(self):
        cell, first, counts, base = [], [], [], 0
        for f, c in zip(self.first, self.count):
            at = np.flatnonzero(f.reshape(-1) != U64_MAX)
            cell.append(at + base)
            first.append(f.reshape(-1)[at])
            counts.append(c.reshape(f.size, -1)[at])
            base += f.size
        return np.concatenate(cell).astype(np.int64), np.concatenate(first), np.concatenate(counts)

    def sfs_end(self):
        self.count = self.first = None


def test_growing_extents_restart_the_session_and_the_partials_merge():
    rng = np.random.default_rng(11)
    blocks = [rng.integers(0, hi, size=(40, 3)) for hi in (3, 3, 9, 5, 20)]
    groups = [[0], [2], [0, 1], [2, 0, 1]]
    acc = sfs.Accumulator(ModelEngine(), groups, 1)
    ordinal = 0
    for b in blocks:
        acc.ensure(b.max(axis=0) + 1)
        acc.eng.sfs_add_target_counts(b, ordinal)
        ordinal += len(b)
    parts = acc.finish()
    assert acc.restarts >= 2
    rows = np.concatenate(blocks)
    for g, part in zip(groups, parts):
        events = [(tuple(int(r[p]) for p in g), [1]) for r in rows]
        assert sfs.spectrum_text(part) == dict_model_text(len(g), 1, events)


# ---- rejected flags ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flags,word", [(["--subsample", "4"], "--subsample "), (["--subsampleIndividuals"], "--subsampleIndividuals"),
                                        (["--header", "a b c"], "--header"), (["--scafCol", "1"], "--scafCol"), (["--posCol", "0"], "--posCol"),
                                        (["--firstSampleCol", "3"], "--firstSampleCol")])
def test_unsupported_flags_are_rejected_by_name(flags, word, capsys):
    args = sfs.make_parser().parse_args(["-i", "x.geno", "--inputType", "genotypes"] + flags)
    msg = sfs.check_supported(args)
    assert msg and word.strip() in msg and "not supported" in msg
    with pytest.raises(SystemExit) as exc:
        sfs.main(["-i", "x.geno", "--inputType", "genotypes"] + flags)          # (rejected before any file or device is opened)
    assert exc.value.code not in (0, None)
    assert word.strip() in capsys.readouterr().err


def test_inert_flags_pass():
    args = sfs.make_parser().parse_args(["-i", "x", "-R", "5", "--verbose", "--seed", "7", "--scafCol", "0", "--posCol", "1", "--firstSampleCol", "2"])
    assert sfs.check_supported(args) is None


# ---- regions -------------------------------------------------------------------------------------------------
def test_regions_are_inclusive_may_be_reversed_and_need_coordinates(tmp_path):
    ch, s, e = sfs.intervals_from(["c1:5-9", "c1:9-5", "c2:7", "c1:3000000000-3000000001:+"])
    assert ch == ["c1", "c1", "c2", "c1"] and s.tolist() == [5, 5, 7, 3000000000] and e.tolist() == [9, 9, 7, 3000000001]
    for bad in (["c1"], ["c1:5-9", "c2:"], ["c1:a-b"]):
        with pytest.raises(OverflowError):
            sfs.intervals_from(bad)
    p = tmp_path / "r.txt"
    p.write_text("c1 5 9 name\nc2 7\n")
    ch, s, e = sfs.intervals_from(None, str(p))
    assert ch == ["c1", "c2"] and s.tolist() == [5, 7] and e.tolist() == [9, 7]
    p.write_text("c1 5 9\nc2\n")
    with pytest.raises(OverflowError):
        sfs.intervals_from(None, str(p))


def test_membership_lists_follow_the_runs_of_a_block():
    m = sfs.Membership(None, None, None)
    assert m.lists(["a", "b"]) is None and m.n_intervals == 1
    m = sfs.Membership(["a"], ["c"], None)
    off, st, en, ids = m.lists(["a", "b", "a", "c"])
    assert off.tolist() == [0, 1, 1, 2, 2] and ids.tolist() == [0, 0] and st[0] < -2 ** 62 and en[0] > 2 ** 62
    m = sfs.Membership(None, ["b"], sfs.intervals_from(["a:1-5", "b:1-5", "a:4-8", "c:2-3"]))
    off, st, en, ids = m.lists(["b", "a", "x", "c", "a"])
    assert m.n_intervals == 4 and off.tolist() == [0, 0, 2, 2, 3, 5]
    assert ids.tolist() == [0, 2, 3, 0, 2] and st.tolist() == [1, 4, 2, 1, 4] and en.tolist() == [5, 8, 3, 5, 8]


# ---- the tie rule ----------------------------------------------------------------------------------------------
def target_base(tot, out=None):
    L = _lib.lib()
    b = C.c_int(-9)
    t = np.ascontiguousarray(tot, dtype=np.int64)
    o = np.ascontiguousarray(out, dtype=np.int64) if out is not None else None
    _lib.check(L.pg_sfs_target_base(t, C.c_void_p(o.ctypes.data) if o is not None else None, C.byref(b)))
    return b.value


def test_minor_allele_follows_numpys_argsort_on_every_tie_pattern():
    """sfs.py:83: totalBaseCounts.argsort()[-2] over all four totals, zeros included; NumPy's small-array sort is not stable, so every
    pattern of equal and unequal values is held against np.argsort itself"""
    assert int(np.array([5, 5, 0, 0]).argsort()[-2]) == 1 and int(np.array([5, 0, 5, 0]).argsort()[-2]) == 0     # not "lower index wins"
    n = 0
    for ranks in itertools.product(range(4), repeat=4):
        for scale in (1, 7):
            tot = np.array(ranks, dtype=np.int64) * scale
            alleles = int((tot > 0).sum())
            want = int(tot.argsort()[-2]) if 1 <= alleles <= 2 else -1
            assert target_base(tot) == want, (tot, want)
            n += 1
    assert n == 512


def test_polarised_target_is_the_first_ingroup_base_the_outgroup_lacks():
    assert target_base([6, 2, 0, 0], [4, 0, 0, 0]) == 1
    assert target_base([6, 2, 0, 0], [0, 4, 0, 0]) == 0
    assert target_base([8, 0, 0, 0], [4, 0, 0, 0]) == 1            # invariant: the first absent base, which counts 0
    assert target_base([0, 0, 8, 0], [0, 0, 3, 0]) == 0
    assert target_base([8, 0, 0, 0], [0, 4, 0, 0]) == 0            # fixed difference: the ingroup's base
    assert target_base([6, 2, 0, 0], [0, 0, 0, 0]) == -1           # no outgroup allele
    assert target_base([6, 2, 0, 0], [1, 1, 0, 0]) == -1           # two outgroup alleles
    assert target_base([6, 2, 0, 0], [0, 0, 4, 0]) == -1           # three alleles in all
    assert target_base([0, 0, 0, 0], [0, 0, 0, 0]) == -1
