"""-m gpu: the sfs.py drop-in.  (1) its command lines against the committed outputs of the unmodified reference (tests/golden/sfs/, made by
tests/golden/make_golden_sfs.py): every output file byte for byte; (2) the accumulation kernels of pg_sfs.hip (k_sfs_rows, k_sfs_base,
k_sfs_target, k_sfs_compact) against a NumPy model written here -- bincount for the counts, the first index for `first`, compared
exactly -- on both table routes (LDS tables by default, PG_SFS_LDS=0 forces the global route)."""
import functools
import json
import os

import numpy as np
import pytest

from sfs_cases import SFS_CASES
from gpu_util import make_engine
from genomics_general_amd import _lib, cli

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
MODES = ["default", "PG_SFS_LDS=0"]


def set_mode(monkeypatch, mode):
    if mode != "default":
        name, _, val = mode.partition("=")
        monkeypatch.setenv(name, val)


# ---- goldens -------------------------------------------------------------------------------------------------
def run_case(case, tmp_path, capsys):
    out = str(tmp_path / case["name"])
    os.makedirs(out)
    geno = os.path.join(GOLD, case["fixture"] + ".geno.gz") if case.get("fixture") else ""
    argv = [a.format(geno=geno, dir=GOLD, out=out) for a in case["argv"]]
    want_dir = os.path.join(GOLD, "sfs", case["name"])
    if case.get("fails"):
        with pytest.raises(SystemExit) as exc:
            cli.sfs_main(argv)
        assert exc.value.code not in (0, None) and os.listdir(out) == []
        return None
    capsys.readouterr()
    assert cli.sfs_main(argv) in (0, None)
    cap = capsys.readouterr()
    names = sorted(os.listdir(want_dir))
    if case.get("pipe"):
        assert names == ["stdout"] and os.listdir(out) == []
        with open(os.path.join(want_dir, "stdout")) as f:
            assert cap.out == f.read()
    else:
        assert sorted(os.listdir(out)) == names
        for fn in names:
            with open(os.path.join(out, fn), "rb") as f, open(os.path.join(want_dir, fn), "rb") as g:
                assert f.read() == g.read(), fn
    return cap.err


@pytest.mark.parametrize("case", SFS_CASES, ids=[c["name"] for c in SFS_CASES])
def test_sfs_reproduces_the_reference_files(case, tmp_path, capsys):
    run_case(case, tmp_path, capsys)


def case_named(name):
    return [c for c in SFS_CASES if c["name"] == name][0]


def timing(err):
    return [json.loads(ln[len("PG_TIMING "):]) for ln in err.splitlines() if ln.startswith("PG_TIMING ")][-1]


def test_table_in_small_blocks_raises_the_extents_and_merges(tmp_path, capsys, monkeypatch):
    """a tiny PG_STREAM_BYTES: many blocks, the running maximum of the counts grows in a later one, the session restarts with larger
    extents and the partial read-outs are merged -- same files"""
    monkeypatch.setenv("PG_STREAM_BYTES", "300")
    monkeypatch.setenv("PG_TIMING", "1")
    tm = timing(run_case(case_named("table_target"), tmp_path, capsys))
    assert tm["blocks"] >= 3 and tm["extent_restarts"] >= 1, tm


@pytest.mark.parametrize("name", ["table_base_minor_regions", "abba_trios_quartets", "bigpos_regions_overlap"])
def test_goldens_on_the_global_route(name, tmp_path, capsys, monkeypatch):
    monkeypatch.setenv("PG_SFS_LDS", "0")
    monkeypatch.setenv("PG_SFS_CHUNK", "1000")
    run_case(case_named(name), tmp_path, capsys)


@pytest.mark.parametrize("name,env", [("abba_polarized_pairs", {"PG_STREAM_BYTES": "50000"}), ("c1_1d", {"PG_GPU_TOKENIZER": "0", "PG_STREAM_BYTES": "30000"}),
                                      ("bigpos_regionsfile_include", {"PG_STREAM_BYTES": "20000"})])
def test_genotype_goldens_streamed_in_blocks(name, env, tmp_path, capsys, monkeypatch):
    """the line ordinal runs on across the blocks of the input (device and host tokenizer)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("PG_TIMING", "1")
    tm = timing(run_case(case_named(name), tmp_path, capsys))
    assert tm["blocks"] >= 3, tm


def test_launcher_runs_as_a_program(tmp_path):
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(GOLD))
    case = case_named("c1_pairs_pipe")
    argv = [a.format(geno=os.path.join(GOLD, "c1.geno.gz"), dir=GOLD, out=str(tmp_path)) for a in case["argv"]]
    r = subprocess.run([sys.executable, os.path.join(root, "sfs.py")] + argv, stdout=subprocess.PIPE, stderr=subprocess.PIPE, cwd=str(tmp_path), timeout=300)
    assert r.returncode == 0, r.stderr.decode()[-800:]
    with open(os.path.join(GOLD, "sfs", case["name"], "stdout"), "rb") as f:
        assert r.stdout == f.read()


# ---- the NumPy model -------------------------------------------------------------------------------------------
def target_of(tot, out):
    """sfs.py:60-85 on one site's totals (out None: the minor allele by np.argsort itself)"""
    alleles = tot > 0
    allA = alleles | (out > 0) if out is not None else alleles
    if not 1 <= allA.sum() <= 2:
        return -1
    if out is not None:
        n_out = int((out > 0).sum())
        if n_out != 1:
            return -1
        cand = np.flatnonzero(~(out > 0) & alleles)
        return int(cand[0]) if len(cand) else int(np.flatnonzero(~alleles)[0])
    return int(tot.argsort()[-2])


def targets(cnt, in_pops, out_pop, need_complete, n_slots):
    """cnt int64 [n][P][4] -> (valid [n], t [n][n_in])"""
    n = len(cnt)
    tot = cnt[:, in_pops].sum(axis=1)
    out = cnt[:, out_pop] if out_pop >= 0 else np.zeros((n, 4), dtype=np.int64)
    rows, inv = np.unique(np.concatenate([tot, out], axis=1), axis=0, return_inverse=True)
    base_u = np.array([target_of(r[:4], r[4:] if out_pop >= 0 else None) for r in rows], dtype=np.int64)
    base = base_u[inv.reshape(-1)]
    valid = base >= 0
    if need_complete:
        valid &= (cnt[:, in_pops].sum(axis=2) == np.asarray(n_slots)[None, :]).all(axis=1)
    t = np.take_along_axis(cnt[:, in_pops], np.maximum(base, 0)[:, None, None], axis=2)[:, :, 0]
    return valid, t


def membership(n, n_intervals, members):
    if members is None:
        return np.ones((n, 1), dtype=np.int64)
    off, st, en, ids, row_run, pos = members
    M = np.zeros((n, n_intervals), dtype=np.int64)
    for r in range(len(off) - 1):
        for j in range(off[r], off[r + 1]):
            M[:, ids[j]] += (row_run == r) & (st[j] <= pos) & (pos <= en[j])
    return M


def model(valid, t, ext, groups, n_intervals, members, ord0=0):
    """{global cell: (first, counts tuple)} over the groups' tables laid end to end"""
    M = membership(len(t), n_intervals, members)
    valid = valid & (M.sum(axis=1) > 0)
    idx = np.flatnonzero(valid)
    want, base = {}, 0
    for g in groups:
        dims = tuple(ext[p] for p in g)
        cell = np.ravel_multi_index(tuple(t[idx, p] for p in g), dims) if len(idx) else np.zeros(0, dtype=np.int64)
        uniq, first_at = np.unique(cell, return_index=True)
        for k in range(M.shape[1]):
            c = np.bincount(cell, weights=M[idx, k], minlength=int(np.prod(dims))).astype(np.int64)
            for u in uniq:
                want.setdefault(base + int(u), [0, [0] * M.shape[1]])[1][k] = int(c[u])
        for u, fa in zip(uniq, first_at):
            want[base + int(u)][0] = ord0 + int(idx[fa])
        base += int(np.prod(dims))
    return {k: (v[0], tuple(v[1])) for k, v in want.items()}


def read_out(e):
    cell, first, counts = e.sfs_read()
    assert len(set(cell.tolist())) == len(cell)
    return {int(c): (int(f), tuple(int(x) for x in cc)) for c, f, cc in zip(cell, first, counts)}


@functools.lru_cache(maxsize=None)
def rows_engine(n_dip, n_pops, L, seed, var_thr, miss_thr):
    e, lay, codes, _ = make_engine(n_dip, n_pops, L, seed, var_thr=var_thr, miss_thr=miss_thr)
    hap_pop = np.asarray(lay.hap_pop)
    cnt = np.stack([np.stack([((codes[:, hap_pop == p] >> b) & 1).sum(axis=1) for b in range(4)], axis=1) for p in range(n_pops)], axis=1).astype(np.int64)
    cnt.setflags(write=False)
    n_slots = [int((hap_pop == p).sum()) for p in range(n_pops)]
    return e, cnt, n_slots


GROUPS3 = [[0], [1], [2], [0, 1], [0, 2], [1, 2], [2, 0, 1]]


def check_rows(e, cnt, n_slots, in_pops, out_pop, groups, members=None, n_intervals=1, ord0=0, expect_lds=None):
    ext = [n_slots[p] + 1 for p in in_pops]
    cells, on_lds = e.sfs_begin(ext, groups, n_intervals)
    if expect_lds is not None:
        assert on_lds.tolist() == expect_lds, on_lds
    try:
        e.sfs_add_sites(0, len(cnt), ord0, in_pops, out_pop, members)
        got = read_out(e)
    finally:
        e.sfs_end()
    valid, t = targets(cnt, in_pops, out_pop, True, [n_slots[p] for p in in_pops])
    want = model(valid, t, ext, groups, n_intervals, members, ord0)
    assert got == want
    return want


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("L", [1, 63, 64, 65, 257])
def test_rows_small_site_counts(L, mode, monkeypatch):
    set_mode(monkeypatch, mode)
    e, cnt, n_slots = rows_engine(6, 3, L, 40 + L, 30000, 1500)
    check_rows(e, cnt, n_slots, [0, 1, 2], -1, GROUPS3, expect_lds=[mode == "default"] * len(GROUPS3))
    check_rows(e, cnt, n_slots, [0, 2], 1, [[0], [1], [1, 0]], ord0=2 ** 40)             # an outgroup in the middle, ordinals past 32 bits


@pytest.mark.parametrize("mode", MODES)
def test_rows_across_chunk_boundaries(mode, monkeypatch):
    set_mode(monkeypatch, mode)
    monkeypatch.setenv("PG_SFS_CHUNK", "4097")                                           # 18 launches, none a multiple of the block
    e, cnt, n_slots = rows_engine(6, 3, 70001, 7, 20000, 1000)
    want = check_rows(e, cnt, n_slots, [0, 1, 2], -1, GROUPS3)
    assert len(want) > 50
    check_rows(e, cnt, n_slots, [0, 1], 2, [[0], [1], [0, 1]])


@pytest.mark.parametrize("mode", MODES)
def test_all_sites_monomorphic_hit_one_cell(mode, monkeypatch):
    set_mode(monkeypatch, mode)
    e, cnt, n_slots = rows_engine(6, 3, 100000, 3, 0, 0)
    want = check_rows(e, cnt, n_slots, [0, 1, 2], -1, [[0], [0, 1, 2]])
    assert sorted(want.values()) == [(0, (100000,)), (0, (100000,))]


@pytest.mark.parametrize("mode", MODES)
def test_high_variation_touches_many_cells(mode, monkeypatch):
    set_mode(monkeypatch, mode)
    e, cnt, n_slots = rows_engine(6, 3, 20000, 5, 64000, 300)
    want = check_rows(e, cnt, n_slots, [0, 1, 2], -1, GROUPS3)
    assert len(want) > 150
    check_rows(e, cnt, n_slots, [1, 2], 0, [[0], [1], [0, 1]])


@pytest.mark.parametrize("mode", MODES)
def test_four_dimensions_of_five_diploids_take_the_global_route(mode, monkeypatch):
    set_mode(monkeypatch, mode)
    e, cnt, n_slots = rows_engine(20, 4, 30000, 9, 50000, 200)
    groups = [[0], [0, 1, 2, 3], [3, 1]]
    want = check_rows(e, cnt, n_slots, [0, 1, 2, 3], -1, groups, expect_lds=[mode == "default", False, mode == "default"])
    assert len(want) > 500 and 11 ** 4 > 8192


def interval_members(n, n_runs, spec, seed):
    """spec[r] = list of (start, end, id); rows get runs in blocks and UNSORTED positions in [0, 1000)"""
    rng = np.random.default_rng(seed)
    row_run = ((np.arange(n) * n_runs) // max(n, 1)).astype(np.int32)
    pos = rng.integers(0, 1000, size=n).astype(np.int64) + (2 ** 31 - 500)
    off, st, en, ids = [0], [], [], []
    for r in range(n_runs):
        for s, t, k in spec.get(r, []):
            st.append(s + 2 ** 31 - 500)
            en.append(t + 2 ** 31 - 500)
            ids.append(k)
        off.append(len(st))
    return (np.array(off, dtype=np.int32), np.array(st, dtype=np.int64), np.array(en, dtype=np.int64), np.array(ids, dtype=np.int32), row_run, pos)


INTERVALS = {
    "one": (1, {0: [(100, 600, 0)]}),
    "three_overlapping": (3, {0: [(0, 500, 0), (300, 800, 1)], 2: [(0, 999, 2), (400, 450, 0)]}),
    "seventy": (70, {0: [(10 * k, 10 * k + 300, k) for k in range(70)], 1: [(0, 999, 69), (500, 500, 3)], 2: []}),
}


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("which", ["none"] + list(INTERVALS))
def test_interval_membership(which, mode, monkeypatch):
    set_mode(monkeypatch, mode)
    monkeypatch.setenv("PG_SFS_CHUNK", "1111")
    e, cnt, n_slots = rows_engine(6, 3, 3000, 21, 30000, 500)
    if which == "none":
        check_rows(e, cnt, n_slots, [0, 1, 2], -1, GROUPS3)
        return
    n_intervals, spec = INTERVALS[which]
    members = interval_members(len(cnt), 3, spec, 77)
    want = check_rows(e, cnt, n_slots, [0, 1, 2], -1, [[0], [1, 2], [0, 1, 2]], members, n_intervals)
    assert any(0 in c for _, c in want.values()) or n_intervals == 1               # rows with zeros for the other intervals
    if which == "seventy":
        assert max(sum(x > 0 for x in c) for _, c in want.values()) > 64           # one cell counted by more than 64 intervals


@pytest.mark.parametrize("mode", MODES)
def test_table_routes(mode, monkeypatch):
    set_mode(monkeypatch, mode)
    monkeypatch.setenv("PG_SFS_CHUNK", "700")
    e, _, _ = rows_engine(6, 3, 64, 1, 30000, 0)                                   # (any context: the tables are uploaded)
    rng = np.random.default_rng(8)
    n, ext, groups = 5000, [7, 4, 12], [[0], [2], [1, 2], [2, 1, 0]]
    tc = np.stack([rng.integers(0, x, size=n) for x in ext], axis=1).astype(np.int32)
    tc[rng.random(n) < 0.7] = 0                                                    # most sites in the all-zero cell
    members = interval_members(n, 3, INTERVALS["three_overlapping"][1], 5)
    for mem, ni in ((None, 1), (members, 3)):
        e.sfs_begin(ext, groups, ni)
        try:
            e.sfs_add_target_counts(tc[:2000], 10, mem if mem is None else mem[:4] + (mem[4][:2000], mem[5][:2000]))
            e.sfs_add_target_counts(tc[2000:], 2010, mem if mem is None else mem[:4] + (mem[4][2000:], mem[5][2000:]))
            got = read_out(e)
        finally:
            e.sfs_end()
        assert got == model(np.ones(n, dtype=bool), tc.astype(np.int64), ext, groups, ni, mem, 10)
    # base counts: monomorphic, biallelic (with ties), three alleles, empty; columns picked out of five, the outgroup among them
    kind = rng.integers(0, 4, size=n)
    cnt = np.zeros((n, 5, 4), dtype=np.int64)
    a, b, c = rng.integers(0, 4, size=(3, n))
    for p in range(5):
        x, y, z = rng.integers(0, 6, size=(3, n))
        cnt[np.arange(n), p, a] += np.where(kind < 3, x, 0)
        cnt[np.arange(n), p, b] += np.where((kind == 1) | (kind == 2), y, 0)
        cnt[np.arange(n), p, c] += np.where(kind == 2, z, 0)
    for in_cols, out_col in (([3, 0, 4], -1), ([4, 1], 2)):
        ext = [int(cnt[:, p].max()) + 1 for p in in_cols]
        groups = [[k] for k in range(len(in_cols))] + [list(range(len(in_cols)))[::-1]]
        e.sfs_begin(ext, groups, 1)
        try:
            e.sfs_add_base_counts(cnt, 0, in_cols, out_col)
            got = read_out(e)
        finally:
            e.sfs_end()
        valid, t = targets(cnt, in_cols, out_col, False, None)
        assert 0.2 < valid.mean() < 0.95
        assert got == model(valid, t, ext, groups, 1, None)


def test_counts_beyond_the_extents_and_tables_beyond_the_budget_are_errors():
    e, _, _ = rows_engine(6, 3, 64, 1, 30000, 0)
    e.sfs_begin([4, 4], [[0, 1]], 1)
    try:
        with pytest.raises(_lib.PopgenError, match="extent"):
            e.sfs_add_target_counts(np.array([[1, 2], [3, 4]], dtype=np.int32), 0)
        with pytest.raises(_lib.PopgenError, match="extent"):
            e.sfs_add_target_counts(np.array([[-1, 2]], dtype=np.int32), 0)
    finally:
        e.sfs_end()
    e.set_scratch_limit(64 << 20)
    try:
        with pytest.raises(_lib.PopgenError, match="bytes"):
            e.sfs_begin([101, 101, 101, 101], [[0, 1, 2, 3]], 1)
        with pytest.raises(_lib.PopgenError, match="pg_sfs_begin must be called first"):
            e.sfs_read()
    finally:
        e.set_scratch_limit(48 << 30)
