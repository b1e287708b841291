"""The cases of tests/vcf_cell_cases.py contain what they are built for -- shown without a GPU: the emulated device path
(tests/vcf_emul.cpp: pg_vcf_core.h's rules behind a byte-by-byte walk of the tabs) takes every regular set whole and gives the model's
bytes, which is what entitles tests/test_gpu_vcf_cells.py to demand that the device hands no block over; the host parser gives the same
bytes; the planted lines of HOSTLINES are handed over, and only they; and the geometry of the kernel's tab scan -- worked out from
the text for every residue b of the block's first byte -- has the lines on both sides of every edge the sets are named after.  These
are conditions on the cases, not on the kernels."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import vcf_cell_cases as VC
from test_vcf import _host_rows, _plan

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REGULAR = VC.regular_cases()


@pytest.fixture(scope="module")
def emul(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("vcf_cell_emul") / "libvcf_emul.so")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", os.path.join(ROOT, "tests", "vcf_emul.cpp"), "-o", so])
    return C.CDLL(so)


def emul_rows(emul, plan, body, cap):
    """(status, text, rows, line, taken) of the emulated device path over a block of whole lines, with room for cap bytes of rows"""
    out = np.empty(cap + 64, dtype=np.uint8)
    n, rows, line, taken = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int(0)
    fn = emul.pgv_emul_block
    fn.restype = C.c_int
    rc = fn(body, C.c_int64(len(body)), *plan.site_args(), C.c_char(plan.sep.encode()), 1 if plan.args.addRefTrack else 0,
            C.c_char_p(None), 0, C.c_char_p(None), 0, C.c_void_p(out.ctypes.data), C.c_int64(cap), C.byref(n), C.byref(rows),
            C.byref(line), C.byref(taken))
    return rc, out[:n.value].tobytes(), rows.value, line.value, bool(taken.value)


def first_difference(got, want):
    k = next((i for i, (x, y) in enumerate(zip(got, want)) if x != y), min(len(got), len(want)))
    return "first difference at byte %d of %d / %d: %r != %r" % (k, len(got), len(want), got[max(k - 30, 0):k + 30], want[max(k - 30, 0):k + 30])


@pytest.mark.parametrize("build", [b for _, b in REGULAR], ids=[n for n, _ in REGULAR])
def test_the_emulated_device_path_and_the_host_parser_give_the_models_rows(emul, build, tmp_path):
    case = build()
    want = VC.expected(case)
    plan = _plan(VC.argv_of(case, tmp_path), case["names"])
    assert list(plan.sel_col) == case["sel"]
    rc, text, rows, line, taken = emul_rows(emul, plan, case["body"], len(want))
    assert taken and rc == 0, "line %d went to the host: %r" % (line, case["lines"][line][:200])
    assert text == want, first_difference(text, want)
    assert rows == want.count(b"\n")
    host, k = _host_rows(plan, case["body"])
    assert host == want, first_difference(host, want)
    assert k == rows


def test_the_row_far_beyond_the_room_is_the_models_too(emul, tmp_path):
    small, big = VC.room("fits"), VC.room("overflows")
    for case in (small, big):
        want = VC.expected(case)
        plan = _plan(VC.argv_of(case, tmp_path), case["names"])
        rc, text, _, _, taken = emul_rows(emul, plan, case["body"], len(want))
        assert taken and rc == 0 and text == want
        host, _ = _host_rows(plan, case["body"])
        assert host == want
    # the rows of the first are longer than its text and inside the room the device route gives them; those of the second far outside
    rows, text, cap = len(VC.expected(small)), len(small["body"]), VC.out_cap_of(small)
    print("ROOM fits: %d bytes of rows, %d of text, room for %d" % (rows, text, cap))
    assert text < rows <= cap
    rows, text, cap = len(VC.expected(big)), len(big["body"]), VC.out_cap_of(big)
    print("ROOM overflows: %d bytes of rows, %d of text, room for %d" % (rows, text, cap))
    assert rows > 10 * cap
    assert len(small["lines"]) == 20 and small["n_cols"] == 50
    t = small["truth"][7]
    assert t["alleles"] == ["A", "A" + "C" * 40] and all(c == ((1, 1), "/") for c in t["calls"])


@pytest.mark.parametrize("name", VC.HOSTLINES)
def test_the_planted_line_and_no_other_is_handed_to_the_host(emul, name, tmp_path):
    case = VC.hostline(name)
    at = VC.planted_line(case)
    plan = _plan(VC.argv_of(case, tmp_path), case["names"])
    rc, _, _, line, taken = emul_rows(emul, plan, case["body"], 4 * len(case["body"]))
    assert taken and rc == 1 and line == at, (rc, line, at)
    # without it the block is the device's: the model's rows of the other lines
    lines = [ln for i, ln in enumerate(case["lines"]) if i != at]
    truth = [t for i, t in enumerate(case["truth"]) if i != at]
    body = ("\n".join(lines) + "\n").encode("latin-1")
    want = VC.model(truth, case["sel"], case["sep"], case["missing"])
    rc, text, _, _, _ = emul_rows(emul, plan, body, len(want))
    assert rc == 0 and text == want
    if case["raises"]:                                            # a named column missing: the host parser words the error
        from genomics_general_amd._lib import PopgenError
        with pytest.raises(PopgenError, match=case["raises"]):
            _host_rows(plan, case["body"])
    else:                                                         # the host parser reads the planted line without complaint
        _host_rows(plan, case["body"])
    # several blocks, the planted line's neither the first nor the last
    block = int(case["env"]["PG_STREAM_BYTES"])
    before = sum(len(ln) + 1 for ln in case["lines"][:at])
    assert before > 2 * block and len(case["body"]) - before > 2 * block


# ---- geometry: for every residue b of the block's first byte -----------------------------------------------------------------------
def data_geometry(case):
    return [g for g in VC.geometry(case["lines"]) if g is not None]


def test_align_every_section_shape_stands_at_all_sixteen_places_of_a_word():
    for name in VC.ALIGN:
        case = VC.align(name)
        geo = data_geometry(case)
        if case["section_bytes"] is not None:
            assert {g["S"] for g in geo} == {case["section_bytes"]}          # start mask and end mask in the same word
            assert all(not g["tabs"] for g in geo)
        for b in range(16):
            places = sorted({VC.A_of(g, b) for g in geo})
            assert places == list(range(16)), (name, b)
            if case["section_bytes"] == 3:                                   # ... or the section over the seam of two words
                assert {VC.A_of(g, b) for g in geo if VC.A_of(g, b) + 3 > 16} == {14, 15}
        print("ALIGN %s: %d data lines, S in %s, 16 places of A at every b" % (name, len(geo), sorted({g["S"] for g in geo})[:6]))
    assert VC.align("cols3")["n_cols"] == 3 and max(g["S"] for g in data_geometry(VC.align("cols3"))) < 32


def test_steps_sections_end_on_both_sides_of_a_step_and_tabs_stand_on_its_edge():
    for B in VC.STEPS:
        geo = data_geometry(VC.steps(B))
        pairs = {(g["S"], (g["ls"] + g["cells_off"]) % 16) for g in geo}
        assert pairs == {(S, r) for S in range(B - VC.STEPS_SPAN, B + VC.STEPS_SPAN + 1) for r in range(16)}
        for b in range(16):
            ends = [VC.A_of(g, b) + g["S"] for g in geo]
            n_end = {d: sum(1 for e in ends if e == B + d) for d in (-1, 0, 1)}
            tabs = [set(VC.walk_tabs(g, b)) for g in geo]
            n_tab = {d: sum(1 for t in tabs if B + d in t) for d in (-1, 0)}
            n_new = sum(1 for e in ends if B < e <= B + 16)
            if b == 0:
                print("STEPS %d (b = 0): %d lines; A + S = B - 1 / B / B + 1 in %d / %d / %d; a tab at walk offset B - 1 / B in %d / %d; "
                      "sections ending in the first 16 bytes of the next step: %d" % (B, len(geo), n_end[-1], n_end[0], n_end[1], n_tab[-1], n_tab[0], n_new))
            assert min(n_end.values()) >= 1 and min(n_tab.values()) >= 1 and n_new >= 16, (B, b)


def test_extra_the_last_named_tab_falls_on_both_sides_of_the_first_step():
    case = VC.extra("exit")
    geo = data_geometry(case)
    n = case["n_cols"]
    assert all(len(g["tabs"]) >= n for g in geo)                              # more columns than the header names, on every line
    for b in range(16):
        at = [VC.walk_tabs(g, b)[n - 1] for g in geo]
        assert 1023 in at and 1024 in at, b
        if b == 0:
            print("EXTRA exit (b = 0): %d lines, the %d-th tab at walk offset 1023 in %d and 1024 in %d" % (len(geo), n, at.count(1023), at.count(1024)))
    misc = VC.extra("misc")
    kinds = {t["kind"] for t in misc["truth"] if t is not None}
    assert kinds == {"space_near", "space_far", "trailing_tab", "high_byte", "plain", "two_extra"}
    lines = [ln for ln, t in zip(misc["lines"], misc["truth"]) if t is not None]
    truth = [t for t in misc["truth"] if t is not None]
    geo = data_geometry(misc)
    for b in range(16):
        same_word = later_step = 0
        for ln, t, g in zip(lines, truth, geo):
            tab = VC.A_of(g, b) + g["tabs"][misc["n_cols"] - 1] if len(g["tabs"]) >= misc["n_cols"] else None
            if t["kind"] == "space_near":
                sp = VC.A_of(g, b) + ln.index(" ") - g["cells_off"]
                same_word += sp // 16 == tab // 16
            if t["kind"] == "space_far":
                sp = VC.A_of(g, b) + ln.index(" ") - g["cells_off"]
                assert sp - tab == 3000
                later_step += sp // 1024 > tab // 1024
        assert same_word >= 1 and later_step >= 1, b
    assert any("\xe9" in ln for ln in lines) and any(ln.endswith("\t") for ln in lines)


def test_hostlines_the_blank_stands_at_every_place_of_a_word():
    cases = [VC.hostline("blank_r%d" % r) for r in range(16)]
    for b in range(16):
        where = []
        for case in cases:
            at = VC.planted_line(case)
            g = VC.geometry(case["lines"])[at]
            ln = case["lines"][at]
            where.append((VC.A_of(g, b), VC.A_of(g, b) + ln.index("\x0b") - g["cells_off"]))
        assert sorted(w % 16 for _, w in where) == list(range(16))           # the first byte of a word, the last, and all between
        assert sum(1 for a, w in where if w < 16) == 13 and all(w == a + 3 for a, w in where)   # in the word that holds cells_off
    print("HOSTLINES: the blank at all 16 places of a word, in cells_off's word in 13 of 16, at every b")


def test_lanes_calls_of_different_lengths_on_both_sides_of_the_64th_lane():
    for name in VC.LANES:
        case = VC.lanes(name)
        assert len(case["lines"]) == 40 and sum(1 for t in case["truth"] if t["indel"]) == 10
        if len(case["sel"]) < 65:
            continue
        c63, c64 = case["sel"][63], case["sel"][64]
        n = 0
        for t in case["truth"]:
            if not t["indel"]:
                continue
            i63, i64 = t["calls"][c63][0], t["calls"][c64][0]
            if None in i63 or None in i64:
                continue
            n += len({len(t["alleles"][i]) for i in i63 + i64}) > 1
        print("LANES %s: %d indel lines with selected samples 63 and 64 called, alleles of different lengths" % (name, n))
        assert n >= 1, name
    # the selections: all in header order, reversed header order, scattered; ploidy 1 and 2 mixed over the 64th lane
    assert [len(VC.lanes("all_%d" % n)["sel"]) for n in VC.LANES_ALL] == VC.LANES_ALL
    for n in VC.LANES_SEL:
        rev, scat = VC.lanes("rev_%d" % n)["sel"], VC.lanes("scat_%d" % n)["sel"]
        assert len(rev) == len(set(rev)) == n and rev == sorted(rev, reverse=True)
        assert len(scat) == len(set(scat)) == n and scat != sorted(scat) and scat != sorted(scat, reverse=True)
    for n in VC.LANES_PL:
        t = VC.lanes("pl_%d" % n)["truth"][0]
        assert [len(c[0]) for c in t["calls"]][60:65] == [2, 2, 1, 2, 2]
    pl = VC.lanes("pl_129")
    assert pl["add_ref"] and pl["sep"] == "," and pl["missing"] == "?"


def test_waves_the_three_block_shapes_and_a_last_block_partly_empty():
    assert [VC.wpb_of(n) for n in VC.WAVES_COLS] == [4, 2, 2, 1, 1]
    for wpb in (4, 2):
        assert any(n % wpb for n in VC.WAVES_LINES) and any(n % wpb == 0 for n in VC.WAVES_LINES)
    case = VC.waves(3841, 5)
    assert case["sel"][:2] == [3840, 0] and sum(1 for t in case["truth"] if t["indel"]) == 1
    assert not case["lines"][0].endswith("\t")                               # the last column ends at line_len, not at a tab
    print("WAVES: wpb", [VC.wpb_of(n) for n in VC.WAVES_COLS], "for", VC.WAVES_COLS)


def test_scan_lines_without_a_row_stand_at_every_place_of_a_stretch():
    for n in VC.SCAN:
        case = VC.scan(n)
        assert len(case["lines"]) == n
        per = (n + 1023) // 1024
        none = [i for i, t in enumerate(case["truth"]) if t is None or not t["kept"]]
        assert {i % per for i in none} == set(range(per))
        assert any(t is None for t in case["truth"]) and any(t is not None and not t["kept"] for t in case["truth"])
        print("SCAN %d: %d lines a thread, %d lines without a row" % (n, per, len(none)))
    assert [(n + 1023) // 1024 for n in VC.SCAN] == [1, 1, 1, 1, 1, 2, 3]


@pytest.mark.parametrize("build", [b for _, b in REGULAR], ids=[n for n, _ in REGULAR])
def test_no_regular_set_is_empty(build):
    """at least four lines in five kept, a complex row, a missing call and not only missing calls: an empty output cannot hide a
    kernel that writes nothing"""
    case = build()
    kept = [t for t in case["truth"] if t is not None and t["kept"]]
    assert len(kept) >= 0.8 * len(case["lines"]), (len(kept), len(case["lines"]))
    assert any(len(set(map(len, t["alleles"]))) > 1 for t in kept)
    calls = [t["calls"][c][0] for t in kept for c in case["sel"]]
    n_missing = sum(1 for c in calls if None in c)
    assert 1 <= n_missing < len(calls) / 2, (n_missing, len(calls))
