"""tests/select_craft.py without a GPU: the seams of the designs follow the constants the library reports (kr_debug_select_layout), every
design holds the inputs it is there for, its tables pass kr_debug_select's own checks, and the --filter case leaves every selection
flag determined."""
import numpy as np
import pytest

import select_craft as sc
from select_ref import select_ref


@pytest.fixture(scope="module")
def lay(capi):
    return capi.select_layout()


@pytest.fixture(scope="module")
def ix():
    return sc.Index()


@pytest.fixture(scope="module")
def built(ix, lay):
    return {name: make() for name, make in sc.designs(ix, lay).items()}


def test_sizes_and_seams_follow_the_layout(lay):
    assert lay == dict(lane_max=8, group_small=16, group_mid=32, wave_gl=64, big_regs=256, big_step2=128, row_block=1024, row_round=16)
    assert sc.sizes(lay) == [0, 1, 3, 4, 5, 8, 9, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 383, 384, 385,
                             511, 512, 513, 600]
    assert sc.seams(lay, 600) == [0, 3, 7, 15, 31, 63, 127, 191, 255, 383, 598]
    assert sc.seams(lay, 257) == [0, 3, 7, 15, 31, 63, 127, 191, 255] and sc.seams(lay, 9) == [0, 3, 7] and sc.seams(lay, 1) == []
    moved = dict(lay, lane_max=12, big_regs=512)  # a changed constant moves the designs
    assert 13 in sc.sizes(moved) and 513 in sc.sizes(moved) and 11 in sc.seams(moved, 600) and 511 in sc.seams(moved, 600)
    # the row kernels: a block of reads, and a round of the workgroup within it
    assert {lay["row_block"] - 1, lay["row_block"], lay["row_block"] + 1, lay["row_block"] + lay["row_round"]} <= set(sc.WAVE_NREADS)


def rel(a, b):
    return "<" if a < b else "=" if a == b else ">"


def test_seams_design_crosses_every_seam_with_every_relation(built, lay, ix):
    """for every size and every seam p that fits: a strand pair at (p, p + 1) with d_rc <, =, > d_or and matches_rc <, =, > matches_or
    (all nine where the closest lies elsewhere), and the closest as the pair's forward and as its reverse record"""
    t, ref, _ = sc.tables(built["seams"])
    seen = {}
    for recs in ref:
        n = len(recs)
        cl = select_ref(recs)["closest"]
        for p in sc.seams(lay, n):
            (k0, d0, _, m0), (k1, d1, _, m1) = recs[p], recs[p + 1]
            assert k0 ^ 1 == k1 and not k0 & 1
            role = "or" if cl == p else "rc" if cl == p + 1 else "-"
            seen.setdefault((n, p), set()).add((role, rel(d1, d0), rel(m1, m0)))
    for n in sc.sizes(lay):
        for p in sc.seams(lay, n):
            got = seen[(n, p)]
            assert {(d, m) for r, d, m in got if r == "-"} == {(d, m) for d in "<=>" for m in "<=>"} or n < 4, (n, p)
            if n <= lay["wave_gl"]:
                assert {x for x in got if x[0] != "-"} == set(sc.FOCUS), (n, p)
    roles = {(p, x) for (n, p), got in seen.items() if n > lay["wave_gl"] for x in got if x[0] != "-"}
    assert {x for _, x in roles} == set(sc.FOCUS)
    assert ("rc", "=", "<") in {x for got in seen.values() for x in got}  # the override undoes the merge


def test_ties_design(built, lay):
    t, ref, _ = sc.tables(built["ties"])
    far, strand_beats_index, all_equal = set(), 0, 0
    for recs in ref:
        ds = [d for _, d, _, _ in recs]
        at = [i for i, d in enumerate(ds) if d == min(ds)]
        if len(at) == len(ds):
            all_equal += 1
        elif len(at) >= 2:
            far.add((at[0], at[-1] - at[0]))
            cl = select_ref(recs)["closest"]
            strand_beats_index += cl != at[-1]  # a forward record at the highest index loses to a reverse one below it
    gl, big = lay["wave_gl"], lay["big_regs"]
    assert (gl - 1, 1) in far and (big - 1, 1) in far and any(b == big for _, b in far) and any(a == 0 and b >= big for a, b in far)
    assert strand_beats_index > 20 and all_equal >= 30


@pytest.mark.parametrize("name", ["neighbours", "neighbours_s1"])
def test_neighbours_design(built, lay, name):
    """every border lies in adjacent record slots, is no pair to the reference (both records stand for their leaves), and -- IF a form
    took it for one -- would unselect the later read's first record at some borders (a lost backward guard shows) and the earlier
    read's last at others (a lost forward guard shows), decided by d and by matches, for full groups of 16 and of 32 lanes, full waves,
    steps of a lane's walk and reads of every larger form"""
    t, ref, _ = sc.tables(built[name], contiguous=True)
    borders = {}
    for r in range(len(ref) - 1):
        a, b = ref[r], ref[r + 1]
        if min(len(a), len(b)) >= 4 and a[-1][0] ^ 1 == b[0][0] and not a[-1][0] & 1:  # (the small reads between the chains are not designed)
            assert int(t["rd_off"][r]) + len(a) == int(t["rd_off"][r + 1])  # adjacent record slots too
            oa, ob = select_ref(a), select_ref(b)
            assert oa["sel"][-1] and ob["sel"][0] and oa["closest"] != len(a) - 1 and ob["closest"] != 0
            (_, d_or, _, m_or), (_, d_rc, _, m_rc) = a[-1], b[0]
            wins = "or" if d_rc > d_or or (d_rc == d_or and m_rc < m_or) else "rc"  # src/query.cpp:129-133, were they a pair
            borders.setdefault((len(a), len(b)), set()).add((wins, "d" if d_rc != d_or else "m"))
    gs, gm, gl, L, big = (lay[k] for k in ("group_small", "group_mid", "wave_gl", "lane_max", "big_regs"))
    every = {(w, by) for w in ("or", "rc") for by in ("d", "m")}
    assert borders[(gs, gs)] == every and borders[(gm, gm)] == every and borders[(4, 4)] == every and borders[(L, L)] == every
    for n in (gl, gl + 1, 2 * gl, big, big + 1):  # the wave's fast path, the loop in memory, the register form, the two passes
        assert {w for w, _ in borders[(n, n)]} == {"or", "rc"}, n
    assert (gs, gm) in borders and (gm, gs) in borders and (gl, gs) in borders
    mirrors = sum(1 for a, b in zip(ref, ref[1:]) if min(len(a), len(b)) >= 4 and a[-1][0] & 1 and a[-1][0] ^ 1 == b[0][0])
    assert mirrors == 6


def test_dmax_design(built):
    t, ref, _ = sc.tables(built["dmax"])
    closest = {min(d for _, d, _, _ in recs) for recs in ref}
    assert closest == {sc.POOL[1], sc.POOL[2], sc.POOL[3]} and sc.DMAX[0] == sc.POOL[2] and sc.DMAX[1] < sc.POOL[2] < sc.DMAX[2] == sc.POOL[3]
    for dm in sc.DMAX:  # every outcome: NA, not NA without rows, rows
        outs = [select_ref(recs, dist_max=dm) for recs in ref]
        kinds = {(o["na"], bool(o["rows"])) for o in outs}
        assert (False, True) in kinds
        assert (True, False) in kinds or dm == sc.DMAX[2]
    assert any(not o["na"] and not o["rows"] for o in (select_ref(recs, dist_max=sc.DMAX[0]) for recs in ref))  # d == dist_max exactly
    assert any(len(recs) > 256 for recs in ref)


def test_wave_designs(built, lay):
    L, gs, gm, gl, big = (lay[k] for k in ("lane_max", "group_small", "group_mid", "wave_gl", "big_regs"))
    assert [len(built[f"waves{n}"]) for n in sc.WAVE_NREADS] == list(sc.WAVE_NREADS)
    ns = [len(r) for r in built["waves1040"]]
    small, mid = set(), set()
    for w in range(0, len(ns) // 64):
        wave = ns[64 * w:64 * w + 64]
        if w == 1:
            assert min(wave) > gm  # a wave of large reads only
            continue
        small.add(sum(L < n <= gs for n in wave)), mid.add(sum(gs < n <= gm for n in wave))
    assert small == set(sc.WAVE_SMALL) and mid == set(sc.WAVE_MID)
    w0 = ns[:64]
    assert any(gm < n <= gl for n in w0) and any(gl < n <= big for n in w0) and any(n > big for n in w0)
    t, ref, _ = sc.tables(built["waves1040"])
    # a read without rows between a read of the register form and one of the two-pass form, each of more than 64 rows
    rows = [len(select_ref(recs)["rows"]) for recs in ref]
    assert any(a > 64 and gl < na <= big and b == 0 and c > 64 and nc > big for a, b, c, na, nc in zip(rows, rows[1:], rows[2:], ns, ns[2:]))
    # ... and with dist_max set, reads that have records but no row beside reads that have rows
    rows = [len(select_ref(recs, dist_max=sc.DMAX[0])["rows"]) for recs in ref]
    assert sum(1 for a, b, nb in zip(rows, rows[1:], ns[1:]) if a > 0 and b == 0 and nb > 0) > 50


@pytest.mark.parametrize("th", [4, 2])
def test_tables_pass_the_librarys_checks(capi, built, ix, th):
    nnodes = ix.tree.nnodes + 1
    for name, reads in built.items():
        t, ref, pos = sc.tables(reads, th=th, contiguous=name.startswith("neighbours"))
        assert len(pos) == sum(len(r) for r in ref) <= 125000 and len(ref) <= 2048, name
        assert capi.select_check(t, 2048, 1 << 17, nnodes, th, nnodes if th == 4 else 0) == capi.KR_OK, (name, capi.load().kr_last_error())
        used = set(zip((t["rec_w0"] != 0).tolist(), (t["rec_rep"] >= sc.DIRECT_FLAG).tolist(), (t["rec_rep"] == sc.HOLE).tolist()))
        if len(pos) > 500:  # packed words and planes, direct places and list positions, in every combination; holes between reads
            assert used >= ({(a, b, False) for a in (False, True) for b in (False, True)} if th == 4 else {(False, False, False)}), name


@pytest.mark.parametrize("th", [4, 2])
def test_filter_case_leaves_every_flag_determined(capi, ix, th):
    t, ref, fs, errs = sc.filter_case(ix, th)
    assert sorted({len(r) for r in ref}) == list(sc.FILTER_SIZES)
    nnodes = ix.tree.nnodes + 1
    assert capi.select_check(t, 2048, 1 << 17, nnodes, th, nnodes if th == 4 else 0) == capi.KR_OK
    for dm in (None, sc.POOL[4]):
        chisq, outs, ratio = sc.filter_reference(ref, fs, errs, dm)
        print(f"th {th} dist_max {dm}: chisq {chisq!r}, smallest |chi - chisq| / bound {ratio:.3g}")
        assert ratio >= 4
        nsel = sum(sum(o["sel"]) for o in outs)
        nchi = sum(sum(c is not None for c in o["chi"]) for o in outs)
        assert 0.2 * nchi < nsel < 0.8 * nchi or dm is not None  # the threshold lies among the values, not beyond them
