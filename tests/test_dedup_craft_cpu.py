"""tests/dedup_craft.py without a device: every design sits where it claims (by the reference alone), every design's tables pass
kr_debug_dedup_check, check() accepts what a plain sequential model of the stage produces, and rejects one corrupted result per
invariant of the contract."""
import copy

import numpy as np
import pytest

import dedup_craft as dc

MAX_READS, MAX_RECORDS = 8192, 16384


@pytest.fixture(scope="module")
def lay(capi):
    return capi.dedup_layout()


@pytest.fixture(scope="module")
def tables(lay):
    return {name: f(lay) for name, f in dc.DESIGNS.items()}


@pytest.fixture(scope="module")
def ix():
    return dc.Index()


def cfg_of(lay, ix, **kw):
    return dc.Config(lay, ix.rho, **kw)


def test_class_numbering():
    assert len(dc.CLASS_OF) == 55 and sorted(dc.CLASS_OF.values()) == list(range(55))
    assert dc.CLASSES[0] == (1, 0, 0, 0, 0) and dc.CLASSES[1] == (2, 0, 0, 0, 0) and dc.CLASSES[3] == (0, 1, 0, 0, 0) and dc.CLASSES[54] == (0, 0, 0, 0, 3)
    assert all(1 <= sum(c) <= 3 for c in dc.CLASSES)


def test_layout_is_the_documented_one(capi, lay):
    assert lay == dict(oslots=8, classes=55, max_events=3, min_slots=1024, probe_rounds=48, rep_chunk=16, rep_chunk_max=256, dedup_blocks=4096,
                       oslot_reads=4096, hash_word=0x9E3779B97F4A7C15, hash_leaf=0x85EBCA6B)
    assert lay["classes"] == len(dc.CLASS_OF)


def test_index_conditions(capi, lay, ix, tmp_path):
    places = lay["oslots"] * lay["classes"] * dc.NNODES
    assert dc.NNODES % 2 == 1 and places % 16 == 8  # the last 16-place group of kr_dedup_direct_kernel lies half outside the places
    assert places % 4096 != 0 and places % 4 == 0
    assert len(set(ix.rho[1:])) >= 3 and 0.0 in ix.rho[1:]
    hx = capi.HostIndex(ix.write(str(tmp_path / "idx")))
    assert hx.lib_arrays()["rho"].tolist() == ix.rho and len(ix.rho) == dc.NNODES
    assert hx.view.tree_nnodes + 1 == dc.NNODES
    hx.close()


def test_every_design_passes_the_entry_check(capi, lay, tables):
    for name, t in tables.items():
        assert capi.dedup_check(t, MAX_READS, MAX_RECORDS, dc.NNODES, 4) == capi.KR_OK, (name, capi.load().kr_last_error())
    for th in (2, 6):
        assert capi.dedup_check(dc.design_th_other(lay, th), MAX_READS, MAX_RECORDS, dc.NNODES, th) == capi.KR_OK
    allt = dc.concat(list(tables.values()))
    assert len(allt["rd_off"]) <= MAX_READS and len(allt["rec_key"]) <= MAX_RECORDS
    assert capi.dedup_check(allt, MAX_READS, MAX_RECORDS, dc.NNODES, 4) == capi.KR_OK


def test_classes_design(lay, tables):
    t = tables["classes"]
    pl = dc.direct_places(t, 4, dc.NNODES, lay)
    prob = dc.problems_of(t)
    _, rd = dc.in_read(t)
    osl = dc.oslots(t, lay)
    assert osl[130] == 0 and osl[255] == 7 and osl[77] == 0xFF and sorted(osl[100:106].tolist()) == list(range(1, 7))
    for leaf in (5, dc.TOP):
        got = {(int(p) // dc.NNODES) % lay["classes"] for p, k in zip(pl, t["rec_key"]) if p >= 0 and k >> 1 == leaf and int(p) // dc.NNODES < lay["classes"]}
        assert got == set(range(55)), leaf
    neighbours = [dc.ev(0, 4), (1, 1, 1, 1, 0), dc.ev(2, 255)]
    for i, p in enumerate(prob):
        if p is None:
            continue
        c, om = dc.unpack(p[2])
        if c in neighbours or om in (256, 77):
            assert pl[i] < 0, (i, c, om)
        # every record has a duplicate in another read
        twins = [j for j, q in enumerate(prob) if q == p and rd[j] != rd[i]]
        assert twins, i
    assert any(dc.unpack(p[2])[1] == 255 and pl[i] >= 0 for i, p in enumerate(prob) if p)  # a direct record at the slot of 255 k-mers


def test_last_place_design(lay, tables):
    t = tables["last_place"]
    assert dc.direct_places(t, 4, dc.NNODES, lay).max() == lay["oslots"] * lay["classes"] * dc.NNODES - 1
    assert dc.oslots(t, lay)[50] == 7


def test_oslot_designs(lay, tables):
    a = dc.oslots(tables["oslots_a"], lay)
    assert a[30] == 7 and a[20] == 0xFF and a[16] == 0 and a[10] == 6 and (a != 0xFF).sum() == 8
    b = dc.oslots(tables["oslots_b"], lay)
    assert (b[91], b[92], b[90]) == (0, 1, 2) and (b != 0xFF).sum() == 3
    c = dc.oslots(tables["oslots_c"], lay)
    assert c[99] == 0xFF and (c[41], c[40]) == (0, 1) and (c != 0xFF).sum() == 2
    t = tables["oslots_d"]
    n = len(t["rd_off"])
    assert n == lay["oslot_reads"] + 1 and (n + lay["oslot_reads"] - 1) // lay["oslot_reads"] == 2  # a grid of two blocks
    with_recs = np.nonzero(t["rd_cnt"])[0]
    assert len(with_recs) == 25 and ((with_recs[:-1] % 512) >= 256).all() and with_recs[-1] % 512 < 256  # block 1's reads, and one of block 0's
    d = dc.oslots(t, lay)
    assert d[30] == 7 and d[20] == 0xFF and (d != 0xFF).sum() == 8  # 30: the last read makes it 2 : 2 ... the tie goes to the larger count
    assert (t["rd_onmers"][t["rd_cnt"] == 0] == 99).all() and d[99] == 0xFF


def slots_of(t, lay, mask):
    return [None if p is None or p[0] != "p" else dc.first_slot(p[2], p[1], mask, lay) for p in dc.problems_of(t)]


def test_table_designs(lay, ix, tables):
    mask = lay["min_slots"] - 1
    cfg = cfg_of(lay, ix)
    # same word, other leaves
    t = tables["same_word_other_leaf"]
    assert len(set(t["rec_w0"].tolist())) == 1 and len(set((t["rec_key"] >> 1).tolist())) == 40 and len(t["rec_key"]) == 80
    sl = slots_of(t, lay, mask)
    assert np.bincount(sl[:40]).max() >= 3 and (dc.direct_places(t, 4, dc.NNODES, lay) < 0).all()
    # the wrap
    t = tables["chain_wrap"]
    sl = slots_of(t, lay, mask)
    assert len(set(dc.problems_of(t))) == 12 and all(mask - 3 <= s <= mask for s in sl) and (dc.direct_places(t, 4, dc.NNODES, lay) < 0).all()
    m = dc.model(t, cfg, dc.fake_brent)
    assert (m["dd_table"][mask - 3:mask + 1, 0] != 0).all() and (m["dd_table"][:8, 0] != 0).all() and m["problems"] == 12
    # one wave, one problem; then one wave of 64 problems with one first slot
    t = tables["one_wave_same_problem"]
    prob, sl = dc.problems_of(t), slots_of(t, lay, mask)
    assert len(set(prob[:64])) == 1 and len(set(prob[64:128])) == 64 and len(set(sl[64:128])) == 1 and len(prob) == 128 and sl[0] != sl[64]
    # beyond the probe limit
    t = tables["beyond_48"]
    prob, sl = dc.problems_of(t), slots_of(t, lay, mask)
    assert len(prob) == 124 and prob[60:64] == [None] * 4 and prob[:60] == prob[64:] and len(set(prob[:60])) == 60 and len(set(sl[:60])) == 1
    m = dc.model(t, cfg, dc.fake_brent)
    assert (m["dd_table"][:, 0] != 0).sum() == lay["probe_rounds"] and m["problems"] == 60 + 12  # twelve problems listed twice
    # crowded
    t = tables["crowded"]
    prob = dc.problems_of(t)
    assert len(prob) == 10000 and len(set(prob)) == 5000 and prob[:5000] == prob[5000:] and (dc.direct_places(t, 4, dc.NNODES, lay) < 0).all()
    assert dc.table_mask(10000, 1 << 14, 8, lay) == 1023 and dc.table_mask(10000, 1 << 14, 1, lay) == 8191  # (10,000 >> 1 is above 4,096)


def test_own_holes_and_threshold_designs(lay, tables):
    t = tables["own"]
    assert (t["rec_w0"] == 0).tolist() == [False, True, True, False, False, True, True, True, False, True, False]
    assert t["rec_hist"][1].tolist() == [300, 0, 0, 0, 0] and t["rd_onmers"][1] == 70000
    for end in (255, 256, 257):
        t = tables[f"holes_{end}"]
        inr, _ = dc.in_read(t)
        gaps = [int(t["rd_off"][r + 1] - t["rd_off"][r] - t["rd_cnt"][r]) for r in range(3)]
        assert gaps == [1, 63, 64] and len(inr) == end and inr[-1] and (t["rec_key"][~inr] == 0).all() and (t["rec_key"][inr] != 0).all()
        pl = dc.direct_places(t, 4, dc.NNODES, lay)
        assert (pl >= 0).any() and ((pl < 0) & inr).any()
    for th in (2, 6):
        t = dc.design_th_other(lay, th)
        assert (t["rec_w0"] == 0).all() and t["rec_hist"].shape == (257, th + 1)
        assert (dc.direct_places(t, th, dc.NNODES, lay) < 0).all()


def configs(lay, ix):
    return dict(default=cfg_of(lay, ix), direct_off=cfg_of(lay, ix, dd_nodes=0), shift8=cfg_of(lay, ix, dd_shift=8))


def test_check_accepts_the_sequential_model(lay, ix, tables):
    for cname, cfg in configs(lay, ix).items():
        for name, t in list(tables.items()) + [("all", dc.concat(list(tables.values())))]:
            m = dc.model(t, cfg, dc.fake_brent, table_room=2048)
            f = dc.check(t, m, cfg, dc.fake_brent, allow_excess=False, what=(cname, name))
            assert f["holes"] == 0 and f["listed"] == f["problems"]
            if name == "beyond_48":
                assert f["excess"] == 60 - lay["probe_rounds"] and f["absent"] == 60 - lay["probe_rounds"]
            elif name == "one_wave_same_problem":
                assert f["excess"] == 0 and f["absent"] == 64 - lay["probe_rounds"]
            elif name != "all" and not (cname == "shift8" and name == "crowded"):  # (in one batch the long chains of two designs meet)
                assert f["excess"] == 0 and f["absent"] == 0, (cname, name, f)
            if cname == "direct_off":
                assert f["direct"] == 0 and not (m["rec_rep"][m["rec_rep"] != dc.HOLE] & dc.FLAG).any()
    for th in (2, 6):
        cfg = cfg_of(lay, ix, th=th)
        t = dc.design_th_other(lay, th)
        f = dc.check(t, dc.model(t, cfg, dc.fake_brent), cfg, dc.fake_brent)
        assert f["distinct"] == f["listed"] == int(dc.in_read(t)[0].sum()) and f["direct"] == 0 and f["in_table"] == 0


@pytest.fixture(scope="module")
def good(lay, ix, tables):
    t = dc.concat([tables[n] for n in ("classes", "same_word_other_leaf", "chain_wrap", "own", "holes_257")])
    cfg = cfg_of(lay, ix)
    m = dc.model(t, cfg, dc.fake_brent)
    dc.check(t, m, cfg, dc.fake_brent)
    return t, cfg, m


def rejected(good, match, change):
    t, cfg, m = good
    r = copy.deepcopy(m)
    change(t, cfg, r)
    with pytest.raises(AssertionError, match=match):
        dc.check(t, r, cfg, dc.fake_brent)


def test_check_accepts_holes_in_the_list(good):
    t, cfg, m = good
    r = copy.deepcopy(m)
    r["rep_list"][r["problems"]] = dc.HOLE
    r["problems"] += 1
    assert dc.check(t, r, cfg, dc.fake_brent)["holes"] == 1


def test_check_rejects_a_record_resolved_to_another_leafs_problem(good):
    def change(t, cfg, r):
        prob = dc.problems_of(t)
        w = dc.pack(dc.ev(0, 5), 130)
        i, j = [k for k, p in enumerate(prob) if p and p[0] == "p" and p[2] == w][:2]
        assert prob[i][1] != prob[j][1]
        r["rec_rep"][i] = r["rec_rep"][j]
    rejected(good, "1: record resolved to another problem", change)


def test_check_rejects_an_index_listed_twice(good):
    def change(t, cfg, r):
        r["rep_list"][3] = r["rep_list"][2]
    rejected(good, "2: a record listed twice", change)


def test_check_rejects_a_value_at_a_hole(good):
    def change(t, cfg, r):
        r["rep_list"][r["problems"]] = dc.HOLE
        r["rep_dv"][r["problems"]] = (0.25, -3.0)
        r["problems"] += 1
    rejected(good, "5: a value at a hole of the list", change)


def test_check_rejects_an_empty_slot_inside_a_chain(good):
    def change(t, cfg, r):
        tab, mask = r["dd_table"], r["mask"]
        for s in np.nonzero(tab[:mask + 1, 0])[0].tolist():
            f = dc.first_slot(int(tab[s, 0]), int(tab[s, 1]) & dc.M32, mask, cfg.lay)
            if f != s:
                tab[f] = 0
                return
        raise RuntimeError("no displaced entry in the model's table")
    rejected(good, "4: an empty slot inside a chain", change)


def test_check_rejects_a_position_at_a_place_nobody_names(good):
    def change(t, cfg, r):
        r["dd_direct"][int(np.nonzero(r["dd_direct"] == dc.HOLE)[0][0])] = 0
    rejected(good, "3: a place nobody names holds something", change)


def test_check_rejects_a_direct_problem_in_the_table(good):
    def change(t, cfg, r):
        pl = dc.direct_places(t, 4, cfg.dd_nodes, cfg.lay)
        i = int(np.nonzero(pl >= 0)[0][0])
        key, w = int(t["rec_key"][i]), int(t["rec_w0"][i])
        s = dc.first_slot(w, key >> 1, r["mask"], cfg.lay)
        while r["dd_table"][s, 0] != 0:
            s = (s + 1) & r["mask"]
        r["dd_table"][s] = (w, (key >> 1) | (int(r["dd_direct"][pl[i]]) + 1) << 32)
    rejected(good, "3: a direct problem in the table", change)


def test_check_rejects_a_value_that_is_not_the_problems(good):
    def change(t, cfg, r):
        r["rep_dv"][5, 0] = np.nextafter(r["rep_dv"][5, 0], 1.0)
    rejected(good, "5: ", change)


def test_check_rejects_a_direct_record_at_another_place(good):
    def change(t, cfg, r):
        pl = dc.direct_places(t, 4, cfg.dd_nodes, cfg.lay)
        i = int(np.nonzero(pl >= 0)[0][0])
        other = int(np.nonzero(r["dd_direct"] != dc.HOLE)[0][-1])
        assert other != pl[i]
        r["rec_rep"][i] = dc.FLAG | other
    rejected(good, "1: record resolved to another problem|3: a direct record at another place", change)
