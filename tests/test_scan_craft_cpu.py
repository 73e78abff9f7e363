"""The crafted tables of tests/scan_craft.py, checked without a GPU: the plain reference agrees with the oracle on every geometry, and
every designed read sits on the boundary it was designed for -- evaluated from the reference's counts and the layout numbers the library
reports (kr_debug_scan_layout), for every table layout the scan kernels serve.  A changed constant moves the designs or fails here; it
cannot quietly leave a path of the scan without a read (tests/test_gpu_scan_tables.py runs the same tables on the GPU)."""
import pytest

import scan_craft

LAYOUTS = [(0, 0), (0, 2), (0, 3), (5, 0), (6, 0), (7, 0), (8, 0), (9, 0)]  # (slot format, log_g)
GEOS = ("one", "two", "half")


@pytest.fixture(scope="module")
def crafts(capi):
    made = {}

    def get(fmt, log_g, geo):
        key = (fmt, log_g, geo)
        if key not in made:
            cr = scan_craft.designs(capi.scan_layout(fmt, log_g), geo)
            made[key] = (cr, scan_craft.reference(cr, [r.seq for r in cr.reads]))
        return made[key]

    return get


def test_layout_numbers(capi):
    """one source for the kernels and the host: the shapes with_scan_shape picks, and what follows from them"""
    for fmt, log_g in LAYOUTS:
        l = capi.scan_layout(fmt, log_g)
        assert l["G"] * l["PPS"] == 64 and l["list_cap"] == 128 == 2 * 64 and l["seg_pos"] == 128 and l["read_chunk"] <= 64
        assert l["item_stage"] % 16 == 0 and l["item_chunk"] % 16 == 0 and l["item_chunk"] > l["item_stage"]
        if fmt == 0:
            assert l["G"] == 1 << log_g and not l["slotted"] and l["W"] == l["CAP"] == 0
            assert l["step_bits"] == 64 // l["CPL"] * l["CPL"] and l["step_bits"] % l["CPL"] == 0
        elif fmt == 9:
            assert (l["line_codes"], l["slot_codes"], l["CAP"]) == (40, 80, 80) and l["G"] * l["CPL"] * 5 == l["line_codes"] and l["W"] == 64
        else:
            assert l["W"] == 4 * l["G"] * l["CPL"] == {5: 32, 6: 64, 7: 128, 8: 48}[fmt] and l["CAP"] == l["W"] - 2
        if l["slotted"]:  # one hit bit per (pass, chunk) of a full list
            assert l["step_bits"] == l["list_cap"] // l["PPS"] * l["CPL"] <= 64
    assert capi.scan_layout(7)["step_bits"] == 64  # the one shape that uses all 64 hit bits
    assert capi.scan_layout(0, 0) != capi.scan_layout(0, 2) != capi.scan_layout(0, 3)
    for bad in ((4, 0), (10, 0), (0, 1), (0, 4)):
        with pytest.raises(capi.KrError):
            capi.scan_layout(*bad)


@pytest.mark.parametrize("th", [0, 4, 16])
@pytest.mark.parametrize("geo,fmt,log_g", [("one", 6, 0), ("two", 0, 2), ("half", 9, 0), ("two", 7, 0), ("one", 0, 0)],
                         ids=["one_slots", "two_packed", "half_filter", "two_wide_slots", "one_sparse_shape"])
def test_reference_equals_oracle(crafts, po, tmp_path, geo, fmt, log_g, th):
    cr, _ = crafts(fmt, log_g, geo)
    ox = po.Index(cr.write(str(tmp_path / "ix")))
    bases, offs = cr.batch()
    ref = ox.dist(bases, offs, None, po.params(collect=7, hdist_th=th))
    mine = scan_craft.reference(cr, [r.seq for r in cr.reads], th)
    got = sorted((i,) + h for i, c in enumerate(mine) for h in c["hits"])
    h = ref["hits"]
    want = sorted(zip(h["read"].tolist(), h["strand"].tolist(), h["kpos"].tolist(), h["lib"].tolist(), h["cmer_index"].tolist(), h["hd"].tolist(), h["se"].tolist()))
    assert got == want and len(got) > (3000 if th == 16 else 50 if th == 0 else 1000)  # (the comparison is not empty)
    assert [c["hdist_filt"] for c in mine] == ref["reads"]["hdist_filt"].tolist()
    assert [c["onmers"] for c in mine] == ref["reads"]["onmers"].tolist()
    ox.close()


@pytest.mark.parametrize("geo", GEOS)
@pytest.mark.parametrize("fmt,log_g", LAYOUTS, ids=[f"fmt{f}_g{g}" for f, g in LAYOUTS])
def test_every_design_is_on_its_boundary(crafts, fmt, log_g, geo):
    cr, counts = crafts(fmt, log_g, geo)
    assert len({r.name for r in cr.reads}) == len(cr.reads)
    for r, c in zip(cr.reads, counts):
        assert r.expect and scan_craft.check(cr, r, c), (r.name, r.expect, r.probes[:3], {k: v for k, v in c.items() if k != "hits"})


@pytest.mark.parametrize("fmt,log_g", LAYOUTS, ids=[f"fmt{f}_g{g}" for f, g in LAYOUTS])
def test_the_designs_reach_the_lists(crafts, capi, fmt, log_g):
    """what the geometries reach together, per layout: the probe counts of a group, the item counts of a read, the start alignments of
    the buckets that give a hit, the tail alignments, the hit ordinals at the layout's edges, the packed indexes 0 and 1"""
    lay = capi.scan_layout(fmt, log_g)
    PPS, CAP, STAGE, CHUNK = lay["PPS"], lay["CAP"], lay["item_stage"], lay["item_chunk"]
    nact, items, starts, tails, ords, lens, index = set(), set(), set(), set(), set(), set(), set()
    for geo in GEOS:
        cr, counts = crafts(fmt, log_g, geo)
        for c in counts:
            nact |= set(scan_craft.nact_of(c, lay))
            items.add(c["items"])
            index |= {h[3] for h in c["hits"]}
            for key, os_ in c["hit_ords"].items():
                start, n = c["probed"][key]
                starts.add(start & 3)
                lens.add(n)
                ords |= {o for o in os_ if o <= max(CAP + 1, 2)} | {"last" for o in os_ if o == n - 1}
                if lay["slotted"] and n > CAP:
                    tails.add((start + CAP) & 3)
                    ords |= {"tail_first" for o in os_ if o == CAP} | {"slot_last" for o in os_ if o == CAP - 1}
    assert nact >= {0, 1, PPS - 1, PPS, PPS + 1, lay["list_cap"]} - ({PPS - 1, PPS + 1} if PPS == 64 and lay["slotted"] else set()), sorted(nact)
    if not lay["slotted"]:
        assert lay["list_cap"] - 1 in nact  # (an odd count of a full group: packed tables only, where an empty row is not listed)
    assert items >= {0, 1, STAGE - 1, STAGE, STAGE + 1} and max(items) > CHUNK + STAGE
    assert starts == {0, 1, 2, 3} and {0, 1} <= index and ords >= {0, 1, 2, "last"}
    if lay["slotted"]:
        assert tails == {0, 1, 2, 3} and ords >= {"slot_last", "tail_first"} and lens >= {1, 2, 3, CAP - 1, CAP, CAP + 1, CAP + 2, CAP + 3, CAP + 4, CAP + 5}
        assert max(lens) > CAP + 4 * lay["G"] and max(lens) >= CAP + 200
        if lay["line_codes"]:
            assert lens >= {39, 40, 41, 79, 80, 81}
    else:
        E, F = 4 * lay["G"] * lay["CPL"], lay["step_bits"] // lay["CPL"]
        assert lens >= set(range(1, 10)) | {E - 1, E, E + 1, 2 * E + 1, E * (F - 1)} and max(lens) > E * F
