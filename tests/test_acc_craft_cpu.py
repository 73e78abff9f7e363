"""The designed reads of tests/acc_craft.py, checked without a GPU: the plain reference agrees with the oracle on every read, and every
read sits on the boundary it was designed for -- evaluated from the reference's counts and the layout numbers the library reports
(kr_debug_acc_layout), so a changed layout constant moves the designs or fails here; it cannot quietly leave a route of
kr_acc_kernel_t without a read (tests/test_gpu_acc_paths.py runs the same reads on the GPU)."""
import numpy as np
import pytest

import acc_craft


@pytest.fixture(scope="module")
def crafted(capi, po, tmp_path_factory):
    lay = capi.acc_layout(acc_craft.TH + 1)
    cr, reads = acc_craft.designs(lay)
    ox = po.Index(cr.write(str(tmp_path_factory.mktemp("acc_craft") / "ix")))
    return lay, cr, reads, ox


def oracle_records(po, ox, bases, offs, th):
    ref = ox.dist(bases, offs, None, po.params(collect=7, hdist_th=th))
    acc = ref["accs"][ref["accs"]["passed"] == 1]
    return ref, sorted(zip(acc["read"].tolist(), ((acc["se"] << 1) | acc["strand"]).tolist(), [tuple(x[:th + 1]) for x in acc["hist"].tolist()]))


def test_layout_numbers(capi):
    """the layout the designs are derived from: one function for the kernel and the host"""
    lay = capi.acc_layout(5)
    assert lay["key_words"] == 7 and lay["ev_cap"] < lay["ev_words"] and lay["ev_cap"] % 128 == 0  # (finish_big_read needs whole 128-event tiles)
    for np_planes in (1, 4, 5, 7):
        for segs, multi in ((1, 0), (2, 0), (1, 1)):
            l = capi.acc_layout(np_planes, segs, multi)
            assert 64 <= l["ev_cap"] < l["ev_words"] and l["ev_cap"] % 64 == 0
    assert capi.acc_layout(5, 2)["ev_words"] >= lay["ev_words"]
    with pytest.raises(capi.KrError):
        capi.acc_layout(0)


def test_tree_numbering_is_the_index_s(crafted):
    lay, cr, reads, ox = crafted
    t = cr.tree
    assert ox.info.nnodes == t.nnodes and ox.info.nleaves == t.nleaf
    assert all(ox.name(se) == t.names[se] and ox.kind(se) == t.kind[se] for se in range(1, t.nnodes + 1))


@pytest.mark.parametrize("th,segs", [(4, 1), (3, 1), (6, 1), (4, 2), (3, 2), (4, 3)], ids=["th4", "th3", "th6", "th4_two_segments", "th3_two_segments", "th4_three_segments"])
def test_reference_equals_oracle(crafted, po, th, segs):
    lay, cr, reads, ox = crafted
    bases, offs = cr.batch(segs=segs)
    assert all((len(r.form_of(segs)) - acc_craft.K) // 128 + 1 == segs for r in cr.reads)
    seqs = [r.form_of(segs) for r in cr.reads]
    mine = acc_craft.reference(cr, seqs, th)
    ref, want = oracle_records(po, ox, bases, offs, th)
    got = sorted((i, key, hist) for i, c in enumerate(mine) for key, hist in c["records"].items())
    assert got == want and len(got) > 1000
    assert [c["hdist_filt"] for c in mine] == ref["reads"]["hdist_filt"].tolist()
    assert [c["onmers"] for c in mine] == ref["reads"]["onmers"].tolist()


def test_every_read_is_on_its_boundary(crafted):
    lay, cr, reads, ox = crafted
    counts = acc_craft.reference(cr, [r.seq for r in cr.reads])
    E, W = lay["ev_cap"], lay["ev_words"]
    B = lambda n: acc_craft.batch_keys(lay, n)
    routes = set()
    for r, c in zip(cr.reads, counts):
        p = acc_craft.predict_paths(c, lay)
        route = p["route"]
        routes.add(route)
        assert c["nev"] == r.nplanned, (r.name, "a chance neighbour in a bucket: choose another seed")
        assert c["nev"] <= E + lay["ev_spill"] if lay["ev_spill"] else True
        assert eval(r.expect, dict(c=c, p=p, route=route, E=E, W=W, B=B, len=len)), (r.name, r.expect, {k: v for k, v in c.items() if k not in ("records", "per_key")}, p)
    assert routes == {"one", "several", "big", "general"}
    # a twice-hit position in a later key batch, both bucket orders, hd 4, both strands, positions 0 and 127, side by side and apart
    groups = [(k_, pos, h) for c in counts for k_, pos, h in c["groups"]]
    assert {tuple(h) for _, _, h in groups} >= {(0, 1), (1, 0), (2, 2), (0, 4)} and {k_ & 1 for k_, _, _ in groups} == {0, 1}
    assert {pos for _, pos, _ in groups} >= {0, 127}
    assert {tuple(sorted(h)) for _, _, h in groups} >= {(0, 1), (2, 2), (0, 1, 3), (0, 4, 4), (2, 4, 4)}
