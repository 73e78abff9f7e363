"""The designs of tests/place_craft.py on the CPU: every designed read sits on the boundary it names, judged from the records the oracle
returns and the constants the library reports (capi.place_layout), so a changed kPlLeaves, kPlNodes, kPlBlock, kPlChain, chained factor or
runs limit moves the designs or fails here; every route of place_read is predicted for reads on both sides of its boundary; and
place_craft.reference -- exact rationals, no routes -- gives the oracle's candidate nodes for every read of every design."""
from fractions import Fraction

import pytest

import place_craft as pc

THS = (4, 7, 8)


class World:
    def __init__(self, capi, po, root):
        self.capi, self.po, self.root = capi, po, root
        self.lay = capi.place_layout()
        self._d, self._rec, self._ev = {}, {}, {}

    def design(self, name):
        """(craft, placement tree, idx_to_pt, user Newick, index directory, oracle index with the placement tree set)"""
        if name not in self._d:
            cr, tree, idx, nwk = pc.build(name, self.lay)
            d = str(self.root / name.replace("/", "_"))
            cr.write(d)
            ox = self.po.Index(d)
            ox.set_placement_tree(nwk)
            self._d[name] = (cr, tree, idx, nwk, d, ox)
        return self._d[name]

    def records(self, name, th):
        if (name, th) not in self._rec:
            cr, _, _, _, _, ox = self.design(name)
            b, o, n = cr.batch()
            self._rec[(name, th)] = pc.records_of_oracle(ox.dist(b, o, n, self.po.params(hdist_th=th, collect=1))["accs"], len(n))
        return self._rec[(name, th)]

    def evaluate(self, name, th, tau, no_filter):
        key = (name, th, tau, no_filter)
        if key not in self._ev:
            cr, tree, idx, _, _, _ = self.design(name)
            self._ev[key] = pc.evaluate(cr, tree, idx, self.records(name, th), th, tau, no_filter, self.lay)
        return self._ev[key]

    def placed(self, name, th, tau, no_filter):
        """the oracle's placements with nothing filtered by the chi-square: per read {node: (d_llh, v_llh)}"""
        cr, _, _, _, _, ox = self.design(name)
        b, o, n = cr.batch()
        pl = ox.place(b, o, n, self.po.params(hdist_th=th, tau=tau, no_filter=no_filter, chisq=1e300))["placements"]
        got = [dict() for _ in n]
        for x in pl:
            got[int(x["read"])][int(x["edge"]) + 1] = (float(x["d_llh"]), float(x["v_llh"]))
        return got


@pytest.fixture(scope="module")
def world(capi, po, tmp_path_factory):
    return World(capi, po, tmp_path_factory.mktemp("place_craft"))


def test_layout_is_reported(capi):
    lay = capi.place_layout()
    assert set(lay) == set(capi.PLACE_LAYOUT) and all(v > 0 for v in lay.values())
    assert lay["leaves"] % 64 == 0 and lay["runs_leaves"] > lay["leaves"] and lay["chain"] > lay["chain_factor"] * 64
    assert list(capi.place_paths()) == list(capi.PLACE_WITNESSES)  # (no device: nothing was counted, nothing is touched)


@pytest.mark.parametrize("name", [n for n in pc.TREES if not n.endswith("/user")])
def test_every_design_sits_where_it_says(world, name):
    cr = world.design(name)[0]
    for gated in sorted({r.gated for r in cr.reads}):
        ev = world.evaluate(name, 4, 2, 0 if gated else 1)
        for rd, (q, p) in zip(cr.reads, ev):
            if rd.gated == gated:
                assert eval(rd.expect, dict(q=q, p=p, L=world.lay, Fraction=Fraction)) is True, (name, rd.name, rd.expect, {k: v for k, v in p.items() if v})


def test_the_user_tree_has_covered_nodes_that_are_no_candidates(world):
    """two leaves of the user tree carry names the index does not have: their parents have eff_nchildren < nchildren, reads reach them
    through the other children, and they are no candidates; the index leaves of those names are on no node"""
    cr, tree, idx = world.design("lad357/user")[:3]
    assert sum(1 for se in cr.tree.leaf_se if idx[se] == 0) == len(pc.USER_RENAME)
    short = {n for n in range(1, tree.nnodes + 1) if tree.kids[n] and tree.eff[n] < len(tree.kids[n])}
    assert len(short) == len(pc.USER_RENAME) and not any(tree.elig[n] for n in short)
    hit = [n for q, _ in world.evaluate("lad357/user", 4, 2, 1) if q for n in q["gate"] if n in short and n not in q["candidates"]]
    assert len(hit) >= 10 and set(hit) == short


def test_every_route_is_predicted_on_both_sides_of_its_boundary(world):
    lay = world.lay
    F, CAP, LL, LN, RL, B = (lay[k] for k in ("chain_factor", "chain", "leaves", "nodes", "runs_leaves", "block"))
    ps = []
    for name in pc.TREES:
        ps += [p for _, p in world.evaluate(name, 4, 2, 1)]
    has = lambda f: any(f(p) for p in ps if p.get("home"))
    # weights: walked at tot_chain = F nl, chained at F nl + 1; chained at the scratch's size, walked one beyond
    assert has(lambda p: p["walked_shallow"] and p["tot_chain"] == F * p["nl"]) and has(lambda p: p["chained"] and p["tot_chain"] == F * p["nl"] + 1)
    assert has(lambda p: p["chained"] and p["tot_chain"] == CAP and p["home"] == "lds") and has(lambda p: p["walked_deep"] and p["tot_chain"] == CAP + 1 and p["home"] == "lds")
    # the arrays' home by leaves and by ancestors
    assert has(lambda p: p["nl"] == LL and p["home"] == "lds") and has(lambda p: p["nl"] == LL + 1 and p["na"] <= LN and p["home"] == "inline")
    assert has(lambda p: p["na"] == LN and p["home"] == "lds") and has(lambda p: p["na"] == LN + 1 and p["nl"] <= LL and p["home"] == "inline")
    # runs
    assert has(lambda p: p["nl"] == RL and not p["runs_off"]) and has(lambda p: p["nl"] == RL + 1 and p["runs_off"])
    assert has(lambda p: p["nl"] == B and p["multi_block_lanes"] == 0) and has(lambda p: p["nl"] == 2 * B + 1 and p["multi_block_lanes"] > 0)
    # wide by count (255 | 256 at th = 4) and by th (7 | 8)
    assert has(lambda p: p["wide"]) and has(lambda p: not p["wide"])
    names = [r.name for r in world.design("lad2")[0].reads]
    by = dict(zip(names, world.evaluate("lad2", 4, 2, 1)))
    assert by["count255"][1]["wide"] == 0 and by["count256"][1]["wide"] == 1
    for th, wide in ((7, 0), (8, 1)):
        ev = pc.evaluate(*world.design("lad2")[:3], world.records("lad2", th), th, 2, 1, lay)
        assert all(p["wide"] == wide for (_, p), n in zip(ev, names) if p.get("home") and not n.startswith("count"))
    # the early exits: a single leaf, and the closest leaf's gate at 1 | 2
    assert any(p["single"] for p in ps)
    gated = dict(zip(names, world.evaluate("lad2", 4, 2, 0)))
    assert gated["gate_closest_1"][1]["tau_stopped"] == 1 and gated["gate_closest_2"][1]["tau_stopped"] == 0 and gated["gate_closest_2"][1]["home"] == "lds"
    # the same reads with the LDS limits lowered, and with the second launch
    cr, tree, idx = world.design("lad2")[:3]
    for big_first, home in ((True, "inline"), (False, "second")):
        ev = pc.evaluate(cr, tree, idx, world.records("lad2", 4), 4, 2, 1, lay, lds=(3, 8), big_first=big_first)
        homes = {n: p["home"] for (_, p), n in zip(ev, names)}
        assert homes["nl2"] == "lds" and homes["nl63"] == home and homes["chain_cap+0"] == home
        if big_first:  # the inline scratch is larger: the read one beyond kPlChain is chained there
            assert dict(zip(names, ev))["chain_cap+1"][1]["chained"] == 1


CASES = [(n, th) for n in pc.TREES for th in THS]


@pytest.mark.parametrize("name,th", CASES)
def test_reference_gives_the_oracles_candidates(world, name, th):
    """no_filter = 1 and a chi-square bound nothing fails: the placements are the candidates but the root.  With the gate on (tau 2 and 1)
    likewise.  No read is left out."""
    cr, tree = world.design(name)[:2]
    for tau, nf in ((2, 1), (2, 0), (1, 0)):
        ev, got = world.evaluate(name, th, tau, nf), world.placed(name, th, tau, nf)
        for rd, (q, _), g in zip(cr.reads, ev, got):
            want = set() if q is None else {c for c in q["candidates"] if q["single"] or c != tree.root}
            assert want == set(g), (name, th, tau, nf, rd.name, sorted(want ^ set(g))[:10])
        assert sum(len(g) for g in got) > len(cr.reads)


@pytest.mark.parametrize("name", pc.TREES)
def test_no_gate_sum_lies_near_the_gate(world, name):
    """A sum within 1e-6 of 1.0 that is not exactly 1 would make the candidate set depend on the rounding of the sum: no design has one
    (th 4, 7, 8; tau 1 and 2).  A sum of exactly 1 is allowed where it is exact in doubles too: a leaf's count, or weights that are all
    powers of two (the binary trees)."""
    cr, tree = world.design(name)[:2]
    for th in THS:
        for tau in (2, 1):
            for rd, (q, _) in zip(cr.reads, world.evaluate(name, th, tau, 1)):
                if q is None:
                    continue
                for node, g in q["gate"].items():
                    if g == 1:
                        ws = [w.denominator for (_, a), w in q["weight"].items() if a == node]  # (none: a leaf, whose sum is a count)
                        assert all(x & (x - 1) == 0 for x in ws), (name, rd.name, node)
                    else:
                        assert abs(float(g) - 1.0) > 1e-6, (name, th, tau, rd.name, node, float(g))


def test_oracle_v_llh_of_internal_candidates_is_within_the_cpu_margin(world):
    """v_llh of every internal placement of every design at th 4, 7, 8 -- of a read of more than 300 leaves the 50 nearest the root --
    against the objective in 256-bit arithmetic on the reference's exact problem at the oracle's d, in units of that problem's B
    (tests/llh_mp.py).  The worst ratio is printed; M_PLACE_CPU is that figure, and the device gets twice it (tests/test_gpu_place_craft.py)."""
    worst, n = 0.0, 0
    for name in pc.TREES:
        cr, tree = world.design(name)[:2]
        for th in THS:
            ev, got = world.evaluate(name, th, 2, 1), world.placed(name, th, 2, 1)
            for rd, (q, p), g in zip(cr.reads, ev, got):
                if q is None or q["single"]:
                    continue
                for node in pc.llh_nodes(q, tree, p["nl"], g):
                    worst, n = max(worst, pc.llh_ratio(q, node, th, *g[node])), n + 1
    print(f"oracle: worst |v_llh - f| / B over {n} internal candidates: {worst:.4f}")
    assert n > 1000 and worst <= pc.M_PLACE_CPU
