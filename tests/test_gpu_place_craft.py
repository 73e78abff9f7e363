"""Every route of the per-read kernel of `place` (place_read, kr_dev_place.inc) on the crafted trees and reads of tests/place_craft.py.

Per tree (the binary ladder, the ladder with rungs of 3, 5, 7 children, the same under a user tree with uncovered children, the balanced
tree of 8,192 leaves), hdist_th in (4, 7, 8) -- th = 4 runs the <.., 5> instantiations, the others <.., 0>, and th = 8 re-reads the
histograms -- and the option sets {}, multi=0, tau=1 chisq=3.841 and nothing filtered, in jplace, tabular and --summarize:

  device back end = host back end     text, placement records and summary byte for byte; also with the text written on the device
  device = oracle                      text byte for byte, the same (read, edge) keys
  device = exact reference             the node sets of place_craft.reference under options that filter nothing; v_llh of the internal
                                       candidates within M_PLACE_GPU B of the objective in 256-bit arithmetic at the device's d
  witnesses                            under KR_DEBUG_PLACE_PATHS=1 the counts place_craft.predict_paths gives from the tapped records,
                                       with the arrays in LDS, inline in global scratch (KR_DEBUG_PLACE_LDS lowered), in the second launch
                                       (KR_PLACE_BIG_FIRST=0; KR_PLACE_HEAVY_GLOBAL=1) -- and the same bytes as without the knob,
                                       where every witness stays 0

The witnesses are those of the WIT instantiations of kr_place_kernel (docs/design/06_place.md), counted where the paths run; what those
kernels compute is held to the unwitnessed kernels' bytes here.  No tolerance but the v_llh margin, which tests/test_place_craft_cpu.py sets from the oracle."""
import numpy as np
import pytest

import place_craft as pc

pytestmark = pytest.mark.gpu

THS = (4, 7, 8)
UNFILTERED = dict(no_filter=1, chisq=1e300)
# (with the default chi-square bound a read keeps the few candidates next to its closest leaf: a wrong weight far up the tree, or a wrong
#  histogram of an ancestor, shows only where nothing is filtered -- the ladders run that too, in every mode)
OPTS = {"default": {}, "no-multi": dict(multi=0), "tau1": dict(tau=1, chisq=3.841), "unfiltered": UNFILTERED}
MODES = {"jplace": 0, "tabular": 1, "summary": 2}
ENVS = {"lds": {}, "inline": {"KR_DEBUG_PLACE_LDS": "3,8"}, "second": {"KR_DEBUG_PLACE_LDS": "3,8", "KR_PLACE_BIG_FIRST": "0"},
        "second/global": {"KR_DEBUG_PLACE_LDS": "3,8", "KR_PLACE_BIG_FIRST": "0", "KR_PLACE_HEAVY_GLOBAL": "1"}}
MAX_RECORDS = 1 << 16  # the balanced tree's reads of 4,096 and 4,097 leaves: beyond 128 records a read


class World:
    def __init__(self, capi, po, root):
        self.capi, self.po, self.root = capi, po, root
        self.lay = capi.place_layout()
        self._d, self._o, self._ev = {}, {}, {}

    def design(self, name):
        if name not in self._d:
            cr, tree, idx, nwk = pc.build(name, self.lay)
            d = str(self.root / name.replace("/", "_"))
            cr.write(d)
            self._d[name] = dict(cr=cr, tree=tree, idx=idx, nwk=nwk, dir=d, hx=self.capi.HostIndex(d), batch=cr.batch())
        return self._d[name]

    def placer(self, name, th, tabular, **opts):
        D = self.design(name)
        b, o, n = D["batch"]
        opts = dict(opts)
        no_filter = opts.pop("no_filter", 0)
        pl = self.capi.Placer(D["hx"], D["nwk"], 0, tabular=tabular, max_reads=len(n), max_bases=len(b), max_records=MAX_RECORDS, hdist_th=th, **opts)
        pl.popts.no_filter = no_filter
        return pl

    def run(self, name, th, tabular, want_pl=True, host=False, **opts):
        """(text, placement bytes, summary) of one call on a new Placer"""
        pl = self.placer(name, th, tabular, **opts)
        b, o, n = self.design(name)["batch"]
        text, p = pl.place(b, o, n, host=host, want_placements=want_pl)
        out = (text, p.tobytes() if want_pl else b"", pl.summary() if tabular == 2 and want_pl else "")
        pl.close()
        return out

    def oracle(self, name, th, tabular, **opts):
        """(text or summary, sorted (read, edge) keys or None)"""
        key = (name, th, tabular, tuple(sorted(opts.items())))
        if key not in self._o:
            D = self.design(name)
            b, o, n = D["batch"]
            ox = self.po.Index(D["dir"])
            ox.set_placement_tree(D["nwk"])
            okw = dict(no_filter=0, hdist_th=th)
            okw.update(opts)
            if tabular == 2:
                self._o[key] = (ox.place_summarize(b, o, self.po.params(**okw)), None)
            else:
                r = ox.place(b, o, n, self.po.params(**okw), tabular=bool(tabular))
                self._o[key] = (r["text"], sorted((int(a), int(e)) for a, e in zip(r["placements"]["read"], r["placements"]["edge"])))
            ox.close()
        return self._o[key]

    def tapped(self, name, th):
        """the records of the batch as the Placer's front end leaves them"""
        key = (name, th)
        if key not in self._ev:
            pl = self.placer(name, th, 0)
            b, o, n = self.design(name)["batch"]
            pl.st.submit(np.ascontiguousarray(b, dtype=np.uint8), np.ascontiguousarray(o, dtype=np.uint64), self.capi.KR_TAP_ACCS)
            self._ev[key] = pc.records_of_result(pl.st.collect(), th)
            pl.close()
        return self._ev[key]

    def evaluate(self, name, th, tau, no_filter, lds=None, big_first=True):
        key = (name, th, tau, no_filter)
        D = self.design(name)
        if key not in self._ev:
            self._ev[key] = pc.evaluate(D["cr"], D["tree"], D["idx"], self.tapped(name, th), th, tau, no_filter, self.lay)
        ev = self._ev[key]
        if lds is None and big_first:
            return ev
        return [(q, pc.predict_paths(q, D["tree"], self.lay, th, lds, big_first)) for q, _ in ev]


@pytest.fixture(scope="module")
def world(capi, po, tmp_path_factory):
    return World(capi, po, tmp_path_factory.mktemp("place_craft_gpu"))


CASES = [(n, th) for n in pc.TREES for th in THS]


@pytest.mark.parametrize("mname", list(MODES))
@pytest.mark.parametrize("oname", list(OPTS))
@pytest.mark.parametrize("name,th", CASES)
def test_device_host_and_oracle_agree_byte_for_byte(world, name, th, oname, mname):
    opts, tabular = OPTS[oname], MODES[mname]
    host = world.run(name, th, tabular, host=True, **opts)
    dev = world.run(name, th, tabular, **opts)
    assert dev == host
    assert len(host[0]) + len(host[1]) > 0
    otext, okeys = world.oracle(name, th, tabular, **opts)
    assert (dev[2] if tabular == 2 else dev[0]) == otext
    if okeys is not None:
        p = np.frombuffer(dev[1], dtype=world.capi.PLACEMENT_DT)
        assert sorted((int(a), int(e)) for a, e in zip(p["read"], p["edge"])) == okeys
    if tabular != 2:  # the rows written on the device
        assert world.run(name, th, tabular, want_pl=False, **opts)[0] == host[0]


@pytest.mark.parametrize("name,th", CASES)
def test_device_candidates_are_the_exact_references(world, name, th):
    """Nothing filtered: the placements are the candidates but the root.  Node sets equal place_craft.reference's on the device's own
    records; v_llh of every internal candidate (of a read of more than 300 leaves: the 50 nearest the root) within M_PLACE_GPU B of the objective in 256-bit arithmetic on
    the exact accumulated problem, at the device's d."""
    D = world.design(name)
    dev = world.run(name, th, 0, **UNFILTERED)
    assert dev == world.run(name, th, 0, host=True, **UNFILTERED)
    p = np.frombuffer(dev[1], dtype=world.capi.PLACEMENT_DT)
    got = [dict() for _ in D["cr"].reads]
    for x in p:
        got[int(x["read"])][int(x["edge"]) + 1] = (float(x["d_llh"]), float(x["v_llh"]))
    worst, n = 0.0, 0
    for rd, (q, pp), g in zip(D["cr"].reads, world.evaluate(name, th, 2, 1), got):
        want = set() if q is None else {c for c in q["candidates"] if q["single"] or c != D["tree"].root}
        assert want == set(g), (name, th, rd.name, sorted(want ^ set(g))[:10])
        if q is None or q["single"]:
            continue
        for node in pc.llh_nodes(q, D["tree"], pp["nl"], g):
            worst, n = max(worst, pc.llh_ratio(q, node, th, *g[node])), n + 1
    print(f"device: {name} th {th}: worst |v_llh - f| / B over {n} internal candidates: {worst:.4f}")
    assert n > 100 and worst <= pc.M_PLACE_GPU, (name, th, worst)


def witnessed(world, monkeypatch, name, th, env, **opts):
    """one call under KR_DEBUG_PLACE_PATHS=1 and `env`: (output, what the witnesses moved by)"""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    monkeypatch.setenv("KR_DEBUG_PLACE_PATHS", "1")
    w0 = world.capi.place_paths()
    out = world.run(name, th, 0, **opts)
    w1 = world.capi.place_paths()
    monkeypatch.delenv("KR_DEBUG_PLACE_PATHS")
    z0 = world.capi.place_paths()
    plain = world.run(name, th, 0, **opts)
    assert world.capi.place_paths() == z0, "witnesses moved without the knob"
    for k in env:
        monkeypatch.delenv(k)
    assert out == plain, "the witnessed kernels' output differs"
    return out, {k: w1[k] - w0[k] for k in w1}


WITNESS_CASES = [(n, th, e) for n in ("lad2", "lad357", "lad357/user") for th in (4, 8) for e in ENVS if th == 4 or e in ("lds", "inline")]
WITNESS_CASES += [("bal", 4, e) for e in ENVS] + [("bal", 8, "lds")]


@pytest.mark.parametrize("name,th,env", WITNESS_CASES)
def test_every_predicted_route_leaves_its_witness(world, monkeypatch, name, th, env):
    lds = tuple(int(x) for x in ENVS[env]["KR_DEBUG_PLACE_LDS"].split(",")) if "KR_DEBUG_PLACE_LDS" in ENVS[env] else None
    big_first = ENVS[env].get("KR_PLACE_BIG_FIRST") != "0"
    for opts, tau, nf in ((UNFILTERED, 2, 1), ({}, 2, 0)):
        out, moved = witnessed(world, monkeypatch, name, th, ENVS[env], **opts)
        assert out == world.run(name, th, 0, host=True, **opts)
        want = dict.fromkeys(world.capi.PLACE_WITNESSES, 0)
        for _, p in world.evaluate(name, th, tau, nf, lds, big_first):
            for k in want:
                want[k] += p[k]
        assert moved == want, (name, th, env, nf)


def test_the_witnesses_cover_every_route(world, monkeypatch):
    """What the issue of this suite asks to see non-zero, over the cases above: chained; walked, shallow and beyond the scratch; wide by
    count and by th; runs off; multi-block runs; each home; the early exits.  (No design reaches a dropped duplicate: see
    docs/design/06_place.md.)"""
    _, a = witnessed(world, monkeypatch, "lad2", 4, {}, **UNFILTERED)
    assert all(a[k] > 0 for k in ("chained", "walked_shallow", "walked_deep", "wide", "single", "home_lds", "multi_block_lanes")), a
    assert a["wide"] == 1 and a["runs_off"] == 0 and a["home_inline"] == 0 and a["home_second"] == 0 and a["dup_dropped"] == 0, a
    _, g = witnessed(world, monkeypatch, "lad2", 4, {})
    assert g["tau_stopped"] > 0, g
    _, b = witnessed(world, monkeypatch, "lad2", 8, {}, **UNFILTERED)
    assert b["wide"] == b["home_lds"] > 1, b
    _, c = witnessed(world, monkeypatch, "bal", 4, {}, **UNFILTERED)
    assert c["runs_off"] == 1 and c["home_inline"] == 4 and c["walked_deep"] == 2, c
    _, d = witnessed(world, monkeypatch, "lad2", 4, ENVS["second"], **UNFILTERED)
    assert d["home_second"] > 0 and d["home_inline"] == 0, d
