"""The routes of kr_acc_kernel_t's epilogues, each run by a read designed for it (tests/acc_craft.py) and each WITNESSED: streams run
under KR_DEBUG_SKIP=512, where the kernel counts the paths it enters (kr_debug_acc_paths), and every case asserts the counts predicted
from the plain reference's numbers (events, marked keys, live events, positions hit twice) and the layout the library reports -- next
to the records (equal to the plain reference and to the oracle), the rows and the per-strand hdist_filt.
tests/test_acc_craft_cpu.py checks, without a GPU, that the designs sit on their boundaries."""
import os

import numpy as np
import pytest

import acc_craft
from conftest import assert_rows_close, rows_of_oracle

pytestmark = pytest.mark.gpu

FAST = ("fast_entered", "fast_false_early", "fast_compact", "fast_false_compacted", "fast_big_read", "fast_one_batch", "fast_multi_batch",
        "fast_extra_batches", "fix_dup_calls", "gen_entered_1")


@pytest.fixture(scope="module")
def crafted(capi, po, tmp_path_factory):
    lay = capi.acc_layout(acc_craft.TH + 1)
    cr, reads = acc_craft.designs(lay)
    path = cr.write(str(tmp_path_factory.mktemp("acc_craft") / "ix"))
    hx = capi.HostIndex(path)
    return dict(lay=lay, cr=cr, reads=reads, hx=hx, dx=hx.upload(0), ox=po.Index(path), counts={})


def counts_of(c, reads, th=4, segs=1):
    """the plain reference of these reads, computed once per (read, threshold, form)"""
    out = []
    for r in reads:
        key = (r.name, th, segs)
        if key not in c["counts"]:
            c["counts"][key] = acc_craft.reference(c["cr"], [r.form_of(segs)], th)[0]
        out.append(c["counts"][key])
    return out


def stream(capi, c, monkeypatch, dbg, th=4, max_reads=512, max_records=1 << 18, dx=None):
    monkeypatch.setenv("KR_DEBUG_SKIP", str(dbg))
    return (dx or c["dx"]).stream(params=capi.default_params(hdist_th=th), max_reads=max_reads, max_bases=max_reads * 400, max_records=max_records)


def run_exact(capi, po, c, st, reads, th=4, segs=1, flags=None, oracle=True):
    """submit the reads; records, rows and readtaps against the plain reference and the oracle.  Returns (reference counts, path witnesses)."""
    flags = capi.KR_TAP_ACCS if flags is None else flags
    bases, offs = c["cr"].batch(reads, segs=segs)
    counts = counts_of(c, reads, th, segs)
    st.submit(bases, offs, flags)
    res = st.collect()
    if flags & capi.KR_TAP_ACCS:
        got = sorted(zip(res.rec_read.tolist(), res.rec_key.tolist(), [tuple(x) for x in res.rec_hist.tolist()]))
        assert got == sorted((i, key, hist) for i, n in enumerate(counts) for key, hist in n["records"].items())
    else:
        assert res.rec_hist is None
        assert sorted(zip(res.rec_read.tolist(), res.rec_key.tolist())) == sorted((i, key) for i, n in enumerate(counts) for key in n["records"])
    assert st.readtaps(len(reads)).tolist() == [n["hdist_filt"] for n in counts]
    assert res.read_onmers.tolist() == [n["onmers"] for n in counts]
    if oracle:
        ref = c["ox"].dist(bases, offs, None, po.params(collect=7, hdist_th=th))
        if flags & capi.KR_TAP_ACCS:
            acc = ref["accs"][ref["accs"]["passed"] == 1]
            assert got == sorted(zip(acc["read"].tolist(), ((acc["se"] << 1) | acc["strand"]).tolist(), [tuple(x[:th + 1]) for x in acc["hist"].tolist()]))
        assert_rows_close(res.rows(), rows_of_oracle(ref))
        assert st.readtaps(len(reads)).tolist() == ref["reads"]["hdist_filt"].tolist()
    return counts, st.acc_paths()


def predicted(c, counts):
    tot = dict.fromkeys(FAST, 0)
    for n in counts:
        p = acc_craft.predict_paths(n, c["lay"])
        for k in FAST:
            tot[k] += p[k]
    return tot


def assert_fast_paths(c, counts, paths):
    want = predicted(c, counts)
    assert {k: paths[k] for k in FAST} == want, paths
    assert paths["fix_dup_moved"] <= paths["fix_dup_calls"]
    assert paths["gen_entered_2"] == paths["gen_entered_merge"] == paths["gen_no_fit"] == paths["set_aside"] == paths["plane_redo"] == 0, paths


def test_every_design_alone_takes_its_route(capi, po, crafted, monkeypatch):
    """th = 4, one segment: each designed read as a batch of its own -- records exact, path witnesses exactly as predicted: the capacity
    edge (nev = E - 1 .. E + 257, all live and mostly droppable), compaction that does and does not suffice (768 / 772 / E live events),
    B(nev) keys and one more, three batches, positions hit twice and three times, finish_big_read with 63 .. 500 keys"""
    c = crafted
    st = stream(capi, c, monkeypatch, 512)
    assert c["lay"] == {**st.acc_layout(), "ev_spill": 0, "tab_spill": 0, "kt_spill": 0} and st.acc_layout()["ev_spill"] > 257
    routes = {}
    for r in c["cr"].reads:
        counts, paths = run_exact(capi, po, c, st, [r])
        assert_fast_paths(c, counts, paths)
        route = acc_craft.predict_paths(counts[0], c["lay"])["route"]
        routes[route] = routes.get(route, 0) + 1
        if r.name in ("dups_limit1", "batches_2", "batches_3"):
            assert paths["fix_dup_moved"] > 0, (r.name, paths)
        if route == "general":
            assert paths["gen_fused"] + paths["gen_sparse"] + paths["gen_extra_batches"] + paths["gen_big"] > 0, (r.name, paths)
    assert min(routes.get(k, 0) for k in ("one", "several", "big", "general")) >= 3, routes


def test_packed_word_alone(capi, po, crafted, monkeypatch):
    """without KR_TAP_ACCS a record is its key and the packed word: the routes write it themselves (finish_big_read from its planes)"""
    c = crafted
    st = stream(capi, c, monkeypatch, 512)
    reads = [r for r in c["cr"].reads if r.name.startswith(("big_", "batches_", "dups_", "compact_"))]
    for r in reads:
        counts, paths = run_exact(capi, po, c, st, [r], flags=0)
        assert_fast_paths(c, counts, paths)


def test_state_between_reads(capi, po, crafted, monkeypatch):
    """one batch of 288 reads: a wave takes 8 consecutive reads, every chunk alternates a heavy read of each route with light reads; the
    batch twice on one stream.  A bitmap word, position map or global plane that a route leaves behind shows in its neighbour."""
    c = crafted
    light = c["reads"]["light"]
    heavy = [r for r in c["cr"].reads if r is not light]
    # (neighbours change from chunk to chunk: the heavy reads advance by 5 a step)
    reads = [x for i in range(144) for x in (heavy[(5 * i) % len(heavy)], light)]
    assert len(heavy) % 5 and len(reads) >= 256 and {r.name for r in reads} == set(c["reads"])
    st = stream(capi, c, monkeypatch, 512)
    for again in range(2):
        counts, paths = run_exact(capi, po, c, st, reads, oracle=again == 0)
        assert_fast_paths(c, counts, paths)


def test_flat_colours_listed_and_walked(capi, po, crafted, monkeypatch):
    """the same index with its colours as runs of leaf ranks and leaf lists (default), with lists of at most 4 leaves, and with every
    colour walked through its parts: identical records (the colours of 60 .. 250 leaves are chains of pair colours over clades)"""
    c = crafted
    try:
        os.environ["KR_FLAT_MAX"] = "0"
        dx_walk = c["hx"].upload(0)
        os.environ["KR_FLAT_MAX"] = "4"
        dx_mix = c["hx"].upload(0)
    finally:
        del os.environ["KR_FLAT_MAX"]
    for dx in (dx_walk, dx_mix):
        st = stream(capi, c, monkeypatch, 512, dx=dx)
        counts, paths = run_exact(capi, po, c, st, c["cr"].reads, oracle=False)
        assert_fast_paths(c, counts, paths)
        st.close()


@pytest.mark.parametrize("name", ["edge_drop_+0", "batches_3", "big_64", "compact_772"], ids=["one_batch", "several_batches", "big_read", "general"])
def test_record_room(capi, po, crafted, monkeypatch, name):
    """a stream whose max_records is too small for the read: KR_ERR_CAPACITY, never truncated records, whichever route writes them; the
    next batch on the same stream, which fits, is exact"""
    c = crafted
    st = stream(capi, c, monkeypatch, 512, max_records=8)
    r = c["reads"][name]
    assert counts_of(c, [r])[0]["nkeys"] > 8
    bases, offs = c["cr"].batch([r])
    st.submit(bases, offs, capi.KR_TAP_ACCS)
    with pytest.raises(capi.KrError) as e:
        st.collect()
    assert e.value.code == capi.KR_ERR_CAPACITY
    counts, paths = run_exact(capi, po, c, st, [c["reads"]["light"]] * 2)
    assert_fast_paths(c, counts, paths)


def test_other_instantiations(capi, po, crafted, monkeypatch):
    """the same designed reads through the general epilogue (th = 3 and th = 6: PB = 7), lengthened to two segments (PB = 8) and to three
    (merge), and through the plane tables (bits 8 and 8192): expected values recomputed by the reference; each class of finalize_events
    counted exactly, and every form of it witnessed somewhere in the set"""
    c = crafted
    all_reads = c["cr"].reads
    seen = dict.fromkeys(("gen_fused", "gen_sparse", "gen_extra_batches", "gen_big", "gen_keytab_global", "set_aside"), 0)

    def go(dbg, th, segs=1, reads=all_reads):
        st = stream(capi, c, monkeypatch, 512 + dbg, th=th)
        counts, paths = run_exact(capi, po, c, st, reads, th=th, segs=segs)
        st.close()
        for k in seen:
            seen[k] += paths[k]
        return sum(n["nev"] > 0 for n in counts), paths

    for th, dbg in ((3, 0), (3, 2048), (6, 0), (4, 4096)):  # one segment, general epilogue
        nz, p = go(dbg, th)
        assert p["gen_entered_1"] == nz == len(all_reads) and p["gen_entered_2"] == p["gen_entered_merge"] == 0, (th, dbg, p)
        # (a forced bit keeps the straight-line epilogue out; without one it is entered and hands every read on)
        assert (p["fast_entered"], p["fast_false_early"]) == ((len(all_reads),) * 2 if dbg == 0 else (0, 0)), (th, dbg, p)
        assert p["gen_no_fit"] == p["set_aside"] == p["plane_redo"] == 0, (th, dbg, p)
        if dbg == 2048:
            assert p["gen_big"] > 0, p
        if th == 3 and dbg == 0:
            assert p["gen_sparse"] > 0 and p["gen_fused"] > 0 and p["gen_extra_batches"] > 0, p
        if th == 6:
            assert p["gen_keytab_global"] > 0, p
    for th in (4, 3):  # two segments: every read set aside by the first launch, finished by the second
        nz, p = go(0, th, segs=2)
        assert p["set_aside"] == len(all_reads) and p["fast_entered"] == p["gen_entered_1"] == 0, (th, p)
        # (finalize_events<PB = 8> leaves a read to the merge launch -- which finds events in its first segment only -- if its keys need
        #  more than 16 LDS batches of 256-bit planes and more than the wave's global planes hold: big_500)
        lay2, kw = capi.acc_layout(th + 1, 2), (th + 1) * 8

        def left_over(n):
            behind = lay2["ev_words"] - ((((min(n["nev"], lay2["ev_cap"]) + 1) & ~1) + n["nkeys"] + 3) & ~3)  # words behind events and key table
            return n["nkeys"] > 16 * (behind // kw) and n["nkeys"] * kw > 2 * acc_craft.NLEAF * (th + 1) * 4

        over = sum(left_over(n) for n in counts_of(c, all_reads, th, 2))
        assert over == 1 and p["gen_entered_2"] == nz and p["gen_entered_merge"] == p["gen_no_fit"] == over and p["plane_redo"] == 0, (th, p)
    nz, p = go(0, 4, segs=3)  # three segments: the merge instantiation, one call per segment with events (all in the first)
    assert p["set_aside"] == len(all_reads) and p["fast_entered"] == p["gen_entered_1"] == p["gen_entered_2"] == 0, p
    assert p["gen_entered_merge"] == nz and p["plane_redo"] == 0, p
    nz, p = go(8, 4)  # no event mode: the plane tables
    assert p["set_aside"] == len(all_reads) and p["fast_entered"] == p["gen_entered_1"] == p["gen_entered_2"] == p["gen_entered_merge"] == 0, p
    nz, p = go(8192, 4, segs=2)  # ... for reads of several segments
    assert p["set_aside"] == len(all_reads) and p["fast_entered"] == p["gen_entered_1"] == p["gen_entered_2"] == p["gen_entered_merge"] == 0, p
    assert all(seen.values()), seen
