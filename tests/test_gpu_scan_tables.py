"""Every table layout of the scan at its bucket boundaries, on the crafted tables of tests/scan_craft.py: one test per kernel shape
(packed x log_g 0 / 2 / 3 x occupancy bitmap; slot formats 5, 6, 7, 8 through kr_scan_pipe_kernel_t and, under KR_SCAN_PIPE=0, through
kr_scan_kernel_t<SLOT = true>; format 9 through kr_scan_filt_kernel_t) and geometry (one library, two libraries: the SL instantiations).
Each asserts the shape that the index and the stream report, then requires the table hits, hdist_filt, onmers and histograms to equal
the plain reference and the oracle EXACTLY, with the hit tap (TAP instantiations) and without it (the instantiations production runs).
tests/test_scan_craft_cpu.py checks, without a GPU, that the designs sit on their boundaries for every one of these layouts."""
import numpy as np
import pytest

import scan_craft
from conftest import assert_rows_close, rows_of_oracle

pytestmark = pytest.mark.gpu

# kernel shape: (id, slot format, log_g, occupancy bitmap, KR_SCAN_PIPE)
SHAPES = ([(f"packed_g{g}_bm{b}", 0, g, b, 1) for g in (0, 2, 3) for b in (0, 1)]
          + [(f"fmt{f}_pipe", f, 0, 0, 1) for f in (5, 6, 7, 8)] + [(f"fmt{f}_nopipe", f, 0, 0, 0) for f in (5, 6, 7, 8)] + [("fmt9", 9, 0, 0, 1)])
BY_ID = {s[0]: s for s in SHAPES}
FAMILIES = ("packed_g2_bm0", "fmt6_pipe", "fmt6_nopipe", "fmt9")


@pytest.fixture(scope="module")
def tables(capi, po, tmp_path_factory):
    """the crafted tables of (slot format, log_g, geometry), written once: Craft, host index, oracle index, and the references by th"""
    made = {}

    def get(fmt, log_g, geo):
        key = (fmt, log_g, geo)
        if key not in made:
            cr = scan_craft.designs(capi.scan_layout(fmt, log_g), geo)
            path = cr.write(str(tmp_path_factory.mktemp(f"scan_{fmt}_{log_g}_{geo}") / "ix"))
            made[key] = dict(cr=cr, hx=capi.HostIndex(path), ox=po.Index(path), ref={}, oracle={})
        return made[key]

    return get


def upload(capi, t, monkeypatch, shape):
    name, fmt, log_g, occ, pipe = shape
    monkeypatch.setenv("KR_SLOT_LOG2W", str(fmt))
    monkeypatch.setenv("KR_LOG_G", str(log_g))
    monkeypatch.setenv("KR_OCC_BITMAP", str(occ))
    monkeypatch.setenv("KR_SCAN_PIPE", str(pipe))
    dx = t["hx"].upload(0)
    assert dx.slot_format == fmt and (fmt != 0 or (dx.log_g, dx.occ_bitmap) == (log_g, bool(occ)))
    return dx


def stream(capi, dx, shape, th, nreads, nbases):
    name, fmt, log_g, occ, pipe = shape
    st = dx.stream(params=capi.default_params(hdist_th=th), max_reads=nreads, max_bases=nbases + 64, max_records=nreads * 64)
    info = st.scan_info()
    assert info["pipe"] == (fmt in (5, 6, 7, 8) and pipe == 1) and info["filt"] == (fmt == 9 and th <= capi.scan_layout(9)["filt_max_th"]), (name, info)
    return st


def reference_of(t, reads, th):
    out = []
    for r in reads:
        if (r.name, th) not in t["ref"]:
            t["ref"][(r.name, th)] = scan_craft.reference(t["cr"], [r.seq], th)[0]
        out.append(t["ref"][(r.name, th)])
    return out


def run_exact(capi, po, t, dx, shape, reads, th=scan_craft.TH):
    """the batch with the taps: hits, readtaps, onmers and histograms exact; then without: the same rows, close to the oracle's"""
    bases, offs = t["cr"].batch(reads)
    counts = reference_of(t, reads, th)
    ref = t["ox"].dist(bases, offs, None, po.params(collect=7, hdist_th=th))
    st = stream(capi, dx, shape, th, len(reads), len(bases))
    st.submit(bases, offs, capi.KR_TAP_HITS | capi.KR_TAP_ACCS)
    res = st.collect()
    h = st.hits()
    got = sorted(zip(h["read"].tolist(), h["strand"].tolist(), h["kpos"].tolist(), h["lib"].tolist(), h["cmer_index"].tolist(), h["hd"].tolist(), h["se"].tolist()))
    want = sorted((i,) + x for i, c in enumerate(counts) for x in c["hits"])
    if got != want:
        lost, extra = sorted(set(want) - set(got)), sorted(set(got) - set(want))
        names = sorted({reads[x[0]].name for x in lost + extra})
        raise AssertionError(f"{shape[0]}: table hits differ from the reference in reads {names[:12]}: {len(lost)} lost {lost[:4]}, {len(extra)} extra {extra[:4]}, "
                             f"{len(got) - len(set(got))} doubled")
    assert st.readtaps(len(reads)).tolist() == [c["hdist_filt"] for c in counts]
    assert res.read_onmers.tolist() == [c["onmers"] for c in counts]
    acc = ref["accs"][ref["accs"]["passed"] == 1]
    assert sorted(zip(res.rec_read.tolist(), res.rec_key.tolist(), [tuple(x) for x in res.rec_hist.tolist()])) == \
        sorted(zip(acc["read"].tolist(), ((acc["se"] << 1) | acc["strand"]).tolist(), [tuple(x[:th + 1]) for x in acc["hist"].tolist()]))
    rows = res.rows()
    assert_rows_close(rows, rows_of_oracle(ref))
    demand = st.scan_info()["item_slots"]
    assert demand >= sum(c["items"] for c in counts) or shape[1] == 9  # (filter slots: the items are candidates)
    st.close()
    st = stream(capi, dx, shape, th, len(reads), len(bases))
    st.submit(bases, offs)
    res2 = st.collect()
    assert res2.rows() == rows
    assert res2.read_onmers.tolist() == [c["onmers"] for c in counts]
    st.close()
    return counts, demand


@pytest.mark.parametrize("geo", ["one", "two"])
@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_every_design_through_every_shape(capi, po, tables, monkeypatch, shape, geo):
    """th = 4, every designed read of the layout in one batch"""
    t = tables(shape[1], shape[2], geo)
    dx = upload(capi, t, monkeypatch, shape)
    counts, _ = run_exact(capi, po, t, dx, shape, t["cr"].reads)
    assert sum(len(c["hits"]) for c in counts) > 1000
    dx.close()


@pytest.mark.parametrize("geo", ["one", "two"])
@pytest.mark.parametrize("th", ["none", "most"])
@pytest.mark.parametrize("name", ["fmt6_pipe", "fmt9", "packed_g2_bm0"])
def test_other_thresholds(capi, po, tables, monkeypatch, name, th, geo):
    """th = 0 (only the query's own code is a hit) and th = 16 (every entry of a probed bucket is one: the item list's chunks, the
    stage and the hit windows fill up); format 9 at the largest threshold its candidates carry"""
    shape = BY_ID[name]
    th = 0 if th == "none" else (capi.scan_layout(9)["filt_max_th"] if shape[1] == 9 else 16)
    t = tables(shape[1], shape[2], geo)
    dx = upload(capi, t, monkeypatch, shape)
    counts, _ = run_exact(capi, po, t, dx, shape, t["cr"].reads, th=th)
    if th == 16:
        lay = capi.scan_layout(shape[1], shape[2])
        assert max(c["items"] for c in counts) > lay["item_chunk"] + lay["item_stage"]
    dx.close()


@pytest.mark.parametrize("name", FAMILIES + ("fmt7_pipe", "packed_g0_bm1"))
def test_odd_probe_counts(capi, po, tables, monkeypatch, name):
    """half of the residues served: groups of 0, 1, PPS - 1, PPS, PPS + 1 listed probes on slotted tables"""
    shape = BY_ID[name]
    t = tables(shape[1], shape[2], "half")
    dx = upload(capi, t, monkeypatch, shape)
    run_exact(capi, po, t, dx, shape, t["cr"].reads)
    dx.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_batch_sizes(capi, po, tables, monkeypatch, name):
    """batches of 1 .. 1,025 reads (the designs repeated): the read cursors' ranges and the per-visit stores of the reads' results"""
    shape = BY_ID[name]
    t = tables(shape[1], shape[2], "two")
    dx = upload(capi, t, monkeypatch, shape)
    designs = t["cr"].reads
    chunk = capi.scan_layout(shape[1], shape[2])["read_chunk"]
    for n in (1, chunk - 1, chunk, chunk + 1, 1023, 1024, 1025):
        run_exact(capi, po, t, dx, shape, [designs[(7 * i + n) % len(designs)] for i in range(n)])
    dx.close()


@pytest.mark.parametrize("name", FAMILIES)
def test_item_list_out_of_room(capi, po, tables, monkeypatch, name):
    """a stream whose scan is told that the item list holds at most half of what the batch asks for: KR_ERR_CAPACITY ("hit list overflow")
    from wait, collect and collect_device, never a read whose item range lies outside what was written; the next batch on the same
    stream, of reads without a hit, is exact"""
    shape = BY_ID[name]
    t = tables(shape[1], shape[2], "one")
    dx = upload(capi, t, monkeypatch, shape)
    reads = t["cr"].reads
    counts, demand = run_exact(capi, po, t, dx, shape, reads)
    lay = capi.scan_layout(shape[1], shape[2])
    assert demand > lay["item_chunk"]
    monkeypatch.setenv("KR_DEBUG_ITEM_CAP", str(demand // 2))
    bases, offs = t["cr"].batch(reads)
    st = stream(capi, dx, shape, scan_craft.TH, len(reads), len(bases))
    monkeypatch.delenv("KR_DEBUG_ITEM_CAP")
    assert st.scan_info()["item_cap"] == demand // 2
    st.submit(bases, offs, capi.KR_TAP_ACCS)
    for call in (st.wait, st.collect, st.collect_device):
        with pytest.raises(capi.KrError) as e:
            call()
        assert e.value.code == capi.KR_ERR_CAPACITY and "hit list overflow" in str(e.value)
    assert st.scan_info()["item_slots"] > demand // 2
    quiet, rng = [], np.random.default_rng(5)  # reads that probe empty rows only
    while len(quiet) < 8:
        r = scan_craft.Read(f"quiet_{len(quiet)}", "".join("ACGT"[i] for i in rng.integers(0, 4, scan_craft.K + 40)), "")
        if not scan_craft.reference(t["cr"], [r.seq])[0]["probed"]:
            quiet.append(r)
    bases, offs = t["cr"].batch(quiet)
    st.submit(bases, offs, capi.KR_TAP_ACCS)
    res = st.collect()
    assert res.nrecs == 0 and res.read_onmers.tolist() == [c["onmers"] for c in reference_of(t, quiet, scan_craft.TH)]
    assert (st.readtaps(len(quiet)) == 0xFFFFFFFF).all() and st.scan_info()["item_slots"] == 0
    st.close()
    dx.close()
