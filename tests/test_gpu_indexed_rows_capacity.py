"""KR_ROWS_INDEXED at the ends of its list (include/krepp_amd.h; docs/design/05): a row's DIST is dist_list[rec_dix[i]], the list holds
`dist_cap` entries (the lane's record slots: it aliases rec_v) while list positions are handed out up to `rep_cap`, which is 4 M more.
At test size neither end can be reached -- every capacity has a floor far above a small batch --, so KR_DEBUG_LIST_CAPS="dist,rep"
lowers what the kernels are told the list holds:

* positions beyond dist_cap: the batch is run again without the hint and comes back with rec_d, never with a rec_dix >= ndist;
* positions beyond rep_cap: kErrRecCap from the de-duplication stage (both kernels, and the call site of records that are their
  own problem), KR_ERR_CAPACITY for plain and indexed batches alike, and nothing of the failed batch survives in the stream;
* the device view of an honoured batch has its DIST column (rec_dix per record slot, dist_list, ndist);
* a batch without rows has ndist == 0;
* thresholds other than 4, KR_DD_DIRECT=0 and batches of 1 / 63 / 64 / 65 reads (wave and chunk edges of take_positions).

The reference is always the rows of a plain KR_ROWS_ONLY batch of the same reads (pinned to the oracle in tests/test_gpu_parity.py),
compared as sorted (read, key, bits of DIST): no tolerance anywhere.  One lane; every stream's buffers are poisoned (KR_DEBUG_POISON)."""
import ctypes as C

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FLOOR = 256  # kListCapFloor (kr_host_stream.inc): the knob lowers no capacity below it


@pytest.fixture(scope="module")
def toy(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    yield hx, dx
    dx.close()
    hx.close()


@pytest.fixture(scope="module")
def reads(toy_genomes, synth):
    return synth.sample_reads(toy_genomes, 5003, seed=21)  # (the inputs of test_indexed_rows_are_the_rows)


@pytest.fixture(autouse=True)
def one_lane_poisoned(monkeypatch):
    monkeypatch.setenv("KR_LANES", "1")
    monkeypatch.setenv("KR_DEBUG_POISON", "all")
    monkeypatch.delenv("KR_DEBUG_LIST_CAPS", raising=False)
    monkeypatch.delenv("KR_DD_DIRECT", raising=False)


def rows(r):
    return sorted(zip(r.rec_read.tolist(), r.rec_key.tolist(), r.rec_d.view(np.uint64).tolist()))


def new_stream(capi, dx, bases, offs, th=4):
    return dx.stream(params=capi.default_params(hdist_th=th), max_reads=len(offs) - 1, max_bases=max(1, len(bases)))


_plain = {}


def plain(capi, toy, bases, offs, names, th=4, tag="all"):
    """The reference, once per (threshold, batch): rows, text and bytes copied back of a plain rows-only batch on a stream of its own."""
    if (th, tag) not in _plain:
        hx, dx = toy
        st = new_stream(capi, dx, bases, offs, th)
        st.submit(bases, offs, capi.KR_ROWS_ONLY)
        r = st.collect()
        assert r.rec_dix is None and r.nrows == len(r.rec_key)
        _plain[(th, tag)] = dict(rows=rows(r), na=r.read_na.tolist(), nrows=r.nrows, cnt=r.read_cnt.copy(), text=st.format_dist(hx, names), d2h=st.last_d2h_bytes())
        st.close()
    return _plain[(th, tag)]


def test_list_overflow_is_rerun_with_rec_d(capi, toy, reads, monkeypatch):
    """List positions beyond dist_list: rerun without the hint -- rec_d, the plain batch's rows, text and 12-byte rows.
    Before the rerun existed: ndist = min(extent, dist_cap) with rows pointing past it -- IndexError in capi.Result, a read past the
    list in kr_format_dist."""
    hx, dx = toy
    bases, offs, names = reads
    n = len(offs) - 1
    ref = plain(capi, toy, bases, offs, names)
    IX = capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED
    st = new_stream(capi, dx, bases, offs)
    st.submit(bases, offs, IX)
    ix = st.collect()
    assert ix.rec_dix is not None and rows(ix) == ref["rows"]
    U = len(np.unique(ix.rec_dix))  # distinct problems the rows refer to: timing-independent, and a lower bound of every extent
    e0, f0 = st.indexed_list()
    assert f0 == 0 and e0 >= U
    dist = U // 2
    assert dist > FLOOR
    monkeypatch.setenv("KR_DEBUG_LIST_CAPS", f"{dist},")
    for k in range(2):
        st.submit(bases, offs, IX)
        r = st.collect()
        e, f = st.indexed_list()
        print(f"U {U} dist_cap {dist} extent {e} fallbacks {f}")
        assert e >= U > dist and f == f0 + k + 1
        assert r.rec_dix is None and not st._rv.rec_dix and st._rv.rec_d
        assert rows(r) == ref["rows"] and r.read_na.tolist() == ref["na"]
        assert st.format_dist(hx, names) == ref["text"]
        assert st.last_d2h_bytes() == ref["d2h"] == 9 * n + 12 * ref["nrows"]
    st.close()


def test_boundary_decided_by_the_run_itself(capi, toy, reads, monkeypatch):
    """dist_cap = an extent this batch has had: which lane wins a CAS moves the extent from run to run, so each run says itself
    (kr_debug_indexed_list) on which side it fell -- rerun exactly when extent > dist_cap, the reference's rows either way."""
    hx, dx = toy
    bases, offs, names = reads
    ref = plain(capi, toy, bases, offs, names)
    IX = capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED
    st = new_stream(capi, dx, bases, offs)
    st.submit(bases, offs, IX)
    st.collect()
    E, f = st.indexed_list()
    assert f == 0 and E > FLOOR
    monkeypatch.setenv("KR_DEBUG_LIST_CAPS", f"{E},")
    for _ in range(3):
        st.submit(bases, offs, IX)
        r = st.collect()
        e, f1 = st.indexed_list()
        print(f"dist_cap {E} extent {e} fallbacks {f} -> {f1}")
        assert f1 - f in (0, 1) and (f1 - f == 1) == (e > E)
        assert rows(r) == ref["rows"] and st.format_dist(hx, names) == ref["text"]
        if f1 == f:
            assert r.rec_dix is not None and int(r.rec_dix.max()) < len(r.dist_list) == st._rv.ndist == min(e, E)
        else:
            assert r.rec_dix is None
        f = f1
    monkeypatch.delenv("KR_DEBUG_LIST_CAPS")
    st.submit(bases, offs, IX)
    r = st.collect()
    e, f1 = st.indexed_list()
    assert f1 == f and r.rec_dix is not None and len(r.dist_list) == st._rv.ndist == e and int(r.rec_dix.max()) < e
    assert rows(r) == ref["rows"]
    st.close()


@pytest.mark.parametrize("cfg", ["default", "no_direct_part", "th3_every_record_its_own_problem"])
def test_positions_run_out_in_the_dedup_stage(capi, toy, reads, monkeypatch, cfg):
    """rep_cap below the positions in use: kErrRecCap from take_positions (kr_dedup_kernel: table winners; records that are their own
    problem -- all of them with hdist_th = 3) or from kr_dedup_direct_kernel, whichever comes first.  KR_ERR_CAPACITY from collect,
    wait and collect_device, for a plain and an indexed batch; the stream then returns the reference's rows."""
    hx, dx = toy
    bases, offs, names = reads
    th = 3 if cfg.startswith("th3") else 4
    ref = plain(capi, toy, bases, offs, names, th)
    IX = capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED
    if cfg == "no_direct_part":
        monkeypatch.setenv("KR_DD_DIRECT", "0")  # (read when the stream is made)
    st = new_stream(capi, dx, bases, offs, th)
    st.submit(bases, offs, IX)
    ix = st.collect()
    assert ix.rec_dix is not None and rows(ix) == ref["rows"]
    U = len(np.unique(ix.rec_dix))
    rep = U // 2
    assert rep > FLOOR
    for flags in (capi.KR_ROWS_ONLY, IX):
        monkeypatch.setenv("KR_DEBUG_LIST_CAPS", f",{rep}")
        st.submit(bases, offs, flags)
        for call in (st.collect, st.wait, st.collect_device):
            with pytest.raises(capi.KrError) as e:
                call()
            assert e.value.code == capi.KR_ERR_CAPACITY, (cfg, flags, call)
        monkeypatch.delenv("KR_DEBUG_LIST_CAPS")
        st.submit(bases, offs, flags)
        r = st.collect()
        assert (r.rec_dix is not None) == (flags == IX)
        assert rows(r) == ref["rows"] and r.read_na.tolist() == ref["na"] and st.format_dist(hx, names) == ref["text"], (cfg, flags)
    assert st.indexed_list()[1] == 0
    st.close()


def test_device_view_has_the_dist_column(capi, toy, reads):
    """kr_batch_collect_device of an honoured indexed batch: rec_d NULL (the rows lie there), rec_dix per record slot, dist_list and
    ndist on the device.  Before: rec_d, rec_dix and dist_list all NULL -- a view without DIST."""
    import torch
    hx, dx = toy
    bases, offs, names = reads
    ref = plain(capi, toy, bases, offs, names)
    st = new_stream(capi, dx, bases, offs)
    st.submit(bases, offs, capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED)
    rv = st.collect_device()
    assert not rv.rec_d and rv.rec_dix and rv.dist_list and rv.ndist > 0

    class DevPtr:
        def __init__(self, ptr, nbytes):
            self.__cuda_array_interface__ = {"shape": (int(nbytes),), "typestr": "|u1", "data": (int(ptr), False), "version": 2}

    def dev(ptr, n, dt):
        a = torch.as_tensor(DevPtr(C.cast(ptr, C.c_void_p).value, n * np.dtype(dt).itemsize), device="cuda:0").cpu().numpy()
        return a.view(dt)

    n = rv.nreads
    off, cnt = dev(rv.read_off, n, np.uint32), dev(rv.read_cnt, n, np.uint32)
    key, sel, dix = dev(rv.rec_key, rv.nrecs, np.uint32), dev(rv.rec_sel, rv.nrecs, np.uint8), dev(rv.rec_dix, rv.nrecs, np.uint32)
    dl = dev(rv.dist_list, rv.ndist, np.float64).view(np.uint64)
    at = [(r, i) for r in range(n) for i in range(int(off[r]), int(off[r]) + int(cnt[r])) if sel[i]]
    assert len(at) == ref["nrows"] and all(int(dix[i]) < rv.ndist for _, i in at)
    assert sorted((r, int(key[i]), int(dl[dix[i]])) for r, i in at) == ref["rows"]
    assert st.indexed_list() == (rv.ndist, 0)
    # ... and the host view of the same batch
    r = st.collect()
    assert r.rec_dix is not None and rows(r) == ref["rows"]
    # a plain batch on the same stream afterwards
    st.submit(bases, offs, capi.KR_ROWS_ONLY)
    rv = st.collect_device()
    assert rv.rec_d and not rv.rec_dix and not rv.dist_list and rv.ndist == 0
    st.close()


def test_a_batch_without_rows_has_an_empty_list(capi, toy, reads):
    """300 reads without a valid k-mer: no record, no row, `NA` for every read.  As a stream's first indexed batch and after one
    with rows: ndist == 0 (it kept the earlier batch's count), rec_dix non-NULL (the hint was honoured), the plain batch's text."""
    hx, dx = toy
    bases, offs, names = reads
    ref = plain(capi, toy, bases, offs, names)
    m = 300
    seq = np.frombuffer((b"ACGTTGCAAGGCTTAACCGN" * 8)[:150], np.uint8)  # an N in every window of 21
    nb, no, nn = np.tile(seq, m), (np.arange(m + 1) * 150).astype(np.uint64), [f"none{i}" for i in range(m)]
    want = plain(capi, toy, nb, no, nn, tag="none")
    assert want["nrows"] == 0 and want["na"] == [1] * m and want["text"] == "".join(f"{x}\tNA\tNaN\n" for x in nn)
    IX = capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED
    st = new_stream(capi, dx, bases, offs)
    for after_rows in (False, True):
        st.submit(nb, no, IX)
        r = st.collect()
        assert st._rv.rec_dix and not st._rv.rec_d and st._rv.ndist == 0, after_rows
        assert r.nrows == 0 and len(r.rec_key) == 0 and r.read_na.tolist() == [1] * m
        assert st.format_dist(hx, nn) == want["text"]
        if not after_rows:
            st.submit(bases, offs, IX)
            r = st.collect()
            assert st._rv.ndist > 0 and rows(r) == ref["rows"]
    st.close()


@pytest.mark.parametrize("cfg", ["th2", "th6", "no_direct_part", "small_batches"])
def test_paths_the_indexed_form_had_not_met(capi, toy, reads, monkeypatch, cfg):
    """Indexed rows == plain rows where every record is its own problem (thresholds other than 4: no packed word, the second
    take_positions call site), without the direct part, and for batches of 1, 63, 64 and 65 reads."""
    hx, dx = toy
    bases, offs, names = reads
    IX = capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED
    th = {"th2": 2, "th6": 6}.get(cfg, 4)
    if cfg == "no_direct_part":
        monkeypatch.setenv("KR_DD_DIRECT", "0")
    st = new_stream(capi, dx, bases, offs, th)
    if cfg != "small_batches":
        ref = plain(capi, toy, bases, offs, names, th)
        assert ref["nrows"] > 0
        st.submit(bases, offs, IX)
        r = st.collect()
        assert r.rec_dix is not None and int(r.rec_dix.max()) < len(r.dist_list) == st._rv.ndist
        assert rows(r) == ref["rows"] and r.read_na.tolist() == ref["na"] and st.format_dist(hx, names) == ref["text"]
    else:
        r0 = int(np.nonzero(plain(capi, toy, bases, offs, names)["cnt"])[0][0])  # (so that the batch of one read has a row)
        for m in (1, 63, 64, 65):
            b, o, nm = bases[int(offs[r0]):int(offs[r0 + m])], offs[r0:r0 + m + 1] - offs[r0], names[r0:r0 + m]
            ref = plain(capi, toy, b, o, nm, tag=m)
            assert ref["nrows"] > 0
            st.submit(b, o, IX)
            r = st.collect()
            assert r.rec_dix is not None and int(r.rec_dix.max()) < len(r.dist_list) == st._rv.ndist, m
            assert rows(r) == ref["rows"] and r.read_na.tolist() == ref["na"] and st.format_dist(hx, nm) == ref["text"], m
    assert st.indexed_list()[1] == 0
    st.close()
