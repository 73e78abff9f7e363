"""Every buffer that grows with the batches (kr_buf.h: the stream's host record arrays, its text buffer, the tiles, the place
workspace, the index's likelihood workspace) through "first allocation, growth, reuse without growth": one stream per consumer is
given 64 reads, then 2,000, then the first 64 again, and every batch's result must equal, bit for bit, what a fresh stream gives
for that batch alone.  2,000 exceeds every first-allocation floor that depends on the read count (n + n / 4); the fixed floors
(2^20 candidate slots, 65,536 records) are not crossed here -- tests/test_gpu_place_capacity.py's capped runs grow above those.
Allocation failure is not provoked on the device: tests/buf_check.cpp covers that path on the CPU."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = (64, 2000, 64)


@pytest.fixture(scope="module")
def toy(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    return hx, hx.upload(0)


@pytest.fixture(scope="module")
def batches(synth, toy_genomes):
    small = synth.sample_reads(toy_genomes, SIZES[0], seed=41)
    return [small, synth.sample_reads(toy_genomes, SIZES[1], seed=42), small]


def bits(a):
    return None if a is None else np.ascontiguousarray(a).view(np.uint64).tolist()


def records(res, rows_only=False):
    """Every record of a collected batch with everything the host arrays hold of it, in a canonical order (record slots are handed
    out to waves as they come: their order in the arrays is not part of the result).  A rows-only batch copies no k-mer counts back."""
    cols = [res.rec_read.tolist(), res.rec_key.tolist(), res.rec_sel.tolist(), bits(res.rec_d)]
    cols += [c for c in (bits(res.rec_v), bits(res.rec_chisq), [tuple(h) for h in res.rec_hist.tolist()] if res.rec_hist is not None else None) if c is not None]
    per_read = (res.nreads, res.nrows, res.read_cnt.tolist(), None if rows_only else res.read_onmers.tolist(), res.read_na.tolist())
    return per_read, sorted(zip(*cols))


def new_stream(capi, dx, batches):
    return dx.stream(max_reads=4096, max_bases=max(len(b[0]) for b in batches) + 64)


def through_one_stream_and_fresh_ones(capi, dx, batches, run):
    """run(stream, batch) -> result; the three batches on one stream against each on a stream of its own"""
    st = new_stream(capi, dx, batches)
    for i, b in enumerate(batches):
        got = run(st, b)
        fresh = new_stream(capi, dx, batches)
        want = run(fresh, b)
        fresh.close()
        assert got == want, f"batch {i} ({len(b[2])} reads) on a stream that had other batches before differs from a fresh stream's"
    st.close()


def test_collect_full_records(capi, toy, batches):
    def run(st, b):
        st.submit(b[0], b[1], capi.KR_TAP_ACCS)  # (every host array: key, sel, d, v, chisq and the histogram planes)
        return records(st.collect())

    through_one_stream_and_fresh_ones(capi, toy[1], batches, run)


def test_rows_only_indexed(capi, toy, batches):
    def run(st, b):
        st.submit(b[0], b[1], capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED)
        res = st.collect()
        assert res.rec_dix is not None  # (the 8-byte rows and the list of distinct DIST values did come back)
        assert len(res.rec_dix) == 0 or int(res.rec_dix.max()) < len(res.dist_list)
        # the list as the rows name it: its positions are handed out to waves in chunks as they come, so where a value lies in it,
        # and what the unused positions between the chunks hold, is not part of the result (records() has every row's value)
        return records(res, rows_only=True), sorted(set(bits(res.dist_list[res.rec_dix])))

    through_one_stream_and_fresh_ones(capi, toy[1], batches, run)


def test_device_text(capi, toy, batches):
    hx, dx = toy

    def run(st, b):
        if not getattr(st, "_text_on", False):
            st.text_enable(hx, 1 << 22, 1 << 20)
        st.submit_text(b[0], b[1], b[2])
        return st.collect_text()

    through_one_stream_and_fresh_ones(capi, dx, batches, run)


def test_tiled_batch_then_untiled(capi, toy, toy_genomes, batches):
    """The middle batch holds one sequence long enough to be tiled (more than 1,024 k-mer positions); the batch behind it is not."""
    g = next(iter(toy_genomes.values()))
    b, o, n = batches[1]
    long_b = np.concatenate([b, g[1000:4000]])
    long_o = np.concatenate([o, np.array([len(b) + 3000], np.uint64)])
    tiled = [batches[0], (long_b, long_o, n + ["contig"]), batches[2]]

    def run(st, bt):
        st.submit(bt[0], bt[1], capi.KR_TAP_ACCS)
        return records(st.collect())

    through_one_stream_and_fresh_ones(capi, toy[1], tiled, run)


@pytest.mark.parametrize("want_placements", [False, True], ids=["device-text", "kept-candidates-to-the-host"])
def test_place_on_the_device(capi, toy, batches, want_placements):
    """want_placements=False: the rows are formatted on the device (tree, reads, candidate, kept, sorted, ids and text workspaces);
    True: the kept candidates come back to the host (their page-locked arrays)."""
    hx = toy[0]
    mb = max(len(b[0]) for b in batches) + 64

    def run(pl, b):
        before, tbefore = capi.place_counters(), capi.place_text_counters()
        text, p = pl.place(b[0], b[1], b[2], want_placements=want_placements)
        assert capi.place_counters()[0] == before[0] + 1, "the batch did not go through the device back end"
        if not want_placements:
            assert capi.place_text_counters()[0] > tbefore[0], "the rows were not written on the device"
        return text, p.tobytes()

    pl = capi.Placer(hx, None, 0, tabular=True, max_reads=4096, max_bases=mb)
    for i, b in enumerate(batches):
        got = run(pl, b)
        fresh = capi.Placer(hx, None, 0, tabular=True, max_reads=4096, max_bases=mb)
        want = run(fresh, b)
        fresh.close()
        assert got == want, f"batch {i} ({len(b[2])} reads) differs from a fresh placer's"
    pl.close()


def test_llh_batch_workspace(capi, toy):
    """kr_llh_batch with n = 100, 10,000, 100 on one index against the same three calls, each on an index uploaded afresh"""
    lib = capi.load()
    th = 4
    rng = np.random.default_rng(11)

    def call(dx, n, seed):
        r = np.random.default_rng(seed)
        hist = np.floor(r.random((n, th + 1)) * 20)
        uc = np.floor(r.random(n) * 100)
        rho = r.uniform(0.05, 1.0, n)
        d, v = np.zeros(n), np.zeros(n)
        capi.check(lib.kr_llh_batch(dx.h, th, 0, n, hist.ctypes.data, uc.ctypes.data, rho.ctypes.data, None, d.ctypes.data, v.ctypes.data))
        return bits(d), bits(v)

    seeds = [int(s) for s in rng.integers(0, 1 << 30, 3)]
    sizes = (100, 10000, 100)
    got = [call(toy[1], n, s) for n, s in zip(sizes, seeds)]
    want = []
    for n, s in zip(sizes, seeds):
        fresh = toy[0].upload(0)
        want.append(call(fresh, n, s))
        fresh.close()
    assert got == want
