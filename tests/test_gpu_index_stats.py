"""kr_index_stats_device against kr_index_stats_cpu and the numpy restatement (tests/inspect_ref.py), with KR_STATS_KEEP_COUNTS: the
count kernel's routes and seams, the value histograms' sort passes, bad colour ids, the memory fallback.  kr_debug_index_stats
proves which route an input took; the LDS cap and the run length are read from it, not written down here."""
import numpy as np
import pytest

import inspect_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def dbg0(capi):
    d = capi.index_stats_debug()
    assert d["cap"] >= 2 and d["run"] >= 64
    return d


def random_pse(rng, ns):
    pse = rng.integers(0, ns, size=(ns, 2), dtype=np.uint32)
    pse[:2] = 0
    return pse


def both(capi, se, pse, device_view=False, **env):
    """device (host view, or the arrays uploaded with torch first) == cpu == restatement; returns (stats, debug counters)"""
    se = np.asarray(se, np.uint32)
    pse = np.asarray(pse, np.uint32).reshape(-1, 2)
    want = ref.stats_ref(se, pse, len(pse))
    view, keep = ref.craft_view(capi, [dict(se=se, pse=pse)])
    cpu = capi.index_stats(view, keep_counts=True)[0]
    ref.assert_stats_equal(cpu, want)
    if device_view:
        import torch

        cmer = keep[1] if len(se) else np.zeros((1, 2), np.uint32)
        t_cmer = torch.from_numpy(cmer.view(np.int32)).cuda()
        t_pse = torch.from_numpy(np.ascontiguousarray(pse).view(np.int32)).cuda()
        torch.cuda.synchronize()
        dview, dkeep = ref.craft_view(capi, [dict(ptrs=(t_cmer.data_ptr(), t_pse.data_ptr(), len(se), len(pse)))])
        got = capi.index_stats(dview, device=0, keep_counts=True, view_flags=capi.KR_VIEW_DEVICE)[0]
    else:
        got = capi.index_stats(view, device=0, keep_counts=True)[0]
    ref.assert_stats_equal(got, want)
    return got, capi.index_stats_debug()


def test_entry_counts(capi, dbg0):
    rng = np.random.default_rng(1)
    ns = 300
    pse = random_pse(rng, ns)
    run = dbg0["run"]
    for n in (0, 1, 63, 64, 65, run - 1, run, run + 1):
        se = rng.integers(0, ns, size=n, dtype=np.uint32)
        got, d = both(capi, se, pse)
        assert d["path"] == 1 and d["lds"] + d["global"] == n and d["chunks"] == (1 if n else 0), (n, d)


@pytest.mark.parametrize("device_view", [False, True])
@pytest.mark.parametrize("n,chunk", [(200, 70), (200, 67), (135, 67)])
def test_three_chunks(capi, dbg0, monkeypatch, device_view, n, chunk):
    """seams inside a wave's 64 entries (70), on an odd entry, where a chunk read in place no longer starts on 16 bytes (67), and
    in front of the last entry (2 * 67 + 1)"""
    rng = np.random.default_rng(2)
    ns = dbg0["cap"] + 50
    monkeypatch.setenv("KR_STATS_CHUNK_KMERS", str(chunk))
    se = rng.integers(0, ns, size=n, dtype=np.uint32)
    se[[0, chunk - 1, chunk, 2 * chunk - 1, 2 * chunk, n - 1]] = [1, 2, 3, dbg0["cap"], dbg0["cap"] + 1, 5]
    got, d = both(capi, se, random_pse(rng, ns), device_view=device_view)
    assert d["path"] == 1 and d["chunks"] == 3 and d["lds"] + d["global"] == n


def test_every_kmer_below_the_cap_is_served_from_lds(capi, dbg0):
    n = 3 * dbg0["run"] + 17
    got, d = both(capi, np.full(n, 7, np.uint32), np.zeros((20, 2), np.uint32))
    assert d["lds"] == n and d["global"] == 0
    assert got["se_count"][7] == n


def test_distinct_colours_above_the_cap_go_global(capi, dbg0):
    cap, n = dbg0["cap"], 5000
    ns = cap + n
    rng = np.random.default_rng(3)
    got, d = both(capi, cap + rng.permutation(n).astype(np.uint32), random_pse(rng, ns))
    assert d["lds"] == 0 and d["global"] == n


def test_colours_around_the_cap(capi, dbg0):
    cap = dbg0["cap"]
    se = np.array([cap - 1] * 5 + [cap] * 7 + [cap + 1] * 11 + [cap - 1, cap, cap + 1], np.uint32)
    got, d = both(capi, se, np.zeros((cap + 2, 2), np.uint32))
    assert (d["lds"], d["global"]) == (6, 20)
    assert [int(got["se_count"][c]) for c in (cap - 1, cap, cap + 1)] == [6, 8, 12]


def test_lds_route_switched_off(capi, dbg0, monkeypatch):
    monkeypatch.setenv("KR_STATS_LDS_CAP", "0")
    got, d = both(capi, np.full(1000, 7, np.uint32), np.zeros((20, 2), np.uint32))
    assert d["cap"] == 0 and d["lds"] == 0 and d["global"] == 1000


def test_zipf_mix_twice(capi, dbg0):
    rng = np.random.default_rng(4)
    ns, n = 50_000, 200_000
    se = np.minimum(rng.zipf(1.3, size=n), ns - 1).astype(np.uint32)
    pse = random_pse(rng, ns)
    a, da = both(capi, se, pse)
    b, db = both(capi, se, pse)
    for k in ("se_count", "se_outdeg", "mer_value", "mer_freq", "deg_value", "deg_freq"):
        np.testing.assert_array_equal(a[k], b[k])
    assert (da["lds"], da["global"]) == (db["lds"], db["global"]) and da["lds"] > 0 and da["global"] > 0


def test_device_view_equals_host_view(capi, dbg0):
    rng = np.random.default_rng(5)
    ns, n = dbg0["cap"] + 1000, 3 * dbg0["run"] + 5
    se = rng.integers(0, ns, size=n, dtype=np.uint32)
    pse = random_pse(rng, ns)
    a, da = both(capi, se, pse)
    b, db = both(capi, se, pse, device_view=True)
    for k in ("se_count", "se_outdeg", "mer_value", "mer_freq", "deg_value", "deg_freq"):
        np.testing.assert_array_equal(a[k], b[k])
    assert da["path"] == db["path"] == 1 and (da["lds"], da["global"]) == (db["lds"], db["global"])


def test_histogram_of_equal_counts_is_one_row(capi):
    ns = 2500  # more than one tile of the sort
    se = np.repeat(np.arange(ns, dtype=np.uint32), 3)
    pse = np.zeros((ns, 2), np.uint32)
    pse[1:, 0] = np.arange(1, ns)  # every colour 1 .. names itself once, and colour 0 once
    got, d = both(capi, se, pse)
    assert got["mer_value"].tolist() == [3] and got["mer_freq"].tolist() == [ns - 1]
    assert got["deg_value"].tolist() == [1] and got["deg_freq"].tolist() == [ns - 1]
    assert d["passes_mer"] == 1 and d["passes_deg"] == 1


def test_histogram_of_distinct_counts(capi):
    ns = 200
    se = np.repeat(np.arange(ns, dtype=np.uint32), np.arange(ns))  # colour c carries c k-mers: no value 0 among 1 ..
    got, d = both(capi, se, np.zeros((ns, 2), np.uint32))
    assert got["mer_value"].tolist() == list(range(1, ns)) and (got["mer_freq"] == 1).all()
    assert got["deg_value"].tolist() == [0] and d["passes_mer"] == 1 and d["passes_deg"] == 0  # (no digit can differ: no pass)


@pytest.mark.parametrize("big,passes", [(255, 1), (256, 2), (65535, 2), (70000, 3)])
def test_histogram_sort_passes(capi, big, passes):
    """a colour with `big` k-mers beside colours with 0 and 1: as many 8-bit passes as the maximum has digits"""
    ns = 10
    se = np.concatenate([np.full(big, 3, np.uint32), np.array([4, 5], np.uint32)])
    pse = np.zeros((ns, 2), np.uint32)
    pse[2:, 1] = 6  # colour 6 is named eight times
    got, d = both(capi, se, pse)
    assert got["mer_value"].tolist() == [0, 1, big] and got["mer_freq"].tolist() == [ns - 4, 2, 1]
    assert got["deg_value"].tolist() == [0, 8] and got["deg_freq"].tolist() == [ns - 2, 1]
    assert d["passes_mer"] == passes and d["passes_deg"] == 1


def test_nsubsets_one_and_two(capi):
    got, d = both(capi, [0, 0], [[3, 3]])
    assert len(got["mer_value"]) == 0 and len(got["deg_value"]) == 0
    got, d = both(capi, [1, 1, 0], [[0, 0], [1, 1]])
    assert got["mer_value"].tolist() == [2] and got["deg_value"].tolist() == [2] and got["deg_freq"].tolist() == [1]
    got, d = both(capi, [], [[0, 0], [0, 0]])
    assert got["mer_value"].tolist() == [0] and d["passes_mer"] == 0


def error_of(capi, view, **kw):
    with pytest.raises(capi.KrError) as e:
        capi.index_stats(view, keep_counts=True, **kw)
    assert e.value.code == capi.KR_ERR_FORMAT
    return str(e.value)


@pytest.mark.parametrize("over", [0, 1])
def test_bad_colour_ids(capi, dbg0, over):
    """se == nsubsets and nsubsets + 1 only: the device counters have 64 entries of slack behind nsubsets, so a missing guard would
    show as a wrong answer or a missing error here, never as an access out of bounds"""
    rng = np.random.default_rng(6)
    ns = 500
    bad_id = ns + over
    pse = random_pse(rng, ns)
    se = rng.integers(0, ns, size=3000, dtype=np.uint32)
    se_bad = se.copy()
    se_bad[[700, 2100]] = bad_id
    view, keep = ref.craft_view(capi, [dict(se=se_bad, pse=pse)])
    host = error_of(capi, view)
    assert "cmer[700]" in host and "colour id %d" % bad_id in host
    assert error_of(capi, view, device=0) == host
    pse_bad = pse.copy()
    pse_bad[3, 1] = bad_id
    pse_bad[400, 0] = bad_id
    view2, keep2 = ref.craft_view(capi, [dict(se=se, pse=pse_bad)])
    host = error_of(capi, view2)
    assert "se_to_pse[3]" in host and "colour id %d" % bad_id in host
    assert error_of(capi, view2, device=0) == host
    both(capi, se, pse)  # a good call on the same process succeeds afterwards


@pytest.mark.parametrize("device_view", [False, True])
def test_memory_fallback(capi, dbg0, monkeypatch, device_view):
    rng = np.random.default_rng(7)
    ns = dbg0["cap"] + 300
    monkeypatch.setenv("KR_STATS_MAX_MB", "0")
    got, d = both(capi, rng.integers(0, ns, size=5000, dtype=np.uint32), random_pse(rng, ns), device_view=device_view)
    assert d["path"] == 2
    monkeypatch.delenv("KR_STATS_MAX_MB")
    got, d = both(capi, rng.integers(0, ns, size=5000, dtype=np.uint32), random_pse(rng, ns), device_view=device_view)
    assert d["path"] == 1


def test_toy_index(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    cpu = capi.index_stats(hx, keep_counts=True)
    dev = capi.index_stats(hx, device=0, keep_counts=True)
    L = ref.read_lib(toy_index_dir, "-m4r1-frac")
    ref.assert_stats_equal(dev[0], ref.stats_ref(L["cmer"][:, 1], L["pse"], L["nsubsets"]))
    assert capi.format_inspect(hx, dev) == capi.format_inspect(hx, cpu) == ref.inspect_text(toy_index_dir)
    assert capi.index_stats(hx, device=0)[0]["se_count"] is None
