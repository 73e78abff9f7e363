"""The floating-point part of `krepp dist` / `place` on the device -- objective (pown_dd, kr_log, llh_dpart / llh_combine), Brent,
de-duplication, the (d, v) hand-over to the select kernel -- against the 256-bit reference of tests/llh_mp.py (fixture
tests/golden/llh_mp.npy; only numpy is needed here) and against the straight minimiser on the same problems.

Bounds are in units of the fixture's error unit B.  M_GPU = 2 * M_CPU (tests/test_llh_reference_cpu.py): the device composes two
different < 1 ulp primitives (pown_dd, kr_log) where the CPU composes glibc's, in the same order of operations; their per-operation
errors can add with either sign.  M_GPU is not tuned from what the device returns; the device's measured worst ratios are printed by
the tests and recorded in docs/design/10_oracle.md."""
import ctypes as C
import os
import shutil
import struct

import numpy as np
import pytest

import llh_mp
from helpers import write_index
from llh_mp import M_CPU, M_GPU, minimiser_condition

pytestmark = pytest.mark.gpu

# M_GPU = 2 * M_CPU = 4 (tests/llh_mp.py).  Measured afterwards on an MI355X, worst |f - f_mp| / B: 1.82 (uc0); per class interior 1.54, small_d 1.66,
# half 1.67, rho0 1.45, rho1 1.12, tiny_rho 1.65, big 1.61, boundary 1.20 -- the same with KR_DEBUG_LLH=1


def llh_batch(capi, dx, th, mode, hist, uc, rho, d_in=None):
    """kr_llh_batch: mode 0 -> (d, v) of the minimisation, mode 1 -> f(d_in)"""
    lib = capi.load()
    hist, uc, rho = (np.ascontiguousarray(a, dtype=np.float64) for a in (hist, uc, rho))
    n = len(uc)
    assert hist.shape == (n, th + 1)
    d_in = np.ascontiguousarray(d_in, dtype=np.float64) if d_in is not None else None
    d, v = np.full(n, np.nan), np.full(n, np.nan)
    capi.check(lib.kr_llh_batch(dx.h, th, mode, n, hist.ctypes.data, uc.ctypes.data, rho.ctypes.data,
                                d_in.ctypes.data if d_in is not None else None, d.ctypes.data if mode == 0 else None, v.ctypes.data))
    return (d, v) if mode == 0 else v


def llh_eval_indexed(capi, dx, th, hist, uc, rho, pidx, d_in):
    lib = capi.load()
    vp = C.c_void_p
    lib.kr_llh_eval_indexed.argtypes = [vp, C.c_uint32, C.c_uint64, vp, vp, vp, C.c_uint64, vp, vp, vp]
    hist, uc, rho, d_in = (np.ascontiguousarray(a, dtype=np.float64) for a in (hist, uc, rho, d_in))
    pidx = np.ascontiguousarray(pidx, dtype=np.uint32)
    v = np.full(len(pidx), np.nan)
    capi.check(lib.kr_llh_eval_indexed(dx.h, th, len(uc), hist.ctypes.data, uc.ctypes.data, rho.ctypes.data, len(pidx), pidx.ctypes.data,
                                       d_in.ctypes.data, v.ctypes.data))
    return v


@pytest.fixture(scope="module")
def cases():
    return llh_mp.load_cases()


@pytest.fixture(scope="module")
def kh_indexes(capi, tmp_path_factory):
    """a tiny crafted index of each (k, h): only k, h (and, for batches, rho) matter to the likelihood"""
    out = {}
    for k, h in llh_mp.KH:
        d = str(tmp_path_factory.mktemp(f"ix{k}_{h}"))
        ppos = [int(round(i * (k - 1) / (h - 1))) for i in range(h)]
        write_index(d, k, h, min(65536, max(1, 4 ** h // 256)), 0, False, ppos, {0: [(0, 1)]}, [(0, 0), (0, 1), (0, 2), (1, 2)], [0.0] * 4, nwk="(a:1,b:1);")
        hx = capi.HostIndex(d)
        out[(k, h)] = (hx, hx.upload(0))
    return out


def groups(cases, only_min=False):
    """the fixture's cases by (k, h, th): one device call takes one threshold on one index"""
    g = {}
    for c in cases:
        if only_min and "dstar" not in c:
            continue
        g.setdefault((c["k"], c["h"], c["th"]), []).append(c)
    return g


def arrays(cs):
    return (np.array([c["mc"] for c in cs]), np.array([c["uc"] for c in cs]), np.array([c["rho"] for c in cs]), np.array([c["d"] for c in cs]),
            np.array([c["f"] for c in cs]), np.array([c["B"] for c in cs]))


def check_objective(capi, kh_indexes, cases, tag):
    worst = {}
    rng = np.random.default_rng(3)
    for (k, h, th), cs in sorted(groups(cases).items()):
        dx = kh_indexes[(k, h)][1]
        hist, uc, rho, d, f, B = arrays(cs)
        n0 = len(cs)
        cls = np.array([c["cls"] for c in cs])

        def judge(v, ix, what):
            r = np.abs(v - f[ix]) / B[ix]
            for c_ in np.unique(cls[ix]):
                worst[c_] = max(worst.get(c_, 0.0), float(r[cls[ix] == c_].max()))
            bad = np.nonzero(~(r <= M_GPU))[0]  # (a NaN fails)
            assert len(bad) == 0, (tag, what, k, h, th, cls[ix][bad[0]], d[ix][bad[0]], v[bad[0]], f[ix][bad[0]], float(r[bad[0]]))

        # every case several times over in one call of several thousand, in a shuffled order; the indexed form with the
        # problems stored once
        ix = rng.permutation(np.tile(np.arange(n0), 48))
        judge(llh_batch(capi, dx, th, 1, hist[ix], uc[ix], rho[ix], d[ix]), ix, "batch")
        judge(llh_eval_indexed(capi, dx, th, hist, uc, rho, ix, d[ix]), ix, "indexed")
        if th == 4:  # the sizes around a workgroup, the 4-thread staging (above 2^16) and, at k = 29, the grid-stride loop (above 4096 * 256)
            for n in (1, 255, 256, 257, (1 << 16) + 77) + (((1 << 20) + 300,) if k == 29 else ()):
                ix = np.arange(n) % n0 if n < 300 else rng.integers(0, n0, n)
                judge(llh_batch(capi, dx, th, 1, hist[ix], uc[ix], rho[ix], d[ix]), ix, f"batch n={n}")
                judge(llh_eval_indexed(capi, dx, th, hist, uc, rho, ix, d[ix]), ix, f"indexed n={n}")
    print(f"device |f - f_mp| / B ({tag}), worst per class:", {k_: round(v_, 2) for k_, v_ in worst.items()})


def test_device_objective_within_the_error_unit(capi, kh_indexes, cases):
    """kr_llh_batch(mode 1) and kr_llh_eval_indexed (llh_eval<0>: the general instantiation) on every evaluation case"""
    check_objective(capi, kh_indexes, cases, "pown_dd")


def test_device_objective_has_the_bits_of_ideal_primitives(capi, kh_indexes, cases):
    """The two hand-written primitives, by their own contracts and with no tolerance: the device objective equals llh_mp.f_ieee -- the
    same operations in IEEE doubles with a correctly rounded (1 - d)^k and the classic log -- in every bit, on every case.  pown_dd
    claims correct rounding except near ties (no case lies within its ~2^-45 ulp of one), kr_log claims to be that log, the kernel claims
    the reference's order and is compiled without contraction.  A power a few ulps off or a log coefficient changed in a late digit moves
    bits here, where the bound M_GPU B (which grants k + 3 roundings on the sum) cannot see them."""
    ndiff = 0
    for (k, h, th), cs in sorted(groups(cases).items()):
        hist, uc, rho, d, _, _ = arrays(cs)
        v = llh_batch(capi, kh_indexes[(k, h)][1], th, 1, hist, uc, rho, d)
        want = np.array([llh_mp.f_ieee(k, h, th, c["mc"], c["uc"], c["rho"], c["d"]) for c in cs])
        bad = np.nonzero(v.view(np.uint64) != want.view(np.uint64))[0]
        ndiff += len(bad)
        if len(bad):
            print("differs:", k, h, th, [(cs[i]["cls"], cs[i]["d"], float(v[i]).hex(), float(want[i]).hex()) for i in bad[:4]])
    assert ndiff == 0, f"{ndiff} of {len(cases)} device values differ from the IEEE objective with ideal primitives"


def test_device_objective_with_the_library_pow(capi, kh_indexes, cases, monkeypatch):
    """the same with KR_DEBUG_LLH=1: the device library's pow in place of pown_dd, same bound"""
    monkeypatch.setenv("KR_DEBUG_LLH", "1")
    check_objective(capi, kh_indexes, cases, "ocml pow")


def test_device_minimiser_lies_in_brents_window(capi, po, kh_indexes, cases):
    """kr_llh_batch(mode 0) (brent_min<0>) on every minimised case and kr_debug_brent (brent_min<5> at th = 4, <0> otherwise) on those
    with integer histograms: the minimiser condition of tests/test_llh_reference_cpu.py with M_GPU, the objective at the device's d
    evaluated by kr_llh_batch(mode 1) (pinned above); against the oracle on the same case d within 1e-6 relative (the north-star
    bound) and v within (M_GPU + M_CPU) B."""
    worst_v = worst_d = 0.0
    nint = 0
    for (k, h, th), cs in sorted(groups(cases, only_min=True).items()):
        dx = kh_indexes[(k, h)][1]
        hist, uc, rho, _, _, _ = arrays(cs)
        runs = [("llh_batch", np.arange(len(cs)), llh_batch(capi, dx, th, 0, hist, uc, rho))]
        ii = np.array([i for i, c in enumerate(cs) if not c["frac"]])
        onm = (hist[ii].sum(1) + uc[ii]).astype(np.uint32)
        assert np.all(onm.astype(np.float64) - hist[ii].sum(1) == uc[ii])
        runs.append(("debug_brent", ii, dx.brent(th, hist[ii].astype(np.uint32), onm, rho[ii])))
        nint += len(ii)
        for what, sel, (d, v) in runs:
            assert np.all(np.isfinite(d)) and np.all(np.isfinite(v)), (what, k, th)
            f_at_d = llh_batch(capi, dx, th, 1, hist[sel], uc[sel], rho[sel], d)
            for j, i in enumerate(sel):
                c = cs[i]
                worst_v = max(worst_v, minimiser_condition(c, float(d[j]), float(v[j]), float(f_at_d[j]), M_GPU, what))
                od, ov, _ = po.brent(k, h, th, c["mc"], c["uc"], c["rho"])
                B = llh_mp.err_unit(k, h, th, c["mc"], c["uc"], c["rho"], od)
                assert abs(d[j] - od) <= 1e-6 * od, (what, c["cls"], k, th, d[j], od)
                assert abs(v[j] - ov) <= (M_GPU + M_CPU) * B, (what, c["cls"], k, th, v[j], ov, B)
                worst_d = max(worst_d, abs(d[j] - od) / od)
    assert nint >= 200
    print(f"device minimiser: worst |v - f(d)| / B {worst_v:.2f}, worst |d - d_oracle| / d_oracle {worst_d:.2e}")


# ---------------------------------------------------------------------------
# The production path (kr_dedup_* -> kr_llh_pre_kernel -> kr_llh_kernel -> select) against the straight minimiser
# ---------------------------------------------------------------------------
def run_batch(capi, dx, th, bases, offs, flags, max_records):
    st = dx.stream(params=capi.default_params(hdist_th=th), max_reads=len(offs) - 1, max_bases=len(bases), max_records=max_records)
    st.submit(bases, offs, flags)
    res = st.collect()
    st.close()
    return res


def rows_of(res):
    """(read, key, bits of d, selected, bits of v) of every record, in (read, key) order"""
    o = np.lexsort((res.rec_key, res.rec_read))
    return res.rec_read[o], res.rec_key[o], res.rec_d.view(np.uint64)[o], res.rec_sel[o], res.rec_v.view(np.uint64)[o]


REGIMES = [("default", {}), ("two_lanes", {"KR_LANES": "2", "KR_LANE_MIN_READS": "4"}), ("small_table", {"KR_DD_SHIFT": "8"}),
           ("poison", {"KR_DEBUG_POISON": "all"})]


def check_production(capi, hx, dx, th, bases, offs, monkeypatch, max_records, tag):
    """every record's (rec_d, rec_v) of a tapped batch equals kr_debug_brent on that record's histogram, k-mer count and rho, bit for
    bit -- the pre-kernel's spliced abscissas, the lane-refilled state machine and the de-duplication change no bit ("same
    operations, same order") -- in the default regime; in every other regime each record's (read, key, selected) and the bits of
    its d AND of its v are the default regime's, hence the straight minimiser's too."""
    rho_of = hx.lib_arrays()["rho"]
    base = None
    for name, env in REGIMES:
        for k_, v_ in env.items():
            monkeypatch.setenv(k_, v_)
        res = run_batch(capi, dx, th, bases, offs, capi.KR_TAP_ACCS, max_records)
        for k_ in env:
            monkeypatch.delenv(k_)
        assert res.nrecs > 0, (tag, name)
        assert not np.isnan(res.rec_d[res.rec_sel.astype(bool)]).any() and not np.isnan(res.rec_v[res.rec_sel.astype(bool)]).any(), (tag, name)
        rows = rows_of(res)
        if base is None:
            base = rows
            onm = res.read_onmers[res.rec_read]
            d, v = dx.brent(th, res.rec_hist, onm, rho_of[res.rec_key >> 1])
            nd = int((d.view(np.uint64) != res.rec_d.view(np.uint64)).sum())
            nv = int((v.view(np.uint64) != res.rec_v.view(np.uint64)).sum())
            print(f"{tag} th={th}: {res.nrecs} records, {nd} differ in d, {nv} in v from the straight minimiser; "
                  f"counts above 255: {int((res.rec_hist.max(1) > 255).sum())}, k-mers above 255: {int((onm > 255).sum())}")
            assert nd == 0 and nv == 0, (tag, th, nd, nv)
        else:
            if len(rows[0]) != len(base[0]) or not (np.array_equal(rows[0], base[0]) and np.array_equal(rows[1], base[1])):
                a, b = set(zip(rows[0].tolist(), rows[1].tolist())), set(zip(base[0].tolist(), base[1].tolist()))
                raise AssertionError((tag, th, name, "records (read, key) only here", sorted(a - b)[:20], "only in the default regime", sorted(b - a)[:20]))
            for a, b in zip(rows, base):
                assert np.array_equal(a, b), (tag, th, name)
    return base


def doubled(bases, offs):
    """every read twice: half of all problems are duplicates"""
    n = len(offs) - 1
    lens = np.diff(offs).astype(np.int64)
    return np.concatenate([bases, bases]), np.concatenate([[0], np.cumsum(np.concatenate([lens, lens]))]).astype(np.uint64), 2 * n


def with_rho(src, dst, values):
    """a copy of an index directory whose leaves' rho cycle through `values` (crecord: counts, colour pairs, then rho)"""
    shutil.copytree(src, dst)
    path = [os.path.join(dst, f) for f in os.listdir(dst) if f.startswith("crecord")][0]
    raw = bytearray(open(path, "rb").read())
    nrho, npse = struct.unpack_from("<II", raw, 0)
    rho = np.array([values[i % len(values)] for i in range(nrho)], np.float64)
    raw[8 + 8 * npse:8 + 8 * npse + 8 * nrho] = rho.tobytes()
    assert len(raw) == 8 + 8 * npse + 8 * nrho
    open(path, "wb").write(raw)
    return rho


@pytest.mark.parametrize("th", [2, 4, 6])
def test_production_path_equals_straight_minimiser_toy(capi, synth, toy_genomes, toy_index_dir, tmp_path, monkeypatch, th):
    """the toy index with 3,000 reads of 150 bases, and with its rho replaced by 0, 1e-9, 0.3, 1 in turn, reads of 90, 150 and 5,000
    bases (more than 255 k-mers leave the direct part, counts above 255 the table); th != 4 has no packed word: every record is its
    own problem through load_problem"""
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    bases, offs, _ = synth.sample_reads(toy_genomes, 3000, seed=91)
    check_production(capi, hx, dx, th, bases, offs, monkeypatch, 0, "toy")
    # (the loader scales a library's rho by (r + 1) / m = 1 / 2 on this index, Index::make_rho_partial: the file holds the doubles)
    with_rho(toy_index_dir, str(tmp_path / "ix"), [0.0, 2e-9, 0.6, 2.0])
    hx2 = capi.HostIndex(str(tmp_path / "ix"))
    assert set(hx2.lib_arrays()["rho"].tolist()) == {0.0, 1e-9, 0.3, 1.0}
    dx2 = hx2.upload(0)
    parts = [synth.sample_reads(toy_genomes, n, seed=92 + i, length=L)[:2] for i, (n, L) in enumerate(((600, 90), (600, 150), (40, 5000)))]
    bases = np.concatenate([p[0] for p in parts])
    offs = np.concatenate([[0], np.cumsum(np.concatenate([np.diff(p[1]).astype(np.int64) for p in parts]))]).astype(np.uint64)
    b2, o2, _ = doubled(bases, offs)
    rows = check_production(capi, hx2, dx2, th, b2, o2, monkeypatch, 0, "rho 0 / 1e-9 / 0.3 / 1")
    assert {float(x) for x in hx2.lib_arrays()["rho"][np.unique(rows[1] >> 1)]} == {0.0, 1e-9, 0.3, 1.0}  # leaves of every rho are met


def test_production_path_equals_straight_minimiser_star_tree_and_small_table(capi, synth, tmp_path, monkeypatch):
    """160 close relatives (hundreds of records per read, most of them not direct: every leaf is a problem of its own), every read
    twice.  With KR_DD_SHIFT=8 the table has its floor of 1,024 slots for tens of thousands of distinct problems: duplicates find no
    room (the crowded mode or the 48-round limit) and become list entries of their own -- shown by the list of a one-lane indexed
    batch being longer than the default's; a run that cannot show it fails."""
    n = 160
    names = [f"s{i}" for i in range(n)]
    nwk = "(" + ",".join(f"{x}:0.003" for x in names) + ");"
    g = synth.evolve_genomes(nwk, 4000, seed=23)
    tsv = synth.write_genomes(g, str(tmp_path / "g"))
    (tmp_path / "t.nwk").write_text(nwk)
    idx = str(tmp_path / "ix")
    capi.build_index(tsv, idx, nwk=str(tmp_path / "t.nwk"), k=29, w=31, h=13, m=2, r=0, frac=True, num_threads=4)
    hx = capi.HostIndex(idx)
    dx = hx.upload(0)
    bases, offs, _ = synth.sample_reads(g, 400, seed=4)
    b2, o2, nreads = doubled(bases, offs)
    cap = nreads * 2 * n
    rows = check_production(capi, hx, dx, 4, b2, o2, monkeypatch, cap, "star")
    assert len(rows[0]) > 50 * nreads
    monkeypatch.setenv("KR_LANES", "1")
    nlist = {}
    for shift in ("1", "8"):
        monkeypatch.setenv("KR_DD_SHIFT", shift)
        res = run_batch(capi, dx, 4, b2, o2, capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED, cap)
        assert res.rec_dix is not None and res.rec_v is None  # (a rows-only batch carries DIST alone: v was compared in check_production)
        nlist[shift] = len(res.dist_list)
        sel = rows[3].astype(bool)
        got = sorted(zip(res.rec_read.tolist(), res.rec_key.tolist(), res.rec_d.view(np.uint64).tolist()))
        assert got == sorted(zip(rows[0][sel].tolist(), rows[1][sel].tolist(), rows[2][sel].tolist())), shift
    print("list of distinct problems: default table", nlist["1"], "entries, 1,024-slot table", nlist["8"])
    assert nlist["8"] > nlist["1"] + nreads  # the duplicates that found no room
