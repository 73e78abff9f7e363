"""Every form of the selection (docs/design/05_likelihood_select_rows_text.md: the form table) and the row kernels on crafted records
(tests/select_craft.py), through kr_debug_select: the lane's view is the submit path's own, the launches are launch_select's and
launch_rows'.  Every design runs with the default form and the wave-per-read kernel, with each of the four flag sets, and is held to
tests/select_ref.py with no tolerance: rd_na, every record's selection flag, d and v bit for bit, the reads' row counts and first rows,
the rows in record order (plain: key and the bits of d; indexed: key and the resolved list position, dist_list carrying the bits of d),
and under --filter every record's chi bit for bit against llh_mp.f_ieee."""
import ctypes as C

import numpy as np
import pytest

import select_craft as sc

pytestmark = pytest.mark.gpu

POISON8, POISON32 = 0xA5, 0xA5A5A5A5
POISON64 = np.frombuffer(bytes([0xA5] * 8), np.uint64)[0]


class Env:
    def __init__(self, capi, tmp):
        self.capi = capi
        self.ix = sc.Index()
        self.lay = capi.select_layout()
        self.hx = capi.HostIndex(self.ix.write(str(tmp / "idx")))
        assert self.hx.lib_arrays()["rho"].tolist() == self.ix.rho  # what the filter form reads is what the reference is given
        self.dx = self.hx.upload(0)
        self.designs = sc.designs(self.ix, self.lay)
        self._reads, self._tables, self._refs, self._streams = {}, {}, {}, {}

    def tables(self, name, th):
        if name not in self._reads:
            self._reads[name] = self.designs[name]()
        if (name, th) not in self._tables:
            self._tables[(name, th)] = sc.tables(self._reads[name], th=th, contiguous=name.startswith("neighbours"))
        return self._tables[(name, th)]

    def reference(self, name, th, multi, dmax):
        key = (name, multi, dmax)  # (the threshold changes neither keys nor values: one reference for th 4 and th 2)
        if key not in self._refs:
            self._refs[key] = sc.reference(self.tables(name, th)[1], multi, dmax)
        return self._refs[key]

    def stream(self, th=4, multi=1, dmax=None, no_filter=1, chisq=2.706):
        key = (th, multi, dmax, no_filter, chisq)
        if key not in self._streams:
            p = self.capi.default_params(hdist_th=th, multi=multi, no_filter=no_filter, chisq=chisq, dist_max=float("nan") if dmax is None else dmax)
            self._streams[key] = self.dx.stream(p, max_reads=2048, max_bases=1 << 16, max_records=1 << 17)
        return self._streams[key]

    def close(self):
        for s in self._streams.values():
            s.close()
        self.dx.close()
        self.hx.close()


@pytest.fixture(scope="module")
def env(capi, tmp_path_factory):
    e = Env(capi, tmp_path_factory.mktemp("select_forms"))
    yield e
    e.close()


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def slots_of(t):
    """the record slots of the reads, read by read"""
    return np.concatenate([np.arange(o, o + n, dtype=np.int64) for o, n in zip(t["rd_off"].tolist(), t["rd_cnt"].tolist())] + [np.zeros(0, np.int64)])


def check(capi, out, t, ref, outs, pos, flags, what, filt=False):
    """one kr_debug_select result against select_ref's"""
    nrecs = len(t["rec_key"])
    slots = slots_of(t)
    free = np.ones(nrecs, bool)
    free[slots] = False
    rows_mode = bool(flags & capi.KR_ROWS_ONLY)
    indexed = rows_mode and bool(flags & capi.KR_ROWS_INDEXED) and not filt
    assert (out["rows_mode"], out["rows_indexed"], out["keep_v"]) == (int(rows_mode), int(indexed), int(not rows_mode)), what
    # ---- the reads and their records, as the select kernel left them
    assert out["rd_na"].tolist() == [int(o["na"]) for o in outs], what
    sel = np.array([s for o in outs for s in o["sel"]], np.uint8)
    got = out["rec_sel"][slots]
    bad = np.nonzero(got != sel)[0]
    assert len(bad) == 0, (what, "rec_sel", len(bad), [(int(np.searchsorted(t["rd_off"], slots[i], "right") - 1), int(slots[i])) for i in bad[:5]])
    assert (out["rec_sel"][free] == POISON8).all(), (what, "a selection flag written outside the reads")
    d = np.array([x[1] for recs in ref for x in recs])
    v = np.array([x[2] for recs in ref for x in recs])
    assert (bits(out["rec_d"][slots]) == bits(d)).all(), (what, "rec_d")
    assert (bits(out["rec_d"][free]) == POISON64).all(), (what, "rec_d written outside the reads")
    if out["keep_v"] or filt:  # (the --filter kernel needs v_closest: it writes rec_v in a rows-only batch too)
        assert (bits(out["rec_v"][slots]) == bits(v)).all(), (what, "rec_v")
    if indexed:
        assert (out["rec_rep"][slots] == pos).all(), (what, "the resolved list positions")
    else:
        assert (out["rec_rep"] == t["rec_rep"]).all(), (what, "rec_rep")
    # ---- the rows
    if not rows_mode:
        assert out["nrows"] == 0
        return
    cnt = np.array([len(o["rows"]) for o in outs], np.uint32)
    assert (out["rd_rcnt"] == cnt).all(), (what, "rd_rcnt", np.nonzero(out["rd_rcnt"] != cnt)[0][:5])
    assert out["nrows"] == int(cnt.sum()), what
    first = np.concatenate([[0], np.cumsum(cnt)[:-1]]).astype(np.uint32)
    assert (out["rd_roff"] == first).all(), (what, "rd_roff", np.nonzero(out["rd_roff"] != first)[0][:5])
    nrows = int(out["nrows"])
    keys = np.array([k for o in outs for k, _ in o["rows"]], np.uint32)
    rd = np.array([x for o in outs for _, x in o["rows"]], np.float64)
    bad = np.nonzero(out["row_key"][:nrows] != keys)[0]
    assert len(bad) == 0, (what, "row_key", len(bad), bad[:5])
    if indexed:
        assert (out["row_dix"][:nrows] == pos[sel != 0]).all(), (what, "row_dix")
        assert (bits(out["dist_list"]) == bits(t["rep_dv"][:, 0])).all(), (what, "dist_list")
        assert (bits(out["dist_list"][out["row_dix"][:nrows]]) == bits(rd)).all(), (what, "dist_list[row_dix]")
    else:
        assert (bits(out["row_d"][:nrows]) == bits(rd)).all(), (what, "row_d")


def flag_sets(capi):
    return [0, capi.KR_TAP_ACCS, capi.KR_ROWS_ONLY, capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED]


RANDOM = [d + (f"_s{s}" if s else "") for s in sc.SEEDS for d in ("seams", "ties", "neighbours", "dmax")]
# th = 4: every design with multi 1 / 0 and dist_max unset / at a pool value; the designs whose point is dist_max or a border also one
# double below and above it
CASES = [(name, 4, multi, dmax) for name in RANDOM + [f"waves{n}" for n in sc.WAVE_NREADS] for multi in (1, 0) for dmax in (None, sc.DMAX[0])]
CASES += [(name, 4, multi, dmax) for name in ("dmax", "dmax_s1", "neighbours") for multi in (1, 0) for dmax in sc.DMAX[1:]]
# th = 2, one stream (multi 1, dist_max unset): the general instantiation (planes only, no direct part)
CASES += [(name, 2, 1, None) for name in ("seams", "ties", "neighbours", "neighbours_s1", "waves1040")]


@pytest.mark.parametrize("name,th,multi,dmax", CASES, ids=lambda x: "unset" if x is None else str(x))
def test_every_form_against_the_reference(env, capi, name, th, multi, dmax):
    t, ref, pos = env.tables(name, th)
    outs = env.reference(name, th, multi, dmax)
    st = env.stream(th=th, multi=multi, dmax=dmax)
    for form in (0, 1):
        for flags in flag_sets(capi):
            out = st.debug_select(t, flags=flags, form=form)
            check(capi, out, t, ref, outs, pos, flags, (name, th, multi, dmax, "form", form, "flags", flags))


def test_refusals_on_a_live_stream(env, capi):
    """the limits kr_debug_select checks against are the stream's and the index's own"""
    st = env.stream()
    t, _, _ = env.tables("dmax", 4)
    lib = capi.load()

    def rc(tab, flags=0, form=0, st=st):
        s, keep = capi.select_tables(tab)
        r = capi.KrSelectResult()
        return lib.kr_debug_select(st.h, C.byref(s), flags, form, C.byref(r))

    assert rc(t, form=2) == capi.KR_ERR_ARG and rc(t, flags=capi.KR_TAP_HITS) == capi.KR_ERR_ARG and rc(t, flags=capi.KR_ROWS_INDEXED) == capi.KR_ERR_ARG
    assert rc(dict(t, nreads=2049, rd_off=np.zeros(2049, np.uint32), rd_cnt=np.zeros(2049, np.uint32), rd_onmers=np.zeros(2049, np.uint32))) == capi.KR_ERR_ARG
    key = t["rec_key"].copy()
    key[int(t["rd_off"][-1]) + int(t["rd_cnt"][-1]) - 1] = (env.ix.tree.nnodes + 1) << 1  # the first se beyond rho
    assert rc(dict(t, rec_key=key)) == capi.KR_ERR_ARG
    n = (1 << 17) + 1
    big = dict(rd_off=[0], rd_cnt=[0], rd_onmers=[1], rec_key=np.zeros(n, np.uint32), rec_rep=np.full(n, sc.HOLE, np.uint32), rec_w0=np.zeros(n, np.uint64))
    assert rc(big) == capi.KR_ERR_ARG  # more records than max_records
    t2, _, _ = env.tables("dmax", 2)

    def rc2(tab):
        return rc(tab, st=env.stream(th=2))

    assert rc(t) == capi.KR_OK and rc2(t) == capi.KR_ERR_ARG
    assert st.debug_select(t)["nrows"] == 0 and env.stream(th=2).debug_select(t2)["nrows"] == 0


@pytest.mark.parametrize("th,dmax", [(4, None), (4, sc.POOL[4]), (2, None)], ids=lambda x: "unset" if x is None else str(x))
def test_filter_form_chi_square_bit_for_bit(env, capi, th, dmax):
    """kr_select_kernel<NPT, true> at 0, 1, 63, 64, 65, 128, 129 and 300 records: every record's v is llh_mp.f_ieee of its own problem at
    its own d, the reference chi is 2 (f_ieee(closest's problem, d) - v_closest) in doubles, and rec_chisq carries its bits; records that
    represent no leaf, and every record of an NA read, carry NaN.  The threshold lies in a gap of the case's chi values at least four
    error bounds wide on either side (tests/test_select_craft_cpu.py), so every selection flag is determined and asserted."""
    from llh_mp import M_GPU

    t, ref, fs, errs = sc.filter_case(env.ix, th)
    chisq, outs, ratio = sc.filter_reference(ref, fs, errs, dmax)
    assert ratio >= 4
    st = env.stream(th=th, multi=1, dmax=dmax, no_filter=0, chisq=chisq)
    pos = np.arange(len(t["rec_key"]), dtype=np.uint32)
    want = np.array([np.nan if c is None else c for o in outs for c in o["chi"]])
    err = np.array([np.nan if c is None else 2 * M_GPU * e(o["closest"], recs[i][1]) + np.spacing(abs(c))
                    for recs, o, e in zip(ref, outs, errs) for i, c in enumerate(o["chi"])])
    slots = slots_of(t)
    for form in (0, 1):
        for flags in flag_sets(capi):
            what = ("filter", th, dmax, "form", form, "flags", flags)
            out = st.debug_select(t, flags=flags, form=form)
            got = out["rec_chisq"][slots]
            there = ~np.isnan(want)
            assert np.isnan(got[~there]).all(), (what, "chi of a record that represents nothing")
            worst = float(np.max(np.abs(got[there] - want[there]) / err[there])) if there.any() else 0.0
            print(f"{what}: {int(there.sum())} chi values, {int((bits(got[there]) != bits(want[there])).sum())} differ in bits, worst |chi - ref| / bound {worst:.3g}")
            assert (bits(got[there]) == bits(want[there])).all(), (what, "rec_chisq")
            check(capi, out, t, ref, outs, pos, flags, what, filt=True)
