"""kr_debug_select / kr_debug_select_check / kr_debug_select_layout (include/krepp_amd.h) as far as no device is needed: the symbols, NULL
arguments, the documented layout, and every reason kr_debug_select has to refuse a table."""
import ctypes as C

import numpy as np

import select_craft as sc


def good():
    """two reads of 3 and 2 records, a slot between them"""
    return dict(rd_off=[0, 4], rd_cnt=[3, 2], rd_onmers=[100, 100], rec_key=[2, 3, 8, 0, 4, 10], rec_rep=[0, 1, sc.DIRECT_FLAG | 1, sc.HOLE, 1, 0],
                rec_w0=[1 << 63 | 1, 0, 1 << 63 | 1, 0, 0, 1 << 63 | 1], rec_hist=np.ones((6, 5), np.uint32), rec_read=[0, 0, 0, 0, 1, 1],
                rep_dv=[[0.1, -1.0], [0.2, -2.0]], dd_direct=[sc.HOLE, 1], dd_dv=[[0.0, 0.0], [0.2, -2.0]])


def test_symbols_and_null_arguments(capi):
    lib = capi.load()
    for sym in ("kr_debug_select", "kr_debug_select_check", "kr_debug_select_layout"):
        assert hasattr(lib, sym) and sym in capi.EXPORTS
    t, keep = capi.select_tables(good())
    r = capi.KrSelectResult()
    assert lib.kr_debug_select(None, C.byref(t), 0, 0, C.byref(r)) == capi.KR_ERR_ARG and b"kr_debug_select" in lib.kr_last_error()
    assert lib.kr_debug_select(None, None, 0, 0, None) == capi.KR_ERR_ARG
    assert lib.kr_debug_select_check(None, 1, 1, 1, 4, 0) == capi.KR_ERR_ARG
    assert lib.kr_debug_select_layout(None) == capi.KR_ERR_ARG


def test_layout_is_the_documented_one(capi):
    assert capi.select_layout() == dict(lane_max=8, group_small=16, group_mid=32, wave_gl=64, big_regs=256, big_step2=128, row_block=1024,
                                        row_round=16)


def test_every_refusal(capi):
    lim = dict(max_reads=2, max_records=6, nnodes=6, hdist_th=4, direct_nodes=1)
    assert capi.select_check(good(), **lim) == capi.KR_OK

    def refused(what, lim=lim, **change):
        t = good()
        for k, v in change.items():
            if callable(v):
                v(t[k])
            else:
                t[k] = v
        assert capi.select_check(t, **lim) == capi.KR_ERR_ARG, what
        assert b"kr_debug_select" in capi.load().kr_last_error()

    def put(i, v):
        return lambda a: a.__setitem__(i, v)

    refused("more reads than the stream holds", lim=dict(lim, max_reads=1))
    refused("no reads", nreads=0)
    refused("more records than the stream holds", lim=dict(lim, max_records=5))
    refused("list longer than the records' capacity", lim=dict(lim, max_records=6), nrep=7)
    refused("problems beyond the list", problems=3)
    refused("more direct places than the stream has", lim=dict(lim, direct_nodes=0))
    refused("keys equal", rec_key=put(1, 2))
    refused("keys descend", rec_key=put(2, 1))
    refused("key beyond the nodes", rec_key=put(5, 12))
    refused("a read leaves the records", rd_cnt=put(1, 3))
    refused("reads overlap", rd_off=put(1, 2))
    refused("reads descend", rd_off=[4, 0], rd_cnt=[2, 3])
    refused("hole inside a read", rec_rep=put(1, sc.HOLE))
    refused("list position out of range", rec_rep=put(0, 2))
    refused("direct place out of range", rec_rep=put(2, sc.DIRECT_FLAG | 2))
    refused("direct place that names nothing", rec_rep=put(2, sc.DIRECT_FLAG | 0))
    refused("direct place whose position is out of range", dd_direct=put(1, 2))
    refused("a packed word without hdist_th 4", lim=dict(lim, hdist_th=2, direct_nodes=0), dd_direct=None, dd_dv=None, rec_rep=put(2, 0))
    refused("planes-only record without planes", rec_hist=None, rec_read=None)
    refused("planes without the records' reads", rec_read=None)
    refused("a planes-only record of another read", rec_read=put(1, 1))
    refused("null read table", rd_onmers=None)
    refused("null record table", rec_w0=None, nrecs=6)
    refused("null list", rep_dv=None, nrep=2)
    refused("null direct places", dd_dv=None, ndirect=2)
