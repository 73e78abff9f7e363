"""kr_debug_dedup / kr_debug_dedup_check / kr_debug_dedup_layout (include/krepp_amd.h) as far as no device is needed: the symbols, NULL
arguments, and every reason kr_debug_dedup has to refuse a table, each by name."""
import ctypes as C

import numpy as np

import dedup_craft as dc

W = dc.pack((1, 0, 0, 0, 0), 100)


def good():
    """two reads of 3 and 2 records with a hole between them and one behind; records 1 and 4 travel as planes"""
    return dict(rd_off=[0, 4], rd_cnt=[3, 2], rd_onmers=[100, 100], rec_key=[2, 3, 8, 0, 4, 10, 0], rec_w0=[W, 0, W, 0, 0, W, 0],
                rec_hist=np.ones((7, 5), np.uint32), rec_read=[0, 0, 0, 0, 1, 1, 0])


def test_symbols_and_null_arguments(capi):
    lib = capi.load()
    for sym in ("kr_debug_dedup", "kr_debug_dedup_check", "kr_debug_dedup_layout"):
        assert hasattr(lib, sym) and sym in capi.EXPORTS
    t, keep = capi.dedup_tables(good())
    r = capi.KrDedupResult()
    assert lib.kr_debug_dedup(None, C.byref(t), C.byref(r)) == capi.KR_ERR_ARG and b"kr_debug_dedup" in lib.kr_last_error()
    assert lib.kr_debug_dedup(None, None, None) == capi.KR_ERR_ARG
    assert lib.kr_debug_dedup_check(None, 1, 1, 1, 4) == capi.KR_ERR_ARG and b"kr_debug_dedup_check" in lib.kr_last_error()
    assert lib.kr_debug_dedup_layout(None) == capi.KR_ERR_ARG and b"kr_debug_dedup_layout" in lib.kr_last_error()


def test_every_refusal(capi):
    lim = dict(max_reads=2, max_records=7, nnodes=6, hdist_th=4)
    assert capi.dedup_check(good(), **lim) == capi.KR_OK
    planes = dict(good(), rec_w0=[0] * 7)
    assert capi.dedup_check(planes, **dict(lim, hdist_th=2)) == capi.KR_OK  # (no packed word: any threshold)

    def refused(what, reason, lim=lim, **change):
        t = good()
        for k, v in change.items():
            if callable(v):
                v(t[k])
            else:
                t[k] = v
        assert capi.dedup_check(t, **lim) == capi.KR_ERR_ARG, what
        msg = capi.load().kr_last_error()
        assert msg.startswith(b"kr_debug_dedup: ") and reason in msg, (what, msg)

    def put(i, v):
        return lambda a: a.__setitem__(i, v)

    refused("more reads than the stream holds", b"nreads out of range", lim=dict(lim, max_reads=1))
    refused("no reads", b"nreads out of range", nreads=0)
    refused("more records than the stream holds", b"more records", lim=dict(lim, max_records=6))
    refused("a read leaves the records", b"read ranges overlap, descend or leave", rd_cnt=put(1, 4))
    refused("reads overlap", b"read ranges overlap, descend or leave", rd_off=put(1, 2))
    refused("reads descend", b"read ranges overlap, descend or leave", rd_off=[4, 0], rd_cnt=[2, 3])
    refused("key beyond the nodes", b"key beyond the index's nodes", rec_key=put(5, 12))
    refused("key 0 inside a read", b"hole (key 0) inside a read", rec_key=put(1, 0))
    refused("a record between the reads", b"record outside the reads' ranges", rec_key=put(3, 2))
    refused("a record behind the reads", b"record outside the reads' ranges", rec_key=put(6, 2))
    refused("a packed word at threshold 2", b"threshold other than 4", lim=dict(lim, hdist_th=2))
    refused("a packed word at threshold 6", b"threshold other than 4", lim=dict(lim, hdist_th=6))
    refused("a packed word without bit 63", b"without bit 63", rec_w0=put(2, W & ~(1 << 63)))
    refused("a packed word with another k-mer count", b"k-mer count is not its read's", rec_w0=put(5, dc.pack((1, 0, 0, 0, 0), 101)))
    refused("a packed word with another k-mer count (the read's changed)", b"k-mer count is not its read's", rd_onmers=put(0, 99))
    refused("no word and no histogram", b"without a histogram", rec_hist=None, rec_read=None)
    refused("planes without the records' reads", b"come together", rec_read=None)
    refused("a planes-only record of another read", b"names another read", rec_read=put(1, 1))
    refused("a planes-only record of no read", b"names another read", rec_read=put(4, 7))
    refused("null read table", b"null read table", rd_onmers=None)
    refused("null record table", b"null record table", rec_w0=None, nrecs=7)
