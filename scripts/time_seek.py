#!/usr/bin/env python3
"""`seek` batches that are resident in HBM, through the C ABI, two ways in alternating rounds of ONE process:
  old   kr_batch_submit (the dist chain on the sketch as a one-leaf index; a long sequence with KR_TILE_DEVICE) + kr_batch_collect +
        kr_format_seek on the host
  new   kr_batch_submit_text(KR_SEEK) + kr_batch_collect_text: the seek kernels, the report text written by the device
Sketch: one synthetic genome of 5 Mbp, k 26 (the defaults of `krepp sketch`).  Legs: 1 M and 4 M reads of 150 bases (1 % substitutions),
and the genome itself (1 % substitutions) as one contig.  Per leg, after the warm-up rounds: the device time of the last batch (old:
kr_batch_timing's total; new: kr_debug_seek_ms' hist / solve / text), the host clock around collect (+ format) -- both end in a stream
synchronise --, and reads/s from the host clock around the whole of submit .. text in host memory.  The two texts must be equal.
usage: time_seek.py [rounds] [out.txt]"""
import ctypes as C
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from krepp_amd import capi

rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 10
out_path = sys.argv[2] if len(sys.argv) > 2 else None
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ACGT = np.frombuffer(b"ACGT", np.uint8)
rng = np.random.default_rng(17)
G = 5_000_000
genome = ACGT[rng.integers(0, 4, G)]
work = tempfile.mkdtemp(prefix="krepp_seek_")
fa, skc = os.path.join(work, "g.fa"), os.path.join(work, "g.skc")
with open(fa, "wb") as f:
    f.write(b">g\n" + genome.tobytes() + b"\n")
capi.build_sketch(fa, skc)
hx = capi.HostIndex(skc, sketch=True)
dx = hx.upload(0)
lib = capi.load()
lib.kr_format_seek.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(capi.KrResultView), C.c_uint32, C.c_void_p, C.POINTER(C.c_void_p), C.POINTER(C.c_uint64)]
TH = 4


def mutate(a, rate):
    n = int(rate * a.size)
    flat = a.reshape(-1)
    flat[rng.integers(0, a.size, n)] = ACGT[rng.integers(0, 4, n)]


def reads_leg(n):
    starts = rng.integers(0, G - 150, n)
    a = genome[starts[:, None] + np.arange(150)[None, :]]
    mutate(a, 0.01)
    return a.reshape(-1), (np.arange(n + 1, dtype=np.uint64) * 150)


def contig_leg():
    a = genome.copy()
    mutate(a, 0.01)
    return a, np.array([0, G], np.uint64)


def med(xs):
    return float(np.median(xs))


for what, (bases, offs) in (("1 M reads x 150", reads_leg(1_000_000)), ("4 M reads x 150", reads_leg(4_000_000)), ("1 contig x 5 Mbp", contig_leg())):
    n = len(offs) - 1
    blob = b"\0".join(b"r%d" % i for i in range(n)) + b"\0"
    ids = np.frombuffer(blob, np.uint8)
    id_off = np.zeros(n + 1, np.uint32)
    id_off[1:] = np.cumsum(np.fromiter((len(b"r%d" % i) + 1 for i in range(n)), np.uint32, n))
    name_ptrs = (ids.ctypes.data + id_off[:-1].astype(np.uint64)).astype(np.uint64)
    tb, to = torch.from_numpy(bases).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    long_seq = n == 1
    vmax = n + (G // 128 + 1024 if long_seq else 0)
    old = dx.stream(params=capi.default_params(hdist_th=TH), max_reads=vmax, max_bases=len(bases) + 64)
    new = dx.stream(params=capi.default_params(hdist_th=TH), max_reads=n, max_bases=len(bases) + 64)
    new.seek_enable(max(1 << 20, 32 * n), len(blob))
    old_flags = capi.KR_BASES_DEVICE | (capi.KR_TILE_DEVICE if long_seq else 0)
    t = {k: [] for k in ("old_all", "old_collect", "old_format", "old_dev", "new_all", "new_collect", "new_hist", "new_solve", "new_text")}
    texts = {}
    # (a stream that is given batches of a million reads tries other item lists during its first 13 batches: the old path is timed after them)
    warm = 14 if n >= 1_000_000 else 2
    for rnd in range(rounds + warm):
        # ---- old
        t0 = time.perf_counter()
        capi.check(lib.kr_batch_submit(old.h, tb.data_ptr(), to.data_ptr(), n, old_flags))
        t1 = time.perf_counter()
        old.collect_view()
        t2 = time.perf_counter()
        txt, ln = C.c_void_p(), C.c_uint64()
        capi.check(lib.kr_format_seek(hx.h, dx.h, C.byref(old._rv), TH, name_ptrs.ctypes.data, C.byref(txt), C.byref(ln)))
        t3 = time.perf_counter()
        if rnd == rounds + warm - 1:
            texts["old"] = C.string_at(txt, ln.value)
        lib.kr_free(txt)
        dev_old = old.timing().ms_total
        # ---- new
        t4 = time.perf_counter()
        capi.check(lib.kr_batch_submit_text(new.h, tb.data_ptr(), to.data_ptr(), n, capi.KR_BASES_DEVICE | capi.KR_SEEK, ids.ctypes.data, id_off.ctypes.data, 1))
        t5 = time.perf_counter()
        ptr, ln2 = C.c_void_p(), C.c_uint64()
        capi.check(lib.kr_batch_collect_text(new.h, C.byref(ptr), C.byref(ln2)))
        t6 = time.perf_counter()
        if rnd == rounds + warm - 1:
            texts["new"] = C.string_at(ptr, ln2.value)
        ms = new.seek_ms()
        if rnd >= warm:
            t["old_all"].append(t3 - t0), t["old_collect"].append(t2 - t1), t["old_format"].append(t3 - t2), t["old_dev"].append(dev_old)
            t["new_all"].append(t6 - t4), t["new_collect"].append(t6 - t5)
            t["new_hist"].append(ms[0]), t["new_solve"].append(ms[1]), t["new_text"].append(ms[2])
    assert texts["old"] == texts["new"] and len(texts["new"]) > 0, "the two reports differ"
    say(f"== {what}: {len(texts['new'])} bytes of report, {rounds} rounds after {warm} warm-ups (medians)")
    say(f"  old: kernels {med(t['old_dev']):9.3f} ms   collect {med(t['old_collect']) * 1e3:9.3f} ms + kr_format_seek {med(t['old_format']) * 1e3:9.3f} ms   "
        f"end to end {med(t['old_all']) * 1e3:9.3f} ms (min {min(t['old_all']) * 1e3:.3f})   {n / med(t['old_all']):14.0f} reads/s")
    say(f"  new: hist {med(t['new_hist']):7.3f} + solve {med(t['new_solve']):7.3f} + text {med(t['new_text']):7.3f} ms   collect_text {med(t['new_collect']) * 1e3:9.3f} ms   "
        f"end to end {med(t['new_all']) * 1e3:9.3f} ms (min {min(t['new_all']) * 1e3:.3f})   {n / med(t['new_all']):14.0f} reads/s")
    old.close(), new.close()
    del tb, to
if out_path:
    with open(out_path, "w") as f:
        f.write("\n".join(lines) + "\n")
