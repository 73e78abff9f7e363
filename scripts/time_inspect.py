#!/usr/bin/env python3
"""Times the statistics of `krepp inspect` through the C ABI on the benchmark index of bench.py (--workload syn1000: 1000 genomes,
the table inflated with random filler to --index-gb GB) in one session on one GPU:
  (a) kr_index_stats_cpu
  (b) kr_index_stats_device from the host view: the whole call, and the split into H2D copies and count kernels by events
  (c) ... with KR_VIEW_DEVICE (cmer uploaded first): the count kernel's bytes read per second
  (d) the count kernel on two adversarial tables: every entry in one colour; all colours distinct and at or above the LDS cap
      (--distinct-entries of them: the colour record of such a table has as many entries)
  (e) (c) with the LDS route switched off (KR_STATS_LDS_CAP=0)
One warm-up call and --repeats timed calls each; min / median / max are printed and written to --out.

  python scripts/time_inspect.py --out profiles/inspect_timing.txt [--index-gb 10] [--index-dir DIR]
--index-dir: statistics of a built index directory as well (host view, device view is not made), e.g. the 256-genome index of
docs/design/07."""
import argparse
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--index-gb", type=float, default=10.0)
    ap.add_argument("--genomes", type=int, default=1000)
    ap.add_argument("--genome-len", type=int, default=100_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--distinct-entries", type=int, default=1 << 28)
    ap.add_argument("--index-dir", default=None)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from krepp_amd import capi, synth

    capi.load()
    dev = torch.device("cuda", a.device)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def spread(v):
        return "min %.4f  median %.4f  max %.4f  (n=%d)" % (min(v), statistics.median(v), max(v), len(v))

    def timed(label, view, nbytes, device=None, flags=capi.KR_VIEW_HOST, env=None, repeats=None):
        old = {k_: os.environ.get(k_) for k_ in (env or {})}
        os.environ.update(env or {})
        try:
            wall, copy, kern, rest = [], [], [], []
            out = None
            for it in range(1 + (repeats or a.repeats)):
                t0 = time.perf_counter()
                out = capi.index_stats(view, device=device, view_flags=flags)
                dt = time.perf_counter() - t0
                if it == 0:
                    continue  # warm-up
                wall.append(dt)
                if device is not None:
                    d = capi.index_stats_debug()
                    copy.append(d["copy_ms"] / 1e3), kern.append(d["kernel_ms"] / 1e3), rest.append(d["rest_ms"] / 1e3)
            say("%s\n    whole call, s:      %s" % (label, spread(wall)))
            if device is not None:
                d = capi.index_stats_debug()
                say("    H2D copies, s:      %s" % spread(copy))
                say("    count kernels, s:   %s   = %.1f GB/s of cmer read at the median" % (spread(kern), nbytes / statistics.median(kern) / 1e9))
                say("    out-degrees + histograms, s: %s" % spread(rest))
                say("    path %d, chunks %d, LDS increments %d, global increments %d, LDS cap %d, sort passes %d / %d" %
                    (d["path"], d["chunks"], d["lds"], d["global"], d["cap"], d["passes_mer"], d["passes_deg"]))
            return out
        finally:
            for k_, v in old.items():
                if v is None:
                    os.environ.pop(k_, None)
                else:
                    os.environ[k_] = v

    def same(x, y):
        return all(np.array_equal(x[0][k_], y[0][k_]) for k_ in ("mer_value", "mer_freq", "deg_value", "deg_freq"))

    say("# time_inspect.py: %s, torch %s, one session, warm-up 1, repeats %d" % (torch.cuda.get_device_name(dev), torch.__version__, a.repeats))
    if a.index_dir:
        hx = capi.HostIndex(a.index_dir)
        nb = sum(hx.view.libs[i].nkmers for i in range(hx.view.nlibs)) * 8
        say("## built index %s: %d libraries, %.3f GB of cmer" % (a.index_dir, hx.view.nlibs, nb / 1e9))
        c = timed("(a) kr_index_stats_cpu", hx.view, nb)
        d = timed("(b) kr_index_stats_device, host view", hx.view, nb, device=a.device)
        say("    equal lists: %s" % same(c, d))

    work = tempfile.mkdtemp(prefix="krepp_time_inspect_")
    nwk_text = synth.yule_newick(a.genomes, 2)
    genomes = synth.evolve_genomes(nwk_text, a.genome_len, seed=2)
    open(os.path.join(work, "yule.nwk"), "w").write(nwk_text)
    tsv = synth.write_genomes(genomes, os.path.join(work, "g"))
    idx = os.path.join(work, "idx")
    capi.build_index(tsv, idx, nwk=os.path.join(work, "yule.nwk"), k=29, w=35, h=13, m=4, r=1, frac=True, num_threads=16)
    hx = capi.HostIndex(idx)
    inc, cmer, shm = synth.inflate_in_child(idx, a.index_gb, a.device)
    try:
        n = cmer.size // 2
        nb = n * 8
        lv = capi.KrLibView()
        C.memmove(C.byref(lv), C.byref(hx.view.libs[0]), C.sizeof(lv))
        lv.cmer = C.cast(cmer.ctypes.data, capi.u32p)
        lv.nkmers = n
        arr = (capi.KrLibView * 1)(lv)
        view = capi.KrIndexView()
        C.memmove(C.byref(view), C.byref(hx.view), C.sizeof(view))
        view.libs = arr
        say("## syn1000 benchmark table: %d entries (%.2f GB of cmer), %d colours, %d tree nodes" % (n, nb / 1e9, lv.nsubsets, hx.nnodes))
        ra = timed("(a) kr_index_stats_cpu", view, nb, repeats=2)
        rb = timed("(b) kr_index_stats_device, host view (chunks through page-locked staging)", view, nb, device=a.device)
        say("    equal lists (a) == (b): %s" % same(ra, rb))

        t_cmer = torch.from_numpy(cmer.view(np.int32)).to(dev)
        t_pse = torch.from_numpy(hx.lib_arrays(0)["pse"].view(np.int32).copy()).to(dev)
        torch.cuda.synchronize()
        dlv = capi.KrLibView()
        C.memmove(C.byref(dlv), C.byref(lv), C.sizeof(lv))
        dlv.cmer = C.cast(t_cmer.data_ptr(), capi.u32p)
        dlv.pse = C.cast(t_pse.data_ptr(), capi.u32p)
        darr = (capi.KrLibView * 1)(dlv)
        dview = capi.KrIndexView()
        C.memmove(C.byref(dview), C.byref(view), C.sizeof(view))
        dview.libs = darr
        rc = timed("(c) kr_index_stats_device, KR_VIEW_DEVICE (cmer read in place)", dview, nb, device=a.device, flags=capi.KR_VIEW_DEVICE)
        say("    equal lists (a) == (c): %s;  docs/design/02 measured 6.9 TB/s for lines streamed from HBM on this machine" % same(ra, rc))
        re_ = timed("(e) as (c) with the LDS route off (KR_STATS_LDS_CAP=0)", dview, nb, device=a.device, flags=capi.KR_VIEW_DEVICE,
                    env={"KR_STATS_LDS_CAP": "0"}, repeats=2)
        say("    equal lists (a) == (e): %s" % same(ra, re_))

        # (d) adversarial tables, in device memory
        t_cmer[:, 1] = 7  # every entry in one colour
        torch.cuda.synchronize()
        timed("(d1) every entry in colour 7 (all increments on one LDS counter), %d entries" % n, dview, nb, device=a.device, flags=capi.KR_VIEW_DEVICE)
        del t_cmer, t_pse
        torch.cuda.empty_cache()
        cap = capi.index_stats_debug()["cap"]
        nd = min(n, a.distinct_entries)
        ns = cap + nd
        d_cmer = torch.zeros((nd, 2), dtype=torch.int32, device=dev)
        d_cmer[:, 1] = (torch.randperm(nd, device=dev) + cap).to(torch.int32)
        d_pse = torch.zeros((ns, 2), dtype=torch.int32, device=dev)
        torch.cuda.synchronize()
        dlv.cmer = C.cast(d_cmer.data_ptr(), capi.u32p)
        dlv.pse = C.cast(d_pse.data_ptr(), capi.u32p)
        dlv.nkmers, dlv.nsubsets = nd, ns
        darr[0] = dlv
        timed("(d2) all colours distinct and at or above the cap (all increments global), %d entries, %d colours" % (nd, ns), dview, nd * 8,
              device=a.device, flags=capi.KR_VIEW_DEVICE, repeats=2)
    finally:
        import shutil

        shutil.rmtree(shm, True)
        shutil.rmtree(work, True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        open(a.out, "w").write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
