"""The seek batch's C ABI without a device: the four entry points are declared and exported, NULL arguments are refused, the unit
size is a whole number of segments, `krepp seek --help` names the flag; and the two brute forces of tests/seek_craft.py agree with
each other and with the oracle on which reads match at all."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import seek_craft as sc
from conftest import ROOT

NAMES = ("kr_stream_seek_enable", "kr_batch_collect_seek", "kr_debug_seek_layout", "kr_debug_seek_ms")


def test_symbols_declared_and_exported(capi):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    for n in NAMES:
        assert re.search(r"KR_API\s+int\s+" + n + r"\s*\(", hdr), n
        assert n in capi.EXPORTS and hasattr(lib, n), n
    assert re.search(r"#define\s+KR_SEEK\s+256u", hdr) and capi.KR_SEEK == 256
    assert "typedef struct kr_seek_view" in hdr
    # the mirror of kr_seek_view: two counts, four pointers
    assert C.sizeof(capi.KrSeekView) == 8 + 4 * 8
    assert [f[0] for f in capi.KrSeekView._fields_] == ["nreads", "np", "d", "d_strand", "hist", "onmers"]
    flags = [capi.KR_BASES_DEVICE, capi.KR_TAP_ACCS, capi.KR_TAP_HITS, capi.KR_BASES_PINNED, capi.KR_ROWS_ONLY, capi.KR_ROWS_INDEXED,
             capi.KR_TILE_DEVICE, capi.KR_TILE_ROWS]
    assert all(capi.KR_SEEK & f == 0 for f in flags)


def test_null_arguments_are_refused(capi):
    lib = capi.load()
    v = capi.KrSeekView()
    ms = (C.c_float * 3)()
    assert lib.kr_stream_seek_enable(None, 0, 0) == capi.KR_ERR_ARG
    assert lib.kr_stream_seek_enable(None, 1 << 20, 1 << 20) == capi.KR_ERR_ARG
    assert lib.kr_batch_collect_seek(None, C.byref(v)) == capi.KR_ERR_ARG
    assert lib.kr_debug_seek_ms(None, ms) == capi.KR_ERR_ARG
    assert lib.kr_debug_seek_layout(None) == capi.KR_ERR_ARG
    assert b"null" in lib.kr_last_error() or b"argument" in lib.kr_last_error()


def test_unit_is_whole_segments(capi):
    lay = capi.seek_layout()
    assert lay["segment"] == 128
    assert lay["unit"] > 0 and lay["unit"] % 128 == 0
    assert lay["hist_waves"] >= 1 and lay["row_block"] == 1024


def test_help_lists_the_flag():
    exe = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
    r = subprocess.run([exe, "seek", "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--gpu-seek" in r.stdout and "seek kernels and report text on the GPU (identical output)" in r.stdout
    r = subprocess.run([exe, "dist", "--help"], capture_output=True, text=True)
    assert "--gpu-seek" not in r.stdout.split("krepp seek")[0]


def test_brute_forces_agree(capi, po, tmp_path):
    """the literal brute force (closed_form / row_of per k-mer) against its numpy twin, on all three sketches; and against the oracle:
    a read is NaN exactly when no bin of either strand counts anything"""
    rng = np.random.default_rng(5)
    T = capi.seek_layout()["unit"]  # (reads of T and T + 1 positions: the lengths the unit split's seam tests are crafted at)
    for name, cfg, glen in (("a", sc.CFG_A, 9000), ("b", sc.CFG_B, 9000), ("c", sc.CFG_C, 9000)):
        g = sc.random_dna(rng, glen)
        sk = po.Sketch(sc.write_sketch(capi, tmp_path, name, [g], cfg))
        reads = [g[100:250], sc.revcomp(g[400:520]), sc.mutate(rng, g[1000:1300], 0.05), g[2000:2100] + "N" + g[2101:2200], "N" * 40,
                 sc.random_dna(rng, 150), g[5:5 + cfg["k"]], g[7:7 + cfg["k"] - 1], g[3000:3150].lower(), g[3000:3100] + "\xc1" + g[3101:3200],
                 g[4000:4000 + T + cfg["k"] - 1], g[4000:4000 + T + cfg["k"] - 2] + "N" + g[4000 + T + cfg["k"] - 1:4000 + 2 * T]]
        for th in (0, 4, 6):
            h1, o1 = sc.brute_hist(sk, reads, th)
            h2, o2 = sc.brute_hist_np(sk, reads, th)
            assert np.array_equal(h1, h2) and np.array_equal(o1, o2), (name, th)
            bases, offs = sc.pack(reads)
            rows = po.Sketch.seek(sk, bases, offs, [f"r{i}" for i in range(len(reads))], hdist_th=th)["rows"]
            assert np.array_equal(np.isnan(rows["d_llh"]), h1.sum(axis=(1, 2)) == 0), (name, th)
        assert h1[0, 0].sum() > 0 and h1[1, 1].sum() > 0 and o1[7] == 0 and o1[6] == 1
        assert o1[10] == T and o1[11] == 2 * T - 2 * cfg["k"] + 1  # (the N takes the k positions that hold it)
        sk.close()
