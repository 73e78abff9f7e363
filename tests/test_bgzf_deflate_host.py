"""The BGZF encoder's host instantiation (csrc/kr_deflate.h through kr_bgzf_deflate_host): no device.  Every output is inflated with
zlib -- whole and member by member -- and with the project's own decoder and walk; header, BSIZE, CRC-32, ISIZE and the bound are
checked; kr_debug_bgzf_deflate_stats shows that a crafted input took the path it was built for.  The device's kernel must give the
same bytes (test_gpu_bgzf_deflate.py)."""
import ctypes as C
import os
import re
import subprocess
import sys
import zlib

import pytest

import deflate_cases as dc
from conftest import ROOT

NEW = ["kr_bgzf_deflate_bound", "kr_bgzf_deflate_host", "kr_bgzf_eof", "kr_debug_bgzf_deflate_stats", "kr_stream_bgzf_out_enable",
       "kr_batch_collect_text_bgzf", "kr_debug_bgzf_deflate", "kr_debug_bgzf_deflate_ms"]

# Our size against zlib level 1 with Z_FIXED on the same members.  zlib-1 follows hash chains of depth 4 and takes candidates from
# anywhere; the encoder sees one candidate a position, never from the position's own tile of 64.
RATIO_LIMIT = 1.3


def test_the_symbols_are_declared_and_exported_and_reject_null_arguments(capi):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    declared = set(re.findall(r"KR_API\s+[\w\s\*]+?\b(kr_\w+)\s*\(", hdr))
    for sym in NEW:
        assert sym in declared and sym in capi.EXPORTS and hasattr(lib, sym), sym
    buf, n, ms, p = (C.c_uint8 * 64)(), C.c_uint64(0), C.c_float(0), C.c_void_p()
    assert lib.kr_bgzf_deflate_host(None, 64, buf, 64, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_bgzf_deflate_host(buf, 64, None, 64, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_bgzf_deflate_host(buf, 64, buf, 64, None) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_deflate_stats(buf, 64, None) == capi.KR_ERR_ARG
    assert lib.kr_stream_bgzf_out_enable(None) == capi.KR_ERR_ARG
    assert lib.kr_batch_collect_text_bgzf(None, C.byref(p), C.byref(n), C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_deflate(None, buf, 64, buf, 64, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_deflate_ms(None, C.byref(ms)) == capi.KR_ERR_ARG
    lib.kr_bgzf_eof(None)  # (nothing to write to: nothing happens)


def test_the_bound_and_the_end_member(capi):
    assert capi.bgzf_eof() == dc.EOF_MEMBER and capi.bgzf_member_size(capi.bgzf_eof()) == 28
    assert zlib.decompress(capi.bgzf_eof(), wbits=31) == b""
    for n, want in ((0, 0), (1, 32), (dc.MEMBER, dc.MEMBER + 31), (dc.MEMBER + 1, dc.MEMBER + 1 + 62), (10 * dc.MEMBER, 10 * dc.MEMBER + 310)):
        assert capi.bgzf_deflate_bound(n) == want


@pytest.mark.parametrize("name", sorted(dc.cases()))
def test_every_case_inflates_to_its_input(capi, name):
    data = dc.cases()[name]
    comp = capi.bgzf_deflate_host(data)
    dc.check_stream(capi, data, comp)
    assert capi.bgzf_deflate_host(data) == comp  # the same call twice
    assert capi.bgzf_deflate_stats(data)["members"] == -(-len(data) // dc.MEMBER)


def test_no_input_gives_no_member(capi):
    assert capi.bgzf_deflate_host(b"") == b"" and capi.bgzf_deflate_stats(b"")["members"] == 0


def test_a_buffer_that_is_too_small_is_refused(capi):
    data = dc.cases()["len_%d" % (dc.MEMBER + 1)]
    comp = capi.bgzf_deflate_host(data)
    assert capi.bgzf_deflate_host(data, cap=len(comp)) == comp
    with pytest.raises(capi.KrError) as e:
        capi.bgzf_deflate_host(data, cap=len(comp) - 1)
    assert e.value.code == capi.KR_ERR_CAPACITY


def test_long_overlapping_matches(capi):
    data = dc.cases()["equal_70000"]
    st = capi.bgzf_deflate_stats(data)
    assert st["members"] == 2 and st["stored"] == 0 and st["longest"] == 258
    # the first tile of a member has nothing to match; from there on matches of 258, the last one ending on the member's last byte
    assert st["literals"] == 2 * 64 and st["matches"] == -(-(dc.MEMBER - 64) // 258) + -(-(70000 - dc.MEMBER - 64) // 258)
    assert len(capi.bgzf_deflate_host(data)) < 1000


@pytest.mark.parametrize("ln", [3, 4, 257, 258, 259])
def test_match_lengths(capi, ln):
    """X, 70 distinct bytes, X again: candidates are found by a hash of 4 bytes, so X of 3 bytes is not found, longer ones are, cut at 258"""
    st = capi.bgzf_deflate_stats(dc.cases()["match_%d" % ln])
    assert st["stored"] == 0
    if ln == 3:
        assert st["matches"] == 0
    else:
        assert st["matches"] >= 1 and st["longest"] == min(ln, 258) and st["farthest"] == ln + 70


@pytest.mark.parametrize("off", [0, 1, 63, 64])
def test_the_distance_limit(capi, off):
    at = capi.bgzf_deflate_stats(dc.cases()["dist_32768_at_%d" % off])
    assert at["farthest"] == 32768 and at["stored"] == 0
    beyond = capi.bgzf_deflate_stats(dc.cases()["dist_32769_at_%d" % off])
    assert beyond["farthest"] < 32769 and beyond["stored"] == 0
    assert beyond["literals"] >= at["literals"] + 90  # the second A went out as literals


@pytest.mark.parametrize("name", ["random_member", "random_1000"])
def test_bytes_that_do_not_compress_are_stored(capi, name):
    data = dc.cases()[name]
    comp = capi.bgzf_deflate_host(data)
    mem = dc.members_of(capi, comp)
    assert len(mem) == 1 and dc.is_stored(mem[0]) and len(comp) == len(data) + 31
    st = capi.bgzf_deflate_stats(data)
    assert st["stored"] == st["members"] == 1


def test_the_bytes_do_not_depend_on_the_thread_count(capi):
    data = dc.report_text(1000) + dc.cases()["random_member"] + dc.cases()["equal_70000"]  # 17 members and more: several a thread
    assert len(data) > 16 * dc.MEMBER
    want = capi.bgzf_deflate_host(data)
    code = ("import sys, hashlib; sys.path.insert(0, %r); sys.path.insert(0, %r)\n"
            "import deflate_cases as dc\nfrom krepp_amd import capi\n"
            "data = dc.report_text(1000) + dc.cases()['random_member'] + dc.cases()['equal_70000']\n"
            "print(hashlib.sha256(capi.bgzf_deflate_host(data)).hexdigest())\n") % (ROOT, os.path.join(ROOT, "tests"))
    import hashlib
    for nt in ("1", "4"):
        r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, KR_HOST_THREADS=nt), capture_output=True, text=True, check=True)
        assert r.stdout.strip() == hashlib.sha256(want).hexdigest(), nt


def zlib1_fixed(data):
    """zlib level 1 with fixed codes on the same members, 26 bytes of BGZF frame a member"""
    total = 0
    for a in range(0, len(data), dc.MEMBER):
        z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_FIXED)
        total += len(z.compress(data[a:a + dc.MEMBER]) + z.flush()) + 26
    return total


def test_the_ratio_on_report_text_stays_near_zlib_level_1(capi):
    data = dc.report_text(2000)
    ours, ref = len(capi.bgzf_deflate_host(data)), zlib1_fixed(data)
    print("report text %d bytes: ours %d (%.4f), zlib-1 Z_FIXED %d (%.4f), factor %.4f" % (len(data), ours, ours / len(data), ref, ref / len(data), ours / ref))
    assert ours <= RATIO_LIMIT * ref
    assert capi.bgzf_deflate_stats(data)["stored"] == 0
