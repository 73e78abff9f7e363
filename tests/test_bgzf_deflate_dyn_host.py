"""Level 2 of the BGZF encoder on the host (csrc/kr_deflate.h through kr_bgzf_deflate_host_level): the tokens of level 1 under dynamic
Huffman codes.  No device.  Every output passes deflate_cases.check_stream (zlib whole and member by member, the project's own
inflater and walk, header, BSIZE, CRC-32, ISIZE, the n + 31 bound); kr_debug_bgzf_deflate_stats_level shows which block type a
crafted input got; kr_debug_huffman_lengths runs the code-length builder alone.  The device must give the same bytes
(test_gpu_bgzf_deflate_dyn.py)."""
import ctypes as C
import hashlib
import json
import os
import re
import zlib

import numpy as np
import pytest

import deflate_cases as dc
import deflate_dyn_cases as dd
from conftest import GOLDEN, ROOT

NEW = ["kr_bgzf_deflate_host_level", "kr_stream_bgzf_out_level", "kr_debug_bgzf_deflate_stats_level", "kr_debug_huffman_lengths",
       "kr_debug_huffman_lengths_device"]

# Level 2 against zlib level 1 with dynamic codes on the same members: the factor the fixed form is given against Z_FIXED
RATIO_LIMIT = 1.3


@pytest.fixture(scope="module")
def fixture_text():
    return dc.report_text(2000)


def test_the_symbols_are_declared_and_exported(capi):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    declared = set(re.findall(r"KR_API\s+[\w\s\*]+?\b(kr_\w+)\s*\(", hdr))
    for sym in NEW:
        assert sym in declared and sym in capi.EXPORTS and hasattr(lib, sym), sym


# ---- 1. round trip ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dc.cases()) + sorted(dd.dyn_cases()))
def test_every_case_inflates_to_its_input(capi, name):
    data = dc.cases()[name] if name in dc.cases() else dd.dyn_cases()[name]
    comp = capi.bgzf_deflate_host(data, level=2)
    dc.check_stream(capi, data, comp)
    assert capi.bgzf_deflate_host(data, level=2) == comp  # the same call twice
    st = capi.bgzf_deflate_stats(data, level=2)
    assert st["members"] == -(-len(data) // dc.MEMBER) == st["stored"] + st["fixed"] + st["dynamic"]


def test_the_fixture_inflates_to_its_input(capi, fixture_text):
    dc.check_stream(capi, fixture_text, capi.bgzf_deflate_host(fixture_text, level=2))


# ---- 2. never larger -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dc.cases()) + sorted(dd.dyn_cases()) + ["fixture"])
def test_a_level_2_member_is_never_larger_and_keeps_level_1s_bytes_where_it_keeps_its_block(capi, fixture_text, name):
    data = fixture_text if name == "fixture" else dc.cases()[name] if name in dc.cases() else dd.dyn_cases()[name]
    one = dc.members_of(capi, capi.bgzf_deflate_host(data, level=1))
    two = dc.members_of(capi, capi.bgzf_deflate_host(data, level=2))
    assert len(one) == len(two)
    for m1, m2 in zip(one, two):
        assert len(m2) <= len(m1)
        assert dd.btype(m1) in (0, 1) and dd.btype(m2) in (0, 1, 2)
        if dd.btype(m2) != 2:
            assert m2 == m1
        else:
            assert len(m2) < len(m1)


# ---- 3. every route, witnessed by the stats ----------------------------------------------------------------------------------------
def test_bytes_that_do_not_compress_are_stored(capi):
    data = dc.cases()["random_member"]
    st = capi.bgzf_deflate_stats(data, level=2)
    assert st["stored"] == st["members"] == 1 and st["fixed"] == st["dynamic"] == 0 and st["header_bits"] == 0
    assert capi.bgzf_deflate_host(data, level=2) == capi.bgzf_deflate_host(data)


def test_a_short_text_keeps_the_fixed_codes(capi):
    """a dynamic header costs a text of a few bytes more than its codes save (len_63 is long enough to gain: the stats say so)"""
    data = dc.cases()["len_4"]
    st = capi.bgzf_deflate_stats(data, level=2)
    assert st["fixed"] == st["members"] == 1 and st["dynamic"] == st["stored"] == 0 and st["header_bits"] == 0
    assert capi.bgzf_deflate_host(data, level=2) == capi.bgzf_deflate_host(data)
    assert capi.bgzf_deflate_stats(dc.cases()["len_63"], level=2)["dynamic"] == 1


def test_the_fixture_is_all_dynamic(capi, fixture_text):
    st = capi.bgzf_deflate_stats(fixture_text, level=2)
    assert st["members"] == st["dynamic"] == 35 and st["stored"] == st["fixed"] == 0 and st["limited"] == 0
    assert 35 * 100 < st["header_bits"] < 35 * 4500
    one = capi.bgzf_deflate_stats(fixture_text, level=1)
    for key in ("literals", "matches", "longest", "farthest"):  # the same tokens
        assert st[key] == one[key]
    assert one["fixed"] == 35 and one["dynamic"] == one["limited"] == one["header_bits"] == 0


@pytest.mark.parametrize("data", [b"a", dc.cases()["len_1"]], ids=["a", "len_1"])
def test_one_literal(capi, data):
    """one literal and the end of the block, no distance: the distance code is two forced symbols.  The member keeps the fixed codes."""
    st = capi.bgzf_deflate_stats(data, level=2)
    assert (st["literals"], st["matches"], st["members"]) == (1, 0, 1) and st["fixed"] == 1
    comp = capi.bgzf_deflate_host(data, level=2)
    dc.check_stream(capi, data, comp)
    assert comp == capi.bgzf_deflate_host(data)


def test_one_distance_symbol_is_forced_to_two(capi):
    """equal_70000 does not do it: a candidate comes from an earlier tile, so its matches start 1 .. 64 bytes behind one (the stats:
    farthest > 1).  200 bytes without a repeat, twenty times over, do: the only candidate of a position is the one 200 back."""
    st = capi.bgzf_deflate_stats(dc.cases()["equal_70000"], level=2)
    assert st["dynamic"] == st["members"] == 2 and 1 < st["farthest"] <= 64 and st["literals"] == 2 * 64 and st["longest"] == 258
    data = dd.dyn_cases()["one_distance"]
    st = capi.bgzf_deflate_stats(data, level=2)
    assert st["dynamic"] == st["members"] == 1 and st["farthest"] == 200 and st["literals"] >= 200 and st["matches"] >= 10
    mem = dc.check_stream(capi, data, capi.bgzf_deflate_host(data, level=2))
    tokens = zlib.decompressobj(-15)  # every match at distance 200: zlib's output grows by whole matches from byte 200 on
    assert tokens.decompress(mem[0][18:-8]) == data
    assert dd.btype(mem[0]) == 2
    assert mem[0][19] & 31 == 15  # HDIST - 1, behind BFINAL, BTYPE and HLIT (8 bits): distance 200 is symbol 15, and nothing above it


@pytest.mark.parametrize("n", [300, 3000])
def test_no_match_at_all(capi, n):
    """the distance code is empty before forcing; whether the block is dynamic is the sizes' affair: the stats say it"""
    data = dc.distinct(n)
    st = capi.bgzf_deflate_stats(data, level=2)
    assert st["matches"] == 0 and st["literals"] == n and st["stored"] == 0
    mem = dc.check_stream(capi, data, capi.bgzf_deflate_host(data, level=2))
    assert dd.btype(mem[0]) == (2 if st["dynamic"] else 1)
    if n == 3000:
        assert st["dynamic"] == 1  # 3,000 literals from 144 bytes: 8 bits each under the fixed codes, fewer under their own


# ---- 4. the limiter, in a real member ----------------------------------------------------------------------------------------------
def literal_depth(data):
    """the least depth of an optimal code for the bytes of `data` and the end-of-block symbol, from heapq"""
    freq = np.bincount(np.frombuffer(data, np.uint8), minlength=286).astype(np.int64)
    freq[256] = 1
    return dd.huffman_cost_and_depth(freq)[1]


def test_the_limiter_in_a_real_member(capi):
    """39,516 literals, no match; every optimal code for them is 18 deep (the rare bytes' counts are tie-free), so the 15-bit limit
    is needed whatever tree the builder makes"""
    data = dd.limiter_input(True)
    assert literal_depth(data) == 18
    st = capi.bgzf_deflate_stats(data, level=2)
    print("limiter input: %d bytes, stats %r" % (len(data), st))
    assert st["members"] == st["dynamic"] == 1 and st["limited"] >= 1
    assert st["matches"] == 0 and st["literals"] == len(data) == 39516
    comp = capi.bgzf_deflate_host(data, level=2)
    dc.check_stream(capi, data, comp)
    assert len(comp) < 0.7 * len(data)  # 32 fillers of about equal counts and the rarer rest: well below 8 bits a byte


def test_the_fibonacci_member(capi):
    """The issue's input: rare counts 1, 1, 2, 3, 5, ..., 987; 35,353 literals, no match.  A Huffman tree for it CAN be 20 deep, and
    the limit was expected to be needed.  It is not: every Fibonacci sum ties with the next count, the builder takes the leaf before
    the inner node on a tie, and the optimal code it makes is 13 deep (heapq with the same rule agrees).  limited == 0 is then the
    right answer, and the member is coded at the Huffman optimum; test_the_limiter_in_a_real_member has the limiter at work."""
    data = dd.limiter_input(False)
    depth = literal_depth(data)
    st = capi.bgzf_deflate_stats(data, level=2)
    print("Fibonacci input: %d bytes, least optimal depth %d, stats %r" % (len(data), depth, st))
    assert depth == 13
    assert st["members"] == st["dynamic"] == 1 and st["limited"] == (1 if depth > 15 else 0)
    assert st["matches"] == 0 and st["literals"] == len(data) == 35353
    comp = capi.bgzf_deflate_host(data, level=2)
    dc.check_stream(capi, data, comp)
    assert 22000 < len(comp) < 24000  # "about 23 KB against 35,358 stored"


# ---- 5. the builder alone ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(dd.builder_cases()))
def test_the_code_length_builder(capi, name):
    freq, maxbits, expect = dd.builder_cases()[name]
    lens, limited = capi.huffman_lengths(freq, maxbits)
    dd.check_lengths(freq, maxbits, lens, limited, expect)
    assert capi.huffman_lengths(freq, maxbits)[0].tolist() == lens.tolist()


def test_the_builder_refuses_what_it_cannot_code(capi):
    lib = capi.load()
    lens, flag = (C.c_uint8 * 286)(), C.c_uint32(0)
    ok = (C.c_uint32 * 286)(*([1] * 286))
    assert lib.kr_debug_huffman_lengths(ok, 286, 15, lens, C.byref(flag)) == capi.KR_OK
    assert lib.kr_debug_huffman_lengths(None, 286, 15, lens, C.byref(flag)) == capi.KR_ERR_ARG
    assert lib.kr_debug_huffman_lengths(ok, 286, 15, None, C.byref(flag)) == capi.KR_ERR_ARG
    assert lib.kr_debug_huffman_lengths(ok, 286, 15, lens, None) == capi.KR_ERR_ARG
    assert lib.kr_debug_huffman_lengths(ok, 287, 15, lens, C.byref(flag)) == capi.KR_ERR_ARG
    assert lib.kr_debug_huffman_lengths(ok, 0, 15, lens, C.byref(flag)) == capi.KR_ERR_ARG
    assert lib.kr_debug_huffman_lengths(ok, 286, 16, lens, C.byref(flag)) == capi.KR_ERR_ARG
    assert lib.kr_debug_huffman_lengths(ok, 286, 7, lens, C.byref(flag)) == capi.KR_ERR_ARG  # 286 codes of 7 bits: there are 128
    big = (C.c_uint32 * 2)(1 << 22, 1)
    assert lib.kr_debug_huffman_lengths(big, 2, 15, lens, C.byref(flag)) == capi.KR_ERR_ARG


# ---- 6. ratio ----------------------------------------------------------------------------------------------------------------------
def zlib1_dynamic(data):
    """zlib level 1 with dynamic codes on the same members, 26 bytes of BGZF frame a member"""
    total = 0
    for a in range(0, len(data), dc.MEMBER):
        z = zlib.compressobj(1, zlib.DEFLATED, -15, 8, zlib.Z_DEFAULT_STRATEGY)
        total += len(z.compress(data[a:a + dc.MEMBER]) + z.flush()) + 26
    return total


def test_the_ratio_on_report_text(capi, fixture_text):
    one, two, ref = len(capi.bgzf_deflate_host(fixture_text)), len(capi.bgzf_deflate_host(fixture_text, level=2)), zlib1_dynamic(fixture_text)
    n = len(fixture_text)
    print("report text %d bytes: level 1 %d (%.4f), level 2 %d (%.4f), zlib-1 dynamic %d (%.4f), factor %.4f"
          % (n, one, one / n, two, two / n, ref, ref / n, two / ref))
    assert two < one
    assert two <= RATIO_LIMIT * ref


# ---- 7. level 1 unchanged ----------------------------------------------------------------------------------------------------------
def level1_inputs(fixture_text):
    return dict(dc.cases(), report_text_2000=fixture_text)


def test_level_1_writes_the_bytes_it_wrote_before_level_2_existed(capi, fixture_text):
    want = json.load(open(os.path.join(GOLDEN, "bgzf_level1_sha256.json")))
    inputs = level1_inputs(fixture_text)
    assert sorted(want) == sorted(inputs)
    for name, data in inputs.items():
        assert hashlib.sha256(capi.bgzf_deflate_host(data)).hexdigest() == want[name], name
        assert hashlib.sha256(capi.bgzf_deflate_host(data, level=1)).hexdigest() == want[name], name


# ---- 8. arguments ------------------------------------------------------------------------------------------------------------------
def test_levels_other_than_1_and_2_are_refused(capi):
    for level in (0, 3):
        with pytest.raises(capi.KrError) as e:
            capi.bgzf_deflate_host(b"some text", level=level)
        assert e.value.code == capi.KR_ERR_ARG
        with pytest.raises(capi.KrError) as e:
            capi.bgzf_deflate_stats(b"some text", level=level)
        assert e.value.code == capi.KR_ERR_ARG
    lib = capi.load()
    buf, n = (C.c_uint8 * 64)(), C.c_uint64(0)
    assert lib.kr_bgzf_deflate_host_level(None, 64, 2, buf, 64, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_bgzf_deflate_host_level(buf, 64, 2, None, 64, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_bgzf_deflate_host_level(buf, 64, 2, buf, 64, None) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_deflate_stats_level(buf, 64, 2, None) == capi.KR_ERR_ARG
    assert lib.kr_stream_bgzf_out_level(None, 2) == capi.KR_ERR_ARG
    assert lib.kr_debug_huffman_lengths_device(None, buf, 2, 15, buf, C.byref(C.c_uint32(0))) == capi.KR_ERR_ARG


def test_a_buffer_that_is_too_small_is_refused(capi):
    data = dc.cases()["len_%d" % (dc.MEMBER + 1)]
    comp = capi.bgzf_deflate_host(data, level=2)
    assert capi.bgzf_deflate_host(data, cap=len(comp), level=2) == comp
    with pytest.raises(capi.KrError) as e:
        capi.bgzf_deflate_host(data, cap=len(comp) - 1, level=2)
    assert e.value.code == capi.KR_ERR_CAPACITY


def test_no_input_gives_no_member(capi):
    assert capi.bgzf_deflate_host(b"", level=2) == b""
    st = capi.bgzf_deflate_stats(b"", level=2)
    assert st["members"] == 0 and st["dynamic"] == 0


def test_members_deflated_together_equal_members_deflated_alone(capi, fixture_text):
    """35 members spread over the thread pool, each with its thread's state and token list: the bytes of one call a member"""
    comp = capi.bgzf_deflate_host(fixture_text, level=2)
    sizes = [len(m) for m in dc.members_of(capi, comp)]
    one_by_one = b"".join(capi.bgzf_deflate_host(fixture_text[a:a + dc.MEMBER], level=2) for a in range(0, len(fixture_text), dc.MEMBER))
    assert one_by_one == comp and len(sizes) == 35
