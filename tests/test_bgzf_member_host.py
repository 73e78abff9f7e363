"""The BGZF encoder's member length as a parameter (csrc/kr_deflate.h: the cut is made outside deflate_member;
kr_bgzf_deflate_host_member, kr_bgzf_deflate_bound_member), on the host, no device.  At 65,280 the bytes are
kr_bgzf_deflate_host_level's; at any other length from 256 the output is whole members of that many input bytes (the last one
shorter) that gzip inflates to the text.  Nothing is compared with a tolerance."""
import gzip
import struct
import zlib

import pytest

import deflate_cases as dc

LENGTHS = (256, 257, 4099, 16320, 65279)


@pytest.mark.parametrize("level", [1, 2])
def test_the_default_length_gives_the_bytes_of_the_level_call(capi, level):
    for name, data in sorted(dc.cases().items()):
        got = capi.bgzf_deflate_host_member(data, level, dc.MEMBER)
        assert got == capi.bgzf_deflate_host(data, level=level), name
    assert capi.bgzf_deflate_bound_member(10**6, dc.MEMBER) == capi.bgzf_deflate_bound(10**6)


def texts(L):
    """k L - 1, k L and k L + 1 bytes of report-shaped text for k = 1 and 3, and the same lengths of bytes nothing matches in"""
    text = dc.report_text(max(60, 3 * L // 1000 + 10), seed=L)
    assert len(text) > 3 * L + 1
    out = {}
    for k in (1, 3):
        for d in (-1, 0, 1):
            out["text_%dL%+d" % (k, d)] = text[:k * L + d]
    out["distinct_3L+1"] = dc.distinct(3 * L + 1, L)  # stored or barely coded members: the slot's last bytes
    return out


@pytest.mark.parametrize("level", [1, 2])
@pytest.mark.parametrize("L", LENGTHS)
def test_other_lengths(capi, L, level):
    for name, data in texts(L).items():
        comp = capi.bgzf_deflate_host_member(data, level, L)
        n = len(data)
        k, cb, u = capi.bgzf_walk(comp, 1 << 40)  # whole members to the end
        assert (k, cb, u) == (-(-n // L), len(comp), n), name
        assert gzip.decompress(comp) == data, name
        assert len(comp) <= capi.bgzf_deflate_bound_member(n, L) == n + 31 * k, name
        for i, m in enumerate(dc.members_of(capi, comp)):  # the cuts are where the length says
            part = data[i * L:(i + 1) * L]
            assert zlib.decompress(m, wbits=31) == part and len(m) <= len(part) + 31, (name, i)
            assert struct.unpack("<II", m[-8:]) == (zlib.crc32(part), len(part)), (name, i)
        assert capi.bgzf_inflate_host(comp) == data, name


def test_a_level_2_member_is_never_larger(capi):
    data = dc.report_text(200)
    for L in LENGTHS:
        one = dc.members_of(capi, capi.bgzf_deflate_host_member(data, 1, L))
        two = dc.members_of(capi, capi.bgzf_deflate_host_member(data, 2, L))
        assert len(one) == len(two) and all(len(b) <= len(a) for a, b in zip(one, two))


@pytest.mark.parametrize("L", [0, 255, 65281, 1 << 20])
def test_bad_arguments(capi, L):
    for level in (1, 2):
        with pytest.raises(capi.KrError) as e:
            capi.bgzf_deflate_host_member(b"some text", level, L, cap=1000)
        assert e.value.code == capi.KR_ERR_ARG
    assert capi.bgzf_deflate_bound_member(1000, L) == 0


def test_a_bad_level_and_a_small_buffer(capi):
    with pytest.raises(capi.KrError) as e:
        capi.bgzf_deflate_host_member(b"some text", 3, 4099)
    assert e.value.code == capi.KR_ERR_ARG
    data = dc.report_text(30)
    comp = capi.bgzf_deflate_host_member(data, 1, 257)
    with pytest.raises(capi.KrError) as e:
        capi.bgzf_deflate_host_member(data, 1, 257, cap=len(comp) - 1)
    assert e.value.code == capi.KR_ERR_CAPACITY
    assert capi.bgzf_deflate_host_member(b"", 1, 257) == b""
