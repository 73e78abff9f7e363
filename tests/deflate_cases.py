"""Inputs for the BGZF encoder's tests (test_bgzf_deflate_host.py, test_gpu_bgzf_deflate.py): each the smallest input that reaches its
seam, and the checks every output must pass whatever produced it."""
import functools
import gzip
import struct
import zlib

import numpy as np

MEMBER = 0xFF00  # input bytes of a member
EOF_MEMBER = bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000")


def distinct(n, start=0, avoid=b""):
    """n bytes below 144 (8-bit literals) in which no 4 consecutive bytes occur twice (a counter over the bytes outside `avoid`):
    nothing to match"""
    alphabet = [b for b in range(144) if b not in avoid]
    out = bytearray()
    i = start
    while len(out) < n:
        out += bytes([alphabet[i % 251 % len(alphabet)], alphabet[i // 251 % 241 % len(alphabet)], alphabet[(i * 7 + 3) % 239 % len(alphabet)]])
        i += 1
    return bytes(out[:n])


def report_text(nreads, seed=1):
    """the report-shaped text of the design note: nreads x 33 rows `SRR1234567.N <tab> G######### <tab> 0.##### <newline>`, the
    reference names from a vocabulary of 500"""
    rng = np.random.default_rng(seed)
    vocab = [b"G%09d" % v for v in rng.integers(0, 10**9, 500)]
    rows = []
    for r in range(nreads):
        rid = b"SRR1234567.%d" % r
        for ref, d in zip(rng.integers(0, 500, 33), rng.integers(0, 100000, 33)):
            rows.append(b"%s\t%s\t0.%05d\n" % (rid, vocab[ref], d))
    return b"".join(rows)


def far_match(offset, extra):
    """A = 100 distinct bytes other than 'x' at `offset`, then 'x' up to distance 32,768 (+ extra), then A again"""
    a = distinct(100, 7, avoid=b"x")
    return b"x" * offset + a + b"x" * (32768 - len(a) + extra) + a


@functools.lru_cache(maxsize=None)
def cases():
    """name -> bytes"""
    rng = np.random.default_rng(20240702)
    out = {}
    text = report_text(100)
    for n in (0, 1, 3, 4, 63, 64, 65, 128, MEMBER - 1, MEMBER, MEMBER + 1, 3 * MEMBER + 1):
        out["len_%d" % n] = (text * (n // len(text) + 1))[:n]
    out["equal_70000"] = b"a" * 70000
    for ln in (3, 4, 257, 258, 259):
        x = distinct(ln, 1000)
        out["match_%d" % ln] = x + distinct(70, 5000) + x + distinct(5, 9000)
    for off in (0, 1, 63, 64):
        out["dist_32768_at_%d" % off] = far_match(off, 0)
        out["dist_32769_at_%d" % off] = far_match(off, 1)
    out["random_member"] = rng.integers(0, 256, MEMBER, dtype=np.uint8).tobytes()
    out["random_1000"] = rng.integers(0, 256, 1000, dtype=np.uint8).tobytes()
    return out


def members_of(capi, comp):
    """comp cut into its BGZF members with kr_bgzf_member_size"""
    out, off = [], 0
    while off < len(comp):
        ms = capi.bgzf_member_size(comp[off:off + 65536])
        assert 28 <= ms <= len(comp) - off, (off, ms)
        out.append(comp[off:off + ms])
        off += ms
    return out


def check_stream(capi, data, comp):
    """what every encoder output must satisfy for the input `data`; returns the members"""
    assert gzip.decompress(comp + capi.bgzf_eof()) == data
    assert len(comp) <= capi.bgzf_deflate_bound(len(data))
    mem = members_of(capi, comp)
    assert len(mem) == -(-len(data) // MEMBER)
    for i, m in enumerate(mem):
        part = data[i * MEMBER:(i + 1) * MEMBER]
        assert zlib.decompress(m, wbits=31) == part
        assert len(m) <= len(part) + 31
        assert m[:16] == EOF_MEMBER[:16] and struct.unpack("<H", m[16:18])[0] == len(m) - 1  # header, BSIZE
        crc, isize = struct.unpack("<II", m[-8:])
        assert isize == len(part) and crc == zlib.crc32(part)
    if comp:
        assert capi.bgzf_inflate_host(comp) == data
    assert capi.bgzf_walk(comp, 1 << 40) == (len(mem), len(comp), len(data))
    return mem


def is_stored(member):
    return (member[18] & 6) == 0  # BTYPE 00
