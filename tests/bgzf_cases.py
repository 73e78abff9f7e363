"""BGZF members for the tests of the device's inflate (tests/test_bgzf_host.py on the CPU, tests/test_gpu_bgzf_*.py on the GPU).
zlib is the reference throughout: every member's expected bytes are what zlib.decompress gives for its payload, and every case is
built once per session (corpus() and damaged() are cached)."""
import functools
import struct
import zlib

import numpy as np


def wrap(payload, data):
    """a raw deflate payload as a BGZF member: the 18-byte header, the payload, CRC-32 and ISIZE of `data`"""
    bsize = 12 + 6 + len(payload) + 8 - 1
    assert bsize < 65536, bsize
    return (b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, bsize) + payload +
            struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data)))


def deflate(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flushes=()):
    """raw deflate of `data`; flushes: (position, mode) pairs, the stream is flushed with that mode at those positions"""
    co = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    out, pos = b"", 0
    for at, mode in flushes:
        out += co.compress(data[pos:at]) + co.flush(mode)
        pos = at
    return out + co.compress(data[pos:]) + co.flush()


def member(data, level=6, strategy=zlib.Z_DEFAULT_STRATEGY, mem_level=8, flushes=()):
    return wrap(deflate(data, level, strategy, mem_level, flushes), data)


EOF_MEMBER = member(b"")


def members(data, block=20000, level=6, eof=True):
    """`data` in members of `block` bytes: (the file's bytes, each member's offset in it, each member's first inflated byte)"""
    out, offs, ustart = bytearray(), [], []
    for i in range(0, len(data), block):
        offs.append(len(out))
        ustart.append(i)
        out += member(data[i:i + block], level)
    if eof:
        offs.append(len(out))
        ustart.append(len(data))
        out += EOF_MEMBER
    return bytes(out), offs, ustart


class Bits:
    """a deflate bit stream: fields LSB first, Huffman codes MSB first"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def bits(self, v, n):
        self.acc |= (v & ((1 << n) - 1)) << self.n
        self.n += n
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, n):
        for i in range(n - 1, -1, -1):
            self.bits((c >> i) & 1, 1)

    def align(self):
        if self.n:
            self.bits(0, 8 - self.n)

    def bytes(self):
        self.align()
        return bytes(self.out)


def single_distance_code():
    """a dynamic block whose distance alphabet is ONE code of length 1 (an incomplete set zlib accepts): literal 'A' has code 0,
    end-of-block 10, length 3 (symbol 257) 11; distance 1 has code 0.  "A", then 40 matches of 3 at distance 1."""
    w = Bits()
    w.bits(1, 1), w.bits(2, 2)                      # last block, dynamic
    w.bits(1, 5), w.bits(0, 5), w.bits(14, 4)       # HLIT 258, HDIST 1, HCLEN 18
    order = [16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15]
    cl = {0: 2, 1: 2, 2: 2, 18: 2}                  # codes: 0 -> 00, 1 -> 01, 2 -> 10, 18 -> 11
    for s in order[:18]:
        w.bits(cl.get(s, 0), 3)
    code = {0: 0, 1: 1, 2: 2, 18: 3}

    def zeros(n):
        w.code(code[18], 2), w.bits(n - 11, 7)

    zeros(65), w.code(code[1], 2)                   # lengths of 0..64: 0; 'A': 1
    zeros(138), zeros(52)                           # 66..255: 0
    w.code(code[2], 2), w.code(code[2], 2)          # 256, 257: 2
    w.code(code[1], 2)                              # the distance code: length 1
    w.code(0, 1)                                    # 'A'
    for _ in range(40):
        w.code(3, 2), w.code(0, 1)                  # length 3, distance 1
    w.code(2, 2)                                    # end of block
    return w.bytes()


def distance_32768(rng):
    """a stored block of 32,768 random bytes, then a fixed-Huffman block with one match of 258 at distance 32,768 (zlib's own
    deflate never looks further back than 32,506)"""
    head = rng.integers(0, 256, 32768, dtype=np.uint8).tobytes()
    w = Bits()
    w.bits(0, 1), w.bits(0, 2), w.align()
    w.bits(32768, 16), w.bits(32768 ^ 0xFFFF, 16)
    w.out += head
    w.bits(1, 1), w.bits(1, 2)
    w.code(0xC0 + 5, 8)                             # symbol 285: length 258
    w.code(29, 5), w.bits(32768 - 24577, 13)        # distance code 29 + 13 extra bits
    w.code(0, 7)                                    # end of block
    return w.bytes()


def fastq_text(rng, nreads, length=150, name=b"r"):
    acgt, qual = np.frombuffer(b"ACGT", np.uint8), np.frombuffer(b"#5?FIJ", np.uint8)
    recs = []
    for i in range(nreads):
        ln = int(rng.integers(max(1, length // 2), length + 1))
        recs.append(b"@%s%d\n%s\n+\n%s\n" % (name, i, acgt[rng.integers(0, 4, ln)].tobytes(), qual[rng.integers(0, len(qual), ln)].tobytes()))
    return b"".join(recs)


@functools.lru_cache(maxsize=None)
def corpus():
    """name -> (BGZF bytes, the bytes zlib inflates them to).  One member each unless the name says otherwise."""
    rng = np.random.default_rng(20240611)
    text = fastq_text(rng, 300)[:60000]
    fib, skew = [1, 1], bytearray()
    while sum(fib) + fib[-1] + fib[-2] <= 65536:
        fib.append(fib[-1] + fib[-2])
    for i, f in enumerate(fib):
        skew += bytes([i]) * f
    skew = bytes(np.random.default_rng(5).permutation(np.frombuffer(bytes(skew), np.uint8)))
    two = bytes(np.where(rng.random(65536) < 0.03, 66, 65).astype(np.uint8))
    rnd = rng.integers(0, 256, 65536, dtype=np.uint8).tobytes()
    d32k = distance_32768(rng)
    cases = {
        "eof_member": (EOF_MEMBER, b""),
        "one_byte": (member(b"A"), b"A"),
        "two_bytes": (member(b"AC"), b"AC"),
        "isize_65535": (member(rnd[:20000] + text[:45535], 6), rnd[:20000] + text[:45535]),
        "isize_65536": (member((text * 2)[:65536], 6), (text * 2)[:65536]),
        "stored": (member(text[:30000], 0), text[:30000]),
        "fixed": (member(text, 6, zlib.Z_FIXED), text),
        "huffman_only": (member(text[:40000], 6, zlib.Z_HUFFMAN_ONLY), text[:40000]),
        "rle": (member(b"A" * 30000 + b"C" * 999 + text[:5000], 6, zlib.Z_RLE), b"A" * 30000 + b"C" * 999 + text[:5000]),
        "level1": (member(text, 1), text),
        "level6": (member(text, 6), text),
        "level9": (member(text, 9), text),
        "flushes": (member(text, 6, flushes=((1000, zlib.Z_SYNC_FLUSH), (1000, zlib.Z_FULL_FLUSH), (20000, zlib.Z_FULL_FLUSH), (45000, zlib.Z_SYNC_FLUSH))), text),
        "one_byte_64k": (member(b"G" * 65536), b"G" * 65536),
        "random_64k": (member(rnd[:0xff00], 6), rnd[:0xff00]),  # (bgzip's 64 KB: what still fits a member when nothing compresses)
        "two_symbols": (member(two, 9), two),
        "skewed_lengths": (member(skew, 9), skew),
        "distance_32768": (wrap(d32k, zlib.decompress(d32k, -15)), zlib.decompress(d32k, -15)),
        "single_distance_code": (wrap(single_distance_code(), b"A" * 121), b"A" * 121),
    }
    assert zlib.decompress(single_distance_code(), -15) == b"A" * 121
    assert len(cases["distance_32768"][1]) == 32768 + 258 and cases["distance_32768"][1][-258:] == cases["distance_32768"][1][:258]
    for k in (1, 4, 5, 64, 257):  # workgroup and grid tails: four members a workgroup
        parts = [text[(37 * i) % 50000:][:(1 + (211 * i) % 1500)] for i in range(k)]
        cases["members_%d" % k] = (b"".join(member(p, 1 + i % 9) for i, p in enumerate(parts)), b"".join(parts))
    return cases


def small_members():
    """(a ~300-byte dynamic-Huffman member, a fixed-Huffman member, their inflated bytes): the members whose every bit is flipped"""
    text = fastq_text(np.random.default_rng(9), 4, 90)
    dyn, fix = member(text, 6), member(text, 6, zlib.Z_FIXED)
    assert 250 <= len(dyn) <= 400 and dyn[18] & 6 == 4 and fix[18] & 6 == 2, (len(dyn), dyn[18], fix[18])
    return dyn, fix, text


def set_isize(m, isize):
    return m[:-4] + struct.pack("<I", isize)


def with_payload(m, payload):
    """the member m with another payload (BSIZE follows; the trailer stays)"""
    bsize = 18 + len(payload) + 8 - 1
    return m[:16] + struct.pack("<H", bsize) + payload + m[-8:]


@functools.lru_cache(maxsize=None)
def damaged():
    """name -> (BGZF bytes of ONE damaged member, the words its error message must hold).  Every one is rejected by the decoder's
    host instantiation (tests/test_bgzf_host.py checks that before any of them reaches a GPU)."""
    dyn, fix, text = small_members()
    w = Bits()
    w.bits(1, 1), w.bits(1, 2), w.code(1, 7), w.code(0, 5), w.code(0, 7)  # fixed block: length 3 at distance 1 with no output yet
    return {
        "bad_crc": (dyn[:-8] + struct.pack("<I", (zlib.crc32(text) ^ 1) & 0xFFFFFFFF) + dyn[-4:], "wrong CRC-32"),
        "isize_minus_1": (set_isize(dyn, len(text) - 1), "more output than ISIZE"),
        "payload_cut_by_one": (with_payload(dyn, dyn[18:-9]), "the payload ends inside a block"),
        "distance_in_front": (wrap(w.bytes(), b"AAA"), "distance in front of the member's output"),
        "block_type_3": (wrap(b"\x07", b""), "block type 3"),
    }
