"""Ordinary gzip inputs for the device inflater's tests (test_gzip_sym_host.py on the serial twin, test_gpu_gzip_inflate.py on the
kernels), built with Python's zlib: FASTQ-shaped text from a seeded generator -- names with a running number, 150 random bases,
spread-out qualities, so the stream is not trivially compressible -- compressed in the ways that reach the inflater's paths.

A case is (name, gzip bytes, sub_bytes, ratio_cap, max_comp_bytes).  Fixture A: 600 records at memLevel 3 with sub 1,024: every
1,024-byte range holds a block start (blocks of 284-728 compressed bytes), so all but the last searched sub-chunk find a true start
and every window is inherited across many chunks.  Fixture B: 300 records at the default memLevel with sub 4,096: three blocks, so
nearly every searched sub-chunk finds none and the chunk that runs decodes through the empty ones.  (memLevel 1 is no way to small
blocks: its blocks fall below the 256 symbols a block start must decode to.)"""
import functools
import random
import struct
import zlib

BIG = 1 << 20  # a super-chunk that holds every input here


def fastq_text(records, seed, first=0):
    rng = random.Random(seed)
    out = []
    for i in range(first, first + records):
        seq = "".join(rng.choice("ACGT") for _ in range(150))
        qual = "".join(chr(33 + rng.randrange(41)) for _ in range(150))
        out.append("@read%d/1 run=%d\n%s\n+\n%s\n" % (i, seed, seq, qual))
    return "".join(out).encode()


def member(data, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY, flush_at=None, flush=zlib.Z_SYNC_FLUSH):
    c = zlib.compressobj(level, zlib.DEFLATED, 31, mem_level, strategy)
    if flush_at is None:
        return c.compress(data) + c.flush()
    return c.compress(data[:flush_at]) + c.flush(flush) + c.compress(data[flush_at:]) + c.flush()


def wrap(raw, data, flags=0):
    """a raw deflate stream as a gzip member; flags: FEXTRA 4, FNAME 8, FCOMMENT 16, FHCRC 2"""
    h = bytes([0x1F, 0x8B, 8, flags, 0, 0, 0, 0, 0, 3])
    if flags & 4:
        h += struct.pack("<H", 6) + b"ab\x02\x00xy"
    if flags & 8:
        h += b"reads.fq\0"
    if flags & 16:
        h += b"a comment\0"
    if flags & 2:
        h += struct.pack("<H", zlib.crc32(h) & 0xFFFF)
    return h + raw + struct.pack("<II", zlib.crc32(data), len(data) & 0xFFFFFFFF)


def raw_deflate(data, level=6, mem_level=8, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, mem_level, strategy)
    return c.compress(data) + c.flush()


def gunzip(gz):
    """every member, as gzread reads them; bytes behind the last member that are no member are ignored"""
    out = b""
    while gz[:2] == b"\x1f\x8b":
        d = zlib.decompressobj(31)
        out += d.decompress(gz)
        if not d.eof:
            raise zlib.error("the member is cut short")
        gz = d.unused_data
    return out


@functools.lru_cache(maxsize=None)
def fixture_a():
    return member(fastq_text(600, 1), mem_level=3)


@functools.lru_cache(maxsize=None)
def fixture_b():
    return member(fastq_text(300, 2))


def decoy():
    """A block start inside a stored block: a full-flushed dynamic part, stored blocks whose data are the bytes of a memLevel-3 deflate
    stream of other text (true block headers, where no block of THIS stream starts), and a final part.  Sub-chunks of 1,024 bytes
    begin inside the stored data and find those starts; the chain steps over them."""
    t1, other, t3 = fastq_text(120, 11), fastq_text(150, 12), fastq_text(120, 13)
    inner = raw_deflate(other, mem_level=3)
    c = zlib.compressobj(6, zlib.DEFLATED, -15, 3)
    part1 = c.compress(t1) + c.flush(zlib.Z_FULL_FLUSH)  # ends byte-aligned, history forgotten: the final part reaches back no further
    stored = b""
    for i in range(0, len(inner), 60000):
        piece = inner[i:i + 60000]
        stored += b"\x00" + struct.pack("<HH", len(piece), len(piece) ^ 0xFFFF) + piece
    part3 = c.compress(t3) + c.flush()
    data = t1 + inner + t3
    gz = wrap(part1 + stored + part3, data)
    assert gunzip(gz) == data
    return gz


def binary(n=60000, seed=9):
    rng = random.Random(seed)
    return member(bytes(rng.randrange(256) if rng.randrange(7) else 0 for _ in range(n)))


@functools.lru_cache(maxsize=None)
def valid_cases():
    a, b = fixture_a(), fixture_b()
    text = fastq_text(400, 3)
    m1, m2, m3 = member(fastq_text(100, 4), mem_level=3), member(fastq_text(120, 5), mem_level=3), member(fastq_text(50, 6), 9, 3)
    run = fastq_text(50, 7) + b"A" * 100000 + fastq_text(200, 8)
    cases = [("A", a, 1024, 16, BIG), ("B", b, 4096, 16, BIG)]
    for sub in (512, 1024, 4096, 65536):
        cases += [("A-sub%d" % sub, a, sub, 16, BIG), ("B-sub%d" % sub, b, sub, 16, BIG)]
    cases += [
        ("A-five-super-chunks", a, 1024, 16, len(a) // 5 + 1024),
        ("level1", member(text, 1, 3), 1024, 16, BIG), ("level9", member(text, 9, 3), 1024, 16, BIG),
        ("fixed", member(text, 6, 3, zlib.Z_FIXED), 1024, 16, BIG), ("huffman-only", member(text, 6, 3, zlib.Z_HUFFMAN_ONLY), 1024, 16, BIG),
        ("rle", member(text, 6, 3, zlib.Z_RLE), 1024, 16, BIG), ("level0", member(text, 0), 1024, 16, BIG),
        ("sync-flush", member(text, 6, 3, flush_at=len(text) // 2), 1024, 16, BIG),
        ("full-flush", member(text, 6, 3, flush_at=len(text) // 2, flush=zlib.Z_FULL_FLUSH), 1024, 16, BIG),
        ("two-members", m1 + m2, 1024, 16, BIG), ("three-members", m1 + m2 + m3, 1024, 16, BIG),
        ("member-ends-at-the-super-chunk-end", m1 + m2 + m3, 1024, 16, len(m1)),
        ("trailer-across-super-chunks", m1 + m2 + m3, 512, 16, len(m1) - 5),
        ("junk-behind-the-last-member", m1 + m2 + bytes(range(100)), 1024, 16, BIG),
        ("header-fields", wrap(raw_deflate(text, mem_level=3), text, 4 | 8 | 16 | 2), 1024, 16, BIG),
        ("header-fname", wrap(raw_deflate(text, mem_level=3), text, 8), 1024, 16, BIG),
        ("run-of-As-ratio4", member(run, mem_level=3), 1024, 4, BIG),
        ("decoy-in-a-stored-block", decoy(), 1024, 16, BIG),
        ("binary", binary(), 1024, 16, 8192),
    ]
    return tuple(cases)


def damaged_cases():
    """(name, bytes): truncations of every class (inside the header, the first block, the stream, the last block, the trailer),
    flipped bytes through the stream, a wrong CRC, a wrong ISIZE.  zlib refuses most; a flip may leave the text unchanged."""
    b = fixture_b()
    out = [("cut-%d" % n, b[:n]) for n in list(range(0, 40, 3)) + list(range(40, len(b) - 8, 4099)) + list(range(len(b) - 12, len(b)))]
    for pos in range(10, len(b), 1777):
        f = bytearray(b)
        f[pos] ^= 0x10
        out.append(("flip-%d" % pos, bytes(f)))
    return out


def wrong_trailer():
    b = bytearray(fixture_b())
    crc, isize = bytearray(b), bytearray(b)
    crc[-6] ^= 1
    isize[-2] ^= 1
    return bytes(crc), bytes(isize), len(b) - 8


# ---- hand-assembled streams: the seams of the symbolic decoder, each with the smallest input that reaches it ----------------------
_LEN_BASE = [3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258]
_LEN_EXT = [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0]
_DIST_BASE = [1, 2, 3, 4, 5, 7, 9, 13, 17, 25, 33, 49, 65, 97, 129, 193, 257, 385, 513, 769, 1025, 1537, 2049, 3073, 4097, 6145, 8193, 12289, 16385, 24577]
_DIST_EXT = [0, 0, 0, 0, 1, 1, 2, 2, 3, 3, 4, 4, 5, 5, 6, 6, 7, 7, 8, 8, 9, 9, 10, 10, 11, 11, 12, 12, 13, 13]


class BitWriter:
    """a raw deflate stream written block by block: stored blocks and fixed-Huffman blocks of given tokens"""

    def __init__(self):
        self.acc, self.n, self.out = 0, 0, bytearray()

    def put(self, v, nbits):
        self.acc |= v << self.n
        self.n += nbits
        while self.n >= 8:
            self.out.append(self.acc & 0xFF)
            self.acc >>= 8
            self.n -= 8

    def code(self, c, nbits):  # Huffman codes go most significant bit first
        self.put(int(format(c, "0%db" % nbits)[::-1], 2), nbits)

    def symbol(self, s):
        if s < 144:
            self.code(0x30 + s, 8)
        elif s < 256:
            self.code(0x190 + s - 144, 9)
        elif s < 280:
            self.code(s - 256, 7)
        else:
            self.code(0xC0 + s - 280, 8)

    def stored(self, data, final=False):
        assert len(data) < 65536
        self.put(1 if final else 0, 1)
        self.put(0, 2)
        if self.n:
            self.put(0, 8 - self.n)
        self.out += struct.pack("<HH", len(data), len(data) ^ 0xFFFF) + data

    def fixed(self, tokens, final=False):
        """tokens: a byte value, or (length, distance)"""
        self.put(1 if final else 0, 1)
        self.put(1, 2)
        for t in tokens:
            if isinstance(t, int):
                self.symbol(t)
                continue
            length, dist = t
            k = max(i for i in range(29) if _LEN_BASE[i] <= length and (i < 28 or length == 258))
            if length == 258:
                k = 28
            self.symbol(257 + k)
            self.put(length - _LEN_BASE[k], _LEN_EXT[k])
            d = max(i for i in range(30) if _DIST_BASE[i] <= dist)
            self.code(d, 5)
            self.put(dist - _DIST_BASE[d], _DIST_EXT[d])
        self.symbol(256)

    def raw(self, stream):  # a byte-aligned deflate stream made elsewhere, behind a byte boundary
        assert self.n == 0
        self.out += stream

    def done(self):
        if self.n:
            self.put(0, 8 - self.n)
        return bytes(self.out)


def _member_of(w):
    raw = w.done()
    data = zlib.decompress(raw, -15)  # (zlib accepts the hand-made stream, and says what it holds)
    return wrap(raw, data)


def _text(n, seed):
    return fastq_text(n // 300 + 2, seed)[:n]


@functools.lru_cache(maxsize=None)
def seam_cases():
    """Super-chunks cut between hand-made blocks: the first block is a stored one of 33,000 bytes (33,005 with its header), so with
    super-chunks of 33,006 bytes -- or of 40,000 over stretches of 33-37 KB -- the stretch behind it is sub-chunk 0 of the next
    super-chunk, with a full inherited window."""
    cases = []
    A = _text(33000, 21)

    def three(tokens_b, tokens_c=None):
        w = BitWriter()
        w.stored(A)
        w.fixed(tokens_b, final=tokens_c is None)
        if tokens_c is not None:
            w.fixed(tokens_c, final=True)
        return _member_of(w)

    cases.append(("seam-distance-32768-first", three([(10, 32768), 65, 67, (258, 32768), 10]), 32768, 16, 33006))
    cases.append(("seam-source-straddles-window-and-output", three([120, 121, (20, 5), (258, 7), (33, 32768), 10]), 32768, 16, 33006))
    cases.append(("seam-fewer-than-64-symbols", three([(5, 32768), 71, 71, (4, 1), 10]), 32768, 16, 33006))
    fill = list(_text(40000, 22))
    tail = [(258, 32768), (258, 32768), (100, 32767), (3, 1)] + list(_text(9000, 23))
    for n in (32767, 32768, 32769):  # the window behind the chunk: one inherited byte / all its own output / the same, one symbol dropped
        head = [(30, 32768), (258, 20000)]
        b = head + fill[: n - 288]
        cases.append(("seam-chunk-of-%d-symbols" % n, three(b, tail), 32768, 16, 40000))
    # a fixed block and a stored block in mid-chain, between dynamic blocks that sub-chunks of 1,024 bytes find
    t1, t3 = fastq_text(60, 24), fastq_text(60, 25)
    c1 = zlib.compressobj(6, zlib.DEFLATED, -15, 3)
    w = BitWriter()
    w.raw(c1.compress(t1) + c1.flush(zlib.Z_FULL_FLUSH))
    w.fixed(list(_text(700, 26)) + [(40, 300), (258, 1)])
    w.stored(_text(600, 27))
    c3 = zlib.compressobj(6, zlib.DEFLATED, -15, 3)
    w.raw(c3.compress(t3) + c3.flush())
    cases.append(("seam-fixed-and-stored-in-mid-chain", _member_of(w), 1024, 16, BIG))
    return tuple(cases)
