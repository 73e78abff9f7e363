"""The host side of block-gzipped input inflated on the device (kr_batch_submit_bgzf), as far as no device is needed: the member
decoder's host instantiation (csrc/kr_inflate.h through kr_debug_bgzf_inflate_host) against zlib on good and damaged members, the
walk over members, the chunk cut inside a member, and the host reader opened at a position inside a member.  Every comparison is
byte equality with what zlib gives."""
import ctypes as C
import gzip
import os
import re
import struct
import zlib

import numpy as np
import pytest

import bgzf_cases as bc
from conftest import GOLDEN, ROOT

NEW = ["kr_stream_bgzf_enable", "kr_batch_submit_bgzf", "kr_debug_bgzf_inflate", "kr_debug_bgzf_inflate_host", "kr_debug_bgzf_ms",
       "kr_bgzf_member_size", "kr_bgzf_walk", "kr_bgzf_chunk_cut", "kr_fastx_open_at_bgzf"]


def test_the_symbols_are_declared_and_exported_and_reject_null_arguments(capi):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    declared = set(re.findall(r"KR_API\s+[\w\s\*]+?\b(kr_\w+)\s*\(", hdr))
    for sym in NEW:
        assert sym in declared and sym in capi.EXPORTS and hasattr(lib, sym), sym
    buf, n = (C.c_uint8 * 64)(), C.c_uint64(0)
    k, m, u = C.c_uint32(0), C.c_uint64(0), C.c_uint32(0)
    out, h, ms = capi.KrFastqParse(), C.c_void_p(), C.c_float(0)
    assert lib.kr_stream_bgzf_enable(None, 1 << 20) == capi.KR_ERR_ARG
    assert lib.kr_batch_submit_bgzf(None, buf, 64, 0, 0, None, 0, 0, 1, C.byref(out)) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_inflate(None, buf, 64, buf, 64, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_ms(None, C.byref(ms)) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_inflate_host(None, 64, buf, 64, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_inflate_host(buf, 64, None, 64, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_debug_bgzf_inflate_host(buf, 64, buf, 64, None) == capi.KR_ERR_ARG
    assert lib.kr_bgzf_member_size(None, 64) == 0
    assert lib.kr_bgzf_walk(None, 64, 1 << 20, C.byref(k), C.byref(m), C.byref(m)) == capi.KR_ERR_ARG
    assert lib.kr_bgzf_walk(buf, 64, 1 << 20, None, C.byref(m), C.byref(m)) == capi.KR_ERR_ARG
    assert lib.kr_bgzf_chunk_cut(None, 64, 0, 0, C.byref(m), C.byref(u)) == 0
    assert lib.kr_fastx_open_at_bgzf(None, 0, 0, C.byref(h)) == capi.KR_ERR_ARG
    assert lib.kr_fastx_open_at_bgzf(b"x.fq.gz", 0, 0, None) == capi.KR_ERR_ARG
    assert lib.kr_fastx_open_at_bgzf(b"/nonexistent/x.fq.gz", 0, 0, C.byref(h)) == capi.KR_ERR_IO


@pytest.mark.parametrize("name", sorted(bc.corpus()))
def test_the_host_decoder_gives_zlibs_bytes(capi, name):
    comp, want = bc.corpus()[name]
    assert capi.bgzf_inflate_host(comp) == want
    assert capi.bgzf_inflate_host(comp + bc.EOF_MEMBER + comp) == want + want


def rejected(capi, comp):
    """the error message when kr_debug_bgzf_inflate_host refuses comp with KR_ERR_FORMAT, None when it inflates"""
    try:
        capi.bgzf_inflate_host(comp, cap=1 << 17)
    except capi.KrError as e:
        assert e.code == capi.KR_ERR_FORMAT, e
        return str(e)
    return None


def zlib_accepts(payload, isize):
    d = zlib.decompressobj(-15)
    try:
        out = d.decompress(payload, isize + 1)
    except zlib.error:
        return None
    return out if d.eof and not d.unused_data and not d.unconsumed_tail and len(out) == isize else None


@pytest.mark.parametrize("which", ["dynamic", "fixed"])
def test_every_single_bit_flip_of_a_member(capi, which):
    """payload and trailer: each flip is KR_ERR_FORMAT -- where zlib still inflates the payload cleanly, as a CRC error; header:
    rejected, or the original bytes.  The decoder's verdict on every flipped payload is zlib's.  A few flips in each member spell
    the SAME bytes (zlib inflates them to the original text): those are accepted, as they must be."""
    dyn, fix, text = bc.small_members()
    m = dyn if which == "dynamic" else fix
    assert capi.bgzf_inflate_host(m) == text
    crc_errors = same = 0
    for bit in range(len(m) * 8):
        f = bytearray(m)
        f[bit >> 3] ^= 1 << (bit & 7)
        msg = rejected(capi, bytes(f))
        if bit < 18 * 8:
            assert msg is not None or capi.bgzf_inflate_host(bytes(f)) == text, bit
            continue
        z = zlib_accepts(bytes(f[18:-8]), len(text)) if bit < (len(m) - 8) * 8 else None
        if z == text:  # another spelling of the same bytes (a match at another distance inside a run): nothing is damaged, nothing
            assert msg is None and capi.bgzf_inflate_host(bytes(f)) == text, bit  # can tell -- zlib and the CRC accept it too
            same += 1
            continue
        assert msg is not None and "offset 0" in msg, bit
        if bit < (len(m) - 8) * 8:
            assert ("wrong CRC-32" in msg) == (z is not None), (bit, msg)
            crc_errors += z is not None
    assert crc_errors > 0 and same < crc_errors  # (flips inside a literal's code leave a well-formed stream)


def test_truncated_members_and_wrong_sizes_are_rejected(capi):
    dyn, fix, text = bc.small_members()
    for m in (dyn, fix):
        for n in range(1, len(m)):
            assert rejected(capi, m[:n]) is not None, n
            assert rejected(capi, m + m[:n]) is not None and "offset %d" % len(m) in rejected(capi, m + m[:n]), n
        for n in range(18, len(m) - 8):  # the payload cut short inside a whole member
            assert rejected(capi, bc.with_payload(m, m[18:n])) is not None, n
        assert "more output than ISIZE" in rejected(capi, bc.set_isize(m, len(text) - 1))
        assert "less output than ISIZE" in rejected(capi, bc.set_isize(m, len(text) + 1))
        assert "ISIZE above 65,536" in rejected(capi, bc.set_isize(m, 65537))
        assert "input left over" in rejected(capi, bc.with_payload(m, m[18:-8] + b"\x00"))
        big = m[:16] + struct.pack("<H", len(m) + 5 - 1) + m[18:]  # BSIZE larger than the buffer
        assert rejected(capi, big) is not None
        xl = m[:10] + struct.pack("<H", len(m)) + m[12:]  # XLEN larger than the member
        assert rejected(capi, xl) is not None
    for name, (comp, words) in bc.damaged().items():
        msg = rejected(capi, comp)
        assert msg is not None and words in msg and "offset 0" in msg, (name, msg)
        msg = rejected(capi, dyn + bc.EOF_MEMBER + comp + dyn)
        assert msg is not None and words in msg and "offset %d" % (len(dyn) + len(bc.EOF_MEMBER)) in msg, (name, msg)


def test_member_size_and_walk(capi):
    rng = np.random.default_rng(3)
    text = bc.fastq_text(rng, 900)
    comp, offs, ustart = bc.members(text, 20000)
    sizes = np.diff(offs + [len(comp)])
    for o, s in zip(offs, sizes):
        assert capi.bgzf_member_size(comp[o:]) == s and capi.bgzf_member_size(comp[o:o + 18]) == s
        assert capi.bgzf_member_size(comp[o:o + 17]) == 0 and capi.bgzf_member_size(comp[o + 1:]) == 0
    assert capi.bgzf_member_size(gzip.compress(b"ACGT")) == 0 and capi.bgzf_member_size(b"") == 0
    ends = ustart[1:] + [len(text)]
    for limit in (0, 1, 19999, 20000, 20001, 40000, 59999, len(text) - 1, len(text), 1 << 30):
        k = max(1, sum(1 for e in ends if e <= limit))
        while k < len(ends) and ends[k] == ends[k - 1]:
            k += 1  # (the empty EOF member costs nothing)
        want = (k, offs[k] if k < len(offs) else len(comp), ends[k - 1])
        assert capi.bgzf_walk(comp, limit) == want, limit
    # the walk ends at bytes that are no whole member: a cut member, an ordinary gzip member
    assert capi.bgzf_walk(comp[:offs[2] + 40], 1 << 30) == (2, offs[2], 40000)
    assert capi.bgzf_walk(comp[:offs[2]] + gzip.compress(b"ACGT"), 1 << 30) == (2, offs[2], 40000)
    assert capi.bgzf_walk(comp[:17], 1 << 30) == (0, 0, 0) and capi.bgzf_walk(b"", 1 << 30) == (0, 0, 0)


def record_starts(text, fasta=False):
    marker = b">" if fasta else b"@"
    lines, starts, pos = text.split(b"\n"), [], 0
    for i, ln in enumerate(lines):
        if (ln.startswith(marker) if fasta else (i % 4 == 0 and ln != b"")):
            starts.append(pos)
        pos += len(ln) + 1
    return starts


def check_cut(capi, text, upto, skip, fasta, block=20000):
    """the members that hold text[:upto] (whole members: the chunk ends where the last one does) cut behind `skip`: the raw-bytes
    cut of the same chunk, as (member, byte inside it)"""
    comp, offs, ustart = bc.members(text[:upto], block, eof=False)
    chunk = text[skip:upto]
    want = capi.fasta_chunk_cut(chunk) if fasta else capi.fastq_chunk_cut(chunk)
    cut, moff, uoff = capi.bgzf_chunk_cut(comp, skip, fasta)
    assert cut == want
    if want:
        k = (want + skip) // block
        assert (moff, uoff) == (offs[k], (want + skip) % block)
    else:
        assert (moff, uoff) == (len(comp), 0)
    return cut


def test_chunk_cut_inside_members(capi):
    rng = np.random.default_rng(11)
    text = bc.fastq_text(rng, 2000, 150)
    assert len(text) > 200000
    starts = record_starts(text)
    # the cut in the last member, in the second last (the last member lies inside one record's tail), at a member boundary
    assert check_cut(capi, text, 110000, 0, False) // 20000 == 5
    assert check_cut(capi, text, 110000, 777, False) > 0
    k = next(i for i, s in enumerate(starts) if s > 100000)
    cut = check_cut(capi, text, starts[k] + 3, 0, False)  # three bytes of a name in the last member: the cut is the record in front
    assert cut == starts[k - 1] and cut < 100000
    pad = 100000 - starts[k - 1]  # a record start moved onto the boundary of two members: a longer name in front of it
    t2 = text[:starts[k - 2] + 1] + b"x" * pad + text[starts[k - 2] + 1:]
    s2 = record_starts(t2)
    assert 100000 in s2
    assert check_cut(capi, t2, 100000 + 60, 0, False) in (100000, s2[s2.index(100000) - 1])
    assert check_cut(capi, t2, 100000 + 400, 0, False) >= 100000
    # quality lines that begin with '@' are no record starts
    recs = []
    for i in range(600):
        ln = int(rng.integers(40, 120))
        recs.append(b"@q%d\n%s\n+\n@%s\n" % (i, b"ACGT"[i % 4:i % 4 + 1] * ln, b"I" * (ln - 1)))
    tq = b"".join(recs)
    for upto in (len(tq), len(tq) - 3, len(tq) - 130, 41000):
        cut = check_cut(capi, tq, upto, 0, False, block=5000)
        assert cut in record_starts(tq)
    # FASTA
    fa = b"".join(b">c%d some words\n%s\n" % (i, b"\n".join(b"ACGTTGCAAC"[:int(rng.integers(1, 11))] * 6 for _ in range(int(rng.integers(1, 30))))) for i in range(400))
    fs = record_starts(fa, True)
    for upto in (len(fa), fs[-1] + 1, fs[-1], 50000):
        cut = check_cut(capi, fa, upto, 123, True, block=7000)
        assert cut + 123 in fs
    # no cut within 1 MiB: one record longer than that
    long = b"@long\n" + b"A" * ((1 << 20) + 70000)
    comp, _, _ = bc.members(text[:starts[50]] + long, 60000, level=1, eof=False)
    assert capi.bgzf_chunk_cut(comp, 0, False) == (0, len(comp), 0)
    assert capi.bgzf_chunk_cut(bc.EOF_MEMBER, 0, False) == (0, len(bc.EOF_MEMBER), 0)


def records(capi, path, bgzf_at=None):
    names, bases, offs = capi.read_fastx(path, bgzf_at=bgzf_at)
    return names, [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(names))]


def test_open_at_bgzf_at_every_record_start_of_query_toy_gives_the_tail(capi, tmp_path):
    raw = open(os.path.join(GOLDEN, "query_toy.fq"), "rb").read()
    names, seqs = records(capi, os.path.join(GOLDEN, "query_toy.fq"))
    starts = record_starts(raw)
    assert len(starts) == len(names) == 100
    block = starts[40]  # a record start on a member boundary
    comp, offs, ustart = bc.members(raw, block)
    assert len(offs) >= 3 and ustart[1] == starts[40]
    path = tmp_path / "q.fq.gz"
    path.write_bytes(comp)
    assert records(capi, str(path)) == (names, seqs)
    for i, s in enumerate(starts + [len(raw)]):
        k = min(s // block, len(offs) - 2)  # (the end of the data: also as the last byte of the last data member, below)
        assert records(capi, str(path), (offs[k], s - ustart[k])) == (names[i:], seqs[i:]), i
    assert records(capi, str(path), (offs[1], 0)) == (names[40:], seqs[40:])
    assert records(capi, str(path), (offs[0], block - 1))[0] == names[40:]  # (the '\n' in front of a record start is no record)
    assert records(capi, str(path), (offs[-1], 0)) == ([], [])  # the empty EOF member
    assert records(capi, str(path), (len(comp), 0)) == ([], [])  # the end of the file
    h = C.c_void_p()
    lib = capi.load()
    assert lib.kr_fastx_open_at_bgzf(os.fsencode(str(path)), len(comp) + 1, 0, C.byref(h)) == capi.KR_ERR_ARG
    assert lib.kr_fastx_open_at_bgzf(os.fsencode(str(path)), offs[-1], 5, C.byref(h)) == capi.KR_ERR_FORMAT  # more than the member holds
    # an ordinary gzip member appended: the tail from inside the block-gzipped part runs through it, and it can be the start
    extra = b"@tail1\nACGTACGTAC\n+\nIIIIIIIIII\n@tail2\nGGGTTTAAAC\n+\nIIIIIIIIII\n"
    both = tmp_path / "both.fq.gz"
    both.write_bytes(comp + gzip.compress(extra))
    want_n, want_s = names + ["tail1", "tail2"], seqs + [b"ACGTACGTAC", b"GGGTTTAAAC"]
    assert records(capi, str(both)) == (want_n, want_s)
    assert records(capi, str(both), (offs[1], starts[70] - ustart[1])) == (want_n[70:], want_s[70:])
    assert records(capi, str(both), (len(comp), 0)) == (["tail1", "tail2"], want_s[100:])


def test_cli_help_says_that_bgzf_files_are_inflated_on_the_gpu():
    import subprocess
    exe = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
    for sub in ("dist", "place", "seek"):
        out = subprocess.run([exe, sub, "--help"], capture_output=True).stdout.decode()
        assert "--gpu-parse" in out and "BGZF files, inflated on the GPU" in out, out
