"""kr_fastq_pair_cut (no device) against a brute force written here: the largest n <= max_records such that both buffers hold 4n
complete lines, and the byte behind the 4n-th newline of each; b None: one interleaved buffer, the largest even n.  Only newlines
count -- a quality line that begins with '@', CRLF and a last line without '\\n' change nothing about how they are counted."""
import ctypes as C

import numpy as np
import pytest


def rec(name, seq, qual=None, eol=b"\n"):
    return b"@" + name + eol + seq + eol + b"+" + eol + (qual or b"I" * len(seq)) + eol


def brute(a, b, max_records):
    def ends(buf):  # the byte behind every 4th newline
        nl = [i + 1 for i, c in enumerate(buf) if c == 0x0A]
        return nl[3::4]
    ea = ends(a)
    if b is None:
        n = min(len(ea), max_records) & ~1
        return (ea[n - 1] if n else 0), 0, n
    eb = ends(b)
    n = min(len(ea), len(eb), max_records)
    return (ea[n - 1] if n else 0), (eb[n - 1] if n else 0), n


def check(capi, a, b, max_records=0xFFFFFFFF):
    got = capi.fastq_pair_cut(a, b, max_records)
    assert got == brute(a, b, max_records), (a[:80], None if b is None else b[:80], max_records)
    return got


def mates(n, la=150, lb=100, eol=b"\n"):
    rng = np.random.default_rng(n + la)
    seq = lambda k: bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), k))
    a = [rec(b"r%d/1" % i, seq(la + i % 7), eol=eol) for i in range(n)]
    b = [rec(b"r%d/2" % i, seq(lb + i % 5), eol=eol) for i in range(n)]
    return a, b


def test_empty_and_fewer_than_four_lines(capi):
    assert check(capi, b"", b"") == (0, 0, 0)
    assert check(capi, b"", None) == (0, 0, 0)
    r = rec(b"x", b"ACGT")
    for k in range(len(r)):  # every proper prefix of one record: no record
        assert check(capi, r[:k], r)[2] == 0
        assert check(capi, r, r[:k])[2] == 0
    assert check(capi, r, r) == (len(r), len(r), 1)
    assert check(capi, b"\n\n\n", b"\n\n\n\n") == (0, 0, 0)
    assert check(capi, b"\n\n\n\n", b"\n\n\n\n") == (4, 4, 1)


def test_mates_of_different_lengths_cut_differently(capi):
    a, b = mates(9)
    ca, cb, n = check(capi, b"".join(a), b"".join(b))
    assert n == 9 and ca == sum(map(len, a)) and cb == sum(map(len, b)) and ca != cb


def test_last_line_without_newline(capi):
    a, b = mates(5)
    A, B = b"".join(a), b"".join(b)
    assert check(capi, A[:-1], B)[2] == 4  # a's fifth record is not whole
    assert check(capi, A, B[:-1])[2] == 4
    ca, cb, n = check(capi, A[:-1], B[:-1])
    assert n == 4 and ca == sum(map(len, a[:4])) and cb == sum(map(len, b[:4]))
    assert check(capi, A + b"@cut\nACG", B + b"@cut\nACGT\n+\n")[2] == 5


def test_quality_line_that_begins_with_at(capi):
    a = [rec(b"q%d" % i, b"ACGTACGT", b"@@IIIIII") for i in range(4)]
    b = [rec(b"q%d" % i, b"ACGT", b"@+@+") for i in range(4)]
    ca, cb, n = check(capi, b"".join(a), b"".join(b))
    assert n == 4 and ca == sum(map(len, a)) and cb == sum(map(len, b))


def test_crlf(capi):
    a, b = mates(6, eol=b"\r\n")
    ca, cb, n = check(capi, b"".join(a), b"".join(b))
    assert n == 6 and ca == sum(map(len, a)) and cb == sum(map(len, b))
    a2, _ = mates(6)
    assert check(capi, b"".join(a2), b"".join(b))[2] == 6  # one side only


@pytest.mark.parametrize("na,nb", [(7, 7), (7, 3), (3, 7), (1, 7), (7, 1), (0, 7), (7, 0)])
def test_shorter_side_and_max_records_clamp(capi, na, nb):
    a, b = mates(7)
    A, B = b"".join(a[:na]), b"".join(b[:nb])
    for mx in (0, 1, 2, 3, 6, 7, 8, 0xFFFFFFFF):
        ca, cb, n = check(capi, A, B, mx)
        assert n == min(na, nb, mx) and ca == sum(map(len, a[:n])) and cb == sum(map(len, b[:n]))


@pytest.mark.parametrize("nrec", [0, 1, 2, 3, 5])
def test_interleaved(capi, nrec):
    a, b = mates(3)
    il = [x for p in zip(a, b) for x in p][:nrec]
    buf = b"".join(il)
    ca, cb, n = check(capi, buf, None)
    assert n == nrec & ~1 and cb == 0 and ca == sum(map(len, il[:n]))
    for mx in (0, 1, 2, 3, 4, 5):
        assert check(capi, buf, None, mx)[2] == min(nrec, mx) & ~1
    assert check(capi, buf + b"@cut\nAC", None)[2] == nrec & ~1
    assert check(capi, buf[:-1], None)[2] == max(nrec - 1, 0) & ~1


def test_random_buffers(capi):
    rng = np.random.default_rng(5)
    for _ in range(200):
        a = bytes(rng.choice(np.frombuffer(b"\n\n@+AC\r", np.uint8), int(rng.integers(0, 60))))
        b = bytes(rng.choice(np.frombuffer(b"\n\n@+AC\r", np.uint8), int(rng.integers(0, 60))))
        mx = int(rng.integers(0, 6))
        check(capi, a, b, mx)
        check(capi, a, None, mx)


def test_null_arguments(capi):
    lib = capi.load()
    ca, cb, n = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0)
    assert lib.kr_fastq_pair_cut(None, 0, b"", 0, 1, C.byref(ca), C.byref(cb), C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_fastq_pair_cut(b"", 0, b"", 0, 1, None, C.byref(cb), C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_fastq_pair_cut(b"", 0, b"", 0, 1, C.byref(ca), None, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_fastq_pair_cut(b"", 0, b"", 0, 1, C.byref(ca), C.byref(cb), None) == capi.KR_ERR_ARG
    assert lib.kr_fastq_pair_cut(b"", 0, None, 0, 1, C.byref(ca), None, C.byref(n)) == capi.KR_OK  # interleaved: no cut_b needed
