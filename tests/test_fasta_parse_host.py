"""The host side of FASTA records found on the device (kr_batch_submit_fasta): the entry point rejects null arguments before it
touches a device; kr_fasta_chunk_cut returns the last record start of a chunk and nothing else; and the sequential reader opened
at such a cut (kr_fastx_open_at) gives the tail of the records the whole file gives."""
import ctypes as C

import numpy as np

from fasta_fuzz import fuzz_fasta, records


def test_submit_fasta_rejects_null_arguments(capi):
    lib = capi.load()
    out = capi.KrFastqParse()
    buf = (C.c_uint8 * 16)()
    assert lib.kr_batch_submit_fasta(None, buf, 16, 0, 1, C.byref(out)) == capi.KR_ERR_ARG
    assert lib.kr_batch_submit_fasta(None, None, 16, 0, 1, None) == capi.KR_ERR_ARG
    assert b"kr_batch_submit_fasta" in lib.kr_last_error()
    assert "kr_batch_submit_fasta" in capi.EXPORTS and "kr_fasta_chunk_cut" in capi.EXPORTS


def test_chunk_cut_returns_the_last_record_start_only(capi):
    cut = capi.fasta_chunk_cut
    assert cut(b"") == 0 and cut(b">") == 0 and cut(b"A") == 0  # n of 0 and of 1
    assert capi.load().kr_fasta_chunk_cut(None, 0) == 0
    assert cut(b">a\nACGT\n") == 0                      # the start at position 0 is never returned
    assert cut(b">>\n") == 0 and cut(b"\n>") == 1
    assert cut(b">a\nAC>GT\nAC\n") == 0                 # a '>' mid-line is never returned
    assert cut(b">a x>y\nACGT\n>b\nAC>GT") == 12        # ... nor one behind the last start
    assert cut(b">a\r\nACGT\r\n>b\r\nAC") == 10         # a '>' behind "\r\n" is returned
    assert cut(b">a\nA\r>b\n") == 0                     # (a bare '\r' ends no line)
    assert cut(b">a\nA\n>b\nC\n>c\nG\n") == 10
    assert cut(b"ACGT\nACGT\n") == 0                    # no start at all
    assert cut(b">x\n>y\n") == 3
    raw = b">a\nACGT\n>b\nAC"
    assert [cut(raw[:n]) for n in range(len(raw) + 1)] == [0] * 9 + [8] * 5  # the cut needs its '>' inside the chunk


def test_open_at_every_cut_of_fuzzed_fasta_gives_the_tail(capi, tmp_path):
    checked = 0
    for seed in range(6):
        rng = np.random.default_rng(100 + seed)
        raw, starts = fuzz_fasta(rng, 60, 0.0)
        path = tmp_path / ("c%d.fa" % seed)
        path.write_bytes(raw)
        want = records(capi, str(path))
        assert len(want[0]) == len(starts)
        n, seen = len(raw), set()
        while n > 1:  # walk the cuts from the end of the file: every record start but the first
            c = capi.fasta_chunk_cut(raw[:n])
            if c == 0:
                break
            assert c in starts and c not in seen
            seen.add(c)
            i = starts.index(c)
            assert records(capi, str(path), c) == (want[0][i:], want[1][i:]), (seed, c)
            # (a chunk that ends inside the record's header or body still cuts there)
            nxt = starts[i + 1] if i + 1 < len(starts) else len(raw)
            assert capi.fasta_chunk_cut(raw[:min(nxt, c + 1 + int(rng.integers(0, 40)))]) == c
            n = c
            checked += 1
        assert seen == set(starts[1:])
    assert checked == 6 * 59
