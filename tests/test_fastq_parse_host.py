"""The host side of FASTQ records found on the device (kr_batch_submit_fastq): the sequential reader opened at a record start
(kr_fastx_open_at) gives the tail of the records the whole file gives, byte for byte; the new entry points reject bad arguments
before they touch a device."""
import ctypes as C
import gzip
import json
import os

import pytest

from conftest import GOLDEN


def records(capi, path, offset=None):
    names, bases, offs = capi.read_fastx(path, offset=offset)
    return names, [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(names))]


def test_open_at_every_record_start_of_query_toy_gives_the_tail(capi):
    path = os.path.join(GOLDEN, "query_toy.fq")
    raw = open(path, "rb").read()
    names, seqs = records(capi, path)
    lines = raw.split(b"\n")
    starts, pos = [], 0
    for i, ln in enumerate(lines):
        if i % 4 == 0 and ln:
            starts.append(pos)
        pos += len(ln) + 1
    assert len(starts) == len(names) == 100
    for i, off in enumerate(starts + [len(raw)]):
        n2, s2 = records(capi, path, off)
        assert n2 == names[i:] and s2 == seqs[i:], i


@pytest.mark.parametrize("key", ["edge", "trunc"])
def test_open_at_every_record_start_of_the_kseq_edge_texts(capi, tmp_path, key):
    ks = json.load(open(os.path.join(GOLDEN, "kseq_ref.json")))
    text, want = ks[key + "_text"].encode("latin-1"), ks[key]
    path = tmp_path / (key + ".fx")
    path.write_bytes(text)
    names, seqs = records(capi, str(path))
    assert names == want["names"] and [s.decode() for s in seqs] == want["seqs"]
    for i, nm in enumerate(names):  # a record's marker byte: kseq looks for the next '>' / '@' from there
        off = 0 if i == 0 else min(text.index(b"\n" + m + nm.encode()) + 1 for m in (b">", b"@") if b"\n" + m + nm.encode() in text)
        n2, s2 = records(capi, str(path), off)
        assert n2 == names[i:] and s2 == seqs[i:], (key, i, off)
    assert records(capi, str(path), len(text)) == ([], [])


def test_open_at_refuses_gzip_and_offsets_past_the_end(capi, tmp_path):
    lib = capi.load()
    src = open(os.path.join(GOLDEN, "query_toy.fq"), "rb").read()
    gz = tmp_path / "q.fq.gz"
    gz.write_bytes(gzip.compress(src))
    h = C.c_void_p()
    assert lib.kr_fastx_open_at(os.fsencode(str(gz)), 0, C.byref(h)) == capi.KR_ERR_UNSUPPORTED
    plain = tmp_path / "q.fq"
    plain.write_bytes(src)
    assert lib.kr_fastx_open_at(os.fsencode(str(plain)), len(src) + 1, C.byref(h)) == capi.KR_ERR_ARG
    assert lib.kr_fastx_open_at(os.fsencode(str(tmp_path / "missing.fq")), 0, C.byref(h)) == capi.KR_ERR_IO


def test_new_entry_points_reject_null_arguments(capi):
    lib = capi.load()
    h = C.c_void_p()
    out = capi.KrFastqParse()
    assert C.sizeof(capi.KrFastqParse) == 64
    pos, ln = capi.u64p(), capi.u32p()
    buf = (C.c_uint8 * 16)()
    assert lib.kr_fastx_open_at(None, 0, C.byref(h)) == capi.KR_ERR_ARG
    assert lib.kr_fastx_open_at(b"x.fq", 0, None) == capi.KR_ERR_ARG
    assert lib.kr_stream_fastq_enable(None, 1 << 20) == capi.KR_ERR_ARG
    assert lib.kr_batch_submit_fastq(None, buf, 16, 0, 1, C.byref(out)) == capi.KR_ERR_ARG
    assert lib.kr_batch_submit_fastq(None, None, 16, 0, 1, None) == capi.KR_ERR_ARG
    assert lib.kr_batch_fastq_names(None, C.byref(pos), C.byref(ln)) == capi.KR_ERR_ARG
    assert lib.kr_debug_fastq_batch(None, None, None) == capi.KR_ERR_ARG



def test_cli_help_lists_gpu_parse():
    import subprocess
    from conftest import ROOT
    exe = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
    out = subprocess.run([exe, "dist", "--help"], capture_output=True).stdout.decode()
    assert "--gpu-parse" in out and "FASTQ records found on the GPU (identical output" in out, out


def test_fastq_chunk_cut_is_the_last_record_start_whose_plus_line_is_inside(capi):
    """kr_fastq_chunk_cut on prefixes of clean four-line records: the last record start s > 0 whose '+' line begins inside the
    prefix (its name and sequence lines are then complete, and a byte follows them), by the generator's own bookkeeping; quality
    lines that begin with '@' or '+' are no record starts.  0 when there is none, for no bytes, and when the last MiB has no newline."""
    import numpy as np
    rng = np.random.default_rng(20260119)
    qual = np.frombuffer(b"@+!#5?FIJ~", np.uint8)
    parts, starts, plus, pos = [], [], [], 0
    for i in range(3000):
        ln = int(rng.integers(1, 151))
        name = b"@r%d" % i + (b" lane %d/1" % int(rng.integers(0, 9)) if i % 3 == 0 else b"")
        seq = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, ln)].tobytes()
        q = bytearray(qual[rng.integers(2, len(qual), ln)].tobytes())
        if i % 5 == 1:
            q[0] = ord("@")
        if i % 5 == 3:
            q[0] = ord("+")
        rec = name + b"\n" + seq + b"\n+" + (name[1:] if i % 7 == 0 else b"") + b"\n" + bytes(q) + b"\n"
        starts.append(pos)
        plus.append(pos + len(name) + 1 + ln + 1)
        parts.append(rec)
        pos += len(rec)
    raw = b"".join(parts)
    assert len(raw) < (1 << 20) and all(raw[s] == 64 for s in starts) and all(raw[p] == 43 and raw[p - 1] == 10 for p in plus)
    starts, plus = np.array(starts), np.array(plus)

    def want(n):  # (plus is ascending: the records in front of the first '+' at or behind n)
        k = int(np.searchsorted(plus, n, side="left")) - 1
        return int(starts[k]) if k >= 1 else 0

    lib = capi.load()
    assert lib.kr_fastq_chunk_cut(None, 0) == 0 and lib.kr_fastq_chunk_cut(None, 4096) == 0
    ns = {0, 1, len(raw), len(raw) - 1} | set(range(int(starts[0]), int(starts[3]) + 2)) | set(range(int(starts[1500]) - 2, int(starts[1502]) + 2))
    ns |= {int(x) for x in rng.integers(0, len(raw) + 1, 400)}
    ns |= {int(p) + d for p in plus[rng.integers(0, len(plus), 60)] for d in (0, 1)}
    for n in sorted(ns):
        assert capi.fastq_chunk_cut(raw[:n]) == want(n), n
    assert want(0) == want(1) == 0 and want(int(plus[1])) == 0 and want(int(plus[1]) + 1) == int(starts[1])
    # longer than 1 MiB, no newline in the last MiB: no cut, whatever lies in front
    assert capi.fastq_chunk_cut(raw[:int(starts[2000])] + b"@long\n" + b"A" * ((1 << 20) + 7)) == 0
