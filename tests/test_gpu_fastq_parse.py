"""FASTQ records found on the device (csrc/kr_dev_fastq.inc; kr_stream_fastq_enable / kr_batch_submit_fastq): the accepted prefix
of a chunk of raw bytes followed by the sequential reader opened where it ends (kr_fastx_open_at) gives exactly the records the
sequential reader gives for the whole file, under fuzzed corruptions; capacity and long-sequence stops land where they must; and a
batch submitted as raw bytes gives the rows and the device text of the same batch submitted parsed."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGTN", np.uint8)


@pytest.fixture(scope="module")
def toy(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    yield hx, dx
    dx.close()
    hx.close()


def records(capi, path, offset=None):
    names, bases, offs = capi.read_fastx(path, offset=offset)
    return names, [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(names))]


def fuzz_fastq(rng, n, p_bad):
    """n four-line records, each corrupted with probability p_bad; returns (bytes, record start offsets)"""
    out, starts, pos = [], [], 0
    for i in range(n):
        L = int(rng.integers(0, 90)) if rng.random() < 0.95 else 0
        seq = ACGT[rng.integers(0, 5, L)].tobytes()
        qual = bytes(rng.integers(33, 127, L).astype(np.uint8))
        name = b"r%d_%d" % (i, int(rng.integers(0, 1 << 30)))
        head, sep, nl = b"@" + name, b"+", b"\n"
        kind = rng.choice(["crlf", "wrap", "qshort", "qlong", "plusname", "ws", "marker", "qat", "empty", "high", "fasta"]) \
            if rng.random() < p_bad else None
        if kind == "crlf":
            nl = b"\r\n"
        elif kind == "wrap" and L >= 2:
            h = int(rng.integers(1, L))
            seq = seq[:h] + b"\n" + seq[h:]
        elif kind == "qshort" and L >= 1:
            qual = qual[:-1]
        elif kind == "qlong":
            qual = qual + b"I"
        elif kind == "plusname":
            sep = b"+" + name + b" x"
        elif kind == "ws":
            head += bytes([int(rng.choice([32, 9, 11, 12, 13]))]) + b"comment\tmore"
        elif kind == "marker" and L >= 1:
            j = int(rng.integers(0, L))
            seq = seq[:j] + bytes([int(rng.choice([64, 62, 43]))]) + seq[j + 1:]
        elif kind == "qat" and L >= 1:
            qual = b"@" + qual[1:]
        elif kind == "empty":
            seq, qual = b"", b""
        elif kind == "high" and L >= 1:
            j = int(rng.integers(0, L))
            if rng.random() < 0.5:
                seq = seq[:j] + bytes([int(rng.integers(128, 256))]) + seq[j + 1:]
            else:
                qual = qual[:j] + bytes([int(rng.integers(128, 256))]) + qual[j + 1:]
        if kind == "fasta":
            rec = b">" + name + b"\n" + seq + b"\n"
        else:
            rec = head + nl + seq + nl + sep + nl + qual + nl
        starts.append(pos)
        out.append(rec)
        pos += len(rec)
    raw = b"".join(out)
    if rng.random() < 0.3:
        raw = raw[:-1]  # no final newline
    return raw, starts


def device_then_host(capi, st, path, raw, starts, rng, max_chunk_recs=40):
    """The CLI's protocol: chunks cut at record starts, each submitted from where the previous one was accepted; the first
    chunk that ends early (other than at capacity) hands over to the sequential reader at that byte."""
    want = records(capi, path)
    got_n, got_s = [], []
    cuts = sorted(set(starts[1:]) | {len(raw)})
    pos, ci = 0, 0
    while pos < len(raw):
        while ci < len(cuts) and cuts[ci] <= pos:
            ci += 1
        end = cuts[min(len(cuts) - 1, ci + int(rng.integers(0, max_chunk_recs)))]
        s = st.submit_fastq(raw[pos:end], at_eof=int(end == len(raw)))
        assert s["rejected"] == s["nreads"] and s["consumed"] <= end - pos
        assert (s["status"] == capi.KR_FASTQ_OK) == (s["consumed"] == end - pos)
        names, seqs = st.fastq_names(), st.fastq_batch(s)
        assert len(names) == len(seqs) == s["nreads"]
        assert s["nbases"] == sum(len(x) for x in seqs)
        if s["nreads"]:
            st.wait()
        got_n += names
        got_s += seqs
        # `consumed` is a record boundary of the sequential parse: the reader opened there gives the rest
        assert records(capi, path, pos + s["consumed"]) == (want[0][len(got_n):], want[1][len(got_s):])
        pos += s["consumed"]
        if s["status"] == capi.KR_FASTQ_OK or (s["status"] == capi.KR_FASTQ_CAPACITY and s["nreads"]):
            continue
        break
    tail = records(capi, path, pos) if pos < len(raw) else ([], [])
    assert (got_n + tail[0], got_s + tail[1]) == want
    return len(got_n), len(want[0])


def test_record_parity_under_fuzzing(capi, toy, tmp_path):
    hx, dx = toy
    st = dx.stream(capi.default_params(), max_reads=512, max_bases=512 * 200)
    st.fastq_enable(1 << 20)
    dev_total = all_total = 0
    for seed in range(48):
        rng = np.random.default_rng(seed)
        raw, starts = fuzz_fastq(rng, 300, [0.0, 0.002, 0.01, 0.05][seed % 4])
        path = tmp_path / ("f%d.fq" % seed)
        path.write_bytes(raw)
        d, a = device_then_host(capi, st, str(path), raw, starts, rng)
        dev_total += d
        all_total += a
    assert dev_total > all_total // 3  # the clean files went through the device whole
    st.close()


@pytest.mark.parametrize("key", ["edge", "trunc"])
def test_kseq_edge_texts_through_the_device_path(capi, toy, tmp_path, key):
    hx, dx = toy
    ks = json.load(open(os.path.join(GOLDEN, "kseq_ref.json")))
    raw = ks[key + "_text"].encode("latin-1")
    path = tmp_path / (key + ".fx")
    path.write_bytes(raw)
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
    st.fastq_enable(1 << 16)
    for seed in range(4):
        rng = np.random.default_rng(seed)
        starts = [0] + [i + 1 for i in range(len(raw) - 1) if raw[i] == 10 and raw[i + 1] in (ord("@"), ord(">"))]
        device_then_host(capi, st, str(path), raw, starts, rng, max_chunk_recs=3)
    names, seqs = records(capi, str(path))
    assert names == ks[key]["names"] and [x.decode() for x in seqs] == ks[key]["seqs"]
    st.close()


def clean_fastq(lens, seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for i, L in enumerate(lens):
        s = ACGT[rng.integers(0, 4, L)].tobytes()
        out.append(b"@c%d desc\n%s\n+\n%s\n" % (i, s, b"I" * L))
    return b"".join(out)


def test_capacity_stops_at_record_boundaries_and_resubmits_cover_the_rest(capi, toy, tmp_path):
    hx, dx = toy
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.integers(30, 80, 150)]
    raw = clean_fastq(lens)
    path = tmp_path / "cap.fq"
    path.write_bytes(raw)
    want = records(capi, str(path))
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=64 * 100)
    st.fastq_enable(1 << 20)
    pos, got, counts = 0, [], []
    while pos < len(raw):
        s = st.submit_fastq(raw[pos:])
        counts.append((s["nreads"], s["status"]))
        got += st.fastq_batch(s)
        st.wait()
        assert records(capi, str(path), pos + s["consumed"])[1] == want[1][len(got):]
        pos += s["consumed"]
    assert counts == [(64, capi.KR_FASTQ_CAPACITY), (64, capi.KR_FASTQ_CAPACITY), (22, capi.KR_FASTQ_OK)]
    assert got == want[1]
    st.close()
    # bases: ten reads of 100 fill max_bases = 1000 exactly, the eleventh does not fit
    raw = clean_fastq([100] * 25, seed=1)
    st = dx.stream(capi.default_params(), max_reads=512, max_bases=1000)
    st.fastq_enable(1 << 16)
    s = st.submit_fastq(raw)
    assert (s["nreads"], s["status"], s["nbases"], s["rejected"]) == (10, capi.KR_FASTQ_CAPACITY, 1000, 10)
    assert s["consumed"] == raw.index(b"@c10 ")
    st.close()


def test_long_sequences_stop_exactly_at_the_tiling_threshold(capi, toy):
    hx, dx = toy
    k = hx.view.k
    ok_len, long_len = 1024 + k - 1, 1024 + k  # 1024 k-mer positions are not tiled, 1025 are (kTileMinPos)
    raw = clean_fastq([50, 60, ok_len, 70, long_len, 80], seed=2)
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=1 << 16)
    st.fastq_enable(1 << 16)
    s = st.submit_fastq(raw)
    assert (s["nreads"], s["status"]) == (4, capi.KR_FASTQ_LONG)
    assert [len(x) for x in st.fastq_batch(s)] == [50, 60, ok_len, 70]
    st.wait()
    s2 = st.submit_fastq(raw[s["consumed"]:])
    assert (s2["nreads"], s2["status"], s2["consumed"]) == (0, capi.KR_FASTQ_LONG, 0)
    st.close()


def test_stream_without_fastq_enable_and_oversized_chunks_are_refused(capi, toy):
    hx, dx = toy
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
    with pytest.raises(capi.KrError) as e:
        st.submit_fastq(b"@a\nACGT\n+\nIIII\n")
    assert e.value.code == capi.KR_ERR_STATE
    st.fastq_enable(64)
    with pytest.raises(capi.KrError) as e:
        st.submit_fastq(b"@a\nACGT\n+\nIIII\n" * 8)
    assert e.value.code == capi.KR_ERR_ARG
    with pytest.raises(capi.KrError) as e:
        st.fastq_enable(64)
    assert e.value.code == capi.KR_ERR_STATE
    st.close()


def fastq_bytes(bases, offs, names):
    out = []
    for i, nm in enumerate(names):
        s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
        out.append(b"@" + nm.encode() + b" some comment\n" + s + b"\n+\n" + b"F" * len(s) + b"\n")
    return b"".join(out)


@pytest.mark.parametrize("pkw", [dict(), dict(multi=0), dict(no_filter=0)])
def test_rows_and_text_equal_the_parsed_batch_on_the_toy_reads(capi, toy, pkw):
    hx, dx = toy
    names, bases, offs = capi.read_fastx(os.path.join(GOLDEN, "toy_reads.fq"))
    # the toy reads hold a few long sequences, which stay on the host path (LONG): the others, as a FASTQ file of their own
    lim = 1024 + hx.view.k - 1
    keep = [i for i in range(len(names)) if int(offs[i + 1] - offs[i]) <= lim]
    assert len(keep) > 250
    seqs = [bases[int(offs[i]):int(offs[i + 1])] for i in keep]
    names = [names[i] for i in keep]
    bases = np.concatenate(seqs)
    offs = np.zeros(len(keep) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in seqs])
    raw = fastq_bytes(bases, offs, names)
    n, nb = len(names), len(bases) + 64
    a = dx.stream(capi.default_params(**pkw), max_reads=n, max_bases=nb)
    a.text_enable(hx, 1 << 24, 1 << 20)
    a.fastq_enable(len(raw))
    s = a.submit_fastq(raw)
    assert (s["nreads"], s["status"], s["consumed"]) == (n, capi.KR_FASTQ_OK, len(raw))
    assert a.fastq_names() == names
    got = a.collect_text()
    b = dx.stream(capi.default_params(**pkw), max_reads=n, max_bases=nb)
    b.text_enable(hx, 1 << 24, 1 << 20)
    b.submit_text(bases, offs, names)
    assert got == b.collect_text() and len(got) > 0
    # rows without text: the same record sets and DIST values
    c = dx.stream(capi.default_params(**pkw), max_reads=n, max_bases=nb)
    c.fastq_enable(len(raw))
    c.submit_fastq(raw, capi.KR_ROWS_ONLY)
    rc = c.collect().rows()
    d = dx.stream(capi.default_params(**pkw), max_reads=n, max_bases=nb)
    d.submit(bases, offs, capi.KR_ROWS_ONLY)
    assert rc == d.collect().rows() and len(rc) > 0
    for x in (a, b, c, d):
        x.close()


def test_text_equals_the_parsed_batch_on_200000_synthetic_reads(capi, toy, toy_genomes, synth):
    hx, dx = toy
    bases, offs, names = synth.sample_reads(toy_genomes, 200000, seed=11)
    raw = fastq_bytes(bases, offs, names)
    a = dx.stream(capi.default_params(), max_reads=200000, max_bases=len(bases) + 64)
    a.text_enable(hx, 1 << 28, 1 << 23)
    a.fastq_enable(len(raw))
    s = a.submit_fastq(raw)
    assert (s["nreads"], s["status"], s["nbases"]) == (200000, capi.KR_FASTQ_OK, len(bases))
    got = a.collect_text()
    a.close()
    b = dx.stream(capi.default_params(), max_reads=200000, max_bases=len(bases) + 64)
    b.text_enable(hx, 1 << 28, 1 << 23)
    b.submit_text(bases, offs, names)
    want = b.collect_text()
    b.close()
    assert got == want and len(got) > 0
