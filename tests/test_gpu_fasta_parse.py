"""FASTA records found on the device (csrc/kr_dev_fasta.inc; kr_batch_submit_fasta): the accepted prefix of a chunk of raw bytes
followed by the sequential reader opened where it ends (kr_fastx_open_at) gives exactly the records the sequential reader gives
for the whole file, under fuzzed layouts and corruptions; the smallest inputs at which each byte-parallel pass can go wrong; the
stops land where they must; a batch submitted as raw bytes gives the rows and the device text of the same batch submitted parsed;
and FASTA and FASTQ chunks share a stream."""
import numpy as np
import pytest

from fasta_fuzz import fuzz_fasta, records, wrap_body

pytestmark = pytest.mark.gpu

ACGT = np.frombuffer(b"ACGT", np.uint8)


@pytest.fixture(scope="module")
def toy(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    yield hx, dx
    dx.close()
    hx.close()


def seq_of(n, seed):
    return ACGT[np.random.default_rng(seed).integers(0, 4, n)].tobytes()


def names_of(st):
    return [x.encode("latin-1") for x in st.fastq_names()]


def device_then_host(capi, st, path, raw, starts, rng, max_chunk_recs=40):
    """The CLI's protocol: chunks cut at record starts (closed=1), each submitted from where the previous one was accepted; one in
    five is cut inside a record instead (closed=0: its last record is left, and the next chunk starts there).  The first chunk
    that stops for another reason than capacity or such a cut hands over to the sequential reader at that byte.
    Returns (records through the device, records of the file, the whole file went through the device)."""
    want = records(capi, path)
    got_n, got_s = [], []
    cuts = sorted(set(starts[1:]) | {len(raw)})
    pos, ci, whole, force_closed = 0, 0, True, False
    while pos < len(raw):
        while ci < len(cuts) and cuts[ci] <= pos:
            ci += 1
        end = cuts[min(len(cuts) - 1, ci + int(rng.integers(0, max_chunk_recs)))]
        closed = 1
        if not force_closed and rng.integers(0, 5) == 0 and end > pos + 1:
            end, closed = pos + 1 + int(rng.integers(0, end - pos - 1)), 0
        if end == len(raw):
            closed = 1
        s = st.submit_fasta(raw[pos:end], closed=closed)
        assert s["rejected"] == s["nreads"] and s["consumed"] <= end - pos and s["at_eof"] == closed
        assert (s["status"] == capi.KR_FASTQ_OK) == (s["consumed"] == end - pos)
        assert s["newlines"] == raw[pos:end].count(b"\n")
        names, seqs = names_of(st), st.fastq_batch(s)
        assert len(names) == len(seqs) == s["nreads"]
        assert s["nbases"] == sum(len(x) for x in seqs)
        if s["nreads"]:
            st.wait()
        got_n += names
        got_s += seqs
        # `consumed` is a record boundary of the sequential parse: the reader opened there gives the rest
        assert records(capi, path, pos + s["consumed"]) == (want[0][len(got_n):], want[1][len(got_s):])
        pos += s["consumed"]
        force_closed = s["consumed"] == 0
        if s["status"] == capi.KR_FASTQ_OK or (s["status"] == capi.KR_FASTQ_CAPACITY and s["nreads"]):
            continue
        if s["status"] == capi.KR_FASTQ_INCOMPLETE and not closed:
            continue  # the caller cuts again from `consumed`
        whole = False
        break
    tail = records(capi, path, pos) if pos < len(raw) else ([], [])
    assert (got_n + tail[0], got_s + tail[1]) == want
    return len(got_n), len(want[0]), whole and len(got_n) == len(want[0])


def test_record_parity_under_fuzzing(capi, toy, tmp_path):
    hx, dx = toy
    st = dx.stream(capi.default_params(), max_reads=512, max_bases=1 << 17)
    st.fastq_enable(1 << 20)
    dev_total = all_total = 0
    for seed in range(48):
        rng = np.random.default_rng(seed)
        p_bad = [0.0, 0.002, 0.01, 0.05][seed % 4]
        raw, starts = fuzz_fasta(rng, 300, p_bad)
        path = tmp_path / ("f%d.fa" % seed)
        path.write_bytes(raw)
        d, a, whole = device_then_host(capi, st, str(path), raw, starts, rng)
        assert whole or p_bad > 0, seed  # an uncorrupted file goes through the device whole
        dev_total += d
        all_total += a
    # More than half of the records go through the device.  The files are seeded, so the share is one fixed number, not a draw: a
    # Python model of the grammar put in place of the device in device_then_host gives 7,486 of 14,443 records (52 %) for exactly these
    # 48 files, and a correct device gives the same.  (71 % was measured on files of 1 to 120 records; with the same probabilities
    # per record a file of 300 records meets its first corruption, which ends its device share, proportionally earlier: on average
    # the four probabilities give about 100, 75, 25 and 7 %.)
    assert 2 * dev_total > all_total
    st.close()


def check_whole(capi, st, tmp_path, raw, nrec, flags=0, names=True):
    """`raw` goes through the device whole and gives the reader's records"""
    path = tmp_path / "b.fa"
    path.write_bytes(raw)
    want = records(capi, str(path))
    assert len(want[0]) == nrec
    s = st.submit_fasta(raw, flags)
    assert (s["nreads"], s["status"], s["consumed"], s["rejected"]) == (nrec, capi.KR_FASTQ_OK, len(raw), nrec)
    assert s["newlines"] == raw.count(b"\n") and s["nbases"] == sum(len(x) for x in want[1])
    assert st.fastq_batch(s) == want[1]
    if names:
        assert names_of(st) == want[0]
    st.wait()
    return s


def test_boundary_shapes_of_the_tile_passes(capi, toy, tmp_path):
    hx, dx = toy
    td = capi.KR_TILE_DEVICE  # (some of these records are longer than KR_TILE_MIN_POS: never LONG with it)
    st = dx.stream(capi.default_params(), max_reads=2048, max_bases=1 << 18)
    st.fastq_enable(1 << 18)
    # a record start exactly at byte 4096 (the byte in front of it lies in another tile), and one at byte 16 t (... in another lane)
    first = b">a\n" + seq_of(4096 - 3 - 1, 1) + b"\n"
    assert len(first) == 4096
    check_whole(capi, st, tmp_path, first + b">b\nACGT\n", 2, td)
    first = b">a\n" + seq_of(16 * 7 - 3 - 1, 2) + b"\n"
    check_whole(capi, st, tmp_path, first + b">b\nACGT\n" + b">c" + b"\n" * 12 + b">d\nT", 4, td)
    # a header that straddles a tile boundary, and one longer than a tile
    pad = b">a\n" + seq_of(4080 - 4, 3) + b"\n"
    assert len(pad) == 4080
    check_whole(capi, st, tmp_path, pad + b">name_over_the_edge_of_a_tile some comment\nACGTACGT\n>c\nAC\n", 3, td)
    check_whole(capi, st, tmp_path, b">a\nAC\n>long " + b"c > + @ \xc3\xa9" * 500 + b"\nACGTAC\nGT\n>c\nA\n", 3, td)
    # three record starts inside one 16-byte group; two empty sequences
    check_whole(capi, st, tmp_path, b">a\nA\n>b\nC\n>c\nG\n", 3, td)
    check_whole(capi, st, tmp_path, b">x\n>y\n", 2, td)
    # one record of 10,000 bases on one line, and the same record wrapped at 60 with CRLF
    s10 = seq_of(10000, 4)
    st.close()
    st = dx.stream(capi.default_params(), max_reads=2048, max_bases=1 << 18)
    st.fastq_enable(1 << 18)
    check_whole(capi, st, tmp_path, b">one line\n" + s10 + b"\n", 1, td)
    check_whole(capi, st, tmp_path, b">wrapped\r\n" + wrap_body(s10, 60, b"\r\n"), 1, td)
    # 1,500 records: two blocks of the offset passes
    rng = np.random.default_rng(5)
    raw = b"".join(b">r%d c\n" % i + wrap_body(seq_of(int(rng.integers(0, 90)), 100 + i), int(rng.choice([0, 7, 60])), b"\n") for i in range(1500))
    check_whole(capi, st, tmp_path, raw, 1500, td)
    st.close()


def test_a_4_mb_record_between_short_ones(capi, toy, tmp_path):
    """More than 1,024 tiles (a second round of the tile scan), one record of 4 MB wrapped at 60 between short ones"""
    hx, dx = toy
    big = seq_of(4 << 20, 6)
    short = [b">s%d\n" % i + wrap_body(seq_of(150, 200 + i), 60, b"\n") for i in range(400)]
    raw = b"".join(short[:200]) + b">contig of four megabases\n" + wrap_body(big, 60, b"\n") + b"".join(short[200:])
    assert len(raw) > 4_300_000
    k = hx.view.k
    tiles = (len(big) - k + 1 + 127) // 128
    st = dx.stream(capi.default_params(), max_reads=tiles + 1024, max_bases=len(big) + tiles * k + (1 << 18))
    st.fastq_enable(len(raw))
    path = tmp_path / "big.fa"
    path.write_bytes(raw)
    want = records(capi, str(path))
    s = st.submit_fasta(raw, capi.KR_TILE_DEVICE)
    assert (s["nreads"], s["status"], s["consumed"]) == (401, capi.KR_FASTQ_OK, len(raw))
    got = st.fastq_batch(s)
    assert [len(x) for x in got] == [len(x) for x in want[1]] and got == want[1]
    st.wait()
    st.close()


def clean_fasta(lens, seed=0, wrap=60):
    return b"".join(b">c%d desc\n" % i + wrap_body(seq_of(L, seed * 1000 + i), wrap, b"\n") for i, L in enumerate(lens))


def test_capacity_stops_at_record_boundaries(capi, toy, tmp_path):
    hx, dx = toy
    rng = np.random.default_rng(5)
    lens = [int(x) for x in rng.integers(30, 80, 150)]
    raw = clean_fasta(lens, wrap=25)
    path = tmp_path / "cap.fa"
    path.write_bytes(raw)
    want = records(capi, str(path))
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=64 * 100)
    st.fastq_enable(1 << 20)
    pos, got, counts = 0, [], []
    while pos < len(raw):  # max_reads
        s = st.submit_fasta(raw[pos:])
        counts.append((s["nreads"], s["status"]))
        got += st.fastq_batch(s)
        st.wait()
        assert records(capi, str(path), pos + s["consumed"])[1] == want[1][len(got):]
        pos += s["consumed"]
    assert counts == [(64, capi.KR_FASTQ_CAPACITY), (64, capi.KR_FASTQ_CAPACITY), (22, capi.KR_FASTQ_OK)]
    assert got == want[1]
    st.close()
    # max_bases: ten records of 100 fill max_bases = 1000 exactly, the eleventh does not fit; then a record that never fits
    raw = clean_fasta([100] * 25, seed=1)
    st = dx.stream(capi.default_params(), max_reads=512, max_bases=1000)
    st.fastq_enable(1 << 16)
    s = st.submit_fasta(raw)
    assert (s["nreads"], s["status"], s["nbases"], s["rejected"]) == (10, capi.KR_FASTQ_CAPACITY, 1000, 10)
    assert s["consumed"] == raw.index(b">c10 ")
    st.wait()
    s = st.submit_fasta(clean_fasta([1001, 50], seed=2))
    assert (s["nreads"], s["status"], s["consumed"]) == (0, capi.KR_FASTQ_CAPACITY, 0)
    st.close()
    # the id buffer (a stream with text): names of 40 bytes, room for 100 bytes of ids
    raw = b"".join(b">" + (b"n%d" % i).ljust(40, b"x") + b"\nACGTACGT\n" for i in range(5))
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
    st.text_enable(hx, 1 << 16, 100)
    st.fastq_enable(1 << 16)
    s = st.submit_fasta(raw)
    assert (s["nreads"], s["status"], s["id_bytes"]) == (2, capi.KR_FASTQ_CAPACITY, 80)
    assert s["consumed"] == raw.index(b">n2")
    st.collect_text()
    st.close()


def test_long_closed_incomplete_and_not_clean_stops(capi, toy):
    hx, dx = toy
    k = hx.view.k
    ok_len, long_len = 1024 + k - 1, 1024 + k  # 1024 k-mer positions are not tiled, 1025 are (kTileMinPos)
    raw = clean_fasta([50, 60, ok_len, 70, long_len, 80], seed=2)
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=1 << 16)
    st.fastq_enable(1 << 16)
    s = st.submit_fasta(raw)
    assert (s["nreads"], s["status"], s["consumed"]) == (4, capi.KR_FASTQ_LONG, raw.index(b">c4 "))
    assert [len(x) for x in st.fastq_batch(s)] == [50, 60, ok_len, 70]
    st.wait()
    s = st.submit_fasta(raw[s["consumed"]:])
    assert (s["nreads"], s["status"], s["consumed"]) == (0, capi.KR_FASTQ_LONG, 0)
    s = st.submit_fasta(raw, capi.KR_TILE_DEVICE)  # never raised with KR_TILE_DEVICE
    assert (s["nreads"], s["status"], s["consumed"]) == (6, capi.KR_FASTQ_OK, len(raw))
    assert [len(x) for x in st.fastq_batch(s)] == [50, 60, ok_len, 70, long_len, 80]
    st.wait()
    # closed = 0 leaves exactly the last record, with or without its final newline
    raw = clean_fasta([40, 50, 60], seed=3)
    for chunk in (raw, raw[:-1], raw[:-20]):
        s = st.submit_fasta(chunk, closed=0)
        assert (s["nreads"], s["status"], s["consumed"], s["at_eof"]) == (2, capi.KR_FASTQ_INCOMPLETE, raw.index(b">c2 "), 0)
        st.wait()
    s = st.submit_fasta(raw[:-1], closed=1)
    assert (s["nreads"], s["status"], s["consumed"]) == (3, capi.KR_FASTQ_OK, len(raw) - 1)
    assert [len(x) for x in st.fastq_batch(s)] == [40, 50, 60]
    st.wait()
    # a header without '\n' is INCOMPLETE, closed or not
    for closed in (0, 1):
        s = st.submit_fasta(b">a\nACGT\n>b no newline", closed=closed)
        assert (s["nreads"], s["status"], s["consumed"]) == (1, capi.KR_FASTQ_INCOMPLETE, 8)
        st.wait()
    s = st.submit_fasta(b">only a header")
    assert (s["nreads"], s["status"], s["consumed"]) == (0, capi.KR_FASTQ_INCOMPLETE, 0)
    # a first byte other than '>' is NOT_CLEAN with nreads 0
    for chunk in (b"ACGT\n>a\nACGT\n", b"\n>a\nACGT\n", b"@a\nACGT\n+\nIIII\n", b"x"):
        s = st.submit_fasta(chunk)
        assert (s["nreads"], s["status"], s["consumed"]) == (0, capi.KR_FASTQ_NOT_CLEAN, 0), chunk
    # every kind of unclean body stops at its record; a NUL in the name too; the same bytes in a header do not
    for bad in (b"AC+GT", b"AC@GT", b"AC>GT", b"AC\xffGT", b"AC\x80GT", b"+", b"@x\nAC"):
        s = st.submit_fasta(b">a\nAC\n>b\n" + bad + b"\n>c\nAC\n")
        assert (s["nreads"], s["status"], s["consumed"]) == (1, capi.KR_FASTQ_NOT_CLEAN, 6), bad
        st.wait()
    s = st.submit_fasta(b">a\nAC\n>b\0c\nAC\n")
    assert (s["nreads"], s["status"], s["consumed"]) == (1, capi.KR_FASTQ_NOT_CLEAN, 6)
    st.wait()
    s = st.submit_fasta(b">a x\0 > + @ \xff\nAC\n>b\nAC")
    assert (s["nreads"], s["status"]) == (2, capi.KR_FASTQ_OK)
    assert names_of(st) == [b"a", b"b"] and st.fastq_batch(s) == [b"AC", b"AC"]
    st.wait()
    # nbytes == 0 is accepted
    s = st.submit_fasta(b"")
    assert (s["nreads"], s["status"], s["consumed"]) == (0, capi.KR_FASTQ_OK, 0)
    assert st.fastq_names() == []
    st.close()


def test_stream_without_enable_and_oversized_chunks_are_refused(capi, toy):
    hx, dx = toy
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
    with pytest.raises(capi.KrError) as e:
        st.submit_fasta(b">a\nACGT\n")
    assert e.value.code == capi.KR_ERR_STATE
    st.fastq_enable(64)
    with pytest.raises(capi.KrError) as e:
        st.submit_fasta(b">a\nACGT\n" * 9)
    assert e.value.code == capi.KR_ERR_ARG
    with pytest.raises(capi.KrError) as e:
        st.submit_fasta(b">a\nACGT\n", capi.KR_BASES_DEVICE)
    assert e.value.code == capi.KR_ERR_ARG
    # a chunk of 4 GB or more is refused before a byte of it is read (positions are 32-bit)
    import ctypes as C
    out, buf = capi.KrFastqParse(), (C.c_uint8 * 16)(*b">a\nACGT\n")
    for nbytes in (1 << 32, (1 << 32) + 5, 1 << 40):
        assert capi.load().kr_batch_submit_fasta(st.h, buf, nbytes, 0, 1, C.byref(out)) == capi.KR_ERR_ARG
        assert b"below 4 GB" in capi.load().kr_last_error()
    s = st.submit_fasta(b">a\nACGT\n")  # (the stream is as it was)
    assert (s["nreads"], s["status"]) == (1, capi.KR_FASTQ_OK)
    st.wait()
    st.close()


def test_parse_kernel_timer(capi, toy):
    """kr_debug_fastq_parse_ms: the first call makes the events and gives -1, every parse behind it is measured, FASTA and FASTQ"""
    import ctypes as C
    hx, dx = toy
    lib = capi.load()
    st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
    ms = C.c_float(0)
    assert lib.kr_debug_fastq_parse_ms(None, C.byref(ms)) == capi.KR_ERR_ARG
    assert lib.kr_debug_fastq_parse_ms(st.h, C.byref(ms)) == capi.KR_ERR_STATE
    st.fastq_enable(1 << 12)
    st.submit_fasta(b">a\nACGT\n")  # (not measured: nobody has asked yet)
    st.wait()
    assert lib.kr_debug_fastq_parse_ms(st.h, C.byref(ms)) == 0 and ms.value == -1.0
    assert lib.kr_debug_fastq_parse_ms(st.h, C.byref(ms)) == 0 and ms.value == -1.0
    for submit, raw in ((st.submit_fasta, b">a\nACGT\n>b\nAC\n"), (st.submit_fastq, b"@a\nACGT\n+\nIIII\n")):
        assert submit(raw)["nreads"] > 0
        st.wait()
        assert lib.kr_debug_fastq_parse_ms(st.h, C.byref(ms)) == 0 and 0.0 < ms.value < 1000.0
    st.close()


def toy_batch(capi, hx, synth, toy_genomes, with_contig):
    """(names, bases, offsets, FASTA bytes) of 300 short reads, with a sequence above KR_TILE_MIN_POS in the middle or without"""
    bases, offs, names = synth.sample_reads(toy_genomes, 300, seed=21)
    seqs = [bases[int(offs[i]):int(offs[i + 1])] for i in range(300)]
    names = list(names)
    if with_contig:
        seqs.insert(150, next(iter(toy_genomes.values()))[1000:7000])
        names.insert(150, "contig_of_6000")
    bases = np.concatenate(seqs)
    offs = np.zeros(len(seqs) + 1, np.uint64)
    offs[1:] = np.cumsum([len(x) for x in seqs])
    raw = b"".join(b">" + nm.encode() + b" some comment\r\n" + wrap_body(s.tobytes(), 60, b"\r\n") for nm, s in zip(names, seqs))
    return names, bases, offs, raw


def test_rows_and_text_equal_the_parsed_batch(capi, toy, synth, toy_genomes):
    hx, dx = toy
    names, bases, offs, raw = toy_batch(capi, hx, synth, toy_genomes, False)
    n, nb = len(names), len(bases) + 64
    a = dx.stream(capi.default_params(), max_reads=n, max_bases=nb)
    a.text_enable(hx, 1 << 24, 1 << 20)
    a.fastq_enable(len(raw))
    s = a.submit_fasta(raw)
    assert (s["nreads"], s["status"], s["consumed"]) == (n, capi.KR_FASTQ_OK, len(raw))
    assert a.fastq_names() == names
    got = a.collect_text()
    b = dx.stream(capi.default_params(), max_reads=n, max_bases=nb)
    b.text_enable(hx, 1 << 24, 1 << 20)
    b.submit_text(bases, offs, names)
    assert got == b.collect_text() and len(got) > 0
    c = dx.stream(capi.default_params(), max_reads=n, max_bases=nb)
    c.fastq_enable(len(raw))
    c.submit_fasta(raw, capi.KR_ROWS_ONLY)
    rc = c.collect().rows()
    d = dx.stream(capi.default_params(), max_reads=n, max_bases=nb)
    d.submit(bases, offs, capi.KR_ROWS_ONLY)
    assert rc == d.collect().rows() and len(rc) > 0
    for x in (a, b, c, d):
        x.close()


def test_rows_and_text_of_a_batch_with_a_long_sequence(capi, toy, synth, toy_genomes):
    hx, dx = toy
    names, bases, offs, raw = toy_batch(capi, hx, synth, toy_genomes, True)
    n, nb = len(names) + 256, 2 * len(bases) + 4096
    # KR_TILE_DEVICE | KR_TILE_ROWS: rows and device text of the tiled batch
    a = dx.stream(capi.default_params(), max_reads=n, max_bases=nb)
    a.text_enable(hx, 1 << 24, 1 << 20)
    a.fastq_enable(len(raw))
    s = a.submit_fasta(raw, capi.KR_TILE_DEVICE | capi.KR_TILE_ROWS)
    assert (s["nreads"], s["status"]) == (len(names), capi.KR_FASTQ_OK)
    assert a.tile_layout(len(names))["nlong"] == 1
    got = a.collect_text()
    b = dx.stream(capi.default_params(), max_reads=n, max_bases=nb)
    b.text_enable(hx, 1 << 24, 1 << 20)
    b.submit_text(bases, offs, names, capi.KR_TILE_ROWS)
    want = b.collect_text()
    assert got == want and b"contig_of_6000\t" in got
    c = dx.stream(capi.default_params(), max_reads=n, max_bases=nb)
    c.fastq_enable(len(raw))
    c.submit_fasta(raw, capi.KR_ROWS_ONLY | capi.KR_TILE_DEVICE | capi.KR_TILE_ROWS)
    rc = c.collect().rows()
    d = dx.stream(capi.default_params(), max_reads=n, max_bases=nb)
    d.submit(bases, offs, capi.KR_ROWS_ONLY | capi.KR_TILE_ROWS)
    assert rc == d.collect().rows() and len(rc) > 0
    # without KR_TILE_ROWS: no device text for the tiled batch; the host formatter with the names of kr_batch_fastq_names
    s = a.submit_fasta(raw, capi.KR_TILE_DEVICE)
    assert s["nreads"] == len(names)
    with pytest.raises(capi.KrError) as e:
        a.collect_text()
    assert e.value.code == capi.KR_ERR_UNSUPPORTED
    a.collect()
    assert a.format_dist(hx, a.fastq_names()).encode() == want
    for x in (a, b, c, d):
        x.close()


def test_fasta_and_fastq_chunks_share_a_stream(capi, toy):
    hx, dx = toy
    fa = clean_fasta([60, 0, 75, 90], seed=7, wrap=33)
    seqs = [seq_of(L, 900 + i) for i, L in enumerate([50, 70, 64])]
    fq = b"".join(b"@q%d x\n%s\n+\n%s\n" % (i, s, b"I" * len(s)) for i, s in enumerate(seqs))
    alone = {}
    for kind, raw in (("fa", fa), ("fq", fq)):
        st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
        st.fastq_enable(1 << 12)
        s = st.submit_fasta(raw) if kind == "fa" else st.submit_fastq(raw)
        alone[kind] = (s, st.fastq_names(), st.fastq_batch(s))
        st.wait()
        # the other format's call on these bytes: NOT_CLEAN at byte 0
        s = st.submit_fastq(raw) if kind == "fa" else st.submit_fasta(raw)
        assert (s["nreads"], s["status"], s["consumed"]) == (0, capi.KR_FASTQ_NOT_CLEAN, 0)
        st.close()
    assert alone["fa"][0]["nreads"] == 4 and alone["fq"][0]["nreads"] == 3 and alone["fq"][2] == seqs
    for order in (("fa", "fq", "fa"), ("fq", "fa", "fq")):
        st = dx.stream(capi.default_params(), max_reads=64, max_bases=4096)
        st.fastq_enable(1 << 12)
        for kind in order:
            s = st.submit_fasta(fa) if kind == "fa" else st.submit_fastq(fq)
            assert (s, st.fastq_names(), st.fastq_batch(s)) == alone[kind], order
            st.wait()
        st.close()
