"""kr_place_stream_parsed (kr_place.cpp, kr_host_place.inc, kr_dev_place_parsed.inc): reads given as raw FASTQ / FASTA bytes are
placed from what the record finders leave in HBM -- lengths from the offsets, ids gathered out of the chunk -- and give the bytes and
the placement records that kr_place_stream gives for the same reads from host arrays.

The reference of every test is `Placer.place(bases, offsets, names)` on a Placer of its own (the host-array entry point, which this
feature leaves as it was); nothing is compared with a tolerance.  Counters witness the path: a pass through the host back end or the
host formatter cannot stand in for the kernels (and where a test is about a host fallback, that fallback's counter must move).
"""
import ctypes as C
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

USER_OLD = "(G000735195:0.0276038,G000018865:0.0228997)N2640:0.160977"
USER_NEW = "(G000735195:0.03,NEWLEAF:0.02)N2640:0.160977"
# (tabular, placements wanted): device text for the first two, the host's last phase for the others
MODES = {"jplace": (0, False), "tabular": (1, False), "summary": (2, True), "jplace+records": (0, True)}
NAME_LENGTHS = (1, 15, 16, 17, 63, 64, 65, 300)


def tree_of(which):
    if which == "user":
        nwk = open(os.path.join(GOLDEN, "tree_toy.nwk")).read()
        assert USER_OLD in nwk
        return nwk.replace(USER_OLD, USER_NEW)
    return None


def cut(reads, r0, r1, shorten=True):
    """reads [r0, r1) as (bases, offsets, names); shorten: read i loses its last i % 37 bases, so that lengths differ"""
    bases, offs, names = reads
    seqs = [bases[int(offs[i]):int(offs[i + 1]) - (i % 37 if shorten else 0)] for i in range(r0, r1)]
    o = np.zeros(len(seqs) + 1, np.uint64)
    o[1:] = np.cumsum([len(s) for s in seqs])
    return np.concatenate(seqs), o, list(names[r0:r1])


def fastq(batch, comment=b""):
    b, o, names = batch
    out = []
    for i, nm in enumerate(names):
        s = b[int(o[i]):int(o[i + 1])].tobytes()
        out.append(b"@" + nm.encode() + comment + b"\n" + s + b"\n+\n" + b"F" * len(s) + b"\n")
    return out


def fasta(batch, comment=b"", width=0, eol=b"\n"):
    b, o, names = batch
    out = []
    for i, nm in enumerate(names):
        s = b[int(o[i]):int(o[i + 1])].tobytes()
        lines = [s[p:p + width] for p in range(0, len(s), width)] if width else [s]
        out.append(b">" + nm.encode() + comment + eol + eol.join(lines) + eol)
    return out


@pytest.fixture(scope="module")
def ctx(capi, synth, toy_index_dir, toy_genomes):
    class Ctx:
        pass

    c = Ctx()
    c.capi = capi
    c.hx = capi.HostIndex(toy_index_dir)
    c.reads = synth.sample_reads(toy_genomes, 2049, seed=37)
    c.genomes = toy_genomes
    return c


def placer(ctx, mode, tree="backbone", max_reads=4096, max_bases=1 << 20, **opts):
    return ctx.capi.Placer(ctx.hx, tree_of(tree), 0, tabular=MODES[mode][0], max_reads=max_reads, max_bases=max_bases, **opts)


def host_calls(ctx, mode, batches, tree="backbone", **opts):
    """[(text, records)] of Placer.place on each batch in turn, and the summary"""
    pl = placer(ctx, mode, tree, **opts)
    out = []
    for b in batches:
        text, p = pl.place(*b, want_placements=MODES[mode][1])
        out.append((text, p.tobytes()))
    summ = pl.summary() if MODES[mode][0] == 2 else ""
    pl.close()
    return out, summ


def counters(capi):
    return capi.place_counters(), capi.place_text_counters(), capi.place_path_counters()


def diff2(a, b):
    return (b[0] - a[0], b[1] - a[1])


@pytest.mark.parametrize("tree", ["backbone", "user"])
@pytest.mark.parametrize("mode", list(MODES))
def test_parity_with_host_arrays(ctx, mode, tree):
    """Two calls in a row on one Placer (the jplace separator state crosses them), reads of different lengths."""
    capi = ctx.capi
    batches = [cut(ctx.reads, 0, 400), cut(ctx.reads, 400, 700)]
    want, want_summary = host_calls(ctx, mode, batches, tree)
    assert all(len(t) + len(p) > 0 for t, p in want)
    pl = placer(ctx, mode, tree)
    for b, (wt, wp) in zip(batches, want):
        c0 = counters(capi)
        text, p, summ = pl.place_parsed(b"".join(fastq(b, b" 1:N:0 extra")), want_placements=MODES[mode][1])
        c1 = counters(capi)
        assert summ["nreads"] == len(b[2]) and summ["status"] == capi.KR_FASTQ_OK
        assert text == wt and p.tobytes() == wp
        assert diff2(c0[0], c1[0]) == (1, 0), "the batch left the device"
        assert diff2(c0[1], c1[1]) == ((1, 0) if not MODES[mode][1] else (0, 0)), "the rows were not the device's"
    if mode == "jplace":
        assert not want[0][0].startswith(",\n") and want[1][0].startswith(",\n")
    assert (pl.summary() if MODES[mode][0] == 2 else "") == want_summary
    pl.close()


def boundary_names(n):
    """n names of the lengths in NAME_LENGTHS, mixed"""
    out = []
    for i in range(n):
        ln = NAME_LENGTHS[i % len(NAME_LENGTHS)]
        out.append("abcdefghij"[i % 10] if ln == 1 else ("q%d_" % i + "x" * ln)[:ln])
    return out


@pytest.mark.parametrize("n", [1, 2, 1023, 1024, 1025, 2049])
def test_ids_and_lengths_at_the_block_boundaries(ctx, tmp_path, n):
    """Read counts on both sides of the 256 x 4 reads of a block of the offset passes; names of 1 .. 300 bytes mixed, a comment behind
    each (the name ends at the first whitespace).  The ids the device laid out are the host reader's names, and the rows -- which
    carry the ids and depend on every read's length -- are those of the host-array call."""
    capi = ctx.capi
    b, o, _ = cut(ctx.reads, 0, n)
    names = boundary_names(n)
    raw = b"".join(fastq((b, o, names), b"\tlane=3 some comment"))
    q = tmp_path / "q.fq"
    q.write_bytes(raw)
    hn, hb, ho = capi.read_fastx(q)
    assert hn == names and sorted({len(x) for x in names}) == sorted(set(NAME_LENGTHS[:len(names)]))
    want, _ = host_calls(ctx, "tabular", [(hb, ho, hn)])
    pl = placer(ctx, "tabular")
    c0 = counters(capi)
    text, _, summ = pl.place_parsed(raw, want_placements=False)
    c1 = counters(capi)
    assert summ["nreads"] == n
    assert pl.st.place_ids() == [x.encode() for x in hn]
    assert text == want[0][0] and (n < 8 or len(text) > 0)
    assert diff2(c0[0], c1[0]) == (1, 0) and diff2(c0[1], c1[1]) == (1, 0)
    pl.close()


def test_fasta_names_empty_first_middle_and_last(ctx, tmp_path):
    capi = ctx.capi
    n = 1025
    b, o, _ = cut(ctx.reads, 0, n)
    names = boundary_names(n)
    for i in (0, 512, n - 1):
        names[i] = ""
    recs = fasta((b, o, names), b" a comment")
    raw = b"".join(recs)
    assert recs[0].startswith(b"> a comment\n")
    q = tmp_path / "q.fa"
    q.write_bytes(raw)
    hn, hb, ho = capi.read_fastx(q)
    assert hn == names
    for mode in ("tabular", "jplace"):
        want, _ = host_calls(ctx, mode, [(hb, ho, hn)])
        pl = placer(ctx, mode)
        c0 = counters(capi)
        text, _, summ = pl.place_parsed(raw, fasta=True, want_placements=False)
        c1 = counters(capi)
        assert summ["nreads"] == n and summ["status"] == capi.KR_FASTQ_OK
        ids = pl.st.place_ids()
        assert ids == [x.encode() for x in hn] and ids[0] == ids[512] == ids[-1] == b""
        assert text == want[0][0] and len(text) > 0
        assert diff2(c0[0], c1[0]) == (1, 0) and diff2(c0[1], c1[1]) == (1, 0)
        pl.close()


@pytest.mark.parametrize("mode", ["jplace", "summary"])
def test_a_record_that_is_not_clean_ends_the_prefix(ctx, mode):
    """Record 300 of 601 has a quality line shorter than its sequence: the host reader takes it, the record finder stops in front of
    it (KR_FASTQ_NOT_CLEAN).  The call places the 300 accepted reads; the one read goes through kr_place_stream on the same stream;
    the submit from behind it takes the rest.  The three pieces are one host batch's output."""
    capi = ctx.capi
    whole = cut(ctx.reads, 0, 601)
    recs = fastq(whole)
    bad = recs[300].split(b"\n")
    bad[3] = bad[3][:-5]
    recs[300] = b"\n".join(bad)
    want, _ = host_calls(ctx, mode, [whole])  # (the summary's 512-read groups go by global read number: the CLI's test)
    pl = placer(ctx, mode)
    wp = MODES[mode][1]
    raw = b"".join(recs)
    t0, p0, s0 = pl.place_parsed(raw, want_placements=wp, at_eof=1)
    assert s0["nreads"] == 300 and s0["status"] == capi.KR_FASTQ_NOT_CLEAN and s0["consumed"] == len(b"".join(recs[:300]))
    t1, p1 = pl.place(*cut(ctx.reads, 300, 301), want_placements=wp)
    t2, p2, s2 = pl.place_parsed(raw[s0["consumed"] + len(recs[300]):], want_placements=wp)
    assert s2["nreads"] == 300 and s2["status"] == capi.KR_FASTQ_OK
    assert t0 + t1 + t2 == want[0][0]
    p1, p2 = p1.copy(), p2.copy()
    p1["read"] += 300
    p2["read"] += 301
    assert p0.tobytes() + p1.tobytes() + p2.tobytes() == want[0][1]
    pl.close()


@pytest.mark.parametrize("mode", ["jplace", "tabular"])
def test_max_reads_cuts_the_chunk(ctx, mode):
    """600 reads on a stream of 256: KR_FASTQ_CAPACITY twice, each call places exactly the accepted reads, the next submit starts at
    `consumed`; the concatenation is the text of one host batch."""
    capi = ctx.capi
    whole = cut(ctx.reads, 0, 600)
    raw = b"".join(fastq(whole))
    want, _ = host_calls(ctx, mode, [whole])
    pl = placer(ctx, mode, max_reads=256)
    pos, got, taken = 0, "", []
    while pos < len(raw):
        c0 = counters(capi)
        text, _, summ = pl.place_parsed(raw[pos:], want_placements=False)
        c1 = counters(capi)
        assert diff2(c0[0], c1[0]) == (1, 0) and diff2(c0[1], c1[1]) == (1, 0)
        assert pl.st.place_ids() == [x.encode() for x in whole[2][sum(taken):sum(taken) + summ["nreads"]]]
        got += text
        taken.append(summ["nreads"])
        pos += summ["consumed"]
        assert summ["status"] == (capi.KR_FASTQ_CAPACITY if sum(taken) < 600 else capi.KR_FASTQ_OK)
    assert taken == [256, 256, 88] and got == want[0][0]
    pl.close()


@pytest.mark.parametrize("mode", ["jplace", "summary"])
def test_fasta_with_a_long_contig_is_tiled_on_the_device(ctx, mode):
    """Wrapped CRLF FASTA, one record above KR_TILE_MIN_POS among short ones, KR_TAP_ACCS | KR_TILE_DEVICE: the caller's reads are
    placed (their lengths are the caller's offsets', not the tiles'), as the host-tiled Placer.place places them."""
    capi = ctx.capi
    b, o, names = cut(ctx.reads, 0, 60, shorten=False)
    g = list(ctx.genomes.values())[3]
    seqs = [b[int(o[i]):int(o[i + 1])] for i in range(60)]
    seqs.insert(30, np.ascontiguousarray(g[1000:4500]))
    names = names[:30] + ["contig_3"] + names[30:]
    oo = np.zeros(62, np.uint64)
    oo[1:] = np.cumsum([len(s) for s in seqs])
    batch = (np.concatenate(seqs), oo, names)
    want, want_summary = host_calls(ctx, mode, [batch], max_bases=1 << 20)
    raw = b"".join(fasta(batch, b" len=x", width=60, eol=b"\r\n"))
    pl = placer(ctx, mode)
    c0 = counters(capi)
    text, p, summ = pl.place_parsed(raw, fasta=True, flags=capi.KR_TILE_DEVICE, want_placements=MODES[mode][1])
    c1 = counters(capi)
    assert summ["nreads"] == 61 and pl.st.tile_layout(61)["nv"] > 0
    assert text == want[0][0] and p.tobytes() == want[0][1] and len(text) + len(p) > 0
    assert (pl.summary() if MODES[mode][0] == 2 else "") == want_summary
    assert diff2(c0[0], c1[0]) == (1, 0)
    if mode == "jplace":
        assert diff2(c0[1], c1[1]) == (1, 0) and '"contig_3"' in text
    pl.close()


def moved(c0, c1, keys=("reruns_cand", "reruns_keep", "given_up", "text_flag_1", "text_flag_2", "text_flag_8", "text_flag_16")):
    return {k: c1[2][k] - c0[2][k] for k in keys if c1[2][k] != c0[2][k]}


@pytest.mark.parametrize("mode", ["jplace", "tabular", "summary"])
def test_the_whole_batch_on_the_host_back_end(ctx, monkeypatch, mode):
    """KR_PLACE_HOST=1: kr_place_batch is fed the offsets copied back from the stream and the names cut out of the chunk."""
    capi = ctx.capi
    batch = cut(ctx.reads, 0, 500)
    want, want_summary = host_calls(ctx, mode, [batch])
    monkeypatch.setenv("KR_PLACE_HOST", "1")
    pl = placer(ctx, mode)
    c0 = counters(capi)
    text, p, _ = pl.place_parsed(b"".join(fastq(batch, b" c")), want_placements=MODES[mode][1])
    c1 = counters(capi)
    assert diff2(c0[0], c1[0]) == (0, 1) and diff2(c0[1], c1[1]) == (0, 0)
    assert text == want[0][0] and p.tobytes() == want[0][1]
    assert (pl.summary() if MODES[mode][0] == 2 else "") == want_summary
    pl.close()


@pytest.mark.parametrize("mode", ["jplace", "tabular"])
def test_the_hosts_last_phase_formats_with_names_from_the_chunk(ctx, monkeypatch, mode):
    """KR_PLACE_HOST_TEXT=1: the device's back end, emit_placements on the host."""
    capi = ctx.capi
    batch = cut(ctx.reads, 0, 500)
    want, _ = host_calls(ctx, mode, [batch])
    monkeypatch.setenv("KR_PLACE_HOST_TEXT", "1")
    pl = placer(ctx, mode)
    c0 = counters(capi)
    text, _, _ = pl.place_parsed(b"".join(fastq(batch, b" c")), want_placements=False)
    c1 = counters(capi)
    assert diff2(c0[0], c1[0]) == (1, 0) and diff2(c0[1], c1[1]) == (0, 0), "device text was not switched off"
    assert c1[2]["ranges"] - c0[2]["ranges"] == 1 and c1[2]["text_bytes"] == 0
    assert text == want[0][0] and len(text) > 0
    pl.close()


def test_a_text_cap_sends_the_range_to_the_host_formatter(ctx, monkeypatch):
    """KR_DEBUG_PLACE_CAPS t=: half the bytes the range writes -- flag 2, the range is formatted by the host from the chunk's names; the
    same Placer's next batch, knob removed, is the device's again (text_want_min), across the jplace separator."""
    capi = ctx.capi
    batches = [cut(ctx.reads, 0, 500), cut(ctx.reads, 500, 800)]
    want, _ = host_calls(ctx, "jplace", batches)
    raws = [b"".join(fastq(b)) for b in batches]
    probe = placer(ctx, "jplace")
    probe.place_parsed(raws[0], want_placements=False)
    nbytes = capi.place_path_counters()["text_bytes"]
    probe.close()
    assert nbytes >= len(want[0][0]) > 1000
    pl = placer(ctx, "jplace")
    monkeypatch.setenv("KR_DEBUG_PLACE_CAPS", "t=%d" % (nbytes // 2))
    c0 = counters(capi)
    t0, _, _ = pl.place_parsed(raws[0], want_placements=False)
    c1 = counters(capi)
    monkeypatch.delenv("KR_DEBUG_PLACE_CAPS")
    t1, _, _ = pl.place_parsed(raws[1], want_placements=False)
    c2 = counters(capi)
    assert moved(c0, c1) == {"text_flag_2": 1} and diff2(c0[1], c1[1]) == (0, 1) and diff2(c0[0], c1[0]) == (1, 0)
    assert moved(c1, c2) == {} and diff2(c1[1], c2[1]) == (1, 0) and diff2(c1[0], c2[0]) == (1, 0)
    assert (t0, t1) == (want[0][0], want[1][0]) and t1.startswith(",\n")
    pl.close()


@pytest.mark.parametrize("mode", ["jplace", "summary"])
def test_sticky_candidate_caps_end_at_the_host_back_end(ctx, monkeypatch, mode):
    """KR_DEBUG_PLACE_CAPS c=,sticky: half the candidate slots the batch asks for, on every attempt -- given up after two reruns, the
    whole batch goes to kr_place_batch with offsets and names from the stream and the chunk."""
    capi = ctx.capi
    batch = cut(ctx.reads, 0, 500)
    want, want_summary = host_calls(ctx, mode, [batch])
    raw = b"".join(fastq(batch))
    probe = placer(ctx, mode)
    probe.place_parsed(raw, want_placements=MODES[mode][1])
    asked = capi.place_path_counters()["cnt0"]
    probe.close()
    assert asked >= 256
    monkeypatch.setenv("KR_DEBUG_PLACE_CAPS", "c=%d,sticky" % (asked // 2))
    pl = placer(ctx, mode)
    c0 = counters(capi)
    text, p, _ = pl.place_parsed(raw, want_placements=MODES[mode][1])
    c1 = counters(capi)
    assert moved(c0, c1) == {"reruns_cand": 2, "given_up": 1}, moved(c0, c1)
    assert diff2(c0[0], c1[0]) == (0, 1)
    assert text == want[0][0] and p.tobytes() == want[0][1]
    assert (pl.summary() if MODES[mode][0] == 2 else "") == want_summary
    pl.close()


def test_state_errors_leave_the_stream_usable(ctx):
    capi = ctx.capi
    lib = capi.load()
    batch = cut(ctx.reads, 0, 200)
    raw = b"".join(fastq(batch))
    want, _ = host_calls(ctx, "tabular", [batch])
    pl = placer(ctx, "tabular")
    pl.st.fastq_enable(1 << 20)
    pl._fq_on = True

    def parsed_rc(raw_ptr):
        txt, ln = C.c_void_p(), C.c_uint64()
        rc = lib.kr_place_stream_parsed(pl.hx.h, pl.dx.h, pl.pt, pl.st.h, raw_ptr, C.byref(pl.popts), 1, C.byref(pl.prev), C.byref(txt), C.byref(ln), None, None)
        assert rc != 0 and not txt.value
        return rc

    keep = (C.c_uint8 * 16)()
    assert parsed_rc(keep) == capi.KR_ERR_STATE  # nothing submitted yet
    pl.st.submit(batch[0], batch[1], capi.KR_TAP_ACCS)
    assert parsed_rc(keep) == capi.KR_ERR_STATE and b"not kr_batch_submit_fastq" in lib.kr_last_error()
    summ = pl.st.submit_fastq(raw, 0)  # no KR_TAP_ACCS
    assert summ["nreads"] == 200
    assert parsed_rc(pl.st._pinned) == capi.KR_ERR_STATE and b"KR_TAP_ACCS" in lib.kr_last_error()
    summ = pl.st.submit_fastq(b"@half a record\nACGT", capi.KR_TAP_ACCS)
    assert summ["nreads"] == 0
    assert parsed_rc(pl.st._pinned) == capi.KR_ERR_STATE and b"no record" in lib.kr_last_error()
    assert lib.kr_place_stream_parsed(pl.hx.h, pl.dx.h, pl.pt, pl.st.h, None, C.byref(pl.popts), 1, C.byref(pl.prev), None, None, None, None) == capi.KR_ERR_ARG
    ids, off = (C.c_char * 16)(), (C.c_uint32 * 4)()
    assert lib.kr_debug_place_ids(pl.st.h, ids, off) == capi.KR_ERR_STATE
    text, _, _ = pl.place_parsed(raw, want_placements=False)
    assert text == want[0][0] and len(text) > 0
    assert pl.st.place_ids() == [x.encode() for x in batch[2]]
    pl.place(*batch, want_placements=False)  # (a call from host arrays: its ids are the host's staging, not the accessor's)
    assert lib.kr_debug_place_ids(pl.st.h, ids, off) == capi.KR_ERR_STATE
    pl.close()


def test_the_id_layout_is_forgotten_by_a_call_that_goes_to_the_host_back_end(ctx, monkeypatch):
    """kr_debug_place_ids after a parsed call with device text, then after a parsed call under KR_PLACE_HOST (which never reaches the
    device back end): KR_OK with the names, then KR_ERR_STATE -- not the earlier call's layout."""
    capi = ctx.capi
    lib = capi.load()
    batch = cut(ctx.reads, 0, 100)
    raw = b"".join(fastq(batch))
    pl = placer(ctx, "tabular")
    pl.place_parsed(raw, want_placements=False)
    assert pl.st.place_ids() == [x.encode() for x in batch[2]]
    monkeypatch.setenv("KR_PLACE_HOST", "1")
    pl.place_parsed(raw, want_placements=False)
    ids, off = (C.c_char * len(raw))(), (C.c_uint32 * 101)()
    assert lib.kr_debug_place_ids(pl.st.h, ids, off) == capi.KR_ERR_STATE
    pl.close()
