"""kr_batch_submit_bgzf: a chunk given as whole BGZF members gives what kr_batch_submit_fastq / _fasta give for the same chunk's plain
bytes -- the summary, the bases and offsets, the names, the collected rows, the device text, tiles, placements and seek text --
whether the chunk starts and ends inside members or at their ends, with the inflated bytes copied back or not.  Nothing is compared
with a tolerance."""
import os

import numpy as np
import pytest

import bgzf_cases as bc
import seek_craft as sc
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

BLOCK = 20000


@pytest.fixture(scope="module")
def toy(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    yield hx, dx
    dx.close()
    hx.close()


def as_text(names, seqs, fasta):
    if fasta:
        return b"".join(b">%s c\n%s\n" % (n.encode(), b"\n".join(s[p:p + 70] for p in range(0, len(s), 70))) for n, s in zip(names, seqs))
    return b"".join(b"@%s c\n%s\n+\n%s\n" % (n.encode(), s, b"F" * len(s)) for n, s in zip(names, seqs))


@pytest.fixture(scope="module")
def texts(capi, synth, toy_genomes):
    """name -> (plain bytes, record starts): the toy reads (long sequences among them) and 3,000 synthetic reads, as FASTQ and FASTA"""
    out = {}
    n1, b1, o1 = capi.read_fastx(os.path.join(GOLDEN, "toy_reads.fq"))
    b2, o2, n2 = synth.sample_reads(toy_genomes, 3000, seed=5)
    for key, (names, b, o) in {"toy": (n1, b1, o1), "synth": (n2, b2, o2)}.items():
        seqs = [b[int(o[i]):int(o[i + 1])].tobytes() for i in range(len(names))]
        for fasta in (False, True):
            recs = [as_text([n], [s], fasta) for n, s in zip(names, seqs)]
            out[key, fasta] = (b"".join(recs), np.concatenate([[0], np.cumsum([len(r) for r in recs])]).tolist())
    return out


def chunk_of(text, a, b):
    """the whole members of `text` (members of BLOCK bytes) that hold text[a:b): (comp, skip)"""
    m0, m1 = a // BLOCK, -(-b // BLOCK)
    return b"".join(bc.member(text[i * BLOCK:(i + 1) * BLOCK], 1 + i % 9) for i in range(m0, max(m1, m0 + 1))), a - m0 * BLOCK


def stream(capi, hx, dx, text_on, nbytes=1 << 22, max_reads=4096, **pkw):
    st = dx.stream(capi.default_params(**pkw), max_reads=max_reads, max_bases=nbytes)
    if text_on:
        st.text_enable(hx, 1 << 24, 1 << 20)
    st.fastq_enable(nbytes)
    st.bgzf_enable(nbytes)
    return st


def outcome(st, summ, text_on, flags=0):
    got = {"summary": summ, "names": st.fastq_names(), "batch": st.fastq_batch(summ)}
    if summ["nreads"]:
        if text_on:
            got["text"] = st.collect_text()
        else:
            got["rows"] = st.collect().rows()
    return got


@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
@pytest.mark.parametrize("key", ["toy", "synth"])
def test_the_chunk_of_members_gives_what_its_plain_bytes_give(capi, toy, texts, key, fasta):
    hx, dx = toy
    text, starts = texts[key, fasta]
    assert len(text) > 2 * BLOCK
    mid = len(text) // 2 // BLOCK * BLOCK  # the chunk ends where a member does, inside a record
    inside = next(s for s in starts if s > BLOCK + 100)          # a record start inside the second member
    late = max(s for s in starts if s < len(text) - BLOCK // 2)  # ... and one inside the last but one or the last
    spans = [(0, len(text)), (0, late), (inside, len(text)), (inside, late), (inside, inside + 1500), (0, mid)]
    served = 0
    for text_on in (False, True):
        a, b = stream(capi, hx, dx, text_on), stream(capi, hx, dx, text_on)
        for lo, hi in spans:
            plain = text[lo:hi]
            closed = int(hi == len(text) or hi in starts)
            flags = 0 if text_on else capi.KR_ROWS_ONLY
            want = outcome(a, (a.submit_fasta if fasta else a.submit_fastq)(plain, flags, closed), text_on)
            comp, skip = chunk_of(text, lo, hi)
            for want_raw in (True, False):
                summ, raw = b.submit_bgzf(comp, skip, hi - lo, flags, fasta, closed, want_raw=want_raw)
                assert raw == (plain if want_raw else None)
                got = outcome(b, summ, text_on) if want_raw else {"summary": summ, "batch": b.fastq_batch(summ)}
                if summ["nreads"] and not want_raw:
                    b.wait()
                for k in got:
                    assert got[k] == want[k], (k, lo, hi, text_on, want_raw)
            served += want["summary"]["nreads"] > 0
        a.close(), b.close()
    assert served >= 8  # (a span of the toy reads that begins with a long sequence accepts nothing: the same on both sides)


@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
def test_long_sequences_are_tiled_on_the_device(capi, toy, texts, fasta):
    hx, dx = toy
    text, starts = texts["toy", fasta]
    flags = capi.KR_TILE_DEVICE | capi.KR_TILE_ROWS
    a, b = stream(capi, hx, dx, True), stream(capi, hx, dx, True)
    want_s = (a.submit_fasta if fasta else a.submit_fastq)(text, flags, 1)
    assert want_s["status"] == capi.KR_FASTQ_OK and want_s["nreads"] == len(starts) - 1
    want = a.collect_text()
    comp, skip = chunk_of(text, 0, len(text))
    summ, raw = b.submit_bgzf(comp, 0, len(text), flags, fasta, 1)
    assert summ == want_s and raw == text and b.collect_text() == want and len(want) > 0
    a.close(), b.close()


def test_capacity_then_a_resubmit_of_the_bytes_that_came_back(capi, toy, texts):
    hx, dx = toy
    text, starts = texts["synth", False]
    lo, hi = starts[10], starts[900]
    a, b = stream(capi, hx, dx, True, max_reads=256), stream(capi, hx, dx, True, max_reads=256)
    comp, skip = chunk_of(text, lo, hi)
    summ, raw = b.submit_bgzf(comp, skip, hi - lo, 0, False, 1)
    want = a.submit_fastq(text[lo:hi], 0, 1)
    assert summ == want and (summ["status"], summ["nreads"]) == (capi.KR_FASTQ_CAPACITY, 256) and raw == text[lo:hi]
    assert b.collect_text() == a.collect_text()
    pos = summ["consumed"]
    while pos < hi - lo:  # the bytes are on the host now: kr_batch_submit_fastq from raw_out + consumed
        s2, w2 = b.submit_fastq(raw[pos:], 0, 1), a.submit_fastq(text[lo + pos:hi], 0, 1)
        assert s2 == w2 and s2["nreads"] > 0 and b.fastq_names() == a.fastq_names() and b.collect_text() == a.collect_text()
        pos += s2["consumed"]
    assert pos == hi - lo
    a.close(), b.close()


@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
@pytest.mark.parametrize("mode", [0, 1], ids=["jplace", "tabular"])
def test_placements_of_a_chunk_of_members(capi, toy, texts, mode, fasta):
    hx, dx = toy
    text, starts = texts["synth", fasta]
    lo, hi = starts[40], starts[1200]
    comp, skip = chunk_of(text, lo, hi)
    pa = capi.Placer(hx, None, 0, tabular=mode, max_reads=4096, max_bases=1 << 20)
    pb = capi.Placer(hx, None, 0, tabular=mode, max_reads=4096, max_bases=1 << 20)
    wt, wp, ws = pa.place_parsed(text[lo:hi], fasta=fasta)
    gt, gp, gs = pb.place_parsed(comp, fasta=fasta, bgzf=(skip, hi - lo))
    assert gs == ws and ws["nreads"] == 1160 and gt == wt and gp.tobytes() == wp.tobytes() and len(wt) > 0
    pa.close(), pb.close()


@pytest.mark.parametrize("fasta", [False, True], ids=["fastq", "fasta"])
def test_seek_text_of_a_chunk_of_members(capi, tmp_path, fasta):
    g = [sc.random_dna(np.random.default_rng(21), 120000)]
    path = sc.write_sketch(capi, tmp_path, "s", g, sc.CFG_A)
    hx = capi.HostIndex(path, sketch=True)
    dx = hx.upload(0)
    rng = np.random.default_rng(12)
    reads = [sc.mutate(rng, g[0][p:p + 150], 0.02) for p in range(0, 60000, 150)]
    reads.insert(7, g[0][20000:21200])
    reads.insert(13, sc.revcomp(g[0][30000:70000]))
    names = ["r%d" % i for i in range(len(reads))]
    text = sc.fasta_of(names, reads) if fasta else sc.fastq_of(names, reads)
    assert len(text) > 3 * BLOCK
    lo = text.index(b"\n" + (b">" if fasta else b"@") + b"r5\n") + 1
    a, b = (dx.stream(params=capi.default_params(hdist_th=4), max_reads=4096, max_bases=1 << 20) for _ in range(2))
    for st in (a, b):
        st.seek_enable(1 << 22, 1 << 20)
        st.fastq_enable(1 << 20)
    b.bgzf_enable(1 << 20)
    flags = capi.KR_SEEK | capi.KR_TILE_DEVICE
    want_s = (a.submit_fasta if fasta else a.submit_fastq)(text[lo:], flags, 1)
    comp, skip = chunk_of(text, lo, len(text))
    summ, raw = b.submit_bgzf(comp, skip, len(text) - lo, flags, fasta, 1)
    assert summ == want_s and summ["nreads"] == len(reads) - 5 and raw == text[lo:]
    assert b.collect_text() == a.collect_text() and len(a.collect_text()) > 0
    a.close(), b.close(), dx.close(), hx.close()


def test_a_damaged_member_queues_nothing_and_the_next_submit_is_served(capi, toy, texts):
    hx, dx = toy
    text, starts = texts["synth", False]
    b = stream(capi, hx, dx, True)
    comp, _ = chunk_of(text, 0, 3 * BLOCK)
    first = capi.bgzf_member_size(comp)
    bad = bytearray(comp)
    bad[first + 200] ^= 0x10  # inside the second member's payload
    with pytest.raises(capi.KrError) as host:
        capi.bgzf_inflate_host(bytes(bad))
    with pytest.raises(capi.KrError) as e:
        b.submit_bgzf(bytes(bad), 0, 3 * BLOCK, 0, False, 0)
    assert e.value.code == capi.KR_ERR_FORMAT and "offset %d" % first in str(e.value) and str(e.value) == str(host.value)
    with pytest.raises(capi.KrError) as e:
        b.fastq_names()
    assert e.value.code == capi.KR_ERR_STATE
    for bad_args in ((comp, BLOCK, BLOCK), (comp, 0, 3 * BLOCK + 1), (comp, 0, BLOCK - 1)):  # skip outside member 1; past U; two members behind the chunk
        with pytest.raises(capi.KrError) as e:
            b.submit_bgzf(*bad_args)
        assert e.value.code == capi.KR_ERR_ARG, bad_args
    with pytest.raises(capi.KrError) as e:
        b.submit_bgzf(comp[:-3], 0, BLOCK)
    assert e.value.code == capi.KR_ERR_FORMAT
    a = stream(capi, hx, dx, True)
    want = a.submit_fastq(text[:3 * BLOCK], 0, 0)
    summ, raw = b.submit_bgzf(comp, 0, 3 * BLOCK, 0, False, 0)
    assert summ == want and b.collect_text() == a.collect_text()
    a.close(), b.close()
