"""The reads of a seek batch split on the device (csrc/kr_dev_extract.inc, kr_stream_extract_enable) against a split done here: the
chunk's bytes are cut at the record starts this file built them with, and every record goes to the part that the verdict
    matched = !isnan(d) && (isnan(max_dist) || d <= max_dist)
names for the d that collect_seek() returns for the SAME batch -- identical doubles on both sides, no tolerance anywhere.  Records
are kept as the list of their exact bytes, so the expectation never parses anything.  Sketch A of tests/seek_craft.py."""
import math

import numpy as np
import pytest

import seek_craft as sc

pytestmark = pytest.mark.gpu

K = sc.CFG_A["k"]
NAN = float("nan")


def fq(name, seq, qual=None):
    return b"@%s\n%s\n+\n%s\n" % (name.encode(), seq.encode(), (qual or "I" * len(seq)).encode())


def fa(name, seq, wrap=0, eol=b"\n"):
    body = [seq[i:i + wrap] for i in range(0, len(seq), wrap)] if wrap else [seq]
    return b">" + name.encode() + eol + b"".join(s.encode() + eol for s in body)


MAKE = {"fastq": fq, "fasta": fa}


@pytest.fixture(scope="module")
def env(capi, po, tmp_path_factory):
    d = tmp_path_factory.mktemp("seekx")
    g = sc.genome_a()
    hx = capi.HostIndex(sc.write_sketch(capi, d, "a", g, sc.CFG_A), sketch=True)
    dx = hx.upload(0)
    return {"g": g[0], "dx": dx, "hx": hx}


def new_stream(capi, env, raw_cap=1 << 20, max_reads=4096, extract=True, bgzf_in=0, text=True):
    st = env["dx"].stream(params=capi.default_params(hdist_th=4), max_reads=max_reads, max_bases=1 << 20)
    st.seek_enable(1 << 20, 1 << 18) if text else st.seek_enable()
    st.fastq_enable(raw_cap)
    if bgzf_in:
        st.bgzf_enable(bgzf_in)
    if extract:
        st.extract_enable()
    return st


@pytest.fixture(scope="module")
def st(capi, env):
    s = new_stream(capi, env)
    yield s
    s.close()


def verdicts(d, mx=NAN):
    return ~np.isnan(d) & (True if math.isnan(mx) else (d <= mx))


def expect(recs, d, mx=NAN):
    m = verdicts(d, mx)
    assert len(m) == len(recs)
    return b"".join(r for r, k in zip(recs, m) if k), b"".join(r for r, k in zip(recs, m) if not k), int(m.sum())


def run(capi, st, fmt, recs, mx=NAN, tail=b"", at_eof=1, want_status=None):
    """submit recs (+ tail), check the accepted prefix's split; -> (fp, extract dict, d)"""
    raw = b"".join(recs) + tail
    fp = (st.submit_fastq if fmt == "fastq" else st.submit_fasta)(raw, capi.KR_SEEK | capi.KR_TILE_DEVICE, at_eof)
    n = fp["nreads"]
    assert fp["status"] == (capi.KR_FASTQ_OK if want_status is None else want_status), fp
    assert fp["consumed"] == sum(len(r) for r in recs[:n])  # the accepted records tile [0, consumed)
    d = st.collect_seek()["d"]
    wm, wu, nm = expect(recs[:n], d, mx)
    ex = st.collect_extract()
    assert (ex["nreads"], ex["nmatched"], ex["matched_bytes"], ex["unmatched_bytes"]) == (n, nm, len(wm), len(wu))
    assert ex["matched"] == wm and ex["unmatched"] == wu
    return fp, ex, d


def mixed_records(env, fmt):
    """mutated genome substrings and random DNA, a read shorter than k, 1,200 and 40,000 bases, names of 1, 7 and 200 bytes, header
    comments; FASTA: bodies wrapped at 60 with CRLF and a run of empty records"""
    g, rng = env["g"], np.random.default_rng(31)
    mk = MAKE[fmt]
    recs = []
    for i in range(12):
        recs.append(mk(f"m{i} mutated copy={i}", sc.mutate(rng, g[300 * i:300 * i + 150], 0.02)))
        recs.append(mk(f"x{i}", sc.random_dna(rng, 150)))
    recs.append(mk("s", g[50:50 + K - 1]))  # shorter than k: no k-mer, NaN
    recs.append(mk("longish", g[2000:3200]))
    recs.append(mk("n" * 200 + "\tcomment", sc.random_dna(rng, 20000) + g[100:5100] + sc.random_dna(rng, 15000)))
    recs.append(mk("q", sc.random_dna(rng, 1200)))
    if fmt == "fasta":
        recs.insert(5, fa("wrapped crlf", g[4000:4500], wrap=60, eol=b"\r\n"))
        recs.insert(9, fa("wrapped", sc.random_dna(rng, 333), wrap=60))
        recs[14:14] = [b">\n"] * 21  # several records inside one lane's 16 bytes
        recs.insert(40, fa("after the run", g[6000:6150]))
    return recs


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_mixed_all_and_none(capi, env, st, fmt):
    recs = mixed_records(env, fmt)
    fp, ex, d = run(capi, st, fmt, recs)
    assert fp["nreads"] == len(recs)
    assert 0 < ex["nmatched"] < ex["nreads"]  # both classes
    assert len(ex["matched"]) + len(ex["unmatched"]) == sum(map(len, recs))
    g, rng, mk = env["g"], np.random.default_rng(32), MAKE[fmt]
    _, ex, _ = run(capi, st, fmt, [mk(f"e{i}", g[100 * i:100 * i + 150]) for i in range(40)])
    assert ex["nmatched"] == 40 and ex["unmatched"] == b""
    _, ex, _ = run(capi, st, fmt, [mk(f"r{i}", sc.random_dna(rng, 150)) for i in range(40)])
    assert ex["nmatched"] == 0 and ex["matched"] == b""
    assert st.extract_ms() >= 0


def seam_records(env, fmt, target):
    """records alternating matched / unmatched, one of them given a padded name so that the next record starts at byte `target`"""
    g, rng, mk = env["g"], np.random.default_rng(33), MAKE[fmt]
    base = len(mk("", "A" * 150))
    recs, cur, i = [], 0, 0
    seq = lambda j: g[40 * j:40 * j + 150] if j % 2 else sc.random_dna(rng, 150)
    while target - cur > 2 * base + 100:
        recs.append(mk(f"r{i}", seq(i)))
        cur, i = cur + len(recs[-1]), i + 1
    recs.append(mk("p" * (target - cur - base), seq(i)))
    cur, i = cur + len(recs[-1]), i + 1
    assert cur == target
    for _ in range(6):
        recs.append(mk(f"r{i}", seq(i)))
        i += 1
    return recs


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
@pytest.mark.parametrize("target", [4095, 4096, 4097, 4096 + 15, 4096 + 16, 4096 + 17, 2 * 4096 + 16])
def test_seams(capi, env, st, fmt, target):
    recs = seam_records(env, fmt, target)
    _, ex, _ = run(capi, st, fmt, recs)
    assert 0 < ex["nmatched"] < ex["nreads"]


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_last_record_ends_at_consumed(capi, env, st, fmt):
    """bytes behind the last complete record: the prefix ends INCOMPLETE, and nothing at or behind `consumed` is in either part"""
    recs = seam_records(env, fmt, 4096)
    tail = b"@cut\nACGTTGCA" if fmt == "fastq" else b">cut"
    fp, ex, _ = run(capi, st, fmt, recs, tail=tail, at_eof=0, want_status=capi.KR_FASTQ_INCOMPLETE)
    assert fp["nreads"] == len(recs) and b"cut" not in ex["matched"] + ex["unmatched"]


def test_threshold_and_no_stale_verdicts(capi, env):
    st = new_stream(capi, env)
    recs = mixed_records(env, "fastq")
    _, _, d = run(capi, st, "fastq", recs)
    fin = np.sort(d[~np.isnan(d)])
    assert len(fin) >= 8 and fin[0] < fin[-1]
    own = float(fin[len(fin) // 3])  # one read's own d: `<=` keeps that read
    st.extract_max(own)
    _, ex, d2 = run(capi, st, "fastq", recs, mx=own)
    assert np.array_equal(d, d2, equal_nan=True)
    assert ex["nmatched"] == int((fin <= own).sum()) and 0 < ex["nmatched"] < len(fin)
    med = float(np.median(fin))
    st.extract_max(med)
    _, ex, _ = run(capi, st, "fastq", recs, mx=med)
    assert ex["nmatched"] == int((fin <= med).sum())
    # batches of other content on the same stream, under the threshold and without it
    g, rng = env["g"], np.random.default_rng(34)
    run(capi, st, "fastq", [fq(f"r{i}", sc.random_dna(rng, 150)) for i in range(50)], mx=med)
    run(capi, st, "fasta", [fa(f"e{i}", g[90 * i:90 * i + 200]) for i in range(30)], mx=med)
    st.extract_max(NAN)
    _, ex, _ = run(capi, st, "fastq", recs)
    assert ex["nmatched"] == len(fin)
    _, ex, _ = run(capi, st, "fasta", [fa(f"e{i}", g[90 * i:90 * i + 200]) for i in range(30)])
    assert ex["nmatched"] == 30
    # a threshold that is refused leaves the rule in force
    st.extract_max(own)
    for bad in (-0.25, float("inf"), float("-inf")):
        with pytest.raises(capi.KrError) as e:
            st.extract_max(bad)
        assert e.value.code == capi.KR_ERR_ARG
    run(capi, st, "fastq", recs, mx=own)
    st.close()


def test_capacity_prefixes_concatenate(capi, env):
    """max_reads = 8: every submit stops at KR_FASTQ_CAPACITY and extracts exactly its accepted prefix; together: the whole file's"""
    st = new_stream(capi, env, max_reads=8)
    g, rng = env["g"], np.random.default_rng(35)
    recs = [fq(f"c{i}", g[70 * i:70 * i + 150] if i % 3 else sc.random_dna(rng, 150)) for i in range(30)]
    pos, got_m, got_u, want_m, want_u, submits = 0, b"", b"", b"", b"", 0
    while pos < len(recs):
        last = len(recs) - pos <= 8
        fp, ex, d = run(capi, st, "fastq", recs[pos:], want_status=capi.KR_FASTQ_OK if last else capi.KR_FASTQ_CAPACITY)
        assert fp["nreads"] == min(8, len(recs) - pos)
        wm, wu, _ = expect(recs[pos:pos + fp["nreads"]], d)
        got_m, got_u, want_m, want_u = got_m + ex["matched"], got_u + ex["unmatched"], want_m + wm, want_u + wu
        pos, submits = pos + fp["nreads"], submits + 1
    assert submits == 4 and got_m == want_m and got_u == want_u
    assert len(got_m) + len(got_u) == sum(map(len, recs)) and got_m and got_u
    st.close()


def test_not_clean_ends_the_prefix(capi, env, st):
    g, rng = env["g"], np.random.default_rng(36)
    recs = [fq(f"k{i}", g[60 * i:60 * i + 150] if i % 2 else sc.random_dna(rng, 150)) for i in range(20)]
    recs[11] = recs[11].replace(b"\n", b"\r\n")
    marker = b"@k11"
    fp, ex, _ = run(capi, st, "fastq", recs, want_status=capi.KR_FASTQ_NOT_CLEAN)
    assert fp["nreads"] == 11
    both = ex["matched"] + ex["unmatched"]
    assert marker not in both and b"@k12" not in both and b"\r" not in both and len(both) == fp["consumed"]


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_bgzf_input_with_skip(capi, env, fmt):
    recs = mixed_records(env, fmt)
    raw = b"".join(recs)
    junk = MAKE[fmt]("junk in front of the chunk", "ACGT" * 200)
    skip = len(junk)
    comp = capi.bgzf_deflate_host_member(junk + raw, 1, 4096)
    st = new_stream(capi, env, bgzf_in=len(comp) + 64)
    fp, inflated = st.submit_bgzf(comp, skip, len(raw), capi.KR_SEEK | capi.KR_TILE_DEVICE, fasta=fmt == "fasta")
    assert inflated == raw and fp["nreads"] == len(recs) and fp["status"] == capi.KR_FASTQ_OK
    wm, wu, nm = expect(recs, st.collect_seek()["d"])
    ex = st.collect_extract()
    assert ex["matched"] == wm and ex["unmatched"] == wu and ex["nmatched"] == nm and 0 < nm < len(recs)
    st.close()


@pytest.mark.parametrize("member", [65280, 256])
def test_bgzf_output(capi, env, member):
    st = new_stream(capi, env)
    st.bgzf_member(member)
    recs = mixed_records(env, "fastq")
    _, ex, _ = run(capi, st, "fastq", recs)
    for level in (1, 2):
        z = st.collect_extract_bgzf(level)
        assert (z["nreads"], z["nmatched"], z["matched_bytes"], z["unmatched_bytes"]) == (ex["nreads"], ex["nmatched"], len(ex["matched"]), len(ex["unmatched"]))
        assert z["matched"] == capi.bgzf_deflate_host_member(ex["matched"], level, member), (level, "matched")
        assert z["unmatched"] == capi.bgzf_deflate_host_member(ex["unmatched"], level, member), (level, "unmatched")
        only = st.collect_extract_bgzf(level, capi.KR_EXTRACT_UNMATCHED)
        assert only["matched"] is None and only["unmatched"] == z["unmatched"]
    assert st.collect_extract() == ex  # the plain parts are still there
    # an empty part: length 0, no member
    g = env["g"]
    _, ex, _ = run(capi, st, "fastq", [fq(f"e{i}", g[100 * i:100 * i + 150]) for i in range(12)])
    z = st.collect_extract_bgzf(1)
    assert ex["unmatched"] == b"" and z["unmatched"] == b"" and z["unmatched_bytes"] == 0
    assert z["matched"] == capi.bgzf_deflate_host_member(ex["matched"], 1, member)
    st.close()


def test_states_and_arguments(capi, env):
    g = env["g"]
    recs = [fq(f"r{i}", g[100 * i:100 * i + 150]) for i in range(8)]
    raw = b"".join(recs)
    flags = capi.KR_SEEK | capi.KR_TILE_DEVICE

    def code(f, *a):
        with pytest.raises(capi.KrError) as e:
            f(*a)
        return e.value.code

    dx = env["dx"]
    s0 = dx.stream(params=capi.default_params(hdist_th=4), max_reads=64, max_bases=1 << 16)
    assert code(s0.extract_enable) == capi.KR_ERR_STATE  # neither seek nor the record finder
    s0.seek_enable(1 << 16, 1 << 12)
    assert code(s0.extract_enable) == capi.KR_ERR_STATE  # no record finder yet
    s0.fastq_enable(1 << 16)
    assert code(s0.collect_extract) == capi.KR_ERR_STATE  # not enabled
    assert code(s0.extract_max, 0.1) == capi.KR_ERR_STATE
    s0.submit_fastq(raw, flags)
    assert code(s0.collect_extract) == capi.KR_ERR_STATE  # a raw-bytes seek batch, but extract is still off
    assert code(s0.extract_enable, -1.0) == capi.KR_ERR_ARG
    assert code(s0.extract_enable, float("inf")) == capi.KR_ERR_ARG
    s0.extract_enable(0.5)
    assert code(s0.extract_enable) == capi.KR_ERR_STATE  # twice
    assert code(s0.collect_extract) == capi.KR_ERR_STATE  # the batch in flight was queued before
    assert code(s0.extract_ms) == capi.KR_ERR_STATE
    s0.extract_max(NAN)
    s0.submit_fastq(raw, flags)
    assert s0.collect_extract()["nreads"] == 8
    for which in (0, 4, 7):
        assert code(s0.collect_extract, which) == capi.KR_ERR_ARG
        assert code(s0.collect_extract_bgzf, 1, which) == capi.KR_ERR_ARG
    for level in (0, 3):
        assert code(s0.collect_extract_bgzf, level) == capi.KR_ERR_ARG
    one = s0.collect_extract(capi.KR_EXTRACT_MATCHED)
    assert one["unmatched"] is None and one["matched"] == raw and one["unmatched_bytes"] == 0
    # a seek batch from host arrays runs as before and has nothing to extract
    bases, offs = sc.pack([g[100 * i:100 * i + 150] for i in range(8)])
    s0.submit_text(bases, offs, [f"r{i}" for i in range(8)], capi.KR_SEEK)
    assert s0.collect_seek()["nreads"] == 8 and s0.collect_text().count(b"\n") == 8
    assert code(s0.collect_extract) == capi.KR_ERR_STATE
    # a submit that accepted no record
    s0.submit_fastq(raw, flags)
    fp = s0.submit_fastq(b"@cut\nACGT", flags, 0)
    assert fp["nreads"] == 0
    assert code(s0.collect_extract) == capi.KR_ERR_STATE
    # a dist batch
    s0.submit_fastq(raw, flags)
    s0.submit(bases, offs, capi.KR_TAP_ACCS)
    s0.collect()
    assert code(s0.collect_extract) == capi.KR_ERR_STATE
    assert code(s0.collect_extract_bgzf, 1) == capi.KR_ERR_STATE
    s0.close()


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_text_and_values_are_untouched(capi, env, st, fmt):
    """collect_text and collect_seek of a batch on an extract-enabled stream equal those of a stream without it, in either order"""
    recs = mixed_records(env, fmt)
    raw = b"".join(recs)
    plain = new_stream(capi, env, extract=False)
    (plain.submit_fastq if fmt == "fastq" else plain.submit_fasta)(raw, capi.KR_SEEK | capi.KR_TILE_DEVICE)
    wt, wv = plain.collect_text(), plain.collect_seek()
    (st.submit_fastq if fmt == "fastq" else st.submit_fasta)(raw, capi.KR_SEEK | capi.KR_TILE_DEVICE)
    ex = st.collect_extract()
    assert st.collect_text() == wt and wt.count(b"\n") == len(recs)
    v = st.collect_seek()
    assert all(np.array_equal(v[f], wv[f], equal_nan=True) for f in ("d", "d_strand", "hist", "onmers"))
    assert st.collect_extract() == ex and st.collect_text() == wt
    plain.close()
