"""Paired reads split together on the device (kr_ex_pair_kernel in csrc/kr_dev_extract.inc, kr_stream_extract_defer,
kr_batch_extract_pair) against a split done here.  The verdict of a pair is computed in numpy from collect_seek()["d"] of the SAME
two batches -- identical doubles on both sides, no tolerance anywhere --
    matched(d) = !isnan(d) && (isnan(max_dist) || d <= max_dist);  any: matched(d1) || matched(d2);  both: matched(d1) && matched(d2)
and every record goes, as the exact bytes this file built it with, to the part its PAIR's verdict names: record i of the matched part
of stream 1 is the mate of record i of the matched part of stream 2.  Sketch A of tests/seek_craft.py."""
import ctypes as C
import math

import numpy as np
import pytest

import seek_craft as sc

pytestmark = pytest.mark.gpu

K = sc.CFG_A["k"]
NAN = float("nan")
RULES = ["any", "both"]


def fq(name, seq, qual=None):
    return b"@%s\n%s\n+\n%s\n" % (name.encode(), seq.encode(), (qual or "I" * len(seq)).encode())


def fa(name, seq):
    return b">%s\n%s\n" % (name.encode(), seq.encode())


@pytest.fixture(scope="module")
def env(capi, po, tmp_path_factory):
    d = tmp_path_factory.mktemp("seekpairs")
    g = sc.genome_a()
    path = sc.write_sketch(capi, d, "a", g, sc.CFG_A)
    hx = capi.HostIndex(path, sketch=True)
    dx = hx.upload(0)
    return {"g": g[0], "dx": dx, "hx": hx, "path": path}


def new_stream(capi, env, raw_cap=1 << 20, max_reads=4096, max_bases=1 << 20, extract=True, defer=True, mx=NAN):
    st = env["dx"].stream(params=capi.default_params(hdist_th=4), max_reads=max_reads, max_bases=max_bases)
    st.seek_enable(1 << 20, 1 << 18)
    st.fastq_enable(raw_cap)
    if extract:
        st.extract_enable(mx)
        if defer:
            st.extract_defer(True)
    return st


@pytest.fixture(scope="module")
def sts(capi, env):
    a, b = new_stream(capi, env), new_stream(capi, env)
    yield a, b
    a.close()
    b.close()


FLAGS = lambda capi: capi.KR_SEEK | capi.KR_TILE_DEVICE


def matched(d, mx=NAN):
    return ~np.isnan(d) & (True if math.isnan(mx) else (d <= mx))


def pair_verdict(d1, d2, rule, mx=NAN):
    m1, m2 = matched(d1, mx), matched(d2, mx)
    return (m1 | m2) if rule == "any" else (m1 & m2)


def split(recs, keep):
    assert len(recs) == len(keep)
    return b"".join(r for r, k in zip(recs, keep) if k), b"".join(r for r, k in zip(recs, keep) if not k)


def check_side(st, recs, keep):
    wm, wu = split(recs, keep)
    ex = st.collect_extract()
    assert (ex["nreads"], ex["nmatched"], ex["matched_bytes"], ex["unmatched_bytes"]) == (len(recs), int(np.sum(keep)), len(wm), len(wu))
    assert ex["matched"] == wm and ex["unmatched"] == wu
    return ex


def run_two(capi, a, b, r1, r2, rule, mx=NAN, submit=True, fasta=False):
    """mates in two streams: submit both, pair them under `rule`, check both splits; -> (verdict per pair, d1, d2)"""
    if submit:
        for st, recs in ((a, r1), (b, r2)):
            fp = (st.submit_fasta if fasta else st.submit_fastq)(b"".join(recs), FLAGS(capi), 1)
            assert fp["status"] == capi.KR_FASTQ_OK and fp["nreads"] == len(recs), fp
    d1, d2 = a.collect_seek()["d"], b.collect_seek()["d"]
    a.extract_pair(b, getattr(capi, "KR_PAIR_" + rule.upper()))
    keep = pair_verdict(d1, d2, rule, mx)
    ea, eb = check_side(a, r1, keep), check_side(b, r2, keep)
    assert ea["nmatched"] == eb["nmatched"]  # the parts stay in step
    return keep, d1, d2


def run_interleaved(capi, a, r1, r2, rule, mx=NAN, submit=True):
    recs = [x for p in zip(r1, r2) for x in p]
    if submit:
        fp = a.submit_fastq(b"".join(recs), FLAGS(capi), 1)
        assert fp["status"] == capi.KR_FASTQ_OK and fp["nreads"] == len(recs), fp
    d = a.collect_seek()["d"]
    a.extract_pair(a, getattr(capi, "KR_PAIR_" + rule.upper()))
    keep = pair_verdict(d[0::2], d[1::2], rule, mx)
    check_side(a, recs, np.repeat(keep, 2))
    return keep, d[0::2], d[1::2]


def mixed_pairs(env, n=40, seed=51):
    """about n pairs, mates of different lengths and names (/1, /2): genome substrings are matched reads, random DNA unmatched ones, in
    all four combinations; one mate shorter than k and one of 40,000 bases"""
    g, rng = env["g"], np.random.default_rng(seed)
    gen = lambda i, L: sc.mutate(rng, g[150 * i:150 * i + L], 0.02)
    r1, r2 = [], []
    for i in range(n):
        c = i % 4  # 0: both from the genome, 1: mate 1 only, 2: mate 2 only, 3: neither
        s1 = gen(i, 150 + i % 5) if c in (0, 1) else sc.random_dna(rng, 150 + i % 5)
        s2 = gen(i + 1, 100 + i % 3) if c in (0, 2) else sc.random_dna(rng, 100 + i % 3)
        r1.append(fq(f"p{i}/1 first mate", s1))
        r2.append(fq(f"p{i}/2", s2))
    r1.append(fq("short/1", g[50:50 + K - 1])), r2.append(fq("short/2", g[900:1050]))  # shorter than k: NaN
    r1.append(fq("long/1", sc.random_dna(rng, 150))), r2.append(fq("long/2", sc.random_dna(rng, 20000) + g[100:5100] + sc.random_dna(rng, 14900)))
    return r1, r2


def simple_pairs(env, n, seed=52, all_matched=None):
    """n pairs of 150 / 100 bases; all_matched None: the four combinations in turn, True: every mate from the genome, False: every
    mate shorter than k (no k-mer: NaN whatever the bases are -- random DNA of full length now and then finds a hit)"""
    g, rng = env["g"], np.random.default_rng(seed)
    r1, r2 = [], []
    if all_matched is False:
        return ([fq(f"s{i}/1", sc.random_dna(rng, K - 1)) for i in range(n)], [fq(f"s{i}/2", sc.random_dna(rng, K - 2 - i % 3)) for i in range(n)])
    for i in range(n):
        c = i % 4 if all_matched is None else (0 if all_matched else 3)
        o = (37 * i) % (len(g) - 400)
        r1.append(fq(f"s{i}/1", g[o:o + 150] if c in (0, 1) else sc.random_dna(rng, 150)))
        r2.append(fq(f"s{i}/2", g[o + 200:o + 300] if c in (0, 2) else sc.random_dna(rng, 100)))
    return r1, r2


def name_pos(capi, st, r):
    """kr_batch_fastq_names: where record r's name begins in the chunk last submitted (its '@' is the byte in front)"""
    pos, ln = C.POINTER(C.c_uint64)(), C.POINTER(C.c_uint32)()
    capi.check(capi.load().kr_batch_fastq_names(st.h, C.byref(pos), C.byref(ln)))
    return int(pos[r])


def four_combinations(d1, d2):
    m1, m2 = matched(d1), matched(d2)
    return {(bool(x), bool(y)) for x, y in zip(m1, m2)} == {(True, True), (True, False), (False, True), (False, False)}


@pytest.mark.parametrize("rule", RULES)
def test_mixed_two_streams(capi, env, sts, rule):
    r1, r2 = mixed_pairs(env)
    keep, d1, d2 = run_two(capi, *sts, r1, r2, rule)
    assert four_combinations(d1, d2)
    assert 0 < keep.sum() < len(keep)
    assert len(b"".join(r1)) != len(b"".join(r2))
    assert sts[0].extract_ms() >= 0 and sts[1].extract_ms() >= 0


@pytest.mark.parametrize("rule", RULES)
def test_mixed_interleaved(capi, env, sts, rule):
    r1, r2 = mixed_pairs(env)
    keep, d1, d2 = run_interleaved(capi, sts[0], r1, r2, rule)
    assert four_combinations(d1, d2) and 0 < keep.sum() < len(keep)


def test_rules_differ_where_they_must(capi, env, sts):
    r1, r2 = mixed_pairs(env)
    ka, d1, d2 = run_two(capi, *sts, r1, r2, "any")
    kb, _, _ = run_two(capi, *sts, r1, r2, "both", submit=False)  # the pair call twice on one batch: the parts are overwritten
    assert kb.sum() < ka.sum() and not (kb & ~ka).any()
    ka2, _, _ = run_two(capi, *sts, r1, r2, "any", submit=False)
    assert np.array_equal(ka, ka2)
    ki, _, _ = run_interleaved(capi, sts[0], r1, r2, "both")
    kj, _, _ = run_interleaved(capi, sts[0], r1, r2, "any", submit=False)
    assert np.array_equal(ki, kb) and np.array_equal(kj, ka)


@pytest.mark.parametrize("rule", RULES)
def test_one_pair_and_two_interleaved_records(capi, env, sts, rule):
    g = env["g"]
    rng = np.random.default_rng(53)
    for s1, s2 in ((g[0:150], g[300:400]), (g[0:150], sc.random_dna(rng, 100)), (sc.random_dna(rng, 150), sc.random_dna(rng, 100))):
        r1, r2 = [fq("one/1", s1)], [fq("one/2", s2)]
        run_two(capi, *sts, r1, r2, rule)
        run_interleaved(capi, sts[0], r1, r2, rule)


@pytest.mark.parametrize("rule", RULES)
@pytest.mark.parametrize("delta", [-1, 0, 1])
def test_prefix_block_boundary(capi, env, sts, rule, delta):
    n = capi.seek_layout()["row_block"] + delta  # the reads per prefix block of the extract kernels
    r1, r2 = simple_pairs(env, n)
    keep, _, _ = run_two(capi, *sts, r1, r2, rule)
    assert 0 < keep.sum() < n
    half = (n + 1) // 2  # interleaved: n records or n + 1, around the same boundary
    run_interleaved(capi, sts[0], r1[:half], r2[:half], rule)


@pytest.mark.parametrize("rule", RULES)
def test_threshold_equal_to_a_reads_own_d(capi, env, rule):
    r1, r2 = mixed_pairs(env)
    a, b = new_stream(capi, env), new_stream(capi, env)
    _, d1, d2 = run_two(capi, a, b, r1, r2, rule)
    fin = np.sort(np.concatenate([d1[~np.isnan(d1)], d2[~np.isnan(d2)]]))
    assert len(fin) >= 8 and fin[0] < fin[-1]
    own = float(fin[2 * len(fin) // 3])  # one read's own d: `<=` keeps that read
    a.extract_max(own), b.extract_max(own)
    keep, e1, e2 = run_two(capi, a, b, r1, r2, rule, mx=own)
    assert np.array_equal(d1, e1, equal_nan=True) and np.array_equal(d2, e2, equal_nan=True)
    at = (d1 == own) | (d2 == own)
    assert at.any() and 0 < keep.sum() < len(keep)
    if rule == "any":
        assert keep[at].all()  # the read at the threshold is matched, so its pair is
    ki, _, _ = run_interleaved(capi, a, r1, r2, rule, mx=own)
    assert np.array_equal(ki, keep)
    # thresholds that differ are refused; equal again they are taken
    b.extract_max(float(fin[-1]))
    a.submit_fastq(b"".join(r1), FLAGS(capi), 1), b.submit_fastq(b"".join(r2), FLAGS(capi), 1)
    with pytest.raises(capi.KrError) as e:
        a.extract_pair(b)
    assert e.value.code == capi.KR_ERR_STATE and "threshold" in str(e.value)
    b.extract_max(NAN)
    with pytest.raises(capi.KrError) as e:
        a.extract_pair(b)
    assert e.value.code == capi.KR_ERR_STATE
    a.extract_max(NAN)
    a.submit_fastq(b"".join(r1), FLAGS(capi), 1), b.submit_fastq(b"".join(r2), FLAGS(capi), 1)
    run_two(capi, a, b, r1, r2, rule, submit=False)
    a.close(), b.close()


@pytest.mark.parametrize("rule", RULES)
def test_no_stale_pair_values(capi, env, sts, rule):
    a, b = sts
    r1, r2 = mixed_pairs(env)
    k1, _, _ = run_two(capi, a, b, r1, r2, rule)
    k2, _, _ = run_two(capi, a, b, r2, r1, rule)  # the mates' files swapped
    assert np.array_equal(k1, k2)
    m1, m2 = simple_pairs(env, 60, all_matched=True)
    u1, u2 = simple_pairs(env, 60, all_matched=False)
    k, _, _ = run_two(capi, a, b, m1, m2, rule)
    assert k.all()
    k, _, _ = run_two(capi, a, b, u1, u2, rule)
    assert not k.any()
    k, _, _ = run_interleaved(capi, a, m1, m2, rule)
    assert k.all()
    k, _, _ = run_interleaved(capi, a, u1[:20], u2[:20], rule)  # fewer records than the batch before
    assert not k.any()
    k, _, _ = run_two(capi, a, b, r1, r2, rule)
    assert np.array_equal(k, k1)


@pytest.mark.parametrize("rule", RULES)
def test_fasta_records(capi, env, sts, rule):
    g, rng = env["g"], np.random.default_rng(54)
    r1 = [fa(f"c{i}/1", g[200 * i:200 * i + 180] if i % 4 in (0, 1) else sc.random_dna(rng, 180)) for i in range(24)]
    r2 = [fa(f"c{i}/2", g[200 * i + 300:200 * i + 420] if i % 4 in (0, 2) else sc.random_dna(rng, 120)) for i in range(24)]
    keep, d1, d2 = run_two(capi, *sts, r1, r2, rule, fasta=True)
    assert four_combinations(d1, d2) and 0 < keep.sum() < 24


@pytest.mark.parametrize("level", [1, 2])
def test_bgzf_collect_on_both_streams(capi, env, level):
    a, b = new_stream(capi, env), new_stream(capi, env)
    a.bgzf_member(256), b.bgzf_member(256)
    r1, r2 = mixed_pairs(env)
    run_two(capi, a, b, r1, r2, "any")
    for st in (a, b):
        ex = st.collect_extract()
        z = st.collect_extract_bgzf(level)
        assert (z["nreads"], z["nmatched"], z["matched_bytes"], z["unmatched_bytes"]) == (ex["nreads"], ex["nmatched"], len(ex["matched"]), len(ex["unmatched"]))
        assert z["matched"] == capi.bgzf_deflate_host_member(ex["matched"], level, 256)
        assert z["unmatched"] == capi.bgzf_deflate_host_member(ex["unmatched"], level, 256)
        assert st.collect_extract() == ex
    a.close(), b.close()


@pytest.mark.parametrize("rule", RULES)
def test_realign_after_capacity(capi, env, rule):
    """mates of 150 and 100 bases on streams that hold 1,000 bases: the longer mates' side stops first (6 records against 10).  The
    longer prefix is submitted once more, cut at the start of record n_min (kr_batch_fastq_names: name_pos[n_min] - 1), and the loop
    goes on behind both prefixes; the prefixes' parts concatenate to the whole expectation"""
    a, b = new_stream(capi, env, max_bases=1000), new_stream(capi, env, max_bases=1000)
    plain1, plain2 = new_stream(capi, env, extract=False), new_stream(capi, env, extract=False)
    r1, r2 = simple_pairs(env, 23)
    raw = [b"".join(r1), b"".join(r2)]
    plain1.submit_fastq(raw[0], FLAGS(capi), 1), plain2.submit_fastq(raw[1], FLAGS(capi), 1)
    whole = pair_verdict(plain1.collect_seek()["d"], plain2.collect_seek()["d"], rule)
    assert 0 < whole.sum() < 23
    pos, done, got, realigned, rounds = [0, 0], 0, [b"", b"", b"", b""], 0, 0
    while done < 23:
        fps = [st.submit_fastq(raw[k][pos[k]:], FLAGS(capi), 1) for k, st in enumerate((a, b))]
        for fp in fps:
            assert fp["status"] in (capi.KR_FASTQ_OK, capi.KR_FASTQ_CAPACITY) and fp["nreads"] > 0, fp
        n = min(fp["nreads"] for fp in fps)
        for k, st in enumerate((a, b)):
            if fps[k]["nreads"] == n:
                continue
            cut = name_pos(capi, st, n) - 1
            assert raw[k][pos[k] + cut:pos[k] + cut + 1] == b"@"
            fps[k] = st.submit_fastq(raw[k][pos[k]:pos[k] + cut], FLAGS(capi), 0)
            assert fps[k]["status"] == capi.KR_FASTQ_OK and fps[k]["nreads"] == n
            realigned += 1
        keep, _, _ = run_two(capi, a, b, r1[done:done + n], r2[done:done + n], rule, submit=False)
        assert np.array_equal(keep, whole[done:done + n])
        ea, eb = a.collect_extract(), b.collect_extract()
        got = [got[0] + ea["matched"], got[1] + ea["unmatched"], got[2] + eb["matched"], got[3] + eb["unmatched"]]
        pos, done, rounds = [pos[0] + fps[0]["consumed"], pos[1] + fps[1]["consumed"]], done + n, rounds + 1
    assert realigned >= 2 and rounds >= 3
    assert got[0:2] == list(split(r1, whole)) and got[2:4] == list(split(r2, whole))
    for st in (a, b, plain1, plain2):
        st.close()


def test_text_and_values_are_untouched(capi, env, sts):
    a, b = sts
    r1, r2 = mixed_pairs(env)
    want = []
    for recs in (r1, r2):
        plain = new_stream(capi, env, extract=False)
        plain.submit_fastq(b"".join(recs), FLAGS(capi), 1)
        want.append((plain.collect_text(), plain.collect_seek()))
        plain.close()
    a.submit_fastq(b"".join(r1), FLAGS(capi), 1), b.submit_fastq(b"".join(r2), FLAGS(capi), 1)
    assert a.collect_text() == want[0][0]  # before the pair call ...
    a.extract_pair(b, capi.KR_PAIR_BOTH)
    for st, (wt, wv) in zip((a, b), want):  # ... and after it
        ex = st.collect_extract()
        assert st.collect_text() == wt and wt.count(b"\n") == len(r1)
        v = st.collect_seek()
        assert all(np.array_equal(v[f], wv[f], equal_nan=True) for f in ("d", "d_strand", "hist", "onmers"))
        assert st.collect_extract() == ex


def test_states_and_arguments(capi, env):
    g = env["g"]
    recs = [fq(f"r{i}", g[100 * i:100 * i + 150]) for i in range(8)]
    raw, flags = b"".join(recs), FLAGS(capi)

    def err(f, *a):
        with pytest.raises(capi.KrError) as e:
            f(*a)
        return e.value.code, str(e.value)

    STATE, ARG = capi.KR_ERR_STATE, capi.KR_ERR_ARG
    dx = env["dx"]
    s0 = dx.stream(params=capi.default_params(hdist_th=4), max_reads=64, max_bases=1 << 16)
    s0.seek_enable(1 << 16, 1 << 12)
    s0.fastq_enable(1 << 16)
    assert err(s0.extract_defer)[0] == STATE  # before kr_stream_extract_enable
    a, b = new_stream(capi, env, defer=False), new_stream(capi, env)
    assert err(a.extract_pair, s0)[0] == STATE and err(s0.extract_pair, s0)[0] == STATE  # not extract-enabled
    a.submit_fastq(raw, flags), b.submit_fastq(raw, flags)
    assert err(a.extract_pair, b)[0] == STATE and err(b.extract_pair, a)[0] == STATE  # a does not defer
    assert a.collect_extract()["nreads"] == 8  # ... and split its batch by its own reads
    a.extract_defer(True)
    assert err(a.extract_pair, b)[0] == STATE  # a's batch was queued before: already split, not deferred ... (its stream defers now)
    for rule in (0, 3, 4):
        assert err(a.extract_pair, b, rule)[0] == ARG
    # a collect before the pair call
    a.submit_fastq(raw, flags)
    for f in (a.collect_extract, lambda: a.collect_extract_bgzf(1), b.collect_extract):
        code, msg = err(f)
        assert code == STATE and "kr_batch_extract_pair" in msg
    a.extract_pair(b)
    assert a.collect_extract()["nmatched"] == 8 and b.collect_extract()["nmatched"] == 8
    # record counts that differ, named in the message
    b.submit_fastq(b"".join(recs[:5]), flags)
    code, msg = err(a.extract_pair, b)
    assert code == STATE and "8 and 5" in msg
    # an odd interleaved batch
    code, msg = err(b.extract_pair, b)
    assert code == STATE and "5" in msg
    a.extract_pair(a)  # 8 records: four interleaved pairs
    assert a.collect_extract()["nmatched"] == 8
    # the last submit was not a raw-bytes seek batch
    bases, offs = sc.pack([g[100 * i:100 * i + 150] for i in range(8)])
    b.submit_text(bases, offs, [f"r{i}" for i in range(8)], capi.KR_SEEK)
    assert err(a.extract_pair, b)[0] == STATE
    b.submit_fastq(raw, flags)
    fp = b.submit_fastq(b"@cut\nACGT", flags, 0)  # a submit that accepted no record
    assert fp["nreads"] == 0 and err(a.extract_pair, b)[0] == STATE
    # another index
    hx2 = capi.HostIndex(env["path"], sketch=True)
    dx2 = hx2.upload(0)
    c = dx2.stream(params=capi.default_params(hdist_th=4), max_reads=64, max_bases=1 << 16)
    c.seek_enable(1 << 16, 1 << 12), c.fastq_enable(1 << 16), c.extract_enable(), c.extract_defer(True)
    c.submit_fastq(raw, flags)
    b.submit_fastq(raw, flags)
    code, msg = err(b.extract_pair, c)
    assert code == STATE and "index" in msg
    c.close(), dx2.close(), hx2.close()
    # with defer off again a submit splits per read exactly as before
    a.extract_defer(False)
    rng = np.random.default_rng(55)
    mix = [fq(f"m{i}", g[100 * i:100 * i + 150] if i % 2 else sc.random_dna(rng, 150)) for i in range(20)]
    a.submit_fastq(b"".join(mix), flags)
    keep = matched(a.collect_seek()["d"])
    check_side(a, mix, keep)
    assert 0 < keep.sum() < 20
    assert err(a.extract_pair, a)[0] == STATE
    for st in (s0, a, b):
        st.close()
