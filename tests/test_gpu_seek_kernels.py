"""A batch flagged KR_SEEK: the seek kernels (csrc/kr_dev_seek.inc) against three ground truths, independently --
  (a) the brute force of tests/seek_craft.py from the sketch as the oracle reads it: hist and onmers, exactly;
  (b) the old path on the same batch: the dist chain with KR_TAP_ACCS (rec_hist, read_onmers: exactly) and kr_format_seek (the text,
      byte for byte);
  (c) the oracle: po.Sketch.seek's text byte for byte, every non-NaN d within 1e-6 relative of its rows (the project's DIST tolerance),
      NaN exactly where it says NaN --
on reads crafted for the seams of the unit split (T positions a unit, read from kr_debug_seek_layout), then the interfaces: text with
short and long ids, both capacity errors and the halves after them, raw FASTQ / FASTA bytes with long records, the three locations
of the bases, consecutive batches on one stream, and the CLI's --gpu-seek."""
import ctypes as C
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import seek_craft as sc
from conftest import GOLDEN, ROOT
from test_seek import make_reads

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
K = sc.CFG_A["k"]


class Sk:
    """one sketch: the oracle's view, the host index, the device index, streams by threshold"""

    def __init__(self, capi, po, path, genome):
        self.capi, self.path, self.genome = capi, path, genome
        self.po = po.Sketch(path)
        self.hx = capi.HostIndex(path, sketch=True)
        self.dx = self.hx.upload(0)
        self.streams = {}

    def stream(self, th, max_reads=4096, max_bases=1 << 21):
        """(a tile of the old path counts as a read: room for the long reads' tiles)"""
        key = (th, max_reads, max_bases)
        if key not in self.streams:
            st = self.dx.stream(params=self.capi.default_params(hdist_th=th), max_reads=max_reads, max_bases=max_bases)
            st.seek_enable(1 << 22, 1 << 20)
            self.streams[key] = st
        return self.streams[key]


@pytest.fixture(scope="module")
def T(capi):
    return capi.seek_layout()["unit"]


@pytest.fixture(scope="module")
def sketches(capi, po, tmp_path_factory):
    d = tmp_path_factory.mktemp("seek")
    ga = sc.genome_a()
    out = {"A": Sk(capi, po, sc.write_sketch(capi, d, "a", ga, sc.CFG_A), ga)}
    gl = [sc.random_dna(np.random.default_rng(21), 800000)]  # long enough for a read that puts bin 0 above 65,535
    out["AL"] = Sk(capi, po, sc.write_sketch(capi, d, "al", gl, sc.CFG_A), gl)
    gc = [sc.random_dna(np.random.default_rng(23), 9000)]
    out["C"] = Sk(capi, po, sc.write_sketch(capi, d, "c", gc, sc.CFG_C), gc)
    # B: 32 rows.  A random genome of 12,000 bases gives buckets of 47 codes on average (one k-mer in eight is kept: 9,000 bases
    # give 35, and no row above 59 for any of twenty seeds); seed 50 puts 75 into one row (chosen on the CPU, asserted by the test)
    gb = [sc.random_dna(np.random.default_rng(50), 12000)]
    out["B"] = Sk(capi, po, sc.write_sketch(capi, d, "b", gb, sc.CFG_B), gb)
    return out


def reads_a(g, T):
    """tests/test_seek.py's mix, then the reads named for the seams (lengths for k = 21)"""
    names, bases, offs = make_reads(g)
    reads = [bytes(bases[int(offs[i]):int(offs[i + 1])]).decode() for i in range(len(names))]
    c = g[0]
    rng = np.random.default_rng(8)
    for L in (K - 1, K, 84, 85, T + K - 2, T + K - 1, T + K):  # below k; 1, 64, 65 positions; T - 1, T, T + 1 positions
        reads.append(c[300:300 + L])
        names.append(f"len{L}")
    L = 3 * T + 17 + K - 1
    for b in range(T - 1, T + K - 1):  # an N whose invalid k-mers end at the first seam, then straddle it, base by base
        s = c[1000:1000 + L]
        reads.append(s[:b] + "N" + s[b + 1:])
        names.append(f"seamN{b}")
    reads += ["N" * 300, sc.revcomp(c[2000:2400]), c[5000:5150], sc.random_dna(rng, 150), c[6000:6100] + "\xc1" + c[6101:6200]]
    names += ["allN300", "revcomp400", "one_strand", "none", "high_byte"]
    return names, reads


def reads_b(g, th):
    rng = np.random.default_rng(9)
    c = g[0]
    reads, names = [], []
    for i, rate in enumerate((0.0, 0.01, 0.05) * 8):
        p = int(rng.integers(0, len(c) - 300))
        s = sc.mutate(rng, c[p:p + int(rng.integers(60, 300))], rate)
        reads.append(sc.revcomp(s) if i % 2 else s)
        names.append(f"b{i}_{rate}")
    return names, reads


def reads_at_threshold(sk, th):
    """k-mers of the sketch's own codes with exactly th and th + 1 substitutions at non-LSH positions: hits at exactly th (the nearest
    entry of the bucket can only be nearer) and, unless another entry is near, misses at th + 1.  Built from the genome: a minimizer
    k-mer of the genome is found by its exact match, then its non-LSH bases are changed."""
    g = sk.genome[0]
    valid, rix, enc = sc.front_end_np(g[:2000], sk.po.k, sk.po.ppos, sk.po.npos)
    starts, ends = sc.buckets(sk.po)
    k = sk.po.k
    npos = sorted(int(x) for x in sk.po.npos)
    out = []
    for i in range(len(valid)):
        row = sc.row_of(int(rix[0][i]), sk.po.m, sk.po.r, bool(sk.po.frac))
        if row is None or int(enc[0][i]) not in sk.po.codes[starts[row]:ends[row]].tolist():
            continue
        km = list(g[i:i + k])
        for nsub in (th, th + 1):
            if nsub > len(npos):
                continue
            s = km[:]
            for p in npos[:nsub]:  # position p counts from the k-mer's last base
                s[k - 1 - p] = "ACGT"[("ACGT".index(s[k - 1 - p]) + 1) % 4]
            out.append("".join(s))
        if len(out) >= 12:
            break
    assert len(out) >= 8
    return [f"at{j}" for j in range(len(out))], out


def old_path(sk, th, names, reads):
    """(b): the dist chain with KR_TAP_ACCS + kr_format_seek"""
    capi = sk.capi
    bases, offs = sc.pack(reads)
    st = sk.stream(th, max_reads=max(4096, len(reads) + 8192), max_bases=max(1 << 21, len(bases)))
    st.submit(bases, offs, capi.KR_TAP_ACCS)
    res = st.collect()
    text = st.format_seek(sk.hx, sk.dx, names, hdist_th=th)
    return sc.hist_of_taps(res, len(reads), th), res.read_onmers, text


def new_path(sk, th, names, reads):
    capi = sk.capi
    bases, offs = sc.pack(reads)
    st = sk.stream(th, max_reads=max(4096, len(reads) + 8192), max_bases=max(1 << 21, len(bases)))
    st.submit_text(bases, offs, names, capi.KR_SEEK)
    text = st.collect_text().decode("latin-1")
    return st.collect_seek(), text


def check_all(sk, th, names, reads, brute16, literal=None):
    """the three ground truths on one batch"""
    v, text = new_path(sk, th, names, reads)
    assert v["nreads"] == len(reads) and v["np"] == th + 1
    # (a) brute force (computed once with every bin: the first th + 1 are this threshold's)
    bh, bo = brute16
    assert np.array_equal(v["onmers"], bo)
    assert np.array_equal(v["hist"], bh[:, :, :th + 1])
    if literal is not None:
        idx, (lh, lo) = literal
        assert np.array_equal(v["hist"][idx], lh[:, :, :th + 1]) and np.array_equal(v["onmers"][idx], lo)
    # (b) the old path
    oh, oo, otext = old_path(sk, th, names, reads)
    assert np.array_equal(v["hist"], oh) and np.array_equal(v["onmers"], oo)
    assert text == otext
    # (c) the oracle
    bases, offs = sc.pack(reads)
    want = sk.po.seek(bases, offs, names, hdist_th=th)
    wd = want["rows"]["d_llh"]
    assert np.array_equal(np.isnan(v["d"]), np.isnan(wd))
    ok = ~np.isnan(wd)
    assert np.all(np.abs(v["d"][ok] - wd[ok]) <= 1e-6 * np.abs(wd[ok]))
    assert text == want["text"]
    # the view's own consistency: NaN exactly where nothing matched, d the smaller strand
    matched = v["hist"].sum(axis=(1, 2)) > 0
    assert np.array_equal(~np.isnan(v["d"]), matched)
    ds = v["d_strand"][matched]
    assert np.array_equal(v["d"][matched], np.where(ds[:, 0] < ds[:, 1], ds[:, 0], ds[:, 1])) and not np.isnan(ds).any()
    return v


@pytest.fixture(scope="module")
def batch_a(sketches, T):
    """sketch A's batch and its brute forces, computed once: the numpy one on every read, the literal one on a sample"""
    sk = sketches["A"]
    names, reads = reads_a(sk.genome, T)
    brute = sc.brute_hist_np(sk.po, reads, 16)
    n0 = len(reads) - 5 - K - 7
    idx = np.array(list(range(0, n0, 6)) + list(range(n0, n0 + 7)) + [n0 + 7, n0 + 7 + K // 2, n0 + 7 + K - 1] + list(range(len(reads) - 5, len(reads))))
    literal = (idx, sc.brute_hist(sk.po, [reads[i] for i in idx], 16))
    return names, reads, brute, literal


@pytest.mark.parametrize("th", [0, 2, 4, 6])
def test_sketch_a(sketches, batch_a, T, th):
    names, reads, brute, literal = batch_a
    assert np.array_equal(brute[0][literal[0]], literal[1][0]) and np.array_equal(brute[1][literal[0]], literal[1][1])
    v = check_all(sketches["A"], th, names, reads, brute, literal)
    at = {n: i for i, n in enumerate(names)}
    assert v["onmers"][at[f"len{K - 1}"]] == 0 and v["onmers"][at[f"len{K}"]] == 1
    assert [int(v["onmers"][at[f"len{L}"]]) for L in (84, 85, T + K - 2, T + K - 1, T + K)] == [64, 65, T - 1, T, T + 1]
    for b in range(T - 1, T + K - 1):  # the N takes the k positions that hold it, wherever the seam falls among them
        assert v["onmers"][at[f"seamN{b}"]] == 3 * T + 17 - K
    assert v["onmers"][at["allN300"]] == 0 and np.isnan(v["d"][at["allN300"]]) and np.isnan(v["d"][at["none"]])
    assert v["hist"][at["revcomp400"], 1].sum() > 0
    if th == 0:  # one strand matched, the other did not: it is minimised all the same, on an empty histogram
        i = at["one_strand"]
        assert v["hist"][i, 0].sum() > 0 and v["hist"][i, 1].sum() == 0
        assert 0 < v["d_strand"][i, 0] < v["d_strand"][i, 1] <= 0.5 and v["d"][i] == v["d_strand"][i, 0]


def test_long_reads_fill_32_bit_counters(sketches):
    """70,000 exact genome bases (onmers above 65,535: 274 units), and 790,000 (bin 0 above 65,535: the sketch keeps one k-mer in
    eight -- window minimizers of half the residues -- so that is what it takes)"""
    sk = sketches["AL"]
    g = sk.genome[0]
    reads = [g[1000:71000], g[5000:795000], sc.revcomp(g[100000:140000]), g[10:160]]
    names = ["exact70000", "exact790000", "rc40000", "short"]
    brute = sc.brute_hist_np(sk.po, reads, 16)
    v = check_all(sk, 4, names, reads, brute)
    assert v["onmers"][0] == 70000 - K + 1 > 65535
    assert v["hist"][1, 0, 0] > 65535 and v["onmers"][1] == 790000 - K + 1
    assert v["hist"][2, 1, 0] > 255


@pytest.mark.parametrize("th", [1, 4])
def test_sketch_b_long_buckets(sketches, th):
    sk = sketches["B"]
    lens = np.diff(np.concatenate([[0], sk.po.inc.astype(np.int64)]))
    assert sk.po.nrows == 32 and lens.max() > 64 and 40 < lens.mean() < 55
    names, reads = reads_b(sk.genome, th)
    n2, r2 = reads_at_threshold(sk, th)
    names, reads = names + n2, reads + r2
    brute = sc.brute_hist_np(sk.po, reads, 16)
    literal = (np.arange(0, len(reads), 3), sc.brute_hist(sk.po, reads[::3], 16))
    v = check_all(sk, th, names, reads, brute, literal)
    # single k-mers th and th + 1 substitutions away from an entry of their bucket: counted at th or nearer, and (some of them) not at all
    single = v["hist"][len(reads) - len(r2):, 0]
    assert single[0::2].sum(axis=1).tolist() == [1] * len(single[0::2])
    assert (brute[0][len(reads) - len(r2):, 0, :th + 1][1::2].sum(axis=1) == 0).any()
    assert (single[0::2, th] == 1).any()


@pytest.mark.parametrize("th", [0, 4])
def test_sketch_c_one_residue_of_three(sketches, th):
    sk = sketches["C"]
    assert (sk.po.m, sk.po.r, sk.po.frac) == (3, 0, 0)
    rng = np.random.default_rng(10)
    g = sk.genome[0]
    reads = [sc.mutate(rng, g[p:p + 200], rate) for p, rate in zip(range(0, 8000, 400), (0.0, 0.02, 0.06) * 7)]
    reads = [sc.revcomp(s) if i % 2 else s for i, s in enumerate(reads)] + [sc.random_dna(rng, 150)]
    names = [f"c{i}" for i in range(len(reads))]
    brute = sc.brute_hist_np(sk.po, reads, 16)
    literal = (np.arange(0, len(reads), 4), sc.brute_hist(sk.po, reads[::4], 16))
    v = check_all(sk, th, names, reads, brute, literal)
    assert (v["hist"].sum(axis=(1, 2)) > 0).sum() >= 10


# ---------------------------------------------------------------------------------------------------------------------------------
# interfaces
# ---------------------------------------------------------------------------------------------------------------------------------
def ids_1_7_200(n):
    return [("x", "read_%02d" % (i % 100), "L" * 196 + "%04d" % i)[i % 3] for i in range(n)]


@pytest.fixture(scope="module")
def text_a(sketches, batch_a):
    """sketch A's batch under ids of 1, 7 and 200 bytes: the old path's text and the oracle's"""
    sk = sketches["A"]
    _, reads, _, _ = batch_a
    names = ids_1_7_200(len(reads))
    bases, offs = sc.pack(reads)
    _, _, otext = old_path(sk, 4, names, reads)
    want = sk.po.seek(bases, offs, names, hdist_th=4)["text"]
    assert otext == want and {len(n) for n in names} == {1, 7, 200}
    return names, reads, bases, offs, want


def test_text_with_short_and_long_ids(sketches, text_a):
    names, reads, bases, offs, want = text_a
    _, text = new_path(sketches["A"], 4, names, reads)
    assert text == want
    assert text.count("\tNaN\n") >= 20 and len(text.splitlines()) == len(reads)


@pytest.mark.parametrize("which", ["ids", "text"])
def test_a_buffer_one_byte_too_small(capi, sketches, text_a, which):
    """KR_ERR_CAPACITY, and the same stream then serves the batch in two halves with the same bytes"""
    names, reads, bases, offs, want = text_a
    sk = sketches["A"]
    id_bytes = sum(len(n) + 1 for n in names)
    st = sk.dx.stream(params=capi.default_params(hdist_th=4), max_reads=len(reads), max_bases=len(bases))
    st.seek_enable(len(want) - (which == "text"), id_bytes - (which == "ids"))
    with pytest.raises(capi.KrError) as e:
        st.submit_text(bases, offs, names, capi.KR_SEEK)
        st.collect_text()
    assert e.value.code == capi.KR_ERR_CAPACITY
    h = len(reads) // 2
    got = b""
    for lo, hi in ((0, h), (h, len(reads))):
        b2, o2 = sc.pack(reads[lo:hi])
        st.submit_text(b2, o2, names[lo:hi], capi.KR_SEEK)
        got += st.collect_text()
    assert got.decode("latin-1") == want
    st.close()


@pytest.fixture(scope="module")
def raw_reads(sketches):
    g = sketches["AL"].genome[0]
    rng = np.random.default_rng(12)
    reads = [sc.mutate(rng, g[p:p + 150], 0.02) for p in range(0, 6000, 300)]
    reads.insert(7, g[20000:21200])
    reads.insert(13, sc.revcomp(g[30000:70000]))
    names = [f"r{i}" for i in range(len(reads))]
    return names, reads


@pytest.mark.parametrize("fmt", ["fastq", "fasta"])
def test_raw_bytes(capi, sketches, raw_reads, fmt):
    names, reads = raw_reads
    sk = sketches["AL"]
    bases, offs = sc.pack(reads)
    raw = sc.fastq_of(names, reads) if fmt == "fastq" else sc.fasta_of(names, reads)
    st = sk.dx.stream(params=capi.default_params(hdist_th=4), max_reads=4096, max_bases=len(bases) + 1024)
    st.seek_enable(1 << 16, 1 << 16)
    st.fastq_enable(len(raw) + 64)
    submit = st.submit_fastq if fmt == "fastq" else st.submit_fasta
    st.submit_text(bases, offs, names, capi.KR_SEEK)
    want = st.collect_text()
    vw = st.collect_seek()
    assert want.decode() == sk.po.seek(bases, offs, names, hdist_th=4)["text"]
    fp = submit(raw, capi.KR_SEEK | capi.KR_TILE_DEVICE)
    assert fp["nreads"] == len(reads) and fp["status"] == capi.KR_FASTQ_OK and fp["consumed"] == len(raw)
    assert st.collect_text() == want
    v = st.collect_seek()
    assert np.array_equal(v["hist"], vw["hist"]) and np.array_equal(v["onmers"], vw["onmers"]) and np.array_equal(v["d"], vw["d"], equal_nan=True)
    # without KR_TILE_DEVICE the record finder stops at the first record of more than 1,024 k-mer positions, as ever
    fp = submit(raw, capi.KR_SEEK)
    assert fp["nreads"] == 7 and fp["status"] == capi.KR_FASTQ_LONG
    assert st.collect_text() == b"".join(want.splitlines(keepends=True)[:7])
    # values only (no text buffers): the same counts, and no text to collect
    st2 = sk.dx.stream(params=capi.default_params(hdist_th=4), max_reads=4096, max_bases=len(bases) + 1024)
    st2.seek_enable()
    st2.fastq_enable(len(raw) + 64)
    fp = (st2.submit_fastq if fmt == "fastq" else st2.submit_fasta)(raw, capi.KR_SEEK | capi.KR_TILE_DEVICE)
    assert fp["nreads"] == len(reads)
    v2 = st2.collect_seek()
    assert np.array_equal(v2["hist"], vw["hist"]) and np.array_equal(v2["d"], vw["d"], equal_nan=True)
    with pytest.raises(capi.KrError) as e:
        st2.collect_text()
    assert e.value.code == capi.KR_ERR_STATE
    st.close(), st2.close()


def test_bases_in_each_location_and_consecutive_batches(capi, sketches, batch_a):
    import torch

    _, reads, _, _ = batch_a
    sk = sketches["A"]
    bases, offs = sc.pack(reads)
    n = len(reads)
    st = sk.dx.stream(params=capi.default_params(hdist_th=4), max_reads=n, max_bases=len(bases))
    st.seek_enable()
    lib = capi.load()

    def same(a, b):
        return all(np.array_equal(a[f], b[f], equal_nan=True) for f in ("d", "d_strand", "hist", "onmers")) and a["nreads"] == b["nreads"]

    st.submit(bases, offs, capi.KR_SEEK)
    host = st.collect_seek()
    assert host["hist"].sum() > 1000
    pb_, po_ = lib.kr_host_alloc(len(bases)), lib.kr_host_alloc(offs.nbytes)
    assert pb_ and po_
    C.memmove(pb_, bases.ctypes.data, len(bases)), C.memmove(po_, offs.ctypes.data, offs.nbytes)
    pb = np.ctypeslib.as_array(C.cast(pb_, C.POINTER(C.c_uint8)), shape=(len(bases),))
    po = np.ctypeslib.as_array(C.cast(po_, C.POINTER(C.c_uint64)), shape=(len(offs),))
    st.submit(pb, po, capi.KR_SEEK | capi.KR_BASES_PINNED)
    assert same(st.collect_seek(), host)
    tb, to = torch.from_numpy(bases.copy()).cuda(), torch.from_numpy(offs.view(np.int64).copy()).cuda()
    torch.cuda.synchronize()
    st.submit_device(tb.data_ptr(), to.data_ptr(), n, capi.KR_SEEK)
    assert same(st.collect_seek(), host)
    # a second, smaller batch: nothing of the first is left in the counters; a dist-style batch between two seek batches collects as ever
    h = n // 3
    b2, o2 = sc.pack(reads[n - h:])
    st.submit(b2, o2, capi.KR_SEEK)
    small = st.collect_seek()
    assert small["nreads"] == h and all(np.array_equal(small[f], host[f][n - h:], equal_nan=True) for f in ("d", "d_strand", "hist", "onmers"))
    st.submit(bases, offs, capi.KR_TAP_ACCS)
    res = st.collect()
    assert np.array_equal(sc.hist_of_taps(res, n, 4), host["hist"]) and np.array_equal(res.read_onmers, host["onmers"])
    with pytest.raises(capi.KrError) as e:
        st.collect_seek()  # the last batch was not a seek batch
    assert e.value.code == capi.KR_ERR_STATE
    st.submit(b2, o2, capi.KR_SEEK)
    assert same(st.collect_seek(), small)
    with pytest.raises(capi.KrError) as e:
        st.collect()  # ... and this one is
    assert e.value.code == capi.KR_ERR_STATE
    ms = st.seek_ms()
    assert len(ms) == 3 and all(x >= 0 for x in ms) and ms[0] > 0
    lib.kr_host_free(pb_), lib.kr_host_free(po_)
    st.close()


def test_flags_and_states(capi, sketches, toy_index_dir, batch_a):
    _, reads, _, _ = batch_a
    sk = sketches["A"]
    bases, offs = sc.pack(reads[:8])
    names = [f"n{i}" for i in range(8)]
    st = sk.dx.stream(params=capi.default_params(hdist_th=4), max_reads=64, max_bases=1 << 16)

    def code(f, *a):
        with pytest.raises(capi.KrError) as e:
            f(*a)
        return e.value.code

    assert code(st.submit, bases, offs, capi.KR_SEEK) == capi.KR_ERR_STATE  # not enabled
    st.seek_enable(1 << 16, 1 << 12)
    assert code(st.seek_enable) == capi.KR_ERR_STATE  # twice
    for bad in (capi.KR_TAP_ACCS, capi.KR_TAP_HITS, capi.KR_ROWS_ONLY, capi.KR_ROWS_ONLY | capi.KR_ROWS_INDEXED, capi.KR_TILE_ROWS, capi.KR_TILE_DEVICE):
        assert code(st.submit, bases, offs, capi.KR_SEEK | bad) == capi.KR_ERR_ARG, bad
        assert code(st.submit_text, bases, offs, names, capi.KR_SEEK | bad) == capi.KR_ERR_ARG, bad
    st.submit(bases, offs, capi.KR_SEEK)  # no ids: values, and no text
    st.wait()
    assert code(st.collect_text) == capi.KR_ERR_STATE
    assert st.collect_seek()["nreads"] == 8
    assert code(st.submit_text, bases, offs, names, 0) == capi.KR_ERR_STATE  # the dist text was never enabled on this stream
    st.close()
    # an index that is not a sketch
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    s2 = dx.stream(max_reads=64, max_bases=1 << 16)
    assert code(s2.seek_enable) == capi.KR_ERR_ARG
    assert code(s2.submit, bases, offs, capi.KR_SEEK) == capi.KR_ERR_ARG
    s2.close(), dx.close(), hx.close()


# ---------------------------------------------------------------------------------------------------------------------------------
# CLI
# ---------------------------------------------------------------------------------------------------------------------------------
def run_cli(sketch, q, extra, env=None):
    r = subprocess.run([EXE, "seek", "-i", sketch, "-q", str(q)] + extra, capture_output=True, env=dict(os.environ, KR_CLI_TIMING="1", **(env or {})), timeout=600)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    total = int(re.search(r"Total number of sequences queried: (\d+)", err).group(1))
    ms = re.search(r"\[timing\] gpu-seek: (\d+) reads through the seek kernels", err)
    mp = re.search(r"\[timing\] gpu-parse: (\d+) (FASTA|FASTQ) records found on the device", err)
    return r.stdout.split(b"\n", 1)[1], total, (int(ms.group(1)) if ms else None), (int(mp.group(1)) if mp else None)


@pytest.fixture(scope="module")
def cli_files(capi, synth, toy_genomes, tmp_path_factory):
    d = tmp_path_factory.mktemp("seekcli")
    bases, offs, names = synth.sample_reads(toy_genomes, 3000, seed=4)
    recs = b"".join(b"@%s extra\n%s\n+\n%s\n" % (names[i].encode(), bases[int(offs[i]):int(offs[i + 1])].tobytes(), b"F" * int(offs[i + 1] - offs[i])) for i in range(3000))
    (d / "clean.fq").write_bytes(recs)
    (d / "reads.fq.gz").write_bytes(gzip.compress(recs))
    g0 = next(iter(toy_genomes.values()))
    (d / "g0.fa").write_bytes(b">g0\n" + bytes(g0) + b"\n")
    capi.build_sketch(d / "g0.fa", d / "g0.skc")
    return {"clean": str(d / "clean.fq"), "gz": str(d / "reads.fq.gz"), "toy": os.path.join(GOLDEN, "toy_reads.fq"), "SKETCH": str(d / "g0.skc")}


@pytest.mark.parametrize("inp", ["clean", "toy", "gz"])
def test_cli_gpu_seek(cli_files, inp):
    """the stdout bytes after the invocation line are those of `krepp seek` without the flag"""
    want, total, none, _ = run_cli(cli_files["SKETCH"], cli_files[inp], [])
    assert none is None and total > 0 and len(want) > 100 and b"\tNaN\n" in want and re.search(rb"\t0\.\d{5}\n", want)
    got, t1, seek1, parse1 = run_cli(cli_files["SKETCH"], cli_files[inp], ["--gpu-seek"])
    assert got == want and t1 == total and seek1 == total and parse1 is None
    got, t2, seek2, parse2 = run_cli(cli_files["SKETCH"], cli_files[inp], ["--gpu-parse", "--gpu-seek"], {"KR_CLI_PARSE_CHUNK": "100000"})
    assert got == want and t2 == total and seek2 == total
    if inp == "gz":
        assert parse2 is None  # the host reader plus the seek kernels
    else:
        assert parse2 == total  # (toy: the 1,200-base record no longer stops the record finder)
