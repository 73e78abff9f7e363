"""KR_TILE_ROWS: a batch that runs as tiles (long sequences; krepp_amd/csrc/kr_dev_tiles.inc) leaves the device as compact rows and,
on a stream with text enabled, as report text written by the device -- through a host batch, a batch in HBM tiled by kernels and raw
FASTQ bytes.  The yardstick is always the SAME batch submitted WITHOUT the flag: record slots copied back and formatted by
kr_format_dist, the only path such a batch had before the flag.  Rows are compared with ==, text byte for byte."""
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_rows_close, rows_of_oracle

pytestmark = pytest.mark.gpu

K = 21
LONG = 1024 + K  # bases from which a sequence has more than 1,024 k-mer positions (1,045)


# ---- helpers copied from tests/test_gpu_device_tiles.py (the same batches, so that the two files' results can be compared)
LENGTHS = (0, 20, 149, 150, 1043, 1044, 1045, 1172, 1173, 3000, 5000, 12345, 20000)
EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")


def make_seqs(g, lengths, seed):
    rng = np.random.default_rng(seed)
    names_g = list(g)
    seqs = []
    for L in lengths:
        name = names_g[int(rng.integers(0, len(names_g)))]
        o = int(rng.integers(0, 20000 - L + 1))
        s = bytearray(g[name][o:o + L].tobytes())
        for _ in range(L // 40):  # substitutions and the odd N
            s[int(rng.integers(0, L))] = b"ACGTN"[int(rng.integers(0, 5))]
        if L == 12345:  # a run of N across a tile boundary (1280 = 10 * 128), and a long stretch from another genome
            s[1270:1300] = b"N" * 30
            other = g[names_g[(names_g.index(name) + 7) % len(names_g)]]
            s[6000:9000] = other[100:3100].tobytes()
        seqs.append(bytes(s))
    return seqs


def as_batch(seqs):
    bases = np.frombuffer(b"".join(seqs), np.uint8)
    offs = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
    return bases, offs, [f"q{i}_L{len(s)}" for i, s in enumerate(seqs)]


class DeviceBatch:
    """bases and offsets as torch tensors on the GPU; the bases tensor ends exactly at offsets[nreads]"""

    def __init__(self, bases, offs, pad=0):
        import torch

        buf = np.concatenate([np.full(pad, ord("A"), np.uint8), bases])  # (a pad of valid bases: reading it would change results)
        self.bases = torch.from_numpy(buf.copy()).to("cuda:0")
        self.offs = torch.from_numpy((offs + np.uint64(pad)).astype(np.uint64).view(np.int64).copy()).to("cuda:0")
        torch.cuda.synchronize()
        assert self.bases.numel() == int(offs[-1]) + pad
        self.n = len(offs) - 1

    def submit(self, st, flags):
        st.submit_device(self.bases.data_ptr(), self.offs.data_ptr(), self.n, flags)


def accs_of(res):
    return sorted(zip(res.rec_read.tolist(), res.rec_key.tolist(), [tuple(x) for x in res.rec_hist.tolist()]))


def fastq_of(seqs, names):
    return b"".join(b"@" + nm.encode() + b" some comment\n" + s + b"\n+\n" + b"F" * len(s) + b"\n" for nm, s in zip(names, seqs))


def fuzz_batch(synth, gl, rng):
    seqs = []
    nseq = int(rng.integers(3, 40))
    for i in range(nseq):
        kind = int(rng.integers(0, 5)) if i + 1 < nseq else 4  # (one contig at least)
        if kind == 0:
            L = int(rng.integers(0, 300))
        elif kind == 1:
            L = int(rng.integers(1030, 1060))  # around 1,024 k-mer positions
        elif kind == 2:
            L = int(np.exp(rng.uniform(np.log(300), np.log(20000))))
        elif kind == 3:
            L = int(rng.integers(1, 20)) * 128 + int(rng.integers(18, 24))  # around multiples of the tile length
        else:
            L = int(rng.integers(2000, 8000))
        parts, left = [], L
        while left > 0:  # stretches of different references, either strand
            s = gl[int(rng.integers(len(gl)))]
            m = min(left, int(rng.integers(1, 20000)))
            p = int(rng.integers(0, len(s) - m + 1))
            c = s[p:p + m].copy()
            if rng.integers(0, 2):
                c = synth.COMP[c[::-1]]
            parts.append(c)
            left -= m
        r = np.concatenate(parts) if parts else np.zeros(0, np.uint8)
        if L:
            sub = rng.random(L) < rng.choice([0.0, 0.01, 0.05])
            r[sub] = rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(sub.sum()))
            for _ in range(int(rng.integers(0, 3))):  # N runs, some across tile boundaries
                a = int(rng.integers(0, L))
                r[a:min(L, a + int(rng.integers(1, 200)))] = ord("N")
        seqs.append(r.tobytes())
    return seqs


@pytest.fixture(scope="module")
def toy(capi, po, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    return hx, hx.upload(0), po.Index(toy_index_dir)


def new_stream(capi, hx, dx, nbases, max_reads=4096, text_bytes=1 << 22, **pkw):
    st = dx.stream(params=capi.default_params(**pkw), max_reads=max_reads, max_bases=nbases + 64, max_records=1 << 20)
    st.text_enable(hx, text_bytes, 1 << 18)
    return st


def unsupported(capi, st):
    with pytest.raises(capi.KrError) as e:
        st.collect_text()
    assert e.value.code == capi.KR_ERR_UNSUPPORTED


def plain(capi, hx, dx, bases, offs, names, max_reads=4096, **pkw):
    """The batch without the flag: it is tiled, collect_text refuses, the record slots come back and the host formats them."""
    st = new_stream(capi, hx, dx, len(bases), max_reads, **pkw)
    st.submit_text(bases, offs, names)
    assert st.tile_layout(len(names))["nv"] > 0
    unsupported(capi, st)
    res = st.collect()
    out = dict(rows=res.rows(), text=st.format_dist(hx, names).encode(), d2h=st.last_d2h_bytes(), na=res.read_na.copy(), cnt=res.read_cnt.copy())
    st.close()
    return out


def long_mask(offs):
    return np.diff(offs.astype(np.int64)) >= LONG


def has_both_kinds_of_long_reads(want, offs):
    lm = long_mask(offs)
    return bool(np.any(lm & (want["na"] == 1))) and bool(np.any(lm & (want["cnt"] > 1)))


@pytest.fixture(scope="module")
def base(capi, po, toy, toy_genomes):
    """A 3,000-base contig in front, the lengths around the threshold, an all-N contig (tiled, keeps nothing) and a 5,000-base contig
    last; the unflagged run's answer and the oracle's rows."""
    hx, dx, ox = toy
    rng = np.random.default_rng(99)
    rand = lambda L: np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes()
    seqs = [rand(3000)] + make_seqs(toy_genomes, LENGTHS, 5) + [b"N" * 2000, rand(5000)]
    bases, offs, names = as_batch(seqs)
    want = plain(capi, hx, dx, bases, offs, names)
    assert has_both_kinds_of_long_reads(want, offs)
    assert want["na"][0] == 0 and want["na"][-1] == 0 and want["na"][-2] == 1  # (the random contigs keep rows, the N contig none)
    oracle = rows_of_oracle(ox.dist(bases, offs, names, po.params(collect=0)))
    return dict(seqs=seqs, bases=bases, offs=offs, names=names, want=want, oracle=oracle)


def flagged_text_and_rows(capi, hx, dx, bases, offs, names, max_reads=4096, extra=0, **pkw):
    st = new_stream(capi, hx, dx, len(bases), max_reads, **pkw)
    st.submit_text(bases, offs, names, flags=capi.KR_TILE_ROWS | extra)
    lay = st.tile_layout(len(names))
    text = st.collect_text()
    res = st.collect()
    st.close()
    return text, res, lay


def test_rows_of_a_tiled_host_batch(capi, toy, base):
    hx, dx, ox = toy
    bases, offs, names, want = base["bases"], base["offs"], base["names"], base["want"]
    n = len(names)
    for extra in (0, capi.KR_ROWS_INDEXED):
        st = dx.stream(params=capi.default_params(), max_reads=4096, max_bases=len(bases) + 64, max_records=1 << 20)
        st.submit(bases, offs, capi.KR_ROWS_ONLY | capi.KR_TILE_ROWS | extra)
        assert st.tile_layout(n)["nv"] > n
        res = st.collect()
        assert res.rows() == want["rows"]  # bit for bit
        assert_rows_close(res.rows(), base["oracle"])
        assert res.nreads == n and res.nrecs == res.nrows == len(want["rows"]) and np.all(res.rec_sel == 1)
        assert res.rec_dix is None and not st._rv.rec_dix
        assert res.read_na.tolist() == want["na"].tolist()
        assert int(res.read_cnt.sum()) == res.nrows
        d2h = st.last_d2h_bytes()
        print(f"D2H bytes: {d2h} as rows, {want['d2h']} as record slots ({n} reads, {res.nrows} rows)")
        assert d2h == 9 * n + 12 * res.nrows and d2h < want["d2h"]
        st.close()


def test_text_three_ways_in(capi, toy, base):
    hx, dx, ox = toy
    bases, offs, names, want = base["bases"], base["offs"], base["names"], base["want"]
    n = len(names)
    # ---- the host batch
    text, res, lay = flagged_text_and_rows(capi, hx, dx, bases, offs, names)
    assert lay["nv"] > n and text == want["text"] and res.rows() == want["rows"]
    assert b"_L2000\tNA\tNaN\n" in text  # (the long sequence that keeps nothing)
    # ---- the same batch in HBM, tiled by kernels
    db = DeviceBatch(bases, offs)
    st = new_stream(capi, hx, dx, len(bases))
    st.submit_text_device(db.bases.data_ptr(), db.offs.data_ptr(), db.n, names, capi.KR_TILE_DEVICE)  # without the flag: as ever
    assert st.tile_layout(n)["nv"] > n
    unsupported(capi, st)
    assert st.collect().rows() == want["rows"]
    st.submit_text_device(db.bases.data_ptr(), db.offs.data_ptr(), db.n, names, capi.KR_TILE_DEVICE | capi.KR_TILE_ROWS)
    assert st.tile_layout(n)["nv"] > n
    assert st.collect_text() == want["text"]
    assert st.collect().rows() == want["rows"]
    st.close()
    # ---- raw FASTQ bytes, records and ids found on the device (N -> A: the record finder's batch is another one, with its own yardstick)
    seqs = [s.replace(b"N", b"A") for s in base["seqs"]]
    raw = fastq_of(seqs, names)
    st = new_stream(capi, hx, dx, len(bases))
    st.fastq_enable(len(raw))
    s = st.submit_fastq(raw, capi.KR_TILE_DEVICE)
    assert (s["status"], s["nreads"]) == (capi.KR_FASTQ_OK, n) and st.tile_layout(n)["nv"] > n
    unsupported(capi, st)
    fres = st.collect()
    fq_rows, fq_text = fres.rows(), st.format_dist(hx, st.fastq_names()).encode()
    assert np.any(long_mask(offs) & (fres.read_na == 1)) and np.any(long_mask(offs) & (fres.read_cnt > 1))
    s = st.submit_fastq(raw, capi.KR_TILE_DEVICE | capi.KR_TILE_ROWS)
    assert (s["status"], s["nreads"]) == (capi.KR_FASTQ_OK, n) and st.tile_layout(n)["nv"] > n
    assert st.collect_text() == fq_text
    assert st.collect().rows() == fq_rows
    st.close()


def test_text_in_every_report_mode(capi, toy, base):
    hx, dx, ox = toy
    bases, offs, names = base["bases"], base["offs"], base["names"]
    # a dist_max between the smallest and the largest DIST of the long sequence with the most rows: it drops some of its rows
    by_read = {}
    for r, se, d in base["want"]["rows"]:
        by_read.setdefault(r, []).append(d)
    lm = long_mask(offs)
    r_top = max((r for r in by_read if lm[r]), key=lambda r: len(by_read[r]))
    dmax = (min(by_read[r_top]) + max(by_read[r_top])) / 2
    assert min(by_read[r_top]) < dmax < max(by_read[r_top])
    for pkw in (dict(), dict(multi=0), dict(no_filter=0), dict(dist_max=dmax)):
        want = plain(capi, hx, dx, bases, offs, names, **pkw)
        assert has_both_kinds_of_long_reads(want, offs), pkw
        if "dist_max" in pkw:
            kept = sum(1 for r, se, d in want["rows"] if r == r_top)
            assert 0 < kept < len(by_read[r_top])
        text, res, lay = flagged_text_and_rows(capi, hx, dx, bases, offs, names, **pkw)
        assert lay["nv"] > 0 and text == want["text"] and res.rows() == want["rows"], pkw


def block_edge_batches(synth, toy_genomes):
    """(a) 901 caller's reads in one block of 1,024, the tiled batch in two; (b) the caller's reads in two blocks, and the shift
    between a read and its first tile changes inside the second."""
    def short(n, seed):
        rb, ro, _ = synth.sample_reads(toy_genomes, n, seed=seed)
        assert int(ro[-1]) == 150 * n
        return [rb[int(ro[i]):int(ro[i + 1])].tobytes() for i in range(n)]

    c3000, c5000, c20000 = make_seqs(toy_genomes, (3000, 5000, 20000), 11)
    a = short(900, 21)
    a.insert(450, c20000)
    b = short(1100, 22)
    b.insert(0, c3000)
    b.insert(1050, c5000)
    return {"a": a, "b": b}


@pytest.mark.parametrize("which", ["a", "b"])
def test_block_edges(capi, synth, toy, toy_genomes, which):
    hx, dx, ox = toy
    seqs = block_edge_batches(synth, toy_genomes)[which]
    bases, offs, names = as_batch(seqs)
    n = len(names)
    want = plain(capi, hx, dx, bases, offs, names)
    assert np.any(long_mask(offs) & (want["cnt"] > 1))
    text, res, lay = flagged_text_and_rows(capi, hx, dx, bases, offs, names)
    extra = sum(capi.tile_shape(len(s), K)[1] - 1 for s in seqs if len(s) >= LONG)
    assert lay["nv"] == n + extra
    if which == "a":
        assert n == 901 and n <= 1024 < lay["nv"]
    else:
        assert n == 1102 and lay["rfirst"][1050] > 1050 > 1024 and len(seqs[1050]) == 5000
    assert text == want["text"] and res.rows() == want["rows"]
    assert res.nrecs == res.nrows and res.read_na.tolist() == want["na"].tolist()


@pytest.mark.parametrize("seed", [0, 1])
def test_every_tile_boundary_in_short_sequences(capi, synth, toy, toy_genomes, monkeypatch, seed):
    hx, dx, ox = toy
    monkeypatch.setenv("KR_TILE_MIN_POS", "128")  # every sequence of more than one tile is tiled
    rng = np.random.default_rng(7000 + seed)
    bases, offs, names = as_batch(fuzz_batch(synth, list(toy_genomes.values()), rng))
    n, room = len(names), len(names) + len(bases) // 128 + 8
    monkeypatch.setenv("KR_NO_TILES", "1")
    st = new_stream(capi, hx, dx, len(bases), room)
    st.submit_text(bases, offs, names)
    assert st.tile_layout(n)["nv"] == 0
    want_text = st.collect_text()
    want_rows = st.collect().rows()
    st.close()
    monkeypatch.delenv("KR_NO_TILES")
    text, res, lay = flagged_text_and_rows(capi, hx, dx, bases, offs, names, max_reads=room)
    assert lay["nlong"] == int(np.sum(np.diff(offs.astype(np.int64)) >= 128 + K)) > 0
    assert text == want_text and res.rows() == want_rows


def test_capacity_and_rerun(capi, toy, base, monkeypatch):
    hx, dx, ox = toy
    bases, offs, names, want = base["bases"], base["offs"], base["names"], base["want"]
    n = len(names)
    # ---- a text buffer that holds either half of the batch's text, exactly, and not the whole
    per_read = [0] * n
    for line in want["text"].split(b"\n")[:-1]:
        per_read[names.index(line.split(b"\t", 1)[0].decode())] += len(line) + 1
    pre = np.cumsum([0] + per_read)
    m = int(np.argmin(np.abs(pre - pre[-1] / 2)))
    cap = int(max(pre[m], pre[-1] - pre[m]))
    assert 0 < m < n and cap < pre[-1]
    st = new_stream(capi, hx, dx, len(bases), text_bytes=cap)
    st.submit_text(bases, offs, names, flags=capi.KR_TILE_ROWS)
    assert st.tile_layout(n)["nv"] > 0
    with pytest.raises(capi.KrError) as e:
        st.collect_text()
    assert e.value.code == capi.KR_ERR_CAPACITY
    b0 = int(offs[m])
    st.submit_text(bases[:b0], offs[:m + 1], names[:m], flags=capi.KR_TILE_ROWS)
    assert st.tile_layout(m)["nv"] > 0
    first = st.collect_text()
    st.submit_text(bases[b0:], offs[m:] - offs[m], names[m:], flags=capi.KR_TILE_ROWS)
    assert st.tile_layout(n - m)["nv"] > 0
    assert first + st.collect_text() == want["text"]
    st.close()
    # ---- the tiles' records "do not fit": the untiled rerun is a text batch with the flag as without
    monkeypatch.setenv("KR_DEBUG_TILE_OVERFLOW", "1")
    st = new_stream(capi, hx, dx, len(bases))
    st.submit_text(bases, offs, names, flags=capi.KR_TILE_ROWS)
    assert st.tile_layout(n)["nv"] > 0
    assert st.collect_text() == want["text"]
    assert st.tile_layout(n)["nv"] == 0  # (it ran again as it is)
    assert st.collect().rows() == want["rows"]
    monkeypatch.delenv("KR_DEBUG_TILE_OVERFLOW")
    st.submit_text(bases, offs, names, flags=capi.KR_TILE_ROWS)  # and the stream is as good as new
    assert st.tile_layout(n)["nv"] > 0 and st.collect_text() == want["text"]
    st.close()
    # ---- no room for a single tile: the batch is not tiled, with the flag as without
    for fl in (0, capi.KR_TILE_ROWS):
        st = new_stream(capi, hx, dx, len(bases), max_reads=n)
        st.submit_text(bases, offs, names, flags=fl)
        assert st.tile_layout(n)["nv"] == 0
        assert st.collect_text() == want["text"]
        assert st.collect().rows() == want["rows"]
        st.close()


def test_the_flag_is_ignored_where_it_cannot_apply(capi, synth, toy, toy_genomes, base):
    hx, dx, ox = toy
    bases, offs, names = base["bases"], base["offs"], base["names"]
    n = len(names)
    got = []
    for fl in (0, capi.KR_TILE_ROWS):  # taps keep record slots
        st = dx.stream(params=capi.default_params(), max_reads=4096, max_bases=len(bases) + 64, max_records=1 << 20)
        st.submit(bases, offs, capi.KR_TAP_ACCS | fl)
        assert st.tile_layout(n)["nv"] > 0
        res = st.collect()
        got.append((accs_of(res), res.rows(), res.read_onmers.tolist()))
        st.close()
    assert got[0] == got[1] and got[0][1] == base["want"]["rows"]
    # a batch without a long sequence is not tiled: rows and text as ever
    b2, o2, n2 = synth.sample_reads(toy_genomes, 1500, seed=3)
    got = []
    for fl in (0, capi.KR_TILE_ROWS):
        st = new_stream(capi, hx, dx, len(b2))
        st.submit_text(b2, o2, n2, flags=fl)
        assert st.tile_layout(len(n2))["nv"] == 0
        text = st.collect_text()
        res = st.collect()
        got.append((text, res.rows(), res.nrecs, st.last_d2h_bytes()))
        st.close()
    assert got[0] == got[1] and len(got[0][1]) > 0


def cli_dist(idx, q, extra, env=None):
    r = subprocess.run([EXE, "dist", "-i", idx, "-q", str(q)] + extra, capture_output=True,
                       env=dict(os.environ, KR_CLI_TIMING="1", **(env or {})), timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    m = re.search(r"\[timing\] report text: (\d+) batches written from device text, (\d+) through the host formatter", r.stderr.decode())
    assert m, r.stderr.decode()
    return r.stdout.split(b"\n", 1)[1], int(m.group(1)), int(m.group(2))  # (the first line names the invocation)


def test_cli_writes_long_read_batches_from_device_text(toy_index_dir, toy_genomes, tmp_path):
    lens = [150] * 7 + [1045] + [150] * 9 + [5000] + [100, 149, 150] + [20000] + [150] * 4
    seqs = [s.replace(b"N", b"A") for s in make_seqs(toy_genomes, lens, 17)]
    q = tmp_path / "long.fq"
    q.write_bytes(fastq_of(seqs, [f"r{i}" for i in range(len(seqs))]))
    for extra in ([], ["--gpu-parse"]):
        want, dev0, host0 = cli_dist(toy_index_dir, q, extra, env={"KR_CLI_HOST_TEXT": "1"})
        assert dev0 == 0 and host0 >= 1 and want.count(b"\n") > len(seqs)
        got, dev, host = cli_dist(toy_index_dir, q, extra)
        assert got == want, extra
        assert host == 0 and dev >= 1, extra
