"""Long sequences of a batch that is ALREADY IN HBM, tiled on the device (KR_BASES_DEVICE | KR_TILE_DEVICE, kr_batch_submit_fastq with
KR_TILE_DEVICE; krepp_amd/csrc/kr_dev_tiles.inc, the kr_tile_lay_* kernels): the layout the kernels write is the one build_tiles
writes on the host, the results are those of the host-tiled batch, of the same device batch without the flag and of the oracle's
serial scan, bit for bit, and without the flag nothing is tiled.

The device tensors END exactly at offsets[nreads] (and, in the shifted variant, the bases start behind a pad of other bytes): a
kernel that reads a byte outside [bases + offsets[0], bases + offsets[nreads]) reads something that is not the batch's."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT, assert_rows_close, rows_of_oracle

pytestmark = pytest.mark.gpu

K = 21          # the toy index: 1,024 k-mer positions = 1,044 bases
SEG = 128
# every edge of the layout: empty, shorter than k, reads, just below / at / above the threshold, a last tile of one position (1173),
# contigs, one with an N run across a tile boundary, a whole genome
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


def shape(length, k=K):
    nkm = length - k + 1 if length >= k else 0
    nt = (nkm + SEG - 1) // SEG
    return nkm, nt, (length + (nt - 1) * (k - 1) if nt else length)


def expected_layout(bases, offs, spare, tile_min_pos=1024, k=K):
    """The tiled batch by the device's PREFIX rule, computed here: read r is tiled iff it is long and the tiles of the long sequences
    0 .. r add at most `spare` reads to the batch."""
    voff, vtile, rfirst, longs, out = [], [], [], [], []
    pos, added = 0, 0
    for r in range(len(offs) - 1):
        a, b = int(offs[r]), int(offs[r + 1])
        nkm, nt, _ = shape(b - a, k)
        rfirst.append(len(voff))
        long_ = nkm > tile_min_pos
        added += nt - 1 if long_ else 0
        if long_ and added <= spare:
            longs.append((len(voff), nt))
            for ti in range(nt):
                piece = bases[a + ti * SEG:min(b, a + ti * SEG + SEG + k - 1)]
                voff.append(pos), vtile.append(1), out.append(piece)
                pos += len(piece)
        else:
            voff.append(pos), vtile.append(0), out.append(bases[a:b])
            pos += b - a
    voff.append(pos)
    if not longs:
        return {"nv": 0, "nlong": 0}
    return {"nv": len(vtile), "nlong": len(longs), "voff": np.array(voff, np.uint64), "vtile": np.array(vtile, np.uint8),
            "rfirst": np.array(rfirst, np.uint32), "longs": np.array(longs, np.uint32).reshape(-1, 2), "bases": np.concatenate(out)}


def same_layout(a, b):
    assert (a["nv"], a["nlong"]) == (b["nv"], b["nlong"])
    for f in ("voff", "vtile", "rfirst", "longs", "bases"):
        if a["nv"]:
            assert np.array_equal(a[f], b[f]), f


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


def new_stream(capi, dx, nbases, max_reads=4096, **pkw):
    return dx.stream(params=capi.default_params(**pkw), max_reads=max_reads, max_bases=nbases + 64, max_records=1 << 20)


def run_host(capi, dx, bases, offs, flags=0, max_reads=4096, **pkw):
    st = new_stream(capi, dx, len(bases), max_reads, **pkw)
    st.submit(bases, offs, flags)
    lay = st.tile_layout(len(offs) - 1)
    return st, st.collect(), lay


def run_dev(capi, dx, db, nbases, flags=0, max_reads=4096, **pkw):
    st = new_stream(capi, dx, nbases, max_reads, **pkw)
    db.submit(st, flags)
    lay = st.tile_layout(db.n)
    return st, st.collect(), lay


@pytest.fixture(scope="module")
def toy(capi, po, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    return hx, hx.upload(0), po.Index(toy_index_dir)


@pytest.fixture(scope="module")
def mix(capi, po, toy, toy_genomes):
    """the batch, on the host and on the device (plain and with offsets[0] != 0), the oracle's answer and the host-tiled run's"""
    hx, dx, ox = toy
    bases, offs, names = as_batch(make_seqs(toy_genomes, LENGTHS, 5))
    ref = ox.dist(bases, offs, names, po.params(collect=7))
    acc = ref["accs"][ref["accs"]["passed"] == 1]
    want = sorted(zip(acc["read"].tolist(), ((acc["se"] << 1) | acc["strand"]).tolist(), [tuple(x[:5]) for x in acc["hist"].tolist()]))
    st, res, lay = run_host(capi, dx, bases, offs, capi.KR_TAP_ACCS)
    host = dict(accs=accs_of(res), rows=res.rows(), onmers=res.read_onmers.tolist(), taps=st.readtaps(len(names)).tolist(), lay=lay)
    st.close()
    return dict(bases=bases, offs=offs, names=names, ref=ref, want=want, host=host,
                dev=DeviceBatch(bases, offs), dev_shifted=DeviceBatch(bases, offs, pad=77))


def check_against_host(capi, st, res, mix):
    h = mix["host"]
    assert accs_of(res) == h["accs"] and res.rows() == h["rows"]  # bit for bit
    assert res.read_onmers.tolist() == h["onmers"] and st.readtaps(len(mix["names"])).tolist() == h["taps"]


@pytest.mark.parametrize("which", ["dev", "dev_shifted"])
def test_the_device_layout_equals_the_hosts(capi, toy, mix, which):
    hx, dx, ox = toy
    n = len(mix["names"])
    st, res, lay = run_dev(capi, dx, mix[which], len(mix["bases"]), capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE)
    assert lay["nv"] > n and lay["nlong"] == 7
    same_layout(lay, mix["host"]["lay"])
    same_layout(lay, expected_layout(mix["bases"], mix["offs"], 4096 - n))
    assert int(lay["voff"][-1]) == len(lay["bases"])
    st.close()


@pytest.mark.parametrize("which", ["dev", "dev_shifted"])
def test_results_equal_the_host_tiled_run_the_untiled_run_and_the_oracle(capi, po, toy, mix, which):
    hx, dx, ox = toy
    ref, nb = mix["ref"], len(mix["bases"])
    st, res, lay = run_dev(capi, dx, mix[which], nb, capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE)
    assert lay["nv"] > 0
    assert accs_of(res) == mix["want"], "histograms of device-tiled sequences differ from the oracle"
    assert res.read_onmers.tolist() == ref["reads"]["onmers"].tolist()
    assert st.readtaps(len(mix["names"])).tolist() == ref["reads"]["hdist_filt"].tolist()  # the sequence's minima, not a tile's
    assert_rows_close(res.rows(), rows_of_oracle(ref))
    check_against_host(capi, st, res, mix)
    st.close()
    # the same device batch without the flag: nothing is tiled (the default did not change), same results
    st0, res0, lay0 = run_dev(capi, dx, mix[which], nb, capi.KR_TAP_ACCS)
    assert lay0["nv"] == 0 and lay0["nlong"] == 0
    check_against_host(capi, st0, res0, mix)
    st0.close()
    # KR_TAP_HITS keeps the batch as it is
    st1 = new_stream(capi, dx, nb)
    mix[which].submit(st1, capi.KR_TAP_HITS | capi.KR_TILE_DEVICE)
    assert st1.tile_layout(mix[which].n)["nv"] == 0
    st1.collect()
    st1.close()


def test_rows_in_every_report_mode(capi, po, toy, mix):
    hx, dx, ox = toy
    bases, offs, names = mix["bases"], mix["offs"], mix["names"]
    for pkw in (dict(), dict(no_filter=0), dict(multi=0), dict(hdist_th=3), dict(dist_max=0.05)):
        want_rows = rows_of_oracle(ox.dist(bases, offs, names, po.params(collect=0, **pkw)))
        for fl in (0, capi.KR_ROWS_ONLY):
            st, r, lay = run_dev(capi, dx, mix["dev"], len(bases), fl | capi.KR_TILE_DEVICE, **pkw)
            assert lay["nv"] > 0
            assert_rows_close(r.rows(), want_rows)
            sth, rh, _ = run_host(capi, dx, bases, offs, fl, **pkw)
            assert r.rows() == rh.rows(), (pkw, fl)
            st.close(), sth.close()


def test_when_the_room_runs_out_a_prefix_of_the_long_sequences_is_tiled(capi, toy, toy_genomes, mix):
    hx, dx, ox = toy
    n, nb = len(mix["names"]), len(mix["bases"])
    # 1045, 1172 and 1173 bases are 9, 9 and 10 tiles: 8 + 8 reads more fit a spare of 20, the third sequence's 9 do not -- and
    # nothing behind it is tiled
    st, res, lay = run_dev(capi, dx, mix["dev"], nb, capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE, max_reads=n + 20)
    assert (lay["nv"], lay["nlong"]) == (n + 16, 2) and lay["longs"].tolist() == [[6, 9], [15, 9]]
    same_layout(lay, expected_layout(mix["bases"], mix["offs"], 20))
    check_against_host(capi, st, res, mix)
    st.close()
    st, res, lay = run_dev(capi, dx, mix["dev"], nb, capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE, max_reads=n + 16)  # exactly the room
    assert (lay["nv"], lay["nlong"]) == (n + 16, 2)
    check_against_host(capi, st, res, mix)
    st.close()
    st, res, lay = run_dev(capi, dx, mix["dev"], nb, capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE, max_reads=n)  # spare == 0
    assert lay["nv"] == 0
    check_against_host(capi, st, res, mix)
    st.close()
    # where the rules differ: the host, greedy, tiles the short sequence behind the one that does not fit; the device tiles none
    bases, offs, names = as_batch(make_seqs(toy_genomes, (5000, 1045, 150), 3))
    sth, rh, layh = run_host(capi, dx, bases, offs, capi.KR_TAP_ACCS, max_reads=3 + 10)
    assert layh["nlong"] == 1 and layh["longs"].tolist() == [[1, 9]]
    std, rd, layd = run_dev(capi, dx, DeviceBatch(bases, offs), len(bases), capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE, max_reads=3 + 10)
    assert layd["nv"] == 0
    assert accs_of(rd) == accs_of(rh) and rd.rows() == rh.rows()
    sth.close(), std.close()


def test_a_device_tiled_batch_that_overflows_is_run_again_untiled(capi, toy, mix, monkeypatch):
    """The rerun submits the caller's device pointers again (KR_DEBUG_TILE_OVERFLOW simulates the overflow)."""
    hx, dx, ox = toy
    monkeypatch.setenv("KR_DEBUG_TILE_OVERFLOW", "1")
    st = new_stream(capi, dx, len(mix["bases"]))
    mix["dev_shifted"].submit(st, capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE)
    assert st.tile_layout(mix["dev_shifted"].n)["nv"] > 0  # it was tiled ...
    res = st.collect()
    assert st.tile_layout(mix["dev_shifted"].n)["nv"] == 0  # ... and ran again as it is
    check_against_host(capi, st, res, mix)
    monkeypatch.delenv("KR_DEBUG_TILE_OVERFLOW")
    mix["dev_shifted"].submit(st, capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE)  # and the stream is as good as new
    assert st.tile_layout(mix["dev_shifted"].n)["nv"] > 0
    check_against_host(capi, st, st.collect(), mix)
    st.close()


def test_a_batch_without_a_long_sequence_is_submitted_as_it_is(capi, synth, toy, toy_genomes):
    hx, dx, ox = toy
    bases, offs, names = synth.sample_reads(toy_genomes, 3000, seed=2)  # 150-bp reads, three blocks of the layout passes
    db = DeviceBatch(bases, offs)
    st, res, lay = run_dev(capi, dx, db, len(bases), capi.KR_ROWS_ONLY | capi.KR_TILE_DEVICE)
    assert lay["nv"] == 0
    sth, rh, _ = run_host(capi, dx, bases, offs, capi.KR_ROWS_ONLY)
    assert res.rows() == rh.rows() and len(rh.rows()) > 0
    st.close(), sth.close()


def fastq_of(seqs, names):
    return b"".join(b"@" + nm.encode() + b" some comment\n" + s + b"\n+\n" + b"F" * len(s) + b"\n" for nm, s in zip(names, seqs))


def test_fastq_chunks_with_long_records_stay_on_the_device(capi, toy, toy_genomes, tmp_path):
    hx, dx, ox = toy
    lens = [150] * 7 + [1045] + [150] * 9 + [5000] + [100, 149, 150] + [20000] + [150] * 4
    seqs = [s.replace(b"N", b"A") for s in make_seqs(toy_genomes, lens, 17)]
    names = [f"r{i}" for i in range(len(seqs))]
    raw = fastq_of(seqs, names)
    n, nb = len(seqs), sum(lens)
    # the host reader + host batch path
    path = tmp_path / "long.fq"
    path.write_bytes(raw)
    hnames, hbases, hoffs = capi.read_fastx(str(path))
    assert hnames == names
    h = new_stream(capi, dx, nb)
    h.text_enable(hx, 1 << 22, 1 << 16)
    h.submit_text(hbases, hoffs, hnames)
    with pytest.raises(capi.KrError) as e:
        h.collect_text()
    assert e.value.code == capi.KR_ERR_UNSUPPORTED  # (tiled on the host)
    want_rows = h.collect().rows()
    want_text = h.format_dist(hx, hnames)
    assert len(want_rows) > n
    # raw bytes, with device text asked for
    a = new_stream(capi, dx, nb)
    a.text_enable(hx, 1 << 22, 1 << 16)
    a.fastq_enable(len(raw))
    s = a.submit_fastq(raw, capi.KR_TILE_DEVICE)
    assert (s["status"], s["nreads"], s["consumed"], s["nbases"]) == (capi.KR_FASTQ_OK, n, len(raw), nb)
    lay = a.tile_layout(n)
    assert lay["nlong"] == 3 and lay["nv"] == n + 8 + 38 + 156
    same_layout(lay, expected_layout(hbases, hoffs, 4096 - n))
    with pytest.raises(capi.KrError) as e:
        a.collect_text()
    assert e.value.code == capi.KR_ERR_UNSUPPORTED
    assert a.collect().rows() == want_rows
    assert a.fastq_names() == names
    assert a.format_dist(hx, a.fastq_names()) == want_text
    assert a.fastq_batch(s) == seqs  # the untiled bases and offsets
    # ... and without: rows
    c = new_stream(capi, dx, nb)
    c.fastq_enable(len(raw))
    s = c.submit_fastq(raw, capi.KR_ROWS_ONLY | capi.KR_TILE_DEVICE)
    assert (s["status"], s["nreads"]) == (capi.KR_FASTQ_OK, n) and c.tile_layout(n)["nlong"] == 3
    assert c.collect().rows() == want_rows
    # without the flag the first long record still ends the accepted prefix
    s = c.submit_fastq(raw, capi.KR_ROWS_ONLY)
    assert (s["status"], s["nreads"]) == (capi.KR_FASTQ_LONG, 7)
    c.wait()
    for x in (h, a, c):
        x.close()


def test_place_on_a_device_tiled_batch(capi, toy, mix):
    hx, dx, ox = toy
    bases, offs, names = mix["bases"], mix["offs"], mix["names"]
    placer = capi.Placer(hx, None, 0, max_reads=4096, max_bases=len(bases) + 64)
    want, want_pl = placer.place(bases, offs, names)  # the host-tiled batch
    assert placer.st.tile_layout(len(names))["nv"] > 0 and len(want) > 0
    db = DeviceBatch(bases, offs)
    db.submit(placer.st, capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE)
    assert placer.st.tile_layout(len(names))["nv"] > 0
    placer.prev = C.c_int(0)
    arr = (C.c_char_p * len(names))(*[x.encode() for x in names])
    txt, ln, pls, npl = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_uint64()
    capi.check(placer.lib.kr_place_stream(placer.hx.h, placer.dx.h, placer.pt, placer.st.h, len(names), offs.ctypes.data, arr,
                                          C.byref(placer.popts), int(placer.tabular), C.byref(placer.prev), C.byref(txt), C.byref(ln),
                                          C.byref(pls), C.byref(npl)))
    got = C.string_at(txt, ln.value)
    got_pl = C.string_at(pls, npl.value * capi.PLACEMENT_DT.itemsize)
    placer.lib.kr_free(txt), placer.lib.kr_free(pls)
    assert got == want.encode() and got_pl == want_pl.tobytes()
    placer.close()


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


@pytest.mark.parametrize("seed,min_pos", [(0, None), (1, None), (2, "128"), (3, "128"), (4, "300")])
def test_fuzzed_mixes_device_tiled_against_untiled(capi, synth, toy, toy_genomes, monkeypatch, seed, min_pos):
    """Random mixes of reads and chimeric contigs on streams with room for all, some or none of the tiles; with KR_TILE_MIN_POS=128
    every sequence of more than one tile is tiled, so that short sequences carry many tile boundaries."""
    hx, dx, ox = toy
    rng = np.random.default_rng(4000 + seed)
    bases, offs, names = as_batch(fuzz_batch(synth, list(toy_genomes.values()), rng))
    n = len(names)
    db = DeviceBatch(bases, offs, pad=int(rng.integers(0, 50)))
    st0, r0, lay0 = run_dev(capi, dx, db, len(bases), capi.KR_TAP_ACCS, max_reads=n)  # untiled
    assert lay0["nv"] == 0
    want_accs, want_rows, want_taps = accs_of(r0), r0.rows(), st0.readtaps(n).tolist()
    st0.close()
    if min_pos:
        monkeypatch.setenv("KR_TILE_MIN_POS", min_pos)
    tmin = int(min_pos) if min_pos else 1024
    all_tiles = n + len(bases) // 128 + 8
    tiled_once = False
    for max_reads in (all_tiles, n + int(rng.integers(0, max(1, len(bases) // 128))), n):
        st, r, lay = run_dev(capi, dx, db, len(bases), capi.KR_TAP_ACCS | capi.KR_TILE_DEVICE, max_reads=max_reads)
        same_layout(lay, expected_layout(bases, offs, max_reads - n, tmin))
        tiled_once = tiled_once or lay["nv"] > 0
        assert accs_of(r) == want_accs and r.rows() == want_rows and st.readtaps(n).tolist() == want_taps, (seed, max_reads)
        st2, r2, _ = run_dev(capi, dx, db, len(bases), capi.KR_TILE_DEVICE, max_reads=max_reads)  # without the tap
        assert r2.rows() == want_rows
        st.close(), st2.close()
    assert tiled_once


def cli_dist(idx, q, extra, env=None):
    r = subprocess.run([EXE, "dist", "-i", idx, "-q", str(q)] + extra, capture_output=True, env=dict(os.environ, **(env or {})), timeout=300)
    assert r.returncode == 0, r.stderr.decode()
    total = [l for l in r.stderr.decode().splitlines() if l.startswith("Total number of sequences queried")]
    return r.stdout.split(b"\n", 1)[1], total  # (the first line names the invocation)


def test_cli_gpu_parse_with_long_records_scattered_through_the_file(toy_index_dir, toy_genomes, tmp_path):
    rng = np.random.default_rng(8)
    lens = [150] * 200
    for i, L in zip(rng.choice(200, 6, replace=False), (1045, 5000, 20000, 1173, 3000, 12345)):
        lens[int(i)] = L
    seqs = [s.replace(b"N", b"A") for s in make_seqs(toy_genomes, lens, 23)]
    q = tmp_path / "scattered.fq"
    q.write_bytes(fastq_of(seqs, [f"read{i}" for i in range(len(seqs))]))
    for extra in ([], ["--no-multi"]):
        want = cli_dist(toy_index_dir, q, extra)
        assert want[1] == ["Total number of sequences queried: 200"]
        assert cli_dist(toy_index_dir, q, extra + ["--gpu-parse"]) == want, extra
        assert cli_dist(toy_index_dir, q, extra + ["--gpu-parse"], env={"KR_CLI_PARSE_CHUNK": "60000"}) == want, extra
