"""Report text deflated into BGZF members on the GPU (csrc/kr_dev_deflate.inc; kr_stream_bgzf_out_enable, kr_batch_collect_text_bgzf,
kr_debug_bgzf_deflate) and `krepp dist|place|seek --bgzf-out`.  The kernel runs the encoder the host runs (csrc/kr_deflate.h), so its
bytes must EQUAL kr_bgzf_deflate_host's for every input: that equality is the main test, and whatever the host form's output
satisfies (test_bgzf_deflate_host.py) the device's then does.  Nothing is compared with a tolerance."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import deflate_cases as dc
import seek_craft as sc
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")


@pytest.fixture(scope="module")
def toy(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    yield hx, dx
    dx.close()
    hx.close()


@pytest.fixture(scope="module")
def deflater(capi, toy):
    """a stream whose only use is kr_debug_bgzf_deflate / kr_debug_bgzf_inflate"""
    hx, dx = toy
    st = dx.stream(max_reads=64, max_bases=1 << 16)
    st.text_enable(hx, 1 << 16, 1 << 12)
    st.bgzf_out_enable()
    st.fastq_enable(1 << 20)
    st.bgzf_enable(1 << 20)
    yield st
    st.close()


def more_cases():
    rng = np.random.default_rng(77)
    text = dc.report_text(600)
    nine = text[:9 * dc.MEMBER - 1000]  # three workgroups, the last one part empty
    mixed = (text[:100000] + rng.integers(0, 256, 70000, dtype=np.uint8).tobytes() + b"a" * 66000 + dc.distinct(40000, 3) + text[:60000])[:5 * dc.MEMBER + 7]
    assert len(mixed) == 5 * dc.MEMBER + 7 and -(-len(nine) // dc.MEMBER) == 9
    return {"nine_members": nine, "mixed_5_members_and_7": mixed}


ALL = {**dc.cases(), **more_cases()}


@pytest.mark.parametrize("name", sorted(ALL))
def test_the_device_gives_the_hosts_bytes(capi, deflater, name):
    data = ALL[name]
    want = capi.bgzf_deflate_host(data)
    got = deflater.bgzf_deflate(data)
    assert len(got) == len(want) and got == want
    dc.check_stream(capi, data, got)


def test_round_trip_through_both_kernels(capi, deflater):
    data = ALL["nine_members"]
    comp = deflater.bgzf_deflate(data)
    assert len(dc.members_of(capi, comp)) == 9
    assert deflater.bgzf_inflate(comp) == data
    with pytest.raises(capi.KrError) as e:
        deflater.bgzf_deflate(data, cap=len(comp) - 1)
    assert e.value.code == capi.KR_ERR_CAPACITY
    assert deflater.bgzf_deflate(data) == comp
    assert deflater.bgzf_deflate_ms() == -1.0  # the first call makes the events
    deflater.bgzf_deflate(data)
    assert deflater.bgzf_deflate_ms() > 0


@pytest.fixture(scope="module")
def reads(capi, synth, toy_genomes):
    """the toy reads (long sequences among them) and 3,000 synthetic reads"""
    n1, b1, o1 = capi.read_fastx(os.path.join(GOLDEN, "toy_reads.fq"))
    b2, o2, n2 = synth.sample_reads(toy_genomes, 3000, seed=5)
    bases = np.concatenate([b1, b2])
    offs = np.concatenate([o1, o2[1:] + o1[-1]]).astype(np.uint64)
    return bases, offs, list(n1) + list(n2)


@pytest.mark.parametrize("mode", ["default", "no-multi"])
def test_dist_text(capi, toy, reads, mode):
    hx, dx = toy
    bases, offs, names = reads
    st = dx.stream(capi.default_params(multi=0) if mode == "no-multi" else None, max_reads=4 * len(names), max_bases=len(bases) + 64)
    st.text_enable(hx, 1 << 24, 1 << 20)
    st.submit_text(bases, offs, names, capi.KR_TILE_ROWS)
    with pytest.raises(capi.KrError) as e:
        st.collect_text_bgzf()
    assert e.value.code == capi.KR_ERR_STATE  # before kr_stream_bgzf_out_enable
    st.bgzf_out_enable()
    with pytest.raises(capi.KrError) as e:
        st.bgzf_out_enable()
    assert e.value.code == capi.KR_ERR_STATE
    comp, text_len = st.collect_text_bgzf()
    text = st.collect_text()  # the text is still where it was
    assert len(text) > dc.MEMBER and text_len == len(text)  # two members at least
    assert gzip.decompress(comp + capi.bgzf_eof()) == text
    assert comp == capi.bgzf_deflate_host(text)
    assert st.collect_text_bgzf() == (comp, text_len)
    # a second, smaller batch on the same stream
    n = 100
    st.submit_text(bases[:int(offs[n])], offs[:n + 1], names[:n], capi.KR_TILE_ROWS)
    comp2, tl2 = st.collect_text_bgzf()
    text2 = st.collect_text()
    assert 0 < tl2 == len(text2) < len(text) and comp2 == capi.bgzf_deflate_host(text2) and text.startswith(text2)
    st.close()


def test_seek_text(capi, tmp_path):
    g = [sc.random_dna(np.random.default_rng(21), 120000)]
    path = sc.write_sketch(capi, tmp_path, "s", g, sc.CFG_A)
    hx = capi.HostIndex(path, sketch=True)
    dx = hx.upload(0)
    rng = np.random.default_rng(12)
    seqs = [sc.mutate(rng, g[0][p:p + 150], 0.02) for p in range(0, 110000, 25)]
    names = ["read_number_%d" % i for i in range(len(seqs))]
    bases = np.frombuffer("".join(seqs).encode(), dtype=np.uint8)
    offs = np.concatenate([[0], np.cumsum([len(s) for s in seqs])]).astype(np.uint64)
    st = dx.stream(params=capi.default_params(hdist_th=4), max_reads=len(seqs), max_bases=len(bases) + 64)
    with pytest.raises(capi.KrError) as e:
        st.bgzf_out_enable()  # no text buffers yet
    assert e.value.code == capi.KR_ERR_STATE
    st.seek_enable(1 << 22, 1 << 20)
    st.bgzf_out_enable()
    st.submit_text(bases, offs, names, capi.KR_SEEK)
    comp, tl = st.collect_text_bgzf()
    text = st.collect_text()
    assert tl == len(text) > dc.MEMBER and comp == capi.bgzf_deflate_host(text) and gzip.decompress(comp + capi.bgzf_eof()) == text
    st.close(), dx.close(), hx.close()


def test_statuses_and_the_batches_behind_them(capi, toy, reads):
    hx, dx = toy
    bases, offs, names = reads
    n = 400  # the toy reads, with their long sequences, and some synthetic ones
    b, o, nm = bases[:int(offs[n])], offs[:n + 1], names[:n]
    tail = slice(int(offs[n]), int(offs[n + 300]))
    b3, o3, nm3 = bases[tail], offs[n:n + 301] - offs[n], names[n:n + 300]

    def later_batch_is_served(st):
        st.submit_text(b3, o3, nm3)
        comp, tl = st.collect_text_bgzf()
        text = st.collect_text()
        assert tl == len(text) > 0 and comp == capi.bgzf_deflate_host(text)

    # a tiled batch submitted without KR_TILE_ROWS left the device as record slots
    st = dx.stream(max_reads=4 * n, max_bases=len(b) + 64)
    st.text_enable(hx, 1 << 22, 1 << 18)
    st.bgzf_out_enable()
    st.submit_text(b, o, nm)
    for call in (st.collect_text_bgzf, st.collect_text):
        with pytest.raises(capi.KrError) as e:
            call()
        assert e.value.code == capi.KR_ERR_UNSUPPORTED
    later_batch_is_served(st)
    st.close()
    # a text buffer that is too small
    st = dx.stream(max_reads=4 * n, max_bases=len(b) + 64)
    st.text_enable(hx, 8192, 1 << 18)
    st.bgzf_out_enable()
    st.submit_text(b, o, nm, capi.KR_TILE_ROWS)
    for call in (st.collect_text_bgzf, st.collect_text):
        with pytest.raises(capi.KrError) as e:
            call()
        assert e.value.code == capi.KR_ERR_CAPACITY
    st.submit_text(b3[:int(o3[5])], o3[:6], nm3[:5])
    comp, tl = st.collect_text_bgzf()
    assert 0 < tl <= 8192 and comp == capi.bgzf_deflate_host(st.collect_text())
    st.close()
    # before kr_stream_bgzf_out_enable; no batch; a batch without ids
    st = dx.stream(max_reads=4 * n, max_bases=len(b) + 64)
    st.text_enable(hx, 1 << 22, 1 << 18)
    st.submit_text(b3, o3, nm3)
    with pytest.raises(capi.KrError) as e:
        st.collect_text_bgzf()
    assert e.value.code == capi.KR_ERR_STATE
    st.bgzf_out_enable()
    later_batch_is_served(st)
    st.submit(b3, o3, capi.KR_ROWS_ONLY)
    with pytest.raises(capi.KrError) as e:
        st.collect_text_bgzf()
    assert e.value.code == capi.KR_ERR_STATE
    later_batch_is_served(st)
    st.close()


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def cli(sub, idx, q, extra, env=None, out=None):
    """(the report's bytes, stderr): from the file -o names, else from stdout"""
    cmd = [EXE, sub, "-i", idx, "-q", str(q)] + extra + (["-o", str(out)] if out else [])
    r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, KR_CLI_TIMING="1", **(env or {})), timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    if out:
        assert r.stdout == b""
    return (open(out, "rb").read() if out else r.stdout), r.stderr.decode()


def same_report(sub, extra, plain, inflated):
    """equal but for the invocation, which names the flags and the output file"""
    if sub == "place" and "--tabular" not in extra and "--summarize" not in extra:
        strip = lambda t: re.sub(rb'"invocation"\s*:\s*"[^"]*"', b'"invocation": ""', t)
    else:
        strip = lambda t: t.split(b"\n", 1)[1]
        assert plain.split(b"\n", 1)[0].startswith(b"# software: krepp") and inflated.split(b"\n", 1)[0].startswith(b"# software: krepp")
    assert strip(inflated) == strip(plain) and len(strip(plain)) > 100


@pytest.fixture(scope="module")
def files(synth, toy_genomes, tmp_path_factory, capi):
    d = tmp_path_factory.mktemp("bgzf_out")
    bases, offs, names = synth.sample_reads(toy_genomes, 3000, seed=4)
    recs = []
    for i in range(3000):
        s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
        recs.append(b"@%s extra\n%s\n+\n%s\n" % (names[i].encode(), s, b"F" * len(s)))
    g0 = bytes(next(iter(toy_genomes.values())))
    long_read = g0[1000:9000]
    (d / "clean.fq").write_bytes(b"".join(recs))
    (d / "long.fq").write_bytes(b"".join(recs[:50]) + b"@contig\n%s\n+\n%s\n" % (long_read, b"F" * len(long_read)) + b"".join(recs[50:90]))
    (d / "g0.fa").write_bytes(b">g0\n" + g0 + b"\n")
    capi.build_sketch(d / "g0.fa", d / "g0.skc")
    return {"clean": str(d / "clean.fq"), "long": str(d / "long.fq"), "SKETCH": str(d / "g0.skc")}


CLI_CASES = {
    "dist": ("dist", "clean", [], {}, "dev"),
    "dist-gpu-parse": ("dist", "clean", ["--gpu-parse"], {"KR_CLI_PARSE_CHUNK": "100000"}, "dev"),
    "dist-summarize": ("dist", "clean", ["--summarize"], {}, "host"),
    "dist-many-batches": ("dist", "clean", [], {"KR_CLI_BATCH_READS": "700"}, "dev"),
    "seek-gpu-seek": ("seek", "clean", ["--gpu-seek"], {}, "dev"),
    "seek-host": ("seek", "clean", [], {}, "host"),
    "place-jplace": ("place", "clean", [], {"KR_CLI_BATCH_READS": "1000"}, "host"),
    "place-tabular": ("place", "clean", ["--tabular"], {}, "host"),
    "long-read": ("dist", "long", [], {}, "dev"),
    "long-read-host-formatter": ("dist", "long", [], {"KR_CLI_HOST_TEXT": "1"}, "host"),
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_output_inflates_to_the_plain_output(capi, toy_index_dir, files, tmp_path, case):
    sub, q, extra, env, where = CLI_CASES[case]
    idx = files["SKETCH"] if sub == "seek" else toy_index_dir
    plain, _ = cli(sub, idx, files[q], extra, env, out=tmp_path / "plain.out")
    comp, err = cli(sub, idx, files[q], extra + ["--bgzf-out"], env, out=tmp_path / "report.gz")
    same_report(sub, extra, plain, gzip.decompress(comp))
    assert comp.endswith(dc.EOF_MEMBER) and comp.count(dc.EOF_MEMBER) == 1
    k, cb, u = capi.bgzf_walk(comp, 1 << 40)  # our own reader walks it: whole members to the end
    assert cb == len(comp) and u == len(gzip.decompress(comp)) and k >= 2
    m = re.search(r"\[timing\] bgzf-out: (\d+) text bytes, (\d+) compressed bytes \(without the end member\); (\d+) pieces deflated on the device, (\d+) by the host encoder", err)
    assert m, err
    text_bytes, comp_bytes, dev, host = map(int, m.groups())
    assert text_bytes == u and comp_bytes == len(comp) - 28 < text_bytes
    assert host >= 1 and ((dev >= 1) if where == "dev" else (dev == 0)), (dev, host)  # (the header line is the host's always)


def test_cli_to_a_pipe(toy_index_dir, files, tmp_path):
    plain, _ = cli("dist", toy_index_dir, files["clean"], [])
    comp, _ = cli("dist", toy_index_dir, files["clean"], ["--bgzf-out"])
    same_report("dist", [], plain, gzip.decompress(comp))
    assert comp.endswith(dc.EOF_MEMBER)


def test_the_flag_is_in_the_usage_text():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("--bgzf-out") >= 3  # dist, place, seek
