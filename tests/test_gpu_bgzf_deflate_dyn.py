"""Level 2 of the BGZF encoder on the GPU (kr_bgzf_deflate_dyn_kernel in csrc/kr_dev_deflate.inc; kr_stream_bgzf_out_level) and
`krepp dist|place|seek --bgzf-out --bgzf-level 2`.  The kernel runs the encoder the host runs (csrc/kr_deflate.h, deflate_member_dyn),
so its bytes must EQUAL kr_bgzf_deflate_host_level's for every input; what the host form's output satisfies
(test_bgzf_deflate_dyn_host.py) the device's then does.  Nothing is compared with a tolerance."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import deflate_cases as dc
import deflate_dyn_cases as dd
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
    """a stream whose only use is kr_debug_bgzf_deflate and kr_debug_huffman_lengths_device"""
    hx, dx = toy
    st = dx.stream(max_reads=64, max_bases=1 << 16)
    st.text_enable(hx, 1 << 16, 1 << 12)
    st.bgzf_out_enable()
    yield st
    st.close()


def more_cases():
    """as test_gpu_bgzf_deflate.py builds them"""
    rng = np.random.default_rng(77)
    text = dc.report_text(600)
    nine = text[:9 * dc.MEMBER - 1000]  # three workgroups, the last one part empty
    mixed = (text[:100000] + rng.integers(0, 256, 70000, dtype=np.uint8).tobytes() + b"a" * 66000 + dc.distinct(40000, 3) + text[:60000])[:5 * dc.MEMBER + 7]
    assert len(mixed) == 5 * dc.MEMBER + 7 and -(-len(nine) // dc.MEMBER) == 9
    return {"nine_members": nine, "mixed_5_members_and_7": mixed}


ALL = {**dc.cases(), **more_cases(), **dd.dyn_cases()}


@pytest.mark.parametrize("name", sorted(ALL))
def test_the_device_gives_the_hosts_level_2_bytes(capi, deflater, name):
    data = ALL[name]
    want = capi.bgzf_deflate_host(data, level=2)
    got = deflater.bgzf_deflate(data, level=2)
    assert len(got) == len(want) and got == want
    dc.check_stream(capi, data, got)


def test_token_tile_seams_of_pass_2(capi, deflater):
    """prefixes of the report text with 63, 64, 65, 128 and 129 tokens in a dynamic block: one tile of tokens less one, full, and one
    more; two tiles, and one more.  The lengths come from the host's stats."""
    text = dc.report_text(100)
    want = {63, 64, 65, 128, 129}
    found = {}
    for n in range(40, 4000):
        st = capi.bgzf_deflate_stats(text[:n], level=2)
        k = st["literals"] + st["matches"]
        if k in want and k not in found and st["dynamic"] == 1:
            found[k] = n
        if len(found) == len(want):
            break
    assert sorted(found) == sorted(want), found
    for k, n in sorted(found.items()):
        data = text[:n]
        got = deflater.bgzf_deflate(data, level=2)
        assert got == capi.bgzf_deflate_host(data, level=2), (k, n)
        assert dd.btype(got) == 2
        dc.check_stream(capi, data, got)


@pytest.mark.parametrize("name", sorted(dd.builder_cases()))
def test_the_builder_kernel_gives_the_hosts_lengths(capi, deflater, name):
    freq, maxbits, expect = dd.builder_cases()[name]
    lens, limited = capi.huffman_lengths(freq, maxbits)
    dlens, dlimited = deflater.huffman_lengths(freq, maxbits)
    assert dlens.tolist() == lens.tolist() and dlimited == limited
    dd.check_lengths(freq, maxbits, dlens, dlimited, expect)


def test_levels_on_one_stream(capi, toy):
    hx, dx = toy
    data = ALL["nine_members"]
    one, two = capi.bgzf_deflate_host(data, level=1), capi.bgzf_deflate_host(data, level=2)
    assert one == capi.bgzf_deflate_host(data) and len(two) < len(one)
    st = dx.stream(max_reads=64, max_bases=1 << 16)
    st.text_enable(hx, 1 << 16, 1 << 12)
    with pytest.raises(capi.KrError) as e:
        st.bgzf_out_level(2)
    assert e.value.code == capi.KR_ERR_STATE  # before kr_stream_bgzf_out_enable
    st.bgzf_out_enable()
    assert st.bgzf_deflate(data) == one  # level 1 is the default
    assert st.bgzf_deflate(data, level=1) == one
    assert st.bgzf_deflate(data, level=2) == two
    assert st.bgzf_deflate(data) == two  # the level stays
    for bad in (3, 0):
        with pytest.raises(capi.KrError) as e:
            st.bgzf_out_level(bad)
        assert e.value.code == capi.KR_ERR_ARG
        assert st.bgzf_deflate(data) == two  # the level in force stays
    assert st.bgzf_deflate(data, level=1) == one
    with pytest.raises(capi.KrError) as e:
        st.bgzf_out_level(3)
    assert e.value.code == capi.KR_ERR_ARG
    assert st.bgzf_deflate(data) == one
    st.close()


@pytest.fixture(scope="module")
def reads(capi, synth, toy_genomes):
    """the toy reads (long sequences among them) and 3,000 synthetic reads"""
    n1, b1, o1 = capi.read_fastx(os.path.join(GOLDEN, "toy_reads.fq"))
    b2, o2, n2 = synth.sample_reads(toy_genomes, 3000, seed=5)
    bases = np.concatenate([b1, b2])
    offs = np.concatenate([o1, o2[1:] + o1[-1]]).astype(np.uint64)
    return bases, offs, list(n1) + list(n2)


def test_a_real_batch(capi, toy, reads):
    hx, dx = toy
    bases, offs, names = reads
    st = dx.stream(max_reads=4 * len(names), max_bases=len(bases) + 64)
    st.text_enable(hx, 1 << 24, 1 << 20)
    st.bgzf_out_enable()
    st.submit_text(bases, offs, names, capi.KR_TILE_ROWS)
    one, tl1 = st.collect_text_bgzf()
    two, tl2 = st.collect_text_bgzf(level=2)
    text = st.collect_text()
    assert tl1 == tl2 == len(text) > dc.MEMBER  # two members at least
    assert two == capi.bgzf_deflate_host(text, level=2) and one == capi.bgzf_deflate_host(text)
    assert gzip.decompress(two + capi.bgzf_eof()) == text
    assert len(two) < len(one)
    # a second, smaller batch at level 2, then level 1 again: the level may change between batches
    n = 100
    st.submit_text(bases[:int(offs[n])], offs[:n + 1], names[:n], capi.KR_TILE_ROWS)
    comp, tl = st.collect_text_bgzf()
    text2 = st.collect_text()
    assert 0 < tl == len(text2) < len(text) and comp == capi.bgzf_deflate_host(text2, level=2)
    assert st.collect_text_bgzf(level=1)[0] == capi.bgzf_deflate_host(text2)
    st.close()


def test_a_seek_text(capi, tmp_path):
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
    st.seek_enable(1 << 22, 1 << 20)
    st.bgzf_out_enable()
    st.submit_text(bases, offs, names, capi.KR_SEEK)
    one, _ = st.collect_text_bgzf()
    two, tl = st.collect_text_bgzf(level=2)
    text = st.collect_text()
    assert tl == len(text) > dc.MEMBER and two == capi.bgzf_deflate_host(text, level=2) and gzip.decompress(two + capi.bgzf_eof()) == text
    assert len(two) < len(one) and one == capi.bgzf_deflate_host(text)
    st.close(), dx.close(), hx.close()


# ---- the CLI -------------------------------------------------------------------------------------------------------------------
def cli(sub, idx, q, extra, env=None, out=None):
    """(the report's bytes, stderr): from the file -o names"""
    cmd = [EXE, sub, "-i", idx, "-q", str(q)] + extra + ["-o", str(out)]
    r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, KR_CLI_TIMING="1", **(env or {})), timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    assert r.stdout == b""
    return open(out, "rb").read(), r.stderr.decode()


def strip_invocation(report):
    """the first line names the flags and the output file"""
    head, rest = report.split(b"\n", 1)
    assert head.startswith(b"# software: krepp")
    return rest


@pytest.fixture(scope="module")
def files(synth, toy_genomes, tmp_path_factory, capi):
    d = tmp_path_factory.mktemp("bgzf_out_dyn")
    bases, offs, names = synth.sample_reads(toy_genomes, 3000, seed=4)
    recs = []
    for i in range(3000):
        s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
        recs.append(b"@%s extra\n%s\n+\n%s\n" % (names[i].encode(), s, b"F" * len(s)))
    g0 = bytes(next(iter(toy_genomes.values())))
    (d / "clean.fq").write_bytes(b"".join(recs))
    (d / "g0.fa").write_bytes(b">g0\n" + g0 + b"\n")
    capi.build_sketch(d / "g0.fa", d / "g0.skc")
    return {"clean": str(d / "clean.fq"), "SKETCH": str(d / "g0.skc")}


CLI_CASES = {
    "dist": ("dist", [], {}),
    "dist-gpu-parse": ("dist", ["--gpu-parse"], {"KR_CLI_PARSE_CHUNK": "100000"}),
    "seek-gpu-seek": ("seek", ["--gpu-seek"], {}),
    "place-tabular": ("place", ["--tabular"], {}),
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_level_2(capi, toy_index_dir, files, tmp_path, case):
    sub, extra, env = CLI_CASES[case]
    idx = files["SKETCH"] if sub == "seek" else toy_index_dir
    plain, _ = cli(sub, idx, files["clean"], extra, env, out=tmp_path / "plain.out")
    one, err1 = cli(sub, idx, files["clean"], extra + ["--bgzf-out"], env, out=tmp_path / "one.gz")
    two, err2 = cli(sub, idx, files["clean"], extra + ["--bgzf-out", "--bgzf-level", "2"], env, out=tmp_path / "two.gz")
    inflated = gzip.decompress(two)
    assert strip_invocation(inflated) == strip_invocation(plain) and len(plain) > 1000
    assert two.endswith(dc.EOF_MEMBER) and two.count(dc.EOF_MEMBER) == 1
    k, cb, u = capi.bgzf_walk(two, 1 << 40)  # our own reader walks it: whole members to the end
    assert cb == len(two) and u == len(inflated) and k >= 2
    assert len(two) < len(one)
    line1 = [ln for ln in err1.splitlines() if ln.startswith("[timing] bgzf-out:")]
    line2 = [ln for ln in err2.splitlines() if ln.startswith("[timing] bgzf-out:")]
    assert len(line1) == len(line2) == 1 and line1[0].endswith("; level 1") and line2[0].endswith("; level 2")


def test_cli_refuses_a_level_without_bgzf_out_and_levels_it_does_not_have(toy_index_dir, files, tmp_path):
    base = [EXE, "dist", "-i", toy_index_dir, "-q", files["clean"], "-o", str(tmp_path / "never.out")]
    r = subprocess.run(base + ["--bgzf-level", "2"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and "[ERROR] --bgzf-level needs --bgzf-out" in r.stderr
    for bad in ("3", "0", "two"):
        r = subprocess.run(base + ["--bgzf-out", "--bgzf-level", bad], capture_output=True, text=True, timeout=600)
        assert r.returncode == 1 and "[ERROR] --bgzf-level" in r.stderr, bad
    assert not os.path.exists(tmp_path / "never.out")


def test_the_option_is_in_the_usage_text():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("--bgzf-level") >= 3  # dist, place, seek
