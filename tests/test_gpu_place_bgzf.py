"""`place` rows deflated on the GPU (kr_stream_place_bgzf; csrc/kr_host_place.inc: place_device_finish, csrc/kr_host_deflate.inc:
kr::place_text_deflate), the member length as a parameter of the kernels (kr_stream_bgzf_member, kr_debug_bgzf_deflate_at) and
`krepp place --bgzf-out --gpu-deflate` / `--bgzf-member`.

The kernels run the encoder the host runs (csrc/kr_deflate.h) with the same cuts, so wherever one range makes a call's text the
members must EQUAL kr_bgzf_deflate_host_member of the plain call's text, byte for byte; with several ranges they inflate to it.  The
plain text of every comparison comes from a Placer of its own with the setting off.  kr_place_bgzf_counters witnesses who deflated:
a pass through the host encoder cannot stand in for the kernels.  Nothing is compared with a tolerance."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import deflate_cases as dc
from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
USER_OLD = "(G000735195:0.0276038,G000018865:0.0228997)N2640:0.160977"
USER_NEW = "(G000735195:0.03,NEWLEAF:0.02)N2640:0.160977"


# ---- the kernels at the new seams -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def toy(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    dx = hx.upload(0)
    yield hx, dx
    dx.close()
    hx.close()


@pytest.fixture(scope="module")
def deflater(capi, toy):
    """a stream whose only use is kr_debug_bgzf_deflate_at"""
    hx, dx = toy
    st = dx.stream(max_reads=64, max_bases=1 << 16)
    st.text_enable(hx, 1 << 16, 1 << 12)
    st.bgzf_out_enable()
    yield st
    st.bgzf_member(dc.MEMBER)
    st.close()


@pytest.fixture(scope="module")
def seam_inputs():
    """about 3 members of report-shaped and of random bytes for every member length tried, + 63 bytes to skip; a text of many short
    members (more than one workgroup of four)"""
    rng = np.random.default_rng(99)
    text = dc.report_text(200)
    rnd = rng.integers(0, 256, 3 * dc.MEMBER + 100, dtype=np.uint8).tobytes()
    assert len(text) > 3 * dc.MEMBER + 100
    return text, rnd


@pytest.mark.parametrize("L", [dc.MEMBER, 4099, 257])
@pytest.mark.parametrize("level", [1, 2])
def test_kernel_against_host_at_an_odd_base_and_an_odd_cut(capi, deflater, seam_inputs, level, L):
    """The text starts `skip` bytes into an allocation and members start every L bytes from there: for L = 4,099 and 257 at every
    alignment in turn.  3 L + 17 bytes behind the skip: three whole members and a short one."""
    deflater.bgzf_out_level(level)
    deflater.bgzf_member(L)
    for kind, src in zip(("text", "random"), seam_inputs):
        for skip in (0, 1, 2, 3, 63):
            data = src[:skip + 3 * L + 17]
            got = deflater.bgzf_deflate_at(data, skip)
            want = capi.bgzf_deflate_host_member(data[skip:], level, L)
            assert len(got) == len(want) and got == want, (kind, skip)
            assert capi.bgzf_walk(got, 1 << 40) == (4, len(got), len(data) - skip)
    # many short members: 40,000 bytes from an odd base
    data = seam_inputs[0][:40001]
    got = deflater.bgzf_deflate_at(data, 1)
    assert got == capi.bgzf_deflate_host_member(data[1:], level, L) and gzip.decompress(got) == data[1:]
    assert capi.bgzf_walk(got, 1 << 40)[0] == -(-40000 // L)
    deflater.bgzf_out_level(1)
    deflater.bgzf_member(dc.MEMBER)


def test_member_length_arguments_and_the_skip(capi, deflater):
    deflater.bgzf_member(4099)
    for bad in (0, 255, 65281):
        with pytest.raises(capi.KrError) as e:
            deflater.bgzf_member(bad)
        assert e.value.code == capi.KR_ERR_ARG
    data = dc.report_text(10)
    assert deflater.bgzf_deflate(data) == capi.bgzf_deflate_host_member(data, 1, 4099)  # the value in force stayed
    assert deflater.bgzf_deflate_at(data, len(data)) == b""
    with pytest.raises(capi.KrError) as e:
        deflater.bgzf_deflate_at(data, len(data) + 1)
    assert e.value.code == capi.KR_ERR_ARG
    deflater.bgzf_member(dc.MEMBER)
    assert deflater.bgzf_deflate(data) == capi.bgzf_deflate_host(data)


def test_member_length_on_a_dist_stream(capi, synth, toy, toy_genomes):
    hx, dx = toy
    bases, offs, names = synth.sample_reads(toy_genomes, 3000, seed=5)
    st = dx.stream(max_reads=4 * len(names), max_bases=len(bases) + 64)
    st.text_enable(hx, 1 << 24, 1 << 20)
    st.bgzf_out_enable()
    st.submit_text(bases, offs, names, capi.KR_TILE_ROWS)
    comp, text_len = st.collect_text_bgzf()
    text = st.collect_text()
    assert text_len == len(text) > 2 * dc.MEMBER and comp == capi.bgzf_deflate_host(text)
    for level in (1, 2):
        st.bgzf_out_level(level)
        st.bgzf_member(8160)
        c2, tl2 = st.collect_text_bgzf()
        assert tl2 == len(text) and gzip.decompress(c2) == text
        assert c2 == capi.bgzf_deflate_host_member(text, level, 8160)
        assert capi.bgzf_walk(c2, 1 << 40)[0] == -(-len(text) // 8160)
        st.bgzf_member(dc.MEMBER)
        assert st.collect_text_bgzf()[0] == capi.bgzf_deflate_host(text, level=level)
    st.bgzf_out_level(1)
    assert st.collect_text_bgzf() == (comp, text_len)
    st.close()


# ---- kr_place_stream / kr_place_stream_parsed --------------------------------------------------------------------------------------
def tree_kw(tree):
    if tree == "user":
        nwk = open(os.path.join(GOLDEN, "tree_toy.nwk")).read()
        assert USER_OLD in nwk
        return dict(nwk_text=nwk.replace(USER_OLD, USER_NEW))
    if tree == "lineages":
        return dict(lineage_text=open(os.path.join(GOLDEN, "lineages_toy.txt")).read())
    return dict()


def fastq(batch):
    b, o, names = batch
    out = []
    for i, nm in enumerate(names):
        s = b[int(o[i]):int(o[i + 1])].tobytes()
        out.append(b"@" + nm.encode() + b"\n" + s + b"\n+\n" + b"F" * len(s) + b"\n")
    return b"".join(out)


class Ctx:
    def __init__(self, capi, synth, index_dir, genomes):
        self.capi = capi
        self.hx = capi.HostIndex(index_dir)
        bases, offs, names = synth.sample_reads(genomes, 1500, seed=37)
        self.batches = [self.cut(bases, offs, names, 0, 700), self.cut(bases, offs, names, 700, 1100), self.cut(bases, offs, names, 1100, 1500)]
        junk = synth.sample_reads(genomes, 64, seed=43, mix=[(1.0, None)])  # reads that match nothing
        self.junk = (junk[0], junk[1], ["junk%d" % i for i in range(64)])
        self.plain_cache = {}

    @staticmethod
    def cut(bases, offs, names, r0, r1):
        o = (offs[r0:r1 + 1] - offs[r0]).astype(np.uint64)
        return np.ascontiguousarray(bases[int(offs[r0]):int(offs[r1])]), o, list(names[r0:r1])

    def placer(self, tree, tabular, multi=1, **kw):
        t = tree_kw(tree)
        return self.capi.Placer(self.hx, t.get("nwk_text"), 0, tabular=tabular, max_reads=4096, max_bases=1 << 20, lineage_text=t.get("lineage_text"), multi=multi, **kw)

    def plain(self, tree, tabular, multi):
        """the three calls' texts with the setting off, on one Placer (once per configuration)"""
        key = (tree, tabular, multi)
        if key not in self.plain_cache:
            pl = self.placer(tree, tabular, multi)
            self.plain_cache[key] = [pl.place(*b, want_placements=False, raw_text=True)[0] for b in self.batches]
            pl.close()
        return self.plain_cache[key]

    def call(self, pl, batch, entry, want_placements=False):
        if entry == "parsed":
            return pl.place_parsed(fastq(batch), want_placements=want_placements, raw_text=True)[:2]
        return pl.place(*batch, want_placements=want_placements, raw_text=True)


@pytest.fixture(scope="module")
def ctx(capi, synth, toy_index_dir, toy_genomes):
    return Ctx(capi, synth, toy_index_dir, toy_genomes)


def moved(capi, c0):
    c1 = capi.place_bgzf_counters()
    return (c1[0] - c0[0], c1[1] - c0[1])


@pytest.mark.parametrize("multi", [1, 0])
@pytest.mark.parametrize("tabular", [0, 1])
@pytest.mark.parametrize("tree", ["backbone", "user", "lineages"])
def test_one_range_a_call_gives_the_host_encoders_bytes(ctx, tree, tabular, multi):
    """Three calls in a row on one stream; only the first has has_previous == 0 (jplace: its text loses the leading ",\\n", and the
    deflate starts two bytes into the device's text).  Level 1 at the default member length, level 2 at 4,099 (several members a call,
    cut at odd addresses), through both entry points."""
    capi = ctx.capi
    plain = ctx.plain(tree, tabular, multi)
    assert all(len(t) > 4099 for t in plain)
    if tabular == 0:
        assert not plain[0].startswith(b",\n") and plain[1].startswith(b",\n") and plain[2].startswith(b",\n")
    for entry in ("stream", "parsed"):
        for level, L in ((1, dc.MEMBER), (2, 4099)):
            pl = ctx.placer(tree, tabular, multi)
            pl.st.place_bgzf(level)
            pl.st.bgzf_member(L)
            for b, want_text in zip(ctx.batches, plain):
                c0, t0 = capi.place_bgzf_counters(), capi.place_text_counters()
                got, _ = ctx.call(pl, b, entry)
                assert got == capi.bgzf_deflate_host_member(want_text, level, L), (entry, level)
                assert gzip.decompress(got) == want_text
                assert moved(capi, c0) == (1, 0), "the range was not deflated on the device"
                t1 = capi.place_text_counters()
                assert (t1[0] - t0[0], t1[1] - t0[1]) == (1, 0)
            pl.close()


@pytest.mark.parametrize("tabular", [0, 1])
def test_three_ranges_a_call(ctx, monkeypatch, tabular):
    capi = ctx.capi
    plain = ctx.plain("backbone", tabular, 1)
    monkeypatch.setenv("KR_PLACE_RANGES", "3")
    for level, L in ((1, 4099), (2, dc.MEMBER)):
        pl = ctx.placer("backbone", tabular)
        pl.st.place_bgzf(level)
        pl.st.bgzf_member(L)
        for b, want_text in zip(ctx.batches, plain):
            c0 = capi.place_bgzf_counters()
            got, _ = ctx.call(pl, b, "stream")
            assert gzip.decompress(got) == want_text
            k, cb, u = capi.bgzf_walk(got, 1 << 40)
            assert (cb, u) == (len(got), len(want_text)) and k >= 3
            assert moved(capi, c0) == (3, 0)
        pl.close()
    monkeypatch.delenv("KR_PLACE_RANGES")


@pytest.mark.parametrize("tabular", [0, 1])
@pytest.mark.parametrize("how", ["text-cap", "host-text"])
def test_a_range_the_host_formats_goes_through_the_host_encoder(ctx, monkeypatch, tabular, how):
    """A text buffer of half the first call's bytes (KR_DEBUG_PLACE_CAPS "t=", as tests/test_gpu_place_capacity.py sets it: flag 2, the
    host formats the range), or KR_PLACE_HOST_TEXT=1: the host's text goes through kr_bgzf_deflate_host_member at the stream's level and
    member length.  The calls behind it are the device's again once the knob is gone."""
    capi = ctx.capi
    plain = ctx.plain("backbone", tabular, 1)
    pl0 = ctx.placer("backbone", tabular)  # what the device's text takes, for the knob
    ctx.call(pl0, ctx.batches[0], "stream")
    text_bytes = capi.place_path_counters()["text_bytes"]
    pl0.close()
    assert text_bytes >= len(plain[0]) > 0
    for level, L in ((1, dc.MEMBER), (2, 4099)):
        pl = ctx.placer("backbone", tabular)
        pl.st.place_bgzf(level)
        pl.st.bgzf_member(L)
        if how == "text-cap":
            monkeypatch.setenv("KR_DEBUG_PLACE_CAPS", "t=%d" % (text_bytes // 2))
        else:
            monkeypatch.setenv("KR_PLACE_HOST_TEXT", "1")
        c0, p0 = capi.place_bgzf_counters(), capi.place_path_counters()
        got, _ = ctx.call(pl, ctx.batches[0], "stream")
        assert moved(capi, c0) == (0, 1), "the host encoder did not take the range"
        if how == "text-cap":
            assert capi.place_path_counters()["text_flag_2"] - p0["text_flag_2"] == 1
        assert gzip.decompress(got) == plain[0] and got == capi.bgzf_deflate_host_member(plain[0], level, L)
        monkeypatch.delenv("KR_DEBUG_PLACE_CAPS" if how == "text-cap" else "KR_PLACE_HOST_TEXT")
        c0 = capi.place_bgzf_counters()
        got, _ = ctx.call(pl, ctx.batches[1], "stream")  # a device piece behind a host piece
        assert moved(capi, c0) == (1, 0)
        assert got == capi.bgzf_deflate_host_member(plain[1], level, L)
        pl.close()


def test_placements_wanted_with_rows_go_through_the_host_encoder(ctx):
    capi = ctx.capi
    plain = ctx.plain("backbone", 0, 1)
    ref = ctx.placer("backbone", 0)
    want_pl = ref.place(*ctx.batches[0], want_placements=True)[1]
    ref.close()
    pl = ctx.placer("backbone", 0)
    pl.st.place_bgzf(2)
    c0 = capi.place_bgzf_counters()
    got, p = ctx.call(pl, ctx.batches[0], "stream", want_placements=True)
    assert moved(capi, c0) == (0, 1)
    assert got == capi.bgzf_deflate_host_member(plain[0], 2, dc.MEMBER) and p.tobytes() == want_pl.tobytes() and len(p) > 0
    pl.close()


def test_summary_mode_and_a_batch_without_a_reported_read_give_no_member(ctx):
    capi = ctx.capi
    ref = ctx.placer("backbone", 2)
    want_text, want_pl = ref.place(*ctx.batches[0], want_placements=True)
    ref.close()
    pl = ctx.placer("backbone", 2)
    pl.st.place_bgzf(1)
    c0 = capi.place_bgzf_counters()
    got, p = ctx.call(pl, ctx.batches[0], "stream", want_placements=True)
    assert got == b"" and want_text == "" and p.tobytes() == want_pl.tobytes() and len(p) > 0
    assert moved(capi, c0) == (0, 0)
    pl.close()
    for tabular in (0, 1):
        ref = ctx.placer("backbone", tabular)
        assert ref.place(*ctx.junk, want_placements=False)[0] == ""  # (the premise: no read of these is reported)
        ref.close()
        for entry in ("stream", "parsed"):
            pl = ctx.placer("backbone", tabular)
            pl.st.place_bgzf(2)
            c0 = capi.place_bgzf_counters()
            assert ctx.call(pl, ctx.junk, entry)[0] == b""
            assert moved(capi, c0) == (0, 0) and pl.prev.value == 0
            # ... and the call behind it is still the first of its file
            assert ctx.call(pl, ctx.batches[0], entry)[0] == capi.bgzf_deflate_host_member(ctx.plain("backbone", tabular, 1)[0], 2, dc.MEMBER)
            pl.close()


def test_levels(ctx):
    capi = ctx.capi
    plain = ctx.plain("backbone", 0, 1)
    pl = ctx.placer("backbone", 0)
    for bad in (3, 9):
        with pytest.raises(capi.KrError) as e:
            pl.st.place_bgzf(bad)
        assert e.value.code == capi.KR_ERR_ARG
    assert ctx.call(pl, ctx.batches[0], "stream")[0] == plain[0]  # still off
    pl.st.place_bgzf(2)
    assert ctx.call(pl, ctx.batches[1], "stream")[0] == capi.bgzf_deflate_host_member(plain[1], 2, dc.MEMBER)
    with pytest.raises(capi.KrError):
        pl.st.place_bgzf(3)
    pl.st.place_bgzf(0)  # level 0 after level 2: the plain bytes
    c0 = capi.place_bgzf_counters()
    assert ctx.call(pl, ctx.batches[2], "stream")[0] == plain[2]
    assert moved(capi, c0) == (0, 0)
    pl.close()


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


TIMING = r"\[timing\] bgzf-out: (\d+) text bytes, (\d+) compressed bytes \(without the end member\); (\d+) pieces deflated on the device, (\d+) by the host encoder"


@pytest.fixture(scope="module")
def query(synth, toy_genomes, tmp_path_factory):
    d = tmp_path_factory.mktemp("place_bgzf")
    bases, offs, names = synth.sample_reads(toy_genomes, 3000, seed=4)
    recs = []
    for i in range(3000):
        s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
        recs.append(b"@%s extra\n%s\n+\n%s\n" % (names[i].encode(), s, b"F" * len(s)))
    (d / "clean.fq").write_bytes(b"".join(recs))
    return str(d / "clean.fq")


CLI_CASES = {
    "jplace": ([], {}),
    "jplace-batches": ([], {"KR_CLI_BATCH_READS": "1000"}),
    "jplace-gpu-parse": (["--gpu-parse"], {"KR_CLI_PARSE_CHUNK": "100000"}),
    "jplace-level2-member-batches": (["--bgzf-level", "2", "--bgzf-member", "8160"], {"KR_CLI_BATCH_READS": "1000"}),
    "tabular": (["--tabular"], {}),
    "tabular-member-batches": (["--tabular", "--bgzf-member", "8160"], {"KR_CLI_BATCH_READS": "1000"}),
    "tabular-gpu-parse-level2": (["--tabular", "--gpu-parse", "--bgzf-level", "2"], {"KR_CLI_PARSE_CHUNK": "100000", "KR_CLI_BATCH_READS": "1000"}),
}


@pytest.mark.parametrize("case", sorted(CLI_CASES))
def test_cli_gpu_deflate_inflates_to_the_plain_output(capi, toy_index_dir, query, tmp_path, case):
    extra, env = CLI_CASES[case]
    plain_flags = [x for i, x in enumerate(extra) if x not in ("--bgzf-level", "--bgzf-member") and (i == 0 or extra[i - 1] not in ("--bgzf-level", "--bgzf-member"))]
    plain, _ = cli("place", toy_index_dir, query, plain_flags, env, out=tmp_path / "plain.out")
    comp, err = cli("place", toy_index_dir, query, extra + ["--bgzf-out", "--gpu-deflate"], env, out=tmp_path / "report.gz")
    same_report("place", extra, plain, gzip.decompress(comp))
    assert comp.endswith(dc.EOF_MEMBER) and comp.count(dc.EOF_MEMBER) == 1
    k, cb, u = capi.bgzf_walk(comp, 1 << 40)  # our own reader walks it: whole members to the end
    assert cb == len(comp) and u == len(gzip.decompress(comp)) and k >= 2
    m = re.search(TIMING, err)
    assert m, err
    text_bytes, comp_bytes, dev, host = map(int, m.groups())
    assert text_bytes == u and comp_bytes == len(comp) - 28 < text_bytes
    assert dev >= 1 and host >= 1, (dev, host)  # (the frame is the host's always)
    if "--bgzf-member" in extra:
        assert max(int.from_bytes(x[-4:], "little") for x in dc.members_of(capi, comp)) == 8160


def test_cli_default_member_and_one_range_writes_the_file_of_the_host_encoder(capi, toy_index_dir, query, tmp_path):
    """One batch, one range, --bgzf-member 65280: the same members as without --gpu-deflate.  The frame's member alone differs: it
    carries the invocation, which names the flags."""
    host, err_h = cli("place", toy_index_dir, query, ["--tabular", "--bgzf-out"], out=tmp_path / "report.gz")
    dev, err_d = cli("place", toy_index_dir, query, ["--tabular", "--bgzf-out", "--gpu-deflate", "--bgzf-member", "65280"], out=tmp_path / "report.gz")
    assert int(re.search(TIMING, err_h).group(3)) == 0 and int(re.search(TIMING, err_d).group(3)) == 1
    mh, md = dc.members_of(capi, host), dc.members_of(capi, dev)
    assert len(mh) == len(md) >= 3 and mh[1:] == md[1:] and md[-1] == dc.EOF_MEMBER
    fh, fd = gzip.decompress(mh[0]), gzip.decompress(md[0])
    assert fh.startswith(b"# software: krepp") and fh.split(b"\n", 1)[1] == fd.split(b"\n", 1)[1]


@pytest.mark.parametrize("args, message", [
    (["place", "--gpu-deflate"], "--gpu-deflate needs --bgzf-out"),
    (["dist", "--bgzf-out", "--gpu-deflate"], "--gpu-deflate is an option of `place`"),
    (["place", "--bgzf-member", "8160"], "--bgzf-member needs --bgzf-out"),
    (["place", "--bgzf-out", "--bgzf-member", "255"], "--bgzf-member: 256 to 65280"),
    (["dist", "--bgzf-out", "--bgzf-member", "65281"], "--bgzf-member: 256 to 65280"),
])
def test_cli_errors(toy_index_dir, query, args, message):
    r = subprocess.run([EXE, args[0], "-i", toy_index_dir, "-q", query] + args[1:], capture_output=True, text=True, timeout=600)
    assert r.returncode == 1 and message in r.stderr and r.stdout == ""


def test_cli_member_length_on_dist_and_summarize_ignores_gpu_deflate(capi, toy_index_dir, query, tmp_path):
    plain, _ = cli("dist", toy_index_dir, query, [], out=tmp_path / "plain.out")
    comp, err = cli("dist", toy_index_dir, query, ["--bgzf-out", "--bgzf-member", "8160"], out=tmp_path / "report.gz")
    same_report("dist", [], plain, gzip.decompress(comp))
    assert int(re.search(TIMING, err).group(3)) >= 1
    assert max(int.from_bytes(x[-4:], "little") for x in dc.members_of(capi, comp)) == 8160
    plain, _ = cli("place", toy_index_dir, query, ["--summarize"], out=tmp_path / "plain.out")
    comp, err = cli("place", toy_index_dir, query, ["--summarize", "--bgzf-out", "--gpu-deflate"], out=tmp_path / "report.gz")
    same_report("place", ["--summarize"], plain, gzip.decompress(comp))
    assert int(re.search(TIMING, err).group(3)) == 0


def test_the_flags_are_in_the_usage_text():
    r = subprocess.run([EXE, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.count("--bgzf-member") >= 3 and "--gpu-deflate" in r.stdout  # dist, place, seek; place
