"""`krepp seek --gpu-parse --gpu-seek --extract-matched / --extract-unmatched`: the two files against the report of the same run.  The
matched file is exactly the records whose row carries a DIST, in input order, as the bytes they have in the (inflated) input; the
unmatched file is the rest; the report is byte for byte that of the run without the extract flags.  Plain FASTQ, plain FASTA, BGZF,
and ordinary gzip with --gpu-inflate; KR_CLI_PARSE_CHUNK=4096 cuts each input into many chunks."""
import gzip
import os
import re
import subprocess

import numpy as np
import pytest

import seek_craft as sc
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
ENV = {"KR_CLI_PARSE_CHUNK": "4096", "KR_CLI_TIMING": "1"}
GPU = ["--gpu-parse", "--gpu-seek"]


def cli(sketch, q, extra, ok=True):
    r = subprocess.run([EXE, "seek", "-i", sketch, "-q", str(q)] + extra, capture_output=True, env=dict(os.environ, **ENV), timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr.decode()
    return r


def body(stdout):
    """the report behind its first line, which names the invocation"""
    return stdout.split(b"\n", 1)[1]


def rows(stdout):
    """[(id, DIST text)] of a report: behind the invocation line and the column header"""
    lines = stdout.split(b"\n", 2)[2].splitlines()
    return [tuple(l.split(b"\t")) for l in lines]


@pytest.fixture(scope="module")
def files(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("seekxcli")
    g = sc.genome_a()
    sketch = sc.write_sketch(capi, d, "a", g, sc.CFG_A)
    rng = np.random.default_rng(41)
    fq, fa = [], []
    for i in range(120):
        kind = i % 3
        seq = sc.random_dna(rng, 150) if kind == 0 else sc.mutate(rng, g[0][60 * i:60 * i + 150], 0.01 * (1 + i % 9))
        fq.append(b"@q%d some comment %d\n%s\n+\n%s\n" % (i, i, seq.encode(), bytes(33 + (j * 7 + i) % 40 for j in range(len(seq)))))
        body = b"".join(seq[j:j + 60].encode() + b"\n" for j in range(0, len(seq), 60))
        fa.append(b">a%d descr\n%s" % (i, body))
    out = {"SKETCH": sketch, "recs": {"fastq": fq, "fasta": fa, "bgzf": fq, "gzip": fq}}
    (d / "r.fq").write_bytes(b"".join(fq))
    (d / "r.fa").write_bytes(b"".join(fa))
    (d / "r.bgzf.fq.gz").write_bytes(capi.bgzf_deflate_host_member(b"".join(fq), 1, 3000) + capi.bgzf_eof())
    (d / "r.fq.gz").write_bytes(gzip.compress(b"".join(fq)))
    out.update(fastq=str(d / "r.fq"), fasta=str(d / "r.fa"), bgzf=str(d / "r.bgzf.fq.gz"), gzip=str(d / "r.fq.gz"), dir=d)
    return out


def flags_of(inp):
    return GPU + (["--gpu-inflate"] if inp == "gzip" else [])


@pytest.mark.parametrize("inp", ["fastq", "fasta", "bgzf", "gzip"])
def test_split_follows_the_report(files, inp):
    d, recs = files["dir"], files["recs"][inp]
    want = body(cli(files["SKETCH"], files[inp], flags_of(inp)).stdout)
    m, u = d / f"{inp}.m", d / f"{inp}.u"
    r = cli(files["SKETCH"], files[inp], flags_of(inp) + ["--extract-matched", str(m), "--extract-unmatched", str(u)])
    assert body(r.stdout) == want  # the report is unchanged
    rw = rows(r.stdout)
    assert len(rw) == len(recs)
    hit = [dist != b"NaN" for _, dist in rw]
    assert any(hit) and not all(hit)
    gm, gu = m.read_bytes(), u.read_bytes()
    assert gm == b"".join(x for x, k in zip(recs, hit) if k)
    assert gu == b"".join(x for x, k in zip(recs, hit) if not k)
    assert len(gm) + len(gu) == sum(map(len, recs))  # every input byte once
    t = re.search(r"\[timing\] extract: (\d+) matched of (\d+) reads, (\d+) \+ (\d+) bytes, [\d.]+ ms of kernels", r.stderr.decode())
    assert t and [int(x) for x in t.groups()] == [sum(hit), len(recs), len(gm), len(gu)]
    # one file alone
    only = d / f"{inp}.only"
    r = cli(files["SKETCH"], files[inp], flags_of(inp) + ["--extract-unmatched", str(only)])
    assert body(r.stdout) == want and only.read_bytes() == gu


def test_threshold(files):
    """The report prints five decimals: the threshold goes to the midpoint of the widest gap between the sorted reported values, and
    that gap must exceed 1e-4, so that rounding cannot move a read across it"""
    d, recs = files["dir"], files["recs"]["fastq"]
    rw = rows(cli(files["SKETCH"], files["fastq"], GPU).stdout)
    vals = sorted({float(x) for _, x in rw if x != b"NaN"})
    gaps = [(b - a, (a + b) / 2) for a, b in zip(vals, vals[1:])]
    gap, mid = max(gaps)
    assert gap > 1e-4
    m, u = d / "th.m", d / "th.u"
    cli(files["SKETCH"], files["fastq"], GPU + ["--extract-matched", str(m), "--extract-unmatched", str(u), "--extract-max", repr(mid)])
    hit = [x != b"NaN" and float(x) <= mid for _, x in rw]
    assert any(hit) and sum(hit) < sum(x != b"NaN" for _, x in rw)
    assert m.read_bytes() == b"".join(x for x, k in zip(recs, hit) if k)
    assert u.read_bytes() == b"".join(x for x, k in zip(recs, hit) if not k)


@pytest.mark.parametrize("extra", [[], ["--bgzf-level", "2", "--bgzf-member", "1024"]], ids=["default", "level2-member1024"])
def test_bgzf_files(capi, files, extra):
    d = files["dir"]
    pm, pu = d / "z.plain.m", d / "z.plain.u"
    want = body(cli(files["SKETCH"], files["fastq"], GPU + ["--extract-matched", str(pm), "--extract-unmatched", str(pu)]).stdout)
    zm, zu = d / "z.m.gz", d / "z.u.gz"
    r = cli(files["SKETCH"], files["fastq"], GPU + ["--extract-matched", str(zm), "--extract-unmatched", str(zu), "--extract-bgzf"] + extra)
    assert body(r.stdout) == want  # (the report stays plain: --bgzf-out was not given)
    for z, p in ((zm, pm), (zu, pu)):
        comp = z.read_bytes()
        assert comp.endswith(capi.bgzf_eof()) and len(capi.bgzf_eof()) == 28
        assert gzip.decompress(comp) == p.read_bytes() and p.read_bytes()


def test_empty_files_are_created(files):
    d = files["dir"]
    allm = d / "allm.fq"
    allm.write_bytes(b"".join(b"@e%d\n%s\n+\n%s\n" % (i, sc.genome_a()[0][100 * i:100 * i + 150].encode(), b"I" * 150) for i in range(10)))
    m, u = d / "allm.m", d / "allm.u"
    cli(files["SKETCH"], allm, GPU + ["--extract-matched", str(m), "--extract-unmatched", str(u)])
    assert m.read_bytes() == allm.read_bytes() and u.exists() and u.read_bytes() == b""


@pytest.mark.parametrize("case", ["crlf", "no-final-newline", "gzip-without-gpu-inflate", "bgzf-crlf"])
def test_no_host_fallback(capi, files, case):
    d, recs = files["dir"], list(files["recs"]["fastq"])
    q = d / f"{case}.fq"
    if case == "crlf":
        recs[40] = recs[40].replace(b"\n", b"\r\n")
        q.write_bytes(b"".join(recs))
        at = sum(map(len, recs[:40]))
    elif case == "no-final-newline":
        q.write_bytes(b"".join(recs)[:-1])
        at = sum(map(len, recs[:-1]))
    elif case == "bgzf-crlf":
        # a block-gzipped input: N is the file offset of the BGZF member that holds the record's first byte, the inflated byte inside
        # that member stands beside the reason
        recs[40] = recs[40].replace(b"\n", b"\r\n")
        comp = capi.bgzf_deflate_host_member(b"".join(recs), 1, 3000)
        q = d / "crlf.bgzf.fq.gz"
        q.write_bytes(comp + capi.bgzf_eof())
        u_at, at = sum(map(len, recs[:40])), 0
        for _ in range(u_at // 3000):  # every member but the last inflates to 3,000 bytes
            at += capi.bgzf_member_size(comp[at:])
        inner = r"\(inflated byte %d of the BGZF member\) " % (u_at % 3000)
    else:
        q, at = files["gzip"], 0
    m = d / f"{case}.m"
    cli(files["SKETCH"], q, GPU, ok=True)  # without the flags the host reader takes over and the run succeeds
    r = cli(files["SKETCH"], q, GPU + ["--extract-matched", str(m)], ok=False)
    err = r.stderr.decode()
    assert r.returncode == 1, err
    assert re.search(r"\[ERROR\] --extract-\*: .+ %sat input offset %d: the records must be ones the GPU record finder accepts \(include/krepp_amd.h\)" % (inner if case == "bgzf-crlf" else "", at), err), err
