"""`krepp seek --gpu-parse --gpu-seek --extract-* --query2 FILE / --interleaved`: paired reads split together.  The expectation comes
from the two UNPAIRED reports of the same files -- NaN or a number per row --: a pair is matched under `any` when either mate's row
carries a DIST (at most --extract-max, if given), under `both` when both do.  The four files must hold exactly the records of those
pairs, as the bytes they have in the input, record for record in step; both reports must be the unpaired runs' reports.
KR_CLI_PARSE_CHUNK=4096 cuts each input into many chunks, cut by kr_fastq_pair_cut behind the same number of records."""
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
NPAIRS = 150


def cli(sketch, q, extra, ok=True):
    r = subprocess.run([EXE, "seek", "-i", sketch, "-q", str(q)] + extra, capture_output=True, env=dict(os.environ, **ENV), timeout=300)
    if ok:
        assert r.returncode == 0, r.stderr.decode()
    return r


def body(report):
    """the report behind its first line, which names the invocation"""
    return report.split(b"\n", 1)[1]


def dists(report):
    """per row NaN or the printed number"""
    lines = report.split(b"\n", 2)[2].splitlines()
    return np.array([float(l.split(b"\t")[1]) for l in lines])


def matched(d, mx=None):
    return ~np.isnan(d) & (True if mx is None else (d <= mx))


def verdict(d1, d2, rule, mx=None):
    return (matched(d1, mx) | matched(d2, mx)) if rule == "any" else (matched(d1, mx) & matched(d2, mx))


def split(recs, keep):
    return b"".join(r for r, k in zip(recs, keep) if k), b"".join(r for r, k in zip(recs, keep) if not k)


def nrec(fastq_bytes):
    assert fastq_bytes.count(b"\n") % 4 == 0
    return fastq_bytes.count(b"\n") // 4


@pytest.fixture(scope="module")
def files(capi, tmp_path_factory):
    d = tmp_path_factory.mktemp("seekpairscli")
    g = sc.genome_a()
    sketch = sc.write_sketch(capi, d, "a", g, sc.CFG_A)
    rng = np.random.default_rng(61)
    r1, r2 = [], []
    for i in range(NPAIRS):
        c = (i // 2) % 4  # both mates from the genome, mate 1 only, mate 2 only, neither
        o = (53 * i) % (len(g[0]) - 600)
        s1 = sc.mutate(rng, g[0][o:o + 150], 0.01 * (1 + i % 9)) if c in (0, 1) else sc.random_dna(rng, 150)
        s2 = sc.mutate(rng, g[0][o + 300:o + 400], 0.01 * (1 + i % 7)) if c in (0, 2) else sc.random_dna(rng, 100)
        r1.append(b"@p%d/1 comment %d\n%s\n+\n%s\n" % (i, i, s1.encode(), bytes(33 + (j * 7 + i) % 40 for j in range(150))))
        r2.append(b"@p%d/2\n%s\n+\n%s\n" % (i, s2.encode(), bytes(33 + (j * 5 + i) % 40 for j in range(100))))
    il = [x for p in zip(r1, r2) for x in p]
    (d / "R1.fq").write_bytes(b"".join(r1))
    (d / "R2.fq").write_bytes(b"".join(r2))
    (d / "IL.fq").write_bytes(b"".join(il))
    out = {"SKETCH": sketch, "dir": d, "r1": r1, "r2": r2, "il": il, "R1": str(d / "R1.fq"), "R2": str(d / "R2.fq"), "IL": str(d / "IL.fq")}
    # the unpaired reports: what every expectation is computed from
    out["rep1"], out["rep2"], out["repil"] = (cli(sketch, out[k], GPU).stdout for k in ("R1", "R2", "IL"))
    out["d1"], out["d2"] = dists(out["rep1"]), dists(out["rep2"])
    assert len(out["d1"]) == len(out["d2"]) == NPAIRS
    combos = {(bool(a), bool(b)) for a, b in zip(matched(out["d1"]), matched(out["d2"]))}
    assert len(combos) == 4  # all four combinations of (mate 1, mate 2) x (matched, unmatched)
    return out


def paired_args(d, tag, which=("m", "u")):
    p = {k: d / f"{tag}.{k}" for k in ("m1", "u1", "m2", "u2", "o2")}
    a = []
    if "m" in which:
        a += ["--extract-matched", str(p["m1"]), "--extract-matched2", str(p["m2"])]
    if "u" in which:
        a += ["--extract-unmatched", str(p["u1"]), "--extract-unmatched2", str(p["u2"])]
    return p, a


@pytest.mark.parametrize("rule", ["any", "both", None])
def test_two_files(files, rule):
    d = files["dir"]
    p, a = paired_args(d, f"two.{rule}")
    r = cli(files["SKETCH"], files["R1"], GPU + ["--query2", files["R2"], "--output-path2", str(p["o2"])] + a + (["--pair-rule", rule] if rule else []))
    rule = rule or "any"  # the default
    keep = verdict(files["d1"], files["d2"], rule)
    assert 0 < keep.sum() < NPAIRS
    m1, u1, m2, u2 = (p[k].read_bytes() for k in ("m1", "u1", "m2", "u2"))
    assert (m1, u1) == split(files["r1"], keep) and (m2, u2) == split(files["r2"], keep)
    assert len(m1) + len(u1) == os.path.getsize(files["R1"]) and len(m2) + len(u2) == os.path.getsize(files["R2"])
    assert nrec(m1) == nrec(m2) == int(keep.sum()) and nrec(u1) == nrec(u2)  # the files stay in step
    assert body(r.stdout) == body(files["rep1"]) and body(p["o2"].read_bytes()) == body(files["rep2"])
    err = r.stderr.decode()
    t = re.search(r"\[timing\] extract pairs: (\d+) matched of (\d+) pairs \(rule (\w+)\), (\d+) bytes, [\d.]+ ms of kernels", err)
    assert t and t.groups() == (str(int(keep.sum())), str(NPAIRS), rule, str(len(m1) + len(u1) + len(m2) + len(u2))), err
    assert re.search(r"\[timing\] extract: \d+ matched of %d reads" % (2 * NPAIRS), err), err


@pytest.mark.parametrize("rule", ["any", "both"])
def test_interleaved(files, rule):
    d = files["dir"]
    m, u = d / f"il.{rule}.m", d / f"il.{rule}.u"
    r = cli(files["SKETCH"], files["IL"], GPU + ["--interleaved", "--pair-rule", rule, "--extract-matched", str(m), "--extract-unmatched", str(u)])
    keep = verdict(files["d1"], files["d2"], rule)
    dil = dists(files["repil"])  # the interleaved file's own unpaired report says the same
    assert np.array_equal(verdict(dil[0::2], dil[1::2], rule), keep)
    gm, gu = m.read_bytes(), u.read_bytes()
    assert (gm, gu) == split(files["il"], np.repeat(keep, 2))
    assert len(gm) + len(gu) == os.path.getsize(files["IL"]) and nrec(gm) == 2 * int(keep.sum())
    assert body(r.stdout) == body(files["repil"])
    assert re.search(r"\[timing\] extract pairs: %d matched of %d pairs \(rule %s\)" % (keep.sum(), NPAIRS, rule), r.stderr.decode())


@pytest.mark.parametrize("rule", ["any", "both"])
def test_threshold(files, rule):
    """The reports print five decimals: D goes to the midpoint of the widest gap between the sorted printed values, and no printed DIST
    may lie within 1e-4 of it, so that rounding cannot move a read across it"""
    d = files["dir"]
    both = np.concatenate([files["d1"], files["d2"]])
    vals = np.unique(both[~np.isnan(both)])
    gaps = np.diff(vals)
    D = float((vals[np.argmax(gaps)] + vals[np.argmax(gaps) + 1]) / 2)
    assert np.min(np.abs(vals - D)) > 1e-4
    keep = verdict(files["d1"], files["d2"], rule, D)
    assert (matched(both, D) != matched(both)).any() and 0 < keep.sum() < NPAIRS  # the threshold moves reads
    p, a = paired_args(d, f"th.{rule}")
    cli(files["SKETCH"], files["R1"], GPU + ["--query2", files["R2"], "--pair-rule", rule, "--extract-max", repr(D)] + a)
    assert (p["m1"].read_bytes(), p["u1"].read_bytes()) == split(files["r1"], keep)
    assert (p["m2"].read_bytes(), p["u2"].read_bytes()) == split(files["r2"], keep)
    assert not p["o2"].exists()  # --output-path2 was not given: the mates' report is not written


@pytest.mark.parametrize("which", ["m", "u"])
def test_one_file_pair_alone(files, which):
    d = files["dir"]
    p, a = paired_args(d, f"only.{which}", which)
    r = cli(files["SKETCH"], files["R1"], GPU + ["--query2", files["R2"]] + a)
    keep = verdict(files["d1"], files["d2"], "any")
    k = 0 if which == "m" else 1
    assert p[which + "1"].read_bytes() == split(files["r1"], keep)[k] and p[which + "2"].read_bytes() == split(files["r2"], keep)[k]
    other = "u" if which == "m" else "m"
    assert not p[other + "1"].exists() and not p[other + "2"].exists()
    assert body(r.stdout) == body(files["rep1"])


def test_bgzf_files_inflate_to_the_plain_ones(capi, files):
    d = files["dir"]
    p, a = paired_args(d, "z")
    r = cli(files["SKETCH"], files["R1"], GPU + ["--query2", files["R2"], "--pair-rule", "both", "--extract-bgzf", "--bgzf-member", "1024"] + a)
    assert body(r.stdout) == body(files["rep1"])  # (the report stays plain: --bgzf-out was not given)
    keep = verdict(files["d1"], files["d2"], "both")
    want = dict(zip(("m1", "u1"), split(files["r1"], keep)))
    want.update(zip(("m2", "u2"), split(files["r2"], keep)))
    for k in ("m1", "u1", "m2", "u2"):
        comp = p[k].read_bytes()
        assert comp.endswith(capi.bgzf_eof()) and comp.count(capi.bgzf_eof()) >= 1
        assert gzip.decompress(comp) == want[k] and want[k]
    il_m = d / "z.il.m"
    cli(files["SKETCH"], files["IL"], GPU + ["--interleaved", "--extract-bgzf", "--extract-matched", str(il_m)])
    assert gzip.decompress(il_m.read_bytes()) == split(files["il"], np.repeat(verdict(files["d1"], files["d2"], "any"), 2))[0]


def test_empty_files_are_created(files):
    d, g = files["dir"], sc.genome_a()[0]
    a1, a2 = d / "allm1.fq", d / "allm2.fq"
    a1.write_bytes(b"".join(b"@e%d/1\n%s\n+\n%s\n" % (i, g[100 * i:100 * i + 150].encode(), b"I" * 150) for i in range(10)))
    a2.write_bytes(b"".join(b"@e%d/2\n%s\n+\n%s\n" % (i, g[100 * i + 200:100 * i + 300].encode(), b"I" * 100) for i in range(10)))
    p, a = paired_args(d, "allm")
    cli(files["SKETCH"], a1, GPU + ["--query2", str(a2), "--output-path2", str(p["o2"])] + a)
    assert p["m1"].read_bytes() == a1.read_bytes() and p["m2"].read_bytes() == a2.read_bytes()
    assert p["u1"].exists() and p["u2"].exists() and p["u1"].read_bytes() == b"" and p["u2"].read_bytes() == b""
    assert p["o2"].read_bytes().count(b"\n") == 2 + 10
    # two empty inputs: every file is made, and holds nothing but the reports' first lines
    e1, e2 = d / "empty1.fq", d / "empty2.fq"
    e1.write_bytes(b""), e2.write_bytes(b"")
    p, a = paired_args(d, "empty")
    cli(files["SKETCH"], e1, GPU + ["--query2", str(e2), "--output-path2", str(p["o2"])] + a)
    assert all(p[k].exists() and p[k].read_bytes() == b"" for k in ("m1", "u1", "m2", "u2")) and p["o2"].read_bytes().count(b"\n") == 2


@pytest.mark.parametrize("case", ["r2-shorter", "r1-shorter", "r2-cut-short", "interleaved-odd"])
def test_unequal_record_counts(files, case):
    d = files["dir"]
    r1, r2, il = files["r1"], files["r2"], files["il"]
    q1, q2 = d / f"{case}.1.fq", d / f"{case}.2.fq"
    if case == "r2-shorter":
        q1.write_bytes(b"".join(r1)), q2.write_bytes(b"".join(r2[:-3]))
        at = (sum(map(len, r1[:-3])), sum(map(len, r2[:-3])))
    elif case == "r1-shorter":
        q1.write_bytes(b"".join(r1[:100])), q2.write_bytes(b"".join(r2))
        at = (sum(map(len, r1[:100])), sum(map(len, r2[:100])))
    elif case == "r2-cut-short":  # the last record of the mates' file lacks its last byte: no whole record, and no mate
        q1.write_bytes(b"".join(r1)), q2.write_bytes(b"".join(r2)[:-1])
        at = (sum(map(len, r1[:-1])), sum(map(len, r2[:-1])))
    else:
        q1.write_bytes(b"".join(il[:-1]))
        at = (sum(map(len, il[:-2])),)
    p, a = paired_args(d, case)
    if case == "interleaved-odd":
        r = cli(files["SKETCH"], q1, GPU + ["--interleaved", "--extract-matched", str(p["m1"])], ok=False)
        want = r"\[ERROR\] --interleaved: %s \(offset %d\): .*do not hold the same number of records" % (re.escape(str(q1)), at[0])
    else:
        r = cli(files["SKETCH"], q1, GPU + ["--query2", str(q2)] + a, ok=False)
        want = r"\[ERROR\] paired reads: %s \(offset %d\) and %s \(offset %d\) do not hold the same number of records" % (re.escape(str(q1)), at[0], re.escape(str(q2)), at[1])
    err = r.stderr.decode()
    assert r.returncode != 0 and re.search(want, err), err


@pytest.mark.parametrize("case", ["gz", "bgzf", "fasta", "gz-with-gpu-inflate", "interleaved-fasta", "q-gz"])
def test_other_inputs_are_refused_up_front(capi, files, case):
    d = files["dir"]
    out = d / f"refused.{case}"
    out.mkdir()
    raw2 = b"".join(files["r2"])
    q1, extra = files["R1"], []
    if case in ("gz", "gz-with-gpu-inflate"):
        q2 = d / f"{case}.R2.fq.gz"
        q2.write_bytes(gzip.compress(raw2))
        extra = ["--gpu-inflate"] if case == "gz-with-gpu-inflate" else []
        word = "gzip"
    elif case == "bgzf":
        q2 = d / "R2.bgzf.fq.gz"
        q2.write_bytes(capi.bgzf_deflate_host_member(raw2, 1, 3000) + capi.bgzf_eof())
        word = "BGZF"
    elif case == "q-gz":  # the first file
        q1 = d / "R1.fq.gz"
        q1.write_bytes(gzip.compress(b"".join(files["r1"])))
        q2, word = files["R2"], "gzip"
    else:
        q2 = d / f"{case}.fa"
        q2.write_bytes(b"".join(b">c%d\n%s\n" % (i, r.split(b"\n")[1]) for i, r in enumerate(files["r2"])))
        word = "FASTA"
    m1, m2 = out / "m1", out / "m2"
    if case == "interleaved-fasta":
        r = cli(files["SKETCH"], q2, GPU + ["--interleaved", "--extract-matched", str(m1)], ok=False)
        named = q2
    else:
        r = cli(files["SKETCH"], q1, GPU + extra + ["--query2", str(q2), "--extract-matched", str(m1), "--extract-matched2", str(m2)], ok=False)
        named = q1 if case == "q-gz" else q2
    err = r.stderr.decode()
    last = err.rstrip("\n").rsplit("\n", 1)[-1]
    assert r.returncode == 1 and last.startswith("[ERROR] paired reads: only plain FASTQ files are accepted") and word in last and str(named) in last, err
    assert r.stdout == b"" and not os.listdir(out)  # before anything was loaded or created
