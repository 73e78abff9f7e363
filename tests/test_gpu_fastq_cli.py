"""`krepp dist --gpu-parse` (FASTQ records found on the GPU, krepp_main.cpp): the report is the one `krepp dist` writes for the
same input, in every report mode, on clean input, on input that turns into FASTA halfway (the first early stop hands over to the
host reader, chunks behind it are dropped), on a file without a final newline, and on gzip input (the host reader throughout)."""
import gzip
import os
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")


def body(path_or_text):
    t = open(path_or_text, "rb").read() if isinstance(path_or_text, str) else path_or_text
    return t.split(b"\n", 1)[1]  # (the first line names the invocation)


def dist(idx, q, extra, env=None, out=None):
    cmd = [EXE, "dist", "-i", idx, "-q", str(q)] + extra + (["-o", str(out)] if out else [])
    r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, **(env or {})), timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    total = [l for l in r.stderr.decode().splitlines() if l.startswith("Total number of sequences queried")]
    return (body(str(out)) if out else body(r.stdout)), total


def summary_close(a, b):
    la, lb = a.decode().strip().split("\n"), b.decode().strip().split("\n")
    assert la[0] == lb[0] and len(la) == len(lb)
    for x, y in zip(la[1:], lb[1:]):  # weighted counts are sums of 1/n in another order: names exactly, numbers to the last digit
        xs, ys = x.split("\t"), y.split("\t")
        assert xs[0] == ys[0]
        for u, v in zip(xs[1:], ys[1:]):
            assert abs(float(u) - float(v)) <= 2e-5, (x, y)


def check_modes(idx, q, tmp_path, env=None):
    for extra in ([], ["--no-multi"], ["--gpus", "1"], ["--filter"]):
        want = dist(idx, q, extra)
        got = dist(idx, q, extra + ["--gpu-parse"], env)
        assert got == want, extra
    want = dist(idx, q, [], out=tmp_path / "a.tsv")
    assert dist(idx, q, ["--gpu-parse"], env, out=tmp_path / "b.tsv") == want
    ws, wt = dist(idx, q, ["--summarize"])
    gs, gt = dist(idx, q, ["--summarize", "--gpu-parse"], env)
    assert gt == wt
    summary_close(gs, ws)


def synth_fastq(synth, toy_genomes, n, seed, copies=1):
    bases, offs, names = synth.sample_reads(toy_genomes, n, seed=seed)
    out = []
    for c in range(copies):
        for i in range(n):
            s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
            out.append(b"@%s_%d extra\n%s\n+\n%s\n" % (names[i].encode(), c, s, b"F" * len(s)))
    return out


def test_toy_reads(toy_index_dir, tmp_path):
    check_modes(toy_index_dir, os.path.join(GOLDEN, "toy_reads.fq"), tmp_path)  # (long sequences among them: the host takes over)
    check_modes(toy_index_dir, os.path.join(GOLDEN, "toy_reads.fq"), tmp_path, env={"KR_CLI_PARSE_CHUNK": "4096"})


def test_fastq_turning_into_fasta_and_no_final_newline(synth, toy_genomes, toy_index_dir, tmp_path):
    recs = synth_fastq(synth, toy_genomes, 20000, seed=4)
    mixed = b"".join(recs[:12000])
    for r in recs[12000:]:
        name, seq = r.split(b"\n")[:2]
        mixed += b">" + name[1:] + b"\n" + seq + b"\n"
    q = tmp_path / "mixed.fq"
    q.write_bytes(mixed)
    check_modes(toy_index_dir, q, tmp_path, env={"KR_CLI_PARSE_CHUNK": "200000"})  # chunks behind the stop are dropped
    q2 = tmp_path / "nonl.fq"
    q2.write_bytes(b"".join(recs[:3000])[:-1])
    check_modes(toy_index_dir, q2, tmp_path, env={"KR_CLI_PARSE_CHUNK": "100000"})
    q3 = tmp_path / "reads.fq.gz"
    q3.write_bytes(gzip.compress(b"".join(recs[:3000])))
    check_modes(toy_index_dir, q3, tmp_path)


def test_one_million_reads(synth, toy_genomes, toy_index_dir, tmp_path):
    q = tmp_path / "m.fq"
    with open(q, "wb") as f:
        f.write(b"".join(synth_fastq(synth, toy_genomes, 200000, seed=9, copies=5)))
    for extra in ([], ["--no-multi"]):
        want = dist(toy_index_dir, q, extra, out=tmp_path / "a.tsv")
        got = dist(toy_index_dir, q, extra + ["--gpu-parse"], out=tmp_path / "b.tsv")
        assert got == want and want[1] == ["Total number of sequences queried: 1000000"], extra
