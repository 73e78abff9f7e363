"""`krepp dist --gpu-parse` on FASTA (records found on the GPU by kr_batch_submit_fasta, krepp_main.cpp): the report is the one
`krepp dist` writes for the same input, in every report mode -- on reads as wrapped CRLF FASTA at two chunk sizes, on contigs
longer than the tiling threshold, on a contig longer than the chunk (the host takes over), on FASTA that turns into FASTQ
halfway, on a file without a final newline, and on gzip input (the host reader throughout)."""
import gzip
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT
from fasta_fuzz import wrap_body

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")


def body(path_or_text):
    t = open(path_or_text, "rb").read() if isinstance(path_or_text, str) else path_or_text
    return t.split(b"\n", 1)[1]  # (the first line names the invocation)


def dist(idx, q, extra, env=None, out=None, stderr=False):
    cmd = [EXE, "dist", "-i", idx, "-q", str(q)] + extra + (["-o", str(out)] if out else [])
    r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, **(env or {})), timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    err = r.stderr.decode()
    total = [l for l in err.splitlines() if l.startswith("Total number of sequences queried")]
    res = (body(str(out)) if out else body(r.stdout)), total
    return res + (err,) if stderr else res


def summary_close(a, b):
    la, lb = a.decode().strip().split("\n"), b.decode().strip().split("\n")
    assert la[0] == lb[0] and len(la) == len(lb)
    for x, y in zip(la[1:], lb[1:]):  # weighted counts are sums of 1/n in another order: names exactly, numbers to the last digit
        xs, ys = x.split("\t"), y.split("\t")
        assert xs[0] == ys[0]
        for u, v in zip(xs[1:], ys[1:]):
            assert abs(float(u) - float(v)) <= 2e-5, (x, y)


def check_modes(idx, q, tmp_path, envs=(None,)):
    """every report mode; the host reader's report is made once and compared with --gpu-parse under each environment"""
    for extra in ([], ["--no-multi"], ["--gpus", "1"], ["--filter"]):
        want = dist(idx, q, extra)
        assert len(want[0]) > 0
        for env in envs:
            assert dist(idx, q, extra + ["--gpu-parse"], env) == want, (extra, env)
    want = dist(idx, q, [], out=tmp_path / "a.tsv")
    ws, wt = dist(idx, q, ["--summarize"])
    for env in envs:
        assert dist(idx, q, ["--gpu-parse"], env, out=tmp_path / "b.tsv") == want
        gs, gt = dist(idx, q, ["--summarize", "--gpu-parse"], env)
        assert gt == wt
        summary_close(gs, ws)


def found_on_device(idx, q, env=None):
    """(FASTA records the device found, records queried) of one --gpu-parse run, from its KR_CLI_TIMING lines"""
    _, total, err = dist(idx, q, ["--gpu-parse"], dict(env or {}, KR_CLI_TIMING="1"), stderr=True)
    m = re.search(r"\[timing\] gpu-parse: (\d+) FASTA records found on the device", err)
    assert m, err
    return int(m.group(1)), int(total[0].rsplit(" ", 1)[1])


def fasta_of(names, seqs, wrap=60, nl=b"\r\n", comment=b" some comment"):
    return b"".join(b">" + n.encode() + comment + nl + wrap_body(bytes(s), wrap, nl) for n, s in zip(names, seqs))


@pytest.fixture(scope="module")
def toy_fasta(capi):
    names, bases, offs = capi.read_fastx(os.path.join(GOLDEN, "toy_reads.fq"))
    return names, [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(names))]


def contigs(toy_genomes, length):
    names, seqs = [], []
    for g, s in toy_genomes.items():
        for c in range(0, len(s) - length + 1, length):
            names.append("%s_c%d" % (g, c // length))
            seqs.append(s[c:c + length].tobytes())
    return names, seqs


def test_toy_reads_as_wrapped_crlf_fasta(toy_fasta, toy_index_dir, tmp_path):
    names, seqs = toy_fasta
    q = tmp_path / "toy.fa"
    q.write_bytes(fasta_of(names, seqs))
    # (long sequences among them: at 4096 bytes a chunk one of them is longer than the chunk and the host takes over there)
    check_modes(toy_index_dir, q, tmp_path, envs=({"KR_CLI_PARSE_CHUNK": "4096"}, {"KR_CLI_PARSE_CHUNK": "200000"}))
    lim = 4000
    short = [i for i in range(len(names)) if len(seqs[i]) + len(seqs[i]) // 30 + len(names[i]) + 40 < lim // 2]
    q2 = tmp_path / "short.fa"
    q2.write_bytes(fasta_of([names[i] for i in short], [seqs[i] for i in short]))
    for chunk in ("4096", "200000"):  # every chunk holds a second record start: every record is found on the device
        assert found_on_device(toy_index_dir, q2, {"KR_CLI_PARSE_CHUNK": chunk}) == (len(short), len(short))


def test_contigs_longer_than_the_tiling_threshold(toy_genomes, toy_index_dir, tmp_path):
    names, seqs = contigs(toy_genomes, 5000)
    q = tmp_path / "contigs.fa"
    q.write_bytes(fasta_of(names, seqs, wrap=80, nl=b"\n", comment=b""))
    check_modes(toy_index_dir, q, tmp_path)
    assert found_on_device(toy_index_dir, q) == (len(names), len(names))
    # a contig longer than the chunk: no second record start in the chunk, INCOMPLETE with no record, the host reader takes over
    check_modes(toy_index_dir, q, tmp_path, envs=({"KR_CLI_PARSE_CHUNK": "4096"},))
    assert found_on_device(toy_index_dir, q, {"KR_CLI_PARSE_CHUNK": "4096"}) == (0, len(names))


def test_fasta_turning_into_fastq_no_final_newline_and_gzip(synth, toy_genomes, toy_index_dir, tmp_path):
    bases, offs, names = synth.sample_reads(toy_genomes, 20000, seed=4)
    seqs = [bases[int(offs[i]):int(offs[i + 1])].tobytes() for i in range(len(names))]
    mixed = fasta_of(names[:12000], seqs[:12000], nl=b"\n")
    mixed += b"".join(b"@%s extra\n%s\n+\n%s\n" % (n.encode(), s, b"F" * len(s)) for n, s in zip(names[12000:], seqs[12000:]))
    q = tmp_path / "mixed.fa"
    q.write_bytes(mixed)
    check_modes(toy_index_dir, q, tmp_path, envs=({"KR_CLI_PARSE_CHUNK": "200000"},))  # chunks behind the stop are dropped
    dev, total = found_on_device(toy_index_dir, q, {"KR_CLI_PARSE_CHUNK": "200000"})
    assert total == 20000 and 0 < dev < 12000  # (the last FASTA record's body runs into the '@' lines: it is the host's too)
    q2 = tmp_path / "nonl.fa"
    q2.write_bytes(fasta_of(names[:3000], seqs[:3000], nl=b"\n")[:-1])
    check_modes(toy_index_dir, q2, tmp_path, envs=({"KR_CLI_PARSE_CHUNK": "100000"},))
    assert found_on_device(toy_index_dir, q2, {"KR_CLI_PARSE_CHUNK": "100000"}) == (3000, 3000)
    q3 = tmp_path / "reads.fa.gz"
    q3.write_bytes(gzip.compress(fasta_of(names[:3000], seqs[:3000])))
    check_modes(toy_index_dir, q3, tmp_path)
