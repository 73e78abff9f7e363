"""`krepp` on an input of about nineteen batches for two workers: the ways rows reach the output that the one-batch CLI tests do not
take.  Workers placing their device text side by side in a regular file (pwrite), the same written in turn (KR_CLI_SERIAL_WRITE),
jobs that own copies of the reader's batch (KR_CLI_COPY_BATCHES), rows formatted on the host and written by the writer thread
(KR_CLI_HOST_TEXT), the tear-down path (KR_CLI_CLEAN_EXIT), and chunks of raw bytes parsed on the device (--gpu-parse): the
bytes are the oracle's rows of the toy reads, once per repetition, in input order."""
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
REPS = 60


def renamed(rows, names, rep):
    """the rows of the toy reads as those of repetition `rep`: SEQ_ID -> SEQ_ID_rep (other lines as they are)"""
    return [l.split("\t", 1)[0] + f"_{rep}\t" + l.split("\t", 1)[1] if l.split("\t", 1)[0] in names else l for l in rows]


@pytest.fixture(scope="module")
def big_fq(toy_reads, tmp_path_factory):
    names, bases, offs = toy_reads
    recs = [(nm.encode(), bytes(bases[int(offs[i]):int(offs[i + 1])])) for i, nm in enumerate(names)]
    assert max(len(t) for _, t in recs) == 1200
    fq = tmp_path_factory.mktemp("cli_paths") / "big.fq"
    with open(fq, "wb") as f:
        for r in range(REPS):
            f.write(b"".join(b"@%s_%d some comment\n%s\n+\n%s\n" % (nm, r, t, b"I" * len(t)) for nm, t in recs))
    assert len(names) * REPS == 18480
    return fq


@pytest.fixture(scope="module")
def dist_rows(po, toy_index_dir, toy_reads):
    names, bases, offs = toy_reads
    one = po.Index(toy_index_dir).dist(bases, offs, names, po.params(collect=4))["text"].splitlines()
    assert len(one) > len(names)
    return [row for rep in range(REPS) for row in renamed(one, set(names), rep)]


def run(args, env):
    r = subprocess.run([EXE] + args, capture_output=True, env=dict(os.environ, KR_CLI_BATCH_READS="1000", KR_CLI_TIMING="1", **env), timeout=120)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert "Total number of sequences queried: 18480" in err, err
    return r.stdout, err


@pytest.mark.parametrize("case", ["pwrite", "serial-write", "copy-batches", "host-text", "clean-exit", "gpu-parse"])
def test_dist_to_a_file_from_many_batches(case, big_fq, dist_rows, toy_index_dir, tmp_path):
    env = {"pwrite": {}, "serial-write": dict(KR_CLI_SERIAL_WRITE="1"), "copy-batches": dict(KR_CLI_COPY_BATCHES="1"),
           "host-text": dict(KR_CLI_HOST_TEXT="1"), "clean-exit": dict(KR_CLI_CLEAN_EXIT="1"),
           "gpu-parse": dict(KR_CLI_PARSE_CHUNK="65536")}[case]
    out = tmp_path / "rows.tsv"
    stdout, err = run(["dist", "-i", toy_index_dir, "-q", str(big_fq), "-o", str(out)] + (["--gpu-parse"] if case == "gpu-parse" else []), env)
    assert stdout == b""
    lines = out.read_text().splitlines()
    assert lines[1] == "SEQ_ID\tREFERENCE_NAME\tDIST" and lines[0].startswith("# software: krepp")
    assert lines[2:] == dist_rows
    assert int(re.search(r"end of input at \S+ s \((\d+) batches\)", err).group(1)) >= 19, err  # (batches of at most 1,000 reads)
    dev, host = map(int, re.search(r"report text: (\d+) batches written from device text, (\d+) through the host formatter", err).groups())
    assert (dev == 0 and host >= 19) if case == "host-text" else dev >= 19, err
    if case == "gpu-parse":
        assert int(re.search(r"gpu-parse: (\d+) FASTQ records found on the device", err).group(1)) > 0, err
    if case == "clean-exit":
        assert "[timing] tear-down" in err, err


def test_place_tabular_to_a_file_from_many_batches(big_fq, toy_reads, toy_index_dir, tmp_path):
    """`place --tabular -o`: the rows of the toy reads placed as one batch, once per repetition"""
    names = set(toy_reads[0])
    one = subprocess.run([EXE, "place", "-i", toy_index_dir, "-q", os.path.join(GOLDEN, "toy_reads.fq"), "--tabular"], capture_output=True, timeout=120)
    assert one.returncode == 0, one.stderr.decode()
    rows = one.stdout.decode().splitlines()[1:]  # (the first line names the invocation)
    head = [l for l in rows if l.split("\t", 1)[0] not in names]
    body = [l for l in rows if l.split("\t", 1)[0] in names]
    assert len(body) >= 250 and rows == head + body
    out = tmp_path / "placed.tsv"
    run(["place", "-i", toy_index_dir, "-q", str(big_fq), "--tabular", "-o", str(out)], {})
    assert out.read_text().splitlines()[1:] == head + [row for rep in range(REPS) for row in renamed(body, names, rep)]
