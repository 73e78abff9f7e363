"""`krepp dist|place|seek --gpu-parse --gpu-inflate` on ordinary gzip input (krepp_main.cpp: Run::read_chunks_gzip): the file is
inflated on the GPU (kr_gzdev_read), its records are found there, and the output is what the same command writes without the flags,
byte for byte after the invocation line -- with several super-chunks and several chunks per super-chunk, on FASTQ and FASTA, on
input that turns into FASTA halfway (the hand-over through kr_fastx_open_at_gzip), and with a file cut short (exit status 1).  The
`[timing]` lines say how many records the device found and that no stretch went through a host range.  `--gpu-inflate` needs
`--gpu-parse`; `--gpu-parse` alone leaves ordinary gzip with the host reader."""
import gzip
import os
import re
import subprocess

import pytest

from test_gpu_fastq_cli import dist, summary_close
from test_gpu_place_parsed_cli import EXE, run

pytestmark = pytest.mark.gpu

NREADS = 3000
FLAGS = ["--gpu-parse", "--gpu-inflate"]
# gzip.compress cuts this text (about 160 KB compressed) into blocks of about 30 KB: super-chunks of 70,000 bytes hold two whole ones
# (a sub-chunk links), the file is several super-chunks, and a super-chunk inflates to several chunks
ENV = {"KR_GZDEV_SUPER": "70000", "KR_GZDEV_SUB": "4096", "KR_CLI_PARSE_CHUNK": "50000"}


@pytest.fixture(scope="module")
def files(synth, toy_genomes, tmp_path_factory, capi):
    d = tmp_path_factory.mktemp("gzcli")
    bases, offs, names = synth.sample_reads(toy_genomes, 6000, seed=4)
    recs = []
    for i in range(6000):
        s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
        recs.append(b"@%s extra\n%s\n+\n%s\n" % (names[i].encode(), s, b"F" * len(s)))

    def as_fasta(r):
        name, seq = r.split(b"\n")[:2]
        return b">" + name[1:] + b"\n" + seq + b"\n"

    clean = b"".join(recs[:NREADS])
    out = {}
    for key, data in (("clean", gzip.compress(clean)), ("fasta", gzip.compress(b"".join(as_fasta(r) for r in recs[:NREADS]))),
                      ("mixed", gzip.compress(b"".join(recs[:3600]) + b"".join(as_fasta(r) for r in recs[3600:]))),
                      ("truncated", gzip.compress(clean)[:-5000])):
        (d / (key + ".fq.gz")).write_bytes(data)
        out[key] = str(d / (key + ".fq.gz"))
    g0 = next(iter(toy_genomes.values()))
    (d / "g0.fa").write_bytes(b">g0\n" + bytes(g0) + b"\n")
    capi.build_sketch(d / "g0.fa", d / "g0.skc")
    out["SKETCH"] = str(d / "g0.skc")
    return out


def inflate_line(sub, idx, q, extra):
    r = subprocess.run([EXE, sub, "-i", idx, "-q", q] + extra + FLAGS, capture_output=True, env=dict(os.environ, KR_CLI_TIMING="1", **ENV), timeout=600)
    m = re.search(r"\[timing\] gpu-inflate: (\d+) super-chunks, (\d+) sub-chunks linked, (\d+) without a start, (\d+) dropped, host ranges (\d+);", r.stderr.decode())
    assert r.returncode == 0, r.stderr.decode()
    assert m, r.stderr.decode()
    return [int(x) for x in m.groups()]


def check(sub, idx, q, extra, found_want):
    want, want_total, none = run(sub, idx, q, extra)
    assert none is None and want_total > 0 and len(want) > 100
    got, total, found = run(sub, idx, q, extra + FLAGS, ENV)
    assert total == want_total and got == want
    supers, linked, _, _, host_ranges = inflate_line(sub, idx, q, extra)
    assert supers >= 2 and host_ranges == 0, "the run passed through a host range"
    assert found is not None, "no gpu-parse line: the flags were ignored for gzip input"
    if isinstance(found_want, tuple):
        assert found_want[0] <= found <= found_want[1], found
    else:
        assert found == total, (found, total)


@pytest.mark.parametrize("mode", ["default", "no-multi", "summarize"])
def test_dist(toy_index_dir, files, mode):
    if mode == "summarize":
        (ws, wt), (gs, gt) = dist(toy_index_dir, files["clean"], ["--summarize"]), dist(toy_index_dir, files["clean"], ["--summarize"] + FLAGS, ENV)
        assert gt == wt
        summary_close(gs, ws)
    else:
        check("dist", toy_index_dir, files["clean"], {"default": [], "no-multi": ["--no-multi"]}[mode], "all")


def test_the_timing_line_counts_super_chunks_and_no_host_range(toy_index_dir, files):
    supers, linked, _, _, host_ranges = inflate_line("dist", toy_index_dir, files["clean"], ["--no-multi"])
    print(supers, linked, host_ranges)
    assert supers >= 2 and linked >= 1 and host_ranges == 0


@pytest.mark.parametrize("mode", ["jplace", "tabular"])
def test_place(toy_index_dir, files, mode):
    check("place", toy_index_dir, files["clean"], {"jplace": [], "tabular": ["--tabular"]}[mode], "all")


def test_seek(files):
    check("seek", files["SKETCH"], files["clean"], [], "all")


def test_fasta(toy_index_dir, files):
    check("dist", toy_index_dir, files["fasta"], [], "all")


def test_fastq_that_turns_into_fasta_hands_over_at_an_inflated_offset(toy_index_dir, files):
    """the chunk that holds the first FASTA record stops there and the chunks behind it are dropped: kr_fastx_open_at_gzip takes over
    from the inflater's restart point in front of the stop"""
    check("dist", toy_index_dir, files["mixed"], [], (3600 - 600, 3600))


def test_a_truncated_file_is_an_error(toy_index_dir, files):
    r = subprocess.run([EXE, "dist", "-i", toy_index_dir, "-q", files["truncated"]] + FLAGS, capture_output=True, timeout=600, env=dict(os.environ, **ENV))
    assert r.returncode == 1 and b"damaged gzip file" in r.stderr and b"truncated.fq.gz" in r.stderr, (r.returncode, r.stderr.decode())


def test_gpu_inflate_needs_gpu_parse(toy_index_dir, files):
    r = subprocess.run([EXE, "dist", "-i", toy_index_dir, "-q", files["clean"], "--gpu-inflate"], capture_output=True, timeout=600)
    assert r.returncode != 0 and b"--gpu-inflate needs --gpu-parse" in r.stderr


def test_gpu_parse_alone_leaves_gzip_with_the_host_reader(toy_index_dir, files):
    assert run("dist", toy_index_dir, files["clean"], ["--gpu-parse"])[2] is None
