"""`krepp dist|place|seek --gpu-parse` on block-gzipped input (krepp_main.cpp: Run::read_chunks_bgzf): the members are inflated on the
GPU and the output is what the same command writes without the flag, byte for byte after the invocation line -- with chunks whose
cuts fall inside members and with chunks smaller than a member, on input that turns into FASTA halfway (the hand-over is a BGZF
virtual offset), without a final newline, with an ordinary gzip member appended, and with a file cut short (a non-zero exit).  The
`[timing] gpu-parse:` line says how many records the device found: without the feature there is no such line for BGZF input."""
import gzip
import os
import subprocess

import pytest

import bgzf_cases as bc
from test_gpu_fastq_cli import dist, summary_close
from test_gpu_place_parsed_cli import EXE, run

pytestmark = pytest.mark.gpu

CHUNKS = {"cuts-inside-members": "100000", "smaller-than-a-member": "4096"}
NREADS = 3000


@pytest.fixture(scope="module")
def files(synth, toy_genomes, tmp_path_factory, capi):
    d = tmp_path_factory.mktemp("bgzf")
    bases, offs, names = synth.sample_reads(toy_genomes, 6000, seed=4)
    recs = []
    for i in range(6000):
        s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
        recs.append(b"@%s extra\n%s\n+\n%s\n" % (names[i].encode(), s, b"F" * len(s)))

    def as_fasta(r):
        name, seq = r.split(b"\n")[:2]
        return b">" + name[1:] + b"\n" + seq + b"\n"

    clean = b"".join(recs[:NREADS])
    tail = b"".join(recs[NREADS:NREADS + 40])
    out = {}
    for key, data in (("clean", bc.members(clean)[0]), ("fasta", bc.members(b"".join(as_fasta(r) for r in recs[:NREADS]))[0]),
                      ("mixed", bc.members(b"".join(recs[:3600]) + b"".join(as_fasta(r) for r in recs[3600:]))[0]),
                      ("nonl", bc.members(clean[:-1])[0]), ("appended", bc.members(clean)[0] + gzip.compress(tail)),
                      ("appended-no-eof", bc.members(clean, eof=False)[0] + gzip.compress(tail)),
                      ("truncated", bc.members(clean)[0][:-(len(bc.EOF_MEMBER) + 100)])):
        (d / (key + ".gz")).write_bytes(data)
        out[key] = str(d / (key + ".gz"))
    g0 = next(iter(toy_genomes.values()))
    (d / "g0.fa").write_bytes(b">g0\n" + bytes(g0) + b"\n")
    capi.build_sketch(d / "g0.fa", d / "g0.skc")
    out["SKETCH"] = str(d / "g0.skc")
    return out


def check(sub, idx, q, extra, env, found_want):
    want, want_total, none = run(sub, idx, q, extra)
    assert none is None and want_total > 0 and len(want) > 100
    got, total, found = run(sub, idx, q, extra + ["--gpu-parse"], env)
    assert total == want_total and got == want
    assert found is not None, "no gpu-parse line: the flag was ignored for BGZF input"
    if isinstance(found_want, tuple):
        assert found_want[0] <= found <= found_want[1], found
    else:
        assert found == (total if found_want == "all" else found_want), (found, total)


# the report modes of test_gpu_fastq_cli.check_modes, one case each
DIST_MODES = {"default": [], "no-multi": ["--no-multi"], "gpus-1": ["--gpus", "1"], "filter": ["--filter"], "to-a-file": "FILE", "summarize": ["--summarize"]}


@pytest.mark.parametrize("chunk", list(CHUNKS))
@pytest.mark.parametrize("mode", list(DIST_MODES))
def test_dist_in_every_report_mode(toy_index_dir, files, tmp_path, mode, chunk):
    env, q = {"KR_CLI_PARSE_CHUNK": CHUNKS[chunk]}, files["clean"]
    if mode == "to-a-file":
        assert dist(toy_index_dir, q, ["--gpu-parse"], env, out=tmp_path / "b.tsv") == dist(toy_index_dir, q, [], out=tmp_path / "a.tsv")
    elif mode == "summarize":
        (ws, wt), (gs, gt) = dist(toy_index_dir, q, DIST_MODES[mode]), dist(toy_index_dir, q, DIST_MODES[mode] + ["--gpu-parse"], env)
        assert gt == wt
        summary_close(gs, ws)
    else:
        check("dist", toy_index_dir, q, DIST_MODES[mode], env, "all")


@pytest.mark.parametrize("chunk", list(CHUNKS))
@pytest.mark.parametrize("mode", ["jplace", "tabular", "summarize"])
def test_place(toy_index_dir, files, mode, chunk):
    extra = {"jplace": [], "tabular": ["--tabular"], "summarize": ["--summarize"]}[mode]
    check("place", toy_index_dir, files["clean"], extra, {"KR_CLI_PARSE_CHUNK": CHUNKS[chunk]}, "all")


@pytest.mark.parametrize("chunk", list(CHUNKS))
@pytest.mark.parametrize("gpu_seek", [False, True], ids=["host-seek", "gpu-seek"])
def test_seek(files, gpu_seek, chunk):
    check("seek", files["SKETCH"], files["clean"], ["--gpu-seek"] if gpu_seek else [], {"KR_CLI_PARSE_CHUNK": CHUNKS[chunk]}, "all")


@pytest.mark.parametrize("chunk", list(CHUNKS))
def test_fasta(toy_index_dir, files, chunk):
    check("dist", toy_index_dir, files["fasta"], [], {"KR_CLI_PARSE_CHUNK": CHUNKS[chunk]}, "all")


@pytest.mark.parametrize("sub", ["dist", "place", "seek"])
def test_fastq_that_turns_into_fasta_hands_over_at_a_virtual_offset(toy_index_dir, files, sub):
    """the chunk that holds the first FASTA record stops there and the chunks behind it are dropped: the device's count is the
    3,600 FASTQ records less at most what that chunk and the ones behind it held"""
    idx = files["SKETCH"] if sub == "seek" else toy_index_dir
    check(sub, idx, files["mixed"], [], {"KR_CLI_PARSE_CHUNK": "100000"}, (3600 - 400, 3600))


def test_no_final_newline(toy_index_dir, files):
    check("dist", toy_index_dir, files["nonl"], [], {"KR_CLI_PARSE_CHUNK": "100000"}, NREADS - 1)


@pytest.mark.parametrize("sub", ["dist", "place"])
@pytest.mark.parametrize("key", ["appended", "appended-no-eof"])
def test_an_ordinary_gzip_member_appended(toy_index_dir, files, key, sub):
    """the chunk reader ends where the BGZF members do; the host reader reads the gzip member"""
    if sub == "dist":
        check("dist", toy_index_dir, files[key], [], {"KR_CLI_PARSE_CHUNK": "100000"}, NREADS)
    else:
        check("place", toy_index_dir, files[key], ["--summarize"], {"KR_CLI_PARSE_CHUNK": "4096"}, NREADS)


def test_a_truncated_file_is_an_error(toy_index_dir, files):
    r = subprocess.run([EXE, "dist", "-i", toy_index_dir, "-q", files["truncated"], "--gpu-parse"], capture_output=True, timeout=600,
                       env=dict(os.environ, KR_CLI_PARSE_CHUNK="100000"))
    assert r.returncode == 1 and b"block-gzipped" in r.stderr and b"truncated.gz" in r.stderr, (r.returncode, r.stderr.decode())
