"""`krepp place --gpu-parse` and `krepp seek --gpu-parse` (krepp_main.cpp): the output is what the same command writes without the
flag, byte for byte after the invocation line, in every output mode of `place` -- `--summarize` included: its per-512-read sums go
by global read number, so equal bytes mean equal numbering across chunks, submits of a chunk and the hand-over to the host reader --
on clean input, with small chunks, on input that turns into FASTA halfway (the first early stop hands over, chunks behind it are
dropped), without a final newline, on FASTA, and on gzip (the host reader throughout).  The `[timing] gpu-parse:` line says how
many records the device found: without the feature the flag is ignored and there is no such line."""
import gzip
import os
import re
import subprocess

import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
USER_OLD = "(G000735195:0.0276038,G000018865:0.0228997)N2640:0.160977"
USER_NEW = "(G000735195:0.03,NEWLEAF:0.02)N2640:0.160977"
PLACE_MODES = {"jplace": [], "tabular": ["--tabular"], "summarize": ["--summarize"], "no-multi": ["--no-multi"], "tree": ["-t", "TREE"]}
# input -> (environment of the --gpu-parse run, records the device must find for `place`, for `seek`).  "all": every record of the
# file; "all-1": all but the last; (lo, hi): that many; "some": more than none; None: the host reader throughout, no gpu-parse line.
#   toy       tests/golden/toy_reads.fq, 308 clean four-line records, one of 1,200 bases.  `place` submits with KR_TILE_DEVICE: long
#             records are tiled, nothing stops the record finder.  `seek` submits with no flag: the first record of more than 1,024
#             k-mer positions stops it (KR_FASTQ_LONG) and the host reader takes the rest -- "some" is all that can be said.
#   toy/4096  the same in chunks of 4,096 bytes.  The longest record is 2.4 KB, so every chunk holds a record start whose '+' line
#             it also holds: every cut is a true record start and `place` again finds every record.
#   clean     3,000 clean 150-base reads as FASTQ: every record, for both sub-commands.
#   mixed     12,000 FASTQ records, then FASTA: the records in front of the first FASTA record, less at most what the chunk that
#             stopped there and the chunks behind it (dropped) held.
#   nonl      no final newline: the last record is not complete for the record finder (it counts lines), the host reader takes it.
#   fasta     3,000 clean two-line FASTA records: every record.
#   gz        gzip: the host reader.
INPUTS = {"toy": ({}, "all", "some"), "toy/4096": ({"KR_CLI_PARSE_CHUNK": "4096"}, "all", "some"),
          "clean": ({"KR_CLI_PARSE_CHUNK": "100000"}, "all", "all"), "mixed": ({"KR_CLI_PARSE_CHUNK": "200000"}, (11000, 12000), (11000, 12000)),
          "nonl": ({"KR_CLI_PARSE_CHUNK": "100000"}, "all-1", "all-1"), "fasta": ({"KR_CLI_PARSE_CHUNK": "100000"}, "all", "all"),
          "gz": ({}, None, None)}


def run(sub, idx, q, extra, env=None):
    cmd = [EXE, sub, "-i", idx, "-q", str(q)] + extra
    r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, KR_CLI_TIMING="1", **(env or {})), timeout=600)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    out = r.stdout
    if sub == "place" and "--tabular" not in extra and "--summarize" not in extra:
        out = re.sub(rb'"invocation"\s*:\s*"[^"]*"', b'"invocation": ""', out)  # (jplace names the invocation in its metadata)
    else:
        out = out.split(b"\n", 1)[1]  # (the first line names the invocation)
    total = int(re.search(r"Total number of sequences queried: (\d+)", err).group(1))
    m = re.search(r"\[timing\] gpu-parse: (\d+) (FASTA|FASTQ) records found on the device", err)
    return out, total, (int(m.group(1)) if m else None)


@pytest.fixture(scope="module")
def files(synth, toy_genomes, tmp_path_factory, capi):
    d = tmp_path_factory.mktemp("pp")
    bases, offs, names = synth.sample_reads(toy_genomes, 20000, seed=4)
    recs = []
    for i in range(20000):
        s = bases[int(offs[i]):int(offs[i + 1])].tobytes()
        recs.append(b"@%s extra\n%s\n+\n%s\n" % (names[i].encode(), s, b"F" * len(s)))

    def as_fasta(r):
        name, seq = r.split(b"\n")[:2]
        return b">" + name[1:] + b"\n" + seq + b"\n"

    out = {"toy": os.path.join(GOLDEN, "toy_reads.fq"), "toy/4096": os.path.join(GOLDEN, "toy_reads.fq")}
    for key, name, data in (("mixed", "mixed.fq", b"".join(recs[:12000]) + b"".join(as_fasta(r) for r in recs[12000:])),
                            ("nonl", "nonl.fq", b"".join(recs[:3000])[:-1]), ("clean", "clean.fq", b"".join(recs[:3000])), ("fasta", "reads.fa", b"".join(as_fasta(r) for r in recs[:3000])),
                            ("gz", "reads.fq.gz", gzip.compress(b"".join(recs[:3000])))):
        (d / name).write_bytes(data)
        out[key] = str(d / name)
    nwk = open(os.path.join(GOLDEN, "tree_toy.nwk")).read()
    assert USER_OLD in nwk
    (d / "user.nwk").write_text(nwk.replace(USER_OLD, USER_NEW))
    out["TREE"] = str(d / "user.nwk")
    g0 = next(iter(toy_genomes.values()))
    (d / "g0.fa").write_bytes(b">g0\n" + bytes(g0) + b"\n")
    capi.build_sketch(d / "g0.fa", d / "g0.skc")
    out["SKETCH"] = str(d / "g0.skc")
    return out


def check(sub, idx, files, inp, extra):
    env, on_device = INPUTS[inp][0], INPUTS[inp][1 if sub == "place" else 2]
    extra = [files["TREE"] if x == "TREE" else x for x in extra]
    want, want_total, none = run(sub, idx, files[inp], extra)
    assert none is None and want_total > 0 and len(want) > 100
    got, total, found = run(sub, idx, files[inp], extra + ["--gpu-parse"], env)
    assert total == want_total
    assert got == want
    print(sub, inp, extra, "records found on the device:", found, "of", total)
    if on_device is None:
        assert found is None, "gzip input went to the record finder"
        return
    assert found is not None and 0 < found <= total, "no record was found on the device: the flag was ignored"
    if on_device == "all":
        assert found == total
    elif on_device == "all-1":
        assert found == total - 1
    elif on_device != "some":
        assert on_device[0] <= found <= on_device[1]


@pytest.mark.parametrize("mode", list(PLACE_MODES))
@pytest.mark.parametrize("inp", list(INPUTS))
def test_place(toy_index_dir, files, inp, mode):
    check("place", toy_index_dir, files, inp, PLACE_MODES[mode])


@pytest.mark.parametrize("inp", list(INPUTS))
def test_seek(files, inp):
    check("seek", files["SKETCH"], files, inp, [])


@pytest.mark.parametrize("mode", ["jplace", "summarize"])
def test_a_batch_over_capacity_hands_over_at_its_first_record(toy_index_dir, files, mode):
    """KR_DEBUG_CLI_RECORDS: streams whose batches hold 20,000 records.  At the default chunk size the record finder's first batch is the
    12,000 FASTQ records in front of the first FASTA record; it ends in KR_ERR_CAPACITY, so the host reader takes the file from that
    batch's first record -- the first byte -- and splits its own batches until they fit.  Same bytes, and no record counted as found
    on the device (12,000 would be, had the batch fitted: then this test's premise is gone and it fails)."""
    env = {"KR_DEBUG_CLI_RECORDS": "20000"}
    want, want_total, _ = run("place", toy_index_dir, files["mixed"], PLACE_MODES[mode], env)
    got, total, found = run("place", toy_index_dir, files["mixed"], PLACE_MODES[mode] + ["--gpu-parse"], env)
    assert got == want and total == want_total == 20000
    assert found == 0
