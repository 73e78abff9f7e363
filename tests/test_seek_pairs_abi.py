"""The paired-read entry points of a seek batch without a device: the three symbols and two constants are declared, exported and
mirrored, NULL arguments are refused, `krepp seek --help` names the six options, and every option error of the CLI is settled in the
settings parse -- exit status 1 and its message before any device call (the sketch and the queries named here do not exist)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")


def test_symbols_declared_exported_and_mirrored(capi):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    for n in ("kr_stream_extract_defer", "kr_batch_extract_pair", "kr_fastq_pair_cut"):
        assert re.search(r"KR_API\s+int\s+" + n + r"\s*\(", hdr), n
        assert n in capi.EXPORTS and hasattr(lib, n), n
    assert re.search(r"#define\s+KR_PAIR_ANY\s+1u", hdr) and capi.KR_PAIR_ANY == 1
    assert re.search(r"#define\s+KR_PAIR_BOTH\s+2u", hdr) and capi.KR_PAIR_BOTH == 2
    for f in ("extract_defer", "extract_pair"):
        assert hasattr(capi.Stream, f), f
    assert callable(capi.fastq_pair_cut)


def test_null_arguments_are_refused(capi):
    lib = capi.load()
    assert lib.kr_stream_extract_defer(None, 1) == capi.KR_ERR_ARG
    assert b"null" in lib.kr_last_error()
    for rule in (capi.KR_PAIR_ANY, capi.KR_PAIR_BOTH, 0, 3):
        assert lib.kr_batch_extract_pair(None, None, rule) == capi.KR_ERR_ARG
    assert b"null" in lib.kr_last_error()
    n = C.c_uint32(0)
    assert lib.kr_fastq_pair_cut(None, 0, None, 0, 1, None, None, C.byref(n)) == capi.KR_ERR_ARG
    assert b"null" in lib.kr_last_error()


def test_help_names_the_options():
    r = subprocess.run([EXE, "seek", "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--query2 FILE", "--output-path2 FILE", "--extract-matched2 FILE", "--extract-unmatched2 FILE", "--interleaved", "--pair-rule any|both"):
        assert opt in r.stdout, opt
    r = subprocess.run([EXE, "dist", "--help"], capture_output=True, text=True)
    dist = r.stdout.split("krepp seek")[0]
    assert "--extract-" not in dist and "--query2" not in dist and "--interleaved" not in dist and "--pair-rule" not in dist


GPU = ["--gpu-parse", "--gpu-seek"]
M, U = ["--extract-matched", "m.fq"], ["--extract-unmatched", "u.fq"]
M2, U2 = ["--extract-matched2", "m2.fq"], ["--extract-unmatched2", "u2.fq"]
Q2 = ["--query2", "mates.fq"]
OF_SEEK = "are options of `seek`"
NEEDS = "need --gpu-parse, --gpu-seek and --extract-matched or --extract-unmatched"
ERRORS = [
    # pair options on dist or place
    ("dist", Q2, OF_SEEK),
    ("dist", ["--interleaved"], OF_SEEK),
    ("place", ["--pair-rule", "both"], OF_SEEK),
    ("place", ["--output-path2", "o2.txt"], OF_SEEK),
    ("dist", ["--extract-matched2", "m2.fq"], OF_SEEK),
    # paired reads are split on the GPU, into at least one file
    ("seek", Q2, NEEDS),
    ("seek", GPU + Q2, NEEDS),
    ("seek", GPU + ["--interleaved"], NEEDS),
    ("seek", ["--gpu-parse"] + Q2 + M + M2, "needs --gpu-parse and --gpu-seek"),
    # each ...2 file exactly when its sibling is given with --query2
    ("seek", GPU + Q2 + M, "--extract-matched with --query2 needs --extract-matched2"),
    ("seek", GPU + Q2 + U, "--extract-unmatched with --query2 needs --extract-unmatched2"),
    ("seek", GPU + Q2 + M + M2 + U, "--extract-unmatched with --query2 needs --extract-unmatched2"),
    ("seek", GPU + Q2 + M + U2, "--extract-matched with --query2 needs --extract-matched2"),
    ("seek", GPU + Q2 + M + M2 + U2, "--extract-unmatched2 needs --extract-unmatched"),
    ("seek", GPU + Q2 + U + U2 + M2, "--extract-matched2 needs --extract-matched"),
    # ... and an error without --query2
    ("seek", GPU + M + M2, "--extract-matched2 needs --query2"),
    ("seek", GPU + U + U2, "--extract-unmatched2 needs --query2"),
    ("seek", GPU + M + ["--output-path2", "o2.txt"], "--output-path2 needs --query2"),
    ("seek", GPU + M + ["--interleaved"] + M2, "--extract-matched2 needs --query2"),
    ("seek", GPU + M + ["--interleaved", "--output-path2", "o2.txt"], "--output-path2 needs --query2"),
    # --interleaved and --query2
    ("seek", GPU + Q2 + M + M2 + ["--interleaved"], "--interleaved and --query2 exclude each other"),
    # the rule
    ("seek", GPU + M + ["--pair-rule", "any"], "--pair-rule needs --query2 or --interleaved"),
    ("seek", GPU + M + ["--interleaved", "--pair-rule", "either"], "--pair-rule: any or both, not either"),
    ("seek", GPU + Q2 + M + M2 + ["--pair-rule", "ANY"], "--pair-rule: any or both, not ANY"),
    ("seek", GPU + Q2 + M + M2 + ["--pair-rule", ""], "--pair-rule: any or both, not "),
    # --query2 equal to -q
    ("seek", GPU + ["--query2", "no-such-reads"] + M + M2, "--query2 names the same file as -q: no-such-reads"),
    # a ...2 file equal to any other output file
    ("seek", GPU + Q2 + M + ["--extract-matched2", "m.fq"], "an output file is named twice: m.fq"),
    ("seek", GPU + Q2 + M + U + U2 + ["--extract-matched2", "u.fq"], "an output file is named twice: u.fq"),
    ("seek", GPU + Q2 + M + U + M2 + ["--extract-unmatched2", "m2.fq"], "an output file is named twice: m2.fq"),
    ("seek", GPU + Q2 + M + U + M2 + ["--extract-unmatched2", "m.fq"], "an output file is named twice: m.fq"),
    ("seek", GPU + Q2 + M + M2 + ["-o", "rep.txt", "--output-path2", "rep.txt"], "an output file is named twice: rep.txt"),
    ("seek", GPU + Q2 + M + M2 + ["-o", "m2.fq"], "an output file is named twice: m2.fq"),
    ("seek", GPU + Q2 + M + M2 + ["--output-path2", "m.fq"], "an output file is named twice: m.fq"),
    ("seek", GPU + Q2 + M + M2 + ["--output-path2", "m2.fq"], "an output file is named twice: m2.fq"),
    # what held before holds with pairs
    ("seek", GPU + Q2 + ["--extract-matched", "same.fq", "--extract-unmatched", "same.fq"] + M2 + U2, "name the same file: same.fq"),
    ("seek", GPU + M + ["--interleaved", "--extract-max", "2"], "--extract-max: a distance in [0, 1], not 2"),
]


@pytest.mark.parametrize("sub,extra,msg", ERRORS, ids=[f"{i}-{e[0]}" for i, e in enumerate(ERRORS)])
def test_option_errors_exit_1_before_any_device_call(tmp_path, sub, extra, msg):
    r = subprocess.run([EXE, sub, "-i", "no-such-sketch", "-q", "no-such-reads"] + extra, capture_output=True, text=True, cwd=tmp_path,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1, r.stderr
    last = r.stderr.rstrip("\n").rsplit("\n", 1)[-1]  # (behind the version and invocation lines)
    assert last.startswith("[ERROR] ") and msg in last, r.stderr
    assert r.stdout == "" and not os.listdir(tmp_path)  # nothing was loaded, no file was made
