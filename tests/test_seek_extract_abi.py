"""The extract entry points of a seek batch without a device: the five symbols are declared, exported and mirrored, NULL arguments are
refused, `krepp seek --help` names the four options, and every option error of the CLI is settled in the settings parse -- exit
status 1 and its message before any device call (the sketch and the query named here do not exist)."""
import ctypes as C
import os
import re
import subprocess

import pytest

from conftest import ROOT

NAMES = ("kr_stream_extract_enable", "kr_stream_extract_max", "kr_batch_collect_extract", "kr_batch_collect_extract_bgzf", "kr_debug_extract_ms")
EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")


def test_symbols_declared_exported_and_mirrored(capi):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    for n in NAMES:
        assert re.search(r"KR_API\s+int\s+" + n + r"\s*\(", hdr), n
        assert n in capi.EXPORTS and hasattr(lib, n), n
    assert re.search(r"#define\s+KR_EXTRACT_MATCHED\s+1u", hdr) and capi.KR_EXTRACT_MATCHED == 1
    assert re.search(r"#define\s+KR_EXTRACT_UNMATCHED\s+2u", hdr) and capi.KR_EXTRACT_UNMATCHED == 2
    assert "typedef struct kr_extract_view" in hdr
    # two 32-bit counts, two byte counts, two pointers, two lengths
    assert C.sizeof(capi.KrExtractView) == 2 * 4 + 2 * 8 + 2 * 8 + 2 * 8
    assert [f[0] for f in capi.KrExtractView._fields_] == ["nreads", "nmatched", "matched_bytes", "unmatched_bytes", "matched", "unmatched",
                                                           "matched_len", "unmatched_len"]
    for f in ("extract_enable", "extract_max", "collect_extract", "collect_extract_bgzf", "extract_ms"):
        assert hasattr(capi.Stream, f), f


def test_null_arguments_are_refused(capi):
    lib = capi.load()
    v = capi.KrExtractView()
    ms = C.c_float(0)
    assert lib.kr_stream_extract_enable(None, float("nan")) == capi.KR_ERR_ARG
    assert lib.kr_stream_extract_max(None, 0.1) == capi.KR_ERR_ARG
    assert lib.kr_batch_collect_extract(None, 3, C.byref(v)) == capi.KR_ERR_ARG
    assert lib.kr_batch_collect_extract_bgzf(None, 3, 1, C.byref(v)) == capi.KR_ERR_ARG
    assert lib.kr_debug_extract_ms(None, C.byref(ms)) == capi.KR_ERR_ARG
    assert b"null" in lib.kr_last_error()


def test_help_names_the_options():
    r = subprocess.run([EXE, "seek", "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for opt in ("--extract-matched FILE", "--extract-unmatched FILE", "--extract-max D", "--extract-bgzf"):
        assert opt in r.stdout, opt
    r = subprocess.run([EXE, "dist", "--help"], capture_output=True, text=True)
    assert "--extract-" not in r.stdout.split("krepp seek")[0]


GPU = ["--gpu-parse", "--gpu-seek"]
ERRORS = [
    ("dist", ["--extract-matched", "m.fq"], "options of `seek`"),
    ("place", GPU[:1] + ["--extract-bgzf"], "options of `seek`"),
    ("seek", ["--extract-matched", "m.fq"], "needs --gpu-parse and --gpu-seek"),
    ("seek", ["--gpu-parse", "--extract-unmatched", "u.fq"], "needs --gpu-parse and --gpu-seek"),
    ("seek", ["--gpu-seek", "--extract-matched", "m.fq"], "needs --gpu-parse and --gpu-seek"),
    ("seek", GPU + ["--extract-max", "0.1"], "need --extract-matched or --extract-unmatched"),
    ("seek", GPU + ["--extract-bgzf"], "need --extract-matched or --extract-unmatched"),
    ("seek", GPU + ["--extract-matched", "m.fq", "--extract-max", "1.5"], "--extract-max: a distance in [0, 1], not 1.5"),
    ("seek", GPU + ["--extract-matched", "m.fq", "--extract-max", "-0.1"], "--extract-max: a distance in [0, 1], not -0.1"),
    ("seek", GPU + ["--extract-matched", "m.fq", "--extract-max", "abc"], "--extract-max: a distance in [0, 1], not abc"),
    ("seek", GPU + ["--extract-matched", "m.fq", "--extract-max", "nan"], "--extract-max: a distance in [0, 1], not nan"),
    ("seek", GPU + ["--extract-matched", "same.fq", "--extract-unmatched", "same.fq"], "name the same file: same.fq"),
    ("seek", GPU + ["--extract-matched", "m.fq", "-o", "m.fq"], "also the report's (-o): m.fq"),
    ("seek", GPU + ["--extract-unmatched", "u.fq", "-o", "u.fq"], "also the report's (-o): u.fq"),
    ("seek", GPU + ["--bgzf-level", "2"], "--bgzf-level needs --bgzf-out"),  # as ever without --bgzf-out or --extract-bgzf
    ("seek", GPU + ["--extract-matched", "m.fq", "--bgzf-member", "4096"], "--bgzf-member needs --bgzf-out"),
    ("seek", GPU + ["--extract-matched", "m.fq", "--extract-bgzf", "--bgzf-level", "3"], "--bgzf-level: 1 (fixed Huffman codes) or 2 (dynamic codes), not 3"),
]


@pytest.mark.parametrize("sub,extra,msg", ERRORS, ids=[f"{i}-{e[0]}" for i, e in enumerate(ERRORS)])
def test_option_errors_exit_1_before_any_device_call(tmp_path, sub, extra, msg):
    r = subprocess.run([EXE, sub, "-i", "no-such-sketch", "-q", "no-such-reads"] + extra, capture_output=True, text=True, cwd=tmp_path,
                       env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 1, r.stderr
    last = r.stderr.rstrip("\n").rsplit("\n", 1)[-1]  # (behind the version and invocation lines)
    assert last.startswith("[ERROR] ") and msg in last, r.stderr
    assert r.stdout == "" and not os.listdir(tmp_path)  # nothing was loaded, no file was made
