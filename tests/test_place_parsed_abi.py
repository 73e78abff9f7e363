"""kr_place_stream_parsed / kr_debug_place_ids (include/krepp_amd.h) and `krepp place|seek --gpu-parse`, as far as no device is needed:
the symbols are declared and exported, null arguments are KR_ERR_ARG, and the CLI's help lists the flag for both sub-commands."""
import ctypes as C
import os
import re
import subprocess

from conftest import ROOT


def test_symbols_are_declared_and_exported(capi):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    declared = set(re.findall(r"KR_API\s+[\w\s\*]+?\b(kr_\w+)\s*\(", hdr))
    for sym in ("kr_place_stream_parsed", "kr_debug_place_ids"):
        assert sym in declared and sym in capi.EXPORTS and hasattr(lib, sym), sym


def test_null_arguments_are_argument_errors(capi):
    lib = capi.load()
    prev, txt, ln = C.c_int(0), C.c_void_p(), C.c_uint64()
    raw = (C.c_uint8 * 16)()
    p = capi.default_params()
    rc = lib.kr_place_stream_parsed(None, None, None, None, raw, C.byref(p), 0, C.byref(prev), C.byref(txt), C.byref(ln), None, None)
    assert rc == capi.KR_ERR_ARG and b"kr_place_stream_parsed" in lib.kr_last_error()
    assert lib.kr_place_stream_parsed(None, None, None, None, None, None, 0, None, None, None, None, None) == capi.KR_ERR_ARG
    ids, off = (C.c_char * 16)(), (C.c_uint32 * 4)()
    assert lib.kr_debug_place_ids(None, ids, off) == capi.KR_ERR_ARG and b"kr_debug_place_ids" in lib.kr_last_error()
    assert lib.kr_debug_place_ids(None, None, None) == capi.KR_ERR_ARG


def test_cli_help_lists_gpu_parse_for_place_and_seek():
    exe = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
    for sub in ("place", "seek"):
        out = subprocess.run([exe, sub, "--help"], capture_output=True).stdout.decode()
        assert "krepp " + sub in out and "--gpu-parse" in out and "records found on the GPU (identical output" in out, out
