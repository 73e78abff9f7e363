"""The device inflater of ordinary gzip files, as far as no device is needed: the four stages' serial twin (csrc/kr_inflate_sym.h
and csrc/kr_gzip_super.h through kr_debug_gzdev_inflate_host) against zlib, on every kind of stream, cut and damage in gzip_cases.py,
and the host reader opened at an inflated offset (kr_fastx_open_at_gzip).  Every comparison is byte equality with what zlib gives.
The conditions on fixtures A and B are asserted here, so a fixture that breaks them never reaches a GPU."""
import ctypes as C
import os
import re
import zlib

import pytest

import gzip_cases as gc
from conftest import ROOT

NEW = ["kr_gzdev_open", "kr_gzdev_close", "kr_gzdev_read", "kr_gzdev_point", "kr_gzdev_counters", "kr_fastx_open_at_gzip", "kr_debug_gzdev_inflate",
       "kr_debug_gzdev_inflate_host", "kr_debug_gzdev_point_host"]
CASES = {c[0]: c for c in gc.valid_cases() + gc.seam_cases()}


def twin(capi, case):
    _, gz, sub, ratio, max_comp = case
    return capi.gzdev_inflate(gz, sub=sub, ratio=ratio, max_comp=max_comp)


def test_the_symbols_are_declared_and_exported_and_reject_bad_arguments(capi):
    lib = capi.load()
    hdr = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    declared = set(re.findall(r"KR_API\s+[\w\s\*]+?\b(kr_\w+)\s*\(", hdr))
    for sym in NEW:
        assert sym in declared and sym in capi.EXPORTS and hasattr(lib, sym), sym
    h, n, pt = C.c_void_p(), C.c_uint64(0), capi.KrGzipPoint()
    assert lib.kr_gzdev_open(None, 0, 1 << 20, 1024, 16, 4, C.byref(h)) == capi.KR_ERR_ARG
    assert lib.kr_gzdev_open(b"/nonexistent.gz", 0, 1 << 20, 8, 16, 4, C.byref(h)) == capi.KR_ERR_ARG  # sub_bytes below 64
    assert lib.kr_gzdev_read(None, None, 0, C.byref(n)) == capi.KR_ERR_ARG
    assert lib.kr_gzdev_point(None, 0, C.byref(pt)) == capi.KR_ERR_ARG
    assert lib.kr_gzdev_counters(None, None) == capi.KR_ERR_ARG
    assert lib.kr_fastx_open_at_gzip(None, 0, None, C.byref(h)) == capi.KR_ERR_ARG
    with pytest.raises(capi.KrError) as e:
        capi.gzdev_inflate(gc.fixture_b(), sub=8)
    assert e.value.code == capi.KR_ERR_ARG
    with pytest.raises(capi.KrError) as e:
        capi.gzdev_inflate(gc.fixture_b(), sub=4096, cap=1000)  # the buffer inflates to more
    assert e.value.code == capi.KR_ERR_ARG


@pytest.mark.parametrize("name", list(CASES))
def test_the_twin_gives_zlibs_bytes(capi, name):
    r = twin(capi, CASES[name])
    assert r.error is None, r.error
    assert r.data == gc.gunzip(CASES[name][1])
    print(name, r.counters)


@pytest.mark.parametrize("name", [c[0] for c in gc.seam_cases()])
def test_the_seams_are_reached_without_a_host_range(capi, name):
    """the hand-assembled streams cut where they are meant to be: the stretch behind the first stored block is a chunk of its own"""
    r = twin(capi, CASES[name])
    assert r.counters["host_ranges"] == 0 and r.counters["super_chunks"] >= (1 if "mid-chain" in name else 2), r.counters
    n = [int(x) for x in r.tables["length"] if x]
    if "symbols" in name and "fewer" not in name:
        assert n[1] == int(name.split("-")[3]), n
    elif "mid-chain" not in name:
        assert n[0] == 33000 and (n[1] < 64) == ("fewer" in name), n


def test_fixture_a_every_searched_sub_chunk_but_the_last_links(capi):
    r = twin(capi, CASES["A"])
    assert r.counters["host_ranges"] == 0 and r.counters["dropped"] == 0 and r.counters["linked"] >= 100, r.counters
    S, status, length = r.tables["S"], r.tables["status"], r.tables["length"]
    assert len(S) == (len(gc.fixture_a()) + 1023) // 1024 and S[-1] == 0xFFFFFFFF and (S[:-1] != 0xFFFFFFFF).all()
    assert (status[:-2] == 1).all() and status[-2] == 2 and status[-1] == 0  # linked ..., the member's end, idle
    assert int(length.max()) < 32768, "a sub-chunk that inflates to 32 KB inherits no window"


def test_fixture_b_one_chunk_decodes_through_sub_chunks_without_a_start(capi):
    r = twin(capi, CASES["B"])
    assert r.counters["without_start"] >= 10 and r.counters["host_ranges"] == 0, r.counters


def test_five_super_chunks_hand_windows_across(capi):
    r = twin(capi, CASES["A-five-super-chunks"])
    assert r.counters["super_chunks"] >= 5 and r.counters["host_ranges"] == 0, r.counters
    assert (r.tables["status"] == 3).sum() >= 4, "every super-chunk but the last ends at its input's end"


def test_a_ratio_above_the_cap_goes_through_a_host_range(capi):
    r = twin(capi, CASES["run-of-As-ratio4"])
    assert r.counters["host_ranges"] >= 1 and (r.tables["status"] == 4).any(), r.counters


def test_a_decoy_start_in_a_stored_block_is_dropped(capi):
    """the chunk that decodes the stored block runs into the slot of the first decoy start and reports OVERFLOW; the chain ends there,
    the verified prefix is kept, and a second super-chunk -- the file alone would be one -- takes the stored block up: its first
    sub-chunk cannot finish either, which is a host range"""
    case = CASES["decoy-in-a-stored-block"]
    r = twin(capi, case)
    assert r.counters["dropped"] >= 1, r.counters
    nsub = (len(case[1]) + case[2] - 1) // case[2]
    first = r.tables["status"][:nsub]  # the first super-chunk's rows: linked chunks, then the one that overflowed, at the chain's end
    k = int((first == 4).argmax())
    assert (first == 4).any() and (first[:k] == 1).all() and k >= 1
    assert -(-len(case[1]) // case[4]) == 1 and r.counters["super_chunks"] == 2 and r.counters["host_ranges"] == 1, r.counters
    assert r.counters["redone_bytes"] > 0


def test_binary_content_has_no_start_anywhere(capi):
    r = twin(capi, CASES["binary"])
    assert r.counters["linked"] == 0 and r.counters["dropped"] == 0 and r.counters["host_ranges"] >= 1, r.counters
    assert (r.tables["S"][r.tables["S"] != 0xFFFFFFFF] < 8).all(), "only sub-chunk 0 starts anywhere"


def test_members_end_inside_and_at_the_end_of_a_super_chunk(capi):
    r = twin(capi, CASES["three-members"])
    assert (r.tables["status"] == 2).sum() >= 3
    r = twin(capi, CASES["member-ends-at-the-super-chunk-end"])
    assert r.tables["status"][0] in (1, 2) and (r.tables["status"] == 2).sum() >= 3 and r.counters["super_chunks"] >= 3


@pytest.mark.parametrize("name,gz", gc.damaged_cases(), ids=[c[0] for c in gc.damaged_cases()])
def test_damage_is_an_io_error_or_zlibs_bytes(capi, name, gz):
    r = capi.gzdev_inflate(gz, sub=4096)
    try:
        want = gc.gunzip(gz) if gz[:2] == b"\x1f\x8b" else None
    except zlib.error:
        want = None
    if want is None:
        assert r.error is not None and r.error.code == capi.KR_ERR_IO and "damaged gzip file" in str(r.error), (name, r.error)
        assert gc.gunzip(gc.fixture_b()).startswith(r.data) or name.startswith("flip")
    else:
        assert r.error is None and r.data == want


def test_a_wrong_crc_and_a_wrong_isize_name_the_trailers_offset(capi):
    crc, isize, at = gc.wrong_trailer()
    want = gc.gunzip(gc.fixture_b())
    for gz, off, what in ((crc, at, "CRC-32"), (isize, at + 4, "length")):
        r = capi.gzdev_inflate(gz, sub=4096)
        assert r.error is not None and r.error.code == capi.KR_ERR_IO
        assert "damaged gzip file" in str(r.error) and what in str(r.error) and "offset %d)" % off in str(r.error), r.error
        assert r.data == want, "the bytes in front of the damage are handed out"


@pytest.fixture(scope="module")
def fastq_file(tmp_path_factory):
    text = gc.fastq_text(600, 1)
    assert gc.gunzip(gc.fixture_a()) == text
    p = tmp_path_factory.mktemp("gzsym") / "a.fq.gz"
    p.write_bytes(gc.fixture_a())
    return str(p), text


def records(text):
    lines = text.decode().split("\n")
    return [(lines[i][1:], lines[i + 1]) for i in range(0, len(lines) - 1, 4)]


@pytest.mark.parametrize("use_point", [True, False], ids=["point", "from-the-start"])
@pytest.mark.parametrize("where", ["0", "third-super-chunk", "last-record"])
def test_the_host_reader_opens_at_an_inflated_offset(capi, fastq_file, where, use_point):
    path, text = fastq_file
    a = gc.fixture_a()
    max_comp = len(a) // 5 + 1024
    off = {"0": 0, "third-super-chunk": text.index(b"\n@read", len(text) // 2) + 1, "last-record": text.rindex(b"@read")}[where]
    pt = capi.gzdev_point_host(a, off, sub=1024, max_comp=max_comp) if use_point else None
    if pt is not None:
        assert pt.inflated_off <= off and (where == "0") == (pt.inflated_off == 0)
        if where == "third-super-chunk":  # five super-chunks of about a fifth of the text each: the third one's start, a full window
            assert 0.3 * len(text) < pt.inflated_off < 0.5 * len(text) and pt.window_len == 32768
            assert bytes(pt.window) == text[pt.inflated_off - 32768:pt.inflated_off]
    names, bases, offs = capi.read_fastx(path, gzip_at=(off, pt))
    want = records(text[off:])
    assert list(names) == [w[0].split(" ")[0] for w in want] or list(names) == [w[0] for w in want]
    assert bases.tobytes().decode() == "".join(w[1] for w in want)


@pytest.mark.parametrize("use_point", [True, False], ids=["point", "from-the-start"])
@pytest.mark.parametrize("where", ["1", "last-byte"])
def test_the_host_reader_at_offset_1_and_at_the_last_byte(capi, fastq_file, where, use_point):
    """not record starts: the reader is in kseq's "look for the next marker" state there, as kr_fastx_open_at is on a plain file.
    With the point, zlib starts in mid-stream (the last byte: at the last super-chunk's start) and skips to the offset."""
    path, text = fastq_file
    plain = os.path.join(os.path.dirname(path), "a.fq")
    open(plain, "wb").write(text)
    off = 1 if where == "1" else len(text) - 1
    pt = capi.gzdev_point_host(gc.fixture_a(), off, sub=1024, max_comp=len(gc.fixture_a()) // 5 + 1024) if use_point else None
    if pt is not None:
        assert pt.inflated_off <= off and (pt.inflated_off > len(text) // 2) == (where == "last-byte"), pt.inflated_off
    got = capi.read_fastx(path, gzip_at=(off, pt))
    want = capi.read_fastx(plain, offset=off)
    assert list(got[0]) == list(want[0]) and got[1].tobytes() == want[1].tobytes() and (len(want[0]) > 0) == (where == "1")


def test_a_damaged_file_fails_in_the_host_reader_too(capi, tmp_path):
    crc, _, _ = gc.wrong_trailer()
    p = tmp_path / "bad.fq.gz"
    p.write_bytes(crc)
    with pytest.raises(capi.KrError) as e:
        capi.read_fastx(str(p), gzip_at=(0, None))
    assert e.value.code == capi.KR_ERR_IO and "damaged gzip file" in str(e.value)
