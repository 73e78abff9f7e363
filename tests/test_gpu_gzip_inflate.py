"""Ordinary gzip inflated by the four kernels of csrc/kr_dev_gzip.inc (kr_debug_gzdev_inflate, kr_gzdev_*): on every valid input of
gzip_cases.py the bytes are zlib's, and bytes, per-sub-chunk tables (start bit, end bit, status, link, symbols, CRC-32) and counters
equal those of the stages' serial twin (kr_debug_gzdev_inflate_host), which runs the same code.  The conditions on fixtures A and B
are carried here too, so that the test cannot pass through host ranges.  The seams are hand-assembled streams (gzip_cases.seam_cases):
a copy of distance exactly 32,768 as a chunk's first token, a copy whose source straddles window and own output with distance <
length, a chunk of fewer than 64 symbols, chunks of 32,767 / 32,768 / 32,769 symbols (the window behind them: one inherited byte / all
their own output), a stored and a fixed block in mid-chain.  Damaged inputs compare bytes, status and message with the twin's."""
import pytest

import gzip_cases as gc

pytestmark = pytest.mark.gpu

CASES = {c[0]: c for c in gc.valid_cases() + gc.seam_cases()}
DAMAGED = dict(gc.damaged_cases()[::3])


def both(capi, gz, sub, ratio, max_comp):
    return capi.gzdev_inflate(gz, sub=sub, ratio=ratio, max_comp=max_comp, device=0), capi.gzdev_inflate(gz, sub=sub, ratio=ratio, max_comp=max_comp)


@pytest.mark.parametrize("name", list(CASES))
def test_the_kernels_give_the_twins_bytes_tables_and_counters(capi, name):
    _, gz, sub, ratio, max_comp = CASES[name]
    dev, host = both(capi, gz, sub, ratio, max_comp)
    assert dev.error is None, dev.error
    assert dev.data == gc.gunzip(gz)
    assert dev.data == host.data and dev.counters == host.counters, (dev.counters, host.counters)
    for k in dev.tables:
        assert (dev.tables[k] == host.tables[k]).all(), (k, dev.tables[k], host.tables[k])
    if name == "A":
        assert dev.counters["host_ranges"] == 0 and dev.counters["dropped"] == 0 and dev.counters["linked"] >= 100, dev.counters
    if name == "B":
        assert dev.counters["without_start"] >= 10 and dev.counters["host_ranges"] == 0, dev.counters
    if name.startswith("seam"):
        assert dev.counters["host_ranges"] == 0, dev.counters
    if name == "three-members":
        # a member ends inside the super-chunk: the chain ends there, and what the sub-chunks behind it decoded (the next members,
        # each to its own end) is redone by the next super-chunk
        assert dev.counters["super_chunks"] == 3 and (dev.tables["status"] == 2).sum() >= 3 and dev.counters["dropped"] > 0


@pytest.mark.parametrize("name", list(DAMAGED))
def test_damage_gives_the_twins_bytes_status_and_message(capi, name):
    dev, host = both(capi, DAMAGED[name], 4096, 16, gc.BIG)
    assert dev.data == host.data and str(dev.error) == str(host.error)
    assert dev.same_tables(host)


def test_wrong_trailers(capi):
    crc, isize, at = gc.wrong_trailer()
    for gz in (crc, isize):
        dev, host = both(capi, gz, 4096, 16, gc.BIG)
        assert dev.error is not None and dev.error.code == capi.KR_ERR_IO and str(dev.error) == str(host.error)
        assert dev.data == host.data == gc.gunzip(gc.fixture_b())


def test_a_file_is_read_in_pieces_with_restart_points_and_counters(capi, tmp_path):
    a, text = gc.fixture_a(), gc.gunzip(gc.fixture_a())
    p = tmp_path / "a.fq.gz"
    p.write_bytes(a)
    g = capi.Gzdev(p, device=0, max_comp=len(a) // 5 + 1024, sub=1024)
    got = b""
    while True:
        piece = g.read(10007)
        if not piece:
            break
        got += piece
    assert got == text
    c = g.counters()
    assert c["super_chunks"] == 5 and c["host_ranges"] == 0 and c["dropped"] == 0 and c["linked"] >= 100, c
    assert c["us_search"] > 0 and c["us_decode"] > 0 and c["us_chain"] > 0 and c["us_resolve"] > 0
    off = text.rindex(b"@read")
    pt, want = g.point(off), capi.gzdev_point_host(a, off, sub=1024, max_comp=len(a) // 5 + 1024)
    assert (pt.bit, pt.inflated_off, pt.member_len, pt.member_crc, pt.window_len) == (want.bit, want.inflated_off, want.member_len, want.member_crc, want.window_len)
    assert bytes(pt.window) == bytes(want.window) == text[pt.inflated_off - 32768:pt.inflated_off]
    with pytest.raises(capi.KrError):
        g.point(0)  # five super-chunks back: no longer kept
    names, bases, _ = capi.read_fastx(str(p), gzip_at=(off, pt))
    assert len(names) == 1 and bases.tobytes() == text[off:].split(b"\n")[1]
    g.close()
