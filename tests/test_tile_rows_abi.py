"""KR_TILE_ROWS in the header and in its ctypes mirror: the next free submit flag, the same number in both."""
import os
import re

from conftest import ROOT


def submit_flags_of_the_header():
    text = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    names = ("KR_BASES_DEVICE", "KR_TAP_ACCS", "KR_TAP_HITS", "KR_BASES_PINNED", "KR_ROWS_ONLY", "KR_ROWS_INDEXED", "KR_TILE_DEVICE", "KR_TILE_ROWS")
    return {nm: int(re.search(r"^#define %s (\d+)u\b" % nm, text, re.M).group(1)) for nm in names}


def test_the_flag_is_128_in_the_header_and_in_capi():
    from krepp_amd import capi

    text = open(os.path.join(ROOT, "include", "krepp_amd.h")).read()
    assert re.search(r"^#define KR_TILE_ROWS 128u\b", text, re.M)
    assert capi.KR_TILE_ROWS == 128


def test_the_submit_flags_are_distinct_bits_mirrored_in_capi():
    from krepp_amd import capi

    flags = submit_flags_of_the_header()
    assert sorted(flags.values()) == [1 << i for i in range(8)]
    for nm, v in flags.items():
        assert getattr(capi, nm) == v, nm
