"""Pins the oracle against REFERENCE outputs: the committed *_ref.json fixtures were
produced by the reference's own sources (oracle/ref_drivers/ref_shim.cpp), and, when
oracle/_ref/libkrepp_ref.so is present, the calls behind llh_live_ref.json are repeated live."""
import json
import os

import numpy as np

from conftest import GOLDEN
from helpers import llh_live_cases


def test_llh_matches_reference_fixture(po):
    cases = json.load(open(os.path.join(GOLDEN, "llh_ref.json")))
    assert len(cases) >= 200
    for c in cases:
        for dh, fh in zip(c["d"], c["f"]):
            d, want = float.fromhex(dh), float.fromhex(fh)
            got = po.llh(c["k"], c["h"], c["th"], c["hist"], c["uc"], float.fromhex(c["rho"]), d)
            # same operation order, same libm => bit-exact (src/hdhistllh.hpp:71-89)
            assert got == want or (np.isnan(got) and np.isnan(want)), (c, d, got, want)


def test_llh_matches_reference_live(po):
    """300 seeded random problems against the reference's own values: called live when oracle/_ref is built, and as
    recorded from the same calls in llh_live_ref.json (which the live values must equal) in any case."""
    ref = po.ref()
    want = json.load(open(os.path.join(GOLDEN, "llh_live_ref.json")))
    cases = llh_live_cases()
    assert len(want) == len(cases) == 300
    for (k, h, th, hist, uc, rho, d), w in zip(cases, want):
        if ref is not None:
            hc = np.ascontiguousarray(hist)
            assert float(ref.ref_llh(k, h, th, hc.ctypes.data, uc, rho, d)).hex() == w
        assert po.llh(k, h, th, hist, uc, rho, d) == float.fromhex(w)


def test_murmur_matches_reference(po):
    mm = json.load(open(os.path.join(GOLDEN, "murmur_ref.json")))
    l = po.lib()
    for c in mm:
        s = c["name"].encode()
        assert l.ko_murmur3_x86_32(s, len(s), 0) == c["seed0"]
        assert l.ko_murmur3_x86_32(s, len(s), 1) == c["seed1"]
        assert l.ko_name_hash(s) == (c["seed0"] << 32) | c["seed1"]  # src/record.hpp:26-36


def test_fmix64_known_answers(po):
    # MurmurHash3 fmix64 (src/common.hpp:147-155 == src/MurmurHash3.cpp:69-78)
    l = po.lib()
    assert l.ko_xur64(0) == 0
    assert l.ko_xur64(1) == 0xB456BCFC34C2CB2C
    assert l.ko_xur64(0xFFFFFFFFFFFFFFFF) == 0x64B5720B4B825F21
