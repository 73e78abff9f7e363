"""The oracle's likelihood objective and minimiser against the 256-bit reference of tests/llh_mp.py (fixture
tests/golden/llh_mp.npy, written by tests/golden/make_llh_mp.py): what makes the oracle's floating-point part more than
"restated from source", and the anchor of tests/test_gpu_llh_numerics.py.

All bounds are in units of B, the condition-aware error unit the fixture holds for every case (llh_mp.err_unit).

M_CPU is the oracle's own worst |f - f_mp| / B over the fixture, rounded up to the next integer.  Measured (glibc 2.x pow / log,
2,160 cases): 1.89 -- per class: interior 1.54, small_d 1.66, half 1.67, rho0 1.89, rho1 1.03, tiny_rho 1.65, big 1.61, uc0 1.82,
boundary 1.20; th >= 9 alone: 1.78.  The returned v of po.brent against f_mp at the returned d: 1.94 at worst (uc0)."""
import math

import numpy as np
import pytest

import llh_mp
from llh_mp import M_CPU, minimiser_condition  # M_CPU = 2 = ceil(1.89), see above; the device tests use M_GPU = 2 * M_CPU


@pytest.fixture(scope="module")
def cases():
    cs = llh_mp.load_cases()
    assert len(cs) == len(llh_mp.case_keys()) and sum("dstar" in c for c in cs) >= 400
    return cs


def test_fixture_covers_the_classes(cases):
    """every class x (k, h) x th x {integer, fractional} is there, with the inputs the packed record word cannot hold"""
    seen = {(c["cls"], c["k"], c["h"], c["th"], c["frac"]) for c in cases}
    assert len(seen) == len(llh_mp.CLASSES) * len(llh_mp.KH) * len(llh_mp.THS) * 2
    assert any(c["mc"].max() > 255 for c in cases) and any(c["mc"].sum() + c["uc"] > 65535 for c in cases)
    assert any(c["d"] < 1e-9 for c in cases) and any(0.5 - c["d"] < 1e-12 for c in cases)
    assert any("dstar" in c and c["dstar"] == llh_mp.LO for c in cases)
    assert all(c["B"] > 0 and math.isfinite(c["f"]) for c in cases)


def test_fixture_regenerates(cases):
    """a seeded subsample (every 5th case, and every 4th minimised one) computed again equals the committed file, bit for bit (the
    whole file: tests/golden/make_llh_mp.py, which writes the same bytes every time)"""
    pytest.importorskip("mpmath")
    rows = llh_mp.load_rows()
    keys = llh_mp.case_keys()
    nmin = 0
    for i, key in enumerate(keys):
        has_min = int(rows[i][0]) % 10 == 1
        nmin += has_min
        if i % 5 == 0 or (has_min and nmin % 4 == 0):
            assert llh_mp.make_case(key) == rows[i], key
    # ... and the plain-double error unit the minimiser tests use away from the stored abscissas is the file's
    for c in cases[::7]:
        assert llh_mp.err_unit(c["k"], c["h"], c["th"], c["mc"], c["uc"], c["rho"], c["d"]) == pytest.approx(c["B"], rel=1e-9)


def test_oracle_objective_within_the_error_unit(po, cases):
    worst = {}
    for c in cases:
        f = po.llh(c["k"], c["h"], c["th"], c["mc"], c["uc"], c["rho"], c["d"])
        r = abs(f - c["f"]) / c["B"]
        worst[c["cls"]] = max(worst.get(c["cls"], 0.0), r)
        assert r <= M_CPU, (c["cls"], c["k"], c["th"], c["d"], f, c["f"], r)
    print("oracle |f - f_mp| / B, worst per class:", {k: round(v, 2) for k, v in worst.items()})


def test_oracle_minimiser_lies_in_brents_window(po, cases):
    """po.brent on every minimised case.  The objective at the returned d is f_mp itself where mpmath imports; without it, the
    oracle's own objective, which the test above pins to M_CPU B (then that much is added to the bound: nothing is skipped)."""
    try:
        import mpmath  # noqa: F401
        have_mp = True
    except ImportError:
        have_mp = False
    worst = 0.0
    n = 0
    for c in cases:
        if "dstar" not in c:
            continue
        d, v, _ = po.brent(c["k"], c["h"], c["th"], c["mc"], c["uc"], c["rho"])
        if have_mp:
            f_at_d = float(llh_mp.f_mp(c["k"], c["h"], c["th"], list(c["mc"]), c["uc"], c["rho"], d)[0])
            worst = max(worst, minimiser_condition(c, d, v, f_at_d, M_CPU, "oracle"))
        else:
            f_at_d = po.llh(c["k"], c["h"], c["th"], c["mc"], c["uc"], c["rho"], d)
            minimiser_condition(c, d, v, f_at_d, 2 * M_CPU, "oracle")
        n += 1
    assert n >= 400
    print("oracle |v - f_mp(d)| / B, worst:", round(worst, 2))


def test_ideal_primitives_and_the_ieee_objective(cases):
    """llh_mp.f_ieee -- the reference's operation order in IEEE doubles with a correctly rounded power and the classic log -- is what
    the device is required to return bit for bit (tests/test_gpu_llh_numerics.py).  Here its parts are held to their own contracts:
    pow_int_rounded is the correctly rounded power, log_classic (the classic log's main path, also next to 1, where the original
    branches off) stays below 1 ulp, and f_ieee stays within M_CPU B of the 256-bit value on every case.  Measured: log 0.82 ulp at
    worst over 65,000 arguments, f_ieee 1.82 B."""
    rng = np.random.default_rng(1)
    xs = np.concatenate([10 ** rng.uniform(-10, np.log10(0.5), 6000), 1 - 10 ** rng.uniform(-10, -0.31, 6000), rng.uniform(0.5, 1, 6000),
                         [1e-10, 0.5, 1 - 2.0 ** -53, 1 - 1e-10, 2.0 ** -20 + 1, 1 - 2.0 ** -21]]).tolist()
    try:
        import mpmath as mp
    except ImportError:
        mp = None
    worst = 0.0
    for x in xs:
        y = llh_mp.log_classic(x)
        if mp is not None:
            with mp.workprec(200):
                e = float(abs(mp.mpf(y) - mp.log(mp.mpf(x))) / mp.mpf(math.ulp(y)))
                assert llh_mp.pow_int_rounded(x, 29) == float(mp.mpf(x) ** 29), x
        else:  # (the C library's log and pow are below 1 ulp themselves)
            e = abs(y - math.log(x)) / math.ulp(y) / 2
            assert abs(llh_mp.pow_int_rounded(x, 29) - math.pow(x, 29)) <= math.ulp(math.pow(x, 29)), x
        worst = max(worst, e)
        assert e < 1.0, (x, y, e)
    for c in cases:
        f = llh_mp.f_ieee(c["k"], c["h"], c["th"], c["mc"], c["uc"], c["rho"], c["d"])
        assert abs(f - c["f"]) <= M_CPU * c["B"], (c["cls"], c["k"], c["th"], c["d"], f, c["f"])
    print("classic log, worst error in ulp:", round(worst, 3))
