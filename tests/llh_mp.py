"""High-precision reference of the likelihood objective HDistHistLLH::operator() (src/hdhistllh.hpp:71-89), written
from the formula, and the cases of tests/golden/llh_mp.npy (tests/golden/make_llh_mp.py writes the file).

    f(d) = - sum_{x <= th} mc[x] (k ln om + x (ln d - ln om)) - uc ln A,        om = fl(1 - d)
    A    = rho lv + 1 - rho,   lv = sum_{x <= th} (C(k,x) - C(k-h,x)) om^(k-x) d^x + sum_{x > th} C(k,x) om^(k-x) d^x

Two roundings belong to the formula itself: d is a double, and the reference takes log(1.0 - d) and pow(1.0 - d, k) of the
ROUNDED difference, so om = fl(1 - d) here too (at d = 1e-10 the real-number function is 6e-8 relative away from what the
reference's own formulation defines; no implementation could be judged against it there).  Nothing else is rounded: A is
computed exactly from the exact lv, every sum is exact to the working precision (256 bits).

Each value comes with a condition-aware error unit B (see err_unit): one rounding per operation of the first sum, and for the
second term the log of a number that may lie next to 1.  An implementation in doubles that follows the reference's operation
order with correctly rounded pow / log stays within a few B (measured: tests/test_llh_reference_cpu.py).

mpmath is imported only by the functions that need it: the GPU tests read the fixture and use the plain-double helpers
(load_cases, window, err_unit) with numpy alone.
"""
import math
import os

import numpy as np

PREC = 256
LO, HI = 1e-10, 0.5  # the bracket of brent_find_minima at src/query.cpp:430
KH = [(19, 3), (21, 7), (27, 11), (29, 13), (31, 15)]
THS = [0, 2, 4, 6, 9, 16]  # 16 = KR_MAX_HDIST_TH
CLASSES = ["interior", "small_d", "half", "rho0", "rho1", "tiny_rho", "big", "uc0", "boundary"]
MIN_CLASSES = ["interior", "rho0", "rho1", "tiny_rho", "big", "uc0", "boundary"]
FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "llh_mp.npy")
SEED = 20260


def binomials(k, h, th):
    """binom_coef_k[0..k] and binom_coef_hnk[0..th] of the constructor (src/hdhistllh.hpp:51-69), as exact integers"""
    bk = [math.comb(k, x) for x in range(k + 1)]
    hnk = [0] + [math.comb(k, x) - math.comb(k - h, x) for x in range(1, th + 1)]
    return bk, hnk


def window(dstar):
    """w = fract2 of Boost's stopping rule with 16 bits at d*, and the abscissas d* - 2w, d* - w, d*, d* + w, d* + 2w clipped to
    the bracket (doubles).  Brent stops when its bracket lies within x +- fract2(x): the true minimiser is then within w of x."""
    w = 2.0 * (2.0 ** -15 * dstar + 2.0 ** -17)
    return w, [min(HI, max(LO, dstar + j * w)) for j in (-2, -1, 0, 1, 2)]


def err_unit(k, h, th, mc, uc, rho, d):
    """B in plain doubles (an error unit needs no precision; the fixture's B is the same expression in mpmath):
    B = 2^-53 [ sum_x mc[x] (|k ln om| + x |ln d - ln om| + x (|ln d| + |ln om|)) + uc (|ln A| + (rho lv (k + 3) + 1 + rho) / A) ]"""
    bk, hnk = binomials(k, h, th)
    om = 1.0 - d
    ld, lo = math.log(d), math.log(om)
    s = sum(mc[x] * (abs(k * lo) + x * abs(ld - lo) + x * (abs(ld) + abs(lo))) for x in range(th + 1))
    lv = math.fsum((hnk[x] if x <= th else bk[x]) * om ** (k - x) * d ** x for x in range(k + 1))
    A = rho * lv + 1.0 - rho
    return 2.0 ** -53 * (s + uc * (abs(math.log(A)) + (rho * lv * (k + 3) + 1.0 + rho) / A))


def f_mp(k, h, th, mc, uc, rho, d, exact_om=False):
    """(f, B) in mpmath.  exact_om: om = 1 - d unrounded (the smooth function, for the search of the minimiser only)."""
    import mpmath as mp

    with mp.workprec(PREC):
        bk, hnk = binomials(k, h, th)
        dd = mp.mpf(d)
        om = (1 - dd) if exact_om else mp.mpf(1.0 - float(d))
        ld, lo = mp.log(dd), mp.log(om)
        s = mp.mpf(0)
        sb = mp.mpf(0)
        for x in range(th + 1):
            m = mp.mpf(mc[x])
            s -= m * (k * lo + x * (ld - lo))
            sb += m * (abs(k * lo) + x * abs(ld - lo) + x * (abs(ld) + abs(lo)))
        lv = mp.mpf(0)
        for x in range(k + 1):
            lv += (hnk[x] if x <= th else bk[x]) * om ** (k - x) * dd ** x
        r = mp.mpf(rho)
        A = r * lv + 1 - r
        f = s - mp.log(A) * mp.mpf(uc)
        B = mp.ldexp(1, -53) * (sb + mp.mpf(uc) * (abs(mp.log(A)) + (r * lv * (k + 3) + 1 + r) / A))
        return f, B


def argmin_mp(k, h, th, mc, uc, rho):
    """d* = argmin of the objective on [1e-10, 0.5]: golden-section search in mpmath until the bracket is shorter than 1e-30, on
    the smooth function (om = 1 - d exact: with om = fl(1 - d) the function of a real d is a staircase at the 1e-16 level, and the
    two differ by less than B).  The objective is taken as unimodal on the bracket, as the reference's use of Brent takes it; a
    minimum at an end of the bracket is returned as that end."""
    import mpmath as mp

    with mp.workprec(PREC):
        g = (mp.sqrt(5) - 1) / 2
        a, b = mp.mpf(LO), mp.mpf(HI)
        f = lambda t: f_mp(k, h, th, mc, uc, rho, t, exact_om=True)[0]
        c, d = b - g * (b - a), a + g * (b - a)
        fc, fd = f(c), f(d)
        while b - a > mp.mpf("1e-30"):
            if fc <= fd:
                b, d, fd = d, c, fc
                c = b - g * (b - a)
                fc = f(c)
            else:
                a, c, fc = c, d, fd
                d = a + g * (b - a)
                fd = f(d)
        x = float((a + b) / 2)
        if x - LO < 1e-25:
            x = LO
        if HI - x < 1e-25:
            x = HI
        return x


# ---------------------------------------------------------------------------
# The cases: classes x (k, h) x th x {integer, fractional histograms}, seeded
# ---------------------------------------------------------------------------
def _hist(rng, th, total, frac):
    """a histogram of `total` matches skewed to the low distances, as reads give; frac: sums of integer counts over the numbers of
    children, as Minfo::add (src/query.hpp:139-152) accumulates them for `place`"""
    w = rng.random(th + 1) ** 3
    mc = np.floor(w / w.sum() * total)
    if frac:
        den = rng.integers(2, 8, 2)
        mc = np.floor(mc * rng.random(th + 1)) / float(den[0]) + mc / float(den[1])
    return mc


def make_problem(rng, cls, k, h, th, frac):
    """(mc, uc, rho, d) of one case; d is where the objective is evaluated"""
    total = int(rng.integers(1, 126))
    rho = float(rng.uniform(0.02, 0.98))
    d = float(10 ** rng.uniform(-4, math.log10(0.45)))
    if cls == "big":  # what the packed record word cannot hold: counts above 255, more than 65,535 k-mers
        total = int(rng.integers(300, 200_001))
    mc = _hist(rng, th, total, frac)
    if cls == "boundary":  # every match exact: the minimum lies at the lower end of the bracket
        mc[1:] = 0.0
        mc[0] = max(mc[0], 1.0)
    if float(mc.sum()) == 0.0:
        mc[0] = 1.0
    uc = float(rng.integers(0, 61))
    if cls == "big":
        uc = float(rng.integers(0, 200_001))
    if frac:
        uc = uc + float(rng.integers(0, 8)) / 8.0
    if cls == "uc0":
        uc = 0.0
    if cls == "small_d" or cls == "boundary":
        d = float(10 ** rng.uniform(-10, -4))
    if cls == "half":
        d = float(0.5 - 10 ** rng.uniform(-16, -1))
    if cls == "rho0":
        rho = 0.0
    if cls == "rho1":
        rho = 1.0
    if cls == "tiny_rho":
        rho = float(10 ** rng.uniform(-12, -3))
    return mc, uc, rho, min(HI, max(LO, d))


def case_keys():
    """every (class, k, h, th, frac, replicate) in the file's order; the first replicate of a MIN_CLASSES case is also minimised"""
    keys = []
    for ci, cls in enumerate(CLASSES):
        for (k, h) in KH:
            for th in THS:
                for frac in (0, 1):
                    for rep in range(4):
                        keys.append((ci, cls, k, h, th, frac, rep))
    return keys


def make_case(key, with_min=True):
    """one case of the fixture as a list of doubles: [code, mc[0..th], uc, rho, d, f, B] + [d*, B(d*), f at window(d*)] if
    minimised, code = ((class * 100 + k) * 100 + th) * 100 + 10 frac + minimised (h follows from k: KH).  Seeded by the key alone:
    any subsample can be regenerated on its own."""
    ci, cls, k, h, th, frac, rep = key
    rng = np.random.default_rng([SEED, ci, k, th, frac, rep])
    mc, uc, rho, d = make_problem(rng, cls, k, h, th, frac)
    mcl = [float(x) for x in mc]
    f, B = f_mp(k, h, th, mcl, uc, rho, d)
    has_min = with_min and rep == 0 and cls in MIN_CLASSES
    row = [float(((ci * 100 + k) * 100 + th) * 100 + 10 * frac + int(has_min))] + mcl + [float(uc), float(rho), float(d), float(f), float(B)]
    if has_min:
        ds = argmin_mp(k, h, th, mcl, uc, rho)
        _, xs = window(ds)
        row += [float(ds), float(f_mp(k, h, th, mcl, uc, rho, ds)[1])] + [float(f_mp(k, h, th, mcl, uc, rho, x)[0]) for x in xs]
    return row


def save_rows(rows, path=FIXTURE):
    """the rows one after another as one vector of doubles (.npy: exact values, the same bytes every time)"""
    np.save(path, np.array([x for r in rows for x in r], dtype=np.float64))


def load_rows(path=FIXTURE):
    v = np.load(path).tolist()
    rows, i = [], 0
    while i < len(v):
        code = int(v[i])
        n = 1 + (code // 100 % 100 + 1) + 5 + 7 * (code % 10)
        rows.append(v[i:i + n])
        i += n
    return rows


def load_cases(path=FIXTURE):
    """the fixture as dictionaries of plain Python / numpy values (no mpmath)"""
    out = []
    for r in load_rows(path):
        code = int(r[0])
        th, k = code // 100 % 100, code // 10 ** 4 % 100
        q = 1 + th + 1
        c = dict(cls=CLASSES[code // 10 ** 6], k=k, h=dict(KH)[k], th=th, frac=bool(code // 10 % 10), mc=np.array(r[1:q]), uc=r[q], rho=r[q + 1],
                 d=r[q + 2], f=r[q + 3], B=r[q + 4])
        if code % 10:
            c["dstar"], c["B_star"], c["f_win"] = r[q + 5], r[q + 6], r[q + 7:q + 12]
        out.append(c)
    return out


def window_bound(c):
    """The minimiser condition's right-hand side without its error term: the smaller of f(d* - 2w) and f(d* + 2w).  An edge that
    the bracket clips constrains nothing (every point of the bracket on that side lies inside the window: at a boundary minimum
    d* = 1e-10 the clipped edge IS the minimum, which Brent's stopping rule never reaches -- it ends ~1.26e-5 above it), so it
    counts as +inf; both clipped cannot happen (4w < 0.5 - 1e-10)."""
    w, xs = window(c["dstar"])
    lo = c["f_win"][0] if c["dstar"] - 2 * w > LO else math.inf
    hi = c["f_win"][4] if c["dstar"] + 2 * w < HI else math.inf
    return min(lo, hi)


# ---------------------------------------------------------------------------
# The objective in IEEE doubles with ideal primitives: what the device must return bit for bit
# ---------------------------------------------------------------------------
M_CPU = 2  # the oracle's worst |f - f_mp| / B over the fixture (1.89), rounded up: tests/test_llh_reference_cpu.py
M_GPU = 2 * M_CPU  # set before the device was measured: tests/test_gpu_llh_numerics.py


def pow_int_rounded(x, n):
    """x^n for a positive double x and a small positive integer n, correctly rounded (round to nearest even), in integer arithmetic:
    x = m 2^e exactly, x^n = m^n 2^(n e)"""
    m, e = math.frexp(x)
    mi, e = int(m * 2 ** 53), e - 53
    p, pe = mi ** n, e * n
    sh = p.bit_length() - 53
    q, r = p >> sh, p & ((1 << sh) - 1)
    half = 1 << (sh - 1)
    if r > half or (r == half and (q & 1)):
        q += 1
    return math.ldexp(q, pe + sh)


def log_classic(x):
    """The main path of the classic freely distributable libm log (e_log.c: x = 2^k (1 + f), s = f / (2 + f), the degree-14 minimax
    polynomial with its published coefficients Lg1..Lg7, k ln2 in two pieces) for a positive normal double, in IEEE doubles without
    contraction.  The original's separate branch for |f| < 2^-20 is left out, as the device's kr_log leaves it out (test_llh_reference_cpu
    holds this path to the < 1 ulp both claim, at the arguments next to 1 in particular)."""
    import struct

    ln2_hi, ln2_lo = 6.93147180369123816490e-01, 1.90821492927058770002e-10
    Lg1, Lg2, Lg3, Lg4 = 6.666666666666735130e-01, 3.999999999940941908e-01, 2.857142874366239149e-01, 2.222219843214978396e-01
    Lg5, Lg6, Lg7 = 1.818357216161805012e-01, 1.531383769920937332e-01, 1.479819860511658591e-01
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    hx, lx = bits >> 32, bits & 0xFFFFFFFF
    assert 0x00100000 <= hx < 0x7FF00000
    k = (hx >> 20) - 1023
    hx &= 0x000FFFFF
    i = (hx + 0x95F64) & 0x100000
    x = struct.unpack("<d", struct.pack("<Q", ((hx | (i ^ 0x3FF00000)) << 32) | lx))[0]
    k += i >> 20
    f = x - 1.0
    s = f / (2.0 + f)
    dk = float(k)
    z = s * s
    w = z * z
    t1 = w * (Lg2 + w * (Lg4 + w * Lg6))
    t2 = z * (Lg1 + w * (Lg3 + w * (Lg5 + w * Lg7)))
    R = t2 + t1
    if ((hx - 0x6147A) | (0x6B851 - hx)) > 0:
        hfsq = 0.5 * f * f
        return dk * ln2_hi - ((hfsq - (s * (hfsq + R) + dk * ln2_lo)) - f)
    return dk * ln2_hi - ((s * (f - R) - dk * ln2_lo) - f)


def f_ieee(k, h, th, mc, uc, rho, d):
    """HDistHistLLH::operator() (src/hdhistllh.hpp:71-89) in the reference's operation order, every operation one IEEE double operation,
    with a correctly rounded pow and the classic log.  The device claims exactly this of its objective: the same operations in the same
    order (compiled without contraction), pown_dd "correctly rounded except near ties" (its chain carries ~100 bits: a case within 2^-45
    ulp of a tie does not occur among a few thousand), kr_log "the classic log restated".  So the device's value has THESE BITS -- a
    claim with no tolerance, which a pown_dd a few ulps off or a log coefficient changed in a late digit cannot meet."""
    bk, hnk = binomials(k, h, th)
    om = 1.0 - d
    powdc = pow_int_rounded(om, k)
    logdn = log_classic(om)
    logdp = log_classic(d) - logdn
    logdn *= float(k)
    dratio = d / om
    s = lv = 0.0
    for x in range(k + 1):
        if x <= th:
            s -= (logdn + float(x) * logdp) * float(mc[x])
            lv += float(hnk[x]) * powdc
        else:
            lv += powdc * float(bk[x])
        powdc *= dratio
    return s - log_classic(rho * lv + 1.0 - rho) * uc


def minimiser_condition(c, d, v, f_at_d, M, what):
    """The returned point lies inside the window Brent's stopping rule allows around the true minimiser d*, judged by values: the
    objective at d (f_at_d: a trusted evaluation) is not above the smaller of f_mp(d* - 2w), f_mp(d* + 2w) (window_bound: an edge the
    bracket clips constrains nothing) by more than M B; the returned v is the objective at d within M B; a minimum at the lower end of
    the bracket (every match exact) is reported below 1e-4 (the rule stops ~1.26e-5 above the end).  Returns |v - f_at_d| / B."""
    B = err_unit(c["k"], c["h"], c["th"], c["mc"], c["uc"], c["rho"], d)
    assert LO <= d <= HI, (what, c["cls"], d)
    assert f_at_d <= window_bound(c) + M * B, (what, c["cls"], c["k"], c["th"], d, c["dstar"], f_at_d, window_bound(c), B)
    assert abs(v - f_at_d) <= M * B, (what, c["cls"], c["k"], c["th"], d, v, f_at_d, B)
    if c["dstar"] == LO:
        assert d < 1e-4, (what, c["cls"], d)
    return abs(v - f_at_d) / B
