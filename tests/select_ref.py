"""The selection stage of `krepp dist` for one read, restated plainly from the reference (src/query.cpp:96-139 summarize_matches,
158-196 report_distances) and the oracle's iteration order: every forward-strand leaf by ascending se, then every reverse-strand one.
Nothing here is taken from the device kernels; tests/test_select_ref_cpu.py holds it to the oracle before a kernel is judged by it.

A record is (key, d, v, matches) with key = se << 1 | strand; a read's records come in ascending key order, so the two strands of a
leaf are neighbours.  The rule:

  closest      the LAST record in (strand, index) order whose d <= the best so far (the best starts at DBL_MAX), i.e. the smallest d
               and among equal d the largest (strand, index).
  merge        a leaf is represented by its reverse-strand record unless d_rc > d_or, or d_rc == d_or and matches_rc < matches_or.
  override     the closest then represents its own leaf, whatever the merge said.
  NA           the read has no record, or dist_max is set and the closest's d > dist_max (d == dist_max is not NA).
  rows         of a read that is not NA, in record order: --no-multi: the closest alone (no further test: src/query.cpp:193);
               else every representing record with d < dist_max, strictly, and under --filter with
               chi = 2 (f(closest's problem, d) - v_closest) < chisq as well.
"""
import math

DBL_MAX = 1.7976931348623157e308


def select_ref(records, multi=1, no_filter=1, dist_max=None, chisq=2.706, f=None):
    """records: [(key, d, v, matches)] in ascending key order.  dist_max None or NaN: not set.  f(ic, d): the objective of record ic's
    problem at d (--filter only).  Returns dict(na, closest (index or None), sel [bool], chi [float or None: not computed], rows
    [(key, d)] in record order)."""
    n = len(records)
    dmax_set = dist_max is not None and not math.isnan(dist_max)
    best, closest = DBL_MAX, None
    for strand in (0, 1):
        for i, (key, d, _v, _m) in enumerate(records):
            if (key & 1) == strand and d <= best:
                best, closest = d, i
    rep = {}  # node_to_minfo: leaf -> index of the record that stands for it
    for i, (key, _d, _v, _m) in enumerate(records):
        if not key & 1:
            rep[key >> 1] = i
    for i, (key, d, _v, m) in enumerate(records):
        if key & 1:
            io = rep.get(key >> 1)
            rep[key >> 1] = i
            if io is not None:
                d_or, m_or = records[io][1], records[io][3]
                if d > d_or or (d == d_or and m < m_or):
                    rep[key >> 1] = io
    if closest is not None:
        rep[records[closest][0] >> 1] = closest
    na = n == 0 or (dmax_set and best > dist_max)
    sel, chi = [False] * n, [None] * n
    if not na:
        if not multi:
            if closest is not None:
                sel[closest] = True
        else:
            for i in sorted(rep.values()):
                d = records[i][1]
                ok = (not dmax_set) or d < dist_max
                if not no_filter:
                    chi[i] = 2 * (f(closest, d) - records[closest][2])
                    ok = ok and chi[i] < chisq
                sel[i] = ok
    rows = [(records[i][0], records[i][1]) for i in range(n) if sel[i]]
    return dict(na=bool(na), closest=closest, sel=sel, chi=chi, rows=rows)
