"""Crafted records for the select and row kernels (docs/design/05_likelihood_select_rows_text.md: the form table), with the tables
kr_debug_select takes and what tests/select_ref.py says of every read.

The selection is one rule in eight hand-written forms, chosen by the number of records of a read; what tells the forms apart are ties
(equal d between the strands of a leaf, equal minimal d at records far apart) and neighbours that lie across a seam of the form: the
next step of a lane's walk, the next group of 16 or 32 lanes, lane 63 | 0 of the next step of 64, records 255 | 256 of the first pass
and 127 | 128 of the second.  Natural reads do not produce them; here they are the rule: values come from a pool of six distances (two
of them adjacent doubles) and match counts 1..3, and the seams are derived from the constants the library reports
(capi.select_layout), so a changed kSelectLaneMax, KR_SELECT_GL or kRowBlock moves the designs or fails
tests/test_select_craft_cpu.py (the other five numbers of the report restate literals of the kernels by hand: they move the designs
only once the report is changed with the kernel).

A design is a list of reads; a read is a list of records {key, j, m, packed, direct}: key = se << 1 | strand, j its position in the list
of distinct values (d = POOL[j % 6], v distinct per position), m its match count, packed: the problem travels as a packed word
(rec_w0) or as histogram planes only, direct: the value is reached through a direct place or through the list."""
import math

import numpy as np

from acc_craft import FRAC, H, K, M, PPOS, R, Tree
from helpers import write_index
from select_ref import select_ref

NLEAF = 1024  # a read of 600 records of single strands needs 600 leaves
RHO = (0.0, 1e-9, 0.3, 1.0)
D_ADJ = 0.05
POOL = (1e-10, 0.003, D_ADJ, math.nextafter(D_ADJ, 1.0), 0.12, 0.5)  # POOL[2], POOL[3]: adjacent doubles
NREP = 48  # list positions: position j carries (POOL[j % 6], -1 - j / 64)
DIRECT_FLAG = 0x80000000
HOLE = 0xFFFFFFFF
DMAX = (POOL[2], math.nextafter(POOL[2], 0.0), POOL[3])  # dist_max at a pool value, one double below it, one above (= the next pool value)


class Index:
    """The crafted index: a tree of NLEAF leaves and a table of one entry; only its node count and its rho matter (the selection never
    looks at the tree's shape, so the balanced binary tree of acc_craft, which the loader is known to take, serves as well as a star).  rho[se] of leaf i is
    RHO[i % 4] as the loader hands it out: it scales the file's doubles by (r + 1) / m (Index::make_rho_partial), so the file holds
    m / (r + 1) = 2 times that, exactly"""

    def __init__(self):
        self.tree = Tree(NLEAF)
        t = self.tree
        self.rho = [0.0] * (t.nnodes + 1)
        for i, se in enumerate(t.leaf_se):
            self.rho[se] = RHO[i % 4]
        self.leaf_se = sorted(t.leaf_se)

    def write(self, path):
        t = self.tree
        assert FRAC and M == 2 * (R + 1)
        write_index(path, K, H, M, R, FRAC, PPOS, {0: [(0, t.leaf_se[0])]}, list(t.children), [2.0 * x for x in self.rho], nwk=t.nwk)
        return path


def sizes(lay):
    """record counts on both sides of every threshold between two forms, and inside the forms"""
    L, gs, gm, gl, big, st2 = (lay[k] for k in ("lane_max", "group_small", "group_mid", "wave_gl", "big_regs", "big_step2"))
    s = {0, 1, 3, 4, 5, L, L + 1, 600}
    for c in (gs, gm, gl, 2 * gl, 3 * gl, big, big + st2, 2 * big):
        s |= {c - 1, c, c + 1}
    return sorted(s)


def seams(lay, n):
    """p of the record pairs (p, p + 1) that straddle a seam of some form, for a read of n records"""
    L, gs, gm, gl, big, st2 = (lay[k] for k in ("lane_max", "group_small", "group_mid", "wave_gl", "big_regs", "big_step2"))
    ps = {0, 3, L - 1, gs - 1, gm - 1, gl - 1, 2 * gl - 1, 3 * gl - 1, big - 1, big + st2 - 1, n - 2}
    out = []
    for p in sorted(ps):
        if 0 <= p and p + 1 < n and (not out or p > out[-1] + 1):
            out.append(p)
    return out


def make_keys(rng, leaf_se, n, pairs=(), strand_at=None, first=None, last=None, p_pair=0.3):
    """n strictly ascending keys: a strand pair at (p, p + 1) for every p of `pairs`, a given strand at the positions of strand_at,
    elsewhere random pairs and single strands.  first / last: (leaf rank, strand) of the first / last record."""
    pairs, strand_at = set(pairs), dict(strand_at or {})
    keys, i = [], 0
    leaf, limit = (0 if first is None else first[0]), (len(leaf_se) if last is None else last[0])  # leaves [leaf, limit) for all but a given last
    if first is not None:
        strand_at[0] = first[1]
    if last is not None:
        strand_at[n - 1] = last[1]
    while i < n:
        if last is not None and i == n - 1:
            leaf = last[0]
        else:
            room = limit - leaf - (n - i - (last is not None))
            assert room >= 0, "out of leaves"
            if room > 0 and not (first is not None and i == 0):
                leaf += int(rng.integers(0, 2))
        se = leaf_se[leaf]
        free = i not in strand_at and (i + 1) not in strand_at and (i + 1) not in pairs and i + 1 < n
        if i in pairs or (free and rng.random() < p_pair):
            keys += [se << 1, se << 1 | 1]
            i += 2
        else:
            keys.append(se << 1 | (strand_at[i] if i in strand_at else int(rng.integers(0, 2))))
            i += 1
        leaf += 1
    assert len(keys) == n and all(a < b for a, b in zip(keys, keys[1:]))
    return keys


def records(rng, keys, dix, ms):
    """records of a read: d index into POOL and match count per record; list position, packed / planes and direct / list at random"""
    return [dict(key=k, j=int(d) + 6 * int(rng.integers(0, NREP // 6)), m=int(m), packed=bool(rng.integers(0, 2)), direct=bool(rng.integers(0, 2)))
            for k, d, m in zip(keys, dix, ms)]


REL = ("<", "=", ">")
# what a pair that hosts the closest can be: the closest is the reverse record (then d_rc <= d_or) or the forward one (then d_rc > d_or:
# with equal d the reverse record comes later in (strand, index) order).  reverse, '=', matches '<' is the case where the override
# undoes the merge.
FOCUS = [("rc", "<", m) for m in REL] + [("rc", "=", m) for m in REL] + [("or", ">", m) for m in REL]


def pair_values(rng, drel, mrel, lo, hi):
    """(d index forward, d index reverse, matches forward, matches reverse) with d_rc `drel` d_or, matches_rc `mrel` matches_or; d
    indices in [lo, hi]"""
    a, b = sorted(int(x) for x in rng.choice(np.arange(lo, hi + 1), 2, replace=False))
    d_or, d_rc = {"<": (b, a), "=": (a, a), ">": (a, b)}[drel]
    x, y = sorted(int(v) for v in rng.choice([1, 2, 3], 2, replace=False))
    m_or, m_rc = {"<": (y, x), "=": (x, x), ">": (x, y)}[mrel]
    return d_or, d_rc, m_or, m_rc


def seam_read(rng, ix, lay, n, t, focus=True):
    """a read of n records with a strand pair at every seam; variant t: pair j that does not host the closest takes the (d, matches)
    relation (t + j) % 9 -- every seam meets all nine over nine variants --, pair (t // 9 + t % 9) % npairs hosts the closest as
    FOCUS[t % 9] says (9 npairs variants give every pair every entry of FOCUS; a large read is given nine: what the closest does
    to a pair -- the override -- is decided from two broadcast values, the same in every lane and step); focus=False: the closest is a
    record of no seam's pair"""
    ps = seams(lay, n)
    keys = make_keys(rng, ix.leaf_se, n, pairs=ps)
    floor = int(rng.integers(0, 4))  # the read's smallest d; everything that is not the closest lies above it
    dix = rng.integers(floor + 1, 6, n)
    ms = rng.integers(1, 4, n)
    for j, p in enumerate(ps):
        c = (t + j) % 9
        dix[p], dix[p + 1], ms[p], ms[p + 1] = pair_values(rng, REL[c // 3], REL[c % 3], floor + 1, 5)
    if ps and focus:
        p = ps[(t // 9 + t % 9) % len(ps)]
        role, drel, mrel = FOCUS[t % 9]
        _, _, ms[p], ms[p + 1] = pair_values(rng, "=", mrel, 4, 5)
        up = int(rng.integers(floor + 1, 6))
        dix[p], dix[p + 1] = (floor, up) if role == "or" else ((up, floor) if drel == "<" else (floor, floor))
    elif n:  # the closest elsewhere: at a record of no seam's pair if there is one
        free = [i for i in range(n) if all(i != p and i != p + 1 for p in ps)] or [0]
        dix[free[int(rng.integers(0, len(free)))]] = floor
    return records(rng, keys, dix, ms)


def design_seams(ix, lay, seed=0):
    rng = np.random.default_rng(100 + seed)
    reads = []
    for n in sizes(lay):
        for t in range(9 * max(1, len(seams(lay, n))) if n <= lay["wave_gl"] else 9):
            reads.append(seam_read(rng, ix, lay, n, t))
        for t in range(9):
            reads.append(seam_read(rng, ix, lay, n, t, focus=False))
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


def design_ties(ix, lay, seed=0):
    """the minimal d at several records far apart: in different lanes, steps and passes; a forward record at a high index against a
    reverse one at a low index (strand beats index); all d equal"""
    rng = np.random.default_rng(200 + seed)
    gl, big = lay["wave_gl"], lay["big_regs"]
    reads = []
    for n in sizes(lay):
        if n < 2:
            continue
        sets = [{0, n - 1}, {gl - 1, gl}, {big - 1, big}]
        if n > big:
            p = int(rng.integers(0, n - big))
            sets.append({p, p + big})
        sets = [s for s in sets if max(s) < n]
        for s in sets:
            for strands in (None, (1, 0)):  # as they come; or the low index on the reverse strand, the high one on the forward strand
                lo, hi = min(s), max(s)
                sa = {lo: strands[0], hi: strands[1]} if strands and hi > lo + 1 else None
                keys = make_keys(rng, ix.leaf_se, n, strand_at=sa)
                floor = int(rng.integers(0, 5))
                dix = rng.integers(floor + 1, 6, n)
                for i in s:
                    dix[i] = floor
                reads.append(records(rng, keys, dix, rng.integers(1, 4, n)))
        keys = make_keys(rng, ix.leaf_se, n)
        reads.append(records(rng, keys, np.full(n, int(rng.integers(0, 6))), rng.integers(1, 4, n)))  # all d equal
    order = rng.permutation(len(reads))
    return [reads[i] for i in order]


# A border between two reads in adjacent slots: the earlier read ends in the forward record of a leaf, the later one starts with that
# leaf's reverse record.  (d index of the forward record, of the reverse one, matches forward, matches reverse) and which of the two
# would stand for the leaf IF a form took them for a pair: where the forward record would win, a lost backward guard (`gl > 0`, `t > 0`)
# unselects the later read's first record; where the reverse one would, a lost forward guard (`gl + 1 < n`, `t + 1 < n`) unselects the
# earlier read's last.  Consecutive borders alternate, decided by d and by matches in turn.
BORDERS = ((3, 4, 2, 2, "or"), (4, 3, 2, 2, "rc"), (3, 3, 3, 1, "or"), (3, 3, 2, 2, "rc"))


def design_neighbours(ix, lay, seed=0):
    """chains of reads in adjacent record slots where one read ends in key 2s and the next starts with 2s + 1, border q of chain c as
    BORDERS[(q + c) % 4] says: they are no pair, whichever lanes, groups, steps or slots they share.  Chains of reads that fill their
    group of 16 or 32 lanes, the wave, a step of a lane's walk, of reads above 64 records (the loops that look at rec_key[i - 1] and
    rec_key[i + 1] in memory, the register form and the two-pass form), and mixed ones; 5 small reads between the chains.  The two
    mirror chains (one read ends in 2s + 1, the next starts with 2s) are there for completeness: a reverse record looks backward and a
    forward one forward, so no guard stands between them."""
    rng = np.random.default_rng(300 + seed)
    L, gs, gm, gl, big = (lay[k] for k in ("lane_max", "group_small", "group_mid", "wave_gl", "big_regs"))
    reads = []
    chains = [[gs] * 9, [gm] * 5, [gl] * 3, [4] * 8, [L] * 8, [gs, gs - 1, gs, gm, gm, gs, L, 4, gl, gs, gs], [gl + 1] * 3, [2 * gl] * 3, [big] * 3,
              [big + 1] * 3, [gs] * 5, [gm] * 3]
    for c, ns in enumerate(chains):
        mirror = c >= len(chains) - 2
        leaf = 2
        for q, n in enumerate(ns):
            first = None if q == 0 else (leaf, 0 if mirror else 1)
            nxt = leaf + n + 8
            last = None if q == len(ns) - 1 else (nxt, 1 if mirror else 0)
            keys = make_keys(rng, ix.leaf_se, n, first=first, last=last, p_pair=0.2)
            dix = rng.integers(2, 6, n)
            ms = rng.integers(1, 4, n)
            dix[n // 2] = 0  # the closest: elsewhere, so that no override hides the border records
            if q > 0:
                _, dix[0], _, ms[0], _ = BORDERS[(q + c) % 4]
            if q < len(ns) - 1:
                dix[n - 1], _, ms[n - 1], _, _ = BORDERS[(q + 1 + c) % 4]
            reads.append(records(rng, keys, dix, ms))
            leaf = nxt
        for _ in range(5):
            reads.append(seam_read(rng, ix, lay, int(rng.integers(0, 4)), 0))
    return reads


def design_dmax(ix, lay, seed=0):
    """the closest below, exactly at POOL[2] or at POOL[3], the other records at, just above and above it: with dist_max from DMAX
    the comparisons with dist_max are decided by one double"""
    rng = np.random.default_rng(400 + seed)
    reads = []
    for n in (1, 3, lay["lane_max"], 12, 24, 48, 100, lay["big_regs"] + 44):
        for floor in (1, 2, 3):
            for _ in range(3):
                keys = make_keys(rng, ix.leaf_se, n)
                dix = rng.integers(floor, 5, n)
                dix[int(rng.integers(0, n))] = floor
                reads.append(records(rng, keys, dix, rng.integers(1, 4, n)))
    return reads


WAVE_SMALL = (1, 4, 5, 8, 9)  # reads of 9..16 records in a wave: one round of the 16-lane loop, one full, a second with three idle groups, ...
WAVE_MID = (1, 2, 3)          # reads of 17..32 records: half a round, one round, a second with an idle group


def design_waves(ix, lay, nreads, seed=0):
    """nreads reads, wave by wave of 64: wave w holds WAVE_SMALL[w % 5] reads of group_small's form, WAVE_MID[w % 3] of group_mid's, every
    fourth wave one read of each larger form, an empty read between the two largest; wave 1 (if there is one) is all large reads; the rest are
    reads of 0 .. lane_max records"""
    rng = np.random.default_rng(500 + seed + nreads)
    L, gs, gm, gl, big = (lay[k] for k in ("lane_max", "group_small", "group_mid", "wave_gl", "big_regs"))
    ns = []
    for w in range((nreads + 63) // 64):
        wave = [int(rng.integers(0, L + 1)) for _ in range(64)]
        slots = list(rng.permutation(64))
        if w == 1:
            wave = [int(rng.choice([gm + 1, gl, gl + 1, 2 * gl, big, big + 1])) if i % 8 else big + 130 for i in range(64)]
        else:
            if w % 4 == 0:
                s = min(slots[-1], 60)
                wave[s:s + 4] = [int(rng.integers(gm + 1, gl + 1)), int(rng.integers(gl + 1, big + 1)), 0, big + 1 + int(rng.integers(0, 300))]
                slots = [x for x in slots if not s <= x < s + 4]
            for _ in range(WAVE_SMALL[w % 5]):
                wave[slots.pop()] = int(rng.integers(L + 1, gs + 1))
            for _ in range(WAVE_MID[w % 3]):
                wave[slots.pop()] = int(rng.integers(gs + 1, gm + 1))
        ns += wave
    ns = ns[:nreads]
    if nreads == 1:
        ns = [gs]
    return [seam_read(rng, ix, lay, n, int(rng.integers(0, 27))) for n in ns]


SEEDS = (0, 1)  # of the designs whose keys, pairs and values are drawn at random around fixed seams
WAVE_NREADS = (1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 1040)  # around the wave, the workgroup's 256 lanes, the row block and its round


def designs(ix, lay):
    """name -> function that builds the design's reads"""
    d = {}
    for seed in SEEDS:  # name, name_s1, ...
        sfx = f"_s{seed}" if seed else ""
        d.update({"seams" + sfx: lambda seed=seed: design_seams(ix, lay, seed), "ties" + sfx: lambda seed=seed: design_ties(ix, lay, seed),
                  "neighbours" + sfx: lambda seed=seed: design_neighbours(ix, lay, seed), "dmax" + sfx: lambda seed=seed: design_dmax(ix, lay, seed)})
    for n in WAVE_NREADS:
        d[f"waves{n}"] = (lambda n=n: design_waves(ix, lay, n))
    return d


def hist_of(rng, m, np_planes):
    h = [0] * np_planes
    for _ in range(m):
        h[int(rng.integers(0, np_planes))] += 1
    return h


def value_tables():
    """the list of distinct values and the direct places: place p names list position PERM[p]; two places name nothing"""
    rep_dv = np.array([[POOL[j % 6], -1.0 - j / 64.0] for j in range(NREP)])
    perm = np.random.default_rng(7).permutation(NREP)
    dd_direct = np.concatenate([perm, [HOLE, HOLE]]).astype(np.uint32)
    dd_dv = np.concatenate([rep_dv[perm], np.full((2, 2), np.nan)])
    place_of = np.argsort(perm)
    return rep_dv, dd_direct, dd_dv, place_of


def tables(reads, th=4, contiguous=False, seed=1):
    """the kr_debug_select tables of a design, and per read the records as select_ref takes them.  th != 4: no packed words and no direct
    places (the stream has neither).  Record slots that belong to no read lie between the reads unless `contiguous`."""
    rng = np.random.default_rng(seed)
    np_planes = th + 1
    rep_dv, dd_direct, dd_dv, place_of = value_tables()
    rd_off, rd_cnt, rd_onmers = [], [], []
    key, rep, w0, hist, rread, ref = [], [], [], [], [], []

    def hole(c):
        for _ in range(c):
            key.append(0), rep.append(HOLE), w0.append(0), hist.append([0] * np_planes), rread.append(0)

    for r, recs in enumerate(reads):
        if not contiguous:
            hole(int(rng.integers(0, 3)))
        onmers = 100 + r % 40
        rd_off.append(len(key)), rd_cnt.append(len(recs)), rd_onmers.append(onmers)
        for x in recs:
            h = hist_of(rng, x["m"], np_planes)
            packed, direct = x["packed"] and th == 4, x["direct"] and th == 4
            key.append(x["key"])
            rep.append(DIRECT_FLAG | int(place_of[x["j"]]) if direct else x["j"])
            w0.append((sum(c << (8 * i) for i, c in enumerate(h)) | onmers << 40 | 1 << 63) if packed else 0)
            hist.append(h if not packed or rng.random() < 0.5 else [0] * np_planes)  # (a packed record's planes are not looked at)
            rread.append(r)
        ref.append([(x["key"], float(rep_dv[x["j"], 0]), float(rep_dv[x["j"], 1]), x["m"]) for x in recs])
    hole(2)
    t = dict(rd_off=np.array(rd_off, np.uint32), rd_cnt=np.array(rd_cnt, np.uint32), rd_onmers=np.array(rd_onmers, np.uint32),
             rec_key=np.array(key, np.uint32), rec_rep=np.array(rep, np.uint32), rec_w0=np.array(w0, np.uint64),
             rec_hist=np.array(hist, np.uint32).reshape(-1, np_planes), rec_read=np.array(rread, np.uint32), rep_dv=rep_dv)
    if th == 4:
        t.update(dd_direct=dd_direct, dd_dv=dd_dv)
    pos = np.array([x["j"] for recs in reads for x in recs], np.uint32)  # the resolved list position of every record, read by read
    return t, ref, pos


def reference(ref, multi, dist_max):
    """select_ref over the reads of a design (no --filter)"""
    return [select_ref(recs, multi=multi, no_filter=1, dist_max=dist_max) for recs in ref]


# ---------------------------------------------------------------------------
# --filter: chi = 2 (f(closest's problem, d) - v_closest) per representing record
# ---------------------------------------------------------------------------
FILTER_SIZES = (0, 1, 63, 64, 65, 128, 129, 300)


def filter_case(ix, th, seed=0):
    """Reads of FILTER_SIZES records (three each) for kr_select_kernel<NPT, true>: every record has a list position of its own that
    carries (d, f_ieee(its problem, d)), d from POOL.  Returns (tables, per read the select_ref records, per read f(ic, d), per read
    err(ic, d) = llh_mp.err_unit of record ic's problem at d)."""
    from llh_mp import err_unit, f_ieee

    rng = np.random.default_rng(600 + seed + th)
    npl = th + 1
    rd_off, rd_cnt, rd_onmers, key, rep, w0, hist, rread, dv, ddir, ddv = [], [], [], [], [], [], [], [], [], [], []
    ref, fs, errs = [], [], []
    for r, n in enumerate(n for n in FILTER_SIZES for _ in range(3)):
        onmers = 100 + r
        keys = make_keys(rng, ix.leaf_se, n)
        rd_off.append(len(key)), rd_cnt.append(n), rd_onmers.append(onmers)
        probs, recs = [], []
        for k_ in keys:
            m = int(rng.integers(1, 4))
            h = hist_of(rng, m, npl)
            d = POOL[int(rng.integers(0, 6))]
            prob = (K, H, th, [float(c) for c in h], float(onmers - m), ix.rho[k_ >> 1])
            v = f_ieee(*prob, d)
            j = len(dv)
            dv.append((d, v))
            packed, direct = th == 4 and bool(rng.integers(0, 2)), th == 4 and bool(rng.integers(0, 2))
            if direct:
                ddir.append(j), ddv.append((d, v))
            key.append(k_), rep.append(DIRECT_FLAG | (len(ddir) - 1) if direct else j), rread.append(r), hist.append(h)
            w0.append((sum(c << (8 * i) for i, c in enumerate(h)) | onmers << 40 | 1 << 63) if packed else 0)
            probs.append(prob), recs.append((k_, d, v, m))
        ref.append(recs)
        fs.append(lambda ic, d, probs=probs: f_ieee(*probs[ic], d))
        errs.append(lambda ic, d, probs=probs: err_unit(*probs[ic], d))
    t = dict(rd_off=np.array(rd_off, np.uint32), rd_cnt=np.array(rd_cnt, np.uint32), rd_onmers=np.array(rd_onmers, np.uint32),
             rec_key=np.array(key, np.uint32), rec_rep=np.array(rep, np.uint32), rec_w0=np.array(w0, np.uint64),
             rec_hist=np.array(hist, np.uint32).reshape(-1, npl), rec_read=np.array(rread, np.uint32), rep_dv=np.array(dv))
    if th == 4:
        t.update(dd_direct=np.array(ddir, np.uint32), dd_dv=np.array(ddv))
    return t, ref, fs, errs


def filter_reference(ref, fs, errs, dist_max=None):
    """select_ref under --filter with the threshold in the widest gap of the case's chi values between their quartiles.  Returns
    (chisq, per read select_ref's result, the smallest |chi - chisq| / bound over the case) with bound = 2 M_GPU B + ulp(chi): the device's
    chi may differ from the reference's by at most that (tests/llh_mp.py), so a ratio of 4 and more leaves every selection flag determined."""
    from llh_mp import M_GPU

    first = [select_ref(recs, multi=1, no_filter=0, dist_max=dist_max, chisq=0.0, f=f) for recs, f in zip(ref, fs)]
    chi = sorted(c for o in first for c in o["chi"] if c is not None)
    lo, hi = len(chi) // 4, 3 * len(chi) // 4
    g = max(range(lo, hi), key=lambda i: chi[i + 1] - chi[i])
    chisq = 0.5 * (chi[g] + chi[g + 1])
    ratio = math.inf
    for recs, o, err in zip(ref, first, errs):
        for i, c in enumerate(o["chi"]):
            if c is not None:
                ratio = min(ratio, abs(c - chisq) / (2 * M_GPU * err(o["closest"], recs[i][1]) + math.ulp(c)))
    out = [select_ref(recs, multi=1, no_filter=0, dist_max=dist_max, chisq=chisq, f=f) for recs, f in zip(ref, fs)]
    return chisq, out, ratio
