"""A table designer for the scan kernels' bounds logic, with a plain reference.

A design places, in the row of a chosen (read, position, strand) k-mer, a bucket of a chosen length whose matching entries sit at
chosen ordinals; filler entries in the row below set the bucket's start alignment in the packed arrays, and the query's exact code may
stand guard as the last entry of the row below and the first entry of the row above.  The lengths, ordinals and alignments come from
the layout numbers the library reports (capi.scan_layout), never from literals: docs/design/03_scan.md has the boundary table.

`reference` knows nothing of layouts: every k-mer of both strands, every entry of its row, hd32.  From that the hits (read, strand,
kpos, lib, cmer_index, hd, se), hdist_filt per strand, onmers, per group of 64 positions the probes located / with a non-empty row / with
a hit, and per read the hits per segment.  Records and histograms are the oracle's.

Geometries (k = 23, h = 7: 16,384 hash values, 16 non-LSH positions): "one" a library that serves every residue (m = 2, r = 1, frac),
"two" two no_frac libraries in one directory (r = 0 and r = 1), "half" half of the residues served (m = 4, r = 1, frac: whether a probe
has a row is decided by one base of the read, so odd probe counts can be designed)."""
import numpy as np

from acc_craft import Tree
from helpers import closed_form, hd32, revcomp, row_of, write_index

K, H = 23, 7
PPOS = [22, 20, 17, 13, 9, 5, 2]
NPOS = [p for p in range(K) if p not in PPOS]
P0 = min(PPOS)  # rix % 4 is the code of the base at this position of the k-mer (counted from its last base)
GEOS = {"one": [(2, 1, True)], "two": [(2, 0, False), (2, 1, False)], "half": [(4, 1, True)]}
NLEAF = 8
TH = 4
LOW_ROWS = 8  # rows below this are kept for the buckets that start at packed index 0 and 1
_POP16 = np.array([bin(i).count("1") for i in range(65536)], np.uint8)


def nrows_of(m, r, frac):
    return (4 ** H // m) * (r + 1) if frac else 4 ** H // m


def kmer_of(rix, enc):
    """the k-mer whose LSH index is rix and whose residual code is enc (closed_form's inverse)"""
    c = [0] * K
    for j, p in enumerate(sorted(PPOS)):
        c[p] = (rix >> (2 * j)) & 3
    for j, p in enumerate(sorted(NPOS)):
        c[p] = ((enc >> j) & 1) | (((enc >> (16 + j)) & 1) << 1)
    s = "".join("ACGT"[c[K - 1 - i]] for i in range(K))
    f = closed_form(s, PPOS, NPOS)
    assert f[2] == rix and f[3] == enc
    return s


class Retry(Exception):
    """this random read does not fit its design: take another one"""


class Read:
    def __init__(self, name, seq, expect):
        self.name, self.seq, self.expect = name, seq, expect
        self.probes = []  # (pos, strand, lib, row, enc) of the designed probes, in the order of the design's specs


class Craft:
    """The tables under construction for one geometry and one layout."""

    def __init__(self, geo, lay, seed=7):
        self.geo, self.lay = geo, lay
        self.libs = GEOS[geo]
        self.tree = Tree(NLEAF)
        self.pse = list(self.tree.children)
        self.rng = np.random.default_rng(seed)
        self.rows = [dict() for _ in self.libs]   # the final tables (finalize): row -> [(enc, se)]
        self.plan = [dict() for _ in self.libs]   # row -> dict(ent=[enc...], align, guard)
        self.used = [set() for _ in self.libs]    # designed rows and the rows that serve them (filler below, guard above)
        self.start = [dict() for _ in self.libs]  # row -> packed index of its first entry (finalize)
        self.touched = [set() for _ in self.libs] # rows that a strict read probes: no later design may fill them
        self.reads = []
        self.final = False
        self._se = 0

    # ---- geometry
    def locate(self, rix):
        for li, (m, r, frac) in enumerate(self.libs):
            row = row_of(rix, m, r, frac)
            if row is not None:
                return li, row
        return None

    def rix_of(self, lib, row):
        m, r, frac = self.libs[lib]
        return (row // (r + 1)) * m + row % (r + 1) if frac else row * m + r

    def probes(self, seq):
        """{(pos, strand): (lib, row, enc)} of the k-mers of seq that have a row"""
        out = {}
        for i in range(len(seq) - K + 1):
            km = seq[i:i + K]
            if any(ch not in "ACGT" for ch in km):
                continue
            for s, x in ((0, km), (1, revcomp(km))):
                f = closed_form(x, PPOS, NPOS)
                loc = self.locate(f[2])
                if loc is not None:
                    out[(i, s)] = (loc[0], loc[1], f[3])
        return out

    def random_seq(self, n):
        return "".join("ACGT"[i] for i in self.rng.integers(0, 4, n))

    def read(self, name, seq, expect):
        r = Read(name, seq, expect)
        self.reads.append(r)
        return r

    def leaf(self):
        self._se += 1
        return self.tree.leaf_se[self._se % NLEAF]

    # ---- buckets
    def entries(self, q, length, hits=(), dense=False):
        """`length` codes with the query's high half, sorted: those at the ordinals `hits` ({ordinal: hd}, or ordinals: the first one
        the query's own code, the others at hd 1..4) within th = 4, every other one at hd >= 8; dense: all of them at hd 1..4"""
        ql, qh = q & 0xFFFF, q >> 16
        d = _POP16[np.arange(65536) ^ ql]
        if dense:
            pool = np.nonzero((d >= 1) & (d <= 4))[0]
            return [(qh << 16) | int(v) for v in np.sort(self.rng.choice(pool, length, replace=False))]
        hits = dict(hits) if isinstance(hits, dict) else {j: (0, 1, 2, 3, 4, 1, 2, 3, 4)[n % 9] for n, j in enumerate(sorted(hits))}
        assert all(0 <= j < length for j in hits)
        far = np.nonzero(d >= 8)[0]
        low, prev, prev_j = [], -1, -1
        for j in sorted(hits):
            gap = j - prev_j - 1
            cand = np.nonzero(d == hits[j])[0]
            cand = cand[cand > prev]
            ok = cand[np.searchsorted(far, cand) - np.searchsorted(far, prev + 1) >= gap]
            if not len(ok):
                raise Retry
            spread = ok[ok >= 65536 * (j + 1) // (length + 2)]  # (leave the entries behind this one their room)
            v = int(spread[0] if len(spread) else ok[0])
            between = far[(far > prev) & (far < v)]
            low += sorted(self.rng.choice(between, gap, replace=False).tolist()) + [v]
            prev, prev_j = v, j
        rest = far[far > prev]
        if len(rest) < length - 1 - prev_j:
            raise Retry
        low += sorted(self.rng.choice(rest, length - 1 - prev_j, replace=False).tolist())
        out = [(qh << 16) | int(v) for v in low]
        assert out == sorted(set(out)) and len(out) == length
        assert all((hd32(e, q) <= 4) == (j in hits) and (j in hits or hd32(e, q) >= 8) for j, e in enumerate(out))
        return out

    def rows_for(self, row, align, guard):
        return {row} | ({row - 1} if (align is not None or guard) else set()) | ({row + 1} if guard else set())

    def bucket(self, lib, row, ent, align=None, guard=None):
        """plan the bucket of a row: its codes, the start alignment (packed index & 3) that filler in the row below gives it, and the
        code that stands guard as the last entry of the row below and the only entry of the row above"""
        assert not self.final and not (self.rows_for(row, align, guard is not None) & self.used[lib])
        self.plan[lib][row] = dict(ent=list(ent), align=align, guard=guard)
        self.used[lib] |= self.rows_for(row, align, guard is not None)

    def make(self, name, n, expect, specs, seq=None, strict=False):
        """A read of n random bases (or seq(), called anew for every attempt) with one designed bucket per spec: dict(length, hits, dense,
        lo, hi, strand: where the probe may lie; at: the probe itself; align, guard).  specs may be a function of the read's probes.
        A read none of whose probes fits (row taken, no room for the codes) is replaced by another one.  strict: the read's counts matter,
        not only its designed rows: every other probe of it finds an empty row, now and after the designs that follow."""
        for _ in range(4000):
            r = Read(name, seq() if seq else self.random_seq(n), expect)
            pr = self.probes(r.seq)
            try:
                todo, taken, rows = [], set(), [set() for _ in self.libs]
                for sp in (specs(pr) if callable(specs) else specs):
                    align, guard = sp.get("align"), sp.get("guard", False)
                    for key in ([sp["at"]] if "at" in sp else sorted(pr)):
                        if key not in pr or key in taken:
                            continue
                        pos, s = key
                        lib, row, enc = pr[key]
                        if not (sp.get("lo", 0) <= pos < sp.get("hi", 1 << 30)) or sp.get("strand", s) != s:
                            continue
                        need = self.rows_for(row, align, guard)
                        if row < LOW_ROWS or row >= nrows_of(*self.libs[lib]) - 1 or need & (self.used[lib] | rows[lib] | self.touched[lib]):
                            continue
                        if guard and enc < 1 << 24:  # (the filler below a guard is smaller than the guard)
                            continue
                        break
                    else:
                        raise Retry
                    ent = self.entries(enc, sp["length"], sp.get("hits", ()), sp.get("dense", False)) if sp["length"] else []
                    todo.append(((pos, s, lib, row, enc), ent, align, enc if guard else None))
                    taken.add(key)
                    rows[lib] |= need
                if strict and any(k_ not in taken and (row < LOW_ROWS or row in self.used[lib] or row in rows[lib]) for k_, (lib, row, enc) in pr.items()):
                    raise Retry
            except Retry:
                continue
            if strict:
                for lib, row, enc in pr.values():
                    self.touched[lib].add(row)
            for p, ent, align, guard in todo:
                self.bucket(p[2], p[3], ent, align, guard)
                r.probes.append(p)
            self.reads.append(r)
            return r
        raise AssertionError(f"{name}: no read fits this design")

    def finalize(self):
        """lay the planned buckets out: filler (small codes) in the row below gives a bucket its start alignment"""
        assert not self.final
        for lib, plan in enumerate(self.plan):
            total, filler = 0, 1
            for row in sorted(plan):
                b = plan[row]
                g = [b["guard"]] if b["guard"] is not None else []
                pad = (b["align"] - total - len(g)) % 4 if b["align"] is not None else 0
                below = list(range(filler, filler + pad)) + g
                filler += pad
                if below:
                    assert row - 1 not in self.rows[lib] and row - 1 not in plan
                    self.rows[lib][row - 1] = [(e, self.leaf()) for e in below]
                    self.start[lib][row - 1] = total
                    total += len(below)
                assert b["align"] is None or total % 4 == b["align"]
                self.start[lib][row] = total
                if b["ent"]:
                    self.rows[lib][row] = [(e, self.leaf()) for e in b["ent"]]
                    total += len(b["ent"])
                if g:
                    assert row + 1 not in self.rows[lib] and row + 1 not in plan
                    self.rows[lib][row + 1] = [(g[0], self.leaf())]
                    self.start[lib][row + 1] = total
                    total += 1
        self.final = True

    def write(self, path):
        assert self.final
        t = self.tree
        rho = [0.0] + [0.25 if t.kind[se] == 1 else 0.0 for se in range(1, t.nnodes + 1)]
        for (m, r, frac), rows in zip(self.libs, self.rows):
            write_index(path, K, H, m, r, frac, PPOS, rows, self.pse, rho, nwk=t.nwk)
        return path

    def batch(self, reads=None):
        seqs = [r.seq for r in (self.reads if reads is None else reads)]
        bases = np.frombuffer("".join(seqs).encode(), np.uint8)
        offs = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        return bases, offs


def reference(cr, seqs, th=TH):
    """Per read: dict(onmers, hdist_filt [2], hits [(strand, kpos, lib, cmer_index, hd, se)]; per group of 64 positions the probes
    located / with a non-empty row / with a hit; seg_hits per segment; items = hits + one marker per later segment with a hit; probed =
    {(lib, row): (start, length)} of the non-empty buckets probed; hit_ords = {(lib, row): [ordinal of every hit]})."""
    out = []
    for seq in seqs:
        npos = max(0, len(seq) - K + 1)
        ngr = max(1, (npos + 63) // 64)
        c = dict(onmers=0, hdist_filt=[0xFFFFFFFF, 0xFFFFFFFF], hits=[], located=[0] * ngr, nonempty=[0] * ngr, hit_probes=[0] * ngr,
                 seg_hits=[0] * ((ngr + 1) // 2), probed={}, hit_ords={})
        for i in range(npos):
            km = seq[i:i + K]
            if any(ch not in "ACGTacgt" for ch in km):
                continue
            c["onmers"] += 1
            for s, x in ((0, km), (1, revcomp(km))):
                f = closed_form(x, PPOS, NPOS)
                loc = cr.locate(f[2])
                if loc is None:
                    continue
                lib, row = loc
                c["located"][i // 64] += 1
                ent = sorted(cr.rows[lib].get(row, []))
                if not ent:
                    continue
                c["nonempty"][i // 64] += 1
                c["probed"][(lib, row)] = (cr.start[lib][row], len(ent))
                n = 0
                for o, (enc, se) in enumerate(ent):
                    hd = hd32(enc, f[3])
                    if hd <= th:
                        c["hits"].append((s, i, lib, cr.start[lib][row] + o, hd, se))
                        c["hdist_filt"][s] = min(c["hdist_filt"][s], hd)
                        c["hit_ords"].setdefault((lib, row), []).append(o)
                        n += 1
                if n:
                    c["hit_probes"][i // 64] += 1
                    c["seg_hits"][i // 128] += n
        c["items"] = len(c["hits"]) + sum(1 for n in c["seg_hits"][1:] if n)
        out.append(c)
    return out


def nact_of(c, lay):
    """probes the scan lists per group: every located probe of a slotted table, the non-empty ones of a packed table"""
    return c["located"] if lay["slotted"] else c["nonempty"]


def half_read(cr, npos, nloc):
    """geometry "half": a read of npos (<= 64) k-mer positions of which exactly nloc probes have a row.  The forward probe of position i
    has one iff base i + K - 1 - P0 of the read is A or C, the reverse probe iff base i + P0 is G or T: a base that both kinds of probe
    look at gives one row whatever it is, the bases only one looks at are chosen."""
    assert cr.geo == "half"
    seq = list(cr.random_seq(npos + K - 1))
    fwd = {i + K - 1 - P0 for i in range(npos)}
    rev = {i + P0 for i in range(npos)}
    left = nloc - len(fwd & rev)
    assert 0 <= left <= len(fwd ^ rev), (npos, nloc)
    for b in sorted(fwd ^ rev):
        on = left > 0
        left -= on
        seq[b] = ("AC" if (b in fwd) == on else "GT")[int(cr.rng.integers(0, 2))]
    return "".join(seq)


def designs(lay, geo, seed=7):
    """The crafted tables and designed reads for one layout (capi.scan_layout) and geometry: a finalized Craft.  Every read carries
    `expect`, its predicate at th = 4 over the reference's counts c, nact = nact_of(c, layout), p = the read's designed probes
    (pos, strand, lib, row, enc) and S(lib, row) = the packed index of a row's first entry."""
    cr = Craft(geo, lay, seed)
    G, CPL, PPS = lay["G"], lay["CPL"], lay["PPS"]
    slotted, LINE = bool(lay["slotted"]), lay["line_codes"]
    CAP = lay["CAP"] if slotted else 0
    E = 4 * G * CPL                      # entries of every bucket that a pass covers
    F = lay["step_bits"] // CPL          # passes' worth of steps before the packed scan_group flushes
    SEG, STAGE, CHUNK, LIST = lay["seg_pos"], lay["item_stage"], lay["item_chunk"], lay["list_cap"]
    ords_of = "sorted(c['hit_ords'][p[0][2:4]])"
    len_of = "c['probed'][p[0][2:4]][1]"
    start_of = "c['probed'][p[0][2:4]][0]"

    # ---- groups first, while every row is free.  nact = PPS, PPS + 2, 128 = the list's capacity: every probe of 64 positions with a hit
    #      (more than 64 hit chunks; the last probe's hit in the last chunk of its slot or pass: the group's last hit bit); 127 on packed
    #      tables (one row left empty, and so PPS - 1 and PPS + 1); exactly 64 hit chunks (32 positions)
    if geo != "half":
        last_len = CAP if slotted else E
        for name, npos, skip in (("group_full", LIST // 2, 0), ("group_minus_1", LIST // 2, 1), ("group_64_hits", 32, 0), ("group_pps", PPS // 2, 0),
                                 ("group_pps_plus_2", PPS // 2 + 1, 0), ("group_pps_minus_1", PPS // 2, 1), ("group_pps_plus_1", PPS // 2 + 1, 1)):
            want = 2 * npos - skip
            full = name == "group_full"

            def specs(pr, want=want, full=full, npos=npos):
                if len(pr) != 2 * npos:
                    raise Retry
                keys = sorted(pr, key=lambda k_: (k_[1], k_[0]))[:want]  # (the list's order: forward probes, then reverse)
                return [dict(length=last_len, hits={last_len - 1: 1}, at=k_, align=0) if full and k_ == keys[-1] else dict(length=1, hits={0: 0}, at=k_)
                        for k_ in keys]

            cr.make(name, K + npos - 1, f"c['nonempty'][0] == {want} and c['hit_probes'][0] == {want} and c['located'][0] == {2 * npos} "
                    f"and len(c['hits']) == {want} and max(l for s, l in c['probed'].values()) == {last_len if full else 1}"
                    + (f" and c['hit_ords'][p[-1][2:4]] == [{last_len - 1}] and p[-1][:2] == ({npos - 1}, 1)" if full else ""), specs, strict=True)
    else:  # odd probe counts: 0, 1, PPS - 1, PPS, PPS + 1 located probes in a group (slotted tables list them all), one of them with a hit
        for nloc in (0, 1, PPS - 1, PPS, PPS + 1):
            npos = 16 if nloc <= 32 else 64
            cr.make(f"located_{nloc}", 0, f"c['located'][0] == {nloc} and c['nonempty'][0] == {min(nloc, 1)} and len(c['hits']) == {min(nloc, 1)}",
                    [dict(length=1, hits={0: 0})] if nloc else [], seq=lambda npos=npos, nloc=nloc: half_read(cr, npos, nloc), strict=True)
    # ---- packed: the step bits used up exactly at a pass boundary -- the first probe's bucket takes F - 1 passes' worth of steps, the second
    #      pass one more; a third pass (where the list has room) comes after the flush
    if not slotted and geo != "half":
        nprobe = min(2 * PPS + 1, LIST)
        big = E * (F - 1)

        def specs(pr, nprobe=nprobe, big=big):
            keys = sorted(pr, key=lambda k_: (k_[1], k_[0]))[:nprobe]
            return [dict(length=big, hits={0: 0, big - 1: 1}, at=k_, align=0) if n == 0 else dict(length=1, hits={0: 0}, at=k_) for n, k_ in enumerate(keys)]

        cr.make("flush_at_pass_end", K + 63, f"nact[0] == {nprobe} and len(c['hits']) == {nprobe + 1} and {len_of} == {big} == {E} * ({lay['step_bits']} // {CPL} - 1) "
                f"and {start_of} % 4 == 0 and {ords_of} == [0, {big - 1}]", specs, strict=True)
    # ---- the item stage: a read of STAGE - 1, STAGE, STAGE + 1 items from two groups of one segment (every entry of two buckets is a hit)
    for d in (-1, 0, 1):
        cr.make(f"items_{STAGE + d}", K + 64, f"c['items'] == {STAGE + d} and c['hit_probes'][0] >= 1 and c['hit_probes'][1] >= 1 and len(c['seg_hits']) == 1",
                [dict(length=200, dense=True, hi=40), dict(length=STAGE + d - 200, dense=True, lo=64)], strict=True)
    # ---- bucket lengths around the slot's capacity (slotted, filter slots) or around a pass (packed); hits at the first and last entry and
    #      at the layout's own edges: entry 0, 1, 2 (first word of a slot's chunk 1), CAP - 1 (last slot word), CAP (first tail entry)
    if slotted:
        lengths = [0, 1, 2, 3, CAP - 1, CAP] + [CAP + d for d in range(1, 6)] + ([LINE - 1, LINE, LINE + 1] if LINE else [])
    else:
        lengths = [0, 1, 2, 3, E - 1, E, E + 1, 2 * E + 1]
    for n in lengths:
        ords = sorted({j for j in (0, 1, 2, CAP - 1, CAP, n - 1, LINE - 1, LINE) if 0 <= j < n})
        cr.make(f"len_{n}", K + 40, (f"{ords_of} == {ords} and {len_of} == {n}") if n else "p[0][2:4] not in c['probed'] and sum(c['located']) > 0", [dict(length=n, hits=ords)])
    # ---- a tail (slotted: the entries past CAP, read from the packed arrays) at every alignment (start + CAP) & 3: one chunk, more than one
    #      round of the G lanes, about CAP + 200; hits in the last slot word and the first and last tail entry; the query's own code stands
    #      guard as the last entry of the row below and the first entry of the row above
    if slotted:
        for ta in range(4):
            for extra in (1, 4 * G + 3, 200):
                n = CAP + extra
                ords = sorted({CAP - 1, CAP, n - 1})
                cr.make(f"tail_{ta}_{extra}", K + 40, f"{ords_of} == {ords} and {len_of} == {n} and ({start_of} + {CAP}) % 4 == {ta} "
                        f"and {n} - {CAP} > {0 if extra == 1 else 4 * G}", [dict(length=n, hits=ords, align=(ta - CAP) % 4, guard=True)])
    # ---- chunks shared with the neighbouring buckets: every start alignment x lengths 1..9, guarded below and above; and a guarded bucket
    #      without a hit of its own, from which nothing may come out
    for a in range(4):
        for n in range(1, 10):
            ords = sorted({0, n - 1})
            cr.make(f"start_{a}_len_{n}", K + 40, f"{ords_of} == {ords} and {start_of} % 4 == {a} and {len_of} == {n} "
                    "and S(p[0][2], p[0][3] - 1) < S(p[0][2], p[0][3]) < S(p[0][2], p[0][3] + 1)", [dict(length=n, hits=ords, align=a, guard=True)])
        cr.make(f"guard_only_{a}", K + 40, f"p[0][2:4] not in c['hit_ords'] and {start_of} % 4 == {a} and {len_of} == 2", [dict(length=2, align=a, guard=True)])
    # ---- packed: a bucket longer than a flush's worth of steps, alone in its group: scan_group flushes in the middle of the bucket and resumes;
    #      hits in the last entry before the resumption point and in the first one after it
    if not slotted:
        for a in (0, 3):
            edge = E * F - a  # ordinal of the first entry that the second flush sees
            n = edge + E + 5
            ords = [0, edge - 1, edge, n - 1]
            cr.make(f"flush_resume_{a}", K, f"len(c['hits']) == 4 and {ords_of} == {ords} and {len_of} == {n} and {start_of} % 4 == {a} and sum(c['nonempty']) == 1 "
                    f"and {edge} + {a} == {E} * ({lay['step_bits']} // {CPL})", [dict(length=n, hits=ords, align=a)], strict=True)
    # ---- reads: lengths around k and around the ends of groups and segments; an N; hits at the read's first and last position
    for n in (K - 1, K, K + 63, K + 64, K + 127, K + 128):
        npos = max(0, n - K + 1)
        nd = 0 if n < K else (1 if n == K else 2)
        cr.make(f"length_{n}", n, f"c['onmers'] == {npos} and len(c['located']) == {max(1, (npos + 63) // 64)} and len(p) == {nd} and all(k_[2:4] in c['hit_ords'] for k_ in p)"
                + (f" and p[-1][0] == {npos - 1} and p[0][0] == 0" if nd else ""), [dict(length=3, hits=[1], lo=0, hi=1), dict(length=3, hits=[2], lo=npos - 1)][2 - nd:])

    def with_n():
        s = cr.random_seq(K + 100)
        return s[:60] + "N" + s[61:]

    cr.make("with_N", 0, f"c['onmers'] == {101 - K} and c['hit_ords'][p[0][2:4]] == [0] and c['hit_ords'][p[1][2:4]] == [1]", [dict(length=2, hits=[0], hi=60 - K + 1), dict(length=2, hits=[1], lo=61)], seq=with_n)
    # ---- three segments, the middle one without a hit: the marker in front of the third segment's first item carries its number
    cr.make("segments_1_3", K - 1 + 2 * SEG + 40, "c['seg_hits'][0] >= 2 and c['seg_hits'][1] == 0 and c['seg_hits'][2] >= 3 and c['items'] == sum(c['seg_hits']) + 1",
            [dict(length=5, hits=[0, 4], hi=SEG), dict(length=7, hits=[0, 3, 6], lo=2 * SEG)])
    cr.make("segments_2_3", K - 1 + 2 * SEG + 40, "c['seg_hits'][0] == 0 and c['seg_hits'][1] >= 1 and c['seg_hits'][2] >= 2 and c['items'] == sum(c['seg_hits']) + 2",
            [dict(length=1, hits=[0], lo=SEG, hi=2 * SEG), dict(length=7, hits=[0, 6], lo=2 * SEG)])
    # more item slots than a wave takes at a time, from every group of two segments: item_reserve moves the read's earlier items
    nb = CHUNK // 300 + 2
    cr.make("items_chunk", K - 1 + 2 * SEG, f"c['items'] > {CHUNK} + {STAGE} and all(c['hit_probes']) and len(c['hit_probes']) == 4 and c['seg_hits'][1] > 0",
            [dict(length=300, dense=True, lo=64 * (i % 4), hi=64 * (i % 4) + 64) for i in range(nb)])
    # ---- buckets that start at packed index 0 and 1 (the slot's start word - 2 wraps): rows 0 and 2 of every library
    for lib in range(len(cr.libs)):
        q0, q1 = (int(cr.rng.integers(1 << 24, 1 << 31)) & ~0xFFFF | 0x4321 for _ in range(2))
        cr.bucket(lib, 0, cr.entries(q0, 1, [0]))
        cr.bucket(lib, 2, cr.entries(q1, 3, [0, 2]))
        cr.read(f"index_0_lib{lib}", cr.random_seq(9) + kmer_of(cr.rix_of(lib, 0), q0) + cr.random_seq(9),
                f"S({lib}, 0) == 0 and ({lib}, 0) in c['hit_ords'] and [h[3] for h in c['hits'] if h[2] == {lib}][:1] == [0]")
        cr.read(f"index_1_lib{lib}", cr.random_seq(9) + kmer_of(cr.rix_of(lib, 2), q1) + cr.random_seq(9),
                f"S({lib}, 2) == 1 and c['hit_ords'][({lib}, 2)] == [0, 2]")
    # ---- rows at bit 0 and bit 31 of an occupancy word (packed tables with the bitmap), each beside a probed empty row
    for lib in range(len(cr.libs)):
        for bit, beside in ((0, 1), (31, -1)):
            while True:
                row = int(cr.rng.integers(2, nrows_of(*cr.libs[lib]) // 32 - 2)) * 32 + bit
                if not ({row - 1, row, row + 1} & (cr.used[lib] | cr.touched[lib])):
                    break
            q = int(cr.rng.integers(1 << 24, 1 << 31)) & ~0xFFFF | 0x4321
            cr.bucket(lib, row, cr.entries(q, 2, [0, 1]))
            cr.bucket(lib, row + beside, [])  # stays empty
            cr.read(f"occ_bit{bit}_lib{lib}", cr.random_seq(5) + kmer_of(cr.rix_of(lib, row + beside), q) + "AC" + kmer_of(cr.rix_of(lib, row), q) + cr.random_seq(5),
                    f"{row} % 32 == {bit} and c['hit_ords'][({lib}, {row})] == [0, 1] and ({lib}, {row + beside}) not in c['probed'] and sum(c['located']) > sum(c['nonempty'])")
    # ---- false positives in a slot's own words: rows whose entries are far from every small code, probed by queries that ARE the slot's
    #      length word and its start word (A-rich k-mers) and by codes at hd 1 from them; a short bucket probed by the all-ones code (a
    #      slot's unused words; T-rich)
    late = []
    for lib in range(len(cr.libs)):
        for kind, n in (("len_word", 5), ("start_word", 3), ("ones", 2)):
            while True:
                row = int(cr.rng.integers(LOW_ROWS + 1, nrows_of(*cr.libs[lib]) - 2))
                if not ({row - 1, row} & (cr.used[lib] | cr.touched[lib])):
                    break
            hi16 = 0x00F0 if kind == "ones" else 0xFF00
            cr.bucket(lib, row, sorted((hi16 + j) << 16 | int(cr.rng.integers(0, 65536)) for j in range(n)), align=1)
            late.append((kind, lib, row, n))
    cr.finalize()
    for kind, lib, row, n in late:
        q = {"len_word": n, "start_word": cr.start[lib][row], "ones": 0xFFFFFFFF}[kind]
        for flip in (0, 1):
            cr.read(f"false_{kind}_lib{lib}_{flip}", cr.random_seq(7) + kmer_of(cr.rix_of(lib, row), q ^ (flip << 9)) + cr.random_seq(7),
                    f"c['probed'][({lib}, {row})] == ({cr.start[lib][row]}, {n}) and ({lib}, {row}) not in c['hit_ords'] and S({lib}, {row}) >= 2")
    return cr


def check(cr, r, c):
    """the read's predicate over the reference's counts"""
    return eval(r.expect, dict(c=c, nact=nact_of(c, cr.lay), p=r.probes, S=lambda lib, row: cr.start[lib].get(row), len=len, sorted=sorted, sum=sum, max=max, all=all))
