"""A read designer for the accumulate kernel's epilogues, with a plain reference.

A read is designed as a PLAN: table entries (k-mer position, strand, hd, colour) written into a hand-made index, so that the read has a
chosen number of events, marked keys, live events and positions hit twice -- on the boundaries of the kernel's routes
(docs/design/04_accumulate.md: the boundary table).  The expected records come from `reference`, which knows nothing of routes: every
k-mer of the read on both strands, every entry of its row, hd32, one event per leaf of the colour, per (leaf, strand) and position the
smallest hd, the histograms, hdist_filt and the limit 2 * hdist_filt + 1 as oracle/ computes them.  From the same events it counts what
the routes depend on; `predict_paths` turns the counts and the layout the library reports (capi.acc_layout) into the path witnesses a
read must leave (capi.Stream.acc_paths)."""
import numpy as np

from helpers import closed_form, hd32, revcomp, row_of, write_index

K, H, M, R, FRAC = 25, 9, 4, 1, True  # 16 non-LSH positions; residues 0 and 1 of 4 are served: half of the k-mers have a row
PPOS = [24, 23, 21, 17, 13, 10, 6, 4, 2]
NPOS = [p for p in range(K) if p not in PPOS]
NLEAF = 256
NPOSITIONS = 128  # k-mer positions of a designed read: one segment
TH = 4


class Tree:
    """Balanced binary tree of NLEAF leaves L0.., numbered in post-order like the index does (leaf i has rank i)."""

    def __init__(self, nleaf=NLEAF):
        self.nleaf = nleaf
        self.se_of_clade = {}  # (first leaf, size) -> se
        self.kind = [0]        # by se: 1 leaf, 2 internal
        self.children = [(0, 0)]
        self.names = [""]
        self.nwk = self._build(0, nleaf) + ";"
        self.nnodes = len(self.kind) - 1
        self.leaf_se = [self.se_of_clade[(i, 1)] for i in range(nleaf)]

    def _build(self, a, n):
        if n == 1:
            txt, ch, name = f"L{a}:0.01", (0, len(self.kind)), f"L{a}"
        else:
            left, right = self._build(a, n // 2), self._build(a + n // 2, n // 2)
            ch, name = (self.se_of_clade[(a, n // 2)], self.se_of_clade[(a + n // 2, n // 2)]), f"C{a}_{n}"
            txt = f"({left},{right}){name}:0.01"
        self.se_of_clade[(a, n)] = len(self.kind)
        self.kind.append(1 if n == 1 else 2)
        self.children.append(ch)
        self.names.append(name)
        return txt


class Craft:
    """The index under construction: the tree, the colour table (clades, then pair colours for arbitrary leaf ranges) and the rows."""

    def __init__(self):
        self.tree = Tree()
        self.pse = list(self.tree.children)
        self.rows = {}
        self._range = {}
        self.reads = []  # Read objects

    def clades(self, a, b):
        """aligned clades that tile the leaf range [a, b)"""
        out = []
        while a < b:
            n = 1
            while a % (2 * n) == 0 and a + 2 * n <= b:
                n *= 2
            out.append(self.tree.se_of_clade[(a, n)])
            a += n
        return out

    def colour(self, a, b):
        """a colour whose leaves are exactly the ranks [a, b): a leaf, a clade, or a chain of pair colours over disjoint clades"""
        if (a, b) not in self._range:
            parts = self.clades(a, b)
            c = parts[0]
            for p in parts[1:]:
                self.pse.append((c, p))
                c = len(self.pse) - 1
            self._range[(a, b)] = c
        return self._range[(a, b)]

    def write(self, path):
        t = self.tree
        rho = [0.0] + [0.25 if t.kind[se] == 1 else 0.0 for se in range(1, t.nnodes + 1)]
        write_index(path, K, H, M, R, FRAC, PPOS, self.rows, self.pse, rho, nwk=t.nwk)
        return path

    def batch(self, reads=None, segs=1):
        seqs = [r.form_of(segs) for r in (self.reads if reads is None else reads)]
        bases = np.frombuffer("".join(seqs).encode(), np.uint8)
        offs = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        return bases, offs


class Read:
    """One designed read: a random sequence of 128 k-mer positions whose k-mers at `need` (position, strand) have a row, and the entries
    planned for it.  form_of(2) / form_of(3): the read lengthened to two / three segments by a tail of bases (its k-mers are not planned)."""

    def __init__(self, craft, name, seed, need=((0, 0), (127, 0), (0, 1), (127, 1))):
        self.craft, self.name = craft, name
        rng = np.random.default_rng(seed)
        while True:
            self.seq = "".join("ACGT"[i] for i in rng.integers(0, 4, NPOSITIONS + K - 1))
            self.form = {}
            for i in range(NPOSITIONS):
                km = self.seq[i:i + K]
                for s, x in ((0, km), (1, revcomp(km))):
                    f = closed_form(x, PPOS, NPOS)
                    row = row_of(f[2], M, R, FRAC)
                    if row is not None:
                        self.form[(i, s)] = (row, f[3])
            if all(n in self.form for n in need):
                break
        self.tail = "".join("ACGT"[i] for i in rng.integers(0, 4, 200))
        self.taken = set(need)  # slots the filler leaves alone
        self.masks = {}
        self.nplanned = 0
        self.expect = None      # the predicate the read was designed for, as text over the reference's counts and the layout
        craft.reads.append(self)

    def form_of(self, segs):
        return self.seq + self.tail[:{1: 0, 2: 60, 3: 200}[segs]]

    def free_slots(self, strand):
        return [p for (p, s) in sorted(self.form) if s == strand and (p, s) not in self.taken]

    def add(self, pos, strand, hd, a, b, flip=0):
        """an entry in the row of the k-mer at (pos, strand): the k-mer's code with `hd` positions changed, colour = leaves [a, b).
        flip = 0 / 1: the highest changed bit of the code was 0 / 1, so the entry sorts behind / in front of the exact code."""
        row, enc = self.form[(pos, strand)]
        hi = [j for j in range(15, -1, -1) if ((enc >> (16 + j)) & 1) == flip]
        used = self.masks.setdefault((pos, strand), set())
        for start in range(len(hi) if hd else 1):
            js = hi[start:start + 1] if hd else []
            js += [j for j in range(16) if j not in js][: max(0, hd - len(js))]
            mask = 0
            for n, j in enumerate(js):
                mask |= 1 << (16 + j) if n == 0 else 1 << j  # the first in the high half: it decides the order
            if mask not in used and len(js) == hd:
                break
        else:
            raise AssertionError(f"{self.name}: no unused code left at {(pos, strand)} for hd {hd}")
        used.add(mask)
        assert hd32(enc ^ mask, enc) == hd
        self.craft.rows.setdefault(row, []).append((enc ^ mask, self.craft.colour(a, b)))
        self.taken.add((pos, strand))
        self.nplanned += b - a
        return self

    def group(self, pos, strand, leaf, hds, flips=None, wide=False):
        """one position of key (leaf, strand) hit len(hds) times.  wide: the first hit is a colour of many leaves, which puts the
        group's events far apart in the event list (different 64-event tiles)."""
        for n, hd in enumerate(hds):
            lo, hi = (max(0, leaf - 70), min(NLEAF, leaf + 70)) if (wide and n == 0) else (leaf, leaf + 1)
            self.add(pos, strand, hd, lo, hi, flip=(flips[n] if flips else n & 1))
        return self

    def fill(self, strand, hd, a, b, total):
        """entries of colour [a, b) at free positions of the strand until the read has `total` planned events: whole rounds of
        b - a events, the last one over [a, a + rest)"""
        slots = self.free_slots(strand)
        while self.nplanned < total:
            n = min(b - a, total - self.nplanned)
            assert slots, f"{self.name}: out of k-mer positions"
            self.add(slots.pop(0), strand, hd, a, a + n)
        assert self.nplanned == total
        return self


def reference(craft, seqs, th=TH):
    """Per read: dict(onmers, hdist_filt [2], records {(leaf se << 1 | strand): hist}, and the counts the routes depend on: nev, nkeys
    (marked keys = records), live (events of marked keys), all_keys, groups [(key, position, [hd, ...])] of marked keys hit more than
    once at a position, per_key {key: events} of the marked keys)."""
    t, pse, rows = craft.tree, craft.pse, craft.rows
    out = []
    for seq in seqs:
        events, filt, onmers = [], [None, None], 0
        for i in range(len(seq) - K + 1):
            km = seq[i:i + K]
            if any(ch not in "ACGTacgt" for ch in km):
                continue
            onmers += 1
            for s, x in ((0, km), (1, revcomp(km))):
                f = closed_form(x, PPOS, NPOS)
                row = row_of(f[2], M, R, FRAC)
                if row is None:
                    continue
                for enc, se in sorted(rows.get(row, [])):
                    hd = hd32(enc, f[3])
                    if hd > th:
                        continue
                    filt[s] = hd if filt[s] is None else min(filt[s], hd)
                    queue = [se]
                    while queue:
                        c = queue.pop(0)
                        if c <= t.nnodes:
                            if t.kind[c] == 0:
                                continue
                            if t.kind[c] == 1:
                                events.append((c, s, i, hd))
                                continue
                        queue.extend(pse[c] if c < len(pse) else (0, 0))
        best = {}
        for se, s, i, hd in events:
            d = best.setdefault((se << 1) | s, {})
            d[i] = min(hd, d.get(i, 99))
        lim = [0xFFFFFFFF if f is None else 2 * f + 1 for f in filt]
        records = {}
        for key, d in best.items():
            hist = [0] * (th + 1)
            for hd in d.values():
                hist[hd] += 1
            if min(d.values()) <= lim[key & 1]:
                records[key] = tuple(hist)
        per_key, at = {}, {}
        for se, s, i, hd in events:
            key = (se << 1) | s
            if key in records:
                per_key[key] = per_key.get(key, 0) + 1
                at.setdefault((key, i), []).append(hd)
        out.append(dict(onmers=onmers, hdist_filt=[0xFFFFFFFF if f is None else f for f in filt], records=records, nev=len(events),
                        nkeys=len(records), all_keys=len(best), live=sum(per_key.values()), per_key=per_key,
                        groups=[(k_, i, h) for (k_, i), h in sorted(at.items()) if len(h) > 1]))
    return out


def batch_keys(lay, n):
    """keys of one batch of the straight-line epilogue behind n events (finalize_events_fast)"""
    n = (n + 3) & ~3
    return ((lay["ev_words"] - n) // lay["key_words"]) & ~3 if n < lay["ev_words"] else 0


def predict_paths(c, lay):
    """The path witnesses of one single-segment read at th = 4 from the reference's counts c and the layout: the route through
    finalize_events_fast, and whether the read goes on to finalize_events.  (fix_dup_moved is not predicted.)"""
    p = dict(fast_entered=1, fast_false_early=0, fast_compact=0, fast_false_compacted=0, fast_big_read=0, fast_one_batch=0, fast_multi_batch=0,
             fast_extra_batches=0, fix_dup_calls=0, gen_entered_1=0, route="")
    E = lay["ev_cap"]
    nev, nkeys = c["nev"], c["nkeys"]
    if nev == 0:
        p.update(fast_false_early=1, route="none")
        return p
    if nev > E or batch_keys(lay, nev) < nkeys:
        p["fast_compact"] = 1
        nev = c["live"]
        if nev > E or batch_keys(lay, nev) < min(nkeys, 64):
            if nev <= E or E % 128:
                p.update(fast_false_compacted=1, gen_entered_1=1 if nev else 0, route="general")
            else:
                p.update(fast_big_read=1, route="big")
            return p
    kb = min(batch_keys(lay, nev), (nkeys + 3) & ~3)
    nb = -(-nkeys // kb) if nkeys else 0
    p["fast_one_batch" if nb <= 1 else "fast_multi_batch"] = 1
    p["fast_extra_batches"] = max(0, nb - 1)
    p["fix_dup_calls"] = sum(len(h) - 1 for _, _, h in c["groups"])
    p["route"] = "one" if nb <= 1 else "several"
    return p


def designs(lay):
    """The designed reads (<= 40) for the layout the library reports: (Craft, {name: Read}).  Every read carries `expect`, the predicate
    it was designed for, over the reference's counts c, the layout (E = ev_cap, W = ev_words, B = batch_keys) and its predicted route."""
    E = lay["ev_cap"]
    B = lambda n: batch_keys(lay, n)
    cr = Craft()
    seed = [100]

    def read(name, expect):
        seed[0] += 1
        r = Read(cr, name, seed[0])
        r.expect = expect
        return r

    # ---- the capacity edge.  All live: 60 keys of strand 0, hd 1 (no exact hit: limit 3, every key marked)
    for d in (-1, 0, 1, 63, 64, 65, 255, 256, 257):
        want = "c['nev'] == c['live'] == E + %d and c['nkeys'] == 60 and route == '%s'" % (d, "general" if d <= 0 else "big")
        read(f"edge_live_{d:+d}", want).fill(0, 1, 0, 60, E + d)
    # mostly droppable: one exact hit (limit 1) and 300 events of hd 1 on 40 keys; the rest hd 3 on other leaves
    for d in (-1, 0, 1, 63, 64, 65, 255, 256, 257):
        r = read(f"edge_drop_{d:+d}", "c['nev'] == E + %d and c['live'] == 300 and c['nkeys'] == 40 and p['fast_compact'] == 1 and route == 'one'" % d)
        r.add(0, 0, 0, 0, 1).fill(0, 1, 0, 40, 300).fill(0, 3, 100, 228, E + d)
    # ---- compaction that does not suffice: 64 keys behind 768 / 772 live events; the LDS full of live events
    for live, route in ((768, "one"), (772, "general"), (E, "general")):
        r = read(f"compact_{live}", "c['live'] == %d and c['nkeys'] == 64 and c['nev'] == %d and p['fast_compact'] == 1 and route == '%s' "
                 "and B(768) == 64 and B(772) < 64" % (live, live + 200, route))
        r.add(0, 0, 0, 0, 1).fill(0, 1, 0, 64, live).fill(0, 3, 100, 200, live + 200)
    # ---- key batches: B(nev) keys, one more, and three batches whose last is no multiple of 4; the keys at ordinals B - 1 and B are
    #      hit twice at a position
    nev = 600
    b = B(nev)
    for nk, nb in ((b, 1), (b + 1, 2), (2 * b + 3, 3)):
        r = read(f"batches_{nb}", "c['nev'] == c['live'] == %d and c['nkeys'] == %d and B(%d) == %d and p['fast_extra_batches'] == %d "
                 "and p['fix_dup_calls'] == %d and %d %% 4 != 0" % (nev, nk, nev, b, nb - 1, 2 if nk > b else 1, nk - 2 * b if nb == 3 else 1))
        r.group(0, 0, b - 1, (1, 2), flips=(0, 1))
        if nk > b:
            r.group(127, 0, b, (2, 1), flips=(0, 1))
        r.fill(0, 1, 0, nk, nev)
    # ---- positions hit twice and three times: the hd patterns in both bucket orders, at positions 0 and 127, on both strands, the
    #      group's events side by side and tiles apart.  One exact hit per strand: limit 1.
    r = read("dups_limit1", "len(c['groups']) == 10 and sum(len(h) - 1 for _, _, h in c['groups']) == 15 and c['nkeys'] > 2 * B(c['live']) "
             "and route == 'several' and p['fix_dup_calls'] == 15")
    free = {s: r.free_slots(s) for s in (0, 1)}
    r.group(0, 0, 3, (0, 1), flips=(0, 0)).group(127, 0, 5, (1, 0), flips=(1, 0))
    r.group(0, 1, 7, (0, 1), flips=(0, 1)).group(127, 1, 9, (1, 0), flips=(0, 0))
    r.group(free[0][0], 0, 100, (3, 1, 0), flips=(0, 1, 0), wide=True).group(free[0][1], 0, 11, (0, 3, 1), flips=(0, 0, 1))
    r.group(free[1][0], 1, 100, (0, 3, 1), flips=(0, 1, 0), wide=True).group(free[1][1], 1, 13, (4, 4, 0), flips=(0, 1, 0))
    r.group(free[0][2], 0, 200, (1, 0), flips=(1, 0), wide=True).group(free[0][3], 0, 15, (4, 4, 0), flips=(1, 0, 0))
    r.fill(0, 1, 20, 60, r.nplanned + 200)
    # no hit below hd 2: limit 5, every key marked
    r = read("dups_limit5", "c['hdist_filt'] == [2, 2] and len(c['groups']) == 4 and route == 'one' and p['fix_dup_calls'] == 5")
    free = {s: r.free_slots(s) for s in (0, 1)}
    r.group(0, 0, 3, (2, 2), flips=(0, 1)).group(127, 1, 5, (2, 2), flips=(1, 0))
    r.group(free[0][0], 0, 100, (4, 4, 2), flips=(0, 1, 0)).group(free[1][0], 1, 7, (4, 3), flips=(1, 0))
    r.fill(0, 3, 20, 60, r.nplanned + 150)
    # ---- finish_big_read: live events beyond the LDS, nev no multiple of 128, the tile that straddles E included; positions hit twice
    #      in both orders, hd 4, positions 0 and 127
    for nk, nev in ((63, E + 76), (64, E + 126), (65, E + 226), (131, E + 300)):
        r = read(f"big_{nk}", "c['live'] == c['nev'] == %d and c['nev'] %% 128 != 0 and c['nkeys'] == %d and route == 'big' "
                 "and len(c['groups']) == 4" % (nev, nk))
        r.group(0, 0, 1, (0, 4), flips=(0, 0)).group(127, 0, nk - 1, (4, 1), flips=(1, 0))
        fs = r.free_slots(0)
        r.group(fs[0], 0, 30, (3, 1, 2), flips=(0, 1, 0), wide=False).group(fs[-1], 0, 40, (1, 0), flips=(1, 0))
        r.fill(0, 1, 0, nk, nev)
    # 500 keys on both strands (th = 6: more keys than the general epilogue's key table has room for behind the events)
    read("big_500", "c['nkeys'] == 500 and c['live'] == E + 200 and route == 'big'").fill(0, 1, 0, 250, 600).fill(1, 1, 0, 250, E + 200)
    # 200 keys, all but one with a single event (th = 3: the general epilogue's sparse form)
    read("sparse_200", "c['nkeys'] == 200 and c['nev'] == 203 and sum(n > 1 for n in c['per_key'].values()) == 1 and route == 'several'"
         ).group(0, 0, 5, (1, 2, 3), flips=(0, 1, 0)).fill(0, 1, 0, 200, 203)
    # ---- a light read: three keys, one event each
    read("light", "c['nev'] == 3 and route == 'one'").add(0, 0, 0, 8, 9).add(127, 0, 1, 9, 10).add(0, 1, 0, 10, 11)
    assert len(cr.reads) <= 40
    return cr, {r.name: r for r in cr.reads}
