"""A tree and read designer for the per-read kernel of `place` (place_read, krepp_amd/csrc/kr_dev_place.inc), with a plain reference.

place_read chooses its route from the data (docs/design/06_place.md: the route table): weights through the wave's global scratch or
walked, histograms packed in LDS or re-read, ancestor lanes on their own run of the leaf list or on all of it, runs in blocks, the
arrays in LDS or in global scratch, the two early exits.  The natural inputs of the suite (a 25-leaf tree, 150-base reads) take one
route.  Here trees and reads are made so that every quantity a route depends on sits on its boundary, with a read on either side:

  trees  `lad2`    a binary ladder: leaf i hangs i + 1 levels below the root, so tot_chain of a read is a sum of chosen depths, and
                   every weight is a power of two (the gate sums are exact)
         `lad357`  the same ladder with rungs of 3, 5 and 7 children: weights 1/3, 1/15, 1/105, ... are inexact in doubles, so the
                   order of the divisions shows in the bits; `user`: the same tree given as -t with two leaves under names the index
                   does not have, so that their parents have eff_nchildren < nchildren and are no candidates
         `bal`     a balanced binary tree of 8,192 leaves: reads of 256 | 257 and 4,096 | 4,097 leaves through colours that cover a
                   leaf range, and of 1,024 | 1,025 distinct ancestors
  reads  a plan of table entries (k-mer position, strand, hd, colour) written into a hand-made index (helpers.write_index), as
         tests/acc_craft.py does for the accumulate kernel.

The boundaries come from the library (capi.place_layout), not from this file.  `reference` restates IBatch::report_placement up to the
candidate list in exact rationals from the records of a batch and the tree alone; it knows nothing of routes.  `predict_paths` turns
the same quantities and the layout into the path witnesses a read must leave (capi.place_paths)."""
from fractions import Fraction

import numpy as np

from acc_craft import FRAC, H, K, M, PPOS, R
from helpers import closed_form, revcomp, row_of, write_index

NPOS = [p for p in range(K) if p not in PPOS]
RHO_FILE = 0.25  # every leaf's rho in the file (the loader scales it: Index::make_rho_partial)


class PTree:
    """A tree from a nested list of leaf names, numbered in post-order from 1 like the index and the placement tree number theirs."""

    def __init__(self, shape):
        self.parent, self.kids, self.names, self.kind, self.leaf_se = [0], [[]], [""], [0], []
        self.nwk = self._build(shape) + ";"
        self.nnodes = len(self.kind) - 1
        self.root = self.nnodes
        self.depth = [0] * (self.nnodes + 1)  # number of ancestors
        for se in range(self.nnodes - 1, 0, -1):
            self.depth[se] = self.depth[self.parent[se]] + 1
        self.lo = list(range(self.nnodes + 1))  # the smallest number of the subtree: it is the range [lo, se]
        for se in range(1, self.nnodes):
            self.lo[self.parent[se]] = min(self.lo[self.parent[se]], self.lo[se])
        self.rank = {se: i for i, se in enumerate(self.leaf_se)}
        self.by_name = {self.names[se]: se for se in self.leaf_se}
        self.eff = [len(k) for k in self.kids]
        self.elig = [len(k) != 1 for k in self.kids]

    def _build(self, sh):
        if isinstance(sh, str):
            txt, kids, name, kind = f"{sh}:0.01", [], sh, 1
        else:
            parts, kids = [], []
            for c in sh:
                parts.append(self._build(c))
                kids.append(self._last)
            name, kind = f"N{len(self.kind)}", 2
            txt = "(" + ",".join(parts) + f"){name}:0.01"
        se = len(self.kind)
        self.kind.append(kind), self.kids.append(kids), self.names.append(name), self.parent.append(0)
        for c in kids:
            self.parent[c] = se
        if kind == 1:
            self.leaf_se.append(se)
        self._last = se
        return txt

    def ancestors(self, se):
        out = []
        while self.parent[se]:
            se = self.parent[se]
            out.append(se)
        return out

    def map_index(self, index_tree):
        """this tree as the user tree (-t) of an index built on index_tree: index leaf se -> node here by name (0: none), and eff /
        elig as Tree::map_to_qtree and compute_eff_nchildren leave them: a child counts if a mapped leaf lies below it"""
        idx_to_pt = [0] * (index_tree.nnodes + 1)
        covered = [False] * (self.nnodes + 1)
        for se in index_tree.leaf_se:
            q = self.by_name.get(index_tree.names[se], 0)
            idx_to_pt[se] = q
            while q and not covered[q]:
                covered[q] = True
                q = self.parent[q]
        self.eff = [sum(1 for c in k if covered[c]) for k in self.kids]
        self.elig = [len(k) == e and len(k) != 1 for k, e in zip(self.kids, self.eff)]
        return idx_to_pt


def ladder_shape(nleaf, arity=(2,), rename=None):
    """rung j (from the root) has arity[j % len] children: leaves, and as its last child the next rung; the last rung is all leaves"""
    rungs, i, j = [], 0, 0
    while i < nleaf:
        a = arity[j % len(arity)]
        take = a - 1 if nleaf - i > a else nleaf - i
        rungs.append([(rename or {}).get(f"L{x}", f"L{x}") for x in range(i, i + take)])
        i, j = i + take, j + 1
    sh = rungs[-1]
    for r in reversed(rungs[:-1]):
        sh = r + [sh]
    return sh


def balanced_shape(a, n):
    return f"L{a}" if n == 1 else [balanced_shape(a, n // 2), balanced_shape(a + n // 2, n // 2)]


class Craft:
    """The index under construction: the tree, the colour table (a tree node's colour is its subtree; further colours are chains of
    pairs over nodes) and the rows."""

    def __init__(self, name, tree):
        self.name, self.tree = name, tree
        t = tree
        self.pse = [(0, 0)] * (t.nnodes + 1)
        self._chain = {}
        for se in range(1, t.nnodes + 1):
            k = t.kids[se]
            self.pse[se] = (0, se) if not k else ((k[0], k[1]) if len(k) == 2 else (k[0], self.colour_of_nodes(k[1:])))
        self.rows = {}
        self.reads = []

    def colour_of_nodes(self, nodes):
        """a colour whose leaves are the leaves below `nodes` (disjoint subtrees)"""
        nodes = tuple(nodes)
        if len(nodes) == 1:
            return nodes[0]
        if nodes not in self._chain:
            c = self.colour_of_nodes(nodes[:-1]) if len(nodes) > 2 else nodes[0]
            self.pse.append((c, nodes[-1]))
            self._chain[nodes] = len(self.pse) - 1
        return self._chain[nodes]

    def cover(self, a, b):
        """the largest subtrees that tile the leaf ranks [a, b)"""
        t = self.tree
        if not hasattr(self, "_nleaves"):
            self._nleaves = [0] * (t.nnodes + 1)
            for se in range(1, t.nnodes + 1):  # children precede parents
                self._nleaves[se] += t.kind[se] == 1
                self._nleaves[t.parent[se]] += self._nleaves[se]
        out, i = [], a
        while i < b:
            se = t.leaf_se[i]
            while t.parent[se] and t.lo[t.parent[se]] == t.lo[se] and i + self._nleaves[t.parent[se]] <= b:
                se = t.parent[se]  # the parent's subtree starts at leaf i too and ends before b
            out.append(se)
            i += self._nleaves[se]
        return out

    def colour(self, ranks):
        """a colour for the leaf ranks given: a range (a, b) as ("range", a, b), or a tuple of ranks"""
        if ranks and ranks[0] == "range":
            return self.colour_of_nodes(self.cover(ranks[1], ranks[2]))
        return self.colour_of_nodes([self.tree.leaf_se[i] for i in ranks])

    def write(self, path):
        t = self.tree
        rho = [0.0] + [RHO_FILE if t.kind[se] == 1 else 0.0 for se in range(1, t.nnodes + 1)]
        write_index(path, K, H, M, R, FRAC, PPOS, self.rows, self.pse, rho, nwk=t.nwk)
        return path

    def batch(self):
        seqs = [r.seq for r in self.reads]
        bases = np.frombuffer("".join(seqs).encode(), np.uint8)
        offs = np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)
        return bases, offs, [r.name for r in self.reads]


class Read:
    """One designed read: a random sequence of `npos` k-mer positions and the entries planned for it.  `expect`: the predicate the
    read was designed for, as text over the reference's quantities q, the predicted paths p and the layout L."""

    def __init__(self, craft, name, seed, expect, npos=128, gated=False):
        self.craft, self.name, self.expect, self.gated = craft, name, expect, gated  # gated: `expect` holds with the tau gate on (no_filter = 0)
        rng = np.random.default_rng(seed)
        self.seq = "".join("ACGT"[i] for i in rng.integers(0, 4, npos + K - 1))
        self.free = {0: [], 1: []}
        self.form = {}
        for i in range(npos):
            km = self.seq[i:i + K]
            for s, x in ((0, km), (1, revcomp(km))):
                f = closed_form(x, PPOS, NPOS)
                row = row_of(f[2], M, R, FRAC)
                if row is not None:
                    self.form[(i, s)] = (row, f[3])
                    self.free[s].append(i)
        craft.reads.append(self)

    def hit(self, ranks, hd=0, strand=0, times=1):
        """`times` k-mer positions of the strand hit the colour of the leaf ranks at Hamming distance hd"""
        c = self.craft.colour(tuple(ranks))
        for _ in range(times):
            assert self.free[strand], f"{self.name}: out of k-mer positions"
            row, enc = self.form[(self.free[strand].pop(0), strand)]
            self.craft.rows.setdefault(row, []).append((enc ^ ((1 << hd) - 1), c))
        return self


# ---------------------------------------------------------------------------
# The reference: report_placement up to the candidate list, in exact rationals
# ---------------------------------------------------------------------------
def records_of_oracle(accs, nreads):
    """per read the records of pyoracle.Index.dist(collect=1) as `reference` takes them: the records that passed hdist_filt, in
    (strand, se) order per strand -- key order --, with the choice summarize_matches makes per leaf (src/query.cpp:96-139: the reverse
    strand's record unless the forward one has the smaller d, or the same d and more matches; the closest stands for its leaf)"""
    per = [[] for _ in range(nreads)]
    for a in accs:
        if a["passed"]:
            per[int(a["read"])].append(dict(key=(int(a["se"]) << 1) | int(a["strand"]), hist=tuple(int(x) for x in a["hist"]), d=float(a["d_llh"]),
                                            v=float(a["v_llh"]), matches=int(a["match_count"])))
    for recs in per:
        recs.sort(key=lambda x: x["key"])
        by = {x["key"]: x for x in recs}
        best = None
        for x in sorted(recs, key=lambda x: (x["key"] & 1, x["key"])):
            if best is None or x["d"] <= best["d"]:
                best = x
        for x in recs:
            o = by.get(x["key"] ^ 1)
            if o is None:
                x["sel"] = True
            elif x["key"] & 1:
                x["sel"] = not (x["d"] > o["d"] or (x["d"] == o["d"] and x["matches"] < o["matches"]))
            else:
                x["sel"] = o["d"] > x["d"] or (o["d"] == x["d"] and o["matches"] < x["matches"])
        if best is not None:
            for x in recs:
                if x["key"] >> 1 == best["key"] >> 1:
                    x["sel"] = x is best
    return per


def records_of_result(res, th):
    """the same from a tapped batch (capi.Result: rec_key, rec_hist, rec_d, rec_v, rec_sel)"""
    per = []
    for r in range(res.nreads):
        o, n = int(res.read_off[r]), int(res.read_cnt[r])
        per.append([dict(key=int(res.rec_key[i]), hist=tuple(int(x) for x in res.rec_hist[i][:th + 1]), d=float(res.rec_d[i]), v=float(res.rec_v[i]),
                         sel=bool(res.rec_sel[i])) for i in range(o, o + n)])
    return per


def reference(tree, idx_to_pt, records, read_len, th, tau, no_filter):
    """One read.  tree: the placement tree (PTree with eff / elig); idx_to_pt: index leaf -> its node (0: none).  Returns None for a
    read without records, else dict(closest key, closest_leq, stopped, single, leaves {node: record} (the record that stands: the last
    in record order), dropped (records that lost their node to a later one), order (the nodes of the chosen records in (node, record)
    order, dropped ones included), ancestors (distinct, sorted), weight {(leaf, ancestor)}, acc {ancestor: (hist [Fraction], uc, rho)},
    gate {node: leq sum}, candidates (set of nodes))."""
    valid = [x for x in records if x["d"] <= 1.7976931348623157e308]
    if not valid:
        return None
    best = None
    for i, x in enumerate(records):
        if x["d"] <= 1.7976931348623157e308 and (best is None or x["d"] < best[0] or (x["d"] == best[0] and (x["key"] & 1, i) > best[1])):
            best = (x["d"], (x["key"] & 1, i), x)
    closest = best[2]
    leq = lambda h: sum(h[: tau + 1])
    q = dict(closest=closest["key"], closest_leq=leq(closest["hist"]), single=False, leaves={}, dropped=0, order=[], ancestors=[], weight={}, acc={}, gate={},
             candidates=set(), nrecords=len(records))
    q["stopped"] = not (no_filter or q["closest_leq"] > 1)
    if q["stopped"]:
        return q
    chosen = [(idx_to_pt[x["key"] >> 1], i, x) for i, x in enumerate(records) if x["sel"] and idx_to_pt[x["key"] >> 1]]
    chosen.sort(key=lambda c: (c[0], c[1]))
    q["order"] = [c[0] for c in chosen]
    for node, _, x in chosen:
        q["dropped"] += node in q["leaves"]
        q["leaves"][node] = x
    if not chosen:
        return q
    if len(chosen) == 1:
        q["single"] = True
        q["candidates"] = {idx_to_pt[closest["key"] >> 1]}
        return q
    enmers = read_len - K + 1 if read_len >= K else 0
    acc = {}
    for node in sorted(q["leaves"]):
        x = q["leaves"][node]
        w = Fraction(1)
        for a in tree.ancestors(node):
            w /= tree.eff[a]
            q["weight"][(node, a)] = w
            h, m = acc.setdefault(a, ([Fraction(0)] * (th + 1), [Fraction(0)]))
            for b in range(th + 1):
                if x["hist"][b]:
                    h[b] += x["hist"][b] * w
            m[0] += sum(x["hist"]) * w
    q["ancestors"] = sorted(acc)
    for a, (h, m) in acc.items():
        q["acc"][a] = (h, enmers - m[0], RHO_LOADED)
        q["gate"][a] = sum(h[: tau + 1])
    for node, x in q["leaves"].items():
        q["gate"][node] = Fraction(leq(x["hist"]))
    q["candidates"] = {n for n, g in q["gate"].items() if tree.elig[n] and (no_filter or g > 1)}
    return q


RHO_LOADED = RHO_FILE * (R + 1) / M  # what the loader hands out for a leaf (exact: a power of two)


def predict_paths(q, tree, lay, th, lds=None, big_first=True):
    """The path witnesses of one read (capi.PLACE_WITNESSES) from the reference's quantities and the layout.  lds: (leaves, nodes) of
    KR_DEBUG_PLACE_LDS; big_first: KR_PLACE_BIG_FIRST.  For batches of at most 1,024 reads on a new stream: there every wave of the
    first launch owns a piece of the global scratch (a read beyond the LDS arrays is done inline), and a wave of the second launch has
    kPlChain weights -- the host gives it kPlChain * max(1, chain_waves / heavy_waves), which is kPlChain while the second launch has
    1,024 waves: trees whose whole-tree arrays (32 bytes a leaf + 4 a node) stay below 1 MB a wave, as every tree here does."""
    p = dict.fromkeys(("chained", "walked_shallow", "walked_deep", "wide", "runs_off", "dup_dropped", "single", "tau_stopped", "home_lds", "home_inline",
                       "home_second", "multi_block_lanes"), 0)
    p["home"] = None
    if q is None:
        return p
    if q["stopped"]:
        p["tau_stopped"] = 1
        return p
    if q["single"]:
        p["single"] = 1
        return p
    order = q["order"]
    nl, na = len(order), len(q["ancestors"])
    if nl == 0:
        return p
    ll, ln = lds or (lay["leaves"], lay["nodes"])
    ll, ln = min(ll, lay["leaves"]), min(ln, lay["nodes"])
    home = "lds" if nl <= ll and na <= ln else ("inline" if big_first else "second")
    p["home"] = home
    p["home_" + home] = 1
    cap = lay["chain"] * (lay["inline_chain"] if home == "inline" else 1)
    stand = [n if (i + 1 == nl or order[i + 1] != n) else 0 for i, n in enumerate(order)]  # a node's earlier records: 0
    tot = sum(tree.depth[n] for n in stand if n)
    p["tot_chain"], p["nl"], p["na"] = tot, nl, na
    if lay["chain_factor"] * nl < tot <= cap:
        p["chained"] = 1
    elif tot > cap:
        p["walked_deep"] = 1
    else:
        p["walked_shallow"] = 1
    p["wide"] = int(th >= 8 or any(c > 255 for x in q["chosen_hists"] for c in x))
    runs = nl <= lay["runs_leaves"]
    p["runs_off"] = int(not runs)
    p["dup_dropped"] = int(q["dropped"] > 0)
    B = lay["block"]
    st = np.array(stand, np.int64)
    for a in q["ancestors"]:  # the lane walks blocks of B entries from its first leaf until a block holds an entry beyond a, or the list ends
        e0 = int(np.argmax((st >= tree.lo[a]) & (st <= a))) if runs else 0
        beyond = np.nonzero(st[e0:] > a)[0]
        nb = int(beyond[0]) // B + 1 if len(beyond) else -(-(nl - e0) // B)
        p["multi_block_lanes"] += nb > 1
    return p


def evaluate(craft, tree, idx_to_pt, per_read_records, th, tau, no_filter, lay, lds=None, big_first=True):
    """reference and predicted paths of every read of the craft's batch"""
    out = []
    for rd, recs in zip(craft.reads, per_read_records):
        q = reference(tree, idx_to_pt, recs, len(rd.seq), th, tau, no_filter)
        if q is not None:
            q["chosen_hists"] = [x["hist"] for x in recs if x["sel"] and idx_to_pt[x["key"] >> 1]]
        out.append((q, predict_paths(q, tree, lay, th, lds, big_first)))
    return out


# ---------------------------------------------------------------------------
# The designs
# ---------------------------------------------------------------------------
def ranks_with_depth_sum(tree, nl, target, lo_rank=0):
    """nl leaf ranks (ascending) whose depths sum to `target`: the nl shallowest from lo_rank on, then the deepest of them moved down"""
    ranks = list(range(lo_rank, lo_rank + nl))
    dep = lambda i: tree.depth[tree.leaf_se[i]]
    nleaf = len(tree.leaf_se)
    j, limit = nl - 1, nleaf - 1
    while sum(dep(i) for i in ranks) < target:
        assert j >= 0, "the tree is too shallow for this sum"
        if ranks[j] < limit and dep(ranks[j] + 1) - dep(ranks[j]) <= target - sum(dep(i) for i in ranks):
            ranks[j] += 1
        else:
            limit, j = ranks[j] - 1, j - 1
    assert sum(dep(i) for i in ranks) == target and len(set(ranks)) == nl, (nl, target)
    return ranks


def ranks_with_ancestors(tree, target, step):
    """leaf ranks whose distinct ancestors number exactly `target`: every step-th leaf while the count stays below, then leaves that
    add what is missing"""
    seen, ranks = set(), []

    def gain(i):
        return [a for a in tree.ancestors(tree.leaf_se[i]) if a not in seen]

    for i in range(0, len(tree.leaf_se), step):
        g = gain(i)
        if len(seen) + len(g) <= target:
            seen.update(g), ranks.append(i)
    for i in range(len(tree.leaf_se)):
        if len(seen) == target:
            break
        g = gain(i)
        if i not in ranks and 0 < len(g) <= target - len(seen):
            seen.update(g), ranks.append(i)
    assert len(seen) == target, (len(seen), target)
    return sorted(ranks)


def _reader(cr, seed0):
    seed = [seed0]

    def read(name, expect, npos=128, gated=False):
        seed[0] += 1
        return Read(cr, name, seed[0], expect, npos, gated)

    return read


def _fillers(cr, read, n, nleaf):
    """ordinary reads: a handful of leaves each, a few hits at mixed distances"""
    rng = np.random.default_rng(len(cr.reads))
    for j in range(n):
        r = read(f"fill{j}", "True")
        base = int(rng.integers(0, nleaf - 12))
        for _ in range(int(rng.integers(1, 5))):
            ranks = sorted(set(int(x) for x in base + rng.integers(0, 12, int(rng.integers(1, 6)))))
            r.hit(ranks, hd=int(rng.integers(0, 3)), strand=int(rng.integers(0, 2)), times=int(rng.integers(1, 4)))


def design_ladder(lay, arity=(2,), nleaf=200, name="lad2", rename=None):
    """The ladder's designs (on the binary ladder and on the one with rungs of 3, 5, 7 children): the read sizes up to 65, the chained
    thresholds, the block seams of the runs, the equal-d ties, the gates, and on the binary ladder the wide counts."""
    t = PTree(ladder_shape(nleaf, arity))
    cr = Craft(name, t)
    read = _reader(cr, 1000 + 17 * len(arity))
    F, CAP, B = lay["chain_factor"], lay["chain"], lay["block"]
    T = 3 if arity == (2,) else 4  # exact hits per leaf: no sum of T / (a product of rung sizes) may come to lie on the gate
    deepest = max(t.depth[s] for s in t.leaf_se)
    # ---- read sizes: one leaf (the single placement), two, and around the wave
    read("nl1", "q['single'] and p['single'] == 1").hit([5], 0, 0, 3)
    for nl in (2, 63, 64, 65):
        read(f"nl{nl}", f"p['nl'] == {nl} and p['home'] == 'lds'").hit(list(range(3, 3 + nl)), 0, 0, T).hit([3], 1, 0, 1)
    # ---- the chained threshold: tot_chain = F nl, F nl + 1 (ten leaves) ...
    for d, side in ((0, "walked_shallow"), (1, "chained")):
        ranks = ranks_with_depth_sum(t, 10, F * 10 + d)
        read(f"chain_F{d:+d}", f"p['tot_chain'] == L['chain_factor'] * p['nl'] + {d} and p['nl'] == 10 and p['{side}'] == 1").hit(ranks, 0, 0, T).hit(ranks[:1], 1, 0, 1)
    # ---- ... and the wave's scratch: tot_chain = kPlChain, kPlChain + 1 (the deep tree walked)
    nl_cap = 2 * CAP // deepest + 2
    if nl_cap * (deepest - nl_cap) > CAP + 1 and nl_cap <= lay["leaves"]:
        for d, side in ((0, "chained"), (1, "walked_deep")):
            ranks = ranks_with_depth_sum(t, nl_cap, CAP + d, lo_rank=nleaf // 4)
            read(f"chain_cap{d:+d}", f"p['tot_chain'] == L['chain'] + {d} and p['home'] == 'lds' and p['{side}'] == 1").hit(ranks, 0, 0, T).hit(ranks[-1:], 1, 0, 1)
    # ---- a read deep in the tree: 40 leaves, every weight a product of dozens of divisions
    read("deep40", "p['nl'] == 40 and p['chained'] == 1").hit(list(range(nleaf - 45, nleaf - 5)), 0, 0, T).hit([nleaf - 20], 1, 0, 2)
    # ---- runs below one ancestor: on a ladder the ancestor above the j-th of a read's leaves has all the later ones in its run, so a
    #      read of 2 B + 1 leaves at the top of rungs has runs of every length up to 2 B + 1: B - 1 | B | B + 1 and 2 B | 2 B + 1 among them
    step = 1 if arity == (2,) else max(arity)
    ranks = [j * step for j in range(2 * B + 1)]
    read("runs", f"p['nl'] == {2 * B + 1} and p['multi_block_lanes'] > 0 and p['na'] >= {2 * B + 1}").hit(ranks, 0, 0, T).hit(ranks[4:5], 1, 0, 1)
    read("runs_one_block", f"p['nl'] == {B} and p['multi_block_lanes'] == 0").hit(ranks[:B], 0, 0, T).hit(ranks[1:2], 1, 0, 1)
    # ---- distinct ancestors 64 | 65: the deepest leaf of the read hangs that deep
    for na in (64, 65):
        if na <= deepest:
            deep = next(i for i in range(nleaf) if t.depth[t.leaf_se[i]] == na)
            read(f"na{na}", f"p['na'] == {na}").hit([1, 2, deep], 0, 0, T).hit([deep], 1, 0, 1)
    # ---- equal d: two leaves with the same histogram, and the two strands of one leaf; the closest is the last in (strand, record) order
    read("tie_leaves", "len(set(x['d'] for x in q['leaves'].values())) == 1 and q['closest'] == max(x['key'] for x in q['leaves'].values())").hit([20, 40], 0, 0, 3)
    read("tie_strands", "q['closest'] & 1 == 1 and q['nrecords'] == 3").hit([30], 0, 0, 3).hit([30], 0, 1, 3).hit([31], 1, 0, 2)
    # ---- the tau gate (tau = 2; hits at distance 2 count, at 3 they do not; no hit below 2, so the limit 2 * 2 + 1 keeps every leaf).
    #      The closest leaf: leq 1 stops the read, leq 2 does not
    read("gate_closest_1", "q['closest_leq'] == 1 and q['stopped'] and p['tau_stopped'] == 1", gated=True).hit([50], 2, 0, 1).hit([50], 3, 0, 2).hit([51], 3, 0, 1)
    read("gate_closest_2", "q['closest_leq'] == 2 and not q['stopped'] and p['tau_stopped'] == 0", gated=True).hit([50], 2, 0, 2).hit([50], 3, 0, 1).hit([51], 3, 0, 1)
    if arity == (2,):
        # the two leaves of the last rung and the leaf of the rung above: weights 1/2 and 1/4 are exact.  a, b: the last rung's leaves
        a, b, c = nleaf - 2, nleaf - 1, nleaf - 3
        par = t.parent[t.leaf_se[a]]
        read("gate_anc_1.0", f"q['gate'][{par}] == 1 and {par} not in q['candidates'] and q['gate'][{t.parent[par]}] == 2", gated=True).hit([a, b], 2, 0, 1).hit([c], 2, 0, 3).hit([c], 3, 0, 1)
        read("gate_anc_1.5", f"q['gate'][{par}] == Fraction(3, 2) and {par} in q['candidates']", gated=True).hit([a, b], 2, 0, 1).hit([a], 2, 0, 1).hit([c], 2, 0, 3).hit([c], 3, 0, 1)
        read("gate_leaf_1_2", f"q['gate'][{t.leaf_se[a]}] == 1 and {t.leaf_se[a]} not in q['candidates'] and q['gate'][{t.leaf_se[b]}] == 2 and {t.leaf_se[b]} in q['candidates']",
             gated=True).hit([a, b], 2, 0, 1).hit([b], 2, 0, 1).hit([c], 2, 0, 3)
        # ---- the largest count 255 | 256: a long read with that many exact hits on one leaf
        for cnt, side in ((255, 0), (256, 1)):
            read(f"count{cnt}", f"max(max(x['hist']) for x in q['leaves'].values()) == {cnt} and p['wide'] == {side}", npos=1200).hit([60], 0, 0, cnt).hit([61, 62], 1, 0, 2)
    _fillers(cr, read, 24, nleaf)
    user = None
    if rename:
        user = PTree(ladder_shape(nleaf, arity, rename))
    return cr, user


def design_balanced(lay, levels=13):
    """The balanced tree's designs: reads beyond the LDS arrays by their leaves (256 | 257) and by their ancestors (1,024 | 1,025), and
    around the most leaves whose ancestor lanes walk their own run (4,096 | 4,097)"""
    nleaf = 1 << levels
    t = PTree(balanced_shape(0, nleaf))
    cr = Craft("bal", t)
    read = _reader(cr, 3000)
    LL, LN, RL = lay["leaves"], lay["nodes"], lay["runs_leaves"]
    T = 3
    assert nleaf >= RL + 104
    for nl, home in ((LL, "lds"), (LL + 1, "inline")):
        read(f"nl{nl}", f"p['nl'] == {nl} and p['home'] == '{home}' and p['na'] <= L['nodes']").hit(("range", 100, 100 + nl), 0, 0, 3).hit([100], 1, 0, 1)
    for na, home in ((LN, "lds"), (LN + 1, "inline")):
        ranks = ranks_with_ancestors(t, na, 64)
        read(f"na{na}", f"p['na'] == {na} and p['nl'] <= L['leaves'] and p['home'] == '{home}'").hit(ranks, 0, 0, T).hit(ranks[:1], 1, 0, 1)
    for nl, off in ((RL, 0), (RL + 1, 1)):
        read(f"nl{nl}", f"p['nl'] == {nl} and p['runs_off'] == {off} and p['home'] == 'inline'").hit(("range", 100, 100 + nl), 0, 0, 3).hit([100], 1, 0, 1)
    _fillers(cr, read, 12, nleaf)
    return cr


USER_RENAME = {"L7": "X7", "L40": "X40"}  # two leaves of the user tree under names the index does not have


def build(name, lay):
    """(Craft, placement tree, idx_to_pt, user Newick or None) of a design: lad2, lad357, lad357/user, bal"""
    if name == "lad2":
        cr, _ = design_ladder(lay)
    elif name.startswith("lad357"):
        cr, user = design_ladder(lay, (3, 5, 7), 200, "lad357", USER_RENAME)
        if name.endswith("/user"):
            return cr, user, user.map_index(cr.tree), user.nwk
    else:
        cr = design_balanced(lay)
    t = cr.tree
    return cr, t, [se if t.kind[se] == 1 else 0 for se in range(t.nnodes + 1)], None


TREES = ("lad2", "lad357", "lad357/user", "bal")


# ---------------------------------------------------------------------------
# v_llh of an internal candidate against the objective in 256-bit arithmetic on the exact accumulated problem
# ---------------------------------------------------------------------------
M_PLACE_CPU = 0.844  # the oracle's worst |v_llh - f| / B over the internal candidates of the designs, as measured: tests/test_place_craft_cpu.py
M_PLACE_GPU = 2 * M_PLACE_CPU  # twice the oracle's figure, for the reason tests/llh_mp.py gives for M_GPU; not tuned from the device's numbers
LLH_SAMPLE = 50  # of a read of more than LLH_FULL leaves, the internal candidates nearest the root (the longest weights) are checked
LLH_FULL = 300


def llh_nodes(q, tree, nl, nodes):
    """the internal candidates among `nodes` whose v_llh is held to the 256-bit objective: all of them, or for a read of more than
    LLH_FULL leaves (thousands of candidates) the LLH_SAMPLE nearest the root"""
    inner = [n for n in nodes if n in q["acc"]]
    return inner if nl <= LLH_FULL else sorted(inner, key=lambda n: (tree.depth[n], n))[:LLH_SAMPLE]


def llh_ratio(q, node, th, d, v):
    """|v - f(d)| / B for the internal candidate `node` of a read: f and B (tests/llh_mp.py) on the reference's exact histogram, mismatch
    count and rho"""
    import mpmath as mp

    from llh_mp import PREC, f_mp

    h, uc, rho = q["acc"][node]
    with mp.workprec(PREC):
        mc = [mp.mpf(x.numerator) / x.denominator for x in h]
        f, B = f_mp(K, H, th, mc, mp.mpf(uc.numerator) / uc.denominator, rho, d)
        return float(abs(mp.mpf(v) - f) / B)
