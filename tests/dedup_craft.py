"""Crafted records for the likelihood de-duplication (krepp_amd/csrc/kr_dev_likelihood.inc: kr_dedup_clear_kernel, kr_dedup_oslot_kernel,
kr_dedup_kernel, kr_dedup_direct_kernel, kr_dedup_dv_kernel and the hole-skipping of the two likelihood kernels), with the tables
kr_debug_dedup takes, a plain reference of what the stage must decide, and check(): the stage's contract
(docs/design/05_likelihood_select_rows_text.md, "The de-duplication's contract") on any result.

The reference shares nothing with the kernels: the problem of a record, the k-mer-count slots, the direct places (the class numbering is
restated here), a record's first table slot and the batch's table mask.  Only the numbers kr_debug_dedup_layout reports enter -- the two
hash multipliers, the table floor, the probe limit, the chunk --, so a changed constant moves the designs or fails
tests/test_dedup_craft_cpu.py.

A batch is built with Batch: reads of records (leaf, strand, counts) at chosen record slots, holes (key 0) between them.  A record
packs into one word when the stream is at threshold 4, no count exceeds 255 and its read has fewer than 65,536 k-mers; otherwise its
histogram travels in rec_hist and it is its own problem."""
import numpy as np

from acc_craft import FRAC, H, K, M, PPOS, R
from helpers import write_index

NLEAF = 2175                     # a star: leaves se 1 .. 2175, the root se 2176 (leaves 1,024 apart share the low bits of their hash)
TOP = NLEAF + 1                  # the highest node
NNODES = TOP + 1                 # rho entries = BatchOut::dd_nodes at threshold 4: odd, so 440 * dd_nodes is 8 mod 16
RHO = (0.0, 1e-9, 0.3, 1.0)      # rho[se] = RHO[se % 4]
FLAG, HOLE = 0x80000000, 0xFFFFFFFF
POISON32 = 0xA5A5A5A5
POISON64 = int.from_bytes(bytes([0xA5] * 8), "little")
M64, M32 = (1 << 64) - 1, (1 << 32) - 1


class Index:
    """the crafted index: only its node count and rho matter to the stage (the file holds m / (r + 1) = 2 times rho: the loader scales
    it back, exactly)"""

    def __init__(self):
        self.rho = [0.0] + [RHO[se % 4] for se in range(1, NNODES)]
        self.nwk = "(" + ",".join(f"L{i}:1" for i in range(NLEAF)) + ");"

    def write(self, path):
        assert FRAC and M == 2 * (R + 1)
        write_index(path, K, H, M, R, FRAC, PPOS, {0: [(0, 1)]}, [(0, 0)] * NNODES, [2.0 * x for x in self.rho], nwk=self.nwk)
        return path


# ---------------------------------------------------------------------------------------------------------------------------------
# the reference
# ---------------------------------------------------------------------------------------------------------------------------------
def class_table():
    """{counts: class}: the histograms of 1..3 events with no count above 3, numbered in ascending order of the 10-bit code
    c0 | c1 << 2 | c2 << 4 | c3 << 6 | c4 << 8"""
    out = {}
    for code in range(1024):
        c = tuple((code >> (2 * x)) & 3 for x in range(5))
        if 1 <= sum(c) <= 3:
            out[c] = len(out)
    return out


CLASS_OF = class_table()
CLASSES = sorted(CLASS_OF, key=CLASS_OF.get)


def pack(counts, onmers):
    """the packed word: five 8-bit counts, the read's k-mer count in bits 40..55, bit 63"""
    assert len(counts) == 5 and max(counts) < 256 and onmers < 65536
    return sum(c << (8 * x) for x, c in enumerate(counts)) | onmers << 40 | 1 << 63


def unpack(w):
    return tuple((w >> (8 * x)) & 255 for x in range(5)), (w >> 40) & 0xFFFF


def table_mask(nrecs, dd_slots, dd_shift, lay):
    """slots the batch uses, minus one: the floor, doubled while below the table's size and below nrecs >> dd_shift"""
    m = lay["min_slots"]
    while m < dd_slots and m < (nrecs >> dd_shift):
        m *= 2
    return m - 1


def first_slot(word, leaf, mask, lay):
    return ((((word * lay["hash_word"]) & M64) >> 32) ^ ((leaf * lay["hash_leaf"]) & M32)) & mask


def first_slots(words, leaves, mask, lay):
    """first_slot over numpy arrays"""
    w = np.asarray(words, np.uint64) * np.uint64(lay["hash_word"])
    l = (np.asarray(leaves, np.uint64) * np.uint64(lay["hash_leaf"])) & np.uint64(M32)
    return ((w >> np.uint64(32)) ^ l) & np.uint64(mask)


def oslots(t, lay):
    """dd_oslot: the slot of every k-mer count below 256 (0xFF none): the counts of reads with records, the most frequent first, ties to
    the larger count"""
    freq = {}
    for cnt, om in zip(t["rd_cnt"].tolist(), t["rd_onmers"].tolist()):
        if cnt != 0 and om < 256:
            freq[om] = freq.get(om, 0) + 1
    out = np.full(256, 0xFF, np.uint8)
    for rank, om in enumerate(sorted(freq, key=lambda o: (-freq[o], -o))[:lay["oslots"]]):
        out[om] = rank
    return out


def in_read(t):
    """[nrecs] bool, and the read of every record slot (-1 outside)"""
    n = len(t["rec_key"])
    rd = np.full(n, -1, np.int64)
    for r, (o, c) in enumerate(zip(t["rd_off"].tolist(), t["rd_cnt"].tolist())):
        rd[o:o + c] = r
    return rd >= 0, rd


def problems_of(t):
    """the problem of every record slot: ("p", leaf, word) for a packed record, ("o", slot) for one that is its own, None for a hole"""
    inr, _ = in_read(t)
    out = []
    for i, (key, w) in enumerate(zip(t["rec_key"].tolist(), t["rec_w0"].tolist())):
        out.append(None if not inr[i] else (("p", key >> 1, w) if w else ("o", i)))
    return out


def direct_places(t, th, dd_nodes, lay):
    """[nrecs] the direct place of every record slot, -1 for a record that goes through the table or stands alone"""
    out = np.full(len(t["rec_key"]), -1, np.int64)
    if th != 4 or not dd_nodes:
        return out
    osl = oslots(t, lay)
    inr, _ = in_read(t)
    for i, (key, w) in enumerate(zip(t["rec_key"].tolist(), t["rec_w0"].tolist())):
        if not inr[i] or not w:
            continue
        c, om = unpack(w)
        if max(c) <= 3 and 1 <= sum(c) <= lay["max_events"] and om < 256 and osl[om] != 0xFF and (key >> 1) < dd_nodes:
            out[i] = (int(osl[om]) * lay["classes"] + CLASS_OF[c]) * dd_nodes + (key >> 1)
    return out


def problem_inputs(t, th, rho, recs):
    """(hist [n, th + 1], onmers [n], rho [n]) of the records `recs`: what kr_debug_brent takes"""
    _, rd = in_read(t)
    hist = np.zeros((len(recs), th + 1), np.uint32)
    on = np.zeros(len(recs), np.uint32)
    for a, i in enumerate(recs):
        w = int(t["rec_w0"][i])
        if w:
            hist[a], on[a] = unpack(w)
        else:
            hist[a], on[a] = t["rec_hist"][i], t["rd_onmers"][rd[i]]
    return hist, on, np.array([rho[int(t["rec_key"][i]) >> 1] for i in recs], np.float64)


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


class Config:
    """what a stream is: threshold, nodes of the direct part (0: off), table slots and shift, the index's rho, the library's constants"""

    def __init__(self, lay, rho, th=4, dd_nodes=NNODES, dd_slots=1 << 14, dd_shift=1):
        self.lay, self.rho, self.th, self.dd_nodes, self.dd_slots, self.dd_shift = lay, rho, th, (dd_nodes if th == 4 else 0), dd_slots, dd_shift

    @property
    def places(self):
        return self.lay["oslots"] * self.lay["classes"] * self.dd_nodes


def check(t, r, cfg, brent, allow_excess=True, what=""):
    """The contract of the stage on the result `r` of tables `t` (numbering as in the design document):
    1 every record of a read resolves to a list position below `problems` whose entry is a record of the same problem (the very record if
      it is its own problem); holes keep rec_rep 0xFFFFFFFF
    2 the list holds holes or record indices, none twice, every representative resolves to its own position, poison behind the list
    3 direct records name the reference's place exactly, nobody else is flagged; unnamed places hold 0xFFFFFFFF, a named place one
      position whose entry names it; a direct problem is listed once and has no table entry
    4 the table as read back: published entries of listed problems, no problem in two slots, no empty slot inside a chain
    5 rep_dv bit-equal to brent() on every listed problem, poison at holes and behind the list; dd_dv likewise by place
    6 listed >= distinct; equal for the direct part, and for a batch of at most 64 record slots (unless allow_excess: one wave is
      deterministic as long as no record runs out of probe rounds)
    7 no error flag; problems <= listed + the holes take_positions can leave (derived at the assertion)
    Returns the figures of the case."""
    lay = cfg.lay
    nrecs = len(t["rec_key"])
    inr, rd = in_read(t)
    prob = problems_of(t)
    rec_rep, rep_list, rep_dv = r["rec_rep"], r["rep_list"], r["rep_dv"]
    problems = r["problems"]
    assert r["err"] == 0, (what, "7: error flags", r["err"])
    assert problems <= len(rep_list), (what, "the list read back is shorter than the problems", problems, len(rep_list))
    mask = table_mask(nrecs, r["dd_slots"], r["dd_shift"], lay)
    assert r["mask"] == mask and r["dd_nodes"] == cfg.dd_nodes and r["places"] == cfg.places, (what, "the stream is not the configuration's")
    dd_direct, dd_dv = r["dd_direct"], r["dd_dv"]
    assert len(dd_direct) == cfg.places
    # ---- 2: the list
    lst = rep_list[:problems].astype(np.int64)
    holes = lst == HOLE
    listed_pos = np.nonzero(~holes)[0]
    listed = lst[listed_pos]
    assert (listed < nrecs).all(), (what, "2: a list entry that is no record index")
    assert inr[listed].all(), (what, "2: a hole record listed")
    assert len(np.unique(listed)) == len(listed), (what, "2: a record listed twice")
    assert (rep_list[problems:] == POISON32).all(), (what, "2: written behind the list")
    pos_of_rec = np.full(nrecs, -1, np.int64)
    pos_of_rec[listed] = listed_pos
    # ---- 1: every record resolves
    assert (rec_rep[~inr] == HOLE).all(), (what, "1: rec_rep of a hole record")
    flagged = inr & (rec_rep != HOLE) & ((rec_rep & FLAG) != 0)
    place = np.where(flagged, rec_rep & ~np.uint32(FLAG), 0).astype(np.int64)
    assert (place[flagged] < cfg.places).all(), (what, "1: a flagged place beyond the places")
    pos = rec_rep.astype(np.int64)
    if flagged.any():
        pos[flagged] = dd_direct[place[flagged]]
    recs = np.nonzero(inr)[0]
    assert (pos[recs] < problems).all(), (what, "1: a record that resolves to no list position", recs[pos[recs] >= problems][:5])
    assert (lst[pos[recs]] != HOLE).all(), (what, "1: a record that resolves to a hole of the list")
    for i in recs.tolist():
        j = int(lst[pos[i]])
        assert prob[j] == prob[i], (what, "1: record resolved to another problem", i, prob[i], j, prob[j])
    assert (pos[listed] == listed_pos).all(), (what, "2: a representative that does not resolve to its own position")
    # ---- 3: the direct part
    want_place = direct_places(t, cfg.th, cfg.dd_nodes, lay)
    is_direct = want_place >= 0
    assert (flagged == is_direct).all(), (what, "3: flagged records are not the direct ones", np.nonzero(flagged != is_direct)[0][:5])
    assert (place[is_direct] == want_place[is_direct]).all(), (what, "3: a direct record at another place")
    named = np.zeros(cfg.places, bool)
    named[want_place[is_direct]] = True
    assert (dd_direct[~named] == HOLE).all(), (what, "3: a place nobody names holds something", np.nonzero(dd_direct[~named] != HOLE)[0][:5])
    if named.any():
        p = dd_direct[named].astype(np.int64)
        assert (p < problems).all() and (lst[p] != HOLE).all(), (what, "3: a named place without a list position")
        assert (want_place[lst[p]] == np.nonzero(named)[0]).all(), (what, "3: a place whose list entry does not name it")
    if cfg.th == 4 and cfg.dd_nodes:
        assert (r["dd_oslot"] == oslots(t, lay)).all(), (what, "3: the k-mer-count slots", r["dd_oslot"][r["dd_oslot"] != 0xFF], np.nonzero(r["dd_oslot"] != 0xFF)[0])
    count = {}
    for j in listed.tolist():
        count[prob[j]] = count.get(prob[j], 0) + 1
    direct_probs = {prob[i] for i in np.nonzero(is_direct)[0].tolist()}
    assert all(count[p_] == 1 for p_ in direct_probs), (what, "3/6: a direct problem listed more than once")
    # ---- 4: the table
    tab = r["dd_table"]
    assert len(tab) > mask, (what, "the table read back is shorter than the mask")
    tab = tab[:mask + 1]  # (slots beyond the mask are not part of the result)
    full = np.nonzero(tab[:, 0] != 0)[0]
    seen = {}
    for s in full.tolist():
        w, y = int(tab[s, 0]), int(tab[s, 1])
        assert y >> 32 != 0, (what, "4: a claimed slot whose second word was never published", s)
        leaf, p = y & M32, (y >> 32) - 1
        assert p < problems and lst[p] != HOLE, (what, "4: a slot with a position that lists nothing", s, p)
        assert prob[int(lst[p])] == ("p", leaf, w), (what, "4: a slot whose position lists another problem", s, prob[int(lst[p])], (leaf, w))
        assert ("p", leaf, w) not in seen, (what, "4: a problem in two slots", s, seen.get(("p", leaf, w)))
        assert ("p", leaf, w) not in direct_probs, (what, "3: a direct problem in the table", s)
        seen[("p", leaf, w)] = s
        q = first_slot(w, leaf, mask, lay)
        while q != s:
            assert tab[q, 0] != 0, (what, "4: an empty slot inside a chain", s, q)
            q = (q + 1) & mask
    # ---- 5: the values
    hist, on, rho = problem_inputs(t, cfg.th, cfg.rho, listed.tolist())
    if len(listed):
        d, v = brent(hist, on, rho)
        assert (bits(rep_dv[listed_pos, 0]) == bits(d)).all() and (bits(rep_dv[listed_pos, 1]) == bits(v)).all(), (what, "5: a listed problem's value")
    assert (bits(rep_dv[:problems][holes]) == POISON64).all(), (what, "5: a value at a hole of the list")
    assert (bits(rep_dv[problems:]) == POISON64).all(), (what, "5: a value behind the list")
    if cfg.places:
        assert (bits(dd_dv[~named]) == POISON64).all(), (what, "5: a value at a place nobody names")
        assert (bits(dd_dv[named]) == bits(rep_dv[dd_direct[named].astype(np.int64)])).all(), (what, "5: a place's value is not its position's")
    # ---- 6: the counts
    distinct = len({p_ for p_ in prob if p_ is not None})
    nlisted = len(listed)
    assert nlisted >= distinct, (what, "6: fewer problems listed than there are", nlisted, distinct)
    excess = nlisted - distinct
    if nrecs <= 64 and not allow_excess:
        assert excess == 0, (what, "6: one wave listed a problem twice", excess)
    # ---- 7: the extent of the list.  Only take_positions leaves holes (kr_dedup_direct_kernel takes exactly what it lists unless the
    # batch is over capacity).  A wave's chunk is max(n, c) positions, c = rep_chunk (16 here: it grows only beyond 4 M records), taken
    # when a request of n does not fit the tail before it.  So a chunk serves its first request in full and ends with at most c - 1
    # holes (none if n >= c); and a discarded tail is shorter than the request that discarded it, all of which is listed.  With a chunks
    # and L listed entries of a wave: holes <= min((c - 1) a, L - a + c - 1) <= (c - 1)(L + c - 1) / c.  (The records of a batch below
    # kDedupBlocks * 256 slots are visited once, slot i by wave i / 64.)
    c = lay["rep_chunk"]
    assert nrecs <= lay["dedup_blocks"] * 256
    by_wave = np.bincount(listed[~is_direct[listed]] // 64, minlength=1)
    bound = int(sum((c - 1) * (int(L) + c - 1) // c for L in by_wave if L))
    nholes = problems - nlisted
    assert nholes == int(holes.sum()) and nholes <= bound, (what, "7: more holes in the list than take_positions can leave", nholes, bound)
    waves = len(np.unique(recs // 64))
    assert problems <= nlisted + waves * c + 4095, (what, "7: the list's extent", problems, nlisted, waves)
    for_table = len({p_ for p_ in prob if p_ is not None and p_[0] == "p"} - direct_probs)
    return dict(nrecs=nrecs, distinct=distinct, listed=nlisted, excess=excess, problems=problems, holes=nholes, direct=len(direct_probs),
                in_table=len(full), absent=for_table - len(full), mask=mask)


def model(t, cfg, brent, rep_room=None, table_room=None):
    """A plain sequential run of the stage, as a result of kr_debug_dedup: records in slot order, open addressing with the probe limit,
    the direct places listed behind the table's problems in place order, no holes in the list."""
    lay = cfg.lay
    nrecs = len(t["rec_key"])
    mask = table_mask(nrecs, cfg.dd_slots, cfg.dd_shift, lay)
    prob = problems_of(t)
    want_place = direct_places(t, cfg.th, cfg.dd_nodes, lay)
    rep_room = rep_room or nrecs + 64
    tab = np.zeros((max(table_room or 0, mask + 1), 2), np.uint64)
    rec_rep = np.full(nrecs, HOLE, np.uint32)
    lst = []
    dd_direct = np.full(cfg.places, HOLE, np.uint32)
    for i, p in enumerate(prob):
        if p is None:
            continue
        if want_place[i] >= 0:
            rec_rep[i] = FLAG | int(want_place[i])
            dd_direct[want_place[i]] = i  # (the last record of a place represents it)
            continue
        if p[0] == "p":
            _, leaf, w = p
            s = first_slot(w, leaf, mask, lay)
            for _ in range(lay["probe_rounds"]):
                if tab[s, 0] == 0:
                    tab[s] = (w, leaf | (len(lst) + 1) << 32)
                    lst.append(i)
                if int(tab[s, 0]) == w and int(tab[s, 1]) & M32 == leaf:
                    rec_rep[i] = (int(tab[s, 1]) >> 32) - 1
                    break
                s = (s + 1) & mask
        if rec_rep[i] == HOLE:  # its own problem, or out of rounds
            rec_rep[i] = len(lst)
            lst.append(i)
    for pl in np.nonzero(dd_direct != HOLE)[0].tolist():
        lst.append(int(dd_direct[pl]))
        dd_direct[pl] = len(lst) - 1
    rep_list = np.full(rep_room, POISON32, np.uint32)
    rep_list[:len(lst)] = lst
    rep_dv = np.full((rep_room, 2), POISON64, np.uint64).view(np.float64)
    dd_dv = np.full((cfg.places, 2), POISON64, np.uint64).view(np.float64)
    if lst:
        d, v = brent(*problem_inputs(t, cfg.th, cfg.rho, lst))
        rep_dv[:len(lst), 0], rep_dv[:len(lst), 1] = d, v
    nm = dd_direct != HOLE
    dd_dv[nm] = rep_dv[dd_direct[nm].astype(np.int64)]
    return dict(rec_rep=rec_rep, rep_list=rep_list, rep_dv=rep_dv, dd_direct=dd_direct, dd_dv=dd_dv, dd_table=tab,
                dd_oslot=oslots(t, lay) if cfg.dd_nodes else np.full(256, 0x5A, np.uint8), problems=len(lst), err=0, rep_cap=rep_room,
                places=cfg.places, dd_nodes=cfg.dd_nodes, mask=mask, dd_slots=cfg.dd_slots, dd_shift=cfg.dd_shift)


def fake_brent(hist, on, rho):
    """(tests without a device) a stand-in for kr_debug_brent: any pure function of the problem"""
    h = (np.asarray(hist, np.float64) * (np.arange(hist.shape[1]) + 1.5)).sum(axis=1)
    return h / (np.asarray(on, np.float64) + 1.0) + rho, -h - np.asarray(on, np.float64) * (1.0 + rho)


# ---------------------------------------------------------------------------------------------------------------------------------
# batches
# ---------------------------------------------------------------------------------------------------------------------------------
class Batch:
    """record slots in order: read(onmers, recs) appends a read whose records (leaf, strand, counts) take the next slots, hole(n) leaves
    n slots with key 0, pad_to(slot) holes up to a slot"""

    def __init__(self, th=4):
        self.th = th
        self.rd_off, self.rd_cnt, self.rd_onmers = [], [], []
        self.key, self.w0, self.hist, self.rread = [], [], [], []

    @property
    def nrecs(self):
        return len(self.key)

    def hole(self, n=1):
        for _ in range(n):
            self.key.append(0), self.w0.append(0), self.hist.append([0] * (self.th + 1)), self.rread.append(0)
        return self

    def pad_to(self, slot):
        assert slot >= self.nrecs
        return self.hole(slot - self.nrecs)

    def read(self, onmers, recs=()):
        r = len(self.rd_off)
        self.rd_off.append(self.nrecs), self.rd_cnt.append(len(recs)), self.rd_onmers.append(onmers)
        for leaf, strand, counts in recs:
            counts = tuple(counts)
            assert len(counts) == self.th + 1 and 0 < leaf < NNODES
            packs = self.th == 4 and max(counts) < 256 and onmers < 65536
            self.key.append(leaf << 1 | strand), self.w0.append(pack(counts, onmers) if packs else 0)
            self.hist.append(list(counts)), self.rread.append(r)
        return self

    def tables(self):
        n = self.nrecs
        return dict(rd_off=np.array(self.rd_off, np.uint32), rd_cnt=np.array(self.rd_cnt, np.uint32), rd_onmers=np.array(self.rd_onmers, np.uint32),
                    rec_key=np.array(self.key, np.uint32), rec_w0=np.array(self.w0, np.uint64),
                    rec_hist=np.array(self.hist, np.uint32).reshape(n, self.th + 1), rec_read=np.array(self.rread, np.uint32))


def concat(ts):
    """several batches' tables as one batch, in order"""
    out = {k: [] for k in ts[0]}
    recs = reads = 0
    for t in ts:
        out["rd_off"].append(t["rd_off"] + np.uint32(recs)), out["rec_read"].append(t["rec_read"] + np.uint32(reads))
        for k in ("rd_cnt", "rd_onmers", "rec_key", "rec_w0", "rec_hist"):
            out[k].append(t[k])
        recs, reads = recs + len(t["rec_key"]), reads + len(t["rd_off"])
    return {k: np.concatenate(v) for k, v in out.items()}


def ev(x, c=1):
    """counts with c events at Hamming distance x"""
    return tuple(c if i == x else 0 for i in range(5))


def colliding(lay, mask, want, n, words, leaves=range(1, NNODES), exclude=()):
    """n distinct (leaf, word) whose first slot under `mask` lies in the set `want` (searched in a fixed order); with want None: the
    fullest first slot"""
    leaves = np.array(list(leaves), np.uint64)
    ws = np.array(list(words), np.uint64)
    L, W = np.meshgrid(leaves, ws, indexing="ij")
    sl = first_slots(W.ravel(), L.ravel(), mask, lay).astype(np.int64)
    if want is None:
        want = {int(np.bincount(sl, minlength=mask + 1).argmax())}
    ok = np.nonzero(np.isin(sl, list(want)))[0]
    out = [(int(L.ravel()[i]), int(W.ravel()[i])) for i in ok.tolist() if (int(L.ravel()[i]), int(W.ravel()[i])) not in exclude]
    assert len(out) >= n, (len(out), n)
    return out[:n]


def table_words(onmers=255, lo=5, hi=64):
    """packed words of a read of `onmers` k-mers that can never be direct: one count of lo .. hi - 1 at each Hamming distance"""
    return [pack(ev(x, c), onmers) for c in range(lo, hi) for x in range(5)]


def design_classes(lay):
    """Every one of the 55 classes once on leaf 5 and once on the highest node, and beside them what must not be direct: a count of 4,
    four events of 1, a count of 255 (its read has 255 k-mers, a count with a slot), a read of 256 k-mers, a read whose k-mer count has
    no slot.  Slots: 130 (4 reads; the tie goes to the larger count), 100..105 (4 reads each), 255 (2 reads, tied with 77: the larger count wins), none for 77 and 256.
    Every read is given twice, so every record has a duplicate in another read."""
    b = Batch()
    for _ in range(2):
        for leaf in (5, TOP):
            b.read(130, [(leaf, 0, c) for c in CLASSES] + [(leaf, 1, ev(0, 4)), (leaf, 1, (1, 1, 1, 1, 0))])
        b.read(255, [(5, 0, ev(2, 255)), (TOP, 0, ev(1, 2))])
        b.read(256, [(5, 0, ev(0)), (TOP, 1, ev(4, 3))])
        b.read(77, [(5, 0, ev(0)), (TOP, 1, ev(4, 3))])
    for om in range(100, 106):
        for leaf in (7, 8, 7, 8):
            b.read(om, [(leaf, 0, ev(3, 2))])
    return b.tables()


def design_last_place(lay):
    """(0, 0, 0, 0, 3) -- the last class -- on the highest node in a read whose k-mer count has the slot of rank 7: the last place"""
    b = Batch()
    for om in range(200, 207):
        b.read(om, [(3, 0, ev(0))]).read(om, [(4, 1, ev(1))])
    b.read(50, [(TOP, 1, ev(4, 3))])
    return b.tables()


def design_oslots_a(lay):
    """9 k-mer counts: 10..16 in three reads each, 20 and 30 in two: 30 takes the last slot, 20 none (its records go through the table)"""
    b = Batch()
    for om, n in [(c, 3) for c in range(10, 17)] + [(20, 2), (30, 2)]:
        for q in range(n):
            b.read(om, [(11 + q, 0, ev(1)), (40, 1, ev(2, 2))])
    return b.tables()


def design_oslots_b(lay):
    """three k-mer counts: ranks 0..2, everything else without a slot"""
    b = Batch()
    for om, n in ((90, 1), (91, 3), (92, 2)):
        for q in range(n):
            b.read(om, [(21 + q, 0, ev(0, 3)), (22, 1, ev(4))])
    return b.tables()


def design_oslots_c(lay):
    """the most frequent count (99) belongs only to reads without records, the next (300) is beyond the slots: neither gets one"""
    b = Batch()
    for q in range(10):
        b.read(99)
    for q in range(8):
        b.read(300, [(30 + q % 2, 0, ev(1))])
    b.read(40, [(30, 0, ev(1))]).read(41, [(30, 0, ev(1))]).read(41, [(31, 0, ev(1))])
    return b.tables()


def design_oslots_d(lay):
    """oslot_reads + 1 reads, a grid of two blocks: the reads that decide (the counts of oslots_a) are reads 300.. -- threads of the
    second block (the grid strides by 512 reads, block 1 takes 256..511 of every stride) -- and the last read, which the first takes"""
    n = lay["oslot_reads"] + 1
    deciding = [c for c in range(10, 17) for _ in range(3)] + [20, 20, 30]
    b = Batch()
    for r in range(n):
        if 300 <= r < 300 + len(deciding):
            b.read(deciding[r - 300], [(11, 0, ev(1)), (40, 1, ev(2, 2))])
        elif r == n - 1:
            b.read(30, [(12, 0, ev(1))])
        else:
            b.read(99)
    return b.tables()


def design_same_word_other_leaf(lay):
    """one packed word that cannot be direct, (5, 0, 0, 0, 0) of a 130-k-mer read, on 40 leaves, at least three of which share their
    first slot under the 1,024-slot mask: the probe meets an equal first word with another leaf.  Given twice."""
    w = pack(ev(0, 5), 130)
    mask = lay["min_slots"] - 1
    same = colliding(lay, mask, None, 3, [w])
    leaves = [l for l, _ in same] + [l for l in range(1, NNODES) if l not in {x for x, _ in same}][:37]
    b = Batch()
    for _ in range(2):
        b.read(130, [(l, 0, ev(0, 5)) for l in leaves])
    return b.tables()


def design_chain_wrap(lay):
    """12 distinct table problems whose first slot is one of the last four under the 1,024-slot mask: the chain continues at slot 0.  The
    last three are given a second time."""
    mask = lay["min_slots"] - 1
    ps = colliding(lay, mask, set(range(mask - 3, mask + 1)), 12, table_words())
    b = Batch()
    b.read(255, [(l, 0, unpack(w)[0]) for l, w in ps])
    b.read(255, [(l, 0, unpack(w)[0]) for l, w in ps[-3:]])
    return b.tables()


def design_one_wave_same_problem(lay):
    """slots 0..63: 64 records of one table problem (one CAS winner; the other lanes meet the word before its second word is published);
    slots 64..127: 64 distinct problems with one first slot"""
    mask = lay["min_slots"] - 1
    ps = colliding(lay, mask, None, 64, table_words(hi=256))
    b = Batch()
    b.read(130, [(9, 0, ev(0, 7))] * 64)
    b.read(255, [(l, 0, unpack(w)[0]) for l, w in ps])
    assert first_slot(pack(ev(0, 7), 130), 9, mask, lay) != first_slot(ps[0][1], ps[0][0], mask, lay)
    return b.tables()


def design_beyond_48(lay):
    """60 distinct problems with one first slot in slots 0..59 (one wave), their duplicates in slots 64..123 (the next): no record gets
    further than probe_rounds slots, so at least 60 - probe_rounds problems are absent from the table and their records stand alone"""
    mask = lay["min_slots"] - 1
    ps = colliding(lay, mask, None, 60, table_words(hi=256))
    b = Batch()
    b.read(255, [(l, 0, unpack(w)[0]) for l, w in ps]).pad_to(64)
    b.read(255, [(l, 0, unpack(w)[0]) for l, w in ps])
    return b.tables()


def design_crowded(lay):
    """5,000 distinct table problems (500 leaves, ten words), each given twice: 100 reads of 100 records"""
    ps = [(leaf, c) for c in range(5, 15) for leaf in range(1, 501)]
    b = Batch()
    for _ in range(2):
        for q in range(0, len(ps), 100):
            b.read(130, [(l, l & 1, ev(1, c)) for l, c in ps[q:q + 100]])
    return b.tables()


def design_own(lay):
    """records that are their own problem at threshold 4, between packed ones: a count of 300 (its histogram does not fit the word's
    bytes), reads of 70,000 k-mers (the count does not fit bits 40..55); two identical ones stay two problems"""
    b = Batch()
    b.read(400, [(3, 0, ev(1, 2)), (4, 0, ev(0, 300)), (4, 0, ev(0, 300)), (6, 1, ev(2, 9)), (6, 1, ev(2, 9))])
    b.read(70000, [(3, 0, ev(1, 2)), (3, 0, ev(1, 2)), (TOP, 1, ev(4, 3))])
    b.read(400, [(3, 0, ev(1, 2)), (4, 0, ev(0, 300)), (7, 0, ev(3, 1))])
    return b.tables()


def mixed(th, n, seed):
    """n records of a fixed mix: few events (direct at threshold 4), table problems, with repeats"""
    recs = []
    for q in range(n):
        a = (q * 7 + seed) % 23
        leaf = 1 + (a * 37 + seed) % (NNODES - 1)
        c = [0] * (th + 1)
        c[a % (th + 1)] = 1 + a % 3 if a % 2 else 5 + a % 4
        recs.append((leaf, a & 1, tuple(c)))
    return recs


def design_holes(lay, end, th=4):
    """reads whose ranges leave 1, 63 and 64 key-0 slots between them; the last read ends at slot `end` (255, 256, 257: the edges of a
    wave and of a workgroup in the record loop)"""
    b = Batch(th)
    b.read(130, mixed(th, 10, 1)).hole(1)
    b.read(130, mixed(th, 20, 2)).hole(63)
    b.read(131, mixed(th, 30, 3)).hole(64)
    b.read(130, mixed(th, end - b.nrecs, 4))
    assert b.nrecs == end
    return b.tables()


def design_th_other(lay, th):
    """thresholds 2 and 6: planes only, every record its own problem"""
    return design_holes(lay, 257, th)


DESIGNS = dict(classes=design_classes, last_place=design_last_place, oslots_a=design_oslots_a, oslots_b=design_oslots_b, oslots_c=design_oslots_c,
               oslots_d=design_oslots_d, same_word_other_leaf=design_same_word_other_leaf, chain_wrap=design_chain_wrap,
               one_wave_same_problem=design_one_wave_same_problem, beyond_48=design_beyond_48, crowded=design_crowded, own=design_own,
               holes_255=lambda lay: design_holes(lay, 255), holes_256=lambda lay: design_holes(lay, 256), holes_257=lambda lay: design_holes(lay, 257))
