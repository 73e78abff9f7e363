"""Every route of the likelihood de-duplication (kr_dev_likelihood.inc) on crafted records (tests/dedup_craft.py), through
kr_debug_dedup: the lane's view is the submit path's own, the launches are launch_likelihood's.  Every result is held to
dedup_craft.check -- the stage's contract (docs/design/05_likelihood_select_rows_text.md, "The de-duplication's contract"), values bit
for bit against kr_debug_brent -- and each test names the route it forces and the output that shows the route was taken: a flagged
place, a slot displaced in the read-back table, a problem absent from a full table, a list longer than the distinct problems.

The streams are module-scoped, one per regime (threshold, KR_DD_SHIFT, KR_DD_DIRECT, KR_DEBUG_POISON: all read when a stream is
made), max_reads 8,192 and max_records 16,384; the tests of one regime share its stream on purpose, so every run also meets what the
run before it left in the table, the direct places and the lists.

Not here: the growth of a wave's chunk of list positions beyond 16 (rep_chunk) needs more than 4 M records in a batch and is left to
the large-batch tests (tests/test_gpu_indexed_rows_capacity.py, tests/test_gpu_llh_numerics.py)."""
import contextlib
import os

import numpy as np
import pytest

import dedup_craft as dc

pytestmark = pytest.mark.gpu

REGIMES = dict(default={}, shift8={"KR_DD_SHIFT": "8"}, direct_off={"KR_DD_DIRECT": "0"}, poison={"KR_DEBUG_POISON": "all"},
               poison_shift8={"KR_DEBUG_POISON": "all", "KR_DD_SHIFT": "8"})


@contextlib.contextmanager
def environ(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


class Env:
    def __init__(self, capi, tmp):
        self.capi = capi
        self.ix = dc.Index()
        self.lay = capi.dedup_layout()
        self.hx = capi.HostIndex(self.ix.write(str(tmp / "idx")))
        assert self.hx.lib_arrays()["rho"].tolist() == self.ix.rho  # what the likelihood kernels read is what kr_debug_brent is given
        self.dx = self.hx.upload(0)
        self._tables, self._streams, self._values = {}, {}, {}

    def tables(self, name):
        if name not in self._tables:
            self._tables[name] = dc.concat([self.tables(n) for n in dc.DESIGNS]) if name == "all" else dc.DESIGNS[name](self.lay)
        return self._tables[name]

    def stream(self, regime="default", th=4):
        if (regime, th) not in self._streams:
            with environ(REGIMES[regime]):
                self._streams[(regime, th)] = self.dx.stream(self.capi.default_params(hdist_th=th), max_reads=8192, max_bases=1 << 16, max_records=16384)
        return self._streams[(regime, th)]

    def config(self, regime="default", th=4):
        return dc.Config(self.lay, self.ix.rho, th=th, dd_nodes=0 if regime == "direct_off" else dc.NNODES)

    def brent(self, th):
        """kr_debug_brent with every distinct problem computed once for the module"""
        memo = self._values

        def f(hist, on, rho):
            keys = [(th, tuple(h), int(o), float(r)) for h, o, r in zip(hist.tolist(), on.tolist(), rho.tolist())]
            new = sorted({k for k in keys if k not in memo})
            if new:
                d, v = self.dx.brent(th, np.array([k[1] for k in new], np.uint32), np.array([k[2] for k in new], np.uint32), np.array([k[3] for k in new]))
                memo.update(zip(new, zip(d.tolist(), v.tolist())))
            return np.array([memo[k][0] for k in keys]), np.array([memo[k][1] for k in keys])
        return f

    def run(self, name, regime="default", th=4, tables=None, **kw):
        """one kr_debug_dedup of a design on the regime's stream: (tables, result, figures of check)"""
        t = self.tables(name) if tables is None else tables
        cfg = self.config(regime, th)
        r = self.stream(regime, th).debug_dedup(t, places=cfg.places, **kw)
        f = dc.check(t, r, cfg, self.brent(th), allow_excess=False, what=(name, regime, th))
        print(f"dedup {name} [{regime}, th {th}]: {f}")
        return t, r, f

    def close(self):
        for s in self._streams.values():
            s.close()
        self.dx.close()
        self.hx.close()


@pytest.fixture(scope="module")
def env(capi, tmp_path_factory):
    e = Env(capi, tmp_path_factory.mktemp("dedup_routes"))
    yield e
    e.close()


def resolved(t, r):
    """list position of every record slot (-1 for holes)"""
    rep = r["rec_rep"].astype(np.int64)
    fl = (rep != dc.HOLE) & ((rep & dc.FLAG) != 0)
    rep[fl] = r["dd_direct"][rep[fl] & ~dc.FLAG] if fl.any() else rep[fl]
    rep[r["rec_rep"] == dc.HOLE] = -1
    return rep


def displaced(r, lay):
    """(slot, first slot) of the table entries that do not sit in their first slot"""
    tab, mask = r["dd_table"], r["mask"]
    out = []
    for s in np.nonzero(tab[:mask + 1, 0])[0].tolist():
        f = dc.first_slot(int(tab[s, 0]), int(tab[s, 1]) & dc.M32, mask, lay)
        if f != s:
            out.append((s, f))
    return out


def test_classes_every_class_and_its_neighbours(env):
    """Direct part: all 55 count classes on a leaf and on the highest node (witness: 110 + 13 flagged places, each with one list position,
    every record's rec_rep the reference's flagged place), and beside them the codes that must take the table (a count of 4, four
    events, a count of 255, a read of 256 k-mers, a k-mer count without a slot; witness: not flagged, present in the read-back table)."""
    t, r, f = env.run("classes")
    pl = dc.direct_places(t, 4, dc.NNODES, env.lay)
    assert f["direct"] == len(set(pl[pl >= 0].tolist())) == 2 * 55 + 1 + 6 * 2 and f["excess"] == 0
    assert f["in_table"] == 2 * 2 + 1 + 2 + 2 and f["absent"] == 0  # (a count of 4 and four events on two nodes, the count of 255, two records each of 256 and 77 k-mers)


def test_last_place(env):
    """Direct part: the last place, 440 * dd_nodes - 1, half-way into kr_dedup_direct_kernel's last 16-place group (dd_nodes is odd)
    and in the last, partly filled 4,096-place block; witness: the record's flagged rec_rep and the place's list position and value."""
    t, r, f = env.run("last_place")
    last = env.lay["oslots"] * env.lay["classes"] * dc.NNODES - 1
    i = len(t["rec_key"]) - 1
    assert last % 16 == 7 and r["rec_rep"][i] == (dc.FLAG | last) and r["dd_direct"][last] != dc.HOLE and r["rep_list"][r["dd_direct"][last]] == i
    assert f["excess"] == 0 and f["in_table"] == 0


@pytest.mark.parametrize("name", ["oslots_a", "oslots_b", "oslots_c", "oslots_d"])
def test_kmer_count_slots(env, name):
    """Direct part: the choice of the eight k-mer-count slots -- nine counts with a tie for the last slot (a), fewer than eight (b), a most
    frequent count that only reads without records or of 256 k-mers and more have (c), and 4,097 reads, so that kr_dedup_oslot_kernel
    runs two blocks and the last one out ranks the counts of both (d).  Witness: dd_oslot equals the reference's exactly (check), and
    the records of the count left without a slot sit in the table while the others' are flagged."""
    t, r, f = env.run(name)
    assert f["excess"] == 0 and f["absent"] == 0
    if name in ("oslots_a", "oslots_d"):
        assert r["dd_oslot"][30] == 7 and r["dd_oslot"][20] == 0xFF and f["in_table"] == (3 if name == "oslots_a" else 2)  # the problems of the 20-k-mer reads
    if name == "oslots_c":
        assert r["dd_oslot"][99] == 0xFF and f["in_table"] == 2 and (r["rec_rep"][:8] & dc.FLAG == 0).all()


def test_same_word_other_leaf(env):
    """Table: one histogram word on 40 leaves, three of them with one first slot -- the probe finds an equal first word with another
    leaf and moves on.  Witness: the read-back table holds a displaced entry whose first slot holds the same word with another leaf."""
    t, r, f = env.run("same_word_other_leaf")
    tab = r["dd_table"]
    d = displaced(r, env.lay)
    assert len(d) >= 2 and all(tab[fs, 0] == tab[s, 0] and tab[fs, 1] & dc.M32 != tab[s, 1] & dc.M32 for s, fs in d)
    assert f["distinct"] == 40 and f["absent"] == 0


def test_chain_wraps_to_slot_0(env):
    """Table: a probe chain that runs from the last slots of the 1,024-slot table on to slot 0.  Witness: slots 1,020..1,023 and
    0..7 are taken, and the entries in the low slots have their first slot among the last four."""
    t, r, f = env.run("chain_wrap")
    mask = r["mask"]
    assert mask == 1023 and f["in_table"] == 12 and f["absent"] == 0
    low = [(s, fs) for s, fs in displaced(r, env.lay) if s < 8]
    assert len(low) == 8 and all(fs >= mask - 3 for s, fs in low)
    if f["excess"]:
        print("chain_wrap: excess", f["excess"])


def test_one_wave_same_problem(env):
    """Table: the 64 lanes of one wave hold the same new problem -- one lane's CAS wins, the others see the word with its second word
    not yet published and come round again.  Witness: the 64 records share ONE list position; then 64 distinct problems with one first
    slot in the next wave: probe_rounds of them in a chain, the rest absent from the table and standing alone."""
    t, r, f = env.run("one_wave_same_problem")
    assert len(set(r["rec_rep"][:64].tolist())) == 1
    assert f["in_table"] == 1 + env.lay["probe_rounds"] and f["absent"] == 64 - env.lay["probe_rounds"] and f["excess"] == 0


def test_chain_longer_than_the_probe_limit(env):
    """Table: 60 problems with one first slot, and their duplicates in the next wave.  No record looks further than probe_rounds slots,
    so the table takes at most probe_rounds of them (witness: the read-back table) and the records of the others stand alone: each of
    those problems is listed twice, the list is longer than the distinct problems by at least 60 - probe_rounds (asserted: the model
    says it must be; how much longer depends on which wave publishes first, printed)."""
    t, r, f = env.run("beyond_48")
    rounds = env.lay["probe_rounds"]
    assert f["in_table"] <= rounds and f["absent"] >= 60 - rounds and f["excess"] >= 60 - rounds
    pos = resolved(t, r)
    prob = dc.problems_of(t)
    in_tab = {(int(y) & dc.M32, int(w)) for w, y in r["dd_table"][:r["mask"] + 1].tolist() if w}
    for i in range(60):
        if (prob[i][1], prob[i][2]) not in in_tab:
            assert pos[i] != pos[64 + i]  # absent: both records stand alone


def test_crowded_on_the_floor(env):
    """Table: crowded mode on the 1,024-slot floor (KR_DD_SHIFT=8): 5,000 problems, each given twice.  Witness: at least 3,976 problems
    absent from the full table, their records standing alone, the list longer than the distinct problems."""
    t, r, f = env.run("crowded", "shift8")
    assert r["mask"] == 1023 and r["dd_shift"] == 8
    assert f["absent"] >= f["distinct"] - 1024 and f["listed"] > f["distinct"] and f["excess"] >= f["absent"]


def test_crowded_in_a_roomy_table(env):
    """The same tables on a default stream: the mask is 8,191 (1,024 doubled while below 10,000 >> 1).  The excess of the list over the
    distinct problems is a timing figure here (a wave that meets another's unpublished slot 48 times gives up): printed, not bounded."""
    t, r, f = env.run("crowded")
    assert r["mask"] == 8191 and r["dd_shift"] == 1 and f["distinct"] == 5000


def test_own_problems(env):
    """Records the word cannot describe at threshold 4 (a count of 300, reads of 70,000 k-mers) between packed ones: each is listed
    for itself -- two identical ones at two positions --, with the value of its planes and its read's k-mer count."""
    t, r, f = env.run("own")
    pos = resolved(t, r)
    own = np.nonzero(t["rec_w0"] == 0)[0]
    assert len(own) == 6 and len(set(pos[own].tolist())) == 6 and f["excess"] == 0
    assert (r["rep_list"][pos[own]] == own).all()


@pytest.mark.parametrize("end", [255, 256, 257])
def test_holes_and_the_edges_of_the_record_loop(env, end):
    """List and record loop: key-0 slots between the reads' ranges (1, 63, 64 of them) keep rec_rep 0xFFFFFFFF and are never listed; the
    last record sits at the edge of a wave and of a workgroup (slot 254, 255, 256).  Holes at chunk tails: the list's extent exceeds
    the listed problems (witness: figures 'holes'), the likelihood kernels skip them (rep_dv still poisoned there: check).  Each record
    index is listed at most once, and values are written for every listed problem and for nothing else -- not at holes, not behind the
    list, not at places nobody names (check, invariants 2 and 5, as in every test of this module)."""
    t, r, f = env.run(f"holes_{end}")
    assert f["holes"] > 0 and f["problems"] == f["listed"] + f["holes"]


@pytest.mark.parametrize("th", [2, 6])
def test_other_thresholds(env, th):
    """Thresholds 2 and 6: no packed words, no direct part (dd_nodes 0), every record its own problem, nothing flagged."""
    t, r, f = env.run("th_other", th=th, tables=dc.design_th_other(env.lay, th))
    assert r["dd_nodes"] == 0 and f["direct"] == 0 and f["in_table"] == 0 and f["listed"] == f["distinct"] == int(dc.in_read(t)[0].sum())
    assert not (r["rec_rep"][r["rec_rep"] != dc.HOLE] & dc.FLAG).any()


def test_direct_part_off(env):
    """KR_DD_DIRECT=0: the classes design goes through the table -- nothing flagged, every class de-duplicated there -- and every
    record's value is bit-equal to the direct run's."""
    t, r0, f0 = env.run("classes")
    t, r1, f1 = env.run("classes", "direct_off")
    assert not (r1["rec_rep"][r1["rec_rep"] != dc.HOLE] & dc.FLAG).any() and f1["direct"] == 0
    assert f1["in_table"] + f1["absent"] == f0["in_table"] + f0["direct"]
    inr, _ = dc.in_read(t)
    p0, p1 = resolved(t, r0)[inr], resolved(t, r1)[inr]
    assert (dc.bits(r0["rep_dv"][p0]) == dc.bits(r1["rep_dv"][p1])).all()


def test_all_designs_in_one_batch(env):
    """every design, concatenated: 4,000-odd reads, 11,000-odd record slots, the k-mer-count slots decided over all of them"""
    t, r, f = env.run("all")
    assert f["direct"] > 100 and f["in_table"] > 5000


def test_state_between_batches(env):
    """One stream, a large batch and then a small one: the large batch's table entries lie beyond the small batch's mask (witness: read
    back there, non-empty) and must be ignored; the direct places are cleared in full (check: every place nobody names is 0xFFFFFFFF).
    The small batch's direct records name the places of its first run."""
    t, first, _ = env.run("classes")
    env.run("crowded")
    t, again, f = env.run("classes", table_room=8192)
    assert again["mask"] == 1023 and len(again["dd_table"]) == 8192 and (again["dd_table"][1024:, 0] != 0).sum() > 1000
    fl = (first["rec_rep"] != dc.HOLE) & ((first["rec_rep"] & dc.FLAG) != 0)
    assert fl.any() and (again["rec_rep"][fl] == first["rec_rep"][fl]).all() and f["excess"] == 0
    env.run("all")
    env.run("last_place")
    env.run("chain_wrap")


@pytest.mark.parametrize("name,regime", [("classes", "poison"), ("same_word_other_leaf", "poison"), ("crowded", "poison"), ("crowded", "poison_shift8")])
def test_poisoned_buffers(env, name, regime):
    """KR_DEBUG_POISON=all: nothing depends on what a fresh buffer of the stream holds (table, direct places, k-mer-count histogram)"""
    t, r, f = env.run(name, regime)
    if regime == "poison_shift8":
        assert f["absent"] >= f["distinct"] - 1024


def test_ordinary_batches_after_the_debug_entry(env, capi):
    """after kr_debug_dedup an ordinary submit / collect on the same stream gives the rows of a fresh stream"""
    rng = np.random.default_rng(5)
    reads = [b"A" * 150, b"A" * 70 + b"C" + b"A" * 79, bytes(rng.choice(list(b"ACGT"), 150).tolist()), b"A" * 40]
    bases = np.frombuffer(b"".join(reads), np.uint8)
    offs = np.cumsum([0] + [len(x) for x in reads]).astype(np.uint64)
    used = env.stream()
    env.run("classes")
    fresh = env.dx.stream(capi.default_params(hdist_th=4), max_reads=8192, max_bases=1 << 16, max_records=16384)
    rows = []
    for st in (used, fresh):
        st.submit(bases, offs, capi.KR_TAP_ACCS)
        res = st.collect()
        # (the order of the reads' record groups in the arrays may differ from run to run: compared by read and key)
        recs = sorted(zip(res.rec_read.tolist(), res.rec_key.tolist(), res.rec_sel.tolist(), res.rec_d.view(np.uint64).tolist(), res.rec_v.view(np.uint64).tolist()))
        rows.append((res.rows(), recs, res.read_cnt.tolist(), res.read_na.tolist()))
    fresh.close()
    assert rows[0] == rows[1] and len(rows[0][0]) >= 3
