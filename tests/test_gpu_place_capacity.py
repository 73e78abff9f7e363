"""The recovery paths of the `place` back end on the device (kr_host_place.inc, kr_dev_place.inc, kr_place_stream): what runs only
when a device buffer is too small or a number cannot be formatted on the device.

  1  candidate slots run out            -> the range is run again with what it asked for (cnt[0])
  2  kept-candidate slots run out       -> the range is run again (cnt[3])
  3  the internal candidates' list cut  -> kr_place_llh_kernel minimises by itself, no rerun, the same bits
  4  still out of slots after 2 reruns  -> the whole batch goes to the host back end
  5  the text outgrows its buffer       -> the host formats the range, the next batch gets the room
  6  the text raises a flag             -> the host formats the range

Every workspace has a floor far above what a test-size batch needs, so each test (i) runs its input once with no knob and reads
what it asked for from `capi.place_path_counters()`, (ii) sets KR_DEBUG_PLACE_CAPS from that, (iii) asserts by counter that the
intended path ran, and how often -- a test whose path did not run FAILS --, (iv) compares the output byte for byte with the host
back end (`Placer.place(host=True)`: text, `placements.tobytes()`, summary) and with the oracle (`pyoracle.Index.place`: text byte
for byte, the set of (read, edge) placements; `place_summarize` for the summary), and (v) asserts the device / host batch counts.
No tolerance anywhere.

Inputs: the golden 25-leaf index with its 308 reads and 5,000 sampled reads; a batch whose first reads match nothing, so that the
first of its ranges asks for a fraction of what the later ones do; a 34-leaf index of near-identical genomes for reads that keep
more than 64 candidates.

Text flags.  Flag 1 (a magnitude of 1000 or more) is driven by a user tree with a branch of length 2500 (the distal length is half
the branch).  Flag 4 ("more than 64 candidates kept in a read") is not raised by any kernel any more -- a read's kept candidates
are sorted and formatted 64 at a time -- so its test asserts that such reads ARE formatted on the device, and equal the host's
bytes.  Flag 8 (a number that went through exp or log within 1e-8 of a rounding tie of its fifth decimal) has no constructive
input: the oracle's placements of three 5,000-read samples of the toy genomes (seeds 23, 29, 31: 25,855 placements, pendant
length and LWR of each) come no closer to a tie than 1.09e-5, so no input is pinned here, and the window is not widened.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

USER_OLD = "(G000735195:0.0276038,G000018865:0.0228997)N2640:0.160977"
USER_NEW = "(G000735195:0.03,NEWLEAF:0.02)N2640:0.160977"
MOVING = ("reruns_cand", "reruns_keep", "list_cut", "given_up", "text_flag_1", "text_flag_2", "text_flag_4", "text_flag_8", "text_flag_16")


def tree_kw(tree):
    if tree == "user":
        nwk = open(os.path.join(GOLDEN, "tree_toy.nwk")).read()
        assert USER_OLD in nwk
        return dict(nwk_text=nwk.replace(USER_OLD, USER_NEW))
    if tree == "lineages":
        return dict(lineage_text=open(os.path.join(GOLDEN, "lineages_toy.txt")).read())
    return dict()


class Bench:
    """One index + the references of every (input, tree, mode, options) asked for, computed once."""

    def __init__(self, capi, po, index_dir):
        self.capi, self.po, self.index_dir = capi, po, index_dir
        self.hx = capi.HostIndex(index_dir)
        self.inputs = {}
        self.refs = {}

    def placer(self, inp, tabular, tree="backbone", **opts):
        b, o, n = self.inputs[inp]
        kw = tree_kw(tree) if isinstance(tree, str) else dict(tree)
        no_filter = opts.pop("no_filter", 0)
        pl = self.capi.Placer(self.hx, kw.get("nwk_text"), 0, tabular=tabular, max_reads=len(n), max_bases=len(b), lineage_text=kw.get("lineage_text"), **opts)
        pl.popts.no_filter = no_filter
        return pl

    def place(self, pl, inp, want_pl, host=False):
        b, o, n = self.inputs[inp]
        text, p = pl.place(b, o, n, host=host, want_placements=want_pl)
        return (text, p.tobytes() if want_pl else b"", pl.summary() if int(pl.tabular) == 2 and want_pl else "")

    def reference(self, inp, tabular, want_pl, tree="backbone", **opts):
        """(host back end's output, oracle's text or summary, oracle's sorted (read, edge)) for one call on a new Placer."""
        key = (inp, tabular, want_pl, str(tree), tuple(sorted(opts.items())))
        if key not in self.refs:
            pl = self.placer(inp, tabular, tree, **opts)
            host = self.place(pl, inp, want_pl, host=True)
            pl.close()
            b, o, n = self.inputs[inp]
            ox = self.po.Index(self.index_dir)
            kw = tree_kw(tree) if isinstance(tree, str) else dict(tree)
            if "lineage_text" in kw:
                ox.set_lineage_tree(kw["lineage_text"])
            else:
                ox.set_placement_tree(kw.get("nwk_text"))
            okw = dict(no_filter=0)
            okw.update(opts)
            if tabular == 2:
                otext, okeys = ox.place_summarize(b, o, self.po.params(**okw)), None
            else:
                r = ox.place(b, o, n, self.po.params(**okw), tabular=bool(tabular))
                otext = r["text"]
                okeys = sorted((int(a), int(e)) for a, e in zip(r["placements"]["read"], r["placements"]["edge"]))
            ox.close()
            self.refs[key] = (host, otext, okeys)
        return self.refs[key]

    def check(self, got, inp, tabular, want_pl, tree="backbone", **opts):
        host, otext, okeys = self.reference(inp, tabular, want_pl, tree, **opts)
        assert got == host, "differs from the host back end"
        assert len(host[0]) + len(host[1]) > 0
        assert (got[2] if tabular == 2 else got[0]) == otext, "differs from the oracle"
        if want_pl and okeys is not None:
            p = np.frombuffer(got[1], dtype=self.capi.PLACEMENT_DT)
            assert sorted((int(a), int(e)) for a, e in zip(p["read"], p["edge"])) == okeys


@pytest.fixture(scope="module")
def bench(capi, po, synth, toy_index_dir, toy_reads, toy_genomes):
    bn = Bench(capi, po, toy_index_dir)
    names, bases, offs = toy_reads
    bn.inputs["toy"] = (bases, offs, names)
    bn.inputs["sample"] = synth.sample_reads(toy_genomes, 5000, seed=37)
    # 1,200 reads whose first range -- of 3 (400 reads) or of 16 (75 reads) -- holds 8 reads of the genomes and otherwise reads that
    # match nothing: that range asks for a fraction of the candidate slots the later ones do
    real = synth.sample_reads(toy_genomes, 1200, seed=41, mix=[(1.0, 0.01)])[0].reshape(1200, 150)
    junk = synth.sample_reads(toy_genomes, 1200, seed=43, mix=[(1.0, None)])[0].reshape(1200, 150)
    for nr in (3, 16):
        first = 1200 // nr
        rows = real.copy()
        rows[8:first] = junk[8:first]

        def part(r0, r1):
            return (np.ascontiguousarray(rows[r0:r1]).reshape(-1), np.arange(r1 - r0 + 1, dtype=np.uint64) * np.uint64(150), [f"m{r}" for r in range(r0, r1)])

        bn.inputs[f"mixed{nr}"], bn.inputs[f"mixed{nr}/first"], bn.inputs[f"mixed{nr}/second"] = part(0, 1200), part(0, first), part(first, 2 * first)
    return bn


def moved(c0, c1):
    return {k: c1[k] - c0[k] for k in MOVING if c1[k] != c0[k]}


def uncapped(bench, inp, tabular, want_pl, tree="backbone", **opts):
    """(i): the input on a new Placer with no knob; no recovery path may run; returns what its (last) range asked for."""
    assert "KR_DEBUG_PLACE_CAPS" not in os.environ
    c0, b0 = bench.capi.place_path_counters(), bench.capi.place_counters()
    pl = bench.placer(inp, tabular, tree, **opts)
    got = bench.place(pl, inp, want_pl)
    pl.close()
    c1, b1 = bench.capi.place_path_counters(), bench.capi.place_counters()
    assert moved(c0, c1) == {} and (b1[0] - b0[0], b1[1] - b0[1]) == (1, 0) and c1["attempts"] == 1
    bench.check(got, inp, tabular, want_pl, tree, **opts)
    return c1, got


def capped(bench, monkeypatch, caps, inp, tabular, want_pl, tree="backbone", **opts):
    """(ii): the same under KR_DEBUG_PLACE_CAPS; returns (output, what the path counters moved by, the last range's values, batches)."""
    if caps:
        monkeypatch.setenv("KR_DEBUG_PLACE_CAPS", caps)
    c0, b0, t0 = bench.capi.place_path_counters(), bench.capi.place_counters(), bench.capi.place_text_counters()
    pl = bench.placer(inp, tabular, tree, **opts)
    got = bench.place(pl, inp, want_pl)
    pl.close()
    c1, b1, t1 = bench.capi.place_path_counters(), bench.capi.place_counters(), bench.capi.place_text_counters()
    if caps:
        monkeypatch.delenv("KR_DEBUG_PLACE_CAPS")
    return got, moved(c0, c1), c1, (b1[0] - b0[0], b1[1] - b0[1]), (t1[0] - t0[0], t1[1] - t0[1])


MODES = {"jplace+records": (0, True), "tabular+records": (1, True), "summary": (2, True), "jplace/device-text": (0, False), "tabular/device-text": (1, False)}


@pytest.mark.parametrize("inp,mode,tree,env", [
    ("toy", "jplace+records", "backbone", {}), ("toy", "tabular+records", "backbone", {}), ("toy", "summary", "backbone", {}),
    ("toy", "jplace/device-text", "backbone", {}), ("toy", "tabular/device-text", "backbone", {}),
    ("sample", "jplace+records", "backbone", {}), ("sample", "summary", "backbone", {}), ("sample", "jplace/device-text", "backbone", {}),
    ("sample", "tabular/device-text", "backbone", {}),
    ("sample", "jplace+records", "user", {}), ("sample", "jplace/device-text", "lineages", {}),
    ("sample", "jplace+records", "backbone", {"KR_DEBUG_PLACE_LDS": "3,8"}), ("sample", "tabular/device-text", "backbone", {"KR_DEBUG_PLACE_LDS": "3,8"}),
    ("sample", "jplace+records", "backbone", {"KR_DEBUG_PLACE_LDS": "3,8", "KR_PLACE_BIG_FIRST": "0"}),
    ("sample", "jplace+records", "backbone", {"KR_DEBUG_PLACE_LDS": "3,8", "KR_PLACE_HEAVY_GLOBAL": "1"}),
    ("sample", "jplace+records", "backbone", {"KR_DEBUG_POISON": "all"}), ("sample", "jplace/device-text", "backbone", {"KR_DEBUG_POISON": "all"}),
])
def test_candidate_slots_run_out_and_the_range_is_run_again(bench, monkeypatch, inp, mode, tree, env):
    """Path 1.  Half the candidate slots the uncapped run asked for: place_read raises bit 2 of cnt[1] (kr_dev_place.inc, both places),
    place_device_finish sizes the arrays from cnt[0] and launches the range again -- once --, the batch stays on the device and its
    output is the uncapped run's.  Every output mode, records wanted and text written on the device (whose kernels find a flagged
    range and format nothing of it), the user tree and the lineage tree; with the LDS limits lowered, where heavy reads take their slots
    in the kernel's own global scratch or through the list and the second launch (in LDS or, forced, global scratch); and with
    every new buffer -- the place workspaces included -- filled with 0xA5, so that a slot the rerun leaves stale shows."""
    tabular, want_pl = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want, _ = uncapped(bench, inp, tabular, want_pl, tree)
    assert want["cnt0"] >= 256 and want["cand_cap"] >= want["cnt0"]
    got, mv, last, batches, texts = capped(bench, monkeypatch, f"c={want['cnt0'] // 2}", inp, tabular, want_pl, tree)
    assert mv == {"reruns_cand": 1}, mv
    assert last["attempts"] == 2 and last["flags"] & ~8 == 0 and last["cand_cap"] >= last["cnt0"] > want["cnt0"] // 2
    assert batches == (1, 0), "the batch left the device"
    assert texts == ((0, 0) if want_pl else (1, 0))
    bench.check(got, inp, tabular, want_pl, tree)


@pytest.mark.parametrize("inp,mode,tree,opts,env", [
    ("toy", "jplace/device-text", "backbone", {}, {}), ("toy", "tabular/device-text", "backbone", {}, {}), ("toy", "jplace+records", "backbone", {}, {}),
    ("sample", "jplace/device-text", "backbone", {}, {}), ("sample", "tabular/device-text", "backbone", {}, {}),
    ("sample", "jplace+records", "backbone", {}, {}), ("sample", "summary", "backbone", {}, {}),
    ("sample", "jplace/device-text", "backbone", {"multi": 0}, {}), ("sample", "tabular+records", "backbone", {"multi": 0}, {}),
    ("sample", "jplace/device-text", "user", {}, {}), ("sample", "jplace+records", "lineages", {}, {}),
    ("sample", "jplace/device-text", "backbone", {}, {"KR_DEBUG_POISON": "all"}), ("sample", "jplace+records", "backbone", {}, {"KR_DEBUG_POISON": "all"}),
])
def test_kept_slots_run_out_and_the_range_is_run_again(bench, monkeypatch, inp, mode, tree, opts, env):
    """Path 2.  Candidate slots as ever, half the kept-candidate slots the uncapped run's compaction handed out (cnt[3]):
    kr_place_compact_kernel raises bit 4 and skips the reads it has no slots for, the range is run again -- once -- with
    keep_want_min taken from cnt[3].  With the text written on the device this is the attempt whose skipped reads still name slots
    of the c_* arrays: the text kernels must not follow them (kr_place_text_len_kernel's guard, place_read_prepare's bound), and
    the rerun's text is the host's byte for byte.  Also with records wanted, --no-multi, the other trees, and poisoned buffers."""
    tabular, want_pl = MODES[mode]
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    want, _ = uncapped(bench, inp, tabular, want_pl, tree, **opts)
    assert want["cnt3"] >= 512 and want["keep_cap"] >= want["cnt3"]
    got, mv, last, batches, texts = capped(bench, monkeypatch, f"k={want['cnt3'] // 2}", inp, tabular, want_pl, tree, **opts)
    assert mv == {"reruns_keep": 1}, mv
    assert last["attempts"] == 2 and last["flags"] == 0 and last["cnt3"] == want["cnt3"] and last["keep_cap"] >= want["cnt3"]
    assert batches == (1, 0), "the batch left the device"
    assert texts == ((0, 0) if want_pl else (1, 0)) and last["text_flags"] == 0
    bench.check(got, inp, tabular, want_pl, tree, **opts)


@pytest.mark.parametrize("inp,opts", [("toy", {}), ("sample", {}), ("sample", {"no_filter": 1}), ("sample", {"tau": 1, "chisq": 3.841})])
def test_a_cut_list_of_internal_candidates_changes_no_bit(bench, monkeypatch, inp, opts):
    """Path 3.  The slots of the internal candidates are listed for kr_place_brent_kernel in the kept-candidate arrays (k_se, until the
    compaction takes them over), in chunks of 128 per wave of kr_place_kernel (cnt[12]).  On the 308 reads that list is SHORTER than
    what the compaction hands out (cnt[3]: chunks of 256 for each of its 64 waves), so no kept cap cuts the one and not the other:
    the knob's fourth field gives the list half the entries it asked for.  Bit 8 alone, no rerun, kr_place_brent_kernel returns and
    kr_place_llh_kernel runs every minimisation itself -- d_llh, v_llh and the LWR (from the chi-square) of every placement are the
    bits of the uncapped run and of the host back end."""
    want, base = uncapped(bench, inp, 0, True, **opts)
    assert want["cnt12"] >= 256
    cap = want["cnt12"] // 2
    got, mv, last, batches, _ = capped(bench, monkeypatch, f"l={cap}", inp, 0, True, **opts)
    assert mv == {"list_cut": 1}, mv
    assert last["attempts"] == 1 and last["flags"] == 8 and last["cnt12"] > cap and last["keep_cap"] == want["keep_cap"] >= last["cnt3"] == want["cnt3"]
    assert batches == (1, 0)
    assert got == base, "differs from the uncapped run"
    p = np.frombuffer(got[1], dtype=bench.capi.PLACEMENT_DT)
    assert len(p) > 300 and len(np.unique(p["read"])) < len(p)  # (reads with several placements: internal candidates among them)
    bench.check(got, inp, 0, True, **opts)


@pytest.mark.parametrize("mode", ["jplace+records", "summary", "jplace/device-text", "tabular/device-text"])
def test_a_range_that_stays_out_of_slots_sends_the_batch_to_the_host(bench, monkeypatch, mode):
    """Path 4.  Three ranges and candidate slots that stay as they are ("sticky"): enough for the first range, whose reads mostly match
    nothing, and half of what the second asks for.  The first range is finished and its piece taken; the second is still flagged after
    two reruns, kr_place_stream drops the pieces and hands the whole batch to the host back end (place_counters: (0, 1)); the output
    is that back end's.  With the text written on the device, the range given up is one whose text kernels formatted nothing
    (flag 16, 0 bytes).  The next call on the same Placer, without knobs, stays on the device."""
    tabular, want_pl = MODES[mode]
    monkeypatch.setenv("KR_PLACE_RANGES", "1")
    first, _ = uncapped(bench, "mixed3/first", tabular, want_pl)
    second, _ = uncapped(bench, "mixed3/second", tabular, want_pl)
    cap = second["cnt0"] // 2
    assert 0 < 2 * first["cnt0"] <= cap, (first["cnt0"], second["cnt0"])
    monkeypatch.setenv("KR_PLACE_RANGES", "3")
    monkeypatch.setenv("KR_DEBUG_PLACE_CAPS", f"c={cap},sticky")
    capi = bench.capi
    c0, b0, t0 = capi.place_path_counters(), capi.place_counters(), capi.place_text_counters()
    pl = bench.placer("mixed3", tabular)
    got = bench.place(pl, "mixed3", want_pl)
    c1, b1, t1 = capi.place_path_counters(), capi.place_counters(), capi.place_text_counters()
    assert moved(c0, c1) == {"reruns_cand": 2, "given_up": 1}, moved(c0, c1)
    assert c1["ranges"] - c0["ranges"] == 2 and c1["attempts"] == 3 and c1["flags"] & 2 and c1["cand_cap"] == cap
    assert (b1[0] - b0[0], b1[1] - b0[1]) == (0, 1)
    assert (t1[0] - t0[0], t1[1] - t0[1]) == ((0, 0) if want_pl else (1, 0))  # (the first range's text was taken, then dropped)
    if not want_pl:
        assert c1["text_flags"] & 16 and c1["text_bytes"] == 0
    bench.check(got, "mixed3", tabular, want_pl)
    monkeypatch.delenv("KR_DEBUG_PLACE_CAPS")
    monkeypatch.delenv("KR_PLACE_RANGES")
    again = bench.place(pl, "mixed3", want_pl)  # (a second call: jplace text begins with the separator, the summary has grown)
    c2, b2 = capi.place_path_counters(), capi.place_counters()
    pl.close()
    assert moved(c1, c2) == {} and (b2[0] - b1[0], b2[1] - b1[1]) == (1, 0) and c2["attempts"] == 1
    if tabular == 0:
        assert again[0] == ",\n" + got[0] and again[1] == got[1]
    elif tabular == 1:
        assert again[:2] == got[:2]


@pytest.mark.parametrize("ranges", [3, 16])
@pytest.mark.parametrize("mode", ["jplace+records", "summary", "jplace/device-text"])
def test_a_later_range_is_run_again_behind_the_earlier_ranges_candidates(bench, monkeypatch, ranges, mode):
    """Ranges x rerun.  The first range fits the capped candidate slots and leaves its kept candidates in the host arrays; later ranges
    run out and are run again, and their candidates go behind (`kept_base`, the shift of rd_c0, the renewal of the page-locked
    arrays) -- or, with device text, their rows behind the first range's.  Same output as the host back end and the oracle."""
    tabular, want_pl = MODES[mode]
    inp = f"mixed{ranges}"
    monkeypatch.setenv("KR_PLACE_RANGES", "1")
    first, _ = uncapped(bench, inp + "/first", tabular, want_pl)
    second, _ = uncapped(bench, inp + "/second", tabular, want_pl)
    cap = second["cnt0"] // 2
    assert 0 < 2 * first["cnt0"] <= cap, (first["cnt0"], second["cnt0"])
    monkeypatch.setenv("KR_PLACE_RANGES", str(ranges))
    got, mv, last, batches, texts = capped(bench, monkeypatch, f"c={cap}", inp, tabular, want_pl)
    assert set(mv) == {"reruns_cand"} and 1 <= mv["reruns_cand"] <= ranges - 1, mv
    assert batches == (1, 0) and texts == ((0, 0) if want_pl else (ranges, 0))
    bench.check(got, inp, tabular, want_pl)


@pytest.mark.parametrize("tabular", [0, 1])
def test_text_that_outgrows_its_buffer_is_formatted_by_the_host(bench, monkeypatch, tabular):
    """Path 5.  A text buffer of half the bytes the uncapped run wrote: the range comes back as candidates with flag 2, the host formats
    it, and `text_want_min` gives the NEXT batch on the Placer the room -- with the knob still set (nothing else can have enlarged the
    buffer) and with it removed.  Two Placers, so that the jplace separator crosses a host-formatted piece and a device-written one
    in both orders; every call's bytes are the host back end's for the same sequence of calls."""
    capi = bench.capi
    want, _ = uncapped(bench, "sample", tabular, False)
    small, _ = uncapped(bench, "toy", tabular, False)
    assert want["text_bytes"] > 2 * small["text_bytes"] > 0 and want["text_cap"] >= want["text_bytes"]
    knob = f"t={want['text_bytes'] // 2}"

    def calls(seq, host):
        pl = bench.placer("sample", tabular)
        out = []
        for inp, caps in seq:
            if caps and not host:
                monkeypatch.setenv("KR_DEBUG_PLACE_CAPS", caps)
            c0, t0 = capi.place_path_counters(), capi.place_text_counters()
            b, o, n = bench.inputs[inp]
            text = pl.place(b, o, n, host=host, want_placements=host)[0]
            c1, t1 = capi.place_path_counters(), capi.place_text_counters()
            out.append((text, moved(c0, c1), (t1[0] - t0[0], t1[1] - t0[1]), c1))
            if caps and not host:
                monkeypatch.delenv("KR_DEBUG_PLACE_CAPS")
        pl.close()
        return out

    # host piece, then device pieces: the large batch under the knob, the small one under the knob, the large one without
    seq = [("sample", knob), ("toy", knob), ("sample", None)]
    ref = [t for t, _, _, _ in calls(seq, True)]
    got = calls(seq, False)
    assert [g[0] for g in got] == ref
    assert got[0][1] == {"text_flag_2": 1} and got[0][2] == (0, 1) and got[0][3]["text_bytes"] == want["text_bytes"] > got[0][3]["text_cap"]
    assert got[1][1] == {} and got[1][2] == (1, 0), "text_want_min gave the next batch no room"
    assert got[1][3]["text_cap"] >= want["text_bytes"] and got[1][3]["text_bytes"] == small["text_bytes"]
    assert got[2][1] == {} and got[2][2] == (1, 0)
    if tabular == 0:
        assert not ref[0].startswith(",\n") and ref[1].startswith(",\n") and ref[2].startswith(",\n")
    # device piece, then a host piece
    seq = [("toy", None), ("sample", knob)]
    ref = [t for t, _, _, _ in calls(seq, True)]
    got = calls(seq, False)
    assert [g[0] for g in got] == ref
    assert got[0][1] == {} and got[0][2] == (1, 0)
    assert got[1][1] == {"text_flag_2": 1} and got[1][2] == (0, 1)


def test_a_number_of_1000_or_more_is_formatted_by_the_host(bench, monkeypatch):
    """Path 6, flag 1.  A user tree whose branch above a leaf that receives placements is 2500 long: the distal length (half the
    branch) and the pendant length (less half the branch) of every placement there have four digits in front of the point, which
    the device's "%.5f" does not write.  jplace: the range is counted under flag 1 and its bytes are the host's and the oracle's;
    tabular rows carry neither number and are written on the device."""
    nwk = open(os.path.join(GOLDEN, "tree_toy.nwk")).read()
    assert "G000018865:0.0228997" in nwk
    tree = dict(nwk_text=nwk.replace("G000018865:0.0228997", "G000018865:2500.0"))
    host, otext, _ = bench.reference("sample", 0, False, tree)
    assert ", 1250.00000, " in otext and ", -1249." in otext, "no placement on the long branch"
    for tabular, want_mv, want_t in ((0, {"text_flag_1": 1}, (0, 1)), (1, {}, (1, 0))):
        got, mv, last, batches, texts = capped(bench, monkeypatch, None, "sample", tabular, False, tree)
        assert mv == want_mv and texts == want_t and batches == (1, 0), (tabular, mv, texts)
        assert last["text_flags"] == (1 if tabular == 0 else 0)
        bench.check(got, "sample", tabular, False, tree)


def test_reads_that_keep_more_than_64_candidates_are_formatted_on_the_device(capi, po, synth, tmp_path, monkeypatch):
    """Path 6, flag 4 -- which no kernel raises any more: place_read_prepare sorts a read's kept candidates 64 of its own against all
    of them at a time, and the rows are made tile by tile.  34 near-identical genomes (a tree of 67 nodes, the fewest leaves whose
    tree has more than 64 nodes below the root): without the filter and with a chi-square bound nothing fails, most reads keep 65
    or 66 candidates (checked with the oracle on the CPU first).  The device writes their rows -- no fallback, nothing counted
    under flag 4 -- byte for byte as the host and the oracle do, --no-multi included."""
    n = 34
    nwk = synth.yule_newick(n, 9, mean_blen=0.0003)
    g = synth.evolve_genomes(nwk, 3000, seed=5)
    tsv = synth.write_genomes(g, str(tmp_path / "g"))
    (tmp_path / "t.nwk").write_text(nwk)
    idx = str(tmp_path / "ix")
    capi.build_index(tsv, idx, nwk=str(tmp_path / "t.nwk"), k=21, w=27, h=7, m=4, r=1, frac=True, num_threads=4)
    bn = Bench(capi, po, idx)
    bn.inputs["near"] = synth.sample_reads(g, 200, seed=3)
    ox = po.Index(idx)
    ox.set_placement_tree(None)
    kept = np.bincount(ox.place(*bn.inputs["near"][:2], bn.inputs["near"][2], po.params(no_filter=1, chisq=1e9))["placements"]["read"])
    ox.close()
    assert (kept > 64).sum() >= 50 and kept.max() <= 2 * n - 2
    for tabular in (0, 1):
        for opts in (dict(no_filter=1, chisq=1e9), dict(no_filter=1, chisq=1e9, multi=0)):
            got, mv, last, batches, texts = capped(bn, monkeypatch, None, "near", tabular, False, **opts)
            assert mv == {} and texts == (1, 0) and batches == (1, 0) and last["text_flags"] == 0
            bn.check(got, "near", tabular, False, **opts)
            rec, _, _, _, _ = capped(bn, monkeypatch, None, "near", tabular, True, **opts)
            bn.check(rec, "near", tabular, True, **opts)
