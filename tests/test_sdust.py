"""--sdust-t/-w on the CPU: the host masker against recorded output of the reference's sdust() (tests/golden/sdust_ref.json), the
masked leaf stage against a literal pure-Python walk of src/rqseq.cpp:71-140 fed the FIXTURE's intervals, and the options
through capi and the CLI."""
import os
import subprocess

import numpy as np
import pytest

from sdust_cases import FIXTURE, OUT_OF_ORDER, PARAMS, SEQS, fixture_lists, fuzz_sequence, hll12, implant, masked_ring_buffer_sim, pack

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
NAMES = list(SEQS)
PPOS = [20, 19, 17, 13, 6, 4, 2]
NPOS = [p for p in range(21) if p not in PPOS]


@pytest.fixture(scope="module")
def fuzz():
    return fuzz_sequence()


def test_fixture_lists_are_sorted_with_gaps():
    """What "the runs of the mask's bits are the list" rests on: every recorded list is sorted, its intervals are not empty and
    at least one base apart.  (They may reach past the contig's end behind an N: the reference's stale window.)"""
    covering_n = past_end = 0
    for key, per_seq in FIXTURE["intervals"].items():
        W = int(key.split(",")[1])
        for name, ivs in per_seq.items():
            s = SEQS[name]
            for j, (a, b) in enumerate(ivs):
                assert 0 <= a < b <= len(s) + W, (key, name, a, b)
                if j:
                    assert a > ivs[j - 1][1], (key, name, ivs[j - 1], (a, b))
                covering_n += any(c in b"NnRYKMSW" for c in s[a:b])
                past_end += b > len(s)
    assert covering_n >= 5 and past_end >= 1  # the stale-window cases are in the file


@pytest.mark.parametrize("T,W", PARAMS)
def test_host_masker_equals_reference_lists(capi, T, W):
    bases, offs = pack([SEQS[n] for n in NAMES])
    assert capi.sdust(bases, offs, T, W) == fixture_lists(T, W, NAMES)
    for call in FIXTURE["calls"]:  # the same sequence twice in one call: no state across contigs
        bases, offs = pack([SEQS[n] for n in call])
        assert capi.sdust(bases, offs, T, W) == fixture_lists(T, W, call)


def test_alphabets_differ_where_the_fixture_says(capi):
    """Bytes 1..3 are bases for sdust (masked as a homopolymer) and no bases for the minimizers."""
    s = SEQS["bytes_1_2_3"]
    p = s.index(b"\x01" * 50)
    assert any(a <= p + 10 and b >= p + 40 for a, b in fixture_lists(20, 64, ["bytes_1_2_3"])[0])
    u = s.index(b"U" * 40)
    assert not any(a <= u + 5 and b >= u + 35 for a, b in fixture_lists(20, 64, ["bytes_1_2_3"])[0])


def test_masker_limits(capi):
    bases, offs = pack([b"ACGT" * 10])
    for T, W in ((20, 3), (0, 64)):
        with pytest.raises(capi.KrError):
            capi.sdust(bases, offs, T, W)
    small = pack([b"A" * 40 + b"ACGT" * 10])  # the smallest W (recorded from the reference: nothing at T 20, 0-41 at T 2)
    assert capi.sdust(*small, 20, 4) == [[]] and capi.sdust(*small, 2, 4) == [[(0, 41)]] and capi.sdust(*small, 1, 5) == [[(0, 41)]]
    assert capi.sdust(*pack([b"A" * 300]), 1000, 500) == [[(0, 300)]]  # host path: any W (what the reference gives for it)


def test_host_masker_on_the_fuzz_is_a_sorted_list_and_contigs_are_independent(capi, fuzz):
    """200 kb with implanted stretches, sparse N and long N runs: the list stays sorted with gaps, and a contig's list does not
    depend on what else is in the call."""
    piece = fuzz[30_000:90_000]
    alone = capi.sdust(*pack([piece]), 20, 64)[0]
    both = capi.sdust(*pack([fuzz, piece, SEQS["homopolymer"]]), 20, 64)
    assert both[1] == alone and both[2] == fixture_lists(20, 64, ["homopolymer"])[0]
    assert len(both[0]) > 250 and sum(b - a for a, b in both[0]) > 20_000
    assert all(a < b for a, b in both[0]) and all(both[0][j][0] > both[0][j - 1][1] for j in range(1, len(both[0])))


def test_list_is_not_the_union_of_saved_intervals_behind_two_close_n(capi):
    """Two non-bases within W bases of a homopolymer: the reference's merge keeps the start of an interval that was flushed early
    and drops the bases of the run in front of it.  The host masker does the same (fixture), it does not mask the whole run."""
    for name in OUT_OF_ORDER:
        s = SEQS[name]
        got = capi.sdust(*pack([s]), 20, 64)
        assert got == fixture_lists(20, 64, [name])
        run = s.index(b"G" * 40)
        assert got[0][0][0] > run + 30  # the G run starts well in front of the one interval


LEAF_CONTIGS = ["two_N_within_W", "interval_near_start", "two_intervals_closer_than_k", "interval_N_tail", "N300_between", "N300_short_sides",
                "ends_inside_interval", "final_run_18", "final_run_21", "final_run_23", "final_run_25", "final_run_27",
                "final_run_29", "final_run_33", "cut_by_one_N", "iupac", "lower_case", "bytes_1_2_3", "periods_2_to_7",
                "straddles_chunk", "random", "polyA_len_65", "polyA_len_31"]


@pytest.mark.parametrize("k,w,h", [(21, 27, 7), (21, 21, 7), (21, 60, 7)])
@pytest.mark.parametrize("T,W", [(20, 64), (10, 16)])
def test_masked_cpu_leaf_stage_matches_literal_walk(capi, k, w, h, T, W):
    contigs = [SEQS[n] for n in LEAF_CONTIGS]
    ivs = fixture_lists(T, W, LEAF_CONTIGS)  # the reference's intervals, not the product's
    bases, offs = pack(contigs)
    keys, n1, n2 = capi.minimizers(bases, offs, k, w, h, PPOS, sdust_t=T, sdust_w=W)
    kept = [(c.decode("latin-1"), iv) for c, iv in zip(contigs, ivs)]
    want, sk, seen = masked_ring_buffer_sim([c for c, _ in kept], [iv for _, iv in kept], k, w, 4, 1, True, PPOS, NPOS)
    assert keys.tolist() == want.tolist() and len(want) > 100
    assert n1 == sum(hll12(a) for a, _ in sk) and n2 == sum(hll12(b) for _, b in sk)
    plain = capi.minimizers(bases, offs, k, w, h, PPOS)
    assert plain[0].tolist() != keys.tolist()
    # the walk met the cases the contigs were made for
    by_name = dict(zip([n for n in LEAF_CONTIGS if len(SEQS[n]) >= w], seen))
    assert by_name["interval_near_start"]["passed"] >= 1 and by_name["two_intervals_closer_than_k"]["passed"] >= 3
    assert by_name["interval_N_tail"]["skipped"] > 0 and by_name["N300_between"]["passed"] >= 2
    if (T, W) == (20, 64):
        assert any(s["ended_skipping"] for s in seen)  # (an interval that reaches past the contig's end)
        if w > k:
            assert any(by_name["final_run_%d" % t]["short_final_emit"] for t in (18, 21, 23, 25, 27, 29, 33))


def _genomes(synth, n=40_000, seed=4):
    g = synth.evolve_genomes("((a:0.03,b:0.03):0.02,c:0.05);", n, seed=seed)
    rng = np.random.default_rng(seed)
    out = {}
    for name, seq in g.items():
        codes = np.searchsorted(np.frombuffer(b"ACGT", np.uint8), seq)
        implant(rng, codes, 30)
        out[name] = np.frombuffer(b"ACGT", np.uint8)[codes]
    return out


def _read(d, names):
    return {f: open(os.path.join(d, f), "rb").read() for f in names}


INDEX_FILES = ["%s-m4r1-frac" % f for f in ("cmer", "inc", "crecord", "metadata", "reflist")]


def test_either_value_zero_is_the_unmasked_build(capi, synth, tmp_path):
    g = _genomes(synth)
    tsv = synth.write_genomes(g, str(tmp_path / "g"), contigs=2)
    fa = str(tmp_path / "g" / "a.fna")
    kw = dict(k=21, w=27, h=7, m=4, r=1, frac=True, seed=3)
    capi.build_index(tsv, str(tmp_path / "i0"), **kw)
    capi.build_sketch(fa, str(tmp_path / "s0"), **kw)
    for j, (t, w_) in enumerate(((0, 64), (20, 0), (0, 0))):
        capi.build_index(tsv, str(tmp_path / f"i{j + 1}"), sdust_t=t, sdust_w=w_, **kw)
        capi.build_sketch(fa, str(tmp_path / f"s{j + 1}"), sdust_t=t, sdust_w=w_, **kw)
        assert _read(str(tmp_path / f"i{j + 1}"), INDEX_FILES + ["metadata-m4r1-frac.txt"]) == _read(str(tmp_path / "i0"), INDEX_FILES + ["metadata-m4r1-frac.txt"])
        assert open(tmp_path / f"s{j + 1}", "rb").read() == open(tmp_path / "s0", "rb").read()
    capi.build_index(tsv, str(tmp_path / "im"), sdust_t=20, sdust_w=64, **kw)
    assert _read(str(tmp_path / "im"), INDEX_FILES)["cmer-m4r1-frac"] != _read(str(tmp_path / "i0"), INDEX_FILES)["cmer-m4r1-frac"]
    with pytest.raises(capi.KrError):
        capi.build_index(tsv, str(tmp_path / "bad"), sdust_t=20, sdust_w=3, **kw)


def test_cli_builds_masked_sketch_and_index(capi, synth, tmp_path):
    g = _genomes(synth)
    tsv = synth.write_genomes(g, str(tmp_path / "g"), contigs=2)
    fa = str(tmp_path / "g" / "a.fna")
    two = ["Setting --sdust-w and --sdust-t to >0 will enable dustmasker.",
           "With dustmasker, krepp might fail to model subsampling and be slightly inaccurate."]
    # sketch
    r = subprocess.run([EXE, "sketch", "-i", fa, "-o", str(tmp_path / "s_cli"), "-k", "24", "--seed", "5", "--sdust-t", "20", "--sdust-w", "64"],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lines = r.stderr.splitlines()
    assert two[0] in lines and lines[lines.index(two[0]) + 1] == two[1]
    capi.build_sketch(fa, str(tmp_path / "s_api"), k=24, seed=5, sdust_t=20, sdust_w=64)
    capi.build_sketch(fa, str(tmp_path / "s_plain"), k=24, seed=5)
    assert open(tmp_path / "s_cli", "rb").read() == open(tmp_path / "s_api", "rb").read() != open(tmp_path / "s_plain", "rb").read()
    # index
    r = subprocess.run([EXE, "index", "-i", tsv, "-o", str(tmp_path / "i_cli"), "-k", "21", "-w", "27", "-h", "7", "--seed", "3",
                        "--sdust-t", "20", "--sdust-w", "64"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    assert two[0] in r.stderr.splitlines() and two[1] in r.stderr.splitlines()
    kw = dict(k=21, w=27, h=7, m=4, r=1, frac=True, seed=3)
    capi.build_index(tsv, str(tmp_path / "i_api"), sdust_t=20, sdust_w=64, **kw)
    capi.build_index(tsv, str(tmp_path / "i_plain"), **kw)
    cli, api, plain = (_read(str(tmp_path / d), INDEX_FILES) for d in ("i_cli", "i_api", "i_plain"))
    assert cli == api and cli["cmer-m4r1-frac"] != plain["cmer-m4r1-frac"]
    txt = open(tmp_path / "i_cli" / "metadata-m4r1-frac.txt").read()
    assert "sdust-t: 20\nsdust-w: 64\n" in txt and "sdust" not in open(tmp_path / "i_plain" / "metadata-m4r1-frac.txt").read()
    # an unmasked CLI build prints neither line; a malformed value is refused
    r = subprocess.run([EXE, "sketch", "-i", fa, "-o", str(tmp_path / "s_cli0"), "-k", "24", "--seed", "5", "--sdust-t", "20"], capture_output=True, text=True)
    assert r.returncode == 0 and "dustmasker" not in r.stderr
    assert open(tmp_path / "s_cli0", "rb").read() == open(tmp_path / "s_plain", "rb").read()
    r = subprocess.run([EXE, "sketch", "-i", fa, "-o", str(tmp_path / "s_bad"), "--sdust-t", "-1", "--sdust-w", "64"], capture_output=True, text=True)
    assert r.returncode != 0
