"""`krepp inspect` on the host: kr_index_stats_cpu, kr_format_inspect and the command line against the numpy restatement of
tests/inspect_ref.py.  No GPU is needed and none is touched."""
import os
import subprocess

import numpy as np
import pytest

import inspect_ref as ref
from conftest import ROOT

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
FIVE = "((a:0.03,b:0.03):0.02,(c:0.05,(d:0.01,e:0.01):0.0234567):1e-07);"


def cli(*args, env=None):
    return subprocess.run([EXE, *args], capture_output=True, env=dict(os.environ, **(env or {})), timeout=120)


def lib_ref(index_dir):
    out = []
    for sfx in ref.suffixes(index_dir):
        L = ref.read_lib(index_dir, sfx)
        out.append(ref.stats_ref(L["cmer"][:, 1], L["pse"], L["nsubsets"]))
    return out


def test_stats_of_the_toy_index(capi, toy_index_dir):
    hx = capi.HostIndex(toy_index_dir)
    want = lib_ref(toy_index_dir)
    for keep in (True, False):
        got = capi.index_stats(hx, keep_counts=keep)
        assert len(got) == len(want) == 1
        ref.assert_stats_equal(got[0], want[0], counts=keep)
        assert (got[0]["r"], got[0]["frac"]) == (1, 1)
    assert capi.format_inspect(hx, got) == ref.inspect_text(toy_index_dir)


def test_cli_on_the_toy_index(toy_index_dir):
    """m4r1-frac: two blocks, keys 0 and 1, with the fallback metadata text (the index has no metadata*.txt)"""
    r = cli("inspect", "-i", toy_index_dir)
    assert r.returncode == 0, r.stderr
    want = ref.inspect_text(toy_index_dir)
    assert r.stdout == want
    text = r.stdout.decode()
    assert text.count("======= Partial index: ") == 2 and "======= Partial index: 0 =======\nkrepp version: ?\ndate: ?\n" in text
    assert text.index("Partial index: 0 ") < text.index("Partial index: 1 ")
    assert "\n1\tNUM_COLORS\t" in text and "sdust-w: ?\n0\tNUM_COLORS" in text


@pytest.fixture(scope="module")
def built(capi, synth, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("inspect_built")
    g = synth.evolve_genomes(FIVE, 20_000, seed=8)
    tsv = synth.write_genomes(g, str(tmp / "g"))
    (tmp / "t.nwk").write_text(FIVE)
    kw = dict(k=21, w=27, h=7, m=4, r=1, frac=True, seed=3)
    capi.build_index(tsv, str(tmp / "with_tree"), nwk=str(tmp / "t.nwk"), **kw)
    capi.build_index(tsv, str(tmp / "no_tree"), **kw)
    return tmp


def test_cli_on_a_built_index_with_a_backbone(built):
    d = str(built / "with_tree")
    r = cli("inspect", "-i", d)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ref.inspect_text(d)
    lines = r.stdout.decode().split("\n")
    # branch lengths in the default ostream form: six significant digits, exponent where %g takes it
    assert lines[0] == "Backbone tree: ((a:0.03,b:0.03):0.02,(c:0.05,(d:0.01,e:0.01):0.0234567):1e-07);"
    info = open(os.path.join(d, "metadata-m4r1-frac.txt")).read()
    assert info and ("======= Partial index: 0 =======\n" + info + "0\tNUM_COLORS\t") in r.stdout.decode()
    assert ("======= Partial index: 1 =======\n" + info + "1\tNUM_COLORS\t") in r.stdout.decode()


def test_cli_without_a_backbone(built):
    d = str(built / "no_tree")
    r = cli("inspect", "-i", d)
    assert r.returncode == 0, r.stderr
    assert r.stdout == ref.inspect_text(d)
    assert r.stdout.startswith(b"Backbone tree: NA\n======= Partial index: 0 =======\n")


def test_cli_errors(tmp_path, toy_index_dir):
    r = cli("inspect", "-i", os.path.join(toy_index_dir, "cmer-m4r1-frac"))  # not a directory
    assert r.returncode == 1 and b"[ERROR] " in r.stderr and r.stdout == b""
    d = ref.write_index(str(tmp_path / "x"), [dict(r=0, frac=False, se=[1, 1], pse=[[0, 0], [0, 0]])], ["a"])
    os.remove(os.path.join(d, "crecord-m4r0-no_frac"))
    r = cli("inspect", "-i", d)  # a missing file
    assert r.returncode == 1 and b"[ERROR] " in r.stderr and r.stdout == b""
    d = ref.write_index(str(tmp_path / "y"), [dict(r=0, frac=False, se=[1, 2, 1], pse=[[0, 0], [0, 0]])], ["a"])
    r = cli("inspect", "-i", d)  # a bad colour id: nothing is printed for that index
    assert r.returncode == 1 and r.stdout == b""
    assert b"[ERROR] " in r.stderr and b"-m4r0-no_frac" in r.stderr and b"cmer[1]" in r.stderr and b"colour id 2" in r.stderr


def test_two_libraries_give_two_blocks_in_key_order(capi, tmp_path):
    pse = [[0, 0], [0, 0], [1, 1], [1, 2]]
    libs = [dict(r=1, frac=False, se=[1, 2, 2, 3], pse=pse, info="library: one\n"), dict(r=0, frac=False, se=[3, 3, 3], pse=pse, info="library: zero\n")]
    d = ref.write_index(str(tmp_path / "two"), libs, ["a"])
    hx = capi.HostIndex(d)
    got = capi.index_stats(hx, keep_counts=True)
    want = lib_ref(d)
    assert len(got) == 2
    for g, w in zip(got, want):
        ref.assert_stats_equal(g, w)
    text = capi.format_inspect(hx, got)
    assert text == ref.inspect_text(d)
    s = text.decode()
    assert s.startswith("Backbone tree: NA\n======= Partial index: 0 =======\nlibrary: zero\n0\tNUM_COLORS\t3\n0\tMER_COUNT\t0\t2\n0\tMER_COUNT\t3\t1\n")
    assert "======= Partial index: 1 =======\nlibrary: one\n1\tNUM_COLORS\t3\n1\tMER_COUNT\t1\t2\n1\tMER_COUNT\t2\t1\n1\tOUTDEGREE_COUNT\t0\t1\n" in s
    assert cli("inspect", "-i", d).stdout == text


@pytest.mark.parametrize("se,pse", [
    ([], [[0, 0]]),                                  # nsubsets 1: NUM_COLORS 0 and no histogram rows
    ([0, 0, 0], [[5, 5]]),                           # ... entry 0 is not a parent, whatever it holds
    ([1, 1, 0], [[0, 0], [1, 1]]),                   # nsubsets 2
    ([], [[0, 0], [0, 0], [1, 2]]),                  # nkmers 0
])
def test_small_crafted_views(capi, se, pse):
    view, keep = ref.craft_view(capi, [dict(se=se, pse=pse)])
    got = capi.index_stats(view, keep_counts=True)
    ref.assert_stats_equal(got[0], ref.stats_ref(se, pse, len(pse)))
    if len(pse) == 1:
        assert len(got[0]["mer_value"]) == 0 and len(got[0]["deg_value"]) == 0


def test_nsubsets_one_prints_no_rows(capi, tmp_path):
    d = ref.write_index(str(tmp_path / "one"), [dict(r=2, frac=False, se=[], pse=[[0, 0]])], ["a"])
    hx = capi.HostIndex(d)
    text = capi.format_inspect(hx, capi.index_stats(hx)).decode()
    assert text.endswith("sdust-w: ?\n2\tNUM_COLORS\t0\n") and "MER_COUNT" not in text and "OUTDEGREE_COUNT" not in text


def bad(capi, libs):
    view, keep = ref.craft_view(capi, libs)
    with pytest.raises(capi.KrError) as e:
        capi.index_stats(view, keep_counts=True)
    assert e.value.code == capi.KR_ERR_FORMAT
    return str(e.value)


def test_bad_colour_ids(capi):
    pse = [[0, 0], [0, 0], [1, 1], [2, 1], [3, 3]]  # nsubsets 5
    msg = bad(capi, [dict(se=[1, 2, 5, 4], pse=pse)])  # se == nsubsets
    assert "-m4r1-frac" in msg and "cmer[2]" in msg and "colour id 5" in msg
    msg = bad(capi, [dict(se=[1, 6, 4, 5], pse=pse, r=0, frac=0)])  # two bad entries: the smaller index is named
    assert "-m4r0-no_frac" in msg and "cmer[1]" in msg and "colour id 6" in msg
    p3 = [[0, 0], [0, 0], [1, 1], [2, 5], [3, 3]]  # a child == nsubsets in pse[3]
    msg = bad(capi, [dict(se=[1, 2, 3, 4], pse=p3)])
    assert "se_to_pse[3]" in msg and "colour id 5" in msg
    p23 = [[0, 0], [0, 0], [7, 1], [2, 5], [3, 3]]
    msg = bad(capi, [dict(se=[1, 2, 3, 4], pse=p23)])
    assert "se_to_pse[2]" in msg and "colour id 7" in msg
    msg = bad(capi, [dict(se=[1, 5, 3, 4], pse=p23)])  # cmer is walked first
    assert "cmer[1]" in msg
    p0 = [[9, 9], [0, 0], [1, 1], [2, 1], [3, 3]]  # entry 0 is not a parent
    view, keep = ref.craft_view(capi, [dict(se=[1, 2, 3, 4], pse=p0)])
    capi.index_stats(view)
