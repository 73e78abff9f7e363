"""`krepp index --gpu-colours` / build_index(gpu_colours=True): the groups' distinct leaf sets found on the device and each folded
into a colour once writes, byte for byte, the files of the host path, whose colour loop folds every group."""
import os
import subprocess

import numpy as np
import pytest

from conftest import ROOT

pytestmark = pytest.mark.gpu

FILES = ("cmer", "inc", "crecord", "metadata", "tree", "reflist")
FIVE = "((a:0.03,b:0.03):0.02,(c:0.05,(d:0.01,e:0.01):0.02):0.01);"
EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")


def files(d):
    """the index files of directory d (None: not written)"""
    out = {}
    for f in FILES:
        p = os.path.join(d, f + "-m4r1-frac")
        out[f] = open(p, "rb").read() if os.path.exists(p) else None
    return out


@pytest.fixture(scope="module")
def five(synth, tmp_path_factory):
    """The five-leaf case of test_gpu_build_keys.py"""
    tmp = tmp_path_factory.mktemp("build_colours")
    g = synth.evolve_genomes(FIVE, 200_000, seed=8)
    tsv = synth.write_genomes(g, str(tmp / "g"), contigs=3)
    (tmp / "t.nwk").write_text(FIVE)
    return g, tsv, tmp


KW = dict(k=29, w=35, h=13, m=4, r=1, frac=True, seed=3)


@pytest.fixture(scope="module")
def five_host(capi, five):
    _, tsv, tmp = five
    capi.build_index(tsv, str(tmp / "host"), nwk=str(tmp / "t.nwk"), **KW)
    assert capi.build_colours_stats()["path"] == 0  # not asked
    want = files(str(tmp / "host"))
    assert all(v is not None for v in want.values())
    return want


def test_five_leaves_four_threads(capi, five, five_host):
    _, tsv, tmp = five
    capi.build_index(tsv, str(tmp / "col4"), nwk=str(tmp / "t.nwk"), num_threads=4, gpu_colours=True, **KW)
    st, keys = capi.build_colours_stats(), capi.build_keys_stats()
    assert files(str(tmp / "col4")) == five_host
    nk = int(np.frombuffer(five_host["cmer"][:8], "<u8")[0])
    assert keys["path"] == 1 and st["path"] == 1 and st["passes"] == 8
    assert st["groups"] == nk == keys["keys_out"]
    assert 0 < st["classes"] <= 2 ** 5 - 5 - 1 and st["classes"] < st["multi"] < nk  # sets of two or more of five leaves


def test_balanced_tree_one_thread(capi, five):
    _, tsv, tmp = five
    capi.build_index(tsv, str(tmp / "bal_host"), **KW)
    capi.build_index(tsv, str(tmp / "bal_col"), gpu_colours=True, **KW)
    want = files(str(tmp / "bal_host"))
    assert want["tree"] is None and want["cmer"] is not None
    assert files(str(tmp / "bal_col")) == want


def test_non_binary_tree_stranger_and_a_name_twice(capi, synth, five):
    g, _, tmp = five
    nwk = "((a:0.03,b:0.03,c:0.04):0.02,(d:0.01,e:0.01):0.02);"
    (tmp / "nb.nwk").write_text(nwk)
    stranger = dict(g)
    stranger["zz"] = g["a"][::-1].copy()  # in no tree
    tsv0 = synth.write_genomes(stranger, str(tmp / "g2"))
    tsv = str(tmp / "twice.tsv")
    with open(tsv, "w") as f:  # `b` a second time, with another genome's sequence behind the name
        f.write(open(tsv0).read() + "b\t" + str(tmp / "g2" / "d.fna") + "\n")
    capi.build_index(tsv, str(tmp / "nb_host"), nwk=str(tmp / "nb.nwk"), **KW)
    capi.build_index(tsv, str(tmp / "nb_col"), nwk=str(tmp / "nb.nwk"), num_threads=3, gpu_colours=True, **KW)
    want = files(str(tmp / "nb_host"))
    assert all(v is not None for v in want.values()) and b"zz\n" in want["reflist"]
    assert files(str(tmp / "nb_col")) == want


def test_five_leaves_masked(capi, five):
    _, tsv, tmp = five
    kw = dict(KW, nwk=str(tmp / "t.nwk"), sdust_t=20, sdust_w=64)
    capi.build_index(tsv, str(tmp / "dust_host"), **kw)
    capi.build_index(tsv, str(tmp / "dust_col"), num_threads=4, gpu_colours=True, **kw)
    assert files(str(tmp / "dust_col")) == files(str(tmp / "dust_host"))


def test_falls_back_to_the_host_for_memory(capi, five, five_host, monkeypatch):
    _, tsv, tmp = five
    monkeypatch.setenv("KR_BUILD_KEYS_MAX_MB", "1")
    capi.build_index(tsv, str(tmp / "fallback"), nwk=str(tmp / "t.nwk"), num_threads=4, gpu_colours=True, **KW)
    st = capi.build_colours_stats()
    assert capi.build_keys_stats()["path"] == 2 and st["path"] == 2 and st["classes"] > 0
    assert files(str(tmp / "fallback")) == five_host


@pytest.mark.parametrize("bits", ["0", "3"])
def test_reduced_fingerprints_write_the_same_files(capi, five, five_host, monkeypatch, bits):
    _, tsv, tmp = five
    monkeypatch.setenv("KR_BUILD_COLOUR_HASH_BITS", bits)
    capi.build_index(tsv, str(tmp / ("bits" + bits)), nwk=str(tmp / "t.nwk"), num_threads=4, gpu_colours=True, **KW)
    st = capi.build_colours_stats()
    assert st["path"] == 1 and st["raised"] > 0 and st["classes"] <= st["multi"]
    assert files(str(tmp / ("bits" + bits))) == five_host


def test_sixty_four_leaves(capi, synth, tmp_path):
    nwk = synth.yule_newick(64, 5)
    g = synth.evolve_genomes(nwk, 20_000, seed=8)
    tsv = synth.write_genomes(g, str(tmp_path / "g"))
    (tmp_path / "t.nwk").write_text(nwk)
    ppos = list(range(25, 0, -2))  # given, so that the groups can be made again below
    kw = dict(k=29, w=35, h=13, m=4, r=1, frac=True, ppos=ppos, nwk=str(tmp_path / "t.nwk"))
    capi.build_index(tsv, str(tmp_path / "host"), **kw)
    capi.build_index(tsv, str(tmp_path / "col"), num_threads=4, gpu_colours=True, **kw)
    st = capi.build_colours_stats()
    want = files(str(tmp_path / "host"))
    assert all(v is not None for v in want.values())
    assert files(str(tmp_path / "col")) == want
    assert st["path"] == 1 and 0 < st["classes"] < st["multi"] < st["groups"]
    # the classes are the distinct colours of the groups of several leaves: the host build's cmer, with the groups' lengths
    keys = [capi.minimizers(seq, np.array([0, len(seq)], np.uint64), 29, 35, 13, ppos)[0] for seq in g.values()]
    ranks = np.concatenate([np.full(len(k), q, np.uint32) for q, k in enumerate(keys)])
    grp = capi.key_groups(np.concatenate(keys), ranks, 1 << 25, 64, copy=False)
    try:
        lens = np.diff(grp["goff"].astype(np.int64))
        cmer = np.frombuffer(want["cmer"], "<u4", offset=8).reshape(-1, 2)
        assert len(lens) == len(cmer) == st["groups"] and np.array_equal(cmer[:, 0], (grp["keys"] & np.uint64(0xFFFFFFFF)).astype(np.uint32))
        assert int((lens >= 2).sum()) == st["multi"]
        assert len(np.unique(cmer[lens >= 2, 1])) == st["classes"]
    finally:
        grp["free"]()


def cli(*args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_index_gpu_colours(five, five_host):
    _, tsv, tmp = five
    common = ["-t", str(tmp / "t.nwk"), "-k", "29", "-w", "35", "-h", "13", "--seed", "3", "--num-threads", "4"]
    cli("index", "-i", tsv, "-o", str(tmp / "cli_host"), *common)
    cli("index", "-i", tsv, "-o", str(tmp / "cli_col"), "--gpu-colours", *common)
    want = files(str(tmp / "cli_host"))
    assert want == five_host
    assert files(str(tmp / "cli_col")) == want


def test_cli_help_lists_gpu_colours_for_index_only():
    assert "--gpu-colours" in cli("index", "--help").stdout
    assert "--gpu-colours" not in cli("sketch", "--help").stdout
