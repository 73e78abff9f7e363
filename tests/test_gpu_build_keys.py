"""`krepp index --gpu-keys` / build_index(gpu_keys=True): the key stage on the device's pool writes, byte for byte, the files
of the host path; the same for `krepp sketch` with either GPU stage."""
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
    """The five-leaf case of test_index_built_with_gpu_leaf_stage_is_identical, with its host-path index built once"""
    tmp = tmp_path_factory.mktemp("build_keys")
    g = synth.evolve_genomes(FIVE, 200_000, seed=8)
    tsv = synth.write_genomes(g, str(tmp / "g"), contigs=3)
    (tmp / "t.nwk").write_text(FIVE)
    return g, tsv, tmp


KW = dict(k=29, w=35, h=13, m=4, r=1, frac=True, seed=3)


@pytest.fixture(scope="module")
def five_host(capi, five):
    _, tsv, tmp = five
    capi.build_index(tsv, str(tmp / "host"), nwk=str(tmp / "t.nwk"), **KW)
    want = files(str(tmp / "host"))
    assert all(v is not None for v in want.values())
    return want


def test_five_leaves_four_threads(capi, five, five_host):
    _, tsv, tmp = five
    capi.build_index(tsv, str(tmp / "keys4"), nwk=str(tmp / "t.nwk"), num_threads=4, gpu_keys=True, **KW)
    st = capi.build_keys_stats()
    assert files(str(tmp / "keys4")) == five_host
    assert st["path"] == 1 and st["passes"] == 1 + 8  # 5 leaves: one rank digit; 2^25 rows: 32 + 25 bits of key, eight digits
    nk = int(np.frombuffer(five_host["cmer"][:8], "<u8")[0])
    assert st["keys_out"] == nk and st["pairs_in"] > st["pairs_out"] > nk


def test_balanced_tree_one_thread(capi, five):
    _, tsv, tmp = five
    capi.build_index(tsv, str(tmp / "bal_host"), **KW)
    capi.build_index(tsv, str(tmp / "bal_keys"), gpu_keys=True, **KW)
    want = files(str(tmp / "bal_host"))
    assert want["tree"] is None and want["cmer"] is not None
    assert files(str(tmp / "bal_keys")) == want


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
    capi.build_index(tsv, str(tmp / "nb_keys"), nwk=str(tmp / "nb.nwk"), num_threads=3, gpu_keys=True, **KW)
    want = files(str(tmp / "nb_host"))
    assert all(v is not None for v in want.values()) and b"zz\n" in want["reflist"]
    assert files(str(tmp / "nb_keys")) == want


def test_five_leaves_masked(capi, five):
    _, tsv, tmp = five
    kw = dict(KW, nwk=str(tmp / "t.nwk"), sdust_t=20, sdust_w=64)
    capi.build_index(tsv, str(tmp / "dust_host"), **kw)
    capi.build_index(tsv, str(tmp / "dust_keys"), num_threads=4, gpu_keys=True, **kw)
    assert files(str(tmp / "dust_keys")) == files(str(tmp / "dust_host"))


def test_pool_growth(capi, five, five_host, monkeypatch):
    _, tsv, tmp = five
    monkeypatch.setenv("KR_BUILD_POOL_PAIRS", "4096")
    capi.build_index(tsv, str(tmp / "grow"), nwk=str(tmp / "t.nwk"), num_threads=4, gpu_keys=True, **KW)
    st = capi.build_keys_stats()
    assert st["pool_growths"] >= 1 and st["path"] == 1
    assert files(str(tmp / "grow")) == five_host


def test_falls_back_to_the_host_for_memory(capi, five, five_host, monkeypatch):
    _, tsv, tmp = five
    monkeypatch.setenv("KR_BUILD_KEYS_MAX_MB", "1")
    capi.build_index(tsv, str(tmp / "fallback"), nwk=str(tmp / "t.nwk"), num_threads=4, gpu_keys=True, **KW)
    assert capi.build_keys_stats()["path"] == 2
    assert files(str(tmp / "fallback")) == five_host


def cli(*args):
    r = subprocess.run([EXE, *args], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return r


def test_cli_index_gpu_keys(five, five_host):
    _, tsv, tmp = five
    common = ["-t", str(tmp / "t.nwk"), "-k", "29", "-w", "35", "-h", "13", "--seed", "3", "--num-threads", "4"]
    cli("index", "-i", tsv, "-o", str(tmp / "cli_host"), *common)
    cli("index", "-i", tsv, "-o", str(tmp / "cli_keys"), "--gpu-keys", *common)
    want = files(str(tmp / "cli_host"))
    assert want == five_host
    assert files(str(tmp / "cli_keys")) == want


def test_cli_sketch_gpu_stages(synth, five):
    g, _, tmp = five
    seq = g["a"][:120_000].copy()
    seq[30_000:30_400] = ord("N")
    seq[77_000] = ord("N")
    fa = str(tmp / "sk.fa")
    with open(fa, "wb") as f:
        f.write(b">c1\n" + seq[:60_000].tobytes() + b"\n>tiny\n" + seq[60_000:60_020].tobytes() + b"\n>shorter_than_w\n" + seq[60_020:60_051].tobytes()
                + b"\n>c2 with N runs\n" + seq[60_051:].tobytes() + b"\n>ends_in_a_short_run\n" + seq[:500].tobytes() + b"N" + seq[500:530].tobytes() + b"\n")
    cli("sketch", "-i", fa, "-o", str(tmp / "sk_host"))
    cli("sketch", "-i", fa, "-o", str(tmp / "sk_leaf"), "--gpu-minimizers")
    cli("sketch", "-i", fa, "-o", str(tmp / "sk_keys"), "--gpu-minimizers", "--gpu-keys")
    want = open(str(tmp / "sk_host"), "rb").read()
    assert int(np.frombuffer(want[:8], "<u8")[0]) > 1000
    assert open(str(tmp / "sk_leaf"), "rb").read() == want
    assert open(str(tmp / "sk_keys"), "rb").read() == want
    cli("sketch", "-i", fa, "-o", str(tmp / "skd_host"), "--sdust-t", "20", "--sdust-w", "64")
    cli("sketch", "-i", fa, "-o", str(tmp / "skd_keys"), "--sdust-t", "20", "--sdust-w", "64", "--gpu-keys")
    assert open(str(tmp / "skd_keys"), "rb").read() == open(str(tmp / "skd_host"), "rb").read()


def test_cli_help_lists_gpu_keys():
    assert "--gpu-keys" in cli("index", "--help").stdout
    assert "--gpu-keys" in cli("sketch", "--help").stdout
