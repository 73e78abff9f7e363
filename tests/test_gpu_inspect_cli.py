"""`krepp inspect --gpu-stats` prints, byte for byte, what the run without the flag prints."""
import os
import subprocess

import pytest

import inspect_ref as ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

EXE = os.path.join(ROOT, "krepp_amd", "lib", "krepp")
FIVE = "((a:0.03,b:0.03):0.02,(c:0.05,(d:0.01,e:0.01):0.0234567):1e-07);"


def cli(*args, env=None):
    return subprocess.run([EXE, *args], capture_output=True, env=dict(os.environ, **(env or {})), timeout=300)


def test_toy_index(toy_index_dir):
    host = cli("inspect", "-i", toy_index_dir)
    dev = cli("inspect", "-i", toy_index_dir, "--gpu-stats", env={"KR_CLI_TIMING": "1"})
    assert host.returncode == 0 and dev.returncode == 0, dev.stderr
    assert dev.stdout == host.stdout == ref.inspect_text(toy_index_dir)
    assert b"[timing] inspect:" in dev.stderr and b"(device)" in dev.stderr
    timed = cli("inspect", "-i", toy_index_dir, env={"KR_CLI_TIMING": "1"})
    assert b"(host)" in timed.stderr and timed.stdout == host.stdout


def test_built_index_with_a_backbone(capi, synth, tmp_path):
    g = synth.evolve_genomes(FIVE, 20_000, seed=8)
    tsv = synth.write_genomes(g, str(tmp_path / "g"))
    (tmp_path / "t.nwk").write_text(FIVE)
    d = str(tmp_path / "ix")
    capi.build_index(tsv, d, nwk=str(tmp_path / "t.nwk"), k=21, w=27, h=7, m=4, r=1, frac=True, seed=3)
    host = cli("inspect", "-i", d)
    dev = cli("inspect", "-i", d, "--gpu-stats", "--device", "0", env={"KR_STATS_CHUNK_KMERS": "1001"})
    assert host.returncode == 0 and dev.returncode == 0, dev.stderr
    assert dev.stdout == host.stdout == ref.inspect_text(d)
    assert host.stdout.startswith(b"Backbone tree: ((a:0.03,b:0.03):0.02,")


def test_bad_colour_id(tmp_path):
    d = ref.write_index(str(tmp_path / "y"), [dict(r=0, frac=False, se=[1, 2, 1], pse=[[0, 0], [0, 0]])], ["a"])
    host = cli("inspect", "-i", d)
    dev = cli("inspect", "-i", d, "--gpu-stats")
    assert dev.returncode == 1 and dev.stdout == b""
    err = [l for l in dev.stderr.split(b"\n") if l.startswith(b"[ERROR]")]
    assert err and err == [l for l in host.stderr.split(b"\n") if l.startswith(b"[ERROR]")] and b"cmer[1]" in err[0]
