"""--sdust-t/-w on the GPU: the masked instantiation of the minimizer kernel (fed by the host masker) against the masked CPU leaf
stage, and whole masked indexes built with the GPU leaf stage against the CPU build, byte for byte."""
import os

import numpy as np
import pytest

from sdust_cases import OUT_OF_ORDER, SEQS, implant, pack

pytestmark = pytest.mark.gpu
NAMES = list(SEQS)
ACGT = np.frombuffer(b"ACGT", np.uint8)


def leaf_contigs(synth, w):
    rng = np.random.default_rng(31)
    g = synth.evolve_genomes("(a:0.1,b:0.1);", 300_000, seed=3)["a"]
    codes = np.searchsorted(ACGT, g)
    implant(rng, codes, 50)
    # a stretch over the first tile edge of the contigs cut below: its skip span and its break sit at positions 2047 / 2048 / 2049
    codes[2048 - 60:2048 + 5] = np.resize([0, 2], 65)
    text = ACGT[codes].copy()
    text[100_000:100_007] = ord("N")
    text[200_000:200_450] = ord("n")
    g = text.tobytes()
    contigs = [SEQS[n] for n in NAMES]
    contigs += [g, g[:2047 + w], g[:2048 + w], g[:2049 + w], g[:2047], g[:2048], g[:2049], g[3:2048 + w], g[1:2049 + w]]
    return contigs


@pytest.mark.parametrize("k,w,h,m,r,frac", [(21, 27, 7, 4, 1, True), (29, 35, 13, 4, 1, True), (27, 27, 11, 8, 3, False),
                                            (31, 90, 15, 4, 1, True)])
@pytest.mark.parametrize("T,W", [(20, 64), (10, 16)])
def test_masked_hip_minimizers_bit_exact(capi, synth, k, w, h, m, r, frac, T, W):
    rng = np.random.default_rng(9)
    ppos = sorted(rng.choice(k, h, replace=False).tolist(), reverse=True)
    bases, offs = pack(leaf_contigs(synth, w))
    kc, n1c, n2c = capi.minimizers(bases, offs, k, w, h, ppos, m=m, r=r, frac=frac, sdust_t=T, sdust_w=W)
    kg, n1g, n2g = capi.minimizers(bases, offs, k, w, h, ppos, m=m, r=r, frac=frac, sdust_t=T, sdust_w=W, device=0)
    assert kg.tolist() == kc.tolist() and len(kc) > 1000
    assert (n1g, n2g) == (n1c, n2c)
    plain = capi.minimizers(bases, offs, k, w, h, ppos, m=m, r=r, frac=frac, device=0)
    assert plain[0].tolist() != kg.tolist()  # masking changes the keys


def test_masked_hip_minimizers_w128(capi, synth):
    """sdust_w = 128: any W the host masker takes reaches the same masked kernel."""
    ppos = [20, 19, 17, 13, 6, 4, 2]
    bases, offs = pack(leaf_contigs(synth, 27)[-9:-6] + [SEQS[n] for n in NAMES])
    c = capi.minimizers(bases, offs, 21, 27, 7, ppos, sdust_t=20, sdust_w=128)
    g = capi.minimizers(bases, offs, 21, 27, 7, ppos, sdust_t=20, sdust_w=128, device=0)
    assert g[0].tolist() == c[0].tolist() and (g[1], g[2]) == (c[1], c[2])


FILES = ("cmer", "inc", "crecord", "metadata", "tree", "reflist")


@pytest.fixture(scope="module")
def five_genomes(synth, tmp_path_factory):
    tmp = tmp_path_factory.mktemp("sdust_idx")
    nwk = "((a:0.03,b:0.03):0.02,(c:0.05,(d:0.01,e:0.01):0.02):0.01);"
    g = synth.evolve_genomes(nwk, 200_000, seed=8)
    rng = np.random.default_rng(8)
    out = {}
    for name, seq in g.items():
        codes = np.searchsorted(ACGT, seq)
        implant(rng, codes, 40)
        text = ACGT[codes].copy()
        text[50_000:50_300] = ord("N")
        if name == "c":  # where the reference's list is not the union of the intervals it saved
            text[70_000:70_000 + len(SEQS[OUT_OF_ORDER[0]])] = np.frombuffer(SEQS[OUT_OF_ORDER[0]], np.uint8)
        out[name] = text
    tsv = synth.write_genomes(out, str(tmp / "g"), contigs=3)
    (tmp / "t.nwk").write_text(nwk)
    kw = dict(nwk=str(tmp / "t.nwk"), k=29, w=35, h=13, m=4, r=1, frac=True, seed=3)
    return out, tsv, tmp, kw


def _files(d):
    return {f: open(os.path.join(d, f + "-m4r1-frac"), "rb").read() for f in FILES}


def test_masked_index_gpu_leaf_stage_equals_cpu_leaf_stage(capi, synth, five_genomes):
    genomes, tsv, tmp, kw = five_genomes
    cpu, gpu, plain = str(tmp / "cpu"), str(tmp / "gpu"), str(tmp / "plain")
    capi.build_index(tsv, cpu, sdust_t=20, sdust_w=64, **kw)
    capi.build_index(tsv, gpu, sdust_t=20, sdust_w=64, gpu_minimizers=True, num_threads=4, **kw)
    capi.build_index(tsv, plain, **kw)
    assert _files(cpu) == _files(gpu)
    assert _files(cpu)["cmer"] != _files(plain)["cmer"]
    # `dist` runs on the masked index
    bases, offsets, names = synth.sample_reads(genomes, 256, seed=1)
    hx = capi.HostIndex(gpu)
    st = hx.upload(0).stream(max_reads=256, max_bases=len(bases))
    st.submit(bases, offsets, capi.KR_TAP_ACCS)
    assert len(st.collect().rows()) > 100


def test_masked_index_w128(capi, five_genomes):
    genomes, tsv, tmp, kw = five_genomes
    cpu, gpu = str(tmp / "cpu128"), str(tmp / "gpu128")
    capi.build_index(tsv, cpu, sdust_t=20, sdust_w=128, **kw)
    capi.build_index(tsv, gpu, sdust_t=20, sdust_w=128, gpu_minimizers=True, **kw)
    assert _files(cpu) == _files(gpu)
