#!/usr/bin/env python3
"""Regenerates the committed fixtures under tests/golden/.  Run in the build container
(needs /root/reference for the *_ref.json files, which come from the reference's own
sources compiled into oracle/_ref/ — see oracle/ref_drivers/ref_shim.cpp).

  llh_ref.json     HDistHistLLH::operator() values computed by the REFERENCE header
                   (src/hdhistllh.hpp) on seeded random problems            [reference output]
  llh_live_ref.json  the same, on the problems of tests/helpers.py::llh_live_cases
                   (hex doubles, in order)                                    [reference output]
  murmur_ref.json  MurmurHash3_x86_32 of node names by the REFERENCE source  [reference output]
  kseq_ref.json    records parsed by the REFERENCE kseq.h from query_toy.fq and from an
                   edge-case FASTA/FASTQ text embedded in the JSON           [reference output]
  hll_ref.json     hll::HyperLogLog(12) estimates by the REFERENCE header    [reference output]
  toy_index/       small index (25 synthetic 20-kb genomes, -k 21 -w 27 -h 7, m4r1-frac)
                   built by this repository's CPU builder                     [own output]
  toy_reads.fq, toy_expected.json   reads and the ORACLE's rows / accumulators / hits on
                   that index (hex doubles)                                   [oracle output]
"""
import ctypes as C
import gzip
import json
import os
import shutil
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import pyoracle as po  # noqa: E402
from helpers import llh_live_cases  # noqa: E402
from krepp_amd import capi, synth  # noqa: E402

EDGE_TEXT = (
    ">s1 a comment\nACGTACGTAC\nGGGTTTAA\n>s2\n\nacgtnnACGT\n>s3\tx\nAC GT\n@q1 desc\nACGTTGCA\n+\nIIIIIIII\n"
    "@q2\nAC\nGT\n+q2\nII\nII\n>tail_no_newline\nTTTT"
)


def write_llh_live(ref):
    vals = [float(ref.ref_llh(k, h, th, np.ascontiguousarray(hist).ctypes.data, uc, rho, d)).hex()
            for k, h, th, hist, uc, rho, d in llh_live_cases()]
    json.dump(vals, open(os.path.join(HERE, "llh_live_ref.json"), "w"))


def main():
    ref = po.ref()
    assert ref is not None, "oracle/_ref/libkrepp_ref.so missing: run `make -C oracle` with /root/reference present"
    rng = synth.Rng(12345, 9)
    # ---- llh
    cases = []
    for (k, h, th) in [(27, 11, 4), (29, 13, 4), (21, 7, 4), (31, 15, 6), (27, 11, 0), (19, 3, 16), (29, 13, 2)]:
        for _ in range(40):
            n = 1 + int(rng.below(1, 150)[0])
            hist = np.zeros(th + 1)
            w = rng.uniform(th + 1) ** 3
            cnt = np.floor(w / w.sum() * n * rng.uniform(1)[0])
            hist[:] = cnt
            uc = float(max(0.0, n - hist.sum()))
            rho = float(0.02 + 0.9 * rng.uniform(1)[0])
            ds = [1e-10, 1e-5, 0.5] + (10 ** (-5 * rng.uniform(3))).tolist()
            ds = [min(0.5, float(d)) for d in ds]
            hc = np.ascontiguousarray(hist)
            vals = [ref.ref_llh(k, h, th, hc.ctypes.data, uc, rho, d) for d in ds]
            cases.append(dict(k=k, h=h, th=th, hist=hist.tolist(), uc=uc, rho=rho.hex(), d=[d.hex() for d in ds],
                              f=[float(v).hex() for v in vals]))
    json.dump(cases, open(os.path.join(HERE, "llh_ref.json"), "w"))
    write_llh_live(ref)
    # ---- murmur
    names = ["G000341695", "G001610775", "N4337", "", "a", "ab", "abc", "abcd", "abcde", "x" * 33,
             "Escherichia coli K-12", "root"]
    mm = [dict(name=s, seed0=ref.ref_murmur3_x86_32(s.encode(), len(s), 0), seed1=ref.ref_murmur3_x86_32(s.encode(), len(s), 1))
          for s in names]
    json.dump(mm, open(os.path.join(HERE, "murmur_ref.json"), "w"))
    # ---- kseq
    def parse(path):
        nb = C.create_string_buffer(1 << 20)
        sb = C.create_string_buffer(1 << 22)
        last = C.c_int()
        n = ref.ref_kseq_parse(path.encode(), nb, len(nb), sb, len(sb), C.byref(last))
        nm = nb.raw.split(b"\0")[:n]
        sq = sb.raw.split(b"\0")[:n]
        return dict(n=n, last=last.value, names=[x.decode() for x in nm], seqs=[x.decode() for x in sq])
    edge_path = "/tmp/kr_edge.fx"
    open(edge_path, "w").write(EDGE_TEXT)
    trunc_path = "/tmp/kr_trunc.fq"
    open(trunc_path, "w").write("@a\nACGT\n+\nIIII\n@b\nACGTAC\n+\nIII\n@c\nAC\n+\nII\n")
    gz_path = "/tmp/kr_edge.fx.gz"
    with gzip.open(gz_path, "wt") as f:
        f.write(EDGE_TEXT)
    ks = dict(query_toy=parse(os.path.join(HERE, "query_toy.fq")), edge_text=EDGE_TEXT, edge=parse(edge_path),
              trunc_text=open(trunc_path).read(), trunc=parse(trunc_path), edge_gz=parse(gz_path))
    q = ks["query_toy"]
    import hashlib
    q["sha_names"] = hashlib.sha256("\n".join(q["names"]).encode()).hexdigest()
    q["sha_seqs"] = hashlib.sha256("\n".join(q["seqs"]).encode()).hexdigest()
    q.pop("names"), q.pop("seqs")
    json.dump(ks, open(os.path.join(HERE, "kseq_ref.json"), "w"))
    # ---- hll
    hl = []
    for n in [0, 1, 10, 1000, 5000, 20000, 200000]:
        hs = rng.u64(n) if n else np.zeros(0, np.uint64)
        hs = np.ascontiguousarray(hs)
        est = ref.ref_hll_estimate(hs.ctypes.data if n else None, n, 12)
        hl.append(dict(n=n, seed_pos=int(rng.pos - n), est=float(est).hex()))
    json.dump(dict(seed=12345, stream=9, cases=hl), open(os.path.join(HERE, "hll_ref.json"), "w"))
    # ---- toy index + oracle outputs
    nwk = os.path.join(HERE, "tree_toy.nwk")
    g = synth.evolve_genomes(open(nwk).read(), 20000, seed=7)
    tmp = "/tmp/kr_golden_g"
    tsv = synth.write_genomes(g, tmp, contigs=2)
    idx = os.path.join(HERE, "toy_index")
    shutil.rmtree(idx, ignore_errors=True)
    capi.build_index(tsv, idx, nwk=nwk, k=21, w=27, h=7, m=4, r=1, frac=True, num_threads=4)
    os.remove(os.path.join(idx, "metadata-m4r1-frac.txt"))
    b, o, names = synth.sample_reads(g, 300, seed=1)
    # edge-case reads appended: lowercase, short, exactly k, with Ns, long (multi-segment)
    extra = [("lower", bytes(b[:150]).lower()), ("short", b"ACGTACGTAC"), ("exact_k", bytes(b[150:171])),
             ("empty", b""), ("all_n", b"N" * 150), ("two_n", bytes(b[300:340]) + b"NN" + bytes(b[342:450])),
             ("long", bytes(g["G000341695"][1000:2200])), ("iupac", bytes(b[450:500]) + b"R" + bytes(b[501:600]))]
    chunks = [bytes(b[int(o[i]):int(o[i + 1])]) for i in range(300)] + [e[1] for e in extra]
    names = names + [e[0] for e in extra]
    synth.write_fastq(os.path.join(HERE, "toy_reads.fq"), np.frombuffer(b"".join(chunks), np.uint8),
                      np.cumsum([0] + [len(c) for c in chunks]).astype(np.uint64), names)
    bases = np.frombuffer(b"".join(chunks), np.uint8)
    offs = np.cumsum([0] + [len(c) for c in chunks]).astype(np.uint64)
    ox = po.Index(idx)
    exp = {}
    for tag, p in [("default", po.params(collect=7)), ("filter", po.params(collect=5, no_filter=0)),
                   ("nomulti", po.params(collect=5, multi=0)), ("dmax", po.params(collect=5, dist_max=0.05)),
                   ("th2", po.params(collect=5, hdist_th=2))]:
        r = ox.dist(bases, offs, names, p)
        exp[tag] = dict(rows=[(int(x["read"]), int(x["se"]), float(x["d_llh"]).hex()) for x in r["rows"]],
                        text=r["text"], counters=r["counters"])
        if tag == "default":
            exp[tag]["accs"] = [(int(x["read"]), int(x["se"]), int(x["strand"]), int(x["passed"]), x["hist"][:5].tolist(),
                                 float(x["d_llh"]).hex()) for x in r["accs"]]
            exp[tag]["nhits"] = int(len(r["hits"]))
            exp[tag]["onmers"] = r["reads"]["onmers"].tolist()
            exp[tag]["hdist_filt"] = r["reads"]["hdist_filt"].tolist()
    json.dump(exp, open(os.path.join(HERE, "toy_expected.json"), "w"))
    print("golden fixtures written")


if __name__ == "__main__":
    main()
