#!/usr/bin/env python3
"""Long query sequences that are already in HBM: the same batch of contigs through the C ABI
  (a) as KR_BASES_DEVICE, one wave per sequence (what a device batch got before KR_TILE_DEVICE, and still gets without it),
  (b) as KR_BASES_DEVICE | KR_TILE_DEVICE, tiled by the kr_tile_lay_* kernels (kr_dev_tiles.inc),
  (c) as a host batch, tiled by build_tiles while it is staged (for orientation: it pays a memcpy and PCIe),
in alternating rounds of one process, host clock around submit + collect (which ends in a stream synchronise); the time of the
submit call alone is (b)'s layout, summary wait and copy.  Shapes: docs/design/09.  Then `krepp dist` with and without --gpu-parse on
a synthetic long-read FASTQ file.  Index: 25 references of 400 kb (k27 / w35 / h11), as scripts/time_contigs.py.
usage: time_device_contigs.py [rounds]"""
import os, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
from krepp_amd import capi, synth
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
work = tempfile.mkdtemp(prefix="krepp_dctg_")
nwk = os.path.join(root, "tests", "golden", "tree_toy.nwk")
g = synth.evolve_genomes(open(nwk).read(), 400_000, seed=7)
tsv = synth.write_genomes(g, os.path.join(work, "g"))
idx = os.path.join(work, "idx")
capi.build_index(tsv, idx, nwk=nwk, k=27, w=35, h=11, m=4, r=1, frac=True, num_threads=8)
gl = list(g.values())
hx = capi.HostIndex(idx)
dx = hx.upload(0)


def contigs(L, nc, seed):  # stretches of the references with 1 % substitutions
    rng = np.random.default_rng(seed)
    seqs = []
    for i in range(nc):
        o = int(rng.integers(0, 400_000 - L + 1))
        s = gl[i % len(gl)][o:o + L].copy()
        mut = rng.random(len(s)) < 0.01
        s[mut] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(mut.sum()))]
        seqs.append(s)
    return np.concatenate(seqs), np.cumsum([0] + [len(s) for s in seqs]).astype(np.uint64)


def ms(xs):
    return f"median {np.median(xs) * 1e3:8.2f} ms  min {min(xs) * 1e3:8.2f} ms"


for L, nc in ((400_000, 1), (400_000, 8), (50_000, 200), (5_000, 2000)):
    bases, offs = contigs(L, nc, 3)
    tb, to = torch.from_numpy(bases).cuda(), torch.from_numpy(offs.view(np.int64)).cuda()
    torch.cuda.synchronize()
    vmax = int(len(bases) // 128 + nc + 1024)
    arms = {"a": (capi.KR_ROWS_ONLY, True), "b": (capi.KR_ROWS_ONLY | capi.KR_TILE_DEVICE, True), "c": (capi.KR_ROWS_ONLY, False)}
    st = {a: dx.stream(max_reads=vmax, max_bases=len(bases) + 64, max_records=vmax * 64) for a in arms}
    t_all, t_sub, rows, tm = {a: [] for a in arms}, {a: [] for a in arms}, {}, {}
    for rnd in range(rounds + 2):  # (two warm-up rounds: code objects, buffers made on first use)
        for a, (fl, dev) in arms.items():
            t0 = time.perf_counter()
            if dev:
                st[a].submit_device(tb.data_ptr(), to.data_ptr(), nc, fl)
            else:
                st[a].submit(bases, offs, fl)
            t1 = time.perf_counter()
            rv = st[a].collect_view()
            t2 = time.perf_counter()
            if rnd == rounds + 1:  # (outside the timed window) the output rows as a multiset of (key, DIST)
                sel = np.ctypeslib.as_array(rv.rec_sel, (rv.nrecs,)) != 0
                rows[a] = sorted(zip(np.ctypeslib.as_array(rv.rec_key, (rv.nrecs,))[sel].tolist(), np.ctypeslib.as_array(rv.rec_d, (rv.nrecs,))[sel].tolist()))
            if rnd >= 2:
                t_all[a].append(t2 - t0), t_sub[a].append(t1 - t0)
            tm[a] = st[a].timing()
    assert rows["a"] == rows["b"] == rows["c"] and len(rows["a"]) > 0, "the three arms disagree"
    lay = st["b"].tile_layout(nc)
    print(f"== {nc} x {L} bases ({len(bases) / 1e6:.2f} Mb), {lay['nv']} reads in the tiled batch, {len(rows['a'])} rows, {rounds} rounds", flush=True)
    for a, what in (("a", "device, one wave per sequence"), ("b", "device, KR_TILE_DEVICE       "), ("c", "host batch, tiled on the host")):
        t = tm[a]
        print(f"  ({a}) {what}: {ms(t_all[a])}   submit call alone: {ms(t_sub[a])}   "
              f"(last batch's kernels: scan {t.ms_scan:.2f}, accumulate {t.ms_acc:.2f}, likelihood {t.ms_llh:.2f}, all {t.ms_total:.2f} ms)", flush=True)
    for s_ in st.values():
        s_.close()
    del tb, to

# the CLI on a long-read file: 2,000 reads of 2 to 40 kb (log-uniform), 1 % substitutions
rng = np.random.default_rng(11)
q = os.path.join(work, "long_reads.fq")
with open(q, "wb") as f:
    nb = 0
    for i in range(2000):
        L = int(np.exp(rng.uniform(np.log(2000), np.log(40000))))
        o = int(rng.integers(0, 400_000 - L + 1))
        s = gl[i % len(gl)][o:o + L].copy()
        mut = rng.random(L) < 0.01
        s[mut] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(mut.sum()))]
        f.write(b"@lr%d\n" % i + s.tobytes() + b"\n+\n" + b"I" * L + b"\n")
        nb += L
exe = os.path.join(root, "krepp_amd", "lib", "krepp")
outs, times = {}, {"host reader": [], "--gpu-parse": []}
for rnd in range(4):
    for what, extra in (("host reader", []), ("--gpu-parse", ["--gpu-parse"])):
        o = os.path.join(work, "out_%d.tsv" % len(extra))
        t0 = time.perf_counter()
        r = subprocess.run([exe, "dist", "-i", idx, "-q", q, "-o", o, "--gpus", "1"] + extra, capture_output=True, timeout=300)
        dt = time.perf_counter() - t0
        assert r.returncode == 0, r.stderr.decode()[-2000:]
        outs[what] = open(o, "rb").read().split(b"\n", 1)[1]
        if rnd:
            times[what].append(dt)
assert outs["host reader"] == outs["--gpu-parse"], "the reports differ"
print(f"== krepp dist, 2000 long reads, {nb / 1e6:.1f} Mb, {len(outs['host reader'])} bytes of report, whole process (3 runs after one warm-up)")
for what, xs in times.items():
    print(f"  {what}: {ms(xs)}", flush=True)
