#!/usr/bin/env python3
"""What splitting PAIRED reads together costs (kr_batch_extract_pair; docs/design/13_seek.md 13.7).
  a. kernels: kr_debug_extract_ms of one pair call on 2 x 64 MB of 150-base FASTQ (the mates in two streams: the pair kernel, then
     the four extract kernels for each stream), against the sum of two unpaired extracts of the same two chunks.  Each leg runs in a
     process of its own, the legs alternate, and the unpaired leg can load ANOTHER build of the library (--parent ROOT: a checkout of
     the commit in front of this feature, built) -- the comparison that says whether the pair call costs anything.
  b. CLI: `krepp seek --gpu-parse --gpu-seek` on 2 M pairs in two plain files, paired (four extract files), against the two unpaired
     extract runs of the same files (--parent ROOT: that build's binary): wall seconds and the query phase, three alternating rounds.
  c. the host cutter: kr_fastq_pair_cut on the two 64 MB chunks of (a), GB/s of one thread (no device).
Sketch: one synthetic genome of 5 Mbp, k 26 (the defaults of `krepp sketch`).
usage: time_seek_pairs.py [--parent ROOT] [--out out.txt] [kernels|cli|cut|all]"""
import os, re, subprocess, sys, tempfile, time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
args = sys.argv[1:]


def opt(name, default=None):
    if name in args:
        i = args.index(name)
        v = args[i + 1]
        del args[i:i + 2]
        return v
    return default


parent = opt("--parent")
out_path = opt("--out")
root = opt("--root", HERE)  # (the legs' own processes: the build whose library they load)
work = opt("--work")
what = args[0] if args else "all"
sys.path.insert(0, root)
import numpy as np
from krepp_amd import capi

lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ACGT = np.frombuffer(b"ACGT", np.uint8)
rng = np.random.default_rng(23)
G = 5_000_000
genome = ACGT[rng.integers(0, 4, G)]
REC = 314  # "@r%07d\n" + 150 + "\n+\n" + 150 + "\n"


def sketch(work):
    fa, skc = os.path.join(work, "g.fa"), os.path.join(work, "g.skc")
    if not os.path.exists(skc):
        with open(fa, "wb") as f:
            f.write(b">g\n" + genome.tobytes() + b"\n")
        capi.build_sketch(fa, skc)
    return skc


def mate_chunks(n, first=0):
    """n pairs as two [n, REC] arrays: a mate is a piece of the genome with 1 % substitutions or random, the four combinations in turn"""
    out = []
    for mate in (0, 1):
        a = np.empty((n, REC), np.uint8)
        a[:, 0], a[:, 1] = ord("@"), ord("r")
        num = np.arange(first, first + n)
        for j in range(7):
            a[:, 8 - j] = 48 + (num // 10 ** j) % 10
        a[:, 9] = 10
        seq = genome[rng.integers(0, G - 150, n)[:, None] + np.arange(150)[None, :]]
        hit = rng.random(seq.shape) < 0.01
        seq[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
        rnd = ((np.arange(n) >> mate) & 1) == 1  # mate 0: every other pair; mate 1: every other two pairs
        seq[rnd] = ACGT[rng.integers(0, 4, (int(rnd.sum()), 150))]
        a[:, 10:160] = seq
        a[:, 160:163] = np.frombuffer(b"\n+\n", np.uint8)
        a[:, 163:313] = 33 + rng.integers(0, 41, (n, 150))
        a[:, 163] = ord("I")  # (a quality line never begins with '@')
        a[:, 313] = 10
        out.append(a)
    return out


def med(xs):
    return float(np.median(xs))


def leg(kind):
    """one process: `pair` -- two deferring streams and one pair call per round; `unpaired` -- two streams that split their own batch"""
    skc = sketch(work)
    hx = capi.HostIndex(skc, sketch=True)
    dx = hx.upload(0)
    n = (64 << 20) // REC
    c1, c2 = mate_chunks(n)
    raws = (c1.tobytes(), c2.tobytes())
    sts = []
    for raw in raws:
        st = dx.stream(params=capi.default_params(hdist_th=4), max_reads=n + 1024, max_bases=len(raw) + 64)
        st.seek_enable(max(1 << 20, 32 * n), max(1 << 20, 16 * n))
        st.fastq_enable(len(raw) + 64)
        st.extract_enable()
        if kind == "pair":
            st.extract_defer(True)
        sts.append(st)
    t = []
    for rnd in range(7):
        for st, raw in zip(sts, raws):
            fp = st.submit_fastq(raw, capi.KR_SEEK | capi.KR_TILE_DEVICE)
            assert fp["nreads"] == n and fp["consumed"] == len(raw), fp
        if kind == "pair":
            sts[0].extract_pair(sts[1], capi.KR_PAIR_ANY)
        for st in sts:
            st.wait()
        ms = sts[0].extract_ms() if kind == "pair" else sts[0].extract_ms() + sts[1].extract_ms()
        if rnd >= 2:
            t.append(ms)
    d1, d2 = sts[0].collect_seek()["d"], sts[1].collect_seek()["d"]
    keep = (~np.isnan(d1) | ~np.isnan(d2)) if kind == "pair" else None
    for st, c, d in zip(sts, (c1, c2), (d1, d2)):
        k = keep if kind == "pair" else ~np.isnan(d)
        ex = st.collect_extract()
        assert ex["matched"] == c[k].tobytes() and ex["unmatched"] == c[~k].tobytes(), "the split differs from the one made on the host"
    print(f"LEG {kind} median {med(t):.4f} min {min(t):.4f} max {max(t):.4f} matched {int((keep if kind == 'pair' else ~np.isnan(d1)).sum())} of {n}", flush=True)


def kernels():
    say(f"== (a) 2 x 64 MB of 150-base FASTQ, {(64 << 20) // REC} pairs; ms of kernels per round (HIP events), medians of five rounds after two warm-ups; the legs alternate, a process each")
    say(f"   pair: one kr_batch_extract_pair (pair kernel + 2 x 4 extract kernels), this build; unpaired: two unpaired extracts, {'the build at ' + parent if parent else 'this build, defer off'}")
    res = {"pair": [], "unpaired": []}
    for rnd in range(3):
        for kind in ("pair", "unpaired"):
            r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", parent if kind == "unpaired" and parent else HERE, "--work", work, "leg-" + kind],
                               capture_output=True, text=True, timeout=600)
            assert r.returncode == 0, r.stderr
            l = [x for x in r.stdout.splitlines() if x.startswith("LEG ")][0]
            res[kind].append(float(l.split()[3]))
            say(f"   round {rnd + 1}: {l[4:]}")
    say(f"   pair call: {'  '.join(f'{x:.3f}' for x in res['pair'])} ms (median {med(res['pair']):.3f});  two unpaired extracts: {'  '.join(f'{x:.3f}' for x in res['unpaired'])} ms (median {med(res['unpaired']):.3f})")


def cli():
    skc = sketch(work)
    exe = os.path.join(HERE, "krepp_amd", "lib", "krepp")
    pexe = os.path.join(parent, "krepp_amd", "lib", "krepp") if parent else exe
    q1, q2 = os.path.join(work, "R1.fq"), os.path.join(work, "R2.fq")
    npairs = 2_000_000
    with open(q1, "wb") as f1, open(q2, "wb") as f2:
        for first in range(0, npairs, 250_000):
            c1, c2 = mate_chunks(250_000, first)
            f1.write(c1.tobytes()), f2.write(c2.tobytes())
    say(f"== (b) CLI: {npairs} pairs of 150-base reads, 2 x {os.path.getsize(q1)} bytes of plain FASTQ; krepp seek --gpu-parse --gpu-seek, wall seconds per run and (query phase)")
    f = {k: os.path.join(work, k) for k in ("m1", "u1", "m2", "u2", "rep1", "rep2")}
    base = ["--gpu-parse", "--gpu-seek"]
    paired = [exe, "seek", "-i", skc, "-q", q1, "--query2", q2, "-o", f["rep1"], "--output-path2", f["rep2"], "--extract-matched", f["m1"], "--extract-unmatched", f["u1"],
              "--extract-matched2", f["m2"], "--extract-unmatched2", f["u2"]] + base
    un1 = [pexe, "seek", "-i", skc, "-q", q1, "-o", f["rep1"], "--extract-matched", f["m1"], "--extract-unmatched", f["u1"]] + base
    un2 = [pexe, "seek", "-i", skc, "-q", q2, "-o", f["rep2"], "--extract-matched", f["m2"], "--extract-unmatched", f["u2"]] + base

    def run(cmd):
        t0 = time.perf_counter()
        r = subprocess.run(cmd, capture_output=True, env=dict(os.environ, KR_CLI_TIMING="1"), timeout=900)
        wall = time.perf_counter() - t0
        err = r.stderr.decode()
        assert r.returncode == 0, err
        return wall, float(re.search(r"Done seeking query sequences, elapsed: ([\d.e+-]+) sec", err).group(1)), err

    walls, phases = {"paired": [], "unpaired x 2": []}, {"paired": [], "unpaired x 2": []}
    for rnd in range(3):
        w, p, err = run(paired)
        walls["paired"].append(w), phases["paired"].append(p)
        if rnd == 2:
            for l in err.splitlines():
                if l.startswith("[timing] extract") or l.startswith("[timing] parse"):
                    say(f"    (paired) {l}")
        (w1, p1, _), (w2, p2, _) = run(un1), run(un2)
        walls["unpaired x 2"].append(w1 + w2), phases["unpaired x 2"].append(p1 + p2)
    for k in walls:
        say(f"  {k}: wall " + "  ".join(f"{x:.2f}" for x in walls[k]) + f" s (median {med(walls[k]):.2f});  query phase " + "  ".join(f"{x:.3f}" for x in phases[k]) + f" s (median {med(phases[k]):.3f})")
    say(f"  unpaired x 2: the sum of the two runs ({'the build at ' + parent if parent else 'this build'}), each with its own sketch load")


def cut():
    n = (64 << 20) // REC
    c1, c2 = mate_chunks(n)
    a, b = c1.tobytes(), c2.tobytes()
    lib = capi.load()
    ca, cb, nr = capi.C.c_uint64(0), capi.C.c_uint64(0), capi.C.c_uint32(0)
    ts = []
    for _ in range(7):
        t0 = time.perf_counter()
        capi.check(lib.kr_fastq_pair_cut(a, len(a), b, len(b), 1 << 30, capi.C.byref(ca), capi.C.byref(cb), capi.C.byref(nr)))
        ts.append(time.perf_counter() - t0)
    assert nr.value == n and ca.value == len(a) and cb.value == len(b)
    t1 = []
    for _ in range(7):  # max_records at a CLI batch's 65,536: the cutter stops there
        t0 = time.perf_counter()
        capi.check(lib.kr_fastq_pair_cut(a, len(a), b, len(b), 65536, capi.C.byref(ca), capi.C.byref(cb), capi.C.byref(nr)))
        t1.append(time.perf_counter() - t0)
    say(f"== (c) kr_fastq_pair_cut, one thread: 2 x {len(a)} bytes of 314-byte records in {med(ts) * 1e3:.2f} ms (median of 7): {(len(a) + len(b)) / med(ts) / 1e9:.2f} GB/s; "
        f"stopping at 65,536 records ({ca.value + cb.value} bytes): {med(t1) * 1e3:.2f} ms, {(ca.value + cb.value) / med(t1) / 1e9:.2f} GB/s")


if what.startswith("leg-"):
    leg(what[4:])
    sys.exit(0)
work = work or tempfile.mkdtemp(prefix="krepp_pairs_")
if what in ("kernels", "all"):
    kernels()
if what in ("cli", "all"):
    cli()
if what in ("cut", "all"):
    cut()
if out_path:
    with open(out_path, "a") as f:
        f.write("\n".join(lines) + "\n")
