#!/usr/bin/env python3
"""FASTA records found on the GPU (kr_batch_submit_fasta, kr_dev_fasta.inc) against the sequential host reader, on the same bytes:
  (i)  64 MB of 150-base reads as two-line FASTA,
  (ii) 64 MB of 1 Mb contigs wrapped at 60 columns,
through the C ABI, in alternating rounds of one process after two warm-up rounds, host clock:
  (a) the kr_batch_submit_fasta call (copy to HBM, parse kernels, wait for the 64-byte summary; with KR_TILE_DEVICE it also lays
      the tiles out and waits for that summary), then kr_batch_collect: time to rows; the parse kernels alone by device events
      (kr_debug_fastq_parse_ms),
  (b) kr_fastx_next over the file until its end (the reader alone), then kr_batch_submit + kr_batch_collect: time to rows.
What to expect: (ii) costs within a small factor of (i) per byte in (a) -- every pass is parallel over bytes; a large factor would
mean a pass is serial in the record length.  Then `krepp dist` on both files with and without --gpu-parse (whole process), and,
when KR_BASELINE_EXE names the `krepp` of the commit before kr_batch_submit_fasta, that build's --gpu-parse (which falls back to
the host reader at byte 0).  Index: the toy index of tests/golden.
usage: time_fasta_parse.py [rounds] [megabytes]"""
import ctypes as C
import os, subprocess, sys, tempfile, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
from krepp_amd import capi, synth
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 7
mbytes = int(sys.argv[2]) if len(sys.argv) > 2 else 64
work = tempfile.mkdtemp(prefix="krepp_fa_")
golden = os.path.join(root, "tests", "golden")
idx = os.path.join(golden, "toy_index")
g = synth.evolve_genomes(open(os.path.join(golden, "tree_toy.nwk")).read(), 20000, seed=7)
lib = capi.load()
hx = capi.HostIndex(idx)
dx = hx.upload(0)
k = hx.view.k


def reads_fasta(nbytes):
    n = nbytes // 160
    bases, offs, _ = synth.sample_reads(g, n, seed=3)
    b = bases.tobytes()
    return b"".join(b">r%d\n" % i + b[int(offs[i]):int(offs[i + 1])] + b"\n" for i in range(n)), n


def contigs_fasta(nbytes):
    rng = np.random.default_rng(5)
    gl = list(g.values())
    out, n = [], 0
    while sum(len(x) for x in out) < nbytes:
        s = np.concatenate([gl[int(rng.integers(0, len(gl)))] for _ in range(50)])  # 1 Mb of reference stretches, 1 % substitutions
        mut = rng.random(len(s)) < 0.01
        s[mut] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(mut.sum()))]
        body = s.tobytes()
        out.append(b">contig%d\n" % n + b"\n".join(body[j:j + 60] for j in range(0, len(body), 60)) + b"\n")
        n += 1
    return b"".join(out), n


def ms(xs):
    return f"median {np.median(xs) * 1e3:8.2f} ms  min {min(xs) * 1e3:8.2f} ms"


def reader_alone(path):
    """kr_fastx_open .. kr_fastx_next until the end: seconds, records"""
    h = C.c_void_p()
    t0 = time.perf_counter()
    capi.check(lib.kr_fastx_open(os.fsencode(path), C.byref(h)))
    n = 0
    while True:
        b = capi.KrFastxBatch()
        capi.check(lib.kr_fastx_next(h, 1 << 40, C.byref(b)))
        n += b.nreads
        if not b.more:
            break
    dt = time.perf_counter() - t0
    lib.kr_fastx_close(h)
    return dt, n


files = {}
for what, make in (("(i)  150-base reads, two lines a record", reads_fasta), ("(ii) 1 Mb contigs wrapped at 60", contigs_fasta)):
    raw, nrec = make(mbytes << 20)
    path = os.path.join(work, "q%d.fa" % len(files))
    open(path, "wb").write(raw)
    files[what] = path
    names, bases, offs = capi.read_fastx(path)
    assert len(names) == nrec
    vmax = int(len(bases) // 128 + nrec + 1024)
    fl = capi.KR_ROWS_ONLY | capi.KR_TILE_DEVICE
    a = dx.stream(max_reads=vmax, max_bases=len(bases) + 64, max_records=vmax * 64)
    b = dx.stream(max_reads=vmax, max_bases=len(bases) + 64, max_records=vmax * 64)
    a.fastq_enable(len(raw))
    s = a.submit_fasta(raw, fl)  # (the wrapper's page-locked copy of `raw` is kept: the timed calls below give it to the C call as it is)
    assert (s["nreads"], s["status"], s["nbases"]) == (nrec, capi.KR_FASTQ_OK, len(bases)), s
    rows_a = a.collect().rows()
    pm = C.c_float(0)
    lib.kr_debug_fastq_parse_ms(a.h, C.byref(pm))  # (the first call makes the events; the next parse is measured)
    t_sub, t_rows_a, t_kern, t_read, t_rows_b = [], [], [], [], []
    rows_b = None
    for rnd in range(rounds + 2):
        out = capi.KrFastqParse()
        t0 = time.perf_counter()
        capi.check(lib.kr_batch_submit_fasta(a.h, a._pinned, len(raw), fl, 1, C.byref(out)))
        t1 = time.perf_counter()
        rv = a.collect_view()
        t2 = time.perf_counter()
        capi.check(lib.kr_debug_fastq_parse_ms(a.h, C.byref(pm)))
        t3 = time.perf_counter()
        dt_read, n = reader_alone(path)
        assert n == nrec
        b.submit(bases, offs, capi.KR_ROWS_ONLY)
        res = b.collect()
        t4 = time.perf_counter()
        if rnd == rounds + 1:
            rows_b = res.rows()
        if rnd >= 2:
            t_sub.append(t1 - t0), t_rows_a.append(t2 - t0), t_kern.append(pm.value / 1e3), t_read.append(dt_read), t_rows_b.append(t4 - t3)
    assert rows_a == rows_b and len(rows_a) > 0, "the two arms' rows differ"
    print(f"== {what}: {len(raw) / 1e6:.1f} MB, {nrec} records, {len(bases) / 1e6:.1f} Mb, {len(rows_a)} rows, {rounds} rounds", flush=True)
    print(f"  (a) kr_batch_submit_fasta call:      {ms(t_sub)}   ({len(raw) / np.median(t_sub) / 1e9:.2f} GB/s)", flush=True)
    print(f"      its parse kernels alone (events): {ms(t_kern)}   ({len(raw) / np.median(t_kern) / 1e9:.2f} GB/s)", flush=True)
    print(f"      submit + collect, time to rows:   {ms(t_rows_a)}", flush=True)
    print(f"  (b) the host reader alone:            {ms(t_read)}   ({len(raw) / np.median(t_read) / 1e9:.2f} GB/s)", flush=True)
    print(f"      reader + submit + collect:        {ms(t_rows_b)}", flush=True)
    a.close()
    b.close()

exe = os.path.join(root, "krepp_amd", "lib", "krepp")
arms = [("host reader", exe, []), ("--gpu-parse", exe, ["--gpu-parse"])]
if os.environ.get("KR_BASELINE_EXE"):
    arms.append(("--gpu-parse, the build before this call", os.environ["KR_BASELINE_EXE"], ["--gpu-parse"]))
for what, path in files.items():
    outs, times = {}, {a[0]: [] for a in arms}
    for rnd in range(4):
        for name, x, extra in arms:
            o = os.path.join(work, "out.tsv")
            t0 = time.perf_counter()
            r = subprocess.run([x, "dist", "-i", idx, "-q", path, "-o", o, "--gpus", "1"] + extra, capture_output=True, timeout=600)
            dt = time.perf_counter() - t0
            assert r.returncode == 0, r.stderr.decode()[-2000:]
            outs[name] = open(o, "rb").read().split(b"\n", 1)[1]
            if rnd:
                times[name].append(dt)
    assert len(set(outs.values())) == 1, "the reports differ"
    print(f"== krepp dist --gpus 1, {what}: {len(outs['host reader'])} bytes of report, whole process (3 runs after one warm-up)")
    for name, xs in times.items():
        print(f"  {name}: {ms(xs)}", flush=True)
