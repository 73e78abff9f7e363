#!/usr/bin/env python3
"""`place` with the reads given as raw FASTQ bytes against `place` from host arrays, on the 1000-genome index with its own Yule tree
as backbone (docs/design/06, docs/design/08).  Two comparisons, arms alternating within one process / one session:
  C ABI   kr_batch_submit + kr_place_stream from host arrays  vs  kr_batch_submit_fastq + kr_place_stream_parsed from page-locked
          file bytes, 400,000 reads a call, tabular and jplace text, two warm-up calls then six timed
  CLI     krepp place [--tabular] with the host reader  vs  --gpu-parse, same file, four rounds of which the first is dropped
usage: time_place_parsed.py [reads of the CLI file, default 4,000,000]"""
import ctypes as C
import os, re, subprocess, sys, tempfile, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
from krepp_amd import capi, synth
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000
def say(*a):
    print(" ".join(str(x) for x in a), flush=True)
t0 = time.time()
work = tempfile.mkdtemp(prefix="krepp_pp_")
nwk_text = synth.yule_newick(1000, 2)
genomes = synth.evolve_genomes(nwk_text, 100_000, seed=2)
open(work + "/y.nwk", "w").write(nwk_text)
tsv = synth.write_genomes(genomes, work + "/g")
idx = work + "/idx"
say("genomes written %.1f s" % (time.time() - t0))
capi.build_index(tsv, idx, nwk=work + "/y.nwk", k=29, w=35, h=13, m=4, r=1, frac=True, num_threads=16)
say("index built %.1f s" % (time.time() - t0))
fq = work + "/reads.fq"
first = None
with open(fq, "wb") as f:
    done = 0
    while done < n:
        m = min(200_000, n - done)
        b = np.concatenate([synth.sample_reads(genomes, min(100_000, m - o), seed=7000 + (done + o) // 100_000)[0] for o in range(0, m, 100_000)])
        r = b.reshape(m, 150)
        if first is None:
            first = b.copy()
        f.write(b"".join(b"@r%d\n" % (done + i) + r[i].tobytes() + b"\n+\n" + b"I" * 150 + b"\n" for i in range(m)))
        done += m
        if done % 1_000_000 == 0:
            say("reads written", done, "%.1f s" % (time.time() - t0))

# ---- C ABI: 400,000 reads a call
lib = capi.load()
hx = capi.HostIndex(idx)
NR = 400_000
b400 = np.concatenate([first, synth.sample_reads(genomes, 100_000, seed=8001)[0], synth.sample_reads(genomes, 100_000, seed=8002)[0]])[:NR * 150]
offs = (np.arange(NR + 1, dtype=np.uint64) * np.uint64(150))
names = [b"r%d" % i for i in range(NR)]
arr = (C.c_char_p * NR)(*names)
rows = b400.reshape(NR, 150)
raw = b"".join(b"@r%d\n" % i + rows[i].tobytes() + b"\n+\n" + b"I" * 150 + b"\n" for i in range(NR))
pinned = lib.kr_host_alloc(len(raw))
C.memmove(pinned, raw, len(raw))
for tabular in (1, 0):
    res = {"host": [], "parsed": []}
    pls = {k: capi.Placer(hx, None, 0, tabular=tabular, max_reads=NR, max_bases=NR * 150 + 64) for k in res}
    pls["parsed"].st.fastq_enable(len(raw))
    texts = {}
    for rep in range(8):
        for k in ("host", "parsed"):
            pl = pls[k]
            pl.prev = C.c_int(0)
            txt, ln = C.c_void_p(), C.c_uint64()
            t = time.perf_counter()
            if k == "host":
                capi.check(lib.kr_batch_submit(pl.st.h, b400.ctypes.data, offs.ctypes.data, NR, capi.KR_TAP_ACCS))
                capi.check(lib.kr_place_stream(pl.hx.h, pl.dx.h, pl.pt, pl.st.h, NR, offs.ctypes.data, arr, C.byref(pl.popts), tabular, C.byref(pl.prev), C.byref(txt), C.byref(ln), None, None))
            else:
                fp = capi.KrFastqParse()
                capi.check(lib.kr_batch_submit_fastq(pl.st.h, pinned, len(raw), capi.KR_TAP_ACCS, 1, C.byref(fp)))
                assert fp.nreads == NR, fp.nreads
                capi.check(lib.kr_place_stream_parsed(pl.hx.h, pl.dx.h, pl.pt, pl.st.h, pinned, C.byref(pl.popts), tabular, C.byref(pl.prev), C.byref(txt), C.byref(ln), None, None))
            dt = time.perf_counter() - t
            if rep == 0:
                texts[k] = C.string_at(txt, ln.value)
            lib.kr_free(txt)
            if rep >= 2:  # (two warm-up calls: workspaces grow)
                res[k].append(dt * 1e3)
    assert texts["host"] == texts["parsed"], "outputs differ"
    for k in res:
        v = sorted(res[k])
        say("C ABI", "tabular" if tabular else "jplace", k, "ms per 400,000-read call: min %.1f median %.1f max %.1f (n=%d), text %.1f MB" % (v[0], v[len(v) // 2], v[-1], len(v), len(texts[k]) / 1e6))
    for pl in pls.values():
        pl.close()
lib.kr_host_free(pinned)

# ---- CLI, interleaved
exe = os.path.join(root, "krepp_amd", "lib", "krepp")
res = {}
for rep in range(4):
    for extra in (["--tabular"], []):
        for gp in ([], ["--gpu-parse"]):
            t = time.time()
            r = subprocess.run([exe, "place", "-i", idx, "-q", fq, "-o", work + "/out.txt"] + extra + gp, capture_output=True, text=True, env=dict(os.environ, KR_CLI_TIMING="1"), timeout=300)
            dt = time.time() - t
            assert r.returncode == 0, r.stderr
            el = float(re.search(r"elapsed: ([0-9.e+-]+) sec", r.stderr).group(1))
            key = (" ".join(extra) or "jplace") + (" --gpu-parse" if gp else " host reader")
            if rep >= 1:  # (first round: page cache, clocks)
                res.setdefault(key, []).append(el)
            found = re.search(r"gpu-parse: (\d+)", r.stderr)
            say("CLI", key, "rep", rep, "elapsed %.3f s, whole process %.2f s, device records %s, out %.1f MB" % (el, dt, found.group(1) if found else "-", os.path.getsize(work + "/out.txt") / 1e6))
            if rep == 0:
                say("   ", [l for l in r.stderr.splitlines() if l.startswith("[timing] parse")])
for k, v in res.items():
    v = sorted(v)
    say("CLI", k, "%d reads: elapsed min %.3f s median %.3f s max %.3f s -> %.2f M reads/s at the minimum" % (n, v[0], v[len(v) // 2], v[-1], n / v[0] / 1e6))
say("done %.1f s" % (time.time() - t0))
