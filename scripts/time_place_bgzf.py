#!/usr/bin/env python3
"""`place` text deflated on the device against the host encoder, on the 1000-genome index with its own Yule tree as backbone
(docs/design/15 section 15.7).  Three measurements in one session:
  1  the deflate kernels alone on real place text (jplace and tabular, 65,536 and 400,000 reads, taken once from a plain call):
     kr_debug_bgzf_deflate at levels 1 and 2 and member lengths 65,280 / 32,640 / 16,320 / 8,160, kr_debug_bgzf_deflate_ms of
     repetitions 1-3, the compressed size, and kr_bgzf_deflate_host_member's wall time for the same text on the host's threads
  2  a 400,000-read call through the C ABI, arms alternating, two warm-up calls and six timed: the plain call; the plain call +
     kr_bgzf_deflate_host_level of its text (what `krepp place --bgzf-out` does without --gpu-deflate); kr_stream_place_bgzf at the
     best member length of measurement 1 and at 65,280
  3  krepp place [--tabular] on a file of reads, 65,536-read batches, two workers, to a file, three alternating rounds: another
     build's binary with --bgzf-out (optional: the parent commit's), this build's with --bgzf-out, with --bgzf-out --gpu-deflate,
     and with --bgzf-out --gpu-deflate --bgzf-member <best>
usage: time_place_bgzf.py [reads of the CLI file, default 4,000,000; 0: skip measurement 3] [path of the other build's krepp]"""
import ctypes as C
import gzip
import os, re, subprocess, sys, tempfile, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
from krepp_amd import capi, synth
n_cli = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000
other_exe = sys.argv[2] if len(sys.argv) > 2 else None
MEMBERS = (65280, 32640, 16320, 8160)
def say(*a):
    print(" ".join(str(x) for x in a), flush=True)
def stats(v):
    v = sorted(v)
    return "min %.2f median %.2f max %.2f (n=%d)" % (v[0], v[len(v) // 2], v[-1], len(v))
t0 = time.time()
work = tempfile.mkdtemp(prefix="krepp_pb_")
nwk_text = synth.yule_newick(1000, 2)
genomes = synth.evolve_genomes(nwk_text, 100_000, seed=2)
open(work + "/y.nwk", "w").write(nwk_text)
tsv = synth.write_genomes(genomes, work + "/g")
idx = work + "/idx"
say("genomes written %.1f s" % (time.time() - t0))
capi.build_index(tsv, idx, nwk=work + "/y.nwk", k=29, w=35, h=13, m=4, r=1, frac=True, num_threads=16)
say("index built %.1f s" % (time.time() - t0))

lib = capi.load()
hx = capi.HostIndex(idx)
NR = 400_000
b400 = np.concatenate([synth.sample_reads(genomes, 100_000, seed=7000 + i)[0] for i in range(4)])[:NR * 150]
offs = (np.arange(NR + 1, dtype=np.uint64) * np.uint64(150))
names = [b"r%d" % i for i in range(NR)]
arr = (C.c_char_p * NR)(*names)

def place_call(pl, nr, tabular, keep=False):
    """one kr_batch_submit + kr_place_stream of the first nr reads as the first call of a file: (seconds, text or its length)"""
    pl.prev = C.c_int(0)
    txt, ln = C.c_void_p(), C.c_uint64()
    t = time.perf_counter()
    capi.check(lib.kr_batch_submit(pl.st.h, b400.ctypes.data, offs.ctypes.data, nr, capi.KR_TAP_ACCS))
    capi.check(lib.kr_place_stream(pl.hx.h, pl.dx.h, pl.pt, pl.st.h, nr, offs.ctypes.data, arr, C.byref(pl.popts), tabular, C.byref(pl.prev), C.byref(txt), C.byref(ln), None, None))
    dt = time.perf_counter() - t
    out = C.string_at(txt, ln.value) if keep else int(ln.value)
    return dt, out, txt

# ---- 1: the kernels alone on real place text
texts = {}
for tabular in (0, 1):
    pl = capi.Placer(hx, None, 0, tabular=tabular, max_reads=NR, max_bases=NR * 150 + 64)
    for nr in (65536, NR):
        _, text, txt = place_call(pl, nr, tabular, keep=True)
        lib.kr_free(txt)
        texts[("tabular" if tabular else "jplace", nr)] = text
    pl.close()
dx = hx.upload(0)
st = dx.stream(max_reads=64, max_bases=1 << 16)
st.text_enable(hx, 1 << 16, 1 << 12)
st.bgzf_out_enable()
st.bgzf_deflate_ms()  # (makes the events: the next deflate is the first measured)
kernel_ms = {}
for (kind, nr), text in texts.items():
    for level in (1, 2):
        st.bgzf_out_level(level)
        for L in MEMBERS:
            st.bgzf_member(L)
            ms, comp = [], b""
            for rep in range(3):
                comp = st.bgzf_deflate(text)
                ms.append(st.bgzf_deflate_ms())
            ht = []
            for rep in range(3):
                t = time.perf_counter()
                hcomp = capi.bgzf_deflate_host_member(text, level, L)
                ht.append((time.perf_counter() - t) * 1e3)
            assert hcomp == comp, "the device's members are not the host encoder's"
            kernel_ms[(kind, nr, level, L)] = sorted(ms)[1]
            say("1 kernels", kind, nr, "reads, text %d bytes, level %d, member %5d: %6d members, device ms reps 1-3: %s, compressed %d (%.4f of the text), %.2f GB/s at the median; host encoder ms (%d threads, 3 reps): %s"
                % (len(text), level, L, -(-len(text) // L), " ".join("%.3f" % x for x in ms), len(comp), len(comp) / len(text), len(text) / sorted(ms)[1] / 1e6,
                   int(os.environ.get("OMP_NUM_THREADS", "0")) or os.cpu_count(), " ".join("%.1f" % x for x in ht)))
st.bgzf_member(65280)
st.close(), dx.close()
best = min(MEMBERS, key=lambda L: kernel_ms[("jplace", NR, 1, L)])
best_cli = min(MEMBERS, key=lambda L: kernel_ms[("jplace", 65536, 1, L)])
say("1 best member length at level 1 on jplace text: %d at 400,000 reads, %d at 65,536 reads" % (best, best_cli))

# ---- 2: a 400,000-read call through the C ABI
for tabular in (0, 1):
    arms = ["plain", "plain + host encoder", "device, member %d" % best, "device, member 65280"]
    pls = {k: capi.Placer(hx, None, 0, tabular=tabular, max_reads=NR, max_bases=NR * 150 + 64) for k in arms}
    pls[arms[2]].st.place_bgzf(1), pls[arms[2]].st.bgzf_member(best)
    pls[arms[3]].st.place_bgzf(1)
    res, size = {k: [] for k in arms}, {}
    plain_text = texts[("tabular" if tabular else "jplace", NR)]
    for rep in range(8):
        for k in arms:
            dt, out, txt = place_call(pls[k], NR, tabular, keep=(rep == 0))
            if k == arms[1]:
                t = time.perf_counter()
                ln = out if rep else len(out)
                cap = capi.bgzf_deflate_bound(ln)
                buf = np.empty(cap, np.uint8)
                cl = C.c_uint64(0)
                capi.check(lib.kr_bgzf_deflate_host_level(txt, ln, 1, buf.ctypes.data, cap, C.byref(cl)))
                dt += time.perf_counter() - t
                size[k] = int(cl.value)
            lib.kr_free(txt)
            if rep == 0:
                if k in arms[:2]:
                    assert out == plain_text
                else:
                    assert gzip.decompress(out) == plain_text, "the members do not inflate to the plain call's text"
                    size[k] = len(out)
            if rep >= 2:  # (two warm-up calls: workspaces grow)
                res[k].append(dt * 1e3)
    for k in arms:
        say("2 C ABI", "tabular" if tabular else "jplace", "%-26s" % k, "ms per 400,000-read call:", stats(res[k]), "text %.1f MB" % (len(plain_text) / 1e6), ("-> %.1f MB" % (size[k] / 1e6)) if k in size else "")
    for pl in pls.values():
        pl.close()
say("2 counters: ranges deflated on the device %d, by the library's host encoder %d" % capi.place_bgzf_counters())

# ---- 3: the CLI
if n_cli:
    fq = work + "/reads.fq"
    with open(fq, "wb") as f:
        done = 0
        while done < n_cli:
            m = min(200_000, n_cli - done)
            b = np.concatenate([synth.sample_reads(genomes, min(100_000, m - o), seed=7000 + (done + o) // 100_000)[0] for o in range(0, m, 100_000)])
            r = b.reshape(m, 150)
            f.write(b"".join(b"@r%d\n" % (done + i) + r[i].tobytes() + b"\n+\n" + b"I" * 150 + b"\n" for i in range(m)))
            done += m
    say("reads written", n_cli, "%.1f s" % (time.time() - t0))
    exe = os.path.join(root, "krepp_amd", "lib", "krepp")
    arms = ([("other build --bgzf-out", other_exe, ["--bgzf-out"])] if other_exe else []) + [
        ("this build --bgzf-out", exe, ["--bgzf-out"]),
        ("this build --bgzf-out --gpu-deflate", exe, ["--bgzf-out", "--gpu-deflate"]),
        ("this build --bgzf-out --gpu-deflate --bgzf-member %d" % best_cli, exe, ["--bgzf-out", "--gpu-deflate", "--bgzf-member", str(best_cli)]),
        ("this build, plain text", exe, []),
    ]
    res, sizes = {}, {}
    for rep in range(3):
        for extra in ([], ["--tabular"]):
            for name, binary, flags in arms:
                t = time.time()
                r = subprocess.run([binary, "place", "-i", idx, "-q", fq, "-o", work + "/out.gz"] + extra + flags, capture_output=True, text=True, env=dict(os.environ, KR_CLI_TIMING="1"), timeout=600)
                dt = time.time() - t
                assert r.returncode == 0, r.stderr
                el = float(re.search(r"elapsed: ([0-9.e+-]+) sec", r.stderr).group(1))
                key = (" ".join(extra) or "jplace") + ": " + name
                res.setdefault(key, []).append(el)
                sizes[key] = os.path.getsize(work + "/out.gz")
                line = [l for l in r.stderr.splitlines() if l.startswith("[timing] bgzf-out")]
                say("3 CLI", key, "round", rep, "elapsed %.3f s, whole process %.2f s, file %.1f MB" % (el, dt, sizes[key] / 1e6), line[0] if line else "")
    for k, v in res.items():
        say("3 CLI", k, "%d reads: elapsed s" % n_cli, stats(v), "-> %.2f M reads/s at the median, file %.1f MB" % (n_cli / sorted(v)[len(v) // 2] / 1e6, sizes[k] / 1e6))
say("done %.1f s" % (time.time() - t0))
