#!/usr/bin/env python3
"""What splitting a seek batch's reads on the device costs (kr_stream_extract_enable; docs/design/13_seek.md 13.6).
  1. kernels: kr_debug_extract_ms per chunk, beside kr_debug_fastq_parse_ms and kr_debug_seek_ms of the SAME batches, for a 64 MB chunk
     of 150-base FASTQ (half the reads mutated pieces of the sketched genome, half random) and a 64 MB chunk of sixteen one-line FASTA
     records of 4 MB (every other one a piece of the genome) -- each in a process with the copy kernel's wide stores (a lane whose 16
     bytes lie in one record stores them at once) and in one with byte stores only (KR_EXTRACT_STORE=1, read once per process), and
     the host clock around collect_extract.
     Both parts are checked against a split made here.
  2. CLI: `krepp seek --gpu-parse --gpu-seek` on one FASTQ file of 2 M reads without the extract flags, with both files plain and with
     both files --extract-bgzf: three alternating rounds in this one session, wall time of each run.
Sketch: one synthetic genome of 5 Mbp, k 26 (the defaults of `krepp sketch`).
usage: time_seek_extract.py [out.txt] [kernels|cli|all]"""
import os, subprocess, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from krepp_amd import capi

out_path = sys.argv[1] if len(sys.argv) > 1 else None
what = sys.argv[2] if len(sys.argv) > 2 else "all"
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


ACGT = np.frombuffer(b"ACGT", np.uint8)
rng = np.random.default_rng(19)
G = 5_000_000
genome = ACGT[rng.integers(0, 4, G)]
work = tempfile.mkdtemp(prefix="krepp_extract_")
fa, skc = os.path.join(work, "g.fa"), os.path.join(work, "g.skc")
with open(fa, "wb") as f:
    f.write(b">g\n" + genome.tobytes() + b"\n")
capi.build_sketch(fa, skc)
REC = 314  # "@r%07d\n" + 150 + "\n+\n" + 150 + "\n"


def fastq_chunk(n, first=0):
    """n records of REC bytes as an [n, REC] array: even reads are pieces of the genome with 1 % substitutions, odd ones random"""
    a = np.empty((n, REC), np.uint8)
    a[:, 0] = ord("@")
    a[:, 1] = ord("r")
    num = np.arange(first, first + n)
    for j in range(7):
        a[:, 8 - j] = 48 + (num // 10 ** j) % 10
    a[:, 9] = 10
    seq = genome[rng.integers(0, G - 150, n)[:, None] + np.arange(150)[None, :]]
    hit = rng.random(seq.shape) < 0.01
    seq[hit] = ACGT[rng.integers(0, 4, int(hit.sum()))]
    seq[1::2] = ACGT[rng.integers(0, 4, (len(seq[1::2]), 150))]
    a[:, 10:160] = seq
    a[:, 160:163] = np.frombuffer(b"\n+\n", np.uint8)
    a[:, 163:313] = 33 + rng.integers(0, 41, (n, 150))
    a[:, 163] = ord("I")  # (a quality line never begins with '@')
    a[:, 313] = 10
    return a


def med(xs):
    return float(np.median(xs))


def kernels():
    hx = capi.HostIndex(skc, sketch=True)
    dx = hx.upload(0)
    n = (64 << 20) // REC
    fq = fastq_chunk(n)
    fq_recs = [fq]  # (the expectation below indexes rows)
    recs_fa = []
    for i in range(16):
        body = genome[(i * 60_000) % (G - (4 << 20)):][: 4 << 20].copy() if i % 2 == 0 else ACGT[rng.integers(0, 4, 4 << 20)]
        recs_fa.append(b">c%02d\n" % i + body.tobytes() + b"\n")
    legs = (("64 MB of 150-base FASTQ", fq.tobytes(), "fastq", n), ("64 MB of 4 MB one-line FASTA records", b"".join(recs_fa), "fasta", 16))
    for name, raw, fmt, nrec in legs:
        st = dx.stream(params=capi.default_params(hdist_th=4), max_reads=nrec + 1024, max_bases=len(raw) + 64)
        st.seek_enable(max(1 << 20, 32 * nrec), max(1 << 20, 16 * nrec))
        st.fastq_enable(len(raw) + 64)
        st.extract_enable()
        ms = capi.C.c_float(0)
        capi.check(st.lib.kr_debug_fastq_parse_ms(st.h, capi.C.byref(ms)))  # (the first call makes the events)
        submit = st.submit_fastq if fmt == "fastq" else st.submit_fasta
        say(f"== {name}: {len(raw)} bytes, {nrec} records")
        for label in (("byte stores" if os.environ.get("KR_EXTRACT_STORE") == "1" else "wide stores"),):
            t = {k: [] for k in ("parse", "hist", "solve", "text", "extract", "collect")}
            for rnd in range(7):
                fp = submit(raw, capi.KR_SEEK | capi.KR_TILE_DEVICE)
                assert fp["nreads"] == nrec and fp["consumed"] == len(raw), fp
                st.wait()
                t0 = time.perf_counter()
                ex = st.collect_extract()
                t1 = time.perf_counter()
                capi.check(st.lib.kr_debug_fastq_parse_ms(st.h, capi.C.byref(ms)))
                sm = st.seek_ms()
                if rnd >= 2:
                    t["parse"].append(ms.value), t["hist"].append(sm[0]), t["solve"].append(sm[1]), t["text"].append(sm[2])
                    t["extract"].append(st.extract_ms()), t["collect"].append((t1 - t0) * 1e3)
            m = ~np.isnan(st.collect_seek()["d"])
            if fmt == "fastq":
                wm, wu = fq_recs[0][m].tobytes(), fq_recs[0][~m].tobytes()
            else:
                wm, wu = b"".join(r for r, k in zip(recs_fa, m) if k), b"".join(r for r, k in zip(recs_fa, m) if not k)
            assert ex["matched"] == wm and ex["unmatched"] == wu, "the split differs from the one made on the host"
            say(f"  {label}: parse {med(t['parse']):7.3f} ms   seek hist {med(t['hist']):7.3f} + solve {med(t['solve']):7.3f} + text {med(t['text']):7.3f} ms   "
                f"extract {med(t['extract']):7.3f} ms (min {min(t['extract']):.3f}, {len(raw) / med(t['extract']) / 1e6:.1f} GB/s of chunk)   "
                f"collect_extract (both parts to page-locked memory + Python copies) {med(t['collect']):8.3f} ms   matched {int(m.sum())} of {nrec}")
        st.close()


def cli():
    exe = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "krepp_amd", "lib", "krepp")
    q = os.path.join(work, "reads.fq")
    nreads = 2_000_000
    with open(q, "wb") as f:
        for first in range(0, nreads, 250_000):
            f.write(fastq_chunk(250_000, first).tobytes())
    say(f"== CLI: {nreads} reads of 150 bases, {os.path.getsize(q)} bytes of FASTQ; krepp seek --gpu-parse --gpu-seek -o report, wall seconds per run")
    m, u = os.path.join(work, "m.fq"), os.path.join(work, "u.fq")
    variants = (("no extract flags", []), ("--extract-matched + --extract-unmatched, plain", ["--extract-matched", m, "--extract-unmatched", u]),
                ("--extract-matched + --extract-unmatched --extract-bgzf", ["--extract-matched", m + ".gz", "--extract-unmatched", u + ".gz", "--extract-bgzf"]))
    secs = {v[0]: [] for v in variants}
    for rnd in range(3):
        for label, extra in variants:
            t0 = time.perf_counter()
            r = subprocess.run([exe, "seek", "-i", skc, "-q", q, "--gpu-parse", "--gpu-seek", "-o", os.path.join(work, "report.txt")] + extra,
                               capture_output=True, env=dict(os.environ, KR_CLI_TIMING="1"), timeout=900)
            secs[label].append(time.perf_counter() - t0)
            assert r.returncode == 0, r.stderr.decode()
            if rnd == 2:
                for l in r.stderr.decode().splitlines():
                    if l.startswith("[timing] extract") or l.startswith("Done seeking"):
                        say(f"    ({label}) {l}")
    for label, _ in variants:
        say(f"  {label}: " + "  ".join(f"{x:.2f}" for x in secs[label]) + f" s   (median {med(secs[label]):.2f})")
    say(f"  extract files: plain {os.path.getsize(m)} + {os.path.getsize(u)} bytes, BGZF {os.path.getsize(m + '.gz')} + {os.path.getsize(u + '.gz')} bytes")


if what == "kernels-one":  # (the library reads KR_EXTRACT_STORE once per process: a process per store width)
    kernels()
if what in ("kernels", "all"):
    for store in ("16", "1"):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "", "kernels-one"], capture_output=True, text=True, env=dict(os.environ, KR_EXTRACT_STORE=store))
        assert r.returncode == 0, r.stderr
        for l in r.stdout.splitlines():
            if l.startswith("== ") or l.startswith("  "):
                say(l)
if what in ("cli", "all"):
    cli()
if out_path:
    with open(out_path, "a" if what == "cli" else "w") as f:
        f.write("\n".join(lines) + "\n")
