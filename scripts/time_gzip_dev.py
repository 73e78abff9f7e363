#!/usr/bin/env python3
"""`krepp dist --no-multi -o FILE` on ordinary gzip reads: --gpu-parse alone (gzip keeps the host reader: kr_pgz.inc, the baseline,
code this feature does not touch) against --gpu-parse --gpu-inflate (the file inflated on the GPU, docs/design/08 "Ordinary gzip on
the device").  Reads of 150 bases as `gzip -1` and `gzip -6`, in the page cache.  Arms alternating in one session, four rounds of which
the first is dropped; min / median / max of the other three.  From the device arm's [timing] lines: the four kernels' device time per
super-chunk (by events), the share of the search kernel (it decodes every first block a second time), the copies, and the CLI's
own device-time figures of both arms side by side (what the inflater's kernels do to the scan when both are on the chip).
usage: time_gzip_dev.py [reads, default 4,000,000]"""
import os, re, subprocess, sys, tempfile, time, zlib
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
from krepp_amd import synth
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000
def say(*a):
    print(" ".join(str(x) for x in a), flush=True)
def main():
    t0 = time.time()
    work = tempfile.mkdtemp(prefix="krepp_gzdev_")
    genomes = synth.evolve_genomes(open(os.path.join(root, "tests", "golden", "tree_toy.nwk")).read(), 20000, seed=7)
    idx = os.path.join(root, "tests", "golden", "toy_index")
    exe = os.path.join(root, "krepp_amd", "lib", "krepp")
    rng = np.random.RandomState(5)
    files = {level: open(work + "/reads_l%d.fq.gz" % level, "wb") for level in (1, 6)}
    comp = {level: zlib.compressobj(level, zlib.DEFLATED, 31) for level in files}
    done = raw_bytes = 0
    while done < n:
        m = min(100_000, n - done)
        r = synth.sample_reads(genomes, m, seed=7000 + done // 100_000)[0].reshape(m, 150)
        q = (33 + np.minimum(40, rng.geometric(0.12, size=(m, 150)) + 20)).astype(np.uint8)  # spread-out qualities, mostly high
        text = b"".join(b"@r%d\n" % (done + i) + r[i].tobytes() + b"\n+\n" + q[i].tobytes() + b"\n" for i in range(m))
        done += m
        raw_bytes += len(text)
        for level, f in files.items():
            f.write(comp[level].compress(text))
    for level, f in files.items():
        f.write(comp[level].flush())
        f.close()
    say("reads written:", n, "reads,", raw_bytes, "bytes of FASTQ;", {l: os.path.getsize(f.name) for l, f in files.items()}, "bytes as gzip; %.1f s" % (time.time() - t0))
    arms = {"--gpu-parse (host gzip reader)": ["--gpu-parse"], "--gpu-parse --gpu-inflate": ["--gpu-parse", "--gpu-inflate"]}
    for level, f in files.items():
        res = {}
        for rep in range(4):
            for key, flags in arms.items():
                t = time.time()
                r = subprocess.run([exe, "dist", "-i", idx, "-q", f.name, "--no-multi", "-o", work + "/out.tsv"] + flags, capture_output=True, text=True,
                                   env=dict(os.environ, KR_CLI_TIMING="1"), timeout=900)
                dt = time.time() - t
                assert r.returncode == 0, r.stderr
                el = float(re.search(r"elapsed: ([0-9.e+-]+) sec", r.stderr).group(1))
                if rep >= 1:  # (first round: page cache, clocks)
                    res.setdefault(key, []).append(el)
                found = re.search(r"gpu-parse: (\d+)", r.stderr)
                say("CLI level", level, key, "rep", rep, "elapsed %.3f s, whole process %.2f s, device records %s, out %.1f MB" % (el, dt, found.group(1) if found else "-", os.path.getsize(work + "/out.tsv") / 1e6))
                if rep == 1:
                    for l in r.stderr.splitlines():
                        if l.startswith("[timing]"):
                            say("   ", l)
                m_ = re.search(r"gpu-inflate: (\d+) super-chunks, (\d+) sub-chunks linked, (\d+) without a start, (\d+) dropped, host ranges (\d+); kernels: search ([0-9.]+) ms, decode ([0-9.]+) ms, chain ([0-9.]+) ms, resolve ([0-9.]+) ms; copies ([0-9.]+) ms", r.stderr)
                if m_ and rep >= 1:
                    sc = int(m_.group(1))
                    k = [float(m_.group(i)) for i in range(6, 11)]
                    say("KERNELS level", level, "rep", rep, "%d super-chunks, %s linked, %s without a start, %s dropped, %s host ranges; per super-chunk: search %.2f ms, decode %.2f ms, chain %.2f ms, resolve %.2f ms (search: %.0f %% of the kernels' time); copies %.2f ms; %.2f GB/s of inflated bytes through the kernels"
                        % (sc, m_.group(2), m_.group(3), m_.group(4), m_.group(5), k[0] / sc, k[1] / sc, k[2] / sc, k[3] / sc, 100 * k[0] / sum(k[:4]), k[4] / sc, raw_bytes / sum(k[:4]) / 1e6))
        for k, v in res.items():
            v = sorted(v)
            say("RESULT level", level, k, "%d reads: elapsed min %.3f s median %.3f s max %.3f s -> %.2f M reads/s at the minimum" % (n, v[0], v[len(v) // 2], v[-1], n / v[0] / 1e6))
    say("done %.1f s" % (time.time() - t0))
if __name__ == "__main__":
    main()
