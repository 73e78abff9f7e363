#!/usr/bin/env python3
"""`krepp dist --no-multi -o FILE` on block-gzipped reads: the host BGZF reader (no flag; the baseline, code this feature does not touch)
against --gpu-parse (members inflated on the GPU, docs/design/08 "BGZF on the device").  Arms alternating in one session, four rounds
of which the first is dropped; min / median / max of the other three.  Beside it the inflate kernel alone: kr_debug_bgzf_ms per
chunk of about 32 MB of inflated bytes, as GB/s of inflated bytes.
usage: time_bgzf.py [reads, default 4,000,000] [indexes: toy | toy,syn1000]   (syn1000: the 1000-genome index, built here first)"""
import multiprocessing, os, re, struct, subprocess, sys, tempfile, time, zlib
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root)
import numpy as np
from krepp_amd import capi, synth
n = int(float(sys.argv[1])) if len(sys.argv) > 1 else 4_000_000
which = sys.argv[2].split(",") if len(sys.argv) > 2 else ["toy"]
BLOCK = 0xff00  # bgzip's member size
def say(*a):
    print(" ".join(str(x) for x in a), flush=True)
def member(args):
    data, level = args
    co = zlib.compressobj(level, zlib.DEFLATED, -15)
    p = co.compress(data) + co.flush()
    return b"\x1f\x8b\x08\x04" + b"\x00" * 4 + b"\x00\xff" + struct.pack("<H", 6) + b"BC" + struct.pack("<HH", 2, len(p) + 25) + p + struct.pack("<II", zlib.crc32(data) & 0xFFFFFFFF, len(data))
def main():
    t0 = time.time()
    work = tempfile.mkdtemp(prefix="krepp_bgzf_")
    toy_nwk = open(os.path.join(root, "tests", "golden", "tree_toy.nwk")).read()
    indexes, sources = {}, {}
    if "toy" in which:
        indexes["toy"], sources["toy"] = os.path.join(root, "tests", "golden", "toy_index"), synth.evolve_genomes(toy_nwk, 20000, seed=7)
    if "syn1000" in which:
        nwk_text = synth.yule_newick(1000, 2)
        genomes = synth.evolve_genomes(nwk_text, 100_000, seed=2)
        open(work + "/y.nwk", "w").write(nwk_text)
        capi.build_index(synth.write_genomes(genomes, work + "/g"), work + "/idx", nwk=work + "/y.nwk", k=29, w=35, h=13, m=4, r=1, frac=True, num_threads=16)
        indexes["syn1000"], sources["syn1000"] = work + "/idx", genomes
        say("1000-genome index built %.1f s" % (time.time() - t0))
    exe = os.path.join(root, "krepp_amd", "lib", "krepp")
    pool = multiprocessing.Pool(16)
    for name, idx in indexes.items():
        files = {}
        for level in (1, 6):
            files[level] = open(work + "/%s_l%d.fq.gz" % (name, level), "wb")
        done = raw_bytes = 0
        carry = b""
        while done < n:
            m = min(200_000, n - done)
            b = np.concatenate([synth.sample_reads(sources[name], min(100_000, m - o), seed=7000 + (done + o) // 100_000)[0] for o in range(0, m, 100_000)])
            r = b.reshape(m, 150)
            text = carry + b"".join(b"@r%d\n" % (done + i) + r[i].tobytes() + b"\n+\n" + b"I" * 150 + b"\n" for i in range(m))
            done += m
            whole = len(text) if done >= n else len(text) // BLOCK * BLOCK
            carry = text[whole:]
            raw_bytes += whole
            blocks = [text[i:i + BLOCK] for i in range(0, whole, BLOCK)]
            for level, f in files.items():
                f.write(b"".join(pool.map(member, [(x, level) for x in blocks], chunksize=64)))
        for level, f in files.items():
            f.write(member((b"", level)))
            f.close()
        say(name, "reads written:", n, "reads,", raw_bytes, "bytes of FASTQ;", {l: os.path.getsize(f.name) for l, f in files.items()}, "bytes as BGZF; %.1f s" % (time.time() - t0))
        for level, f in files.items():
            res = {}
            for rep in range(4):
                for gp in ([], ["--gpu-parse"]):
                    t = time.time()
                    r = subprocess.run([exe, "dist", "-i", idx, "-q", f.name, "--no-multi", "-o", work + "/out.tsv"] + gp, capture_output=True, text=True, env=dict(os.environ, KR_CLI_TIMING="1"), timeout=900)
                    dt = time.time() - t
                    assert r.returncode == 0, r.stderr
                    el = float(re.search(r"elapsed: ([0-9.e+-]+) sec", r.stderr).group(1))
                    key = "--gpu-parse (inflate on the GPU)" if gp else "host BGZF reader"
                    if rep >= 1:  # (first round: page cache, clocks)
                        res.setdefault(key, []).append(el)
                    found = re.search(r"gpu-parse: (\d+)", r.stderr)
                    say("CLI", name, "level", level, key, "rep", rep, "elapsed %.3f s, whole process %.2f s, device records %s, out %.1f MB" % (el, dt, found.group(1) if found else "-", os.path.getsize(work + "/out.tsv") / 1e6))
                    if rep == 0:
                        say("   ", [l for l in r.stderr.splitlines() if l.startswith("[timing] parse")])
            for k, v in res.items():
                v = sorted(v)
                say("RESULT", name, "level", level, k, "%d reads: elapsed min %.3f s median %.3f s max %.3f s -> %.2f M reads/s at the minimum" % (n, v[0], v[len(v) // 2], v[-1], n / v[0] / 1e6))
    pool.close()
    # ---- the kernel alone: chunks of about 32 MB of inflated bytes
    hx = capi.HostIndex(os.path.join(root, "tests", "golden", "toy_index"))
    dx = hx.upload(0)
    st = dx.stream(capi.default_params(), max_reads=1024, max_bases=1 << 16)
    st.fastq_enable(40 << 20)
    st.bgzf_enable(40 << 20)
    st.bgzf_ms()
    for level, f in files.items():
        comp = open(f.name, "rb").read()
        off, rates = 0, []
        while off < len(comp) and len(rates) < 12:
            k, cb, u = capi.bgzf_walk(comp[off:off + (40 << 20)], 32 << 20)
            if k == 0:
                break
            out = st.bgzf_inflate(comp[off:off + cb], cap=u)
            ms = st.bgzf_ms()
            assert len(out) == u
            if len(rates) == 0:
                assert out == zlib.decompress(comp[off:off + capi.bgzf_member_size(comp[off:])], 31) + out[BLOCK:]
            rates.append(u / ms / 1e6)
            off += cb
        v = sorted(rates[1:])
        say("RESULT kernel level", level, "%d chunks of ~32 MB inflated (%d members each): GB/s of inflated bytes min %.2f median %.2f max %.2f" % (len(v), k, v[0], v[len(v) // 2], v[-1]))
    say("done %.1f s" % (time.time() - t0))
if __name__ == "__main__":
    main()
