#!/usr/bin/env python3
"""The way OUT of a batch that runs as tiles (one long sequence is enough): report text of the same host batch through the C ABI
  (a) kr_batch_submit_text without KR_TILE_ROWS -> kr_batch_collect_text says KR_ERR_UNSUPPORTED -> kr_batch_collect (record slots)
      + kr_format_dist on the host: the only path before the flag existed,
  (b) kr_batch_submit_text with KR_TILE_ROWS -> kr_batch_collect_text: compact rows and the text written by the device,
  (c) shape (i) WITHOUT its contig -> kr_batch_collect_text (an untiled batch, for orientation),
in alternating rounds of one process, bases and offsets in page-locked memory (KR_BASES_PINNED), ids staged by the submit, host clock
around submit + the collect that yields the text.  Shapes: (i) 65,536 reads of 150 bases and one 5,000-base contig, (ii) 2,000 contigs
of 5 kb.  Index: 25 references of 400 kb (k27 / w35 / h11), as scripts/time_device_contigs.py.  (a) and (c) use nothing newer than
kr_batch_submit_text, so the script also runs where the flag does not exist yet, and leaves (b) out there.
usage: time_tiled_text.py [rounds]"""
import ctypes as C
import os, sys, tempfile, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
from krepp_amd import capi, synth
rounds = int(sys.argv[1]) if len(sys.argv) > 1 else 9
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
work = tempfile.mkdtemp(prefix="krepp_ttxt_")
nwk = os.path.join(root, "tests", "golden", "tree_toy.nwk")
g = synth.evolve_genomes(open(nwk).read(), 400_000, seed=7)
tsv = synth.write_genomes(g, os.path.join(work, "g"))
idx = os.path.join(work, "idx")
capi.build_index(tsv, idx, nwk=nwk, k=27, w=35, h=11, m=4, r=1, frac=True, num_threads=8)
gl = list(g.values())
hx = capi.HostIndex(idx)
dx = hx.upload(0)
lib = capi.load()
TILE_ROWS = getattr(capi, "KR_TILE_ROWS", None)
print(f"KR_TILE_ROWS: {'present' if TILE_ROWS else 'missing: arm (b) is left out'}", flush=True)


def contigs(L, nc, seed):  # stretches of the references with 1 % substitutions
    rng = np.random.default_rng(seed)
    seqs = []
    for i in range(nc):
        o = int(rng.integers(0, 400_000 - L + 1))
        s = gl[i % len(gl)][o:o + L].copy()
        mut = rng.random(len(s)) < 0.01
        s[mut] = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, int(mut.sum()))]
        seqs.append(s)
    return seqs


class Batch:
    """bases and offsets in page-locked memory, the ids packed as kr_batch_submit_text takes them, the names as kr_format_dist does"""

    def __init__(self, seqs, prefix):
        n, nb = len(seqs), sum(len(s) for s in seqs)
        self.n, self.nb = n, nb
        self.p_bases, self.p_offs = lib.kr_host_alloc(max(nb, 1)), lib.kr_host_alloc(8 * (n + 1))
        assert self.p_bases and self.p_offs
        np.ctypeslib.as_array((C.c_uint8 * nb).from_address(self.p_bases))[:] = np.concatenate(seqs)
        np.ctypeslib.as_array((C.c_uint64 * (n + 1)).from_address(self.p_offs))[:] = np.cumsum([0] + [len(s) for s in seqs])
        enc = [b"%s%d" % (prefix, i) for i in range(n)]
        self.ids = np.frombuffer(b"\0".join(enc) + b"\0", np.uint8)
        self.id_off = np.zeros(n + 1, np.uint32)
        np.cumsum([len(e) + 1 for e in enc], out=self.id_off[1:])
        self.names = (C.c_char_p * n)(*enc)

    def free(self):
        lib.kr_host_free(self.p_bases), lib.kr_host_free(self.p_offs)


def stream_for(b):
    vmax = b.nb // 128 + b.n + 1024
    st = dx.stream(max_reads=vmax, max_bases=b.nb + 64, max_records=vmax * 64)
    st.text_enable(hx, max(32 << 20, b.n * 1536), max(1 << 20, b.n * 64))
    return st


def submit(st, b, flags):
    capi.check(lib.kr_batch_submit_text(st.h, b.p_bases, b.p_offs, b.n, capi.KR_BASES_PINNED | flags, b.ids.ctypes.data, b.id_off.ctypes.data, 1))


def device_text(st, keep):
    txt, ln = C.c_void_p(), C.c_uint64()
    capi.check(lib.kr_batch_collect_text(st.h, C.byref(txt), C.byref(ln)))
    return (C.string_at(txt, ln.value) if keep else None), ln.value + 16  # (the text and its 16-byte summary cross PCIe)


def host_text(st, b, keep):
    txt, ln = C.c_void_p(), C.c_uint64()
    assert lib.kr_batch_collect_text(st.h, C.byref(txt), C.byref(ln)) == capi.KR_ERR_UNSUPPORTED
    rv = capi.KrResultView()
    capi.check(lib.kr_batch_collect(st.h, C.byref(rv)))
    capi.check(lib.kr_format_dist(hx.h, C.byref(rv), b.names, C.byref(txt), C.byref(ln)))
    out = C.string_at(txt, ln.value) if keep else None
    lib.kr_free(txt)
    return out, 9 * rv.nreads + 13 * rv.nrecs  # (read_off / read_cnt / read_na, and key, flag, DIST of every record slot)


def ms(xs):
    return f"median {np.median(xs) * 1e3:8.2f} ms  min {min(xs) * 1e3:8.2f} ms"


reads = contigs(150, 65_536, 5)
shapes = (("(i) 65,536 reads of 150 bases + one 5,000-base contig", reads[:32_768] + contigs(5_000, 1, 3) + reads[32_768:], reads),
          ("(ii) 2,000 contigs of 5 kb", contigs(5_000, 2000, 3), None))
for what, seqs, untiled in shapes:
    b = Batch(seqs, b"q")
    arms = {"a": (b, 0)}
    if TILE_ROWS:
        arms["b"] = (b, TILE_ROWS)
    if untiled:
        arms["c"] = (Batch(untiled, b"q"), 0)
    st = {a: stream_for(bb) for a, (bb, fl) in arms.items()}
    t_all, text, d2h, rep = {a: [] for a in arms}, {}, {}, {}
    for rnd in range(rounds + 3):  # two warm-up rounds (code objects, buffers made on first use), `rounds` timed ones, and one more
        keep = rnd == rounds + 2   # whose text is kept and compared (a copy inside the window: that round is not counted)
        for a, (bb, fl) in arms.items():
            t0 = time.perf_counter()
            submit(st[a], bb, fl)
            text[a], d2h[a] = host_text(st[a], bb, keep) if a == "a" else device_text(st[a], keep)
            t1 = time.perf_counter()
            if 2 <= rnd < rounds + 2:
                t_all[a].append(t1 - t0)
            rep[a] = st[a].last_d2h_bytes()
    if "b" in arms:
        assert text["a"] == text["b"] and len(text["a"]) > 0, "the device's text differs from the host formatter's"
    lay = st["a"].tile_layout(b.n)
    print(f"== {what}: {b.n} reads, {lay['nv']} in the tiled batch, {len(text['a'])} bytes of report, {rounds} rounds", flush=True)
    label = {"a": "record slots + kr_format_dist   ", "b": "KR_TILE_ROWS + device text      ", "c": "no contig: untiled, device text "}
    for a in arms:
        print(f"  ({a}) {label[a]}: {ms(t_all[a])}   D2H {d2h[a]:>10} bytes (kr_debug_last_d2h_bytes after the last kr_batch_collect: {rep[a]})", flush=True)
    for s_ in st.values():
        s_.close()
    for bb in {id(x[0]): x[0] for x in arms.values()}.values():
        bb.free()
