"""Helpers of the seek-kernel tests (test_seek_abi.py, test_gpu_seek_kernels.py): the three sketches, the crafted reads, and a brute
force of src/seek.cpp:58-121 from the sketch as the oracle reads it -- per k-mer and strand the minimum Hamming distance over ONE
bucket, counted into hdist_th + 1 bins; onmers = the valid k-mers.

The brute force exists twice.  `brute_hist` is the literal one: closed_form / row_of of tests/helpers.py per k-mer, a Python loop per
bucket.  `brute_hist_np` is the same arithmetic on numpy arrays, for the reads of tens and hundreds of thousands of positions; the
tests run both on the short reads and require them to agree before the fast one is trusted on the long ones."""
import numpy as np

from helpers import closed_form, hd32, revcomp, row_of

# sketch A: tests/test_seek.py's (same genome seed, same positions); B: 32 rows, long buckets; C: m not a power of two, one residue
CFG_A = dict(k=21, w=27, h=7, m=4, r=1, frac=True, ppos=[20, 19, 17, 13, 6, 4, 2])
CFG_B = dict(k=19, w=25, h=3, m=4, r=1, frac=True, ppos=[17, 9, 3])
CFG_C = dict(k=21, w=27, h=7, m=3, r=0, frac=False, ppos=[20, 19, 17, 13, 6, 4, 2])
ACGT = np.frombuffer(b"ACGT", np.uint8)
_CODE = np.full(256, 4, np.uint8)
for _i, _c in enumerate(b"ACGT"):
    _CODE[_c] = _i
    _CODE[_c + 32] = _i
_POP16 = np.array([bin(i).count("1") for i in range(1 << 16)], np.uint8)


def random_dna(rng, n):
    return rng.choice(ACGT, n).tobytes().decode()


def genome_a():
    """the contigs of tests/test_seek.py's sketch"""
    rng = np.random.default_rng(11)
    return [random_dna(rng, n) for n in (9000, 40, 6000, 20)]


def write_sketch(capi, d, name, contigs, cfg):
    fa, sk = d / (name + ".fa"), d / (name + ".skc")
    fa.write_text("".join(f">c{i}\n{c}\n" for i, c in enumerate(contigs)))
    capi.build_sketch(fa, sk, **cfg)
    return str(sk)


def mutate(rng, s, rate):
    a = np.frombuffer(s.encode(), np.uint8).copy()
    hit = rng.random(len(a)) < rate
    a[hit] = (np.searchsorted(ACGT, a[hit]) + rng.integers(1, 4, int(hit.sum()))) % 4  # a substitution always changes the base
    a[hit] = ACGT[a[hit]]
    return a.tobytes().decode()


def pack(reads):
    bases = np.frombuffer("".join(reads).encode("latin-1"), np.uint8)
    offs = np.cumsum([0] + [len(r) for r in reads]).astype(np.uint64)
    return bases, offs


def buckets(sk):
    """row -> residual codes of the bucket, from the oracle's reader (inc: the buckets' ends)"""
    ends = sk.inc.astype(np.int64)
    starts = np.concatenate([[0], ends[:-1]])
    return starts, ends


def brute_hist(sk, reads, th):
    """hist [n, 2, th + 1], onmers [n]: closed_form / row_of per k-mer, the minimum over the bucket in a Python loop"""
    starts, ends = buckets(sk)
    codes = sk.codes.tolist()
    hist = np.zeros((len(reads), 2, th + 1), np.uint32)
    onmers = np.zeros(len(reads), np.uint32)
    frac = bool(sk.frac)
    for n, s in enumerate(reads):
        for i in range(len(s) - sk.k + 1):
            km = s[i:i + sk.k]
            f = closed_form(km, sk.ppos, sk.npos)
            if f is None:
                continue
            onmers[n] += 1
            for strand, g in ((0, f), (1, closed_form(revcomp(km), sk.ppos, sk.npos))):
                row = row_of(g[2], sk.m, sk.r, frac)
                if row is None or row >= len(ends):
                    continue
                best = min((hd32(c, g[3]) for c in codes[starts[row]:ends[row]]), default=99)
                if best <= th:
                    hist[n, strand, best] += 1
    return hist, onmers


def front_end_np(s, k, ppos, npos):
    """valid [npos], rix [2, npos], enc32 [2, npos] of every k-mer position of the sequence (bytes); position p of a k-mer counts from
    its LAST base, the reverse strand is the complement read backwards"""
    a = np.frombuffer(s if isinstance(s, bytes) else s.encode("latin-1"), np.uint8)
    npz = len(a) - k + 1
    if npz <= 0:
        return np.zeros(0, bool), np.zeros((2, 0), np.uint32), np.zeros((2, 0), np.uint32)
    c = _CODE[a].astype(np.uint32)
    bad = np.concatenate([[0], np.cumsum(c >= 4)])
    valid = (bad[k:] - bad[:-k]) == 0
    P, N = sorted(int(x) for x in ppos), sorted(int(x) for x in npos)
    rix, enc = np.zeros((2, npz), np.uint32), np.zeros((2, npz), np.uint32)
    for j, p in enumerate(P):
        rix[0] |= (c[k - 1 - p:k - 1 - p + npz] & 3) << (2 * j)
        rix[1] |= ((3 - c[p:p + npz]) & 3) << (2 * j)
    for j, p in enumerate(N):
        f, r = c[k - 1 - p:k - 1 - p + npz] & 3, (3 - c[p:p + npz]) & 3
        enc[0] |= ((f & 1) << j) | ((f >> 1) << (16 + j))
        enc[1] |= ((r & 1) << j) | ((r >> 1) << (16 + j))
    return valid, rix, enc


def brute_hist_np(sk, reads, th):
    """brute_hist on arrays: the j-th entry of every position's bucket at once, j up to the longest bucket"""
    starts, ends = buckets(sk)
    codes = np.concatenate([sk.codes.astype(np.uint32), np.zeros(1, np.uint32)])
    hist = np.zeros((len(reads), 2, th + 1), np.uint32)
    onmers = np.zeros(len(reads), np.uint32)
    for n, s in enumerate(reads):
        valid, rix, enc = front_end_np(s, sk.k, sk.ppos, sk.npos)
        onmers[n] = int(valid.sum())
        for strand in (0, 1):
            res, q = rix[strand] % sk.m, rix[strand] // sk.m
            if sk.frac:
                ok, row = valid & (res <= sk.r), q * (sk.r + 1) + res
            else:
                ok, row = valid & (res == sk.r), q
            ok &= row < len(ends)
            row, e = row[ok].astype(np.int64), enc[strand][ok]
            b0, ln = starts[row], ends[row] - starts[row]
            best = np.full(len(row), 99, np.uint8)
            for j in range(int(ln.max()) if len(ln) else 0):
                has = j < ln
                z = codes[np.where(has, b0 + j, len(codes) - 1)] ^ e
                hd = _POP16[(z | (z >> 16)) & 0xFFFF]
                best = np.where(has, np.minimum(best, hd), best)
            hist[n, strand] = np.bincount(best[best <= th], minlength=th + 1)[:th + 1]
    return hist, onmers


def hist_of_taps(res, nreads, th):
    """hist [n, 2, th + 1] from a KR_TAP_ACCS batch of the dist path on the sketch (one record per strand that matched)"""
    hist = np.zeros((nreads, 2, th + 1), np.uint32)
    for r, key, h in zip(res.rec_read.tolist(), res.rec_key.tolist(), res.rec_hist):
        assert key >> 1 == 1  # the sketch's one leaf
        hist[r, key & 1] += h
    return hist


def fastq_of(names, reads):
    return "".join(f"@{n}\n{s}\n+\n{'I' * len(s)}\n" for n, s in zip(names, reads)).encode()


def fasta_of(names, reads):
    return "".join(f">{n}\n{s}\n" for n, s in zip(names, reads)).encode()
