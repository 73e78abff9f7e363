"""Shared by test_sdust.py and test_gpu_sdust.py: the recorded sdust() fixture, the fuzz sequence, and the literal pure-Python walk
of RSeq::extract_mers WITH its sdust interval walk (src/rqseq.cpp:71-140)."""
import json
import os

import numpy as np

from helpers import closed_form, row_of

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = json.load(open(os.path.join(HERE, "golden", "sdust_ref.json")))
SEQS = {n: s.encode("latin-1") for n, s in FIXTURE["sequences"].items()}
PARAMS = [tuple(p) for p in FIXTURE["params"]]
# sequences whose intervals the reference saves out of order of start, so that its list is not the union of what it saved
OUT_OF_ORDER = list(FIXTURE["saved_out_of_order"])


def fixture_lists(T, W, names):
    return [[tuple(iv) for iv in FIXTURE["intervals"]["%d,%d" % (T, W)][n]] for n in names]


def pack(contigs):
    """contigs: bytes objects -> (bases u8, offsets u64)"""
    bases = np.frombuffer(b"".join(contigs), np.uint8)
    offs = np.cumsum([0] + [len(c) for c in contigs]).astype(np.uint64)
    return bases, offs


def low_complexity(rng, n):
    """A stretch of n bases: homopolymer, period 2..7 repeat or two-letter text, with a few substitutions."""
    kind = int(rng.integers(0, 3))
    if kind == 0:
        s = np.full(n, rng.integers(0, 4))
    elif kind == 1:
        unit = rng.integers(0, 4, int(rng.integers(2, 8)))
        s = np.resize(unit, n)
    else:
        s = rng.choice(rng.choice(4, 2, replace=False), n)
    s = s.copy()
    for p in rng.choice(n, max(1, n // 40), replace=False):
        s[p] = rng.integers(0, 4)
    return s


def implant(rng, codes, count, lo=40, hi=400):
    """count low-complexity stretches written into the base codes `codes` (0..3) at random places; returns their starts."""
    starts = sorted(int(p) for p in rng.integers(0, len(codes) - hi, count))
    for p in starts:
        n = int(rng.integers(lo, hi))
        codes[p:p + n] = low_complexity(rng, n)
    return starts


def fuzz_sequence(seed=77, n=200_000):
    """About 200 kb: random DNA, ~250 implanted low-complexity stretches, sparse N (1 in 400), and N runs of 300..1500 bases,
    half of them cut into a stretch so that the window behind the run still holds the words in front of it."""
    rng = np.random.default_rng(seed)
    codes = rng.integers(0, 4, n)
    starts = implant(rng, codes, 250)
    text = np.frombuffer(b"ACGT", np.uint8)[codes].copy()
    text[rng.random(n) < 1 / 400] = ord("N")
    for j in range(24):
        p = starts[j * 10] + 30 if j % 2 == 0 else int(rng.integers(0, n - 2000))
        text[p:p + int(rng.integers(300, 1500))] = ord("N")
    return text.tobytes()


def fmix(x):
    x ^= x >> 33
    x = (x * 0xff51afd7ed558ccd) & 0xFFFFFFFFFFFFFFFF
    x ^= x >> 33
    x = (x * 0xc4ceb9fe1a85ec53) & 0xFFFFFFFFFFFFFFFF
    return x ^ (x >> 33)


def masked_ring_buffer_sim(contigs, intervals, k, w, m, r, frac, ppos, npos):
    """tests/test_minimizers.py's ring_buffer_sim extended with the interval walk, line by line as src/rqseq.cpp:71-140 has it.
    contigs: str; intervals: per contig [(start, finish), ...].  Returns (sorted unique keys, per-contig (c1 hashes, c2 hashes),
    per-contig dict of what happened: skipped k-mers, intervals passed, 'ended_skipping', 'short_final_emit')."""
    keys, sketches, seen = set(), [], []
    P, N = sorted(ppos), sorted(npos)
    for t, rgs in zip(contigs, intervals):
        if len(t) < w:
            continue
        ldiff = w - k + 1
        win = [(0, 0)] * ldiff
        kix = l = 0
        c1, c2 = [], []
        what = dict(skipped=0, passed=0, ended_skipping=False, short_final_emit=False)
        mn, mi = len(rgs), 0
        mrs, mre = 0, len(t)
        if mn > 0:
            mrs, mre = rgs[0]
        i = 0
        while i < len(t):
            ch = t[i]
            if ch not in "ACGTacgt":
                l = 0
                i += 1
                continue
            l += 1
            i += 1
            if l < k:
                continue
            f = closed_form(t[i - k:i], ppos, npos)
            if mi < mn and i + k > mrs:
                c1.append(fmix(f[0]) & 0xFFFFFFFF)
                what["skipped"] += 1
                if i < mre:
                    what["ended_skipping"] = i == len(t)
                    continue
                mi += 1
                l = 0
                what["passed"] += 1
                if mi < mn:
                    mrs, mre = rgs[mi]
                continue
            win[kix % ldiff] = (f[0], fmix(f[0]))
            c1.append(win[kix % ldiff][1] & 0xFFFFFFFF)
            kix += 1
            if l < w and i != len(t):
                continue
            if l < w:
                what["short_final_emit"] = True
            x, z = min(win, key=lambda e: e[1])
            c2.append(z & 0xFFFFFFFF)
            codes = [(x >> (2 * p)) & 3 for p in range(k)]
            rix = sum(codes[P[j]] << (2 * j) for j in range(len(P)))
            enc = sum(((codes[N[j]] & 1) << j) | ((codes[N[j]] >> 1) << (16 + j)) for j in range(len(N)))
            row = row_of(rix, m, r, frac)
            if row is not None:
                keys.add((row << 32) | enc)
        sketches.append((c1, c2))
        seen.append(what)
    return np.array(sorted(keys), dtype=np.uint64), sketches, seen


def hll12(hashes):
    reg = np.zeros(4096, np.int64)
    for h in hashes:
        ix, rest = h >> 20, (h << 12) & 0xFFFFFFFF
        lz = 32 - rest.bit_length() if rest else 32
        reg[ix] = max(reg[ix], min(20, lz) + 1)
    mreg = 4096.0
    est = (0.7213 / (1.0 + 1.079 / mreg)) * mreg * mreg / float(np.sum(1.0 / (1 << reg)))
    zeros = int((reg == 0).sum())
    if est <= 2.5 * mreg and zeros:
        est = mreg * np.log(mreg / zeros)
    return est
