"""Inputs and checks for level 2 of the BGZF encoder (dynamic Huffman codes): shared by test_bgzf_deflate_dyn_host.py and
test_gpu_bgzf_deflate_dyn.py.  deflate_cases.py has the inputs of level 1, which level 2 takes as well."""
import functools
import heapq

import numpy as np

import deflate_cases as dc


def de_bruijn(k, n):
    """the de Bruijn sequence B(k, n) as a list of symbols 0 .. k - 1 (Lyndon words in order)"""
    a, seq = [0] * (k * n), []

    def db(t, p):
        if t > n:
            if n % p == 0:
                seq.extend(a[1:p + 1])
        else:
            a[t] = a[t - p]
            db(t + 1, p)
            for j in range(a[t - p] + 1, k):
                a[t] = j
                db(t + 1, t)

    db(1, 1)
    return seq


def rare_counts(tie_free):
    """sixteen counts for the rare bytes 1 .. 16.  Fibonacci (1, 1, 2, 3, 5, ..., 987; 2,583 in all): the deepest Huffman tree these
    counts allow is a chain, but every sum ties with the next count, and a builder that takes the shallower subtree on a tie makes
    an optimal code of depth 13 from them.  Tie-free (1, 2, then c[i] = c[i-1] + c[i-2] + 1: 4, 7, 12, ..., 2,583; 6,746 in all): every sum
    lies strictly below the count after the next, the tree is a chain whatever the tie rule, and EVERY optimal code is deep."""
    c = [1, 2] if tie_free else [1, 1]
    while len(c) < 16:
        c.append(c[-1] + c[-2] + (1 if tie_free else 0))
    assert (c[-1], sum(c)) == ((2583, 6746) if tie_free else (987, 2583))
    return c


@functools.lru_cache(maxsize=None)
def limiter_input(tie_free=True):
    """A member of literals alone with very unequal counts: B(32, 3) over the bytes 64 .. 95 and its first two bytes again (32,770
    bytes in which no 3 bytes repeat: no match), with the rare bytes 1 .. 16 inserted rare_counts() times in a seeded shuffle, each
    behind a filler position of its own (2, 7, 12, ... for the Fibonacci counts, 2, 6, 10, ... for the tie-free ones)."""
    base = [64 + s for s in de_bruijn(32, 3)]
    base += base[:2]
    assert len(base) == 32770
    counts = rare_counts(tie_free)
    rare = np.repeat(np.arange(1, 17, dtype=np.uint8), counts)
    np.random.default_rng(15).shuffle(rare)
    step = 4 if tie_free else 5
    behind = {2 + step * i: int(r) for i, r in enumerate(rare)}
    assert max(behind) < len(base)
    out = bytearray()
    for pos, byte in enumerate(base):
        out.append(byte)
        if pos in behind:
            out.append(behind[pos])
    assert len(out) == 32770 + sum(counts)
    return bytes(out)


@functools.lru_cache(maxsize=None)
def dyn_cases():
    """name -> bytes: what level 2 adds to deflate_cases.cases()"""
    return {
        "limiter": limiter_input(True),
        "limiter_fibonacci": limiter_input(False),
        "one_literal": b"a",                 # one literal and the end of the block; no distance: two forced
        "one_distance": dc.distinct(200) * 20,  # every match 200 bytes back: one distance symbol (15), a second one (0) forced
        "no_match_300": dc.distinct(300),    # no match: the distance code is empty before forcing
        "no_match_3000": dc.distinct(3000),
    }


def btype(member):
    return (member[18] >> 1) & 3  # 0 stored, 1 fixed codes, 2 dynamic codes


def fib_counts(nsym, cap=1 << 21):
    """1, 1, 2, 3, 5, ... up to `cap`, the rest equal: a Huffman tree much deeper than any limit"""
    out, a, b = [], 1, 1
    for _ in range(nsym):
        out.append(min(a, cap))
        a, b = b, a + b
    return out


def builder_cases():
    """name -> (counts, maxbits, the limit must be needed: True / False / None for either)"""
    rng = np.random.default_rng(3)
    out = {
        "fib_286_at_15": (fib_counts(286), 15, True),
        "fib_19_at_7": (fib_counts(9) + [0] * 10, 7, True),  # 1, 1, 2, ..., 34: depth 8
        "fib_19_all_at_7": (fib_counts(19), 7, True),
        "fits_286": ([int(v) for v in rng.integers(50, 400, 286)], 15, False),
        "fits_30": ([int(v) for v in rng.integers(0, 60, 30)], 15, False),
        "fits_19": ([3, 0, 5, 9, 1, 7, 7, 2, 0, 11, 6, 4, 8, 0, 0, 1, 30, 12, 20], 7, False),
        "equal_286": ([7] * 286, 15, False),
        "equal_19": ([1] * 19, 7, False),
        "equal_256_exact": ([5] * 256 + [0] * 30, 15, False),
        "two_symbols": ([0] * 100 + [9] + [0] * 150 + [1] + [0] * 34, 15, False),
        "two_of_19": ([0, 4] + [0] * 16 + [4], 7, False),
        "up_to_65280": ([65280, 65280, 1, 2, 3] + [int(v) for v in rng.integers(0, 65281, 281)], 15, None),
        "text_like": ([0] * 9 + [70000, 2200] + [0] * 21 + [int(v) for v in rng.integers(1, 9000, 64)] + [0] * 161 + [1, 900, 40, 3, 1] + [0] * 24, 15, None),
        "geometric_30": ([1 << min(i, 20) for i in range(30)], 15, True),
    }
    for name, (freq, _, _) in out.items():
        assert len(freq) in (19, 30, 286), name
    return out


def huffman_cost_and_depth(freq):
    """(sum of count x length, greatest length) of a Huffman code for the non-zero counts, the least depth among the optimal ones"""
    heap = [(f, 0, (i,)) for i, f in enumerate(freq) if f]
    depth = {i: 0 for _, _, (i,) in heap}
    heapq.heapify(heap)
    while len(heap) > 1:
        fa, ha, sa = heapq.heappop(heap)
        fb, hb, sb = heapq.heappop(heap)
        for s in sa + sb:
            depth[s] += 1
        heapq.heappush(heap, (fa + fb, max(ha, hb) + 1, sa + sb))  # among equal weights the shallower subtree first
    return sum(freq[i] * d for i, d in depth.items()), max(depth.values())


def check_lengths(freq, maxbits, lens, limited, expect_limited):
    """the four requirements on the builder's result, and the optimum where no limit was needed"""
    freq, lens = [int(f) for f in freq], [int(v) for v in lens]
    assert len(lens) == len(freq)
    for f, ln in zip(freq, lens):
        assert (f == 0) == (ln == 0)
        assert ln <= maxbits
    nz = [(f, ln) for f, ln in zip(freq, lens) if f]
    assert len(nz) >= 2
    assert sum(1 << (maxbits - ln) for _, ln in nz) == 1 << maxbits  # Kraft: exactly 1
    for fa, la in nz:
        for fb, lb in nz:
            assert not (fa > fb and la > lb), (fa, la, fb, lb)
    cost, depth = huffman_cost_and_depth(freq)
    mine = sum(f * ln for f, ln in nz)
    if expect_limited is not None:
        assert limited == expect_limited
    if depth <= maxbits:
        assert not limited and mine == cost
    else:
        assert limited and mine >= cost
