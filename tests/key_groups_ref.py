"""What the key stage of the build returns, stated in numpy (shared by test_key_groups_cpu.py and test_gpu_key_groups.py)."""
import numpy as np


def make_keys(rows, encs):
    return (np.asarray(rows, dtype=np.uint64) << np.uint64(32)) | np.asarray(encs, dtype=np.uint64)


def random_pairs(n, nrows, nleaves, seed, distinct_keys=None):
    """n pairs drawn from few enough distinct keys that keys repeat across leaves and whole pairs repeat."""
    rng = np.random.default_rng(seed)
    nd = max(1, n // 3) if distinct_keys is None else distinct_keys
    pool = make_keys(rng.integers(0, nrows, nd), rng.integers(0, 1 << 32, nd))
    keys = pool[rng.integers(0, nd, n)]
    ranks = rng.integers(0, min(nleaves, 4) if n < 100 else nleaves, n).astype(np.uint32)
    if n > 8:  # a run of one pair, whatever the draw gave
        keys[n // 2:n // 2 + 4] = keys[0]
        ranks[n // 2:n // 2 + 4] = ranks[0]
    return keys, ranks


def groups_numpy(keys, ranks, nrows):
    keys = np.asarray(keys, dtype=np.uint64)
    ranks = np.asarray(ranks, dtype=np.uint32)
    order = np.lexsort((ranks, keys))
    k, r = keys[order], ranks[order]
    if len(k):
        keep = np.ones(len(k), bool)
        keep[1:] = (k[1:] != k[:-1]) | (r[1:] != r[:-1])
        k, r = k[keep], r[keep]
    ukeys, first = np.unique(k, return_index=True)
    goff = np.concatenate([first, [len(k)]]).astype(np.uint64)
    inc = np.cumsum(np.bincount((ukeys >> np.uint64(32)).astype(np.int64), minlength=nrows)).astype(np.uint64)
    return {"keys": ukeys.astype(np.uint64), "goff": goff, "ranks": r.astype(np.uint32), "inc": inc}


def digit_passes(nrows, nleaves):
    """8-bit digits that can differ: ceil(log2(nleaves)) bits of rank, 32 bits of enc + ceil(log2(nrows)) bits of row."""
    bits = lambda v: (v - 1).bit_length()
    return -(-bits(nleaves) // 8) + -(-(32 + bits(nrows)) // 8)
