"""What the colour classes of key groups are, stated with a dictionary (shared by test_colour_classes_cpu.py and
test_gpu_colour_classes.py), and the invariants that hold for the device's classes whatever its fingerprints do."""
import numpy as np

NO_CLASS = 0xFFFFFFFF


def groups_of(sets):
    """goff, ranks of a list of rank lists"""
    goff = np.cumsum([0] + [len(s) for s in sets]).astype(np.uint64)
    ranks = np.array([r for s in sets for r in s], dtype=np.uint32)
    return goff, ranks


def classes_dict(goff, ranks):
    """(class_of, rep) as lists: one class per distinct rank tuple among the groups of >= 2 ranks, in order of first appearance"""
    seen, class_of, rep = {}, [], []
    g, r = [int(v) for v in goff], ranks.tolist()
    for i in range(len(g) - 1):
        s = tuple(r[g[i]:g[i + 1]])
        if len(s) < 2:
            class_of.append(NO_CLASS)
            continue
        if s not in seen:
            seen[s] = len(rep)
            rep.append(i)
        class_of.append(seen[s])
    return class_of, rep


def check_invariants(goff, ranks, class_of, rep):
    """every group of a class has the ranks of rep[class]; rep[c] is the class's smallest group and rep ascends; singles have none"""
    g = goff.astype(np.int64)
    lens = np.diff(g)
    assert len(class_of) == len(lens)
    assert np.array_equal(class_of == NO_CLASS, lens < 2)
    multi = np.flatnonzero(lens >= 2)
    c = class_of[multi].astype(np.int64)
    assert len(rep) == 0 or (np.all(np.diff(rep.astype(np.int64)) > 0) and c.max() == len(rep) - 1)
    assert len(multi) == 0 or c.min() >= 0
    first = np.full(len(rep), len(lens), np.int64)
    np.minimum.at(first, c, multi)  # the smallest group index of every class
    assert np.array_equal(first, rep.astype(np.int64))
    r = rep.astype(np.int64)[c]
    assert np.array_equal(lens[multi], lens[r])
    # the ranks, element for element: positions of every multi-rank group against those of its class's first group
    n = lens[multi]
    within = np.arange(n.sum()) - np.repeat(np.cumsum(n) - n, n)
    assert np.array_equal(ranks[np.repeat(g[multi], n) + within], ranks[np.repeat(g[r], n) + within])
