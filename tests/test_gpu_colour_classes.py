"""The colour classes of key groups on the device (kr_colour_classes_device: fingerprints from one scan, radix sort, content
compare with the predecessor, class numbers by first appearance) against the host's canonical classes, and -- with fingerprints cut
down so that the content compare has to decide -- against the invariants that both functions hold."""
import ctypes as C

import numpy as np
import pytest

from colour_classes_ref import check_invariants, groups_of

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def tile(capi):
    t = capi.build_keys_stats()["tile"]
    assert t >= 256 and t % 256 == 0
    return t


def both(capi, goff, ranks):
    """device classes (after checking them against the host's, array for array) and the stage's counters.
    Full 64-bit fingerprints: two of a few thousand distinct sets share one with probability ~1e-12 (n^2 / 2^65), and only then may
    the device split a set over two classes."""
    want_of, want_rep = capi.group_colour_classes(goff, ranks)
    got_of, got_rep = capi.group_colour_classes(goff, ranks, device=0)
    st = capi.build_colours_stats()
    assert got_of.dtype == np.uint32 and got_rep.dtype == np.uint64
    assert np.array_equal(got_of, want_of) and np.array_equal(got_rep, want_rep)
    multi = int((np.diff(goff.astype(np.int64)) >= 2).sum())
    assert (st["groups"], st["multi"], st["classes"], st["path"]) == (len(goff) - 1, multi, len(want_rep), 1)
    assert st["passes"] == (8 if multi else 0)
    check_invariants(goff, ranks, got_of, got_rep)
    return got_of, got_rep, st


def random_groups(rng, nmulti, nsingle, pool=40, universe=24):
    """nmulti groups of 2..5 ranks drawn from `pool` distinct sets and nsingle groups of one rank, shuffled"""
    sets = [sorted(rng.choice(universe, size=int(rng.integers(2, 6)), replace=False).tolist()) for _ in range(pool)]
    groups = [sets[q] for q in rng.integers(0, pool, nmulti)] + [[int(r)] for r in rng.integers(0, universe, nsingle)]
    return groups_of([groups[q] for q in rng.permutation(len(groups))])


def test_no_group_of_several_ranks(capi):
    goff, ranks = groups_of([[q % 7] for q in range(3000)])
    got_of, got_rep, _ = both(capi, goff, ranks)
    assert len(got_rep) == 0 and (got_of == capi.KR_NO_CLASS).all()
    got_of, got_rep = capi.group_colour_classes(np.zeros(1, np.uint64), np.zeros(0, np.uint32), device=0)  # no group at all
    assert len(got_of) == 0 and len(got_rep) == 0 and capi.build_colours_stats()["path"] == 1
    got_of, _ = capi.group_colour_classes(np.array([0, 1], np.uint64), np.zeros(1, np.uint32), device=0)  # one rank in all
    assert got_of.tolist() == [capi.KR_NO_CLASS]


def test_exactly_one_group_of_several_ranks(capi):
    sets = [[q % 7] for q in range(3000)]
    sets[1234] = [2, 5, 6]
    got_of, got_rep, _ = both(capi, *groups_of(sets))
    assert got_rep.tolist() == [1234] and got_of[1234] == 0


@pytest.mark.parametrize("shape", ["tile-1", "tile", "tile+1", "3*tile+5"])
def test_list_sizes_around_a_tile(capi, tile, shape):
    m = eval(shape, {"tile": tile})
    goff, ranks = random_groups(np.random.default_rng(m), m, 2 * m + 3)
    _, got_rep, st = both(capi, goff, ranks)
    assert st["multi"] == m and 1 < len(got_rep) <= 40


def test_more_ranks_than_one_round_of_the_block_sum_scan(capi, tile):
    # the terms are scanned in blocks of 1024: more than 1024 blocks of them, at the size at which
    # test_gpu_key_groups.py::test_more_tiles_than_one_round_of_the_block_sum_scan does it for the sort's counts
    n = tile * 4096 + tile + 7
    rng = np.random.default_rng(5)
    pool = rng.integers(1, 1 << 16, 3000).astype(np.uint16)  # 3000 sets over 16 leaves, as bit masks
    masks = pool[rng.integers(0, len(pool), n // 6)]
    bits = np.unpackbits(masks.view(np.uint8).reshape(-1, 2), axis=1, bitorder="little")
    lens = bits.sum(axis=1).astype(np.int64)
    ranks = np.nonzero(bits)[1].astype(np.uint32)
    assert len(ranks) > n
    keep = int(np.searchsorted(np.cumsum(lens), n, side="right"))  # whole groups, then one that takes the rest
    goff = np.concatenate([[0], np.cumsum(lens[:keep]), [n]]).astype(np.uint64)
    goff = np.unique(goff)
    _, got_rep, st = both(capi, goff, ranks[:n])
    assert int(goff[-1]) == n > 1024 * 1024 and st["multi"] > 4 * tile and len(got_rep) <= 3001


def test_groups_across_the_scan_blocks(capi):
    # groups of seven ranks: a multiple of 1024 ranks (a block of the term scan) falls inside a group, but for every seventh
    rng = np.random.default_rng(7)
    sets = [sorted(rng.choice(30, size=7, replace=False).tolist()) for _ in range(12)]
    goff, ranks = groups_of([sets[q] for q in rng.integers(0, 12, 2000)])
    assert sum(b % 7 != 0 for b in range(1024, len(ranks), 1024)) >= 10
    _, got_rep, _ = both(capi, goff, ranks)
    assert len(got_rep) == 12


@pytest.mark.parametrize("n", [2, 63, 64, 65])
def test_lengths_around_the_lane_compare(capi, n, monkeypatch):
    a = list(range(n))
    last = a[:-1] + [n]
    first = [n + 1] + a[1:]  # (as a sequence; the builder's are sorted)
    sets = [a, last, [7], a, first, last, a[:-1] + [n + 2], first]
    got_of, got_rep, _ = both(capi, *groups_of(sets))
    assert got_of.tolist() == [0, 1, capi.KR_NO_CLASS, 0, 2, 1, 3, 2] and got_rep.tolist() == [0, 1, 4, 6]
    for bits in ("0", "3"):  # every group a candidate for its predecessor: the ranks decide
        monkeypatch.setenv("KR_BUILD_COLOUR_HASH_BITS", bits)
        goff, ranks = groups_of(sets + [first, first, a, a])
        of, rep = capi.group_colour_classes(goff, ranks, device=0)
        check_invariants(goff, ranks, of, rep)
        assert of[-1] == of[-2] and of[-3] == of[-4]


def test_long_groups_taken_by_a_wave(capi, monkeypatch):
    a = np.arange(65536, dtype=np.uint32)
    last = a.copy()
    last[-1] = 65536            # differs from a in the last rank only
    d = np.arange(1, 65537, dtype=np.uint32)
    d[0] = 0                    # 0, 2, 3, ...
    e = np.arange(1, 65537, dtype=np.uint32)  # 1, 2, 3, ...: differs from d in the first rank only
    groups = [a, last, a, d, e, last, e, e]
    goff = np.cumsum([0] + [len(g) for g in groups]).astype(np.uint64)
    ranks = np.concatenate(groups)
    got_of, got_rep, _ = both(capi, goff, ranks)
    assert got_of.tolist() == [0, 1, 0, 2, 3, 1, 3, 3] and got_rep.tolist() == [0, 1, 3, 4]
    monkeypatch.setenv("KR_BUILD_COLOUR_HASH_BITS", "0")  # list order = group order: only the last two equal their predecessors
    of, rep = capi.group_colour_classes(goff, ranks, device=0)
    st = capi.build_colours_stats()
    check_invariants(goff, ranks, of, rep)
    assert of.tolist() == [0, 1, 2, 3, 4, 5, 6, 6] and st["classes"] == 7 and st["raised"] == 6 and st["passes"] == 0


def test_equal_sums_and_a_prefix(capi):
    got_of, _, _ = both(capi, *groups_of([[0, 3], [1, 2], [0, 3], [0, 1], [0, 1, 2], [0, 1], [1, 2]]))
    assert got_of.tolist() == [0, 1, 0, 2, 3, 2, 1]


def test_b_a_b_a_across_tiles(capi, tile):
    rng = np.random.default_rng(11)
    a, b = [3, 4, 9], [3, 5, 9]
    filler = [sorted(rng.choice(np.arange(10, 40), size=3, replace=False).tolist()) for _ in range(tile + 10)]
    sets = [b, a] + filler + [b, a]
    got_of, got_rep, _ = both(capi, *groups_of(sets))
    assert got_of[0] == 0 and got_of[1] == 1 and got_of[-2] == 0 and got_of[-1] == 1
    assert got_rep[:2].tolist() == [0, 1] and np.all(np.diff(got_rep.astype(np.int64)) > 0)


@pytest.mark.parametrize("bits", ["0", "3"])
def test_reduced_fingerprints_hold_the_invariants(capi, tile, bits, monkeypatch):
    goff, ranks = random_groups(np.random.default_rng(13), 3 * tile + 5, 2000, pool=8)
    monkeypatch.setenv("KR_BUILD_COLOUR_HASH_BITS", bits)
    of, rep = capi.group_colour_classes(goff, ranks, device=0)
    st = capi.build_colours_stats()
    check_invariants(goff, ranks, of, rep)
    assert st["path"] == 1 and st["passes"] == (1 if bits == "3" else 0)
    assert st["raised"] > 0 and 8 <= st["classes"] == len(rep) < st["multi"] == 3 * tile + 5
    monkeypatch.delenv("KR_BUILD_COLOUR_HASH_BITS")
    _, want_rep, _ = both(capi, goff, ranks)
    assert len(want_rep) == 8 and np.array_equal(rep[:1], want_rep[:1])


def test_same_input_twice_gives_the_same_arrays(capi, tile):
    goff, ranks = random_groups(np.random.default_rng(12), 5 * tile + 3, 777)
    a_of, a_rep, _ = both(capi, goff, ranks)
    b_of, b_rep, _ = both(capi, goff, ranks)
    assert np.array_equal(a_of, b_of) and np.array_equal(a_rep, b_rep)


def test_falls_back_to_the_host_for_memory(capi, tile, monkeypatch):
    goff, ranks = random_groups(np.random.default_rng(14), 40000, 100)
    monkeypatch.setenv("KR_BUILD_KEYS_MAX_MB", "1")
    of, rep = capi.group_colour_classes(goff, ranks, device=0)
    want_of, want_rep = capi.group_colour_classes(goff, ranks)
    st = capi.build_colours_stats()
    assert np.array_equal(of, want_of) and np.array_equal(rep, want_rep)
    assert (st["path"], st["multi"], st["classes"], st["passes"]) == (2, 40000, len(rep), 0)


def test_device_errors(capi):
    lib = capi.load()
    goff, ranks = groups_of([[0, 1]])
    res = capi.KrColourClasses()
    vp = C.c_void_p
    capi.group_colour_classes(goff, ranks, device=0)  # (sets the argument types)
    lib.kr_colour_classes_device.argtypes = [C.c_int, vp, vp, C.c_uint64, vp]
    assert lib.kr_colour_classes_device(0, None, ranks.ctypes.data, 1, C.addressof(res)) == capi.KR_ERR_ARG
    assert lib.kr_colour_classes_device(0, goff.ctypes.data, None, 1, C.addressof(res)) == capi.KR_ERR_ARG
    assert lib.kr_colour_classes_device(0, goff.ctypes.data, ranks.ctypes.data, 1, None) == capi.KR_ERR_ARG
    lib.kr_colour_classes_device.argtypes = [C.c_int, vp, vp, C.c_uint64, C.POINTER(capi.KrColourClasses)]
    with pytest.raises(capi.KrError) as e:
        capi.group_colour_classes(np.array([0, 2, 1], np.uint64), ranks, device=0)
    assert e.value.code == capi.KR_ERR_ARG
    with pytest.raises(capi.KrError) as e:
        capi.group_colour_classes(goff, ranks, device=4096)
    assert e.value.code == capi.KR_ERR_ARG
