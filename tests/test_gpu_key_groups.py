"""The key stage of the build on the device (kr_key_groups_device: radix sort of (key, rank) pairs, grouping, row counts) against
its host twin kr_key_groups_cpu, array for array, and the pass counter against the digits that can differ."""
import numpy as np
import pytest

from key_groups_ref import digit_passes, make_keys, random_pairs

pytestmark = pytest.mark.gpu

NAMES = ("keys", "goff", "ranks", "inc")


def both(capi, keys, ranks, nrows, nleaves):
    """device result (after checking it against the host's) and the stage's counters"""
    want = capi.key_groups(keys, ranks, nrows, nleaves)
    got = capi.key_groups(keys, ranks, nrows, nleaves, device=0)
    st = capi.build_keys_stats()
    for name in NAMES:
        assert got[name].dtype == want[name].dtype and got[name].shape == want[name].shape, name
        assert np.array_equal(got[name], want[name]), name
    assert st["path"] == 1
    assert (st["pairs_in"], st["pairs_out"], st["keys_out"]) == (len(keys), len(got["ranks"]), len(got["keys"]))
    assert st["passes"] == (digit_passes(nrows, nleaves) if len(keys) else 0)
    return got, st


@pytest.fixture(scope="module")
def tile(capi):
    t = capi.build_keys_stats()["tile"]
    assert t >= 256 and t % 256 == 0
    return t


@pytest.mark.parametrize("shape", ["0", "1", "tile-1", "tile", "tile+1", "3*tile+5"])
def test_sizes_around_a_tile(capi, tile, shape):
    n = eval(shape, {"tile": tile})
    keys, ranks = random_pairs(n, 8192, 300, seed=n)
    got, _ = both(capi, keys, ranks, 8192, 300)
    if n == 0:
        assert got["goff"].tolist() == [0] and not got["inc"].any()


def test_more_tiles_than_one_round_of_the_block_sum_scan(capi, tile):
    # 256 counts per tile in blocks of 1024: more than 1024 blocks of counts is more than 4096 tiles
    n = tile * 4096 + tile + 7
    rng = np.random.default_rng(5)
    keys = make_keys(rng.integers(0, 4096, n), rng.integers(0, 1 << 20, n))  # (2^32 possible keys: repeats across leaves)
    ranks = rng.integers(0, 16, n).astype(np.uint32)
    got, _ = both(capi, keys, ranks, 4096, 16)
    assert len(got["keys"]) < len(got["ranks"]) < n


def test_one_key_ranks_descending(capi, tile):
    # every pair in one bucket of every key digit: only a stable scatter keeps the order the rank passes made
    n = 3 * tile + 5
    assert n <= 65536
    keys = np.full(n, (77 << 32) | 0xDEADBEEF, dtype=np.uint64)
    ranks = np.arange(n - 1, -1, -1, dtype=np.uint32)
    got, _ = both(capi, keys, ranks, 8192, 65536)
    assert got["ranks"].tolist() == list(range(n)) and got["goff"].tolist() == [0, n]


def test_keys_that_differ_in_one_bit(capi, tile):
    rng = np.random.default_rng(6)
    n = 2 * tile + 100
    ranks = rng.integers(0, 40, n).astype(np.uint32)
    low = make_keys(np.full(n, 5), 0x80000000 | rng.integers(0, 2, n))  # lowest enc bit
    got, _ = both(capi, low, ranks, 1 << 14, 40)
    assert len(got["keys"]) == 2
    high = make_keys(rng.integers(0, 2, n) << 13, np.full(n, 9))  # highest row bit in use with 2^14 rows
    got, _ = both(capi, high, ranks, 1 << 14, 40)
    assert got["keys"].tolist() == [9, (1 << 45) | 9]


@pytest.mark.parametrize("nrows,passes", [(1 << 14, 6 + 2), (10923, 6 + 2), (1, 4 + 2), (257, 6 + 2), (256, 5 + 2)])
def test_row_counts_and_pass_counter(capi, tile, nrows, passes):
    # 10923: what h = 7, m = 3, r = 1 with --frac gives (two of three residues of 16384 hash values)
    keys, ranks = random_pairs(tile + 300, nrows, 1000, seed=nrows)
    keys[:4] = make_keys([nrows - 1, nrows - 1, 0, 0], [1, 2, 1, 2])
    _, st = both(capi, keys, ranks, nrows, 1000)
    assert st["passes"] == passes


def test_two_to_the_thirty_rows_keys_in_the_top_rows(capi, tile):
    nrows, nleaves = 1 << 30, 3
    rng = np.random.default_rng(8)
    n = tile + 50
    keys = make_keys(nrows - 1 - rng.integers(0, 40, n), rng.integers(0, 4, n))
    ranks = rng.integers(0, nleaves, n).astype(np.uint32)
    want = capi.key_groups(keys, ranks, nrows, nleaves, copy=False)
    got = capi.key_groups(keys, ranks, nrows, nleaves, device=0, copy=False)
    try:
        assert capi.build_keys_stats()["passes"] == 8 + 1 == digit_passes(nrows, nleaves)
        for name in ("keys", "goff", "ranks"):
            assert np.array_equal(got[name], want[name]), name
        assert len(got["inc"]) == nrows
        step = 1 << 26
        for a in range(0, nrows, step):
            assert np.array_equal(got["inc"][a:a + step], want["inc"][a:a + step]), a
        assert want["inc"][nrows - 41] == 0 and want["inc"][-1] == len(want["keys"])
    finally:
        got["free"](), want["free"]()


@pytest.mark.parametrize("nleaves,rank_passes", [(1, 0), (2, 1), (256, 1), (257, 2), (65536, 2)])
def test_rank_digit_boundaries(capi, tile, nleaves, rank_passes):
    keys, ranks = random_pairs(2 * tile + 9, 64, nleaves, seed=nleaves, distinct_keys=50)
    ranks[:2] = [nleaves - 1, 0]
    _, st = both(capi, keys, ranks, 64, nleaves)
    assert st["passes"] == rank_passes + 5


def test_duplicate_pairs_and_a_group_across_a_tile_boundary(capi, tile):
    rng = np.random.default_rng(9)
    # in sorted order: tile - 700 pairs of small keys, then ONE key with 1500 pairs (8 ranks: long runs of one pair) across
    # position `tile` (and across the 1024-pair blocks of the grouping), then larger keys
    small = make_keys(rng.integers(0, 10, tile - 700), rng.integers(0, 1 << 32, tile - 700))
    big = np.full(1500, make_keys([10], [12345])[0], dtype=np.uint64)
    large = make_keys(rng.integers(11, 64, tile), rng.integers(0, 1 << 8, tile))
    keys = np.concatenate([small, big, large, small[:300]])  # (and 300 pairs twice over)
    ranks = np.concatenate([rng.integers(0, 500, len(small)), rng.integers(0, 8, 1500), rng.integers(0, 500, tile)]).astype(np.uint32)
    ranks = np.concatenate([ranks, ranks[:300]])
    order = rng.permutation(len(keys))
    got, st = both(capi, keys[order], ranks[order], 64, 500)
    i = got["keys"].tolist().index(int(big[0]))
    assert got["ranks"][int(got["goff"][i]):int(got["goff"][i + 1])].tolist() == list(range(8))
    assert st["pairs_out"] <= st["pairs_in"] - 300 - (1500 - 8)


@pytest.mark.parametrize("descending", [False, True])
def test_input_already_in_order(capi, tile, descending):
    keys, ranks = random_pairs(3 * tile + 77, 8192, 300, seed=11)
    order = np.lexsort((ranks, keys))
    if descending:
        order = order[::-1]
    both(capi, keys[order], ranks[order], 8192, 300)


def test_same_input_twice_gives_the_same_arrays(capi, tile):
    keys, ranks = random_pairs(5 * tile + 3, 8192, 300, seed=12)
    a, _ = both(capi, keys, ranks, 8192, 300)
    b, _ = both(capi, keys, ranks, 8192, 300)
    for name in NAMES:
        assert np.array_equal(a[name], b[name]), name


def test_device_errors(capi):
    one = np.zeros(1, np.uint32)
    with pytest.raises(capi.KrError, match="row out of range") as e:
        capi.key_groups(make_keys([4], [1]), one, 4, 1, device=0)
    assert e.value.code == capi.KR_ERR_FORMAT
    with pytest.raises(capi.KrError) as e:
        capi.key_groups(make_keys([0], [1]), np.array([2], np.uint32), 4, 2, device=0)
    assert e.value.code == capi.KR_ERR_ARG
    with pytest.raises(capi.KrError) as e:
        capi.key_groups(make_keys([0], [1]), one, 4, 65537, device=0)
    assert e.value.code == capi.KR_ERR_ARG
