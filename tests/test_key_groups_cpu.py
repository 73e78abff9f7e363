"""The key stage of the build on the host (kr_key_groups_cpu): pairs sorted by (key, rank), duplicates dropped, groups of equal
key, cumulative row counts -- against a numpy statement of the same result."""
import ctypes as C

import numpy as np
import pytest

from key_groups_ref import groups_numpy, random_pairs


def same(got, want):
    for name in ("keys", "goff", "ranks", "inc"):
        assert got[name].dtype == want[name].dtype, name
        assert np.array_equal(got[name], want[name]), name


@pytest.mark.parametrize("n,nrows,nleaves,seed", [(1, 1, 1, 0), (1000, 16, 5, 1), (50000, 8192, 300, 2), (20000, 3, 65536, 3), (4097, 1 << 14, 2, 4)])
def test_cpu_groups_equal_the_numpy_statement(capi, n, nrows, nleaves, seed):
    keys, ranks = random_pairs(n, nrows, nleaves, seed)
    want = groups_numpy(keys, ranks, nrows)
    got = capi.key_groups(keys, ranks, nrows, nleaves)
    same(got, want)
    assert got["goff"][-1] == len(got["ranks"]) and got["inc"][-1] == len(got["keys"])
    if n >= 1000:
        assert len(got["ranks"]) < n, "the input was meant to hold duplicate pairs"
        assert len(got["keys"]) < len(got["ranks"]), "the input was meant to hold keys of several leaves"


def test_cpu_groups_of_nothing(capi):
    got = capi.key_groups(np.zeros(0, np.uint64), np.zeros(0, np.uint32), 7, 3)
    assert len(got["keys"]) == 0 and len(got["ranks"]) == 0
    assert got["goff"].tolist() == [0]
    assert got["inc"].tolist() == [0] * 7


def test_cpu_groups_errors(capi):
    lib = capi.load()
    key = lambda row, enc: np.array([(row << 32) | enc], dtype=np.uint64)
    one = np.zeros(1, np.uint32)
    with pytest.raises(capi.KrError, match="row out of range") as e:
        capi.key_groups(key(4, 1), one, 4, 1)
    assert e.value.code == capi.KR_ERR_FORMAT
    capi.key_groups(key(3, 1), one, 4, 1)
    with pytest.raises(capi.KrError) as e:
        capi.key_groups(key(0, 1), np.array([2], np.uint32), 4, 2)
    assert e.value.code == capi.KR_ERR_ARG
    capi.key_groups(key(0, 1), np.array([65535], np.uint32), 4, 65536)
    with pytest.raises(capi.KrError) as e:
        capi.key_groups(key(0, 1), one, 4, 65537)
    assert e.value.code == capi.KR_ERR_ARG
    # null arguments
    res = capi.KrKeyGroups()
    vp = C.c_void_p
    lib.kr_key_groups_cpu.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, vp]
    k = key(0, 1)
    assert lib.kr_key_groups_cpu(None, one.ctypes.data, 1, 4, 1, C.addressof(res)) == capi.KR_ERR_ARG
    assert lib.kr_key_groups_cpu(k.ctypes.data, None, 1, 4, 1, C.addressof(res)) == capi.KR_ERR_ARG
    assert lib.kr_key_groups_cpu(k.ctypes.data, one.ctypes.data, 1, 4, 1, None) == capi.KR_ERR_ARG
    lib.kr_key_groups_cpu.argtypes = [vp, vp, C.c_uint64, C.c_uint32, C.c_uint32, C.POINTER(capi.KrKeyGroups)]
    lib.kr_key_groups_free(None)  # (a no-op)


def test_build_params_bits_and_debug_counters(capi):
    assert (capi.KR_BUILD_GPU_MINIMIZERS, capi.KR_BUILD_GPU_KEYS) == (1, 2)
    assert capi._gpu_build_bits(False, False) == 0 and capi._gpu_build_bits(True, False) == 1 and capi._gpu_build_bits(False, True) == 3
    assert set(capi.build_keys_stats()) == {"pairs_in", "pairs_out", "keys_out", "passes", "pool_growths", "path", "tile"}
