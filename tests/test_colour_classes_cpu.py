"""The colour classes of key groups on the host (kr_colour_classes_cpu): one class per distinct rank set among the groups of two or
more ranks, numbered in order of first appearance -- against a dictionary statement of the same result."""
import ctypes as C

import numpy as np
import pytest

from colour_classes_ref import classes_dict, groups_of


@pytest.mark.parametrize("sets", [
    [[0, 1], [2], [0, 1], [1, 2], [0, 1, 2], [1, 2], [5]],
    [[0, 3], [1, 2]],                       # equal sums of ranks
    [[0, 1], [0, 1, 2], [0, 1]],            # a prefix of another
    [[7, 9]] * 5,
    [[1, 2], [0, 1], [1, 2], [0, 1]],       # B, A, B, A
])
def test_cpu_classes_equal_the_dictionary_statement(capi, sets):
    goff, ranks = groups_of(sets)
    class_of, rep = capi.group_colour_classes(goff, ranks)
    want_of, want_rep = classes_dict(goff, ranks)
    assert class_of.dtype == np.uint32 and rep.dtype == np.uint64
    assert class_of.tolist() == want_of and rep.tolist() == want_rep


def test_cpu_classes_first_appearance_numbering_and_singles(capi):
    goff, ranks = groups_of([[3], [4, 5], [1, 2], [4, 5], [9], [1, 2], [0, 9]])
    class_of, rep = capi.group_colour_classes(goff, ranks)
    assert class_of.tolist() == [capi.KR_NO_CLASS, 0, 1, 0, capi.KR_NO_CLASS, 1, 2]
    assert rep.tolist() == [1, 2, 6]


def test_cpu_classes_random_groups(capi):
    rng = np.random.default_rng(3)
    sets = [sorted(rng.choice(12, size=int(rng.integers(1, 5)), replace=False).tolist()) for _ in range(5000)]
    goff, ranks = groups_of(sets)
    class_of, rep = capi.group_colour_classes(goff, ranks)
    want_of, want_rep = classes_dict(goff, ranks)
    assert class_of.tolist() == want_of and rep.tolist() == want_rep
    assert 0 < len(rep) < sum(len(s) > 1 for s in sets), "the input was meant to repeat its sets"


def test_cpu_classes_of_nothing_and_of_singles_only(capi):
    class_of, rep = capi.group_colour_classes(np.zeros(1, np.uint64), np.zeros(0, np.uint32))
    assert len(class_of) == 0 and len(rep) == 0
    goff, ranks = groups_of([[4], [4], [0], [7]])
    class_of, rep = capi.group_colour_classes(goff, ranks)
    assert class_of.tolist() == [capi.KR_NO_CLASS] * 4 and len(rep) == 0


def test_cpu_classes_errors_bits_and_counters(capi):
    lib = capi.load()
    goff, ranks = groups_of([[0, 1]])
    res = capi.KrColourClasses()
    vp = C.c_void_p
    lib.kr_colour_classes_cpu.argtypes = [vp, vp, C.c_uint64, vp]
    assert lib.kr_colour_classes_cpu(None, ranks.ctypes.data, 1, C.addressof(res)) == capi.KR_ERR_ARG
    assert lib.kr_colour_classes_cpu(goff.ctypes.data, None, 1, C.addressof(res)) == capi.KR_ERR_ARG
    assert lib.kr_colour_classes_cpu(goff.ctypes.data, ranks.ctypes.data, 1, None) == capi.KR_ERR_ARG
    lib.kr_colour_classes_cpu.argtypes = [vp, vp, C.c_uint64, C.POINTER(capi.KrColourClasses)]
    with pytest.raises(capi.KrError) as e:  # offsets that go down
        capi.group_colour_classes(np.array([0, 2, 1], np.uint64), ranks)
    assert e.value.code == capi.KR_ERR_ARG
    lib.kr_colour_classes_free.argtypes = [vp]
    lib.kr_colour_classes_free(None)  # (a no-op)
    assert capi.KR_BUILD_GPU_COLOURS == 4 and capi.KR_NO_CLASS == 0xFFFFFFFF
    assert capi._gpu_build_bits(False, False, True) == 7 and capi._gpu_build_bits(True, True) == 3
    assert set(capi.build_colours_stats()) == {"groups", "multi", "classes", "raised", "path", "passes"}
