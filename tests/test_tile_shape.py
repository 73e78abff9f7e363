"""tile_shape (krepp_amd/csrc/kr_dev_tiles.inc): the per-sequence arithmetic the host's build_tiles and the device's layout kernels
share -- k-mer positions, tiles of 128 positions, bases in the tiled batch -- at the lengths where it changes.  No GPU needed."""
import pytest


@pytest.mark.parametrize("length,k,want", [
    (0, 21, (0, 0, 0)), (20, 21, (0, 0, 20)), (21, 21, (1, 1, 21)),          # empty, shorter than k, one position
    (148, 21, (128, 1, 148)), (149, 21, (129, 2, 169)), (150, 21, (130, 2, 170)),  # one full tile; a second tile of one position
    (1043, 21, (1023, 8, 1183)), (1044, 21, (1024, 8, 1184)),                # the threshold: 1,024 positions are eight full tiles
    (1045, 21, (1025, 9, 1205)), (1172, 21, (1152, 9, 1332)), (1173, 21, (1153, 10, 1353)),
    (400000, 27, (399974, 3125, 400000 + 3124 * 26)), (400001, 31, (399971, 3125, 400001 + 3124 * 30)),
    (154, 27, (128, 1, 154)), (155, 27, (129, 2, 181)),
    ((1 << 32) + 5, 21, ((1 << 32) - 15, 1 << 25, (1 << 32) + 5 + ((1 << 25) - 1) * 20)),  # lengths are 64-bit
])
def test_tile_shape_at_the_boundary_lengths(capi, length, k, want):
    assert capi.tile_shape(length, k) == want


def test_tile_shape_covers_every_position_once(capi):
    """tiles of 128 positions that overlap by k - 1 bases: the tiles' bases add up, and their positions are the sequence's"""
    for k in (21, 27, 31):
        for length in list(range(0, 600)) + [1044, 1045, 4999, 5000, 12345]:
            nkm, nt, nbytes = capi.tile_shape(length, k)
            assert nkm == max(0, length - k + 1) and nt == -(-nkm // 128)
            pieces = [min(length, t * 128 + 128 + k - 1) - t * 128 for t in range(nt)]
            assert nbytes == (sum(pieces) if nt else length)
            assert sum(p - k + 1 for p in pieces) == nkm


def test_tile_shape_rejects_null_and_k_zero(capi):
    with pytest.raises(capi.KrError) as e:
        capi.tile_shape(100, 0)
    assert e.value.code == capi.KR_ERR_ARG
