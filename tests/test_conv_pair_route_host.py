"""conv_pair_route (csrc/gemm_x3h.hip) through mt2_conv_pair_route, no GPU: which resblock conv pairs of the vocoder the fused pair
kernel takes, with which launch geometry and LDS bytes, and the status every other pair is sent back to the two-launch form with."""
import pytest

from megatts2_amd import runtime as rt

OK, INVALID, NOT_SUPPORTED = 0, 1, 801          # hipSuccess, hipErrorInvalidValue, hipErrorNotSupported

# per channel count: rows per pass, ring bytes (stages x bytes per stage of the window tiles 98 / 99 / 100), bit of pair_fuse
TILES = {32: (256, 4 * 4096, 1), 64: (256, 4 * 8192, 2), 128: (128, 3 * 16384, 4)}
REFLECT, NO_PLANES, TWO_GIB, MISALIGNED = 1, 2, 4, 8


def ceil8(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("dil", [1, 3, 5])
def test_accepted_pairs_report_geometry_and_lds(C, k, dil):
    bm, ring, _ = TILES[C]
    for R in (1, bm - k, bm - k + 1, bm - k + 2, 700, 3_562_496):
        r = rt.op_conv_pair_route(R, C, k, dil)
        bmo = bm - (k - 1)
        assert r["err"] == OK
        assert (r["bm"], r["bmo"], r["block"]) == (bm, bmo, 768)
        assert r["grid"] == -(-R // bmo)
        assert r["lds"] == ring + (C // 32) * ceil8(bm + (k - 1) * dil) * 128


def test_lds_stays_at_the_window_tiles_size():
    assert rt.op_conv_pair_route(1000, 64, 11, 5)["lds"] == 79872 + 32768
    assert rt.op_conv_pair_route(1000, 128, 11, 5)["lds"] == 94208 + 49152
    assert rt.op_conv_pair_route(1000, 32, 11, 5)["lds"] == 39936 + 16384


def test_widest_span_is_64_rows():
    assert rt.op_conv_pair_route(1000, 64, 9, 8)["err"] == OK                 # (k - 1) dil = 64
    assert rt.op_conv_pair_route(1000, 64, 11, 7)["err"] == NOT_SUPPORTED      # 70
    assert rt.op_conv_pair_route(1000, 64, 7, 11)["err"] == NOT_SUPPORTED      # 66


@pytest.mark.parametrize("C", [4, 8, 16, 48, 96, 256, 512])
def test_other_channel_counts_keep_two_launches(C):
    r = rt.op_conv_pair_route(1000, C, 3, 1)
    assert r["err"] == NOT_SUPPORTED and r["grid"] == 0 and r["lds"] == 0


@pytest.mark.parametrize("C", [32, 64, 128])
def test_every_documented_rejection(C):
    bit = TILES[C][2]
    for flags in (REFLECT, NO_PLANES, TWO_GIB, MISALIGNED):
        r = rt.op_conv_pair_route(1000, C, 7, 3, flags=flags)
        assert r["err"] == NOT_SUPPORTED and r["grid"] == 0 and r["lds"] == 0, flags
    # the option's mask: only the channel count's own bit matters
    assert rt.op_conv_pair_route(1000, C, 7, 3, pair_fuse=7 & ~bit)["err"] == NOT_SUPPORTED
    assert rt.op_conv_pair_route(1000, C, 7, 3, pair_fuse=bit)["err"] == OK
    assert rt.op_conv_pair_route(1000, C, 7, 3, pair_fuse=0)["err"] == NOT_SUPPORTED
    # without the x3h window convolutions the two launches run another kernel: the pair follows them
    assert rt.op_conv_pair_route(1000, C, 7, 3, x3h=15 & ~4)["err"] == NOT_SUPPORTED
    assert rt.op_conv_pair_route(1000, C, 7, 3, x3h=4)["err"] == OK
    # bad arguments
    assert rt.op_conv_pair_route(1000, C, 1, 1)["err"] == INVALID
    assert rt.op_conv_pair_route(1000, C, 3, 0)["err"] == INVALID
    # nothing to launch
    r = rt.op_conv_pair_route(0, C, 3, 1)
    assert r["err"] == OK and r["grid"] == 0
