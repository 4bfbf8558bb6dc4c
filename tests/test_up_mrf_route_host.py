"""up_mrf_route (csrc/gemm_x3h.hip) through mt2_up_mrf_route, no GPU: which MRF-mean -> upsampler boundaries of the vocoder the fused kernel
takes, with which launch geometry and LDS bytes, and the status every other one is sent back to the three launches with."""
import pytest

from megatts2_amd import runtime as rt

OK, INVALID, NOT_SUPPORTED = 0, 1, 801          # hipSuccess, hipErrorInvalidValue, hipErrorNotSupported

# per input channel count: rows per workgroup, ring bytes (stages x bytes per stage of the window tiles 99 / 100), bit of up_fuse
TILES = {64: (256, 4 * 8192, 1), 128: (128, 3 * 16384, 2)}
NO_PLANES, TWO_GIB, Y_OFF16, PLANES_OFF128, LDX_ODD, NULL_INPUT, LDY_SHORT, BIAS_OFF16 = 1, 2, 4, 8, 16, 32, 64, 128
NO_WIN_CONV, NO_X6_CONV, FORCED_CFG, LDR64 = 1, 2, 4, 8
LDS_CU = 160 * 1024


def ceil8(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("ch", [64, 128])
def test_accepted_boundaries_report_geometry_and_lds(ch):
    bm, ring, _ = TILES[ch]
    for R in (1, bm - 1, bm, bm + 1, 11 * bm - 5, 1_781_248):
        r = rt.op_up_mrf_route(R, ch)
        assert r["err"] == OK
        assert (r["bm"], r["block"]) == (bm, 768)
        assert r["grid"] == -(-R // bm)
        assert r["lds"] == ring + (ch // 32) * ceil8(bm + 2) * 128 <= LDS_CU


def test_lds_bytes_per_tile():
    assert rt.op_up_mrf_route(1000, 64)["lds"] == 32768 + 2 * 264 * 128
    assert rt.op_up_mrf_route(1000, 128)["lds"] == 49152 + 4 * 136 * 128


@pytest.mark.parametrize("ch", [64, 128])
def test_no_rows_launch_nothing(ch):
    for R in (0, -3):
        r = rt.op_up_mrf_route(R, ch)
        assert r["err"] == OK and r["grid"] == 0 and r["lds"] == 0


@pytest.mark.parametrize("ch", [4, 16, 32, 48, 96, 256, 512])
def test_other_channel_counts_keep_three_launches(ch):
    r = rt.op_up_mrf_route(1000, ch)
    assert r["err"] == NOT_SUPPORTED and r["grid"] == 0 and r["lds"] == 0


@pytest.mark.parametrize("ch", [64, 128])
def test_every_documented_rejection(ch):
    bit = TILES[ch][2]
    rejected = lambda **kw: rt.op_up_mrf_route(1000, ch, **kw)
    for stride in (1, 4, 8):
        assert rejected(stride=stride)["err"] == NOT_SUPPORTED
    # the option's mask: only the channel count's own bit matters
    assert rejected(up_fuse=3 & ~bit)["err"] == NOT_SUPPORTED
    assert rejected(up_fuse=0)["err"] == NOT_SUPPORTED
    assert rejected(up_fuse=bit)["err"] == OK
    # missing planes, 2 GiB, alignment
    for flags in (NO_PLANES, TWO_GIB, Y_OFF16, PLANES_OFF128, LDX_ODD, BIAS_OFF16):
        r = rejected(flags=flags)
        assert r["err"] == NOT_SUPPORTED and r["grid"] == 0 and r["lds"] == 0 and r["bm"] == 0, flags
    # engine options under which the window kernels do not run in the x3h form
    assert rejected(x3h=15 & ~4)["err"] == NOT_SUPPORTED
    assert rejected(x3h=4)["err"] == OK
    for off in (NO_WIN_CONV, NO_X6_CONV, FORCED_CFG, LDR64):
        assert rejected(off=off)["err"] == NOT_SUPPORTED, off
    # bad arguments
    for flags in (NULL_INPUT, LDY_SHORT):
        r = rejected(flags=flags)
        assert r["err"] == INVALID and r["grid"] == 0, flags


@pytest.mark.parametrize("ch", [64, 128])
def test_operands_just_below_two_gib_are_taken(ch):
    rows = (1 << 31) // (4 * ch)                    # R * ldx * 4 = 2 GiB exactly: rejected; one row less: taken
    assert rt.op_up_mrf_route(rows, ch)["err"] == NOT_SUPPORTED
    assert rt.op_up_mrf_route(rows - 1, ch)["err"] == OK
