"""conv_pair_route (csrc/gemm_x3h.hip) through mt2_conv_pair_route, no GPU: which resblock conv pairs of the vocoder the fused pair
kernel takes, with which launch geometry and LDS bytes, and the status every other pair is sent back to the two-launch form with."""
import pytest

from megatts2_amd import runtime as rt

OK, INVALID, NOT_SUPPORTED = 0, 1, 801          # hipSuccess, hipErrorInvalidValue, hipErrorNotSupported

# per channel count: rows per pass, ring bytes (stages x bytes per stage of the window tiles 98 / 99 / 100), bit of pair_fuse
TILES = {32: (256, 4 * 4096, 1), 64: (256, 4 * 8192, 2), 128: (128, 3 * 16384, 4)}
REFLECT, NO_PLANES, TWO_GIB, MISALIGNED = 1, 2, 4, 8


# beyond the model's geometries: the widest window (span 64), spans off the window's 8-row rounding with even tap counts, two taps
EDGE_GEOMS = [(9, 8), (65, 1), (2, 64), (3, 32), (17, 4), (2, 1), (4, 21), (8, 9), (6, 11), (2, 5)]
MODEL_GEOMS = [(k, d) for k in (3, 7, 11) for d in (1, 3, 5)]
WIN_X3H = {32: 98, 64: 99, 128: 100}            # the x3h window tiles of the two-launch form
WIN_ALL = {32: (30, 34, 98), 64: (31, 58, 99), 128: (32, 59, 100)}
W3, WH = 1, 2                                   # op_gemm_route's operand bits: bf16 planes, fp16 planes
LRELU = 2
LDS_CU = 160 * 1024


def ceil8(n):
    return (n + 7) // 8 * 8


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("k", [3, 7, 11])
@pytest.mark.parametrize("dil", [1, 3, 5])
def test_accepted_pairs_report_geometry_and_lds(C, k, dil):
    accepted_pair_geometry(C, k, dil)


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("k,dil", EDGE_GEOMS)
def test_accepted_pairs_beyond_the_models_report_geometry_and_lds(C, k, dil):
    accepted_pair_geometry(C, k, dil)


def accepted_pair_geometry(C, k, dil):
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


@pytest.mark.parametrize("C,lds", [(32, 57344), (64, 114688), (128, 147456)])
def test_lds_at_the_widest_window(C, lds):
    """span 64, however it is made of taps and dilation: ring + (C / 32) slices of (bm + 64) rows of 128 bytes, within a CU's LDS"""
    bm, ring, _ = TILES[C]
    assert lds == ring + (C // 32) * (bm + 64) * 128 <= LDS_CU
    for k, dil in [(9, 8), (65, 1), (2, 64), (3, 32), (17, 4), (5, 16), (33, 2)]:
        assert (k - 1) * dil == 64
        assert rt.op_conv_pair_route(1000, C, k, dil)["lds"] == lds
        # the two launches it replaces ask for the same bytes: one window region, one ring
        assert rt.op_gemm_route(1000, C, k * C, taps=k, dil=dil, pro_act=LRELU, operands=W3 | WH, force_cfg=WIN_X3H[C]) == \
            (OK, WIN_X3H[C], LRELU, lds, 0)
    # spans off the 8-row rounding round up: 63 -> the same bytes, 55 and 1 -> whole 8-row pieces
    for (k, dil), rows in [((4, 21), bm + 64), ((8, 9), bm + 64), ((6, 11), bm + 56), ((2, 1), bm + 8)]:
        assert rt.op_conv_pair_route(1000, C, k, dil)["lds"] == ring + (C // 32) * rows * 128


@pytest.mark.parametrize("C", [32, 64, 128])
def test_window_tiles_are_chosen_and_forced_for_every_eligible_geometry(C):
    """win_eligible (csrc/gemm_dispatch.hip): un-forced launches with both kinds of planes take the x3h window tile, with bf16 planes
    only the x6 one, with neither the f32 one; each can be forced, with at most a CU's LDS."""
    f32, x6, x3h = WIN_ALL[C]
    for k, dil in MODEL_GEOMS + EDGE_GEOMS:
        span = (k - 1) * dil
        for M in (1, 700, 2700):
            for operands, want in ((W3 | WH, x3h), (W3, x6), (0, f32)):
                err, cfg, variant, lds, _ = rt.op_gemm_route(M, C, k * C, taps=k, dil=dil, pro_act=LRELU, operands=operands)
                assert (err, cfg, variant) == (OK, want, LRELU), (k, dil, M, operands)
                assert 0 < lds <= LDS_CU
            for cfg in WIN_ALL[C]:
                err, got, _, lds, _ = rt.op_gemm_route(M, C, k * C, taps=k, dil=dil, operands=W3 | WH, force_cfg=cfg)
                assert (err, got) == (OK, cfg) and 0 < lds <= LDS_CU
        # the x6 / x3h options off: the f32 window tile still serves the geometry
        assert rt.op_gemm_route(700, C, k * C, taps=k, dil=dil, operands=W3 | WH, x3h=0)[:2] == (OK, x6), (k, dil, span)
    # another channel count on a window tile, a window tile of another channel count
    for other in WIN_ALL[{32: 64, 64: 128, 128: 32}[C]]:
        assert rt.op_gemm_route(700, C, 3 * C, taps=3, operands=W3 | WH, force_cfg=other)[0] == INVALID


def test_the_pair_follows_the_forced_window_tiles():
    """Table: conv_pair_route takes a (C, taps, dil) exactly when the x3h window tile of C can be forced for both of its convolutions
    (dilation dil and dilation 1) - spans up to 64 either way, 65 and above neither - and an un-forced launch goes there too."""
    for C in (32, 64, 128):
        for k in list(range(2, 20)) + [32, 33, 64, 65, 66, 67, 130]:
            for dil in list(range(1, 12)) + [16, 21, 22, 31, 32, 33, 63, 64, 65]:
                span = (k - 1) * dil
                pair = rt.op_conv_pair_route(2700, C, k, dil)["err"]
                forced = [rt.op_gemm_route(2700, C, k * C, taps=k, dil=d, operands=W3 | WH, force_cfg=WIN_X3H[C])[0] for d in (dil, 1)]
                chosen = rt.op_gemm_route(2700, C, k * C, taps=k, dil=dil, operands=W3 | WH)[1]
                if span <= 64:
                    assert pair == OK and forced == [OK, OK] and chosen == WIN_X3H[C], (C, k, dil)
                elif k - 1 <= 64:
                    # conv2 alone (dilation 1) would fit a window tile: the pair still follows conv1
                    assert pair == NOT_SUPPORTED and forced == [INVALID, OK] and chosen != WIN_X3H[C], (C, k, dil)
                else:
                    assert pair == NOT_SUPPORTED and forced == [INVALID, INVALID] and chosen != WIN_X3H[C], (C, k, dil)


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
