"""The fused MRF mean + stride-2 upsampler kernel (up_mrf_x3h_kernel, csrc/gemm_x3h.hip) against tests/upmrf_ref.py (float64 on the
f32 mean) and against the three launches it replaces (avg3, then the two phase GEMMs with the leaky-ReLU prologue) on the same data.

Bars (those of tests/test_gpu_window_conv_edges.py; K = 2 ch <= 256): relative L2 error against float64 below 3e-6 and at most twice the
three-launch form's + 1e-7.  The row sets put a tile boundary, a partial tile and an utterance boundary at every place where the q - 1 /
q + 1 taps of the two phases leave the tile or the row set."""
import functools

import numpy as np
import pytest

import upmrf_ref as ur

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ACT_LRELU = 2
SLOPE = 0.1
SENTINEL = 12345.0
GAP = 4
CHANNELS = pytest.mark.parametrize("ch", [64, 128], ids=lambda c: f"ch{c}")


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


def bm_of(ch):
    from megatts2_amd import runtime
    r = runtime.op_up_mrf_route(1000, ch)
    assert r["err"] == 0
    return r["bm"]


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def blank(R, ld):
    return torch.full((R, ld), SENTINEL, device="cuda", dtype=torch.float32)


@functools.lru_cache(maxsize=None)
def weights(ch):
    rng = np.random.default_rng(100 + ch)
    W = (rng.standard_normal((ch, ch // 2, 4)) * np.exp(rng.uniform(-1, 1, (ch, ch // 2, 4))) / np.sqrt(2 * ch)).astype(np.float32)
    b = rng.standard_normal(ch // 2).astype(np.float32)
    return ur.wcat_from_conv_transpose(W), b


def inputs(ch, R, seed, valid=None, gap_value=0.0):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal((3, R, ch)) * np.exp(rng.uniform(-2, 2, (3, R, ch)))).astype(np.float32)
    if valid is not None:
        x[:, valid == 0] = gap_value
    return x


def three_launches(rt, x, Wcat, b, valid, ch):
    """avg3 -> x; up[:, h co:(h + 1) co] = lrelu(x)[q - 1 + h], lrelu(x)[q + h] times the phase's rows of Wcat + bias, masked."""
    R, co = x.shape[1], ch // 2
    xs = [dev(a) for a in x]
    mean = torch.empty(R, ch, device="cuda", dtype=torch.float32)
    rt.op_avg3(xs[0], xs[1], xs[2], 1.0 / 3.0, mean, R * ch)
    halves = [rt.op_gemm(mean, dev(Wcat[h * co:(h + 1) * co]), dev(b), None, valid, shift0=h - 1, taps=2, dil=1, Cin=ch, M=R, N=co,
                         pro_act=ACT_LRELU, pro_slope=SLOPE) for h in (0, 1)]
    return torch.cat(halves, dim=1).cpu().numpy()


def fused(rt, x, Wcat, b, valid, ch, ldy):
    out = blank(x.shape[1], ldy)
    xs = [dev(a) for a in x]
    y, flag = rt.op_up_mrf(xs[0], xs[1], xs[2], torch.from_numpy(Wcat), dev(b), SLOPE, valid=valid, channels=ch, out=out, want_flag=True)
    torch.cuda.synchronize()
    return y.cpu().numpy(), flag


def check(rt, ch, x, valid_np, label):
    """the fused launch, dense and with ldy = 2 co + 4, against float64 and against the three launches"""
    Wcat, b = weights(ch)
    valid = dev(valid_np) if valid_np is not None else None
    ref = ur.up_mrf_ref(x[0], x[1], x[2], Wcat, b, valid_np, ur.SCALE, SLOPE)
    err_three = rel(three_launches(rt, x, Wcat, b, valid, ch), ref)
    for ldy in (ch, ch + 4):
        got, flag = fused(rt, x, Wcat, b, valid, ch, ldy)
        err_fused = rel(got[:, :ch], ref)
        print(f"up_mrf {label} ch={ch} R={x.shape[1]} ldy={ldy}: err_fused {err_fused:.3e} err_three_launch {err_three:.3e}")
        assert (got[:, ch:] == SENTINEL).all()                           # nothing beyond column 2 co
        assert not (got[:, :ch] == SENTINEL).any()                        # every row is written
        if valid_np is not None:
            assert not got[:, :ch][valid_np == 0].any()                   # masked rows: exact zeros
        assert flag == 0
        assert err_fused <= 2 * err_three + 1e-7
        assert err_fused < 3e-6


@CHANNELS
@pytest.mark.parametrize("rows", ["1", "bm-1", "bm", "bm+1", "11bm-5"])
def test_row_counts_around_the_tile(rt, ch, rows):
    bm = bm_of(ch)
    R = {"1": 1, "bm-1": bm - 1, "bm": bm, "bm+1": bm + 1, "11bm-5": 11 * bm - 5}[rows]
    if rows == "11bm-5":
        r = rt.op_up_mrf_route(R, ch)
        assert r["grid"] == 11 and r["grid"] % 8 != 0 and R % bm != 0    # the XCD tile permutation is no identity; a partial last tile
    check(rt, ch, inputs(ch, R, 7 * ch + R), None, rows)


def ragged(ch):
    """three utterances: A ends on the last row of tile 0 (its q + 1 tap reads a gap row of tile 1), C starts on the first row of tile 2
    (its q - 1 tap reads a gap row of tile 1), B lies inside tile 1; the rows behind C are masked up to a partial last tile."""
    bm = bm_of(ch)
    utts = [(3, bm), (bm + GAP, 2 * bm - GAP), (2 * bm, 2 * bm + 57)]
    R = 2 * bm + 64
    valid = np.zeros(R, np.int32)
    for s, e in utts:
        valid[s:e] = 1
    assert valid[bm - 1] == 1 and valid[bm] == 0 and valid[2 * bm - 1] == 0 and valid[2 * bm] == 1 and R % bm != 0
    return valid


@CHANNELS
@pytest.mark.parametrize("gap_value", [0.0, 3.0], ids=["zero-gaps", "sentinel-gaps"])
def test_ragged_utterances_across_tiles(rt, ch, gap_value):
    valid = ragged(ch)
    check(rt, ch, inputs(ch, valid.shape[0], 11 + ch, valid, gap_value), valid, "ragged gap=%g" % gap_value)


@CHANNELS
def test_range_flag(rt, ch):
    """one input element that lifts |mean| over the fp16 range raises the flag; ordinary data does not (check() asserts that)"""
    valid = ragged(ch)
    Wcat, b = weights(ch)
    x = inputs(ch, valid.shape[0], 13 + ch, valid)
    x[1, 5, 7] = 3.0 * 7.0e4
    m = ur.mean_lrelu_f32(x[0], x[1], x[2], ur.SCALE, SLOPE)
    assert np.abs(m).max() > 65504.0
    _, flag = fused(rt, x, Wcat, b, dev(valid), ch, ch)
    assert flag != 0
    # ... also through the negative branch of the leaky ReLU only when the result itself leaves the range
    x[1, 5, 7] = -3.0 * 7.0e4
    assert np.abs(ur.mean_lrelu_f32(x[0], x[1], x[2], ur.SCALE, SLOPE)).max() < 65504.0
    _, flag = fused(rt, x, Wcat, b, dev(valid), ch, ch)
    assert flag == 0


def test_small_hifigan_waveforms_with_and_without_the_fusion(rt):
    """a generator whose last two stages are 128 -> 64 and 64 -> 32 at stride 2: both boundaries run fused with up_fuse = 3, none with 0"""
    from megatts2_amd import config as C
    from megatts2_amd import megatts2 as M
    from megatts2_amd import weights as Wt
    cfg = C.HifiGanConfig(in_dim=80, upsample_initial_channel=256, upsample_rates=[2, 2, 2], upsample_kernel_sizes=[4, 4, 4])
    sd = Wt.synth_state_dict(Wt.inventory_hifigan(cfg), 0, "hifigan.")
    voc = M.HIFIGAN(cfg, sd)
    rng = np.random.default_rng(5)
    lens = np.asarray([150, 97, 131], np.int32)
    mel = np.zeros((3, 80, 150), np.float32)
    for i, n in enumerate(lens):
        mel[i, :, :n] = rng.standard_normal((80, n)) * 0.5
    x = torch.from_numpy(mel).cuda()
    # the boundaries: stage 0's mean (128 channels, 2 rows per frame) and stage 1's (64 channels, 4 rows per frame)
    for ch, rows in ((128, 2 * int(lens.sum())), (64, 4 * int(lens.sum()))):
        assert rt.op_up_mrf_route(rows, ch, up_fuse=3)["err"] == 0
        assert rt.op_up_mrf_route(rows, ch, up_fuse=0)["err"] == 801
    assert rt.op_up_mrf_route(2 * int(lens.sum()), 256)["err"] == 801            # conv_pre's output is no MRF mean; 256 channels never fuse
    wav = {}
    for mask in (3, 0):
        voc.native.set_option("up_fuse", mask)
        assert voc.native.get_option("up_fuse") == mask
        wav[mask] = voc.decode_batch(x, mel_lens=lens).cpu().numpy()
    assert wav[0].any()
    err = rel(wav[3], wav[0])
    print(f"small HiFi-GAN: rel L2 of up_fuse=3 against up_fuse=0 {err:.3e}")
    assert not np.array_equal(wav[3], wav[0])       # another kernel did run: the fp16-pipe products are no f32 fma chain
    assert err < 1e-5
