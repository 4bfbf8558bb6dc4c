"""The four window-convolution kernel families at the limits their routes accept (win_eligible, csrc/gemm_dispatch.hip;
conv_pair_route, csrc/gemm_x3h.hip: any taps >= 2 with (taps - 1) * dil <= 64) and the model never reaches: the widest window (span
64, also as 65 taps - the pair's smallest output tile), spans off the window's 8-row rounding, even tap counts (one row more reach
to the right), the shortest K loops (two taps of 32 channels: fewer chunks than ring stages), 11 / 19 and more workgroups (the XCD
tile permutation is no identity) and the pair's last-tile edges.  Everything is compared with tests/winconv_ref.py - a float64 tap
sum per utterance - by the project's f32-equivalence rule, the pair also bit for bit with the two launches it replaces.

The f32 tile has the float64 bar of tests/test_gpu_kernels.py (3e-6) up to K = k * C = 1408, as far as those tests go.  Beyond it the
bar is twice the error of the general implicit-GEMM tile 12 (another kernel) on the same data, + 1e-7.  Measured on an MI355X
(profiles/window_conv_edges_errors.txt has every case), relative L2 error against float64, the worst utterance:
      C   k  dil      K    tile 12   f32 tile
     32  65    1   2080  8.196e-07  8.196e-07
     64  65    1   4160  1.151e-06  1.151e-06
    128  17    4   2176  8.271e-07  8.271e-07
    128  65    1   8320  1.615e-06  1.615e-06
(the two run the same fma chain per output element; x6 7.0e-07 ... 1.4e-06 and x3h 3.1e-07 ... 5.9e-07 on these four).
"""
import functools
import math

import numpy as np
import pytest

import winconv_ref as wr

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ACT_NONE, ACT_LRELU = 0, 2
SLOPE = 0.1
SENTINEL = 12345.0
BM = wr.BM
F32_CFG = {32: 30, 64: 31, 128: 32}             # conv_win_f32_kernel
X6_CFG = {32: 34, 64: 58, 128: 59}              # conv_win_x6_kernel
X3H_CFG = {32: 98, 64: 99, 128: 100}            # conv_win_x3h_kernel; the pair replaces two launches of these
GENERAL_CFG = 12                                # an implicit-GEMM tile: no window, no tile permutation of its own
K_COVERED = 1408                                # the largest k * C of the float64 bars in test_gpu_kernels.py

SPAN_64 = [(9, 8), (65, 1), (2, 64), (3, 32), (17, 4)]
OFF_ROUNDING = [(2, 1), (4, 21), (8, 9), (6, 11)]                   # even k; spans 1, 63, 63, 55
CASES = [(C, k, d) for C in (32, 64, 128) for k, d in SPAN_64 + OFF_ROUNDING] + [(32, 2, 5)]        # (2, 1), (2, 5) at C = 32: nk = 2
CASE_IDS = [f"C{C}-k{k}-d{d}" for C, k, d in CASES]
CHANNELS = pytest.mark.parametrize("C", [32, 64, 128], ids=lambda C: f"C{C}")


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def worst(out, ref, utts):
    return max(rel(out[s:e], ref[s:e]) for s, e in utts)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def blank(R, ld):
    return torch.full((R, ld), SENTINEL, device="cuda", dtype=torch.float32)


def bits(t):
    return t.contiguous().view(torch.int32)


def wide(rng, shape, decades):
    return rng.standard_normal(shape) * np.exp(rng.uniform(-decades, decades, shape))


def operands(C, k, dil, R, ldx, seed, valid=None):
    """Rows and weights with a wide dynamic range (the low planes of the split formats matter): x ~ randn exp(U(-4, 4)), zeros in
    masked rows and noise in the columns beyond C; W ~ randn exp(U(-2, 2)) / sqrt(C k)."""
    rng = np.random.default_rng(seed)
    X = wide(rng, (R, ldx), 4.0).astype(np.float32)
    if valid is not None:
        X[:, :C] *= valid[:, None].astype(np.float32)
    W1, W2 = (wide(rng, (2, C, k * C), 2.0) / math.sqrt(C * k)).astype(np.float32)
    b1, b2 = rng.standard_normal((2, C)).astype(np.float32)
    res = rng.standard_normal((R, C)).astype(np.float32)
    return X, W1, W2, b1, b2, res


@functools.lru_cache(maxsize=None)
def single_case(C, k, dil):
    valid, utts, _ = wr.row_layout(C, k, dil, fused=False)
    X, W, _, b, _, res = operands(C, k, dil, valid.shape[0], C, 1000 * C + 10 * k + dil, valid)
    ref = wr.over_rows(X, utts, lambda x, s, e: wr.single_ref(x, W, k, dil, b, res[s:e], SLOPE, SLOPE))
    return valid, utts, X, W, b, res, ref


@functools.lru_cache(maxsize=None)
def pair_case(C, k, dil):
    valid, utts, _ = wr.row_layout(C, k, dil, fused=True)
    X, W1, W2, b1, b2, _ = operands(C, k, dil, valid.shape[0], C + 8, 2000 * C + 10 * k + dil, valid)
    ref = wr.over_rows(X[:, :C], utts, lambda x, s, e: wr.pair_ref(x, W1, b1, W2, b2, k, dil, SLOPE))
    return valid, utts, X, W1, W2, b1, b2, ref


def two_launches(rt, launch, cfg, X, C, k, dil, W1, W2, b1, b2, valid, want_flag=False):
    """t1 = lrelu(conv1(lrelu(x)) + b1), y = x + conv2(t1) + b2 as two launches of one window tile."""
    pad = (k - 1) // 2
    R = X.shape[0]
    kw = dict(want_flag=True) if want_flag else {}
    t1 = launch(X, W1, b1, None, valid=valid, shift0=-pad * dil, taps=k, dil=dil, Cin=C, pro_act=ACT_LRELU, pro_slope=SLOPE,
                epi_act=ACT_LRELU, force_cfg=cfg, out=blank(R, C), **kw)
    t1, f1 = t1 if want_flag else (t1, 0)
    y = launch(t1, W2, b2, X, valid=valid, shift0=-pad, taps=k, dil=1, Cin=C, pro_act=ACT_NONE, pro_slope=SLOPE, epi_act=ACT_NONE,
               force_cfg=cfg, out=blank(R, C), **kw)
    y, f2 = y if want_flag else (y, 0)
    return y, f1, f2


def run_pair(rt, X, C, k, dil, W1, W2, b1, b2, valid):
    """(fused pair [R, C + 4] on sentinels, its flag, the two x3h launches, their flags, the two f32-tile launches)"""
    Xd, W1d, W2d, b1d, b2d = dev(X), dev(W1), dev(W2), dev(b1), dev(b2)
    vd = None if valid is None else dev(valid)
    want, f1, f2 = two_launches(rt, rt.op_conv_x3h, X3H_CFG[C], Xd, C, k, dil, W1d, W2d, b1d, b2d, vd, want_flag=True)
    got, flag = rt.op_conv_pair(Xd, W1d, b1d, W2d, b2d, k, dil, SLOPE, valid=vd, channels=C, out=blank(X.shape[0], C + 4),
                                want_flag=True)
    f32, _, _ = two_launches(rt, rt.op_gemm, F32_CFG[C], Xd, C, k, dil, W1d, W2d, b1d, b2d, vd)
    torch.cuda.synchronize()
    return got, flag, want, (f1, f2), f32


def check_pair(C, got, flag, want, flags2, f32, ref, utts, valid, tag):
    """Every claim about one fused launch: the two launches bit for bit, nothing outside its rows and columns, f32-equivalence."""
    assert torch.equal(bits(got[:, :C]), bits(want))
    assert flag == (flags2[0] | flags2[1]) == 0
    got, f32 = got.cpu().numpy(), f32.cpu().numpy()
    assert (got[:, C:] == SENTINEL).all()                               # nothing beyond the C columns
    assert not (got[:, :C] == SENTINEL).any()                           # every row is written ...
    assert not (f32 == SENTINEL).any()
    if valid is not None:
        assert not got[:, :C][valid == 0].any()                         # ... the masked ones as zeros
    err, err32 = worst(got[:, :C], ref, utts), worst(f32, ref, utts)
    print(f"EDGE_PAIR {tag} f32x2={err32:.3e} pair={err:.3e}")
    assert err <= 2.0 * err32 + 1e-7, (err, err32)


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    runtime.device_check()
    return runtime


@pytest.mark.parametrize("C,k,dil", CASES, ids=CASE_IDS)
def test_window_tiles_against_float64(rt, C, k, dil):
    """One convolution launch (leaky-ReLU prologue and epilogue, bias, residual, row mask) on the f32, x6 and x3h window tiles and on
    the general tile 12, over 11 / 19 row tiles with utterance boundaries in and beside the halos."""
    valid, utts, X, W, b, res, ref = single_case(C, k, dil)
    R, K = X.shape[0], k * C
    pad = (k - 1) // 2
    Xd, Wd, bd, rd = dev(X), dev(W), dev(b), dev(res)
    kw = dict(valid=dev(valid), shift0=-pad * dil, taps=k, dil=dil, Cin=C, pro_act=ACT_LRELU, pro_slope=SLOPE, epi_act=ACT_LRELU)
    f32 = rt.op_gemm(Xd, Wd, bd, rd, force_cfg=F32_CFG[C], out=blank(R, C), **kw).cpu().numpy()
    gen = rt.op_gemm(Xd, Wd, bd, rd, force_cfg=GENERAL_CFG, out=blank(R, C), **kw).cpu().numpy()
    x6 = rt.op_conv_x6(Xd, Wd, bd, rd, force_cfg=X6_CFG[C], out=blank(R, C), **kw).cpu().numpy()
    x3h, flag = rt.op_conv_x3h(Xd, Wd, bd, rd, force_cfg=X3H_CFG[C], out=blank(R, C), want_flag=True, **kw)
    x3h = x3h.cpu().numpy()
    err = {name: worst(out, ref, utts) for name, out in (("f32", f32), ("t12", gen), ("x6", x6), ("x3h", x3h))}
    print(f"EDGE_SINGLE C={C} k={k} dil={dil} K={K} " + " ".join(f"{n}={v:.3e}" for n, v in err.items()))
    for out in (f32, gen, x6, x3h):
        assert not (out == SENTINEL).any()                              # every row of every tile is written ...
        assert not out[valid == 0].any()                                # ... the masked ones as zeros
    assert flag == 0
    assert rel(f32, gen) < 2e-6
    if K <= K_COVERED:
        assert err["f32"] < 3e-6, err
    else:
        assert err["f32"] <= 2.0 * err["t12"] + 1e-7, err
    assert err["x6"] <= 2.0 * err["f32"] + 1e-7, err
    assert err["x3h"] <= 2.0 * err["f32"] + 1e-7, err


@pytest.mark.parametrize("C,k,dil", CASES, ids=CASE_IDS)
def test_pair_against_two_launches_and_float64(rt, C, k, dil):
    """y = x + conv2(lrelu(conv1(lrelu(x)))) on the fused kernel, on rows where utterance boundaries fall inside conv2's halo of one
    output tile, inside conv1's of another and strictly inside a third: the two x3h launches bit for bit, and float64 per utterance
    (a mask applied at the wrong stage in BOTH forms would pass the first and not the second)."""
    valid, utts, X, W1, W2, b1, b2, ref = pair_case(C, k, dil)
    got, flag, want, flags2, f32 = run_pair(rt, X, C, k, dil, W1, W2, b1, b2, valid)
    check_pair(C, got, flag, want, flags2, f32, ref, utts, valid, f"C={C} k={k} dil={dil} K={k * C}")


LAST_TILE_GEOM = (8, 9)                         # even k, span 63


@CHANNELS
@pytest.mark.parametrize("rows", ["bmo", "bmo+1", "2bmo", "11tiles"])
def test_pair_last_tile_edges(rt, C, rows):
    """R exactly one and two output tiles, a last tile of a single output row (every row an utterance row, by a mask of ones), and 11
    tiles with no row mask at all."""
    k, dil = LAST_TILE_GEOM
    bmo = BM[C] - (k - 1)
    assert rt.op_conv_pair_route(1000, C, k, dil)["bmo"] == bmo
    R = {"bmo": bmo, "bmo+1": bmo + 1, "2bmo": 2 * bmo, "11tiles": 10 * bmo + bmo // 2}[rows]
    assert rt.op_conv_pair_route(R, C, k, dil)["grid"] == {"bmo": 1, "bmo+1": 2, "2bmo": 2, "11tiles": 11}[rows]
    valid = None if rows == "11tiles" else np.ones(R, np.int32)
    X, W1, W2, b1, b2, _ = operands(C, k, dil, R, C + 8, 3000 * C + R)
    utts = [(0, R)]
    ref = wr.over_rows(X[:, :C], utts, lambda x, s, e: wr.pair_ref(x, W1, b1, W2, b2, k, dil, SLOPE))
    got, flag, want, flags2, f32 = run_pair(rt, X, C, k, dil, W1, W2, b1, b2, valid)
    check_pair(C, got, flag, want, flags2, f32, ref, utts, valid, f"C={C} k={k} dil={dil} R={rows}")


def changed_rows(a, b):
    return np.flatnonzero((bits(a) != bits(b)).any(dim=1).cpu().numpy())


@CHANNELS
@pytest.mark.parametrize("k,dil", [(9, 8), (4, 21)], ids=["k9-d8", "k4-d21"])
def test_one_input_row_reaches_exactly_its_window(rt, C, k, dil):
    """One input row r of a long utterance changes: the output rows that read it change, to the last one on either side, and NO other
    row changes by a bit - on the x3h window tile (r is the first row of tile 1: the rows that read it lie in tiles 0 and 1) and on the
    pair (r the first row of output tile 1; the rows the pair computes from stale planes and discards would show here)."""
    left, right = wr.reach(k, dil)
    pad = (k - 1) // 2
    rng = np.random.default_rng(C + k + dil)
    new_row = wide(rng, C, 2.0).astype(np.float32)
    # the window tile
    bm = BM[C]
    R = 3 * bm + 17
    X, W1, W2, b1, b2, _ = operands(C, k, dil, R, C, 4000 * C + k)
    valid = dev(np.ones(R, np.int32))
    r = bm
    assert r - right < bm <= r + left or left == 0
    kw = dict(valid=valid, shift0=-left, taps=k, dil=dil, Cin=C, pro_act=ACT_LRELU, pro_slope=SLOPE, epi_act=ACT_LRELU,
              force_cfg=X3H_CFG[C])
    X2 = X.copy()
    X2[r] = new_row
    a = rt.op_conv_x3h(dev(X), dev(W1), dev(b1), None, out=blank(R, C), **kw)
    b = rt.op_conv_x3h(dev(X2), dev(W1), dev(b1), None, out=blank(R, C), **kw)
    rows = changed_rows(a, b)
    assert rows.size and rows.min() == r - right and rows.max() == r + left, (rows.min(), rows.max(), r, left, right)
    # the pair: output row o reads t1 rows o - pad .. o + (k - 1 - pad), each of which reads x rows - left .. + right of itself
    bmo = bm - (k - 1)
    r = bmo
    lo, hi = r - (k - 1 - pad) - right, r + pad + left
    assert 0 <= lo < bmo <= hi < R
    X2 = X.copy()
    X2[r] = new_row
    args = (dev(W1), dev(b1), dev(W2), dev(b2), k, dil, SLOPE)
    a = rt.op_conv_pair(dev(X), *args, valid=valid, out=blank(R, C))
    b = rt.op_conv_pair(dev(X2), *args, valid=valid, out=blank(R, C))
    rows = changed_rows(a, b)
    assert rows.size and rows.min() == lo and rows.max() == hi, (rows.min(), rows.max(), lo, hi)
    assert not bool((a == SENTINEL).any()) and not bool((b == SENTINEL).any())
