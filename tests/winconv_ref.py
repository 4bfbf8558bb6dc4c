"""Float64 numpy restatement of the vocoder's window convolutions and of the fused resblock pair, for any tap count (even ones too),
and the gap-padded row layouts the kernel tests run them on.  No GPU, no torch: tests/test_winconv_ref_host.py checks the
convolution against torch.nn.functional.conv1d, tests/test_gpu_window_conv_edges.py checks the kernels against it.

Conventions (csrc/gemm_dispatch.hip, csrc/gemm_x3h.hip): rows are time, W is [Cout, k * Cin] tap-major (W[:, t * Cin:(t + 1) * Cin] is
tap t), pad = (k - 1) // 2 and
    out[i] = sum_t W_t @ act(x[i + shift0 + t * dil]),   shift0 = -pad * dil,
so a row reaches pad * dil rows to the left and (k - 1 - pad) * dil rows to the right: one row more on the right for even k."""
import numpy as np

BM = {32: 256, 64: 256, 128: 128}               # rows per pass of every window tile and of the pair, per channel count


def reach(k, dil):
    """(left, right) rows a convolution's output row reads beside its own."""
    pad = (k - 1) // 2
    return pad * dil, (k - 1 - pad) * dil


def min_gap(k, dil):
    """The smallest legal gap between two utterances: the larger (right) reach.  Zeros there are the zero padding of both."""
    return reach(k, dil)[1]


def lrelu(v, slope):
    return np.where(v >= 0, v, v * np.float64(np.float32(slope)))


def conv_same(x, W, k, dil):
    """x [n, Cin] -> [n, Cout] in float64: the explicit tap sum over the zero-padded utterance."""
    x = np.asarray(x, np.float64)
    W = np.asarray(W, np.float64)
    n, cin = x.shape
    assert W.shape[1] == k * cin
    left, right = reach(k, dil)
    xp = np.zeros((n + left + right, cin))
    xp[left:left + n] = x
    out = np.zeros((n, W.shape[0]))
    for t in range(k):
        out += xp[t * dil:t * dil + n] @ W[:, t * cin:(t + 1) * cin].T
    return out


def single_ref(x, W, k, dil, bias=None, res=None, pro_slope=None, epi_slope=None):
    """One launch on one utterance: epi(conv(pro(x)) + bias) + res (activations: leaky ReLU of that slope, None = identity)."""
    a = np.asarray(x, np.float64)
    if pro_slope is not None:
        a = lrelu(a, pro_slope)
    y = conv_same(a, W, k, dil)
    if bias is not None:
        y = y + np.asarray(bias, np.float64)
    if epi_slope is not None:
        y = lrelu(y, epi_slope)
    if res is not None:
        y = y + np.asarray(res, np.float64)
    return y


def pair_ref(x, W1, b1, W2, b2, k, dil, slope):
    """The resblock pair on one utterance: y = x + conv2(lrelu(conv1(lrelu(x)) + b1)) + b2, conv1 dilated, conv2 dilation 1, each
    zero-padded at the utterance's ends."""
    t1 = single_ref(x, W1, k, dil, b1, None, slope, slope)
    return single_ref(t1, W2, k, 1, b2, x, None, None)


def over_rows(X, utts, fn):
    """fn per utterance of the gap-padded rows X [R, C]; rows outside every utterance (masked rows) are zeros."""
    X = np.asarray(X, np.float64)
    out = None
    for s, e in utts:
        y = fn(X[s:e], s, e)
        if out is None:
            out = np.zeros((X.shape[0], y.shape[1]))
        out[s:e] = y
    return out


def row_layout(C, k, dil, fused):
    """(valid [R] int32, utterances [(start, end)], tile) for the window tiles of C channels (fused=False: output tiles of bm rows, halo
    = the convolution's reach) or for the fused pair (fused=True: output tiles of bmo = bm - (k - 1) rows, conv2's halo of pad / k - 1 -
    pad rows and conv1's reach beyond it).  Five utterances separated by the smallest legal gap, none in front and none behind:
      A ends one row short of tile 1: the gap starts inside the innermost halo in front of tile 1 (k = 2 has no left halo: B then
        starts inside tile 0's right halo);
      B ends inside conv1's halo in front of tile 3;
      C is one row;
      D is long and ends strictly inside a tile near the end;
      E is no longer than span - 1 rows (one row when the span is 1 or 2) and ends the buffer.
    R makes the bm-row tiles launch 11 (bm = 256) or 19 (bm = 128) workgroups and the tiles of `tile` rows a count 8 q + r, q >= 1,
    0 < r < 8: the XCD permutation of the kernels is no identity and no plain transposition."""
    bm = BM[C]
    pad = (k - 1) // 2
    span = (k - 1) * dil
    tile = bm - (k - 1) if fused else bm
    hl2, hr2 = (pad, k - 1 - pad) if fused else (0, 0)
    hl1, hr1 = reach(k, dil)
    G = min_gap(k, dil)
    target = 11 if bm == 256 else 19
    lo, hi = (target - 1) * bm + 1, target * bm
    a_end = tile - 1
    b_start = a_end + G
    b_end = 3 * tile - hl2 - 1
    c_start = b_end + G
    c_end = c_start + 1
    d_start = c_end + G
    short = max(1, span - 1)
    inner = tile - hl2 - hl1                       # rows of a tile in front of the next tile's halos
    for i3 in range(hi // tile, 4, -1):
        d_end = i3 * tile + (max(1, min(100, inner // 2)) if inner >= 2 else tile // 2)
        e_start = d_end + G
        R = e_start + short
        nt = -(-R // tile)
        if lo <= R <= hi and nt >= 9 and nt % 8 != 0 and d_end - d_start > 2 * span + 2:
            break
    else:
        raise AssertionError(("no layout", C, k, dil, fused))
    utts = [(0, a_end), (b_start, b_end), (c_start, c_end), (d_start, d_end), (e_start, R)]
    valid = np.zeros(R, np.int32)
    for s, e in utts:
        valid[s:e] = 1
    # what the layout is for
    assert all(e > s for s, e in utts) and all(utts[i + 1][0] - utts[i][1] == G for i in range(4))
    assert valid[0] and valid[-1] and int(valid.sum()) == sum(e - s for s, e in utts)
    assert -(-R // bm) == target and nt >= 9 and 0 < nt % 8
    if pad >= 1:
        assert tile - max(hl2, 1) <= a_end < tile                                   # the innermost halo in front of tile 1
        assert 3 * tile - hl2 - hl1 <= b_end < 3 * tile - hl2                       # conv1's halo in front of tile 3
    else:
        assert tile <= b_start < tile + hr2 + hr1 + 1                               # k = 2: tile 0's right halo
    assert i3 * tile < d_end < (i3 + 1) * tile                                      # inside tile i3 ...
    if inner >= 2:
        assert d_end < (i3 + 1) * tile - hl2 - hl1                                  # ... and in front of the next tile's halos
    assert c_end - c_start == 1 and 1 <= R - e_start <= max(1, span - 1)
    return valid, utts, tile
