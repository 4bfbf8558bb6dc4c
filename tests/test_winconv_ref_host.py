"""tests/winconv_ref.py (the float64 restatement the window-convolution kernel tests compare with) against
torch.nn.functional.conv1d in float64 on the CPU, odd and even tap counts, and the row layouts of the kernel tests.  No GPU."""
import numpy as np
import pytest

import winconv_ref as wr

torch = pytest.importorskip("torch")
F = torch.nn.functional

GEOMS = [(9, 8), (65, 1), (2, 64), (3, 32), (17, 4), (2, 1), (4, 21), (8, 9), (6, 11), (2, 5), (3, 1), (7, 3), (11, 5)]
SLOPE = 0.1


def torch_conv(x, W, k, dil, bias=None):
    """x [n, Cin], W [Cout, k * Cin] tap-major -> [n, Cout]: conv1d over the explicitly padded row axis (pad * dil zeros in front,
    (k - 1 - pad) * dil behind: one more tap's worth behind for even k)."""
    cin = x.shape[1]
    w = torch.from_numpy(np.asarray(W, np.float64)).reshape(W.shape[0], k, cin).permute(0, 2, 1).contiguous()       # [Cout, Cin, k]
    xt = torch.from_numpy(np.asarray(x, np.float64)).t()[None]                                                      # [1, Cin, n]
    pad = (k - 1) // 2
    xt = F.pad(xt, (pad * dil, (k - 1 - pad) * dil))
    b = None if bias is None else torch.from_numpy(np.asarray(bias, np.float64))
    return F.conv1d(xt, w, b, dilation=dil)[0].t().numpy()


def lrelu64(v):
    return F.leaky_relu(torch.from_numpy(np.asarray(v, np.float64)), float(np.float32(SLOPE))).numpy()


@pytest.mark.parametrize("k,dil", GEOMS)
@pytest.mark.parametrize("n", [1, 5, 130])
def test_conv_same_is_conv1d_with_explicit_padding(k, dil, n):
    rng = np.random.default_rng(k * 100 + dil + n)
    cin, cout = 6, 5
    x = rng.standard_normal((n, cin))
    W = rng.standard_normal((cout, k * cin))
    want = torch_conv(x, W, k, dil)
    got = wr.conv_same(x, W, k, dil)
    assert got.shape == want.shape == (n, cout)
    assert np.abs(got - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    left, right = wr.reach(k, dil)
    assert left + right == (k - 1) * dil and right - left == (0 if k % 2 else dil) and wr.min_gap(k, dil) == right


@pytest.mark.parametrize("k,dil", GEOMS)
def test_single_and_pair_restatements(k, dil):
    rng = np.random.default_rng(k * 7 + dil)
    C, n = 8, 97
    x = rng.standard_normal((n, C))
    W1, W2 = rng.standard_normal((2, C, k * C)) / np.sqrt(C * k)
    b1, b2 = rng.standard_normal((2, C))
    res = rng.standard_normal((n, C))
    want = lrelu64(torch_conv(lrelu64(x), W1, k, dil, b1)) + res
    got = wr.single_ref(x, W1, k, dil, b1, res, SLOPE, SLOPE)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    t1 = lrelu64(torch_conv(lrelu64(x), W1, k, dil, b1))
    want = x + torch_conv(t1, W2, k, 1, b2)
    got = wr.pair_ref(x, W1, b1, W2, b2, k, dil, SLOPE)
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("k,dil", [(2, 1), (4, 21), (9, 8)])
def test_rows_with_the_smallest_gap_are_the_utterances_on_their_own(k, dil):
    """The convolution over ALL gap-padded rows (zeros in the gaps), read at an utterance's rows, is the utterance's own zero-padded
    convolution when the gaps are min_gap rows - and no longer when one is a row shorter."""
    rng = np.random.default_rng(k + dil)
    C = 4
    G = wr.min_gap(k, dil)
    W = rng.standard_normal((C, k * C))
    for gap, same in ((G, True), (G - 1, False)):
        lens = [(k - 1) * dil + 3, 1, 40]
        utts, r = [], 0
        for n in lens:
            utts.append((r, r + n))
            r += n + gap
        X = np.zeros((r - gap, C))
        for s, e in utts:
            X[s:e] = rng.standard_normal((e - s, C)) + 3.0
        whole = wr.conv_same(X, W, k, dil)
        per = wr.over_rows(X, utts, lambda x, s, e: wr.conv_same(x, W, k, dil))
        agree = all(np.allclose(whole[s:e], per[s:e], rtol=0, atol=1e-12) for s, e in utts)
        assert agree == same


@pytest.mark.parametrize("C", [32, 64, 128])
@pytest.mark.parametrize("k,dil", GEOMS[:10])
@pytest.mark.parametrize("fused", [False, True])
def test_row_layouts_reach_the_edges_they_are_for(C, k, dil, fused):
    valid, utts, tile = wr.row_layout(C, k, dil, fused)             # asserts its own geometry
    R = valid.shape[0]
    assert tile == (wr.BM[C] - (k - 1) if fused else wr.BM[C])
    assert len(utts) == 5 and 2300 <= R <= 2816
    for nt in (-(-R // tile), -(-R // wr.BM[C])):                   # the pair's tiles and the window tiles of the same rows
        assert nt >= 9 and nt % 8 != 0
    assert any(e - s == 1 for s, e in utts)
