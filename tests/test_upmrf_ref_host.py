"""tests/upmrf_ref.py against torch.nn.functional.conv_transpose1d(lrelu(mean), W, b, stride=2, padding=1) in float64, no GPU: the rule
the fused MRF mean + upsampler kernel is held to is the transposed convolution of the model, through the lo / hi tap split of
csrc/model_load.hip."""
import numpy as np
import pytest

import upmrf_ref as ur

torch = pytest.importorskip("torch")

SLOPE = 0.1


def make(ch, R, seed):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((3, R, ch)).astype(np.float32)
    W = (rng.standard_normal((ch, ch // 2, 4)) / np.sqrt(2 * ch)).astype(np.float32)
    b = rng.standard_normal(ch // 2).astype(np.float32)
    return x, W, b


def torch_rows(m, W, b):
    """conv_transpose1d over the rows of m [T, ch] -> [T, 2 co] (= [2 T, co] time-major), float64"""
    y = torch.nn.functional.conv_transpose1d(torch.from_numpy(m.astype(np.float64)).T[None], torch.from_numpy(W.astype(np.float64)),
                                             torch.from_numpy(b.astype(np.float64)), stride=2, padding=1)[0]
    assert y.shape == (W.shape[1], 2 * m.shape[0])
    return y.T.reshape(m.shape[0], 2 * W.shape[1]).numpy()


@pytest.mark.parametrize("ch", [64, 128])
def test_single_utterance_is_conv_transpose1d(ch):
    R = 37
    x, W, b = make(ch, R, ch)
    m = ur.mean_lrelu_f32(x[0], x[1], x[2], ur.SCALE, SLOPE)
    want = torch_rows(m, W, b)
    for valid in (None, np.ones(R, np.int32)):
        got = ur.up_mrf_ref(x[0], x[1], x[2], ur.wcat_from_conv_transpose(W), b, valid, ur.SCALE, SLOPE)
        assert got.shape == (R, ch)
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


@pytest.mark.parametrize("ch", [64, 128])
def test_ragged_rows_with_gaps_are_per_utterance_transposed_convolutions(ch):
    utts = [(0, 9), (11, 30), (31, 32), (36, 50)]           # gaps of 2, 1 and 4 rows; a one-row utterance
    R = 52
    valid = np.zeros(R, np.int32)
    for s, e in utts:
        valid[s:e] = 1
    x, W, b = make(ch, R, 7 + ch)
    x *= valid[None, :, None].astype(np.float32)            # the gap rows of an activation are zeros
    got = ur.up_mrf_ref(x[0], x[1], x[2], ur.wcat_from_conv_transpose(W), b, valid, ur.SCALE, SLOPE)
    assert not got[valid == 0].any()
    for s, e in utts:
        want = torch_rows(ur.mean_lrelu_f32(x[0, s:e], x[1, s:e], x[2, s:e], ur.SCALE, SLOPE), W, b)
        assert np.abs(got[s:e] - want).max() <= 1e-12 * np.abs(want).max()
    # gap rows are read as they are: a sentinel there reaches the neighbouring utterance rows, exactly as over the whole row set
    x[:, valid == 0] = 3.0
    got = ur.up_mrf_ref(x[0], x[1], x[2], ur.wcat_from_conv_transpose(W), b, valid, ur.SCALE, SLOPE)
    want = torch_rows(ur.mean_lrelu_f32(x[0], x[1], x[2], ur.SCALE, SLOPE), W, b)
    want[valid == 0] = 0.0
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_the_mean_keeps_avg3s_order_and_the_leaky_relu_its_expression():
    import rowops_ref as rr
    rng = np.random.default_rng(3)
    a, b, d = (rng.standard_normal(4096) * np.exp(rng.uniform(-6, 6, 4096))).astype(np.float32).reshape(1, -1).repeat(3, 0) * \
        np.asarray([[1.0], [-0.999], [1e-3]], np.float32)
    mean = rr.avg3_f32(a, b, d, 1.0 / 3.0)
    want = np.where(mean >= 0, mean, mean * np.float32(SLOPE)).astype(np.float32)
    assert np.array_equal(ur.mean_lrelu_f32(a, b, d, ur.SCALE, SLOPE), want)
