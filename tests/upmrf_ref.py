"""float64 restatement of the fused MRF mean + stride-2 transposed convolution (up_mrf_x3h_kernel, csrc/gemm_x3h.hip), with co = ch / 2,
h(n) = (n >= co) and rows outside [0, R) reading as zeros:

    m[r, c] = lrelu(((x0[r, c] + x1[r, c]) + x2[r, c]) * scale)            float32, avg3_kernel's operation order
    Y[q, n] = valid[q] ? bias[n mod co] + sum_c m[q - 1 + h, c] Wcat[n, c] + sum_c m[q + h, c] Wcat[n, ch + c] : 0

The mean and the leaky ReLU are taken in float32 first, so the float64 sums see the values the kernel sees; gap rows of the inputs are
read as they are.  Y is [R, 2 co], which is [2 R, co] time-major."""
import numpy as np

SCALE = float(np.float32(1.0) / np.float32(3.0))


def mean_lrelu_f32(x0, x1, x2, scale, slope):
    """lrelu(((x0 + x1) + x2) * scale) in float32 (v >= 0 ? v : v * slope)."""
    x0, x1, x2 = (np.asarray(a, np.float32) for a in (x0, x1, x2))
    m = ((x0 + x1) + x2) * np.float32(scale)
    return np.where(m >= 0, m, m * np.float32(slope)).astype(np.float32)


def wcat_from_conv_transpose(W):
    """ConvTranspose1d(ch, co, kernel 4, stride 2, padding 1) weights [ch, co, 4] -> Wcat [2 co, 2 ch], the lo / hi tap split of
    csrc/model_load.hip at stride 2: rows 0 .. co - 1 (phase 0: input rows q - 1, q) take taps 3, 1; rows co .. (phase 1: rows q, q + 1)
    take taps 2, 0."""
    W = np.asarray(W)
    ch, co, k = W.shape
    assert k == 4 and 2 * co == ch
    lo = np.concatenate([W[:, :, 3].T, W[:, :, 1].T], axis=1)
    hi = np.concatenate([W[:, :, 2].T, W[:, :, 0].T], axis=1)
    return np.ascontiguousarray(np.concatenate([lo, hi], axis=0))


def up_mrf_ref(x0, x1, x2, Wcat, bias, valid=None, scale=SCALE, slope=0.1):
    """Y [R, 2 co] float64."""
    R, ch = np.asarray(x0).shape
    co = ch // 2
    Wcat = np.asarray(Wcat, np.float64)
    assert Wcat.shape == (2 * co, 2 * ch)
    mp = np.zeros((R + 2, ch), np.float64)                  # mp[r + 1] = m[r]
    mp[1:R + 1] = mean_lrelu_f32(x0, x1, x2, scale, slope)
    b = np.zeros(co) if bias is None else np.asarray(bias, np.float64)
    Y = np.empty((R, 2 * co), np.float64)
    for h in (0, 1):
        W = Wcat[h * co:(h + 1) * co]
        Y[:, h * co:(h + 1) * co] = b + mp[h:h + R] @ W[:, :ch].T + mp[h + 1:h + 1 + R] @ W[:, ch:].T
    if valid is not None:
        Y[np.asarray(valid) == 0] = 0.0
    return Y
