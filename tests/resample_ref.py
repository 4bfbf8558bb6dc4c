"""The resampling rule of csrc/resample.hip restated in numpy float64 (no GPU, no library): the Kaiser-windowed-sinc polyphase
filter in the form torchaudio documents for resample(..., resampling_method="sinc_interp_kaiser") with its "kaiser_best" constants.

    g = gcd(sr_in, sr_out);  o = sr_in / g;  n = sr_out / g
    base  = min(o, n) * rolloff;  width = ceil(lpw * o / base);  K = 2 * width + o
    t[p][k] = clamp((-p / n + (k - width) / o) * base, -lpw, +lpw)
    h[p][k] = sinc(pi t) * I0(beta * sqrt(1 - (t / lpw)^2)) / I0(beta) * (base / o)
    y[i * n + p] = sum_k h[p][k] * x[i * o - width + k],  x = 0 outside [0, L),  y cut to ceil(n * L / o)
"""
import math

import numpy as np

LPW = 64
ROLLOFF = 0.9475937167399596
BETA = 14.769656459379492
RATES = (48000, 44100, 22050, 24000, 8000, 32000, 11025)      # the rates the tests resample to 16 kHz


def rule(sr_in, sr_out):
    """-> (o, n, width, K)"""
    g = math.gcd(sr_in, sr_out)
    o, n = sr_in // g, sr_out // g
    base = min(o, n) * ROLLOFF
    width = math.ceil(LPW * o / base)
    return o, n, width, 2 * width + o


def out_len(sr_in, sr_out, L):
    o, n, _, _ = rule(sr_in, sr_out)
    return -((-n * L) // o)


def table(sr_in, sr_out):
    """h [n, K] float64"""
    o, n, width, K = rule(sr_in, sr_out)
    base = min(o, n) * ROLLOFF
    p = np.arange(n, dtype=np.float64)[:, None]
    k = np.arange(K, dtype=np.float64)[None, :]
    t = np.clip((-p / n + (k - width) / o) * base, -LPW, LPW)
    window = np.i0(BETA * np.sqrt(1.0 - (t / LPW) ** 2)) / np.i0(BETA)
    a = t * math.pi
    sinc = np.where(a == 0.0, 1.0, np.sin(a) / np.where(a == 0.0, 1.0, a))
    return sinc * (window * (base / o))


def apply(h, x, o, width, L_out):
    """y [L_out] float64 = the rule's sum with the table h [n, K] (any float type; the sum runs in float64) over the samples x"""
    n, K = h.shape
    x = np.asarray(x, np.float64)
    nblk = -(-L_out // n)
    xp = np.zeros(width + max(x.size, (nblk - 1) * o + K - width) + K, np.float64)
    xp[width:width + x.size] = x
    frames = np.lib.stride_tricks.sliding_window_view(xp, K)[:nblk * o:o]          # frames[i, k] = x[i * o - width + k]
    return (frames @ np.asarray(h, np.float64).T).reshape(-1)[:L_out]


def bound(h, x, o, width, L_out):
    """sum_k |h[p][k]| |x[i * o - width + k]| per output sample: the scale of an f32 dot product's forward error bound"""
    return apply(np.abs(np.asarray(h, np.float64)), np.abs(np.asarray(x, np.float64)), o, width, L_out)


def resample(x, sr_in, sr_out):
    o, _, width, _ = rule(sr_in, sr_out)
    return apply(table(sr_in, sr_out), x, o, width, out_len(sr_in, sr_out, len(x)))


def normalize(y):
    """y / max |y| in f32 with one rounding per sample; unchanged while the peak is below FLT_MIN (audio_io.normalize)"""
    y = np.asarray(y, np.float32)
    peak = np.float32(np.max(np.abs(y))) if y.size else np.float32(0)
    return y if peak < np.finfo(np.float32).tiny else (y / peak).astype(np.float32)


def tones(sr, L, sr_in, sr_out=16000):
    """the three-tone test signal of a sr_in -> sr_out conversion, sampled at rate sr (either of the two): 110 Hz, 997 Hz and
    0.42 * min(sr_in, sr_out) Hz - the last one close under the lower Nyquist frequency -, unit amplitude each"""
    t = np.arange(L, dtype=np.float64) / sr
    return sum(np.sin(2.0 * math.pi * f * t + ph) for f, ph in ((110.0, 0.1), (997.0, 0.7), (0.42 * min(sr_in, sr_out), 1.3)))
