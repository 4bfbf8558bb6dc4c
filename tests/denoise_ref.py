"""Restatement of the stationary-noise suppression rule (csrc/denoise.hip, include/megatts2_hip.h) in numpy.  Test helper: no GPU needed.

Everything runs in float64 by default, the two transforms as the FFTs of griffinlim_ref.  `dt=np.float32` is the rule as it is stated
for f32: every stored array and every operation of steps 2 to 6 is rounded to f32 exactly as the kernels round it (one fma for the
power, one product, one subtraction, one division and one max for the gain, ascending sums and one division for the two means, one
product per part for the gate), so that on the SAME spectrum the f32 run is bit-equal to the device.  The constants the rule fixes in
f32 (beta, g_min and the factor c) are the f32 values in both modes.  The order statistic is numpy's partition: exact, like the
kernel's radix select, and order-free."""
import dataclasses
import math

import numpy as np

import griffinlim_ref as G

FIELDS = ("noise_db", "snr_db", "floored_share", "reduction_db", "frames", "rank", "mean_frame_power", "noise_power")
TINY = np.finfo(np.float64).tiny


@dataclasses.dataclass(frozen=True)
class Config:
    percentile: int = 20
    over_subtraction: float = 3.0
    floor_gain: float = 0.1
    smooth_bins: int = 1
    smooth_frames: int = 1


def rank(T, percentile):
    """k = ((T - 1) percentile + 50) / 100 in integers"""
    return ((int(T) - 1) * int(percentile) + 50) // 100


def factor(percentile):
    """c = (float)(1 / -ln(1 - percentile / 100)): the mean of an exponential distribution over its `percentile` quantile"""
    return np.float32(1.0 / -math.log(1.0 - percentile / 100.0))


def out_len(L, audio):
    return audio.hop_length * (int(L) // audio.hop_length)


def fma_f32(a, b, c):
    """fmaf(a, b, c) for f32 arrays: a b is exact in float64; the sum is rounded to odd in float64 (TwoSum gives its error), which
    makes the final rounding to f32 the one rounding of the exact value"""
    a, b, c = np.broadcast_arrays(*(np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c)))
    with np.errstate(invalid="ignore", over="ignore"):
        ab = np.ascontiguousarray(a * b)
        s = np.ascontiguousarray(ab + c)
        bb = s - ab
        e = (ab - (s - bb)) + (c - bb)
        even = (s.reshape(-1).view(np.int64) & 1).reshape(s.shape) == 0
        fix = (e != 0) & np.isfinite(s) & even
        s = np.where(fix, np.nextafter(s, np.where(e > 0, np.inf, -np.inf)), s)
        return s.astype(np.float32)


def power(S, dt=np.float64):
    """step 2: S complex [T, F] -> P [T, F]"""
    re, im = S.real, S.imag
    if dt == np.float32:
        re, im = re.astype(np.float32), im.astype(np.float32)
        return fma_f32(im, im, re * re)
    return re * re + im * im


def noise_floor(P, percentile, dt=np.float64):
    """step 3: P [T, F] -> Nf [F]"""
    k = rank(P.shape[0], percentile)
    q = np.partition(np.asarray(P, dt), k, axis=0)[k]
    return (q * dt(factor(percentile))).astype(dt)


def gain0(P, Nf, cfg, dt=np.float64):
    """step 4"""
    P, Nf = np.asarray(P, dt), np.asarray(Nf, dt)
    beta, gmin = dt(np.float32(cfg.over_subtraction)), dt(np.float32(cfg.floor_gain))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = ((P - (beta * Nf[None, :]).astype(dt)).astype(dt) / P).astype(dt)
    return np.where(P > 0, np.maximum(gmin, q), gmin).astype(dt)


def mean_along(g, half, axis, dt=np.float64):
    """the mean over the existing cells within `half` along `axis`: sums in ascending index order, one division by the count"""
    g = np.moveaxis(np.asarray(g, dt), axis, 0)
    n = g.shape[0]
    s, cnt = np.zeros_like(g), np.zeros(n, np.int64)
    for d in range(-half, half + 1):
        lo, hi = max(0, -d), min(n, n - d)      # the cells i with 0 <= i + d < n
        if lo < hi:
            s[lo:hi] = (s[lo:hi] + g[lo + d:hi + d]).astype(dt)
            cnt[lo:hi] += 1
    out = (s / cnt.astype(dt).reshape((n,) + (1,) * (g.ndim - 1))).astype(dt)
    return np.moveaxis(out, 0, axis)


def smooth(g0, cfg, dt=np.float64):
    """step 5: along the bins, then along the frames"""
    return mean_along(mean_along(g0, cfg.smooth_bins, 1, dt), cfg.smooth_frames, 0, dt)


def gate(S, g, dt=np.float64):
    """step 6, the products"""
    if dt == np.float32:
        g = np.asarray(g, np.float32)
        return (g * S.real.astype(np.float32)).astype(np.float64) + 1j * (g * S.imag.astype(np.float32)).astype(np.float64)
    return S * g


def figures(P, Nf, g0, g, cfg, dt=np.float64):
    """step 7, in float64"""
    P64, N64, g64 = np.asarray(P, np.float64), np.asarray(Nf, np.float64), np.asarray(g, np.float64)
    T = P.shape[0]
    sP, sN = P64.sum(), N64.sum()
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array([10 * np.log10(sN), 10 * np.log10(max(sP / T - sN, TINY) / sN),
                         float((np.asarray(g0, dt) == dt(np.float32(cfg.floor_gain))).mean()), 10 * np.log10((g64 * g64 * P64).sum() / sP),
                         T, rank(T, cfg.percentile), sP / T, sN])


def denoise(x, audio, cfg=Config(), dt=np.float64, floor=None):
    """the whole rule for one utterance -> dict(y [hop (L // hop)], S, P, Nf, g0, g, figures)"""
    S = G.stft(x, audio, dt)
    P = power(S, dt)
    Nf = noise_floor(P, cfg.percentile, dt) if floor is None else np.asarray(floor, dt)
    g0 = gain0(P, Nf, cfg, dt)
    g = smooth(g0, cfg, dt)
    y = G.istft(gate(S, g, dt), audio, dt)
    return dict(y=y, S=S, P=P, Nf=Nf, g0=g0, g=g, figures=figures(P, Nf, g0, g, cfg, dt))


# ---- test signals --------------------------------------------------------------------------------------------------------------

SIGMA = 0.05
TONE_HZ = 440.0
TONE_AMP = SIGMA * math.sqrt(4.0 * 10.0 ** 0.7)      # a tone on half the time, 7 dB over the noise: (A^2 / 2) / 2 = 10^0.7 sigma^2


def white_noise(L, seed=0, sigma=SIGMA):
    return (sigma * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)


def tone(L, sample_rate=16000, gated=True, amp=TONE_AMP, hz=TONE_HZ):
    """440 Hz, on for alternate half-seconds when gated (off first)"""
    t = np.arange(L) / sample_rate
    x = amp * np.sin(2 * np.pi * hz * t)
    if gated:
        x = x * ((np.floor(t / 0.5).astype(np.int64) % 2) == 1)
    return x


def snr_db(y, clean):
    n = len(y)
    y, clean = np.asarray(y, np.float64), np.asarray(clean[:n], np.float64)
    return 10 * np.log10((clean ** 2).sum() / ((y - clean) ** 2).sum())


def level_db(y, x):
    """the power of y over that of x (over y's length), in dB"""
    n = len(y)
    return 10 * np.log10((np.asarray(y, np.float64) ** 2).sum() / (np.asarray(x[:n], np.float64) ** 2).sum())


def tone_amplitude(y, sample_rate=16000, hz=TONE_HZ):
    """the amplitude of the `hz` component of y, by projection"""
    t = np.arange(len(y)) / sample_rate
    return 2.0 * abs((np.asarray(y, np.float64) * np.exp(-2j * np.pi * hz * t)).sum()) / len(y)


def window_energy(audio):
    w = G.window(audio)
    return float((w * w).sum())
