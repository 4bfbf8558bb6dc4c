"""Float64 restatement of the true-peak look-ahead limiter of csrc/limiter.hip (include/megatts2_hip.h, "True-peak look-ahead
limiter"): the envelope over the interpolator of tests/ebu_ref.py, the need, the hold, the Hann smoothing and the clamp, the trim and
the passes of the normalising form over the loudness of tests/loudness_ref.py; both are imported unchanged.  Everything runs in double
over the f32 inputs, the f32 table and the f32 weights; G, c and t are the f32 values the rule states, and a pass's output is rounded
to f32 where the rule stores it."""
import functools
import math

import numpy as np

import ebu_ref as E
import loudness_ref as R

Z = E.Z
TILE, MAX_H, MAX_PASSES, FIELDS = 1024, 1024, 4, 24


def half_window(sr, window_ms=5.0):
    return int(math.floor(sr * window_ms / 1000.0 + 0.5))


@functools.lru_cache(maxsize=None)
def window64(H):
    """w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (2 H + 2)), k = 0 .. 2 H, divided by their sum (added ascending)"""
    v = [0.5 - 0.5 * math.cos(2.0 * math.pi * float(k + 1) / float(2 * H + 2)) for k in range(2 * H + 1)]
    total = 0.0
    for a in v:
        total += a
    w = np.asarray([a / total for a in v])
    w.flags.writeable = False
    return w


def window(H):
    """the weights as the library holds them: rounded once to f32"""
    return window64(H).astype(np.float32)


def ceiling(ceiling_dbtp):
    return np.float32(10.0 ** (ceiling_dbtp / 20.0))


def envelope(x, sr):
    """E[i] = max(e[i - 1], e[i]), e[i] = max_p |y[i o + p]| for i in [-1, L): a NaN never wins, an Inf does"""
    y = np.abs(E.interpolate(x, sr))                                          # row r is position r - Z
    e = np.fmax.reduce(y, axis=1, initial=0.0)
    L = np.asarray(x).size
    return np.fmax(e[Z - 1:Z - 1 + L], e[Z:Z + L])


def need_of(env, G, c):
    a = float(G) * np.asarray(env, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(a > float(c), float(c) / np.where(a > float(c), a, 1.0), 1.0)


def hold(need, H):
    """m[i] = min of need over [i - H, i + H], need = 1 outside; for i in [-H, L + H): m[H + i]"""
    p = np.concatenate([np.ones(2 * H), need, np.ones(2 * H)])
    return np.lib.stride_tricks.sliding_window_view(p, 2 * H + 1).min(axis=1)


def smooth(need, H):
    """s[i] = min(need[i], 1 - sum_k w[k] (1 - m[i - H + k])) over the f32 weights"""
    m = hold(need, H)
    d = np.convolve(1.0 - m, window(H).astype(np.float64)[::-1], mode="valid")
    return np.minimum(need, 1.0 - d)


def limit(x, sr, G, ceiling_dbtp, H):
    """steps 2-5 -> dict: out (double, before the f32 rounding), s, need, env"""
    x = np.asarray(x, np.float32)
    env = envelope(x, sr)
    need = need_of(env, G, ceiling(ceiling_dbtp))
    s = smooth(need, H)
    with np.errstate(invalid="ignore", over="ignore"):
        out = x.astype(np.float64) * float(G) * s
    return dict(out=out, s=s, need=need, env=env)


def trim(out32, sr, ceiling_dbtp):
    """step 6 -> (TP', t as f32): toward zero, never over the ceiling"""
    c = ceiling(ceiling_dbtp)
    tp = E.true_peak(out32, sr)
    if not tp > float(c):
        return tp, np.float32(1.0)
    q = float(c) / tp
    t = np.float32(q)
    if float(t) > q:
        t = np.nextafter(t, np.float32(0))
    return tp, t


def one_pass(x, sr, G, ceiling_dbtp, H):
    """steps 2-6 with the f32 gain G -> dict: out f32, s, need, tp (before the trim), t, min_s, limited"""
    r = limit(x, sr, np.float32(G), ceiling_dbtp, H)
    out = r["out"].astype(np.float32)
    tp, t = trim(out, sr, ceiling_dbtp)
    if t != 1.0:
        out = out * t
    return dict(out=out, s=r["s"], need=r["need"], tp=tp, t=t, min_s=float(r["s"].min()), limited=int((r["s"] < 1.0).sum()), G=np.float32(G))


def normalize(x, sr, target, ceiling_dbtp, H, passes):
    """step 7 -> the list of the passes' dicts, each with `I`, the loudness of its output; an utterance whose loudness is not finite
    comes back as one pass with out = x"""
    x = np.asarray(x, np.float32)
    I0 = R.measure(x, sr)["I"]
    with np.errstate(over="ignore"):
        G = np.float32(10.0 ** ((target - I0) / 20.0)) if np.isfinite(I0) else np.float32(np.inf)
    if not np.isfinite(G):
        return [dict(out=x.copy(), s=np.ones(x.size), need=np.ones(x.size), tp=E.true_peak(x, sr), t=np.float32(1), min_s=1.0, limited=0,
                     G=np.float32(1), I=I0)]
    res = []
    for k in range(passes):
        p = one_pass(x, sr, G, ceiling_dbtp, H)
        p["I"] = R.measure(p["out"], sr)["I"]
        res.append(p)
        with np.errstate(over="ignore"):
            nxt = np.float32(float(G) * 10.0 ** ((target - p["I"]) / 20.0)) if np.isfinite(p["I"]) else G
        if np.isfinite(nxt):
            G = nxt
    return res


def need_bound(sr, xmax, G, ceiling_dbtp):
    """what the device's need can differ by from the restatement's: E carries the error of one f32 fma chain (ebu_ref.chain_bound - the
    max of two lists differs by no more than their elements do), a = G E one rounding more, c / a another; need = c / a falls from 1
    with slope c / a^2 <= 1 / c, and it is continuous where a crosses c, so a flipped comparison moves it by no more"""
    return float(G) * E.chain_bound(sr, xmax) / float(ceiling(ceiling_dbtp)) + 3.0 * 2.0 ** -24


def smooth_bound(H):
    """what the f32 fma chain of 2 H + 1 terms, the subtraction 1 - m and the last 1 - d can lose: every term is in [0, 1] and the
    weights add up to 1"""
    return (2 * H + 1 + 4) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def pulse_signal(sr=16000, seconds=5.0, tone=0.05, pulse=0.8):
    """a 1 kHz tone of amplitude `tone` with nineteen band-limited pulses of amplitude `pulse`, one every 250 ms: a half-band sinc
    under a raised cosine of 32 samples a side, its centre 0.37 of a sample off the grid.  The crests are 24 dB over the body."""
    n = int(seconds * sr)
    i = np.arange(n)
    x = tone * np.sin(2.0 * np.pi * 1000.0 * i / sr)
    for k in range(1, 20):
        u = i - (k * (sr // 4) + 0.37)
        x += pulse * np.sinc(0.5 * u) * np.where(np.abs(u) < 32, 0.5 + 0.5 * np.cos(np.pi * u / 32.0), 0.0)
    x = x.astype(np.float32)
    x.flags.writeable = False
    return x


@functools.lru_cache(maxsize=None)
def pulse_case(target, passes=3, H=80, ceiling_dbtp=-1.0):
    """the normalising form on the pulse signal (each pass's out is left as it is: read only)"""
    return normalize(pulse_signal(), 16000, target, ceiling_dbtp, H, passes)


@functools.lru_cache(maxsize=None)
def pulse_one_gain(target, ceiling_dbtp=-1.0):
    """what one gain under the ceiling reaches on the pulse signal: (the f32 gain, the loudness of x g)"""
    x = pulse_signal()
    g = E.gain_tp(R.measure(x, 16000)["I"], target, E.true_peak(x, 16000), ceiling_dbtp)
    return g, R.measure(x * g, 16000)["I"]


# the bar of the loudness reached by three passes at H = 80, from this restatement's own reading on the pulse signal (0.017 LU at -23
# LUFS, less at -16): the reading doubled
REACHED_READING, REACHED_BAR = 0.017, 0.034
