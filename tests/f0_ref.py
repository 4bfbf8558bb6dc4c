"""The F0 rule of csrc/f0.hip (YIN, de Cheveigne & Kawahara 2002, steps 2-5) restated in numpy (no GPU, no library).

    frames   T = 1 + L // hop;  frame t reads x over [hop t - 512, hop t + 512), zeros outside [0, L);  s = hop t - 512
    lags     tau_min = ceil(sr / fmax), tau_max = floor(sr / fmin);  refused unless 2 <= tau_min < tau_max <= 256
    d[tau]   = sum_{j < 768} (x[s + j] - x[s + j + tau])^2,  tau = 0 .. 256                                   (float64 here)
    d'[tau]  = d[tau] tau / c[tau],  c[tau] = c[tau - 1] + d[tau],  d'[0] = 1,  d' = 1 where c is not > 0
    tau*     = the end of the downhill walk from the first tau in [tau_min, tau_max] with d' < thr, else the first arg-min there
    voiced   iff d'[tau*] < thr;  refined by a parabola through d'[tau* - 1 .. tau* + 1] when those lie in [1, tau_max]
    f0       = sr / (tau* + delta), 0 when unvoiced

`decide` runs the steps behind d in a chosen dtype: float64, or float32 with every operation rounded on its own - what the kernel
does, so that on the kernel's own d its results are the kernel's bits.  `moments` restates the pitch statistics."""
import math

import numpy as np

FRAME, WINDOW, MAX_LAG = 1024, 768, 256
SR, HOP = 16000, 256
FREQS = (70.0, 80.0, 110.0, 146.83, 220.5, 311.1, 440.0, 493.9)
HARMONICS = ((1.0,), (1.0, 0.5, 0.33, 0.25), (0.3, 1.0, 0.6, 0.4))          # the last: a weak fundamental


def frames(L, hop=HOP):
    return 1 + L // hop


def lags(sr=SR, fmin=62.5, fmax=500.0):
    """(tau_min, tau_max); ValueError where the rule refuses"""
    if not (math.isfinite(fmin) and math.isfinite(fmax) and fmin > 0 and fmax > 0):
        raise ValueError("fmin / fmax must be finite and > 0")
    lo, hi = math.ceil(sr / fmax), math.floor(sr / fmin)
    if not 2 <= lo < hi <= MAX_LAG:
        raise ValueError("lags outside 2 <= tau_min < tau_max <= 256")
    return lo, hi


def framed(x, hop=HOP):
    """[T, 1024] float64: the zero-padded frames"""
    x = np.asarray(x, np.float64)
    T = frames(x.size, hop)
    xp = np.zeros(FRAME // 2 + (T - 1) * hop + FRAME // 2, np.float64)
    xp[FRAME // 2:FRAME // 2 + x.size] = x
    return np.stack([xp[t * hop:t * hop + FRAME] for t in range(T)])


def difference(x, hop=HOP):
    """d [T, 257] float64"""
    fr = framed(x, hop)
    head = fr[:, :WINDOW]
    return np.stack([np.sum((head - fr[:, tau:tau + WINDOW]) ** 2, axis=1) for tau in range(MAX_LAG + 1)], axis=1)


def cmnd(d, dtype=np.float64):
    """d' [T, 257] in `dtype`: one add, one product and one division per value, each rounded on its own"""
    d = np.asarray(d).astype(dtype)
    out = np.ones_like(d)
    c = np.zeros(d.shape[0], dtype)
    with np.errstate(all="ignore"):
        for tau in range(1, MAX_LAG + 1):
            c = (c + d[:, tau]).astype(dtype)
            num = (d[:, tau] * dtype(tau)).astype(dtype)
            ok = c > 0
            out[ok, tau] = (num[ok] / c[ok]).astype(dtype)
    return out


def choose(dp, lo, hi, thr):
    """tau* of one frame's d'"""
    thr = dp.dtype.type(thr)
    below = np.nonzero(dp[lo:hi + 1] < thr)[0]
    if below.size:
        tau = lo + int(below[0])
        while tau + 1 <= hi and dp[tau + 1] < dp[tau]:
            tau += 1
        return tau
    seg = dp[lo:hi + 1]
    if np.isnan(seg).all():
        return lo
    return lo + int(np.nanargmin(seg))                 # the first index that attains the minimum


def decide(d, sr=SR, fmin=62.5, fmax=500.0, thr=0.15, dtype=np.float64):
    """(f0 [T], cmnd [T], lag [T] int32) in `dtype` from d [T, 257]"""
    lo, hi = lags(sr, fmin, fmax)
    if not 0 < thr <= 1:
        raise ValueError("threshold outside (0, 1]")
    dp = cmnd(d, dtype)
    T = dp.shape[0]
    f0, cm, lag = np.zeros(T, dtype), np.zeros(T, dtype), np.zeros(T, np.int32)
    two = dtype(2)
    with np.errstate(all="ignore"):
        for t in range(T):
            tau = choose(dp[t], lo, hi, thr)
            lag[t], cm[t] = tau, dp[t, tau]
            if not dp[t, tau] < dtype(thr):
                continue
            delta = dtype(0)
            if tau - 1 >= 1 and tau + 1 <= hi:
                a, b, c = dp[t, tau - 1], dp[t, tau], dp[t, tau + 1]
                den = dtype(dtype(a - dtype(two * b)) + c)
                if den > 0:
                    delta = dtype(dtype(a - c) / dtype(two * den))
            f0[t] = dtype(dtype(sr) / dtype(dtype(tau) + delta))
    return f0, cm, lag


def yin(x, sr=SR, hop=HOP, fmin=62.5, fmax=500.0, thr=0.15, dtype=np.float64):
    """the whole rule for one utterance -> (f0, cmnd, lag, d)"""
    d = difference(x, hop)
    return decide(d, sr, fmin, fmax, thr, dtype) + (d,)


def interior(L, hop=HOP):
    """the frames whose window lies wholly inside the utterance: 2 <= t and hop t + 512 <= L"""
    return [t for t in range(frames(L, hop)) if t >= 2 and hop * t - 512 >= 0 and hop * t + 512 <= L]


def cents(f, ref):
    return 1200.0 * np.log2(np.asarray(f, np.float64) / ref)


def moments(f0, T=None):
    """[6] float64: n, n / T, mean, sigma, skewness, excess kurtosis over the voiced frames (f0 > 0) among the first T"""
    f = np.asarray(f0, np.float64)[:T]
    T = f.size
    v = f[f > 0]
    n = v.size
    if n == 0:
        return np.zeros(6)
    mu = v.sum() / n
    e = v - mu
    m2, m3, m4 = (e ** 2).sum() / n, (e ** 3).sum() / n, (e ** 4).sum() / n
    if m2 == 0:
        return np.array([n, n / T, mu, 0.0, 0.0, 0.0])
    return np.array([n, n / T, mu, math.sqrt(m2), m3 / m2 ** 1.5, m4 / (m2 * m2) - 3.0])


# ---- test signals ------------------------------------------------------------------------------------------------------------

def tone(f, L, harmonics=(1.0,), seed=0, noise=1e-3, peak=0.5, sr=SR):
    """f32 [L]: sum_k h_k sin(2 pi k f n / sr + 0.3 k) scaled to `peak`, plus N(0, noise^2)"""
    n = np.arange(L, dtype=np.float64)
    x = sum(h * np.sin(2 * np.pi * (k + 1) * f * n / sr + 0.3 * (k + 1)) for k, h in enumerate(harmonics))
    x = peak * x / np.abs(x).max()
    x = (x + noise * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)
    x.setflags(write=False)
    return x


def white(L, rms, seed=0):
    x = (rms * np.random.default_rng(1000 + seed).standard_normal(L)).astype(np.float32)
    x.setflags(write=False)
    return x


def mixed():
    """63 frames at hop 256: 146.83 Hz (1, .5, .33) for 8000 samples, 0.01-rms noise for 4000, zeros for 1000, 311.1 Hz (1, .5) for 3000"""
    x = np.concatenate([tone(146.83, 8000, (1.0, 0.5, 0.33), seed=11), white(4000, 0.01, seed=12), np.zeros(1000, np.float32),
                        tone(311.1, 3000, (1.0, 0.5), seed=13)]).astype(np.float32)
    x.setflags(write=False)
    return x
