"""float64 restatement of the formant rule (include/megatts2_hip.h, csrc/formants.hip) in numpy, and the signals its tests use.

The rule, for one utterance x f32 [L] at sample_rate, a hop, an even window W in [64, 1024], an even order P in [2, 32]:
  1 T = 1 + L // hop;  frame t covers i = hop t - W/2 + j, j = 0 .. W-1;  a sample outside [0, L) is a zero
  2 y[i] = x[i] - alpha * x[i-1] in double (product and difference rounded), x[-1] = 0, alpha = exp(-2 pi pre_hz / sr); pre_hz 0: off
  3 v[j] = y[i] * w[j];  hann: w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5) / W);  rect: 1
  4 r[k] = sum_j v[j] v[j+k], k = 0 .. P: 64 lane chains over j = l, l + 64, ... (j + k < W), then the xor butterfly 32 .. 1;
    r[0] *= 1 + 1e-9;  empty unless r[0] > 1e-300 and finite
  5 Levinson-Durbin, every operation rounded on its own, in the header's order;  empty on |k| >= 1, e <= 0, a non-finite value
  6 roots by Aberth-Ehrlich from 0.9 exp(i (2 pi k / P + 0.4)), all roots updated together, until max |w|^2 < 1e-26; 64 at most
  7 f = arg z sr / 2 pi, bw = -ln|z| sr / pi of the roots with Im z > 0;  kept: fmin < f < sr/2 - fmin and bw < max_bw;  sorted by
    (f, root index);  the first 5
numpy has no fma: the device's chains in step 4 are fma chains, this file's round the product first.  Both are W-term double sums, and
the tests compare r within the bound of such a sum in ANY order, then run step 5 of this file on the device's own r, where the order
is pinned line by line and the result must be equal to the bit.  Steps 6 and 7 are not pinned to the bit either (complex division,
atan2, log)."""
import numpy as np

MAX = 5
MAX_ITERS = 64
STAT_FIELDS = 12
STAT_NAMES = ("frames", "share", "f1", "f2", "f3", "f4", "f1_sigma", "f2_sigma", "f3_sigma", "f4_sigma", "dispersion", "vtl_cm")
HANN, RECT = 0, 1


def window_table(W, kind):
    if kind == RECT:
        return np.ones(W, np.float64)
    j = np.arange(W, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * (j + 0.5) / np.float64(W))


def alpha_of(pre_hz, sr):
    return float(np.exp(-2.0 * np.pi * np.float64(pre_hz) / np.float64(sr))) if pre_hz > 0 else 0.0


def frame_count(L, hop):
    return 1 + L // hop


def frames(x, hop, W, alpha, w):
    """v float64 [T, W] of x f32 [L] (steps 1-3), and the first sample s[t] of every frame"""
    x = np.asarray(x, np.float32).astype(np.float64)
    L = x.size
    T = frame_count(L, hop)
    s = hop * np.arange(T, dtype=np.int64) - W // 2
    i = s[:, None] + np.arange(W, dtype=np.int64)[None, :]
    inside = (i >= 0) & (i < L)
    with np.errstate(all="ignore"):
        xi = x[np.clip(i, 0, L - 1)]
        if alpha != 0.0:
            xp = np.where(i >= 1, x[np.clip(i - 1, 0, L - 1)], 0.0)
            y = xi - np.float64(alpha) * xp
        else:
            y = xi
        v = np.where(inside, y * w[None, :], 0.0)
    return v, s


def autocorr(v, P):
    """r float64 [T, P+1] in the lane order of step 4 (products rounded before they are added), and the sums of |terms| [T, P+1]"""
    T, W = v.shape
    r = np.zeros((T, P + 1), np.float64)
    mag = np.zeros((T, P + 1), np.float64)
    lanes = np.arange(64)
    with np.errstate(all="ignore"):
        for k in range(P + 1):
            n = W - k
            prod = v[:, :n] * v[:, k:]
            rows = -(-n // 64)
            pad = np.zeros((T, rows * 64), np.float64)
            pad[:, :n] = prod
            pad = pad.reshape(T, rows, 64)
            acc = np.zeros((T, 64), np.float64)
            for q in range(rows):
                acc = acc + pad[:, q, :]
            for o in (32, 16, 8, 4, 2, 1):
                acc = acc + acc[:, lanes ^ o]
            r[:, k] = acc[:, 0]
            mag[:, k] = np.abs(prod).sum(axis=1)
        r[:, 0] = r[:, 0] * np.float64(1.0 + 1e-9)
    return r, mag


def levinson(r):
    """step 5 on r float64 [T, P+1] -> (a [T, P+1], e [T], ok [T]); a and e are zeros where ok is False.  Every line is one rounded
    operation per frame, in the header's order, so the bits are the device's."""
    r = np.asarray(r, np.float64)
    T, P1 = r.shape
    P = P1 - 1
    with np.errstate(all="ignore"):
        ok = (r[:, 0] > 1e-300) & np.isfinite(r[:, 0])
        e = r[:, 0].copy()
        a = np.zeros((T, P1), np.float64)
        a[:, 0] = 1.0
        for m in range(1, P + 1):
            acc = r[:, m].copy()
            for i in range(1, m):
                acc = acc + (a[:, i] * r[:, m - i])
            k = (-acc) / e
            ok &= np.abs(k) < 1.0
            new = a.copy()
            for i in range(1, m):
                new[:, i] = a[:, i] + (k * a[:, m - i])
            new[:, m] = k
            a = new
            e = e * (1.0 - (k * k))
            ok &= (e > 0.0) & np.isfinite(e)
        ok &= np.isfinite(a).all(axis=1)
    a[~ok] = 0.0
    e = np.where(ok, e, 0.0)
    return a, e, ok


def aberth(a):
    """step 6 on one frame's a float64 [P+1] -> (roots complex128 [P], iters); iters = -1 (and zeros) where it does not get there"""
    a = np.asarray(a, np.float64)
    P = a.size - 1
    k = np.arange(P, dtype=np.float64)
    z = 0.9 * np.exp(1j * (2.0 * np.pi * k / np.float64(P) + 0.4))
    off = ~np.eye(P, dtype=bool)
    with np.errstate(all="ignore"):
        for it in range(1, MAX_ITERS + 1):
            p = np.ones(P, np.complex128)
            d = np.zeros(P, np.complex128)
            for i in range(1, P + 1):
                d = d * z + p
                p = p * z + a[i]
            q = p / d
            diff = z[:, None] - z[None, :]
            inv = np.where(off, 1.0 / np.where(off, diff, 1.0), 0.0)
            S = np.zeros(P, np.complex128)
            for j in range(P):
                S = S + inv[:, j]
            w = q / (1.0 - q * S)
            z = z - w
            if not (np.isfinite(w.real).all() and np.isfinite(w.imag).all()):
                break
            if np.max(w.real * w.real + w.imag * w.imag) < 1e-26:
                return z, it
    return np.zeros(P, np.complex128), -1


def candidates(z, sr, fmin, max_bw, margin=1e-6):
    """step 7 on one frame's roots -> (freq float64 [5], bw float64 [5], count, near): near = a candidate lies within `margin`
    (relative) of one of the three keep / drop thresholds, or a root within it of the real axis, so that the device may decide otherwise"""
    sr = np.float64(sr)
    up = z.imag > 0.0
    with np.errstate(all="ignore"):
        f = np.arctan2(z.imag, z.real) * sr / (2.0 * np.pi)
        bw = -0.5 * np.log(z.real * z.real + z.imag * z.imag) * sr / np.pi
    keep = up & (f > fmin) & (f < 0.5 * sr - fmin) & (bw < max_bw)

    def close(v, thr):
        return np.abs(v - thr) <= margin * max(abs(thr), 1.0)
    near = bool(np.any(np.abs(z.imag) <= margin) or np.any((np.abs(z.imag) > margin) & up & (close(f, fmin) | close(f, 0.5 * sr - fmin) | close(bw, max_bw))))
    idx = np.flatnonzero(keep)
    idx = idx[np.lexsort((idx, f[idx]))]
    if idx.size > 1 and np.any(np.diff(f[idx]) <= margin * np.abs(f[idx][1:])):
        near = True                                   # two candidates that the device may order the other way
    count = min(idx.size, MAX)
    fo, bo = np.zeros(MAX), np.zeros(MAX)
    fo[:count] = f[idx[:count]]
    bo[:count] = bw[idx[:count]]
    return fo, bo, count, near


def analyse(x, sr, hop, W, P, pre_hz=50.0, fmin=50.0, max_bw=500.0, kind=HANN):
    """the whole rule on one utterance -> dict of float64 / int arrays: v, start, autocorr, mag, lpc, err, roots [T, P] complex, iters,
    freq [T, 5], bw [T, 5], count, near [T] bool"""
    w = window_table(W, kind)
    v, s = frames(x, hop, W, alpha_of(pre_hz, sr), w)
    r, mag = autocorr(v, P)
    out = {"v": v, "start": s, "autocorr": r, "mag": mag}
    out.update(finish(r, sr, fmin, max_bw))
    return out


def finish(r, sr, fmin=50.0, max_bw=500.0):
    """steps 5-7 on r float64 [T, P+1] (the device's own, say)"""
    T, P = r.shape[0], r.shape[1] - 1
    a, e, ok = levinson(r)
    roots = np.zeros((T, P), np.complex128)
    iters = np.full(T, -1, np.int32)
    freq, bw = np.zeros((T, MAX)), np.zeros((T, MAX))
    count = np.zeros(T, np.int32)
    near = np.zeros(T, bool)
    for t in np.flatnonzero(ok):
        roots[t], iters[t] = aberth(a[t])
        if iters[t] > 0:
            freq[t], bw[t], count[t], near[t] = candidates(roots[t], sr, fmin, max_bw)
    return {"lpc": a, "err": e, "ok": ok, "roots": roots, "iters": iters, "freq": freq, "bw": bw, "count": count, "near": near}


def stats(freq, count, f0=None, T=None):
    """one utterance's figures float64 [12] of freq [T_max, 5], count [T_max] over the first T frames (math.fsum-free: plain float64 sums;
    the tests allow the device T * 2^-52 relative for its own order)"""
    freq = np.asarray(freq, np.float32).astype(np.float64)
    T = freq.shape[0] if T is None else int(T)
    use = np.asarray(count[:T]) >= 4
    if f0 is not None:
        use &= np.asarray(f0[:T], np.float32) > 0
    n = int(use.sum())
    out = np.zeros(STAT_FIELDS, np.float64)
    if n == 0:
        return out
    F = freq[:T][use][:, :4]
    mu = F.sum(axis=0) / n
    sig = np.sqrt(((F - mu[None, :]) ** 2).sum(axis=0) / n)
    out[0], out[1] = n, n / T
    out[2:6], out[6:10] = mu, sig
    out[10] = (mu[3] - mu[0]) / 3.0
    out[11] = 2187.5 * (((1.0 / mu[0] + 3.0 / mu[1]) + 5.0 / mu[2]) + 7.0 / mu[3])
    return out


# ---- signals -----------------------------------------------------------------------------------------------------------------------
def resonate(x, sr, poles):
    """x through cascaded two-pole resonators, poles = ((F, bandwidth) in Hz, ...): radius exp(-pi bw / sr), angle 2 pi F / sr; float64"""
    y = np.asarray(x, np.float64).copy()
    for F, bw in poles:
        rho, th = np.exp(-np.pi * bw / sr), 2.0 * np.pi * F / sr
        c1, c2 = 2.0 * rho * np.cos(th), -rho * rho
        out = np.zeros_like(y)
        y1 = y2 = 0.0
        for n in range(y.size):
            o = y[n] + c1 * y1 + c2 * y2
            out[n] = o
            y2, y1 = y1, o
        y = out
    return y


RECOVERY_SETS = (
    (11000, ((700, 150), (1220, 200), (2600, 250), (3500, 300)), 500.0),
    (16000, ((500, 200), (1500, 220), (2500, 260), (3500, 300), (4500, 320), (6000, 350)), 1000.0),
    (11000, ((300, 160), (2300, 180), (3000, 200)), 500.0),
)
RECOVERY_HOP, RECOVERY_W, RECOVERY_FRAME = 512, 1024, 1      # frame 1 covers [0, 1024): the impulse sits 8 samples into it


def recovery_signal(sr, poles):
    """the impulse response of the cascade, the impulse at sample 8: 1024 samples, scaled to a peak of 0.5"""
    x = np.zeros(RECOVERY_W, np.float64)
    x[8] = 1.0
    y = resonate(x, sr, poles)
    return y * (0.5 / np.abs(y).max())


VOICED_SR, VOICED_PERIOD = 11000, 100
VOICED_POLES = ((700, 80), (1220, 90), (2600, 120), (3500, 150))
VOICED = dict(hop=176, W=550, P=10, pre_hz=50.0, fmin=50.0, max_bw=500.0, kind=HANN)


def voiced_signal(n=11000, period=VOICED_PERIOD, sr=VOICED_SR, poles=VOICED_POLES):
    """pulses every `period` samples (110 Hz at 11 kHz) through the resonators, scaled to a peak of 0.5 -> f32"""
    x = np.zeros(n, np.float64)
    x[::period] = 1.0
    y = resonate(x, sr, poles)
    return (y * (0.5 / np.abs(y).max())).astype(np.float32)


def interior(start, W, L, settle=1100):
    """the frames whose window lies inside the signal and behind the resonators' onset"""
    return (start >= settle) & (start + W <= L)


def noise_signal(n, seed, scale=0.3):
    return (np.random.default_rng(seed).standard_normal(n) * scale).astype(np.float32)
