"""The three rules of csrc/prosody.hip restated in numpy (no GPU, no library).

    energy    T = 1 + L // hop;  frame t reads x over [hop t - 512, hop t + 512), zeros outside [0, L);  the mean square of the 1024
              samples.  `energy32` spells out the kernel's order in float32 - lane l one fma chain over the in-frame offsets
              256 i + 4 l + r (i outer, r inner), the 64 partial sums through the xor butterfly 32 .. 1, one product by 2^-10 - and
              gives the kernel's bits;  `energy64` is the plain float64 mean.
    phones    start[p] = sum_{q < p} max(dur[q], 0);  phone p owns [min(start, T), min(start + max(dur[p], 0), T));  eight float64
              fields per phone (`phone_prosody`), and the unclipped sum.
    contour   the voiced frames (f0 > 0) among the first T in order, s = 12 log2 f0, minus their mean with center, rounded once to
              float32 (`contour`; `contour64` is the value before that rounding).

`dtw_rms` is the pitch distance the contours are made for: plain DTW with squared cost in float64, sqrt(total / steps)."""
import math

import numpy as np

import f0_ref as F

FRAME = F.FRAME
FIELDS = ("start", "frames", "voiced_frames", "mean_hz", "mean_semitones", "min_hz", "max_hz", "mean_energy")
EPS_E = (FRAME + 7) * 2.0 ** -24          # the f32 chain bound of the energy: 16 fma + 6 adds deep, 1024 non-negative terms


def frames(L, hop=F.HOP):
    return 1 + L // hop


def framed(x, hop=F.HOP, dtype=np.float64):
    """[T, 1024]: the zero-padded frames"""
    x = np.asarray(x, dtype)
    T = frames(x.size, hop)
    xp = np.zeros(FRAME // 2 + (T - 1) * hop + FRAME // 2, dtype)
    xp[FRAME // 2:FRAME // 2 + x.size] = x
    return np.stack([xp[t * hop:t * hop + FRAME] for t in range(T)])


def energy64(x, hop=F.HOP):
    fr = framed(x, hop)
    return (fr * fr).sum(axis=1) / FRAME


def fma32(x, acc):
    """float32 fma(x, x, acc), correctly rounded, elementwise: the exact 48-bit square plus acc in float64, the float64 rounding
    turned into a rounding to odd by the exact error of the sum (Knuth's two-sum), then one rounding to float32 - 53 >= 24 + 2 bits,
    so the double rounding is harmless"""
    p = x.astype(np.float64) * x.astype(np.float64)
    a = acc.astype(np.float64)
    with np.errstate(all="ignore"):
        s = p + a
        bb = s - p
        err = (p - (s - bb)) + (a - bb)
        fix = np.isfinite(s) & (err != 0) & ((s.view(np.int64) & 1) == 0)
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
        return s.astype(np.float32)


def energy32(x, hop=F.HOP):
    """float32 [T]: the kernel's order, operation by operation"""
    fr = framed(np.asarray(x, np.float32), hop, np.float32)                  # [T, 1024]
    lanes = fr.reshape(-1, 4, 64, 4)                                        # [t, i, l, r]: offset 256 i + 4 l + r
    acc = np.zeros((fr.shape[0], 64), np.float32)
    for i in range(4):
        for r in range(4):
            acc = fma32(lanes[:, i, :, r], acc)
    lane = np.arange(64)
    with np.errstate(all="ignore"):
        for d in (32, 16, 8, 4, 2, 1):
            acc = (acc + acc[:, lane ^ d]).astype(np.float32)
        return (acc[:, 0] * np.float32(2.0 ** -10)).astype(np.float32)


def phone_prosody(f0, dur, energy=None, T=None):
    """(out [Np, 8] float64, dur_sum int) for one utterance: f0 [>= T], dur [Np] ints, energy [>= T] or None"""
    f0 = np.asarray(f0, np.float32)
    T = f0.size if T is None else T
    out = np.zeros((len(dur), 8))
    start = 0
    for p, d in enumerate(dur):
        d = max(int(d), 0)
        t0, t1 = min(start, T), min(start + d, T)
        start += d
        f = f0[t0:t1].astype(np.float64)
        with np.errstate(all="ignore"):
            v = f[f > 0]
        out[p, 0], out[p, 1], out[p, 2] = t0, t1 - t0, v.size
        if v.size:
            with np.errstate(all="ignore"):
                st = 12.0 * np.log2(v / 55.0)
            out[p, 3], out[p, 4], out[p, 5], out[p, 6] = math.fsum(v) / v.size, math.fsum(st) / v.size, v.min(), v.max()
        if energy is not None and t1 > t0:
            out[p, 7] = math.fsum(np.asarray(energy, np.float32)[t0:t1].astype(np.float64)) / (t1 - t0)
    return out, start


def contour64(f0, T=None, center=True):
    """(s [n] float64, index [n]) of one utterance"""
    f0 = np.asarray(f0, np.float32)[:T]
    with np.errstate(all="ignore"):
        index = np.nonzero(f0 > 0)[0]
        s = 12.0 * np.log2(f0[index].astype(np.float64))
    if center and index.size:
        s = s - math.fsum(s) / index.size
    return s, index.astype(np.int32)


def contour(f0, T=None, center=True):
    s, index = contour64(f0, T, center)
    return s.astype(np.float32), index


def dtw_rms(a, b):
    """(sqrt(total / steps), steps) of the DTW of contour a onto b with squared cost, by the direction rule of csrc/dtw.hip
    (diagonal, then up, then left on ties), in float64"""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    c = (a[:, None] - b[None, :]) ** 2
    A = np.zeros_like(c)
    n, m = c.shape
    A[:, 0] = np.cumsum(c[:, 0])
    A[0, :] = np.cumsum(c[0, :])
    for i in range(1, n):
        for j in range(1, m):
            A[i, j] = c[i, j] + min(A[i - 1, j - 1], A[i - 1, j], A[i, j - 1])
    i, j, steps = n - 1, m - 1, 1
    while i > 0 or j > 0:
        if i == 0:
            j -= 1
        elif j == 0:
            i -= 1
        elif A[i - 1, j - 1] <= A[i - 1, j] and A[i - 1, j - 1] <= A[i, j - 1]:
            i, j = i - 1, j - 1
        elif A[i - 1, j] <= A[i, j - 1]:
            i -= 1
        else:
            j -= 1
        steps += 1
    return math.sqrt(A[-1, -1] / steps), steps


def duration_moments(dur):
    """[6] float64 over the realised phones (dur > 0): n, n / Np, mean, sigma, skewness, excess kurtosis - plain numpy formulas"""
    d = np.asarray(dur, np.float64)
    v = d[d > 0]
    if v.size == 0:
        return np.zeros(6)
    mu, sd = v.mean(), v.std()
    if sd == 0:
        return np.array([v.size, v.size / d.size, mu, 0.0, 0.0, 0.0])
    z = (v - mu) / sd
    return np.array([v.size, v.size / d.size, mu, sd, np.mean(z ** 3), np.mean(z ** 4) - 3.0])


# ---- test signals ------------------------------------------------------------------------------------------------------------

SEG = 24                                    # hops per segment of the ground-truth signal
TRUTH = (110.0, 220.0, 0.0, 329.63)         # tone A, tone B, silence, tone C
BORDER = 4                                  # frames of the phone that sits on every segment border


def truth_signal(hop=F.HOP):
    """f32 [4 * 24 * hop]: three harmonic tones (the sets of test_f0_host.py) and a silence, each 24 hops long"""
    parts = []
    for k, f in enumerate(TRUTH):
        parts.append(np.zeros(SEG * hop, np.float32) if f == 0 else F.tone(f, SEG * hop, F.HARMONICS[1], seed=40 + k))
    x = np.concatenate(parts).astype(np.float32)
    x.setflags(write=False)
    return x


def truth_alignment(T, border=BORDER):
    """durations summing to T: every segment border k * 24 sits in the middle of its own `border`-frame phone, the first and last
    `border` / 2 frames of the utterance are edge phones, the interiors lie between -> (dur, the interior phones' indices)"""
    h = border // 2
    dur, inner = [h], []
    for k in range(len(TRUTH)):
        last = k == len(TRUTH) - 1
        inner.append(len(dur))
        dur.append(SEG - border)
        dur.append(border if not last else T - (SEG * len(TRUTH) - h))
    assert sum(dur) == T
    return np.asarray(dur, np.int32), inner


def warped_pair(n=60, seed=3):
    """(a, b) f32 F0 tracks: a steps at random between the four levels 100, 150, 225 and 337.5 Hz (7.02 semitones apart) with two
    unvoiced gaps; b is a with every voiced frame repeated twice, multiplied by 2^(3/12), with other unvoiced gaps inserted.
    Levels, not a smooth curve: under a transposition of 3 semitones a cell off the true warp then costs (7.02 k - 3)^2 >= 9 for
    every k, so no warp is cheaper than the true one and the uncentred distance IS the transposition (on a smooth contour DTW
    trades part of a transposition for a shift in time)."""
    rng = np.random.default_rng(seed)
    a = (100.0 * 1.5 ** rng.integers(0, 4, n)).astype(np.float32)
    a[10:14] = 0
    a[40:43] = 0
    va = a[a > 0]
    vb = (np.repeat(va, 2).astype(np.float32) * np.float32(2.0 ** (3.0 / 12.0))).astype(np.float32)
    b = np.concatenate([np.zeros(3, np.float32), vb[:31], np.zeros(5, np.float32), vb[31:80], np.zeros(2, np.float32), vb[80:],
                        np.zeros(4, np.float32)])
    return a, b
