"""Float64 restatement of the integrated-loudness rule of csrc/loudness.hip (include/megatts2_hip.h, "THE RULE"): ITU-R BS.1770-4
K-weighting, 400 ms blocks every 100 ms, the absolute gate at -70 and the relative gate 10 LU under the gated mean.  The filter is a
plain serial loop over Python floats (doubles) - no chunks, no carry matrix; `sub_block_sums_chunked` restates the device's chunked
form beside it so that the two can be compared on the CPU."""
import math

import numpy as np

ABS_GATE = -70.0
SINE_CASES = ((997.0, 3.0), (100.0, 6.0), (4000.0, 3.0))       # (Hz, seconds) of the ground-truth sines


def sub_block(sr):
    assert sr % 10 == 0 and 8000 <= sr <= 192000
    return sr // 10


def coeffs(sr):
    """b0 b1 b2 a1 a2 of the shelf, then of the high-pass, from the analogue prototypes"""
    f0, G, Q = 1681.974450955533, 3.999843853973347, 0.7071752369554196
    K = math.tan(math.pi * f0 / sr)
    Vh = 10.0 ** (G / 20.0)
    Vb = Vh ** 0.4996667741545416
    a0 = 1.0 + K / Q + K * K
    shelf = [(Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0,
             2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0]
    f0, Q = 38.13547087602444, 0.5003270373238773
    K = math.tan(math.pi * f0 / sr)
    a0 = 1.0 + K / Q + K * K
    return np.array(shelf + [1.0, -2.0, 1.0, 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0])


def _cascade(c, v, state=None):
    """the cascade over the samples v (a list of floats) in transposed direct form II from `state` (zeros) -> (y, end state)"""
    b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = (float(t) for t in c)
    s1, s2, t1, t2 = (0.0, 0.0, 0.0, 0.0) if state is None else (float(t) for t in state)
    y = [0.0] * len(v)
    for i, x in enumerate(v):
        u = b0 * x + s1
        s1 = b1 * x - a1 * u + s2
        s2 = b2 * x - a2 * u
        w = d0 * u + t1
        t1 = d1 * u - e1 * w + t2
        t2 = d2 * u - e2 * w
        y[i] = w
    return np.array(y), np.array([s1, s2, t1, t2])


def kweight(x, sr):
    """y = highpass(shelf((double)x)) from zero state"""
    return _cascade(coeffs(sr), np.asarray(x, np.float64).tolist())[0]


def sub_block_sums(x, sr):
    h = sub_block(sr)
    ns = len(x) // h
    y = kweight(np.asarray(x)[:ns * h], sr)
    return (y * y).reshape(ns, h).sum(axis=1) if ns else np.zeros(0)


def carry_matrix(sr, c):
    """M = A^c: column k is the state reached in c steps of zero input from the unit state e_k"""
    cf = coeffs(sr)
    return np.stack([_cascade(cf, [0.0] * c, np.eye(4)[k])[1] for k in range(4)], axis=1)


def sub_block_sums_chunked(x, sr, c):
    """the device's form with chunks of c samples (c divides h): every chunk from zero state, the states carried by M, every chunk
    again from its entry state"""
    h = sub_block(sr)
    assert h % c == 0
    ns = len(x) // h
    cf, v = coeffs(sr), np.asarray(x, np.float64)[:ns * h].tolist()
    n = ns * h // c
    zero = [_cascade(cf, v[j * c:(j + 1) * c])[1] for j in range(n)]
    M, e, S = carry_matrix(sr, c), np.zeros(4), np.zeros(ns)
    for j in range(n):
        y = _cascade(cf, v[j * c:(j + 1) * c], e)[0]
        S[j * c // h] += float((y * y).sum())
        e = M @ e + zero[j]
    return S


def _lk(z):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def measure(x, sr):
    """-> dict: I, nb, n_abs, n_rel, gamma, peak, lmax, l [nb] (momentary), z [nb], ungated (the mean over every block)"""
    x = np.asarray(x)
    h = sub_block(sr)
    S = sub_block_sums(x, sr)
    nb = max(0, S.size - 3)
    z = np.array([((S[k] + S[k + 1]) + S[k + 2]) + S[k + 3] for k in range(nb)]) / (4.0 * h) if nb else np.zeros(0)
    l = _lk(z)
    over_abs = ~(l <= ABS_GATE)                      # a NaN block counts
    n_abs = int(over_abs.sum())
    gamma = float(_lk(z[over_abs].mean()) - 10.0) if n_abs else -np.inf
    over = over_abs & ~(l <= gamma)
    n_rel = int(over.sum())
    finite = x[~np.isnan(x)]
    return dict(I=float(_lk(z[over].mean())) if n_rel else -np.inf, nb=nb, n_abs=n_abs, n_rel=n_rel, gamma=gamma,
                peak=float(np.abs(finite).max()) if finite.size else 0.0, lmax=float(np.fmax.reduce(l)) if nb else -np.inf, l=l, z=z,
                ungated=float(_lk(z.mean())) if nb else -np.inf)


def gate_margin(m):
    """the smallest distance in LU of any block from either gate (blocks under the absolute gate are not held against the relative
    one); inf without blocks"""
    l = m["l"]
    if not l.size:
        return np.inf
    d = np.abs(l - ABS_GATE).min()
    live = l[l > ABS_GATE]
    if live.size and np.isfinite(m["gamma"]):
        d = min(d, np.abs(live - m["gamma"]).min())
    return float(d)


def gain(I, target, peak=0.0, ceiling=0.0):
    """the f32 gain of the normalising call"""
    if not np.isfinite(I):
        return np.float32(1.0)
    g = 10.0 ** ((target - I) / 20.0)
    capped = ceiling > 0 and peak > 0 and ceiling / peak < g
    g = np.float32(ceiling / peak if capped else g)
    if ceiling > 0 and np.isfinite(g):     # the f32 product with the peak stays at or under the ceiling; capped: the largest such f32
        pk = np.float32(peak)
        for _ in range(4):
            if g > 0 and float(pk * g) > ceiling:
                g = np.nextafter(g, np.float32(0))
        for _ in range(4 if capped else 0):
            up = np.nextafter(g, np.float32(np.inf))
            if not (np.isfinite(up) and float(pk * up) <= ceiling):
                break
            g = up
    return g if np.isfinite(g) else np.float32(1.0)


def response(f, sr):
    """|H(e^{j w})|^2 of the cascade at f Hz, from the coefficients"""
    c, w = coeffs(sr), 2.0 * math.pi * f / sr
    z1, z2 = np.exp(-1j * w), np.exp(-2j * w)
    H = (c[0] + c[1] * z1 + c[2] * z2) / (1 + c[3] * z1 + c[4] * z2) * (c[5] + c[6] * z1 + c[7] * z2) / (1 + c[8] * z1 + c[9] * z2)
    return float(abs(H) ** 2)


def sine_reading(f, sr, amp=1.0):
    """the steady-state reading of a sine: -0.691 + 10 log10(amp^2 |H|^2 / 2)"""
    return -0.691 + 10.0 * math.log10(amp * amp * response(f, sr) / 2.0)


def sine(f, sr, seconds, amp=1.0, level=None):
    """a f32 sine of `seconds`; level: the amplitude is chosen so that its steady-state reading is `level` LUFS"""
    if level is not None:
        amp = 10.0 ** ((level - sine_reading(f, sr)) / 20.0)
    n = int(round(seconds * sr))
    return (amp * np.sin(2.0 * np.pi * f * np.arange(n) / sr)).astype(np.float32)


def gating_case(sr=16000, pad=False):
    """997 Hz at -36, -23, -36 LUFS for 2 s, 6 s, 2 s (97 blocks; with pad 2 s at -72 in front and behind: 137)"""
    parts = [sine(997.0, sr, 2.0, level=-36.0), sine(997.0, sr, 6.0, level=-23.0), sine(997.0, sr, 2.0, level=-36.0)]
    if pad:
        parts = [sine(997.0, sr, 2.0, level=-72.0)] + parts + [sine(997.0, sr, 2.0, level=-72.0)]
    return np.concatenate(parts)
