"""Float64 restatement of the EBU-mode rules of csrc/ebu.hip (include/megatts2_hip.h, "EBU-mode metering"): true peak by an
oversampling Kaiser-windowed sinc, short-term loudness (3 s blocks every 100 ms) and loudness range (EBU Tech 3342) over the
sub-block sums of tests/loudness_ref.py, which is imported unchanged, and the gain of the normalising call under a true-peak
ceiling.  The interpolation runs in double over the f32 table; the sort is numpy's."""
import functools
import math

import numpy as np

import loudness_ref as R

Z, TAPS, BETA = 12, 24, 8.0
ABS_GATE, REL_GATE = -70.0, -20.0
RATES = (8000, 16000, 22050, 44100, 48000)
# (fs / f, phase in degrees) of the ground-truth tones: the crest of each falls between the samples
TONES = ((4, 0.0), (4, 45.0), (6, 60.0), (8, 67.5))


def oversample(sr):
    return -(-192000 // sr)


def bessel_i0(x):
    """I0 by its power series"""
    term, total, q = 1.0, 1.0, 0.25 * x * x
    for k in range(1, 64):
        term *= q / (float(k) * float(k))
        total += term
        if term < 1e-18 * total:
            break
    return total


@functools.lru_cache(maxsize=None)
def table64(sr):
    """h[p][k] in double, [o, 24]; row 0 is the unit sample"""
    o = oversample(sr)
    i0b = bessel_i0(BETA)
    h = np.zeros((o, TAPS))
    for p in range(o):
        for k in range(TAPS):
            t = float(k - Z + 1) - float(p) / float(o)
            u = t / float(Z)
            w = bessel_i0(BETA * math.sqrt(1.0 - u * u)) / i0b if u * u < 1.0 else 0.0
            s = 1.0 if t == 0.0 else math.sin(math.pi * t) / (math.pi * t)
            h[p, k] = s * w if p else float(k == Z - 1)
    h.flags.writeable = False
    return h


def table(sr):
    """the table as the library holds it: rounded once to f32"""
    return table64(sr).astype(np.float32)


def interpolate(x, sr):
    """y [L + Z, o] in double over the f32 table: row r is position i = r - Z, column p the phase; column 0 is the sample itself"""
    x = np.asarray(x, np.float64)
    h = table(sr).astype(np.float64)
    xp = np.concatenate([np.zeros(2 * Z - 1), x, np.zeros(Z)])
    win = np.lib.stride_tricks.sliding_window_view(xp, TAPS)[:x.size + Z]
    with np.errstate(invalid="ignore", over="ignore"):
        y = win @ h.T
    y[:, 0] = np.concatenate([np.zeros(Z), x])                  # phase 0 is never filtered
    return y


def true_peak(x, sr):
    """max |y| taken with v > m from m = 0: a NaN never wins, an Inf does"""
    y = np.abs(interpolate(x, sr))
    return float(np.fmax.reduce(np.fmax.reduce(y, axis=0), initial=0.0)) if y.size else 0.0


def sample_peak(x):
    return float(np.fmax.reduce(np.abs(np.asarray(x, np.float64)), initial=0.0))


def chain_bound(sr, xmax):
    """what one f32 fma chain of 24 terms can lose against the exact sum: 24 2^-24 max_p sum_k |h[p][k]| max |x|"""
    return 24.0 * 2.0 ** -24 * float(np.abs(table(sr).astype(np.float64)).sum(axis=1).max()) * float(xmax)


def db(v):
    return 20.0 * math.log10(v) if v > 0 else -math.inf


def tone(sr, div, phase_deg, amp, n=6000):
    """amp sin(2 pi i / div + phase), n samples, under a 10 ms raised-cosine fade in and out (an abrupt onset overshoots by itself)"""
    i = np.arange(n)
    x = amp * np.sin(2.0 * np.pi * i / div + np.deg2rad(phase_deg))
    f = sr // 100
    ramp = 0.5 - 0.5 * np.cos(np.pi * (np.arange(f) + 0.5) / f)
    x[:f] *= ramp
    x[n - f:] *= ramp[::-1]
    return x.astype(np.float32)


def _lk(z):
    with np.errstate(divide="ignore", invalid="ignore"):
        return -0.691 + 10.0 * np.log10(z)


def fixed_mean(z, mask):
    """the mean of z[mask] in the device's order: partial sums over k = i, i + 256, ... ascending for i < 256, then a halving tree"""
    part = np.zeros(256)
    for i in range(min(256, z.size)):
        acc = 0.0
        for k in range(i, z.size, 256):
            if mask[k]:
                acc += float(z[k])
        part[i] = acc
    s = 128
    while s > 0:
        part[:s] = part[:s] + part[s:2 * s]
        s //= 2
    return part[0] / float(int(mask.sum()))


def percentile_index(n, p):
    return ((n - 1) * p + 50) // 100


def short_term_of_sums(S, h, rel_gate=REL_GATE):
    """-> dict: nst, z3, s [nst], n_abs, n_rel, gamma, p10, p95, lra, smax from the sub-block sums S"""
    S = np.asarray(S, np.float64)
    nst = max(0, S.size - 29)
    z3 = np.zeros(nst)
    for k in range(nst):
        acc = float(S[k])
        for q in range(1, 30):
            acc += float(S[k + q])
        z3[k] = acc / (30.0 * h)
    s = _lk(z3)
    over_abs = ~(s <= ABS_GATE)                      # a NaN block counts
    n_abs = int(over_abs.sum())
    gamma = float(_lk(fixed_mean(z3, over_abs)) + rel_gate) if n_abs else -np.inf
    over = over_abs & ~(s <= gamma)
    n = int(over.sum())
    g = np.sort(s[over])                             # a NaN sorts last
    p10 = float(g[percentile_index(n, 10)]) if n else np.nan
    p95 = float(g[percentile_index(n, 95)]) if n else np.nan
    return dict(nst=nst, z3=z3, s=s, n_abs=n_abs, n_rel=n, gamma=gamma, p10=p10, p95=p95, lra=p95 - p10,
                smax=float(np.fmax.reduce(s)) if nst else -np.inf)


def short_term(x, sr, rel_gate=REL_GATE):
    return short_term_of_sums(R.sub_block_sums(np.asarray(x), sr), R.sub_block(sr), rel_gate)


def gate_margin(m):
    """the smallest distance in LU of any short-term block from either gate (blocks under the absolute gate are not held against the
    relative one); inf without blocks"""
    s = m["s"][np.isfinite(m["s"])]
    if not s.size:
        return np.inf
    d = np.abs(s - ABS_GATE).min()
    live = s[s > ABS_GATE]
    if live.size and np.isfinite(m["gamma"]):
        d = min(d, np.abs(live - m["gamma"]).min())
    return float(d)


def gain_tp(I, target, tp, ceiling_dbtp):
    """the f32 gain of the normalising call under a true-peak ceiling: toward zero where the cap binds, to nearest otherwise"""
    if not np.isfinite(I):
        return np.float32(1.0)
    with np.errstate(over="ignore"):
        g = 10.0 ** ((target - I) / 20.0)
        if tp > 0 and 10.0 ** (ceiling_dbtp / 20.0) / tp < g:
            cap = 10.0 ** (ceiling_dbtp / 20.0) / tp
            g = np.float32(cap)
            if float(g) > cap:
                g = np.nextafter(g, np.float32(0))
        else:
            g = np.float32(g)
    return g if np.isfinite(g) else np.float32(1.0)


def levels(spec, sr=16000, f=1000.0):
    """a sine of f Hz through the (LUFS, seconds) segments of spec"""
    return np.concatenate([R.sine(f, sr, sec, level=lv) for lv, sec in spec])


# EBU Tech 3342's synthetic cases 1-4 (LRA and its own tolerance of 1 LU) and the two gating cases
TECH_3342 = (
    (((-20.0, 20.0), (-30.0, 20.0)), 10.0),
    (((-20.0, 20.0), (-15.0, 20.0)), 5.0),
    (((-40.0, 20.0), (-20.0, 20.0)), 20.0),
    (((-50.0, 20.0), (-35.0, 20.0), (-20.0, 20.0), (-35.0, 20.0), (-50.0, 20.0)), 15.0),
)
REL_GATE_CASE = ((-20.0, 10.0), (-42.0, 10.0))
ABS_GATE_CASE = REL_GATE_CASE + ((-75.0, 5.0),)


@functools.lru_cache(maxsize=None)
def case(spec, rel_gate=REL_GATE):
    return short_term(levels(spec), 16000, rel_gate)
