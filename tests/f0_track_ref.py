"""The rule of the second F0 tracker (csrc/f0.hip: mt2_f0_track) restated in numpy: a Viterbi pass over YIN's lag costs.

The frames, d, c and d' are f0_ref's (steps 1-4), tau_min / tau_max f0_ref.lags.  n = tau_max - tau_min + 1 states, state k the lag
tau_min + k.  In `dtype` (float64, or float32 with every operation rounded on its own - what the kernel does):

    lg[k]    = log2(tau_min + k), computed in double; rounded once to float for float32
    bias[k]  = octave_cost * (lg[k] - lg[0])
    o[t, k]  = q + bias[k],  q = d'[t, tau_min + k] if that is finite, else 1
    tr(j, k) = jump_cost * |lg[k] - lg[j]|
    delta[0, k] = o[0, k];  t >= 1:  best = min_j (delta[t - 1, j] + tr(j, k)), the smallest j winning a tie, psi[t, k] = that j;
               delta'[k] = o[t, k] + best;  m = min_k delta'[k];  delta[t, k] = delta'[k] - m
    path     k*[T - 1] = the smallest k attaining min delta[T - 1, .];  k*[t - 1] = psi[t, k*[t]]
    decision tau* = tau_min + k*[t];  cmnd = d'[t, tau*];  voiced iff cmnd < threshold;  f0 by the parabola of f0_ref.decide

There is no unvoiced state and octave_cost never enters the voicing decision.  `track` runs the rule on a given d, `viterbi_track` on
a waveform; `H` is the signal with dominant even harmonics on which plain YIN answers an octave high."""
import math

import numpy as np

import f0_ref as R

OCTAVE_COST, JUMP_COST = 0.02, 0.5


def check_costs(octave_cost, jump_cost):
    for c in (octave_cost, jump_cost):
        if not (math.isfinite(c) and c >= 0):
            raise ValueError("octave_cost / jump_cost must be finite and >= 0")


def table(lo, hi, dtype=np.float64):
    """lg [n]: log2 of every lag in double, rounded once to `dtype`"""
    return np.array([math.log2(float(tau)) for tau in range(lo, hi + 1)], np.float64).astype(dtype)


def observations(dp, lo, hi, octave_cost=OCTAVE_COST):
    """o [T, n] in dp's dtype"""
    dtype = dp.dtype.type
    lg = table(lo, hi, dtype)
    bias = (dtype(octave_cost) * (lg - lg[0]).astype(dtype)).astype(dtype)
    q = dp[:, lo:hi + 1]
    q = np.where(np.isfinite(q), q, dtype(1))
    return (q + bias[None, :]).astype(dtype)


def transitions(lo, hi, jump_cost=JUMP_COST, dtype=np.float64):
    """tr [n (j), n (k)]"""
    lg = table(lo, hi, dtype)
    return (dtype(jump_cost) * np.abs((lg[None, :] - lg[:, None]).astype(dtype))).astype(dtype)


def path(o, tr):
    """k* [T] of observations o [T, n] under transitions tr [n, n]: the recurrence and the backtrack of the rule, in o's dtype"""
    dtype = o.dtype.type
    T, n = o.shape
    psi = np.zeros((T, n), np.int64)
    delta = o[0].copy()
    for t in range(1, T):
        v = (delta[:, None] + tr).astype(dtype)               # [j, k]
        psi[t] = np.argmin(v, axis=0)                         # the first j that attains the minimum
        best = v[psi[t], np.arange(n)]
        dn = (o[t] + best).astype(dtype)
        delta = (dn - dn.min()).astype(dtype)
    k = np.zeros(T, np.int64)
    k[T - 1] = int(np.argmin(delta))
    for t in range(T - 1, 0, -1):
        k[t - 1] = psi[t, k[t]]
    return k


def track(d, sr=R.SR, fmin=62.5, fmax=500.0, thr=0.15, octave_cost=OCTAVE_COST, jump_cost=JUMP_COST, dtype=np.float64):
    """(f0 [T], cmnd [T], lag [T] int32) in `dtype` from d [T, 257]"""
    lo, hi = R.lags(sr, fmin, fmax)
    if not 0 < thr <= 1:
        raise ValueError("threshold outside (0, 1]")
    check_costs(octave_cost, jump_cost)
    dp = R.cmnd(d, dtype)
    with np.errstate(all="ignore"):
        k = path(observations(dp, lo, hi, octave_cost), transitions(lo, hi, jump_cost, dtype))
    T = dp.shape[0]
    f0, cm, lag = np.zeros(T, dtype), np.zeros(T, dtype), np.zeros(T, np.int32)
    two = dtype(2)
    with np.errstate(all="ignore"):
        for t in range(T):
            tau = lo + int(k[t])
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


def viterbi_track(x, sr=R.SR, hop=R.HOP, fmin=62.5, fmax=500.0, thr=0.15, octave_cost=OCTAVE_COST, jump_cost=JUMP_COST,
                  dtype=np.float64):
    """the whole rule for one utterance -> (f0, cmnd, lag, d)"""
    d = R.difference(x, hop)
    return track(d, sr, fmin, fmax, thr, octave_cost, jump_cost, dtype) + (d,)


# ---- test signals ------------------------------------------------------------------------------------------------------------

H_FREQS, H_WEAK = (110.0, 146.83, 220.5), (0.2, 0.3, 0.4)


def H(f, a, L=16000, vanishing=False, seed=5, sr=R.SR):
    """f32 [L]: a am sin(w n + .3) + sin(2 w n + .6) + .5 a am sin(3 w n + .9) + .5 sin(4 w n + 1.2), w = 2 pi f / sr, with
    am = .75 + .25 sin(2 pi 3 n / sr) - or .5 (1 + sin(2 pi 3 n / sr)) when `vanishing`: the odd harmonics then vanish periodically -
    scaled to peak 0.5, plus N(0, 1e-3^2).  The even harmonics dominate: d'[tau0 / 2] dips under YIN's threshold."""
    n = np.arange(L, dtype=np.float64)
    s = np.sin(2 * np.pi * 3 * n / sr)
    am = 0.5 * (1 + s) if vanishing else 0.75 + 0.25 * s
    w = 2 * np.pi * f * n / sr
    x = a * am * np.sin(w + 0.3) + np.sin(2 * w + 0.6) + 0.5 * a * am * np.sin(3 * w + 0.9) + 0.5 * np.sin(4 * w + 1.2)
    x = 0.5 * x / np.abs(x).max()
    x = (x + 1e-3 * np.random.default_rng(seed).standard_normal(L)).astype(np.float32)
    x.setflags(write=False)
    return x
