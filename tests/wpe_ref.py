"""Restatement of the weighted-prediction-error rule (csrc/wpe.hip, include/megatts2_hip.h) in float64 numpy, vectorised over the bins.
Test helper: no GPU needed.

`wpe(Y, cfg)` takes a complex spectrum [T, F] whose parts are f32 values and runs steps 1-3 of the rule on every bin at once.  The sums
over t of step 2.3 run in the kernel's order (`order="lanes"`: lane l of 64 adds its frames l, l + 64, ... in ascending order, then the
butterfly of strides 32 .. 1) or in plain ascending order (`order="ascending"`) - the difference between the two is the summation-order
noise that sets the bar of tests/test_gpu_wpe.py.  The Cholesky and the two solves are the textbook column forms; their inner sums are
numpy's, so the restatement is NOT bit-equal to the device and is not meant to be.

Two mutations, for testing the tests: `mutate="delay"` predicts from delay + 1 (the first tap of a known filter is missed), and
`mutate="lambda_from_Y"` takes the variance from Y in every iteration (the iteration does nothing after its first pass)."""
import dataclasses

import numpy as np

import griffinlim_ref as G

FIELDS = ("power_in", "power_out", "reduction_db", "frames", "bins_filtered", "bins_passed", "max_tap", "iterations")


@dataclasses.dataclass(frozen=True)
class Config:
    delay: int = 3
    taps: int = 10
    iterations: int = 3
    context: int = 1
    variance_floor: float = 1e-2
    loading: float = 1e-8


def regressor(Y, lag):
    """x[t] = Y[t - lag], 0 where the index is negative"""
    X = np.zeros_like(Y)
    if lag < Y.shape[0]:
        X[lag:] = Y[:Y.shape[0] - lag]
    return X


def variance(D, c):
    """step 2.1: the mean of |D|^2 over the existing frames within c, ascending sums, one division by the count"""
    pw = D.real * D.real + D.imag * D.imag
    T = pw.shape[0]
    s, cnt = np.zeros_like(pw), np.zeros(T)
    for d in range(-c, c + 1):
        lo, hi = max(0, -d), min(T, T - d)
        if lo < hi:
            s[lo:hi] += pw[lo + d:hi + d]
            cnt[lo:hi] += 1
    return s / cnt[:, None]


def tsum(A, order):
    """the sum over axis 0 of A [T, F].  A reduction along the outer axis of a C-contiguous array adds row after row: ascending"""
    A = np.ascontiguousarray(A)
    if order == "ascending":
        return np.add.reduce(A, axis=0)
    T, F = A.shape
    n = (T + 63) // 64
    P = np.zeros((n * 64, F), A.dtype)
    P[:T] = A
    v = np.add.reduce(P.reshape(n, 64, F), axis=0)
    lane = np.arange(64)
    for d in (32, 16, 8, 4, 2, 1):
        v = v + v[lane ^ d]
    return v[0]


def cholesky(R):
    """step 2.5, a column at a time: R [F, K, K] (lower triangle read) -> L, and the bins where a pivot was not a positive finite number"""
    F, K, _ = R.shape
    L = np.zeros_like(R)
    bad = np.zeros(F, bool)
    for j in range(K):
        s = R[:, j:, j] - np.einsum("fim,fm->fi", L[:, j:, :j], np.conj(L[:, j, :j]))
        d = s[:, 0].real
        bad |= ~((d > 0) & np.isfinite(d))
        r = np.sqrt(np.where(bad, 1.0, d))
        L[:, j:, j] = s / r[:, None]
        L[:, j, j] = r
    return L, bad


def solve(L, p):
    """step 2.6: L z = p, then L^H g = z"""
    F, K = p.shape
    z = np.zeros_like(p)
    for j in range(K):
        z[:, j] = (p[:, j] - np.einsum("fm,fm->f", L[:, j, :j], z[:, :j])) / L[:, j, j].real
    g = np.zeros_like(p)
    for j in range(K - 1, -1, -1):
        g[:, j] = (z[:, j] - np.einsum("fm,fm->f", np.conj(L[:, j + 1:, j]), g[:, j + 1:])) / L[:, j, j].real
    return g


def predict(X, g):
    """sum_k conj(g[k]) x_k[t], k ascending: X [K][T, F], g [F, K]"""
    s = np.zeros_like(X[0])
    for k in range(len(X)):
        s = s + np.conj(g[None, :, k]) * X[k]
    return s


def wpe(Y, cfg=Config(), order="lanes", mutate=None):
    """steps 1-3 on Y complex [T, F] -> dict(D [T, F] with f32 parts, g [F, K], filtered [F] bool, iterations [F] int, figures [8])"""
    Y = np.asarray(Y, np.complex128)
    T, F = Y.shape
    K, delay = cfg.taps, cfg.delay + (1 if mutate == "delay" else 0)
    X = [regressor(Y, delay + k) for k in range(K)]
    D = Y.copy()
    g = np.zeros((F, K), np.complex128)
    active = np.ones(F, bool)
    done = np.zeros(F, np.int64)
    with np.errstate(all="ignore"):
        for _ in range(cfg.iterations):
            P = variance(Y if mutate == "lambda_from_Y" else D, cfg.context)
            mx = np.fmax.reduce(P, axis=0)
            active &= (mx > 0) & np.isfinite(mx)
            w = 1.0 / np.fmax(P, cfg.variance_floor * mx[None, :])
            R = np.zeros((F, K, K), np.complex128)
            p = np.zeros((F, K), np.complex128)
            for j in range(K):
                xw = X[j] * w
                for k in range(j + 1):
                    R[:, j, k] = tsum(xw * np.conj(X[k]), order)
                p[:, j] = tsum(xw * np.conj(Y), order)
            tr = np.zeros(F)
            for j in range(K):
                tr = tr + R[:, j, j].real
            idx = np.arange(K)
            R[:, idx, idx] = R[:, idx, idx].real + (cfg.loading * tr / K)[:, None]
            L, bad = cholesky(R)
            active &= ~bad
            gn = solve(L, p)
            g[active] = gn[active]
            D[:, active] = (Y - predict(X, gn))[:, active]
            done += active
    filtered = active
    g[~filtered] = 0
    D[:, ~filtered] = Y[:, ~filtered]
    D = D.real.astype(np.float32).astype(np.float64) + 1j * D.imag.astype(np.float32).astype(np.float64)
    sY, sD = float((np.abs(Y) ** 2).sum()), float((np.abs(D) ** 2).sum())
    with np.errstate(all="ignore"):
        fig = np.array([sY, sD, 10 * np.log10(np.float64(sD) / np.float64(sY)), T, filtered.sum(), F - filtered.sum(),
                        np.abs(g).max() if filtered.any() else 0.0, done.max()])
    return dict(D=D, g=g, filtered=filtered, iterations=done, figures=fig)


def dereverb(x, audio, cfg=Config(), **kw):
    """the whole call for one utterance -> dict(y [hop (L // hop)], S, and wpe's results): a clip of fewer than delay + 4 taps frames
    passes through the two transforms unfiltered"""
    S = G.stft(np.asarray(x, np.float32), audio)
    S = S.real.astype(np.float32).astype(np.float64) + 1j * S.imag.astype(np.float32).astype(np.float64)
    if S.shape[0] < cfg.delay + 4 * cfg.taps:
        F = S.shape[1]
        r = dict(D=S, g=np.zeros((F, cfg.taps), np.complex128), filtered=np.zeros(F, bool), iterations=np.zeros(F, np.int64))
    else:
        r = wpe(S, cfg, **kw)
    r["S"] = S
    r["y"] = G.istft(r["D"], audio)
    return r


def pack(S):
    """complex [T, F] -> the f32 rows [T, S] of mt2_stft's layout: re | im | zero pad"""
    T, F = S.shape
    out = np.zeros((T, (2 * F + 3) & ~3), np.float32)
    out[:, :F], out[:, F:2 * F] = S.real, S.imag
    return out


def unpack(rows, F):
    return rows[:, :F].astype(np.float64) + 1j * rows[:, F:2 * F].astype(np.float64)


# ---- test signals --------------------------------------------------------------------------------------------------------------

def gated_bursts(L, seed=0, sample_rate=16000):
    """white-noise bursts of random length (40 - 200 ms) and level, with EXACTLY silent gaps of 20 - 120 ms between them"""
    rng = np.random.default_rng(seed)
    x = np.zeros(L)
    at = 0
    while at < L:
        n = int(rng.uniform(0.04, 0.2) * sample_rate)
        x[at:at + n] = rng.uniform(0.05, 0.3) * rng.standard_normal(min(n, L - at))
        at += n + int(rng.uniform(0.02, 0.12) * sample_rate)
    return x.astype(np.float32)


def echo(x, hops, hop, gain=0.5):
    """x plus one reflection of `gain`, `hops` hops later"""
    y = np.asarray(x, np.float64).copy()
    d = hops * hop
    y[d:] += gain * np.asarray(x[:len(x) - d], np.float64)
    return y.astype(np.float32)


def error_db(y, clean):
    n = len(y)
    c = np.asarray(clean[:n], np.float64)
    return 10 * np.log10(((np.asarray(y, np.float64) - c) ** 2).sum() / (c ** 2).sum())


def known_filter(K=10, seed=0):
    """a stable prediction filter whose first tap is its largest: |g_k| = 0.2 0.8^k, random phases"""
    rng = np.random.default_rng(1000 + seed)
    return 0.2 * 0.8 ** np.arange(K) * np.exp(2j * np.pi * rng.random(K))


def ar_columns(T, F, g, delay, seed=0):
    """Y[t] = S[t] + sum_k conj(g_k) Y[t - delay - k] in every bin, S complex Gaussian whose variance is 1 and 0.01 in alternate runs of
    12 frames; the parts of Y are rounded to f32, as a spectrum's are.  -> (Y, S)"""
    rng = np.random.default_rng(seed)
    sd = np.where((np.arange(T) // 12) % 2 == 0, 1.0, 0.1)[:, None]
    S = sd * (rng.standard_normal((T, F)) + 1j * rng.standard_normal((T, F))) / np.sqrt(2.0)
    Y = np.zeros((T, F), np.complex128)
    for t in range(T):
        acc = S[t].copy()
        for k in range(len(g)):
            if t - delay - k >= 0:
                acc += np.conj(g[k]) * Y[t - delay - k]
        Y[t] = acc
    Y = Y.real.astype(np.float32).astype(np.float64) + 1j * Y.imag.astype(np.float32).astype(np.float64)
    return Y, S


def resid_db(D, S):
    """||D - S||^2 / ||S||^2 per bin, in dB"""
    return 10 * np.log10((np.abs(D - S) ** 2).sum(axis=0) / (np.abs(S) ** 2).sum(axis=0))


def spectrum_signal(audio, T, seed=11, tail=7):
    """the input of the spectrum tests: bursts with one echo at 4 hops, T frames and `tail` samples more"""
    L = (T - 1) * audio.hop_length + tail
    return echo(gated_bursts(L, seed), 4, audio.hop_length)
