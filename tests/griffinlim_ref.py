"""Restatement of the Griffin-Lim rule (csrc/griffinlim.hip, include/megatts2_hip.h) in numpy.  Test helper: no GPU needed.

Everything runs in float64 by default, the transforms as FFTs.  `dt=np.float32` is the rule as it is stated for f32: every stored
array and every elementwise operation is rounded to f32, and the two transforms are what the rule says they are - one f32 dot per
output value against a basis built in double and rounded once (numpy's f32 matrix product: f32 products and sums, in BLAS's order).
An f32 run whose FFTs stayed in double would leave out the largest rounding of every step and is no yardstick for the iteration.
The constants the rule fixes in f32 (the filterbank, the pseudo-inverse P, c) are the f32 values in both modes; the squared window
is exact in float64, so that istft is torch.istft there."""
import functools

import numpy as np

from megatts2_oracle import melscale_fbanks
from sampling_ref import uniform_np


def window(audio):
    """periodic Hann of win_length centred in n_fft, float64"""
    w = np.zeros(audio.n_fft)
    left = (audio.n_fft - audio.win_length) // 2
    w[left:left + audio.win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(audio.win_length) / audio.win_length)
    return w


@functools.lru_cache(maxsize=None)
def _bases_f32(n_fft, win_length):
    """(forward basis [2F, N], inverse basis [N, 2F]) of the rule, built in double and rounded once to f32: the windowed DFT, and
    the windowed inverse with the 1/N, 2/N Hermitian weights (zero columns for the imaginary parts of bins 0 and N/2)"""
    N, F = n_fft, n_fft // 2 + 1
    w = np.zeros(N)
    left = (N - win_length) // 2
    w[left:left + win_length] = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win_length) / win_length)
    ang = 2.0 * np.pi * ((np.arange(F)[:, None] * np.arange(N)[None, :]) % N) / N
    fwd = np.concatenate([np.cos(ang) * w, -np.sin(ang) * w]).astype(np.float32)
    wt = np.where((np.arange(F) == 0) | (2 * np.arange(F) == N), 1.0, 2.0)[:, None] / N
    im = -np.sin(ang) * wt
    im[(np.arange(F) == 0) | (2 * np.arange(F) == N)] = 0.0
    inv = (np.concatenate([np.cos(ang) * wt, im]) * w).T.astype(np.float32)
    return fwd, np.ascontiguousarray(inv)


def filterbank(audio):
    """the front-end's mel filterbank, rounded to f32: [n_mels, F]"""
    F = audio.n_fft // 2 + 1
    return np.ascontiguousarray(melscale_fbanks(F, audio.f_min, audio.f_max, audio.n_mels, audio.sample_rate).T).astype(np.float32)


def pinv_cholesky(fb):
    """P = fb^T (fb fb^T)^-1 in float64 by Cholesky, [F, n_mels]; numpy.linalg.LinAlgError when the Gram matrix is not positive
    definite"""
    fb = np.asarray(fb, np.float64)
    G = fb @ fb.T
    L = np.linalg.cholesky(G)
    if not (np.diag(L) ** 2 > 1e-12 * np.diag(G).max()).all():
        raise np.linalg.LinAlgError("Gram matrix is not positive definite")
    y = np.linalg.solve(L, fb)
    return np.linalg.solve(L.T, y).T


def mel_to_linear(M, audio, dt=np.float64):
    """A[t, f] = max(0, sum_j exp(M[t, j]) P[f, j])"""
    P = pinv_cholesky(filterbank(audio)).astype(np.float32).astype(dt)
    E = np.exp(np.asarray(M, np.float32).astype(dt))
    return np.maximum((E @ P.T).astype(dt), dt(0))


def phase_uniform(seed, T, F):
    return uniform_np(np.uint64(seed), np.arange(T * F)).reshape(T, F)


def phase_init(A, seed, dt=np.float64):
    """S0 = A (cos, sin)(2 pi u); f32: theta = 2 pi u rounded to f32, as the kernel forms it"""
    T, F = A.shape
    u = phase_uniform(seed, T, F)
    theta = (np.float32(2.0 * np.pi) * u.astype(np.float32)) if dt == np.float32 else 2.0 * np.pi * u
    theta = theta.astype(dt)
    A = np.asarray(A, dt)
    return (A * np.cos(theta)).astype(dt) + 1j * (A * np.sin(theta)).astype(dt)


def istft(S, audio, dt=np.float64, edge_interior=False):
    """torch.istft(center=True, length=(T - 1) hop): S complex [T, F] -> x [(T - 1) hop].  edge_interior: the MUTATION of the rule
    that divides by the interior envelope everywhere (for tests of the tests)."""
    N, h = audio.n_fft, audio.hop_length
    T = S.shape[0]
    w = window(audio)
    w2 = (w * w).astype(dt)                 # f32: rounded once from double, as the kernel's table
    if dt == np.float32:                     # one f32 dot of 2F terms per sample
        packed = np.concatenate([S.real, S.imag], axis=1).astype(np.float32)
        y = packed @ _bases_f32(N, audio.win_length)[1].T
    else:
        y = np.fft.irfft(np.asarray(S, np.complex128), n=N, axis=1) * w
    s, e = np.zeros((T - 1) * h + N, dt), np.zeros((T - 1) * h + N, dt)
    for t in range(T):                       # ascending t: every sample sums its frames in ascending t
        s[t * h:t * h + N] += y[t]
        e[t * h:t * h + N] += w2
    if edge_interior:
        full = np.zeros(h, dt)
        for k in range(N // h):
            full += w2[k * h:(k + 1) * h]
        e = np.tile(full, e.size // h + 1)[:e.size]
    L = (T - 1) * h
    return (s[N // 2:N // 2 + L] / e[N // 2:N // 2 + L]).astype(dt)


def stft(x, audio, dt=np.float64):
    """the front-end's STFT: reflect padding by N/2, frames every hop, windowed rfft -> complex [1 + L // hop, F]"""
    N, h = audio.n_fft, audio.hop_length
    x = np.asarray(x, np.float64)
    xp = np.pad(x, (N // 2, N // 2), mode="reflect")
    T = 1 + x.size // h
    frames = np.stack([xp[t * h:t * h + N] for t in range(T)])
    if dt == np.float32:                     # one f32 dot of N terms per bin and part
        R = frames.astype(np.float32) @ _bases_f32(N, audio.win_length)[0].T
        F = N // 2 + 1
        return R[:, :F].astype(np.float64) + 1j * R[:, F:].astype(np.float64)
    return np.fft.rfft(frames * window(audio), axis=1)


def log_mel(x, audio):
    mag = np.abs(stft(x, audio))
    return np.log(np.maximum(mag @ filterbank(audio).astype(np.float64).T, audio.clip)).astype(np.float32)


def phase_update(R, Rprev, A, c, dt=np.float64, rprev_first=False):
    """-> S_next: D = R - c Rprev, S = D (A / (|D| + 1e-16)).  rprev_first: the MUTATION that overwrites Rprev with R before D."""
    if rprev_first:
        Rprev = R
    c = dt(c)
    dr = (R.real.astype(dt) - (c * Rprev.real.astype(dt)).astype(dt)).astype(dt)
    di = (R.imag.astype(dt) - (c * Rprev.imag.astype(dt)).astype(dt)).astype(dt)
    mag = np.sqrt((dr * dr).astype(dt) + (di * di).astype(dt)).astype(dt)
    g = (np.asarray(A, dt) / (mag + dt(1e-16)).astype(dt)).astype(dt)
    return (dr * g).astype(dt) + 1j * (di * g).astype(dt)


def residual(R, A, dt=np.float64):
    """sum_f (|R| - A)^2 per frame"""
    rr, ri = R.real.astype(dt), R.imag.astype(dt)
    d = (np.sqrt((rr * rr).astype(dt) + (ri * ri).astype(dt)).astype(dt) - np.asarray(A, dt)).astype(dt)
    return (d * d).astype(dt).sum(axis=1, dtype=dt)


def momentum_c(momentum):
    return np.float32(momentum / (1.0 + momentum))


def griffin_lim(M, seed, audio, n_iter=32, momentum=0.99, dt=np.float64, edge_interior=False, rprev_first=False):
    """-> (x [(T - 1) hop], resid [n_iter + 1, T], A [T, F]) for one utterance's log-mel M [T, n_mels]"""
    A = mel_to_linear(M, audio, dt)
    S = phase_init(A, seed, dt)
    c = momentum_c(momentum)
    Rprev = np.zeros_like(S)
    resid = np.zeros((n_iter + 1, A.shape[0]), dt)
    for k in range(n_iter):
        x = istft(S, audio, dt, edge_interior)
        R = stft(x, audio, dt)
        resid[k] = residual(R, A, dt)
        S = phase_update(R, Rprev, A, c, dt, rprev_first)
        Rprev = R
    x = istft(S, audio, dt, edge_interior)
    resid[n_iter] = residual(stft(x, audio, dt), A, dt)
    return x, resid, A


def spectral_convergence(resid, A):
    """sqrt(sum_t resid[k, t] / sum A^2) for every k, in float64"""
    return np.sqrt(np.asarray(resid, np.float64).sum(axis=-1) / (np.asarray(A, np.float64) ** 2).sum())


# ---- test signals (peak-normalised) ------------------------------------------------------------------------------------------

def two_tone_noise(L, sample_rate=16000, seed=0):
    t = np.arange(L) / sample_rate
    x = np.sin(2 * np.pi * 440.0 * t) + 0.5 * np.sin(2 * np.pi * 1730.0 * t + 0.3)
    x = x + 0.05 * np.random.default_rng(seed).standard_normal(L)
    return (x / np.abs(x).max()).astype(np.float32)


def vibrato_stack(L, sample_rate=16000, f0=180.0, n_harm=12):
    t = np.arange(L) / sample_rate
    phase = 2 * np.pi * f0 * t + 6.0 * np.sin(2 * np.pi * 5.5 * t)
    x = sum(np.sin(k * phase) / k for k in range(1, n_harm + 1))
    x = x * (0.6 + 0.4 * np.sin(2 * np.pi * 2.0 * t) ** 2)
    return (x / np.abs(x).max()).astype(np.float32)
