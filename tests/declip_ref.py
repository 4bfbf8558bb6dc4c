"""The declipping rule of csrc/declip.hip (A-SPADE: Kitic, Bertin and Gribonval 2015; the analysis variant of Zaviska et al. 2021)
restated in float64 numpy; its home is include/megatts2_hip.h.  Nothing here is imported from the package: the tests hold the kernels
to this file, and this file to numpy.fft and to ground truth (a known signal, clipped).

All frames of an utterance iterate side by side: the sparsity k of iteration i depends on i alone (k = s (1 + (i - 1) // r)), so the
k-th largest |v|^2 of every active frame is one partition along the bin axis.

fft="numpy" transforms with numpy.fft;  fft="kernel" with the kernel's own transform, restated below: the N-point real DFT as an N / 2
point complex radix-2 (forward: decimation in frequency, natural order in, bit-reversed out;  inverse: decimation in time, bit-reversed
in, natural out) and the split into / from the half spectrum."""
import dataclasses
import math

import numpy as np

NAMES = ("clipped", "hi", "lo", "share", "frames_iterated", "mean_iterations", "max_iterations", "power_change_db")
NEAR_TIE = 1e-9


@dataclasses.dataclass(frozen=True)
class Rule:
    frame: int = 1024
    tol: float = 1e-3
    min_share: float = 1e-4
    min_count: int = 4
    level: float = float("nan")
    step: int = 1
    every: int = 1
    eps: float = 0.02
    max_iter: int = 0

    @property
    def hop(self):
        return self.frame // 4

    @property
    def bins(self):
        return self.frame // 2 + 1

    @property
    def iterations(self):
        return self.max_iter if self.max_iter > 0 else self.every * -(-self.bins // self.step)


def window(N):
    n = np.arange(N, dtype=np.float64)
    return np.sqrt(0.5 - 0.5 * np.cos(2.0 * np.pi * n / N))


def frames_of(length, N):
    return -(-length // (N // 4)) + 3


# ---- detection: every comparison in f32, the counts integers
def detect(y, rule=Rule()):
    y = np.asarray(y, np.float32)
    n = len(y)
    res = {"nonfinite": bool(not np.all(np.isfinite(y))), "need": max(int(rule.min_count), int(math.ceil(rule.min_share * n)))}
    if math.isnan(rule.level):
        with np.errstate(invalid="ignore"):
            hi, lo = np.float32(np.fmax.reduce(y)), np.float32(np.fmin.reduce(y))
    else:
        hi, lo = np.float32(rule.level), np.float32(-np.float32(rule.level))
    tol = np.float32(rule.tol)
    with np.errstate(invalid="ignore", over="ignore"):
        thr_hi = np.float32(hi - np.float32(tol * np.abs(hi)))
        thr_lo = np.float32(lo + np.float32(tol * np.abs(lo)))
        H = (y >= thr_hi) if hi > 0 else np.zeros(n, bool)
        L = (y <= thr_lo) if lo < 0 else np.zeros(n, bool)
    res.update(hi=hi, lo=lo, n_hi=int(H.sum()), n_lo=int(L.sum()))
    res["clip_hi"] = (not res["nonfinite"]) and res["n_hi"] >= res["need"]
    res["clip_lo"] = (not res["nonfinite"]) and res["n_lo"] >= res["need"]
    res["H"] = H if res["clip_hi"] else np.zeros(n, bool)
    res["L"] = L if res["clip_lo"] else np.zeros(n, bool)
    res["clipped"] = res["clip_hi"] or res["clip_lo"]
    return res


def detect_figures(y, rule=Rule()):
    """the eight figures of mt2_clip_detect: no restoration, so the last four are zero"""
    d = detect(y, rule)
    if d["nonfinite"]:
        return np.asarray([0.0, np.nan, np.nan, 0.0, 0.0, 0.0, 0.0, 0.0])
    share = (int(d["H"].sum()) + int(d["L"].sum())) / len(y)
    return np.asarray([float(d["clipped"]), float(d["hi"]), float(d["lo"]), share, 0.0, 0.0, 0.0, 0.0])


# ---- the kernel's transform
def _twiddles(N):
    return np.exp(-2j * np.pi * np.arange(N // 2) / N)


def _bitrev(M):
    bits = M.bit_length() - 1
    r = np.zeros(M, np.int64)
    for i in range(bits):
        r |= ((np.arange(M) >> i) & 1) << (bits - 1 - i)
    return r


def kernel_rfft(x):
    """A x for the rows of x [R, N]: the half spectrum [R, N / 2 + 1], scaled by 1 / sqrt(N)"""
    x = np.asarray(x, np.float64)
    R, N = x.shape
    M, tw = N // 2, _twiddles(N)
    z = (x[:, 0::2] + 1j * x[:, 1::2]).copy()
    h = M // 2
    while h >= 1:
        zz = z.reshape(R, M // (2 * h), 2, h)
        a, b = zz[:, :, 0, :].copy(), zz[:, :, 1, :].copy()
        zz[:, :, 0, :] = a + b
        zz[:, :, 1, :] = (a - b) * tw[np.arange(h) * (N // (2 * h))]
        h //= 2
    Z = z[:, _bitrev(M)]                                                       # Z[k] sits at position bitrev(k)
    X = np.empty((R, M + 1), np.complex128)
    X[:, 0] = Z[:, 0].real + Z[:, 0].imag
    X[:, M] = Z[:, 0].real - Z[:, 0].imag
    k = np.arange(1, M)
    Zk, Zc = Z[:, k], np.conj(Z[:, M - k])
    X[:, k] = 0.5 * (Zk + Zc) + tw[k] * (-0.5j * (Zk - Zc))
    return X / math.sqrt(N)


def kernel_irfft(X):
    """A^H X for the rows of the half spectrum X [R, N / 2 + 1] -> [R, N]"""
    X = np.asarray(X, np.complex128)
    R, M = X.shape[0], X.shape[1] - 1
    N, tw = 2 * M, _twiddles(2 * M)
    k = np.arange(M)
    Xk, Xc = X[:, k], np.conj(X[:, M - k])
    Z = 0.5 * (Xk + Xc) + 1j * (np.conj(tw[k]) * (0.5 * (Xk - Xc)))
    z = np.empty_like(Z)
    z[:, _bitrev(M)] = Z
    h = 1
    while h < M:
        zz = z.reshape(R, M // (2 * h), 2, h)
        a, b = zz[:, :, 0, :].copy(), zz[:, :, 1, :] * np.conj(tw[np.arange(h) * (N // (2 * h))])
        zz[:, :, 0, :] = a + b
        zz[:, :, 1, :] = a - b
        h *= 2
    out = np.empty((R, N))
    out[:, 0::2] = z.real
    out[:, 1::2] = z.imag
    return out * (2.0 / math.sqrt(N))


def _A(x, fft):
    return kernel_rfft(x) if fft == "kernel" else np.fft.rfft(x, axis=1) / math.sqrt(x.shape[1])


def _AH(X, N, fft):
    return kernel_irfft(X) if fft == "kernel" else np.fft.irfft(X, n=N, axis=1) * math.sqrt(N)


def _norm2(d):
    """|d|^2 summed over the FULL spectrum from the half: the inner bins count twice"""
    m = d.real ** 2 + d.imag ** 2
    return m[:, 0] + m[:, -1] + 2.0 * m[:, 1:-1].sum(axis=1)


# ---- the rule
def declip(y, rule=Rule(), fft="numpy", mutate=None):
    """-> dict: out (f32), out64 (the value before its one rounding; the input where the input's bits are written), iters int32 [T],
    figures [8], near_tie bool [T], det (detect's answer).  mutate: None, "no_u" (u never updated) or "free" (no constraint on the
    clipped samples) - the two mutations the host tests must tell from the rule."""
    y = np.asarray(y, np.float32)
    n, N, hop, K = len(y), rule.frame, rule.hop, rule.bins
    T = frames_of(n, N)
    det = detect(y, rule)
    iters, near = np.zeros(T, np.int32), np.zeros(T, bool)
    if not det["clipped"]:
        fig = detect_figures(y, rule)
        return {"out": y.copy(), "out64": y.astype(np.float64), "iters": iters, "figures": fig, "near_tie": near, "det": det}
    w = window(N)
    pad = np.zeros((T + 3) * hop)
    pad[3 * hop:3 * hop + n] = y
    mH, mL = np.zeros(len(pad), bool), np.zeros(len(pad), bool)
    mH[3 * hop:3 * hop + n], mL[3 * hop:3 * hop + n] = det["H"], det["L"]
    own = np.zeros(len(pad), bool)                                             # the utterance's own reliable samples: pads anchor nothing
    own[3 * hop:3 * hop + n] = ~(det["H"] | det["L"])
    idx = np.arange(T)[:, None] * hop + np.arange(N)[None, :]
    F, fH, fL = pad[idx] * w, mH[idx], mL[idx]
    normF = np.sqrt((F * F).sum(axis=1))
    X = F.copy()
    act = np.flatnonzero((normF > 0) & (fH | fL).any(axis=1) & own[idx].any(axis=1))
    U = np.zeros((len(act), K), np.complex128)
    x = F[act].copy()
    Fa, Ha, La, nFa = F[act], fH[act], fL[act], normF[act]
    Ax = _A(x, fft)
    k = rule.step
    for i in range(1, rule.iterations + 1):
        if len(act) == 0:
            break
        v = Ax + U
        m = v.real ** 2 + v.imag ** 2
        kk = min(k, K)
        part = np.partition(m, [K - kk - 1, K - kk] if kk < K else [K - kk], axis=1)
        thr = part[:, K - kk]
        if kk < K:
            with np.errstate(invalid="ignore", divide="ignore"):
                near[act] |= (thr - part[:, K - kk - 1]) < NEAR_TIE * thr
        zb = np.where(m >= thr[:, None], v, 0.0)
        t = _AH(zb - U, N, fft)
        if mutate == "free":
            x = np.where(Ha | La, t, Fa)
        else:
            x = np.where(Ha, np.maximum(t, Fa), np.where(La, np.minimum(t, Fa), Fa))
        Ax = _A(x, fft)
        d = Ax - zb
        nd = np.sqrt(_norm2(d))
        bar = rule.eps * nFa
        near[act] |= np.abs(nd - bar) < NEAR_TIE * bar
        stop = nd <= bar
        iters[act] = i
        X[act] = x
        if mutate != "no_u":
            U = U + d
        if i % rule.every == 0:
            k += rule.step
        go = ~stop
        act, U, x, Ax, Fa, Ha, La, nFa = act[go], U[go], x[go], Ax[go], Fa[go], Ha[go], La[go], nFa[go]
    # synthesis: every sample gathers its four frames in ascending order
    num, den = np.zeros(len(pad)), np.zeros(len(pad))
    for t in range(T):
        num[t * hop:t * hop + N] += X[t] * w
        den[t * hop:t * hop + N] += w * w
    o64 = (num[3 * hop:3 * hop + n] / den[3 * hop:3 * hop + n])
    o32 = o64.astype(np.float32)
    out = y.copy()
    out[det["H"]] = np.maximum(o32, y)[det["H"]]
    out[det["L"]] = np.minimum(o32, y)[det["L"]]
    out64 = y.astype(np.float64)
    out64[det["H"]] = np.maximum(o64, y)[det["H"]]
    out64[det["L"]] = np.minimum(o64, y)[det["L"]]
    fig = detect_figures(y, rule)
    ran = iters > 0
    fig[4] = float(ran.sum())
    fig[5] = float(iters[ran].mean()) if ran.any() else 0.0
    fig[6] = float(iters.max())
    fig[7] = 10.0 * math.log10(float((out.astype(np.float64) ** 2).sum()) / float((y.astype(np.float64) ** 2).sum()))
    return {"out": out, "out64": out64, "iters": iters, "figures": fig, "near_tie": near, "det": det}


# ---- the test signal and its measure
def make_signal(N, seed, sr=16000, length=None):
    """12 harmonics of a 150 Hz fundamental that wobbles +-10 % at 1.5 Hz, amplitudes 0.7^h and random phases; 3 Hz amplitude modulation
    at 40 %; white noise of sigma 0.003; peak-normalised; N + 24 hop samples"""
    rng = np.random.default_rng(seed)
    n = N + 24 * (N // 4) if length is None else length
    t = np.arange(n) / sr
    phase = 2.0 * np.pi * np.cumsum(150.0 * (1.0 + 0.1 * np.sin(2.0 * np.pi * 1.5 * t))) / sr
    x = np.zeros(n)
    for h in range(1, 13):
        x += 0.7 ** h * np.sin(h * phase + rng.uniform(0.0, 2.0 * np.pi))
    x *= 1.0 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t)
    x += 0.003 * rng.standard_normal(n)
    return (x / np.abs(x).max()).astype(np.float32)


def clip(x, theta):
    return np.clip(x, -theta, theta).astype(np.float32)


def sdr_db(ref, est, margin):
    r, e = np.asarray(ref, np.float64)[margin:-margin], np.asarray(est, np.float64)[margin:-margin]
    return 10.0 * math.log10(float((r * r).sum()) / float(((r - e) ** 2).sum()))
