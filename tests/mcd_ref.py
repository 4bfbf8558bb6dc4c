"""Restatement of the mel-cepstral-distortion rule of csrc/mcd.hip (header comment; include/megatts2_hip.h) in numpy.

Three levels, each for what it can be held to:
  float64     table64 / cepstrum64: the rule with the f32 inputs and the f32 table read as doubles - what the kernel's one f32 fma
              chain is held to within coefficient_bound, (N + 2) 2^-24 sum_m |M[m]| |tab[m]|: N roundings of the chain, one of the
              table entry, one of the mel itself where the test built it by an f32 sum.
  f32 chain   cepstrum32_chain and, for rule 4, dtw_ref.cost32_chain (which rounds the square as well as the sum): the host tests
              run the whole rule in them - cepstra, dtw_ref.align, path_row - against ground truth that needs no outside tool.
  bit for bit fma32 is an f32 fused multiply-add in numpy (the product is exact in float64; the sum is rounded to odd there, then
              to nearest in f32, which is the single rounding of the true sum); cost32_fma is the kernels' cost chain on it.  Given
              the kernel's own cepstra, the costs, the DTW (dtw_ref.align) and, sum by sum in the kernel's order, the dB fields of the
              row (path_row) are what the device computes; the cents go through log2, which no two libraries round alike.
"""
import math

import numpy as np

import dtw_ref

FIELDS, MAX_ORDER, THREADS = 8, 32, 256
DB = 4.342944819032518                       # the double nearest 10 / ln 10, which the kernel multiplies by
NAMES = ("cells", "mcd_db", "max_db", "voiced_cells", "f0_rmse_cents", "f0_offset_cents", "vuv_cells", "vuv_error")
assert abs(DB - 10.0 / math.log(10.0)) < 1e-15        # the quotient formed in double is one ulp below


def table64(N, K):
    """tab[k-1][m] = cos(pi (m + 1/2) k / N) / N in double, the operations in the order the library takes them"""
    return np.asarray([[math.cos(math.pi * (m + 0.5) * k / N) / N for m in range(N)] for k in range(1, K + 1)], np.float64)


def table32(N, K):
    return table64(N, K).astype(np.float32)


def cepstrum64(mel, K):
    """mel f32 [T, N] -> float64 [T, K]: the f32 mel against the f32 table, summed in double"""
    mel = np.asarray(mel, np.float32)
    return mel.astype(np.float64) @ table32(mel.shape[1], K).astype(np.float64).T


def coefficient_bound(mel, K):
    """[T, K]: (N + 2) 2^-24 sum_m |M[t][m]| |tab[k][m]|, what an f32 chain over m may differ from cepstrum64 by"""
    mel = np.asarray(mel, np.float32)
    N = mel.shape[1]
    return (N + 2) * 2.0 ** -24 * (np.abs(mel.astype(np.float64)) @ np.abs(table32(N, K).astype(np.float64)).T)


def fma32(a, b, c):
    """f32 fmaf(a, b, c), elementwise, with its single rounding: a b is exact in float64 (48 bits); the float64 sum s = p + c is
    off by err (TwoSum, exact); where err != 0 and s is even, the neighbour on err's side is the odd one of the two doubles around
    the true sum.  Rounding that to f32 is rounding the true sum to f32."""
    a, b, c = (np.asarray(v, np.float32).astype(np.float64) for v in (a, b, c))
    p = a * b
    s = p + c
    bb = s - p
    err = (p - (s - bb)) + (c - bb)
    even = (np.ascontiguousarray(s).view(np.int64) & 1) == 0
    fix = np.isfinite(s) & (err != 0) & even
    with np.errstate(invalid="ignore"):
        s = np.where(fix, np.nextafter(s, np.where(err > 0, np.inf, -np.inf)), s)
    with np.errstate(over="ignore"):
        return s.astype(np.float32)


def cepstrum32_chain(mel, K):
    """the kernel's chain: acc = 0; acc = fmaf(M[t][m], tab[k][m], acc) over m ascending -> f32 [T, K]"""
    mel = np.asarray(mel, np.float32)
    tab = table32(mel.shape[1], K)
    acc = np.zeros((mel.shape[0], K), np.float32)
    for m in range(mel.shape[1]):
        acc = fma32(mel[:, m, None], tab[None, :, m], acc)
    return acc


def cost32_fma(x, y):
    """the cost chain of csrc/dtw.hip bit for bit: d = x - y in f32; acc = fmaf(d, d, acc) over k ascending -> f32 [Tx, Ty]"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    acc = np.zeros((x.shape[0], y.shape[0]), np.float32)
    for k in range(x.shape[1]):
        d = x[:, None, k] - y[None, :, k]
        acc = fma32(d, d, acc)
    return acc


def cell_db(q):
    """rule 4: (10 / ln 10) sqrt(2 (double) q)"""
    return DB * np.sqrt(2.0 * np.asarray(q, np.float32).astype(np.float64))


def tree_sum(v):
    v = np.array(v, np.float64)
    s = v.size // 2
    while s:
        v[:s] += v[s:2 * s]
        s //= 2
    return v[0]


def tree_max(v):
    v = np.array(v, np.float64)
    s = v.size // 2
    while s:
        v[:s] = np.fmax(v[:s], v[s:2 * s])
        s //= 2
    return v[0]


def voiced(f):
    return bool(f > 0)          # False for a NaN


def path_row(cost, lo, hi, f0_a=None, f0_b=None, return_abs=False):
    """rules 4 - 7 in the kernel's order: cost f32 [Ta, Tb] (q of every cell), lo / hi int [Tb] -> float64 [8].  Thread t of 256 takes
    the columns t, t + 256, ... and in a column i ascending; the partial sums meet in the fixed tree.  A run is cut to [0, Ta).
    return_abs: (row, mean |D| over the cells voiced on both sides) - what the signed mean's summation error is relative to."""
    cost = np.asarray(cost, np.float32)
    Ta, Tb = cost.shape
    part = np.zeros((7, THREADS), np.float64)          # cells, sum dB, max dB, both, sum D^2, sum D, one
    sum_abs = 0.0
    pitch = f0_a is not None and f0_b is not None
    for t in range(min(THREADS, Tb)):
        for j in range(t, Tb, THREADS):
            for i in range(max(int(lo[j]), 0), min(int(hi[j]), Ta - 1) + 1):
                db = cell_db(cost[i, j])
                part[0, t] += 1
                part[1, t] += db
                part[2, t] = np.fmax(part[2, t], db)
                if pitch:
                    va, vb = voiced(f0_a[i]), voiced(f0_b[j])
                    if va and vb:
                        with np.errstate(all="ignore"):
                            d = 1200.0 * np.log2(np.float64(f0_a[i]) / np.float64(f0_b[j]))
                        part[3, t] += 1
                        part[4, t] += d * d
                        part[5, t] += d
                        sum_abs += abs(d)
                    elif va != vb:
                        part[6, t] += 1
    n, sdb, n2, sd2, sd, n1 = (tree_sum(part[k]) for k in (0, 1, 3, 4, 5, 6))
    mx = tree_max(part[2])
    row = np.zeros(FIELDS, np.float64)
    row[0], row[1], row[2] = n, sdb / n if n else 0.0, mx
    row[3], row[4], row[5] = n2, math.sqrt(sd2 / n2) if n2 else 0.0, sd / n2 if n2 else 0.0
    row[6], row[7] = n1, n1 / n if n else 0.0
    return (row, sum_abs / n2 if n2 else 0.0) if return_abs else row


def distortion(mel_a, mel_b, K=13, f0_a=None, f0_b=None, chain=cepstrum32_chain, cost=dtw_ref.cost32_chain):
    """the whole rule for one pair -> dict(row, lo, hi, steps, total, ca, cb): cepstra, the DTW of dtw_ref on their costs, the row"""
    ca, cb = chain(mel_a, K).astype(np.float32), chain(mel_b, K).astype(np.float32)
    c = cost(ca, cb)
    r = dtw_ref.align(c)
    return {"row": path_row(c, r["lo"], r["hi"], f0_a, f0_b), "lo": r["lo"], "hi": r["hi"], "steps": r["steps"], "total": r["total"],
            "ca": ca, "cb": cb}


def db_bound(mel_a, mel_b, K, delta):
    """What the MCD of a pair may differ by from DB sqrt(2) |delta|, delta [K] the TRUE cepstral difference of every pair of frames on
    the path, when the cepstra come from f32 chains: with e[k] = max_t bound_a[t][k] + max_t bound_b[t][k] (coefficient_bound), the
    computed difference vector is within |e| (2-norm) of delta, so its norm is within |e| of |delta|; the cost chain's K + 3
    roundings change q by at most (K + 3) 2^-24 of itself, hence sqrt(q) by at most that of itself.  The mean over the cells is
    within what every cell is within; the double sum's own error (cells 2^-53) is far below the f32 terms and is added all the same."""
    e = coefficient_bound(mel_a, K).max(axis=0) + coefficient_bound(mel_b, K).max(axis=0)
    en, dn = float(np.sqrt((e * e).sum())), float(np.sqrt((np.asarray(delta, np.float64) ** 2).sum()))
    cells = mel_a.shape[0] + mel_b.shape[0]
    return DB * math.sqrt(2.0) * (en + (dn + en) * (K + 3) * 2.0 ** -24) * (1.0 + cells * 2.0 ** -53)


def cos_mel(mel, a, k0):
    """mel + a cos(pi (m + 1/2) k0 / N) on every frame, rounded once to f32"""
    mel = np.asarray(mel, np.float32)
    N = mel.shape[1]
    bump = a * np.cos(np.pi * (np.arange(N) + 0.5) * k0 / N)
    return (mel.astype(np.float64) + bump[None, :]).astype(np.float32)


def log_mel(T, N=80, seed=0):
    """random log-mels whose frames are far apart in the low cepstra (so that a frame's own copy is its nearest): per frame a random
    smooth spectrum of 8 cosines, a level and noise in every bin, in the range of a natural-log mel"""
    rng = np.random.default_rng(seed)
    k = np.arange(1, min(8, N - 1) + 1)
    smooth = rng.standard_normal((T, k.size)) @ np.cos(np.pi * (np.arange(N)[None, :] + 0.5) * k[:, None] / N)
    return (smooth + rng.standard_normal((T, N)) * 0.5 + rng.standard_normal((T, 1)) - 4.0).astype(np.float32)


def monotone_path(Ta, Tb, rng):
    """a random path of the DTW's three steps from (0, 0) to (Ta - 1, Tb - 1) -> (lo, hi) int32 [Tb]"""
    lo, hi = np.zeros(Tb, np.int32), np.zeros(Tb, np.int32)
    i = j = 0
    while (i, j) != (Ta - 1, Tb - 1):
        moves = [m for m in ((1, 1), (1, 0), (0, 1)) if i + m[0] < Ta and j + m[1] < Tb]
        di, dj = moves[int(rng.integers(len(moves)))]
        i, j = i + di, j + dj
        if dj:
            lo[j] = i
        hi[j] = i
    return lo, hi
