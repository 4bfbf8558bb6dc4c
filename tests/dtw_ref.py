"""Restatement of the DTW rule of csrc/dtw.hip (header comment; include/megatts2_hip.h) in numpy: accumulation, directions, backtrack
and durations in float32 GIVEN the costs - min is exact and each cell is one rounded add, so the kernels are held to these bit for
bit - and the cost itself in float64, which the kernel's one f32 fma chain is held to within (D + 3) * 2^-24 relative."""
import numpy as np

DIAG, UP, LEFT = 0, 1, 2


def cost64(x, y):
    """c[i, j] = sum_k (x[i, k] - y[j, k])^2 in float64 of the f32 inputs; x [Tx, D], y [Ty, D]"""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    d = x[:, None, :] - y[None, :, :]
    return (d * d).sum(axis=2)


def cost32_chain(x, y):
    """the kernel's own chain in float32 up to the fma's single rounding (here the square is rounded too): for hand cases whose
    squares are exact"""
    x, y = np.asarray(x, np.float32), np.asarray(y, np.float32)
    acc = np.zeros((x.shape[0], y.shape[0]), np.float32)
    for k in range(x.shape[1]):
        d = x[:, None, k] - y[None, :, k]
        acc = (acc + d * d).astype(np.float32)
    return acc


def accumulate(c):
    """c f32 [Tx, Ty] -> (A f32 [Tx, Ty], direction codes int8 [Tx, Ty]); the code of (0, 0) is LEFT and is never followed"""
    c = np.asarray(c, np.float32)
    Tx, Ty = c.shape
    A = np.zeros((Tx, Ty), np.float32)
    dirs = np.full((Tx, Ty), LEFT, np.int8)
    A[0, 0] = c[0, 0]
    for j in range(1, Ty):
        A[0, j] = np.float32(c[0, j] + A[0, j - 1])
    for i in range(1, Tx):
        A[i, 0] = np.float32(c[i, 0] + A[i - 1, 0])
        dirs[i, 0] = UP
        up_row, row, crow = A[i - 1], A[i], c[i]
        for j in range(1, Ty):
            dg, up, lf = up_row[j - 1], up_row[j], row[j - 1]
            if dg <= up and dg <= lf:
                dirs[i, j] = DIAG
            elif up <= lf:
                dirs[i, j] = UP
            row[j] = np.float32(crow[j] + min(dg, up, lf))
    return A, dirs


def backtrack(dirs):
    """direction codes [Tx, Ty] -> (lo int32 [Ty], hi int32 [Ty], steps)"""
    Tx, Ty = dirs.shape
    lo, hi = np.full(Ty, Tx, np.int32), np.full(Ty, -1, np.int32)
    i, j, steps = Tx - 1, Ty - 1, 0
    while True:
        lo[j], hi[j], steps = min(lo[j], i), max(hi[j], i), steps + 1
        if i == 0 and j == 0:
            break
        d = LEFT if i == 0 else UP if j == 0 else dirs[i, j]
        if d == DIAG:
            i, j = i - 1, j - 1
        elif d == UP:
            i -= 1
        else:
            j -= 1
    return lo, hi, steps


def align(c):
    """c f32 [Tx, Ty] -> dict(acc, lo, hi, steps, total)"""
    A, dirs = accumulate(c)
    lo, hi, steps = backtrack(dirs)
    return {"acc": A, "lo": lo, "hi": hi, "steps": steps, "total": A[-1, -1]}


def durations(hi, s):
    """hi int [Ty] non-decreasing, s int [Np] >= 0 with sum = hi[-1] + 1 -> dur int32 [Np]: the frames j with
    cum[p] <= hi[j] < cum[p + 1], counted one by one (the kernel does it by two binary searches)"""
    hi, s = np.asarray(hi, np.int64), np.asarray(s, np.int64)
    cum = np.concatenate([[0], np.cumsum(s)])
    dur = np.zeros(s.size, np.int32)
    for j in range(hi.size):
        p = int(np.searchsorted(cum, hi[j], side="right")) - 1           # the last p with cum[p] <= hi[j]
        assert cum[p] <= hi[j] < cum[p + 1]
        dur[p] += 1
    return dur


def check_path(lo, hi, Tx, Ty):
    """the invariants that make lo / hi a whole monotone path"""
    lo, hi = np.asarray(lo), np.asarray(hi)
    assert lo.shape == hi.shape == (Ty,)
    assert lo[0] == 0 and hi[-1] == Tx - 1 and (lo <= hi).all()
    nxt = lo[1:] - hi[:-1]
    assert ((nxt == 0) | (nxt == 1)).all()
    return int((hi - lo + 1).sum())          # the number of cells = steps


def warp_rows(x, reps):
    """y = x's rows repeated reps[i] times"""
    return np.repeat(np.asarray(x), np.asarray(reps), axis=0)
