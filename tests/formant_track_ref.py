"""The rule of mt2_formant_track (include/megatts2_hip.h, csrc/formant_track.hip) restated in numpy, and the synthetic scene the host
and the GPU tests share.

Everything is in float64 with every operation rounded on its own (numpy never contracts), the f32 inputs convert exactly and the rule
has no transcendental function: every cost, and hence every decision, is reproduced to the bit.

`track` is the literal reading, one Python loop per index.  `track_fast` is the same rule with the states vectorised (the sums still
run q ascending, left to right, element by element - the same bits); the host tests hold the two equal, the GPU tests use the fast one.
"""
import itertools

import numpy as np

MAX = 5                                     # MT2_FORMANT_MAX
DEFAULT_REF = (550.0, 1650.0, 2750.0, 3850.0, 4950.0)


def states(K):
    """the C(5, K) strictly increasing K-tuples of {0 .. 4} in lexicographic order"""
    return list(itertools.combinations(range(MAX), K))


def gaps(freq, bw, count, K):
    """-> (gap bool [T], n int [T]): n = min(count, 5); a gap has n < K or a bad freq / bw among its first n candidates"""
    freq, bw = np.asarray(freq, np.float32), np.asarray(bw, np.float32)
    n = np.minimum(np.asarray(count, np.int64), MAX)
    first = np.arange(MAX)[None, :] < n[:, None]
    with np.errstate(invalid="ignore"):
        bad = ~(np.isfinite(freq) & (freq > 0) & np.isfinite(bw) & (bw >= 0))
    return (n < K) | (bad & first).any(1), n


def local_cost(f, b, ref_q, freq_cost, bw_cost):
    """term_q = (freq_cost * (|f - ref_q| / 1000)) + (bw_cost * (b / f))"""
    return (freq_cost * (np.abs(f - ref_q) / 1000.0)) + (bw_cost * (b / f))


def jump(f_prev, f_now):
    """u_q = (2 * |f' - f|) / (f' + f)"""
    return (2.0 * np.abs(f_now - f_prev)) / (f_now + f_prev)


def track(freq, bw, count, K=4, ref_hz=DEFAULT_REF, freq_cost=1.0, bw_cost=1.0, jump_cost=1.0, return_tables=False):
    """The literal rule -> sel int [T, 5], track_freq, track_bw f32 [T, 5], track_count int32 [T] (and delta, psi on request)."""
    freq, bw = np.asarray(freq, np.float32), np.asarray(bw, np.float32)
    T = len(count)
    st = states(K)
    S = len(st)
    gap, n = gaps(freq, bw, count, K)
    fd, bd = freq.astype(np.float64), bw.astype(np.float64)
    fc, bc, jc = np.float64(freq_cost), np.float64(bw_cost), np.float64(jump_cost)
    ref = [np.float64(r) for r in ref_hz]
    inf = np.float64(np.inf)
    delta = np.zeros((T, S), np.float64)
    psi = np.zeros((T, S), np.int64)
    with np.errstate(all="ignore"):
        for t in range(T):
            if gap[t]:
                if t > 0:
                    bj, best = 0, delta[t - 1, 0]
                    for j in range(1, S):
                        if delta[t - 1, j] < best:
                            bj, best = j, delta[t - 1, j]
                    psi[t, :] = bj
                continue
            for k in range(S):
                if st[k][K - 1] >= n[t]:
                    delta[t, k] = inf
                    continue
                o = None
                for q in range(K):
                    c = st[k][q]
                    term = local_cost(fd[t, c], bd[t, c], ref[q], fc, bc)
                    o = term if o is None else o + term
                if t == 0 or gap[t - 1]:
                    delta[t, k] = o
                    continue
                best, bj = inf, 0
                for j in range(S):
                    if not np.isfinite(delta[t - 1, j]):
                        continue
                    a = None
                    for q in range(K):
                        u = jump(fd[t - 1, st[j][q]], fd[t, st[k][q]])
                        a = u if a is None else a + u
                    v = delta[t - 1, j] + jc * a
                    if v < best:
                        best, bj = v, j
                delta[t, k] = o + best
                psi[t, k] = bj
    out = _backtrack(freq, bw, gap, delta, psi, st, K)
    return out + (delta, psi) if return_tables else out


def _first_min(v, last_wins):
    """arg-min along axis 0, the first of equals - or, for the WRONG rule a test shows its ties with, the last"""
    return len(v) - 1 - np.argmin(v[::-1], axis=0) if last_wins else np.argmin(v, axis=0)


def _backtrack(freq, bw, gap, delta, psi, st, K, last_wins=False):
    T = len(gap)
    sel = -np.ones((T, MAX), np.int32)
    tf = np.zeros((T, MAX), np.float32)
    tb = np.zeros((T, MAX), np.float32)
    tc = np.zeros(T, np.int32)
    k = int(_first_min(delta[T - 1], last_wins))            # the first of equals
    for t in range(T - 1, -1, -1):
        if not gap[t]:
            c = list(st[k])
            sel[t, :K] = c
            tf[t, :K] = freq[t, c]
            tb[t, :K] = bw[t, c]
            tc[t] = K
        k = int(psi[t, k])
    return sel, tf, tb, tc


def track_fast(freq, bw, count, K=4, ref_hz=DEFAULT_REF, freq_cost=1.0, bw_cost=1.0, jump_cost=1.0, last_wins=False):
    """The same rule, the states and the frames of the tables vectorised; only the recurrence loops over t.  last_wins=True is NOT
    the rule: every tie goes to the largest index instead - a test that holds a kernel to the tie-breaks shows with it that its
    inputs have ties that change the answer."""
    freq, bw = np.asarray(freq, np.float32), np.asarray(bw, np.float32)
    T = len(count)
    st = np.asarray(states(K), np.int64)       # [S, K]
    S = len(st)
    gap, n = gaps(freq, bw, count, K)
    fd, bd = freq.astype(np.float64), bw.astype(np.float64)
    fc, bc, jc = np.float64(freq_cost), np.float64(bw_cost), np.float64(jump_cost)
    with np.errstate(all="ignore"):
        o = None                                # [T, S]
        for q in range(K):
            term = local_cost(fd[:, st[:, q]], bd[:, st[:, q]], np.float64(ref_hz[q]), fc, bc)
            o = term if o is None else o + term
        o = np.where(st[None, :, K - 1] < n[:, None], o, np.inf)
        a = None                                # [T - 1, j, k]
        for q in range(K):
            u = jump(fd[:-1, st[:, q]][:, :, None], fd[1:, st[:, q]][:, None, :])
            a = u if a is None else a + u
        tr = jc * a if T > 1 else np.zeros((0, S, S))
        delta = np.zeros((T, S), np.float64)
        psi = np.zeros((T, S), np.int64)
        for t in range(T):
            if gap[t]:
                if t > 0:
                    psi[t, :] = int(_first_min(delta[t - 1], last_wins))
                continue
            if t == 0 or gap[t - 1]:
                delta[t] = o[t]
                continue
            v = np.where(np.isfinite(delta[t - 1])[:, None], delta[t - 1][:, None] + tr[t - 1], np.inf)
            bj = _first_min(v, last_wins)       # the first of equals; 0 where every v is +inf
            bj = np.where(np.isinf(v[bj, np.arange(S)]), 0, bj)
            valid = st[:, K - 1] < n[t]
            delta[t] = np.where(valid, o[t] + v[bj, np.arange(S)], np.inf)
            psi[t] = np.where(valid, bj, 0)
    return _backtrack(freq, bw, gap, delta, psi, [tuple(s) for s in st], K, last_wins)


def path_cost(freq, bw, count, path, K, ref_hz, freq_cost, bw_cost, jump_cost):
    """The total cost of a state sequence over an utterance WITHOUT gaps, summed as the recurrence sums it: ((o_0 + tr_1) + o_1) ... in
    the order delta takes them, i.e. delta[t] = o[t] + (delta[t - 1] + tr); +inf where a state is invalid."""
    fd, bd = np.asarray(freq, np.float32).astype(np.float64), np.asarray(bw, np.float32).astype(np.float64)
    st = states(K)
    n = np.minimum(np.asarray(count), MAX)
    total = None
    with np.errstate(all="ignore"):
        for t, s in enumerate(path):
            if st[s][K - 1] >= n[t]:
                return np.inf
            o = None
            for q in range(K):
                term = local_cost(fd[t, st[s][q]], bd[t, st[s][q]], np.float64(ref_hz[q]), np.float64(freq_cost), np.float64(bw_cost))
                o = term if o is None else o + term
            if t == 0:
                total = o
                continue
            a = None
            for q in range(K):
                u = jump(fd[t - 1, st[path[t - 1]][q]], fd[t, st[s][q]])
                a = u if a is None else a + u
            total = o + (total + np.float64(jump_cost) * a)
    return total


# ---- the scene: five true formants that move, spurious roots between and below them, missing ones ------------------------------------
BASE = (500.0, 1500.0, 2500.0, 3500.0, 4500.0)
AMP = (0.3, 0.2, 0.06, 0.04, 0.03)


def true_tracks(T):
    """-> f, bw float64 [T, 5]"""
    t = np.arange(T)
    f = np.stack([BASE[q] * (1 + AMP[q] * np.sin(2 * np.pi * (t / T) * (1.5 + 0.5 * q) + q)) for q in range(5)], 1)
    b = np.stack([60 + 20 * q + 20 * np.sin(t / 7 + q) for q in range(5)], 1)
    return f, b


def scene(seed, T=192):
    """-> freq, bw f32 [T, 5], count int32 [T], truth int [T, 4] (the slot of true formant q; -1 where it is absent), kind int [T]"""
    r = np.random.default_rng(seed)
    tf, tb = true_tracks(T)
    freq = np.zeros((T, MAX), np.float32)
    bw = np.zeros((T, MAX), np.float32)
    count = np.zeros(T, np.int32)
    truth = -np.ones((T, 4), np.int64)
    kind = np.zeros(T, np.int64)
    prev = 0
    for i in range(T):
        u = r.random()
        w = r.uniform(350, 480)
        lo = r.uniform(150, 260)
        n = int(r.integers(0, 4))
        k = 1 if u < 0.15 else 2 if u < 0.30 else 3 if u < 0.40 else 4 if u < 0.48 else 5 if u < 0.55 else 0
        if k in (1, 2, 5) and k == prev:        # spurious roots are sporadic
            k = 0
        kind[i] = prev = k
        c = [(tf[i, q], tb[i, q], q) for q in range(5)]
        if k == 1:
            c.append((0.5 * (tf[i, 0] + tf[i, 1]), w, -1))
        elif k == 2:
            c.append((lo, w, -1))
        elif k == 3:
            c = c[:4]
        elif k == 4:
            c = c[:n]
        elif k == 5:
            c.append((0.5 * (tf[i, 2] + tf[i, 3]), w, -1))
        c.sort()
        c = c[:MAX]
        count[i] = len(c)
        for slot, (f, b, q) in enumerate(c):
            freq[i, slot], bw[i, slot] = f, b
            if 0 <= q < 4:
                truth[i, q] = slot
    return freq, bw, count, truth, kind


def true_f32(T):
    """the true tracks as the scene stores them: rounded to f32"""
    return true_tracks(T)[0].astype(np.float32)
