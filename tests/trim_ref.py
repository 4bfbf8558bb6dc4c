"""The silence-trimming rule of csrc/trim.hip restated in numpy float64 (no GPU, no library): what librosa documents for
effects.trim(y, top_db) with ref = np.max, centred frames and zero padding, frame 2048 / hop 512.

    s[j] = sum x[i]^2 over [512 j, 512 j + 512) and [0, L);   F = 1 + L // 512;   e[f] = s[f-2] + s[f-1] + s[f] + s[f+1]
    E = max e;  c = float32(10 ** (-top_db / 10));  frame f kept iff e[f] > E * c
    start = 512 * first kept,  end = min(L, 512 * (last kept + 1));  E < FLT_MIN: the utterance is left whole
"""
import numpy as np

FRAME, HOP = 2048, 512
FLT_MIN = float(np.finfo(np.float32).tiny)


def factor(top_db):
    return np.float32(10 ** (-top_db / 10))


def block_sums(x):
    x = np.asarray(x, np.float64)
    nb = -(-x.size // HOP)
    xp = np.zeros(nb * HOP, np.float64)
    xp[:x.size] = x
    return (xp * xp).reshape(nb, HOP).sum(axis=1)


def energies(x):
    """e [F] float64, the block form"""
    s, F = block_sums(x), 1 + len(x) // HOP
    sp = np.zeros(F + 3, np.float64)                 # sp[j + 2] = s[j]
    sp[2:2 + s.size] = s
    return sp[0:F] + sp[1:F + 1] + sp[2:F + 2] + sp[3:F + 3]


def energies_direct(x):
    """e [F] float64 by summing each centred, zero-padded frame [512 f - 1024, 512 f + 1024) directly"""
    x = np.asarray(x, np.float64)
    F = 1 + x.size // HOP
    xp = np.zeros(FRAME // 2 + (F - 1) * HOP + FRAME // 2, np.float64)
    xp[FRAME // 2:FRAME // 2 + x.size] = x
    return np.array([np.sum(xp[f * HOP:f * HOP + FRAME] ** 2) for f in range(F)])


def bounds(x, top_db):
    """(start, end)"""
    e, L = energies(x), len(x)
    E = e.max()
    if E < FLT_MIN:
        return 0, L
    kept = np.nonzero(e > E * float(factor(top_db)))[0]
    return HOP * int(kept[0]), min(L, HOP * (int(kept[-1]) + 1))


def margin(x, top_db):
    """min_f |e[f] / (E c) - 1|: how far the closest frame is from the threshold, relative (inf for a silent utterance)"""
    e = energies(x)
    E = e.max()
    return np.inf if E < FLT_MIN else float(np.abs(e / (E * float(factor(top_db))) - 1.0).min())


def trim_alignment(phone_tokens, durations, start, end, hop=256):
    """the alignment rule, frame by frame: the cut prompt's frames are the original frames [s, s + T'), s = start // hop,
    T' = 1 + (end - start) // hop; a phone keeps those of its frames that are among them, a phone with none left goes"""
    if start % hop:
        raise ValueError("start inside a mel frame")
    s, frames = start // hop, 1 + (end - start) // hop
    owner = np.repeat(np.arange(len(durations)), durations)          # the phone of each original frame
    if s + frames > owner.size:
        raise ValueError("alignment shorter than the cut audio")
    owner = owner[s:s + frames]
    idx = [i for i in range(len(durations)) if (owner == i).any()]
    return [phone_tokens[i] for i in idx], [int((owner == i).sum()) for i in idx]


def burst_signal(L, where, seed=0, floor=1e-3, amp=0.5):
    """f32 [L]: a noise floor (N(0, floor^2)) plus, on about a third of the utterance, a ramped (raised-cosine edges) burst of a
    440 Hz tone and noise at amplitude `amp`; where = "start" | "interior" | "end" puts the burst at that place"""
    rng = np.random.default_rng(7919 * seed + L)
    x = floor * rng.standard_normal(L)
    n = max(1, L // 3)
    a = {"start": 0, "interior": (L - n) // 2, "end": L - n}[where]
    t = np.arange(n, dtype=np.float64)
    ramp = np.minimum(1.0, np.minimum(t + 1, n - t) / max(1.0, n / 8))
    env = 0.5 - 0.5 * np.cos(np.pi * ramp)
    x[a:a + n] += amp * env * (0.7 * np.sin(2 * np.pi * 440.0 * t / 16000.0) + 0.3 * rng.standard_normal(n))
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x
