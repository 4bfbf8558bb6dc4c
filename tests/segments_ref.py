"""The speech-segment rule of csrc/segments.hip restated in numpy (no GPU, no library; the frames and energies are trim_ref's):

    a[f] = e[f] > E c,  E = max e,  c = float32(10 ** (-top_db / 10));  E < FLT_MIN: every frame                    raw
    b    = a, and every inactive run BETWEEN two active frames that is shorter than min_pause frames                close
    c    = b without its runs shorter than min_speech frames                                                       open
    d[f] = some g in [0, F) with |g - f| <= pad has c[g];  c empty: d all true ("nothing found")                    pad
    segment k = the k-th maximal run [f0, f1] of d: frames [f0, f1 + 1), samples [512 f0, min(L, 512 (f1 + 1)))
    cut: the kept frames (d, or not d with keep = "pauses") one after the other, frame f being x[512 f : min(L, 512 (f + 1))]

Everything is written run by run and frame by frame, with no scan: it shares no formulation with the kernel.  `mutate` names a
deliberately wrong variant, for the tests that show the checks can tell: "close_le" closes a pause of exactly min_pause frames too,
"pad_unclamped" lets the pad run past the last frame."""
import numpy as np

import trim_ref as T

HOP = T.HOP
INT_MAX = 2 ** 31 - 1
NAMES = ("frames", "raw_active", "kept_frames", "segments", "kept_samples", "longest_pause", "kept_energy", "dropped_energy")


def runs(flags):
    """[(first, last)] of the maximal runs of true"""
    out, start = [], None
    for f, v in enumerate(list(flags) + [False]):
        if v and start is None:
            start = f
        elif not v and start is not None:
            out.append((start, f - 1))
            start = None
    return out


def raw(e, top_db):
    """a [F] bool.  float32 energies (the device's own) meet the threshold as one f32 product, as the kernel computes it; float64 ones
    (trim_ref.energies) in double, as trim_ref.bounds does"""
    e = np.asarray(e)
    E = max(e.max(), 0)
    if E < T.FLT_MIN:
        return np.ones(e.size, bool)
    thr = np.float32(E) * T.factor(top_db) if e.dtype == np.float32 else float(E) * float(T.factor(top_db))
    return e > thr


def close(a, min_pause, mutate=None):
    b = np.array(a, bool)
    for (_, p), (n, _) in zip(runs(a)[:-1], runs(a)[1:]):
        gap = n - p - 1
        if gap < min_pause or (mutate == "close_le" and gap == min_pause):
            b[p + 1:n] = True
    return b


def open_(b, min_speech):
    c = np.array(b, bool)
    for s, t in runs(b):
        if t - s + 1 < min_speech:
            c[s:t + 1] = False
    return c


def widen(c, pad, mutate=None):
    F = len(c)
    d = np.zeros(F + (pad if mutate == "pad_unclamped" else 0), bool)
    if not np.any(c):
        d[:] = True
    for g in np.nonzero(c)[0]:
        d[max(0, g - pad):min(len(d), g + pad + 1)] = True
    return d


def smooth(a, min_pause, min_speech, pad, mutate=None):
    """-> dict b, c, d (bool arrays), found"""
    b = close(a, min_pause, mutate)
    c = open_(b, min_speech)
    return {"b": b, "c": c, "d": widen(c, pad, mutate), "found": bool(c.any())}


def frame_segments(d):
    """[(f0, f1 + 1)]"""
    return [(s, t + 1) for s, t in runs(d)]


def sample_segments(d, L):
    return [(HOP * s, min(L, HOP * (t + 1))) for s, t in runs(d)]


def bound(F, min_pause, min_speech):
    return max(1, (F + min_pause) // (min_speech + min_pause))


def kept_flags(d, keep):
    d = np.asarray(d, bool)
    return ~d if keep == "pauses" else d


def cut(x, d, keep="speech"):
    x = np.asarray(x)
    parts = [x[HOP * f:min(len(x), HOP * (f + 1))] for f in np.nonzero(kept_flags(d, keep))[0]]
    return np.concatenate(parts) if parts else x[:0]


def figures(e, a, s, keep="speech", L=None):
    """the eight figures (NAMES) from the energies, the raw flags and smooth()'s result; L None: the staged form (512 per kept frame)"""
    e = np.asarray(e, np.float64)
    d = s["d"][:e.size]
    k = kept_flags(d, keep)
    segs = runs(d)
    samples = HOP * int(k.sum()) if L is None else len(cut(np.zeros(L, np.int8), d, keep))
    pauses = [n[0] - p[1] - 1 for p, n in zip(segs[:-1], segs[1:])]
    nk, nd = int(k.sum()), int((~k).sum())
    return np.array([e.size, int(np.sum(a)), nk, len(segs) if s["found"] else -len(segs), samples, max(pauses, default=0),
                     e[k].sum() / nk if nk else 0.0, e[~k].sum() / nd if nd else 0.0])


def analyse(x, top_db=40.0, min_pause=10, min_speech=3, pad=2, keep="speech", e=None):
    """the whole rule on a waveform -> dict: e, a, b, c, d, found, segments (samples), out, figures.  e: other energies than the
    restatement's own (the device's)"""
    x = np.asarray(x)
    e = T.energies(x) if e is None else np.asarray(e)
    a = raw(e, top_db)
    s = smooth(a, min_pause, min_speech, pad)
    return dict(s, e=e, a=a, segments=sample_segments(s["d"], len(x)), out=cut(x, s["d"], keep), figures=figures(e, a, s, keep, len(x)))


def cut_alignment(phone_tokens, durations, segments, hop=256):
    """the alignment rule, frame by frame: the cut prompt's mel frames are, segment by segment, the original frames
    [start // hop, start // hop + (end - start) // hop), and one more behind the last segment's; a phone keeps those of its frames that
    are among them, a phone with none left goes"""
    owner = np.repeat(np.arange(len(durations)), durations)          # the phone of each original frame
    keep = []
    for k, (start, end) in enumerate(segments):
        if start % hop:
            raise ValueError("a segment starts inside a mel frame")
        n = (end - start) // hop + (1 if k == len(segments) - 1 else 0)
        keep.extend(range(start // hop, start // hop + n))
    if keep and keep[-1] >= owner.size:
        raise ValueError("alignment shorter than the cut audio")
    owner = owner[keep]
    idx = [i for i in range(len(durations)) if (owner == i).any()]
    return [phone_tokens[i] for i in idx], [int((owner == i).sum()) for i in idx]


PLAN = (7, 9, 5, 1, 13, 6, 6, 6, 40, 20, 9)      # blocks of 512 samples: pause, speech, pause, ... ; then a tail of 137 samples of pause
TAIL = 137


def plan_signal(plan=PLAN, tail=TAIL, seed=0, floor=1e-4, amp=0.5, shift=0):
    """f32 [L]: tone bursts (440 Hz + noise at `amp`) on a noise floor N(0, floor^2), laid out in blocks of 512 samples that alternate
    pause, speech, pause, ...; `shift` samples of floor in front make the bursts unaligned with the blocks"""
    rng = np.random.default_rng(104729 * seed + len(plan) + shift)
    L = shift + HOP * sum(plan) + tail
    x = floor * rng.standard_normal(L)
    at = shift
    for i, n in enumerate(plan):
        if i % 2:
            t = np.arange(HOP * n, dtype=np.float64)
            x[at:at + HOP * n] += amp * (0.7 * np.sin(2 * np.pi * 440.0 * t / 16000.0) + 0.3 * rng.standard_normal(HOP * n))
        at += HOP * n
    x = x.astype(np.float32)
    x.setflags(write=False)
    return x
