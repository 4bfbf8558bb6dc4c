"""Row f3 measurement: the speech segments and the cut of the pauses (MelFrontEnd.cut_pauses, csrc/segments.hip) on the GPU, next to
the trimmer's time for the same clips.  The clips are 16 kHz, peak-normalised: a noise floor with speech-like bursts of 0.4 - 2.5 s
between pauses of 0.1 - 1.2 s.  cut_ms is the whole call between two device events (the memset, trim's two energy kernels, the
smoothing kernel, the figures kernel, the copy kernel, the copy of the output lengths to the host and the wait for it);
segments_ms is mt2_speech_segments, which only enqueues; the per-kernel split is the handle's stage timer on one more call.
Bytes: the audio is read twice (block sums, copy) and written once - 4 * B * (2 L + Lout_max); GB/s = those bytes over cut_ms.
usage: python tools/bench_segments.py   -> one JSON line per case: 30 s clips at B = 1 and 32, one 10-minute clip"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd.runtime import MelFrontEnd, Pauses

K = 20
SR = 16000
fe = MelFrontEnd()


def clip(B, secs, seed=0):
    rng = np.random.default_rng(seed)
    L = int(secs * SR)
    wav = 1e-3 * rng.standard_normal((B, L))
    for b in range(B):
        at = int(rng.uniform(0.1, 1.2) * SR)
        while at < L:
            n = int(rng.uniform(0.4, 2.5) * SR)
            wav[b, at:at + n] += 0.1 * rng.standard_normal(min(n, L - at))
            at += n + int(rng.uniform(0.1, 1.2) * SR)
    wav /= np.abs(wav).max(axis=1, keepdims=True)
    return torch.from_numpy(wav.astype(np.float32)).cuda()


def timed_ms(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": round(float(np.median(ms)), 4), "least": round(float(np.min(ms)), 4), "largest": round(float(np.max(ms)), 4)}


for B, secs in ((1, 30.0), (32, 30.0), (1, 600.0)):
    y = clip(B, secs)
    L = y.shape[1]
    out = torch.empty_like(y)
    cut = timed_ms(lambda: fe.cut_pauses(y, None, Pauses(), out=out, return_figures=True))
    seg = timed_ms(lambda: fe.speech_segments(y, None, Pauses()))
    trim = timed_ms(lambda: fe.trim(y, None, 40.0, out=out))
    fe.set_profiling(True)
    _, out_lens, fig = fe.cut_pauses(y, None, Pauses(), out=out, return_figures=True)
    split = {k: round(v, 4) for k, v in fe.last_stage_ms().items()}
    fe.set_profiling(False)
    fig = fig.cpu().numpy()
    gbytes = 4e-9 * B * (2 * L + L)
    print(json.dumps({"metric": "cut_pauses ms per call (%d timed calls, 3 warm-up)" % K, "seconds": secs, "batch": B, "samples": L,
                      "frames": int(fig[0, 0]), "segments_first": int(fig[0, 3]), "kept_samples_first": int(out_lens[0]),
                      "cut_ms": cut, "segments_ms": seg, "kernel_split_ms": split, "gbytes": round(gbytes, 5),
                      "gb_per_s": round(gbytes / (cut["median"] * 1e-3), 1), "trim_ms_same_clip": trim}), flush=True)
