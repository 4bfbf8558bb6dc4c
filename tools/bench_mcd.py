"""Mel-cepstral distortion along the DTW path (MelFrontEnd.mcd, csrc/mcd.hip) on the GPU, next to the DTW's own time for the same
clips: two log-mels of `seconds` each (1 + seconds * 16000 / 256 frames of 80 bins; the second is the first read through a smooth
time warp - frame t takes frame t + 40 sin(6 pi t / T), so both start and end together and the timing drifts by up to 40 frames in
between - with noise on top).  The path reduction walks a column's vertical run in one thread, by the rule: a pair whose path ends in
one long run (clips that do not end together) pays for that run cell by cell, which this pair does not show.
mcd_ms is the whole chain (two cepstrum launches, the three DTW launches on the 13 cepstra, the path reduction); cepstrum_ms and
path_ms its two own kernels as calls of their own; dtw_cepstra_ms the DTW call on the 13-column cepstra and dtw_mel_ms the same call on
the 80-bin mels - the yardstick the two new kernels are read against; stage_ms the chain between its own stage events (both cepstrum
launches, the three DTW kernels, the path reduction).
usage: python tools/bench_mcd.py [seconds]   -> one JSON line per B"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd.runtime import MelFrontEnd

secs = float(sys.argv[1]) if len(sys.argv) > 1 else 30.0
K = 20
ORDER = 13
fe = MelFrontEnd()


def median_ms(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


for B in (1, 8):
    T = 1 + int(secs * 16000) // 256
    rng = np.random.default_rng(0)
    a = (np.cumsum(rng.standard_normal((B, T, 80)), axis=1) * 0.3 + rng.standard_normal((B, T, 80)) * 0.05 - 4.0).astype(np.float32)
    t = np.arange(T)
    warp = np.clip(np.rint(t + 40.0 * np.sin(6.0 * np.pi * t / T)).astype(np.int64), 0, T - 1)
    b = (a[:, warp] + 0.1 * rng.standard_normal((B, T, 80))).astype(np.float32)
    f0 = (120.0 * 2.0 ** rng.uniform(-0.3, 0.3, (B, T))).astype(np.float32)
    A, Bm, F = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda(), torch.from_numpy(f0).cuda()
    mcd_ms = median_ms(lambda: fe.mcd(A, Bm, None, None, F, F, order=ORDER))
    cep_ms = median_ms(lambda: fe.mel_cepstrum(A, None, ORDER))
    ca, cb = fe.mel_cepstrum(A, None, ORDER), fe.mel_cepstrum(Bm, None, ORDER)
    path = fe.dtw(ca, cb)
    path_ms = median_ms(lambda: fe.path_distortion(ca, cb, path["lo"], path["hi"], None, None, F, F))
    dtw_cep_ms = median_ms(lambda: fe.dtw(ca, cb))
    dtw_mel_ms = median_ms(lambda: fe.dtw(A, Bm))
    fe.set_profiling(True)                      # the chain's own stage events: both cepstra, the three DTW kernels, the path reduction
    stages = []
    for _ in range(K):
        fe.mcd(A, Bm, None, None, F, F, order=ORDER)
        stages.append(fe.last_stage_ms())
    fe.set_profiling(False)
    stage_ms = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
    row = fe.mcd(A, Bm, None, None, F, F, order=ORDER)[0].cpu().numpy()
    own = 2 * cep_ms + path_ms
    print(json.dumps({"metric": "mcd ms per call (median of %d)" % K, "seconds": secs, "batch": B, "frames": T, "order": ORDER,
                      "cells": int(row[0]), "mcd_db": round(float(row[1]), 4), "mcd_ms": round(mcd_ms, 4),
                      "cepstrum_ms_one_side": round(cep_ms, 4), "path_ms": round(path_ms, 4), "dtw_cepstra_ms": round(dtw_cep_ms, 4),
                      "dtw_mel_ms": round(dtw_mel_ms, 4), "own_kernels_over_dtw_cepstra": round(own / dtw_cep_ms, 4), "stage_ms": stage_ms}), flush=True)
