"""The true-peak look-ahead limiter (MelFrontEnd.limit and MelFrontEnd.loudness_normalize(..., true_peak_ceiling_dbtp=, limiter=),
csrc/limiter.hip) on the GPU: 30 s clips at 16 kHz, B = 1 and 8, medians of 20 calls between device events, with the per-kernel times
of the handle's stage events (medians of 20 profiled calls).  Beside them, on the same clips: the parent's call, normalisation under a
true-peak ceiling by one gain, whose seven launches the limiter call starts with six of.
The clips are noise under a slow swell with a crest 20 dB over the body every 250 ms, so that the ceiling binds and about a twelfth
of the samples are limited.
Work of the new kernels: the envelope is L * (o - 1) * 24 * 5 / 4 f32 fma (o = 12 at 16 kHz: five chains for four samples) over one
read of the audio; the gain kernel is (2 H + 1) fma a sample from LDS (161 at H = 80; the weights end in three zeros, 164 issued)
and (1 + 4 H / 1024) divisions.
usage: python tools/bench_limiter.py [seconds]   -> one JSON line per B"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd.runtime import Limiter, MelFrontEnd

secs = float(sys.argv[1]) if len(sys.argv) > 1 else 30.0
K = 20
SR = 16000
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


def stage_ms(fn):
    fe.set_profiling(True)
    runs = []
    for _ in range(K):
        fn()
        runs.append(fe.last_stage_ms())
    fe.set_profiling(False)
    return {k: round(float(np.median([r[k] for r in runs])), 4) for k in runs[0]}


for B in (1, 8):
    L = int(secs * SR)
    rng = np.random.default_rng(0)
    env = 10.0 ** (-1.0 - 0.3 * np.sin(2 * np.pi * 0.3 * np.arange(L) / SR))
    wav = 0.3 * env * rng.standard_normal((B, L))
    wav[:, SR // 8::SR // 4] = 0.9
    x = torch.from_numpy(wav.astype(np.float32)).cuda()
    out = torch.empty_like(x)
    tp = dict(target_lufs=-23.0, out=out, true_peak_ceiling_dbtp=-1.0)
    res = {"metric": "limiter ms per call (median of %d)" % K, "seconds": secs, "batch": B, "samples": L,
           "normalize_tp_ms_parent_call": round(median_ms(lambda: fe.loudness_normalize(x, **tp)), 4),
           "limit_ms_one_pass": round(median_ms(lambda: fe.limit(x, None, 12.0, -1.0, out=out)), 4)}
    for P in (1, 2, 3):
        res["normalize_limited_ms_%d_pass" % P] = round(median_ms(lambda: fe.loudness_normalize(x, limiter=Limiter(5.0, P), **tp)), 4)
    res["normalize_limited_ms_2_pass_with_stats"] = round(median_ms(lambda: fe.loudness_normalize(x, limiter=Limiter(5.0, 2), return_stats=True, **tp)), 4)
    kernels = stage_ms(lambda: fe.loudness_normalize(x, limiter=Limiter(5.0, 2), **tp))
    res["kernel_ms_normalize_limited_2_pass"] = kernels
    _, st = fe.loudness_normalize(x, limiter=Limiter(5.0, 2), return_stats=True, **tp)
    one = fe.loudness_ebu(fe.loudness_normalize(x, **tp)).cpu().numpy()
    st = st.cpu().numpy()
    res.update({"one_gain_reaches_lufs_row0": round(float(one[0, 0]), 3), "limiter_reaches_lufs_row0": round(float(st[0, 23]), 3),
                "share_limited_row0": round(float(st[0, 20]) / L, 4), "min_gain_row0": round(float(st[0, 19]), 4),
                "envelope_gfma_per_s": round(1e-9 * B * L * 11 * 24 * 1.25 / (kernels["lim_envelope"] * 1e-3), 1),
                "gain_gfma_per_s": round(1e-9 * B * L * 164 / (kernels["lim_gain2"] * 1e-3), 1)})
    print(json.dumps(res), flush=True)
