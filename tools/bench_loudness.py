"""Integrated loudness (MelFrontEnd.loudness) and loudness normalisation (MelFrontEnd.loudness_normalize, csrc/loudness.hip) on the
GPU: 30 s clips at 16 kHz, B = 1 and 8, medians of 20 calls between device events, measuring and normalising separately, with the
per-kernel times of the handle's stage events (medians of 20 profiled calls).  Beside them, on the same clips: MelFrontEnd.trim, the
mel front-end, and - once, B = 1 - the float64 restatement tests/loudness_ref.py on the CPU.
Bytes: the audio is read twice by the filter (zero-state pass, sums pass) and, normalising, read and written once more.
usage: python tools/bench_loudness.py [seconds]   -> one JSON line per B"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
from megatts2_amd.runtime import MelFrontEnd

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
    env = 10.0 ** (-1.0 - np.sin(2 * np.pi * 0.3 * np.arange(L) / SR))
    wav = (0.3 * env * rng.standard_normal((B, L))).astype(np.float32)
    x = torch.from_numpy(wav).cuda()
    out, cut = torch.empty_like(x), torch.empty_like(x)
    measure_ms = median_ms(lambda: fe.loudness(x))
    normalize_ms = median_ms(lambda: fe.loudness_normalize(x, target_lufs=-23.0, out=out))
    kernels = stage_ms(lambda: fe.loudness_normalize(x, target_lufs=-23.0, out=out))
    trim_ms = median_ms(lambda: fe.trim(x, None, 40.0, out=cut))
    mel_ms = median_ms(lambda: fe(x))
    st = fe.loudness(x).cpu().numpy()
    res = {"metric": "loudness ms per call (median of %d)" % K, "seconds": secs, "batch": B, "samples": L,
           "integrated_lufs_row0": round(float(st[0, 0]), 3), "measure_ms": round(measure_ms, 4), "normalize_ms": round(normalize_ms, 4),
           "kernel_ms_normalize": kernels, "measure_gb_per_s": round(4e-9 * B * 2 * L / (measure_ms * 1e-3), 1),
           "trim_ms_same_clip": round(trim_ms, 4), "mel_frontend_ms_same_clip": round(mel_ms, 4)}
    if B == 1:
        import loudness_ref
        t0 = time.perf_counter()
        ref = loudness_ref.measure(wav[0], SR)
        res["numpy_restatement_ms_one_clip"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["restatement_minus_device_lu"] = float(ref["I"] - st[0, 0])
    print(json.dumps(res), flush=True)
