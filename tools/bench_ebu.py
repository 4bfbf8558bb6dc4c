"""EBU-mode metering (MelFrontEnd.loudness_ebu) and normalisation under a true-peak ceiling (MelFrontEnd.loudness_normalize(...,
true_peak_ceiling_dbtp=), csrc/ebu.hip) on the GPU: 30 s clips at 16 kHz, B = 1 and 8, medians of 20 calls between device events, with
the per-kernel times of the handle's stage events (medians of 20 profiled calls).  Beside them, on the same clips: MelFrontEnd.loudness
(the parent's call, whose four kernels run unchanged in front of the two new ones) and - once, B = 1 - the float64 restatement
tests/ebu_ref.py on the CPU.
Work of the new kernels: the true peak is (L + 12) * (o - 1) * 24 f32 fma (o = 12 at 16 kHz) over one read of the audio; the range
kernel reads the ns sub-block sums 30 times (from L2) and passes 18 times over the nst keys.
usage: python tools/bench_ebu.py [seconds]   -> one JSON line per B"""
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
    out = torch.empty_like(x)
    loudness_ms = median_ms(lambda: fe.loudness(x))
    ebu_ms = median_ms(lambda: fe.loudness_ebu(x))
    normalize_ms = median_ms(lambda: fe.loudness_normalize(x, target_lufs=-23.0, out=out))
    normalize_tp_ms = median_ms(lambda: fe.loudness_normalize(x, target_lufs=-23.0, out=out, true_peak_ceiling_dbtp=-1.0))
    kernels = stage_ms(lambda: fe.loudness_normalize(x, target_lufs=-23.0, out=out, true_peak_ceiling_dbtp=-1.0))
    st = fe.loudness_ebu(x).cpu().numpy()
    fma = B * (L + 12) * 11 * 24
    res = {"metric": "EBU-mode ms per call (median of %d)" % K, "seconds": secs, "batch": B, "samples": L,
           "true_peak_dbtp_row0": round(float(20 * np.log10(st[0, 8])), 3), "lra_row0": round(float(st[0, 10]), 3),
           "loudness_ms_parent_call": round(loudness_ms, 4), "ebu_ms": round(ebu_ms, 4), "normalize_ms_parent_call": round(normalize_ms, 4),
           "normalize_tp_ms": round(normalize_tp_ms, 4), "kernel_ms_normalize_tp": kernels,
           "true_peak_gfma_per_s": round(1e-9 * fma / (kernels["ebu_true_peak"] * 1e-3), 1)}
    if B == 1:
        import ebu_ref
        t0 = time.perf_counter()
        tp, m = ebu_ref.true_peak(wav[0], SR), ebu_ref.short_term(wav[0], SR)
        res["numpy_restatement_ms_one_clip"] = round(1e3 * (time.perf_counter() - t0), 1)
        res["restatement_minus_device_true_peak"] = float(tp - st[0, 8])
        res["restatement_minus_device_lra_lu"] = float(m["lra"] - st[0, 10])
    print(json.dumps(res), flush=True)
