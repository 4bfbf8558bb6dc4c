"""Stationary-noise suppression (MelFrontEnd.denoise, csrc/denoise.hip) on the GPU, next to the two transforms it sits between: a
prompt of `seconds` of white noise under a tone gated on for alternate half-seconds, alone and in a batch of 32.
denoise_ms is the whole call (reflect padding, one STFT GEMM per utterance, power, select, gain with the figures, the inverse GEMM,
the overlap-add); stft_istft_ms the existing pair mt2_stft + mt2_istft on the same input - the yardstick; floor_ms and gain_ms the
two public halves as calls of their own on the spectrum (each with its own power pass); stage_ms the call between its own stage
events (dn_stft | dn_floor: power + select | dn_gain: gain + figures | dn_istft); new_kernels_share = (dn_floor + dn_gain) / the sum of
the four stages.
usage: python tools/bench_denoise.py [seconds]   -> one JSON line per B"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd.runtime import MelFrontEnd

secs = float(sys.argv[1]) if len(sys.argv) > 1 else 30.0
K = 20
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


for B in (1, 32):
    L = int(secs * 16000)
    rng = np.random.default_rng(0)
    t = np.arange(L) / 16000.0
    x = (0.05 * rng.standard_normal((B, L)) + 0.224 * np.sin(2 * np.pi * 440.0 * t) * ((np.floor(t / 0.5) % 2) == 1)).astype(np.float32)
    X = torch.from_numpy(x).cuda()
    out = torch.empty(B, 256 * (L // 256), device="cuda", dtype=torch.float32)
    denoise_ms = median_ms(lambda: fe.denoise(X, None, return_figures=True, out=out))
    S = (2 * 513 + 3) & ~3
    T = 1 + L // 256
    spec = torch.empty(B, T, S, device="cuda", dtype=torch.float32)

    def pair():      # the existing calls, on the library's own layout: no packing on the way
        import ctypes as C
        from megatts2_amd import runtime as rt
        ln, tl = np.full(B, L, np.int32), np.full(B, T, np.int32)
        rt._check(fe.lib.mt2_stft(fe.h, rt._stream(), C.byref(fe.ac), rt._ptr(X), rt._iptr(ln), L, B, rt._ptr(spec), T))
        rt._check(fe.lib.mt2_istft(fe.h, rt._stream(), C.byref(fe.ac), rt._ptr(spec), rt._iptr(tl), T, B, rt._ptr(out), out.shape[1]))

    pair_ms = median_ms(pair)
    floor = fe.noise_floor(spec)
    floor_ms = median_ms(lambda: fe.noise_floor(spec))
    gain_ms = median_ms(lambda: fe.spectral_gain(spec, floor, return_gain=False, apply=True, in_place=True))
    pair()
    fe.set_profiling(True)
    stages = []
    for _ in range(K):
        fe.denoise(X, None, return_figures=True, out=out)
        stages.append(fe.last_stage_ms())
    fe.set_profiling(False)
    stage_ms = {k: round(float(np.median([s[k] for s in stages])), 4) for k in stages[0]}
    fig = fe.denoise(X, None, return_figures=True, out=out)[2][0].cpu().numpy()
    own = stage_ms["dn_floor"] + stage_ms["dn_gain"]
    print(json.dumps({"metric": "denoise ms per call (median of %d)" % K, "seconds": secs, "batch": B, "frames": T,
                      "snr_db": round(float(fig[1]), 3), "reduction_db": round(float(fig[3]), 3), "denoise_ms": round(denoise_ms, 4),
                      "stft_istft_ms": round(pair_ms, 4), "floor_ms": round(floor_ms, 4), "gain_ms": round(gain_ms, 4), "stage_ms": stage_ms,
                      "new_kernels_share": round(own / sum(stage_ms.values()), 4),
                      "new_kernels_over_the_two_gemm_stages": round(own / (stage_ms["dn_stft"] + stage_ms["dn_istft"]), 4)}), flush=True)
