"""Declipping by sparsity (MelFrontEnd.declip, csrc/declip.hip) on the GPU, next to the denoiser and the de-reverberation on the same clip:
a prompt of `seconds` of the declipping tests' signal (12 harmonics of a wobbling 150 Hz fundamental, 3 Hz amplitude modulation, a
little noise) at 16 kHz, clipped at 0.5 of its peak, alone and in a batch of 32.
declip_ms is the whole call with figures and iteration counts; stage_ms the call between its own stage events (dc_detect | dc_frames |
dc_overlap | dc_figures); detect_ms is MelFrontEnd.clip_detect alone; denoise_ms and dereverb_ms the two neighbouring stages on the same
input, for scale.  fft_per_s is the frame kernel's achieved rate against its own arithmetic count: two real FFTs of N points an
iteration, the iterations summed over `iters`, over the dc_frames stage time; gflops the same with 2.5 N log2 N flops a real FFT.
Three warm-up calls, then K calls between device events: the median, the least and the largest.
usage: python tools/bench_declip.py [seconds]   -> one JSON line per B"""
import json, math, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd.runtime import Declip, MelFrontEnd

secs = float(sys.argv[1]) if len(sys.argv) > 1 else 30.0
K = 20
SR = 16000
fe = MelFrontEnd()


def signal(n, seed):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / SR
    phase = 2.0 * np.pi * np.cumsum(150.0 * (1.0 + 0.1 * np.sin(2.0 * np.pi * 1.5 * t))) / SR
    x = np.zeros(n)
    for h in range(1, 13):
        x += 0.7 ** h * np.sin(h * phase + rng.uniform(0.0, 2.0 * np.pi))
    x *= 1.0 + 0.4 * np.sin(2.0 * np.pi * 3.0 * t)
    x += 0.003 * rng.standard_normal(n)
    return np.clip(x / np.abs(x).max(), -0.5, 0.5).astype(np.float32)


def timed(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return [round(float(v), 4) for v in (np.median(ms), min(ms), max(ms))]


def stages(fn):
    fe.set_profiling(True)
    rows = []
    for _ in range(K):
        fn()
        rows.append(fe.last_stage_ms())
    fe.set_profiling(False)
    return {k: round(float(np.median([r[k] for r in rows])), 4) for k in rows[0]}


cfg = Declip()
N = cfg.frame
for B in (1, 32):
    L = int(secs * SR)
    x = np.stack([signal(L, b) for b in range(B)])
    X = torch.from_numpy(x).cuda()
    out = torch.empty_like(X)
    out16 = torch.empty(B, 256 * (L // 256), device="cuda", dtype=torch.float32)
    dc = lambda: fe.declip(X, None, cfg, return_figures=True, return_iters=True, out=out)      # noqa: E731
    dt = lambda: fe.clip_detect(X, None, cfg)                                                  # noqa: E731
    dn = lambda: fe.denoise(X, None, return_figures=True, out=out16)                           # noqa: E731
    dr = lambda: fe.dereverb(X, None, return_figures=True, out=out16)                          # noqa: E731
    declip_ms, detect_ms, denoise_ms, dereverb_ms = timed(dc), timed(dt), timed(dn), timed(dr)
    stage_ms = stages(dc)
    _, fig, it = dc()
    fig, it = fig.cpu().numpy(), it.cpu().numpy()
    ffts = 2 * int(it.sum())
    frames_s = stage_ms["dc_frames"] * 1e-3
    print(json.dumps({"metric": "declip ms per call (median, least, largest of %d)" % K, "seconds": secs, "batch": B, "frame": N,
                      "frames": int(cfg.frames(L)), "frames_iterated": int(fig[:, 4].sum()), "mean_iterations": round(float(fig[:, 5].mean()), 1),
                      "max_iterations": int(fig[:, 6].max()), "share_clipped": round(float(fig[:, 3].mean()), 4),
                      "power_change_db": round(float(fig[:, 7].mean()), 3), "declip_ms": declip_ms, "stage_ms": stage_ms, "detect_ms": detect_ms,
                      "denoise_ms": denoise_ms, "dereverb_ms": dereverb_ms, "real_ffts": ffts, "fft_per_s": round(ffts / frames_s, 1),
                      "gflops": round(ffts * 2.5 * N * math.log2(N) / frames_s * 1e-9, 2)}), flush=True)
