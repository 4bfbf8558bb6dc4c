"""Row f3 measurement: the F0 tracker (MelFrontEnd.f0, csrc/f0.hip) and the pitch moments (MelFrontEnd.f0_stats) on the GPU, next to the
mel front-end's time for the same clips.  The clip is a vibrato harmonic stack at 16 kHz.  f0_ms is the whole call between device
events (the length upload and one launch of one workgroup per frame), median of 20 after 3 warm-up calls; f0_diff_ms the same call
writing the difference function [B, T, 257] as well; stats_ms the moments call.  fma: 257 lags x 768 terms a frame.  The numpy
restatement (tests/f0_ref.py, float64 d, float32 steps behind it) is timed once for one clip on the host.
usage: python tools/bench_f0.py [seconds]   -> one JSON line per B"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import f0_ref as R
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


L = int(secs * R.SR)
n = np.arange(L, dtype=np.float64)
rows = []
for b in range(8):
    f = (110.0 + 20.0 * b) * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * n / R.SR))          # 5 Hz vibrato of +- 3 %
    ph = 2 * np.pi * np.cumsum(f) / R.SR
    x = sum(h * np.sin((k + 1) * ph) for k, h in enumerate((1.0, 0.5, 0.33, 0.25)))
    gate = (np.sin(2 * np.pi * 0.7 * n / R.SR + b) > -0.3).astype(np.float64)           # pauses: some frames are unvoiced
    rows.append((0.3 * x * gate + 1e-3 * np.random.default_rng(b).standard_normal(L)).astype(np.float32))
t0 = time.perf_counter()
ref = R.yin(rows[0], dtype=np.float32)
host_ms = (time.perf_counter() - t0) * 1e3

for B in (1, 8):
    x = torch.from_numpy(np.stack(rows[:B])).cuda()
    T = 1 + L // fe.audio.hop_length
    out = torch.empty(B, T, device="cuda", dtype=torch.float32)
    f0_ms = median_ms(lambda: fe.f0(x, out=out))
    f0_diff_ms = median_ms(lambda: fe.f0(x, out=out, return_diff=True))
    f0 = fe.f0(x, out=out)
    stats_ms = median_ms(lambda: fe.f0_stats(f0))
    mel_ms = median_ms(lambda: fe(x))
    st = fe.f0_stats(f0).cpu().numpy()
    agree = float(np.mean((f0[0].cpu().numpy() > 0) == (ref[0] > 0)))
    gfma = 1e-9 * B * T * (R.MAX_LAG + 1) * R.WINDOW
    print(json.dumps({"metric": "f0 ms per call (median of %d)" % K, "seconds": secs, "batch": B, "frames": T, "f0_ms": round(f0_ms, 4),
                      "f0_with_diff_ms": round(f0_diff_ms, 4), "stats_ms": round(stats_ms, 4), "gfma": round(gfma, 3),
                      "gfma_per_s": round(gfma / (f0_ms * 1e-3), 1), "mel_frontend_ms_same_clip": round(mel_ms, 4),
                      "host_restatement_ms_one_clip": round(host_ms, 1), "voicing_agrees_with_restatement": round(agree, 4),
                      "voiced_fraction": round(float(st[0, 1]), 4), "mean_hz": round(float(st[0, 2]), 2), "std_hz": round(float(st[0, 3]), 2)}),
          flush=True)
