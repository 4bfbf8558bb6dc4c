"""De-reverberation by weighted prediction error (MelFrontEnd.dereverb, csrc/wpe.hip) on the GPU, next to the denoiser on the same clip:
a prompt of `seconds` of gated white-noise bursts with one echo at 4 hops, alone and in a batch of 32.
dereverb_ms is the whole call with the figures (reflect padding, one STFT GEMM per utterance, the two transpositions, the bins, the
figures, the inverse GEMM, the overlap-add); stage_ms the call between its own stage events (dr_stft | dr_wpe | dr_istft); denoise_ms
and denoise_stage_ms the same for MelFrontEnd.denoise on the same input, for scale.  Three warm-up calls, then K calls between device
events: the median, the least and the largest.
usage: python tools/bench_dereverb.py [seconds]   -> one JSON line per B"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd.runtime import MelFrontEnd

secs = float(sys.argv[1]) if len(sys.argv) > 1 else 30.0
K = 20
fe = MelFrontEnd()


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


for B in (1, 32):
    L = int(secs * 16000)
    rng = np.random.default_rng(0)
    x = np.zeros((B, L), np.float32)
    at = 0
    while at < L:                                                              # bursts of 40 - 200 ms, silent gaps of 20 - 120 ms
        n = int(rng.uniform(0.04, 0.2) * 16000)
        x[:, at:at + n] = (rng.uniform(0.05, 0.3) * rng.standard_normal((B, min(n, L - at)))).astype(np.float32)
        at += n + int(rng.uniform(0.02, 0.12) * 16000)
    x[:, 1024:] += 0.5 * x[:, :-1024].copy()
    X = torch.from_numpy(x).cuda()
    out = torch.empty(B, 256 * (L // 256), device="cuda", dtype=torch.float32)
    dr = lambda: fe.dereverb(X, None, return_figures=True, out=out)           # noqa: E731
    dn = lambda: fe.denoise(X, None, return_figures=True, out=out)            # noqa: E731
    dereverb_ms, denoise_ms = timed(dr), timed(dn)
    stage_ms, dn_stage_ms = stages(dr), stages(dn)
    fig = fe.dereverb(X, None, return_figures=True, out=out)[2][0].cpu().numpy()
    print(json.dumps({"metric": "dereverb ms per call (median, least, largest of %d)" % K, "seconds": secs, "batch": B, "frames": 1 + L // 256,
                      "reduction_db": round(float(fig[2]), 3), "bins_filtered": int(fig[4]), "dereverb_ms": dereverb_ms, "stage_ms": stage_ms,
                      "denoise_ms": denoise_ms, "denoise_stage_ms": dn_stage_ms,
                      "wpe_share": round(stage_ms["dr_wpe"] / sum(stage_ms.values()), 4)}), flush=True)
