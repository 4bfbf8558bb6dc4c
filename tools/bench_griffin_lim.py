"""Griffin-Lim vocoder measurement (MelFrontEnd.griffin_lim, csrc/griffinlim.hip) on the GPU: production audio configuration,
n_iter = 32, momentum 0.99, T = 431 (the C3 prompt) at B = 1, 8, 32 and T = 1875 (30 s) at B = 1, 8.  The mel is the front-end's
own mel of a vibrato harmonic stack.  gl_ms: the whole call between device events, median of 20.  iter_ms: the handle's stage event
around the 32 iterations over 32 (set_profiling: the call then waits for its last event), median of 20 calls - four launches an
iteration.  hifigan_ms: mt2_hifigan on the same mel with the synthetic production weights, median of 5.  host_f32_ms: the
restatement's f32 run (tests/griffinlim_ref.py, numpy, one utterance) by the host clock, once.  gemm_gflop: 2 * 2 * rows * 1024 *
1028 per iteration pair of GEMMs, times 33 inverse and 32 forward transforms.
usage: python tools/bench_griffin_lim.py [--no-host]   -> one JSON line per (T, B)"""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
from megatts2_amd import config as C, weights  # noqa: E402
from megatts2_amd.runtime import MelFrontEnd, NativeModel, griffin_lim_query  # noqa: E402

K, K_VOC, N_ITER = 20, 5, 32
h = C.production_hifigan()
voc = NativeModel(hg_cfg=h, sd_hifigan=weights.synth_state_dict(weights.inventory_hifigan(h), 0, "hifigan."))
fe = MelFrontEnd()
a = fe.audio


def median_ms(fn, k):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(k):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def vibrato(L):
    t = np.arange(L) / a.sample_rate
    ph = 2 * np.pi * 180.0 * t + 6.0 * np.sin(2 * np.pi * 5.5 * t)
    x = sum(np.sin(k * ph) / k for k in range(1, 13))
    return (x / np.abs(x).max()).astype(np.float32)


for T, Bs in ((431, (1, 8, 32)), (1875, (1, 8))):
    x = vibrato((T - 1) * a.hop_length)
    host_ms = None
    if "--no-host" not in sys.argv:
        import griffinlim_ref as G
        M = G.log_mel(x, a)
        t0 = time.perf_counter()
        G.griffin_lim(M, 0, a, N_ITER, 0.99, np.float32)
        host_ms = (time.perf_counter() - t0) * 1e3
    for B in Bs:
        mel = fe(torch.from_numpy(np.tile(x, (B, 1))).cuda())
        assert mel.shape == (B, T, a.n_mels)
        out = torch.empty(B, (T - 1) * a.hop_length, device="cuda", dtype=torch.float32)
        gl = lambda: fe.griffin_lim(mel, n_iter=N_ITER, out=out)      # noqa: E731
        gl_ms = median_ms(gl, K)
        fe.set_profiling(True)
        stages = {"gl_setup": [], "gl_iterations": [], "gl_final": []}
        for _ in range(K):
            gl()
            for k, v in fe.last_stage_ms().items():
                stages[k].append(v)
        fe.set_profiling(False)
        med = {k: float(np.median(v)) for k, v in stages.items()}
        mel_cf = mel.transpose(1, 2).contiguous()
        hifigan_ms = median_ms(lambda: voc.hifigan(mel_cf), K_VOC)
        rows = B * T
        gflop = 2.0 * rows * 1024 * 1028 * (2 * N_ITER + 1) / 1e9
        print(json.dumps({"metric": "griffin_lim ms per call (median of %d)" % K, "T": T, "batch": B, "n_iter": N_ITER,
                          "gl_ms": round(gl_ms, 3), "setup_ms": round(med["gl_setup"], 3), "iterations_ms": round(med["gl_iterations"], 3),
                          "iter_ms": round(med["gl_iterations"] / N_ITER, 4), "final_ms": round(med["gl_final"], 3),
                          "gemm_gflop": round(gflop, 1), "gemm_tflops_over_call": round(gflop / gl_ms, 2),
                          "audio_s": round(B * (T - 1) * a.hop_length / a.sample_rate, 2), "hifigan_ms_same_mel": round(hifigan_ms, 3),
                          "host_f32_restatement_ms_one_utterance": None if host_ms is None else round(host_ms, 1),
                          "workspace_mib": round(griffin_lim_query(a, None, T_max=T, B=B, n_iter=N_ITER)[0] / 2 ** 20, 1)}), flush=True)
