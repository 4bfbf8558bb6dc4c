"""Row f3 measurement: the prompt-audio resampler (MelFrontEnd.resample, csrc/resample.hip) on the GPU, next to the mel front-end's
time for the same clip and the host's scipy.signal.resample_poly (what audio_io.load_audio(resample=True) runs; a different filter).
usage: python tools/bench_resample.py [seconds]   -> one JSON line per (sr_in, B)"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd.runtime import MelFrontEnd, resample_query

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


for sr_in in (44100, 48000):
    L = int(secs * sr_in)
    Lo, o, n, taps = resample_query(sr_in, 16000, L)
    for B in (1, 8):
        wav = (0.1 * np.random.default_rng(0).standard_normal((B, L))).astype(np.float32)
        x = torch.from_numpy(wav).cuda()
        out = torch.empty(B, Lo, device="cuda")
        raw_ms = median_ms(lambda: fe.resample(x, sr_in, out=out))
        norm_ms = median_ms(lambda: fe.resample(x, sr_in, normalize=True, out=out))
        y = out.clone()
        mel_ms = median_ms(lambda: fe(y))
        try:
            from scipy.signal import resample_poly
            t0 = time.perf_counter(); resample_poly(wav[0], n, o); host_ms = (time.perf_counter() - t0) * 1e3
        except ImportError:
            host_ms = None
        print(json.dumps({"metric": "resample ms per launch (median of %d)" % K, "sr_in": sr_in, "seconds": secs, "batch": B, "o": o, "n": n,
                          "taps": taps, "resample_ms": round(raw_ms, 4), "resample_normalize_ms": round(norm_ms, 4),
                          "mel_frontend_ms_same_clip": round(mel_ms, 4), "gflop": round(2e-9 * B * Lo * taps, 3),
                          "tflops": round(2e-9 * B * Lo * taps / raw_ms, 3),
                          "host_resample_poly_ms_one_utt": None if host_ms is None else round(host_ms, 2)}), flush=True)
