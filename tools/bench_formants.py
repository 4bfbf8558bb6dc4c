"""Formant-row measurement: the formant candidates by linear prediction (MelFrontEnd.formants, csrc/formants.hip) on the GPU, alone
and through megatts2.extract_formants (the resampler to 11 kHz in front), next to extract_f0's time for the same clips as the yardstick.
The clips are 16 kHz: 110 - 220 Hz pulse trains through four resonators, a new vowel every 0.3 s, over a noise floor.  formants_ms is
the handle call on audio already at 11 kHz, between two device events: ONE launch (a wave per frame: order-10 autocorrelation of a
550-sample Hann frame, Levinson-Durbin, Aberth-Ehrlich roots, candidates), the call only enqueues.  extract_ms adds the resampler's launch
and the host work of the Python layer; stats_ms is mt2_formant_stats on the tracks; f0_ms is extract_f0 (YIN) on the 16 kHz clip.
Arithmetic, not bandwidth: a frame reads 2.2 KB and runs about 7 iterations of 10 roots x 10 complex divisions.
usage: python tools/bench_formants.py   -> one JSON line per case: 30 s clips at B = 1 and 32"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd import megatts2 as M
from megatts2_amd.runtime import Formants

K = 20
SR = 16000
fe = M._frontend()
VOWELS = ((730, 1090, 2440, 3400), (270, 2290, 3010, 3700), (300, 870, 2240, 3300), (530, 1840, 2480, 3500), (660, 1720, 2410, 3600))


def vowel_response(formants, n=2048):
    """the impulse response of the four cascaded two-pole resonators of a vowel at SR (down 100 dB within n samples)"""
    h = np.zeros(n)
    h[0] = 1.0
    for F, bw in zip(formants, (80, 90, 120, 150)):
        rho, th = np.exp(-np.pi * bw / SR), 2 * np.pi * F / SR
        c1, c2, y1, y2 = 2 * rho * np.cos(th), -rho * rho, 0.0, 0.0
        for i in range(n):
            y1, y2 = h[i] + c1 * y1 + c2 * y2, y1
            h[i] = y1
    return h


def clip(B, secs, seed=0):
    rng = np.random.default_rng(seed)
    L = int(secs * SR)
    wav = np.zeros((B, L))
    seg = int(0.3 * SR)
    resp = [vowel_response(v) for v in VOWELS]
    for b in range(B):
        src = np.zeros(L)
        at = 0
        while at < L:                             # one pitch per vowel
            period, end = int(SR / rng.uniform(110.0, 220.0)), min(L, (at // seg + 1) * seg)
            while at < end:
                src[at] = 1.0
                at += period
        y = np.zeros(L + 2048)
        for s0 in range(0, L, seg):               # a vowel per segment, its pulses ringing on into the next
            x = np.convolve(src[s0:s0 + seg], resp[int(rng.integers(len(VOWELS)))])
            y[s0:s0 + x.size] += x
        wav[b] = y[:L] / np.abs(y[:L]).max() * 0.5 + 1e-3 * rng.standard_normal(L)
    return torch.from_numpy(wav.astype(np.float32)).cuda()


def timed_ms(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(K):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(); fn(); e1.record(); torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return {"median": round(float(np.median(ms)), 4), "least": round(float(np.min(ms)), 4), "largest": round(float(np.max(ms)), 4)}


for B, secs in ((1, 30.0), (32, 30.0)):
    y = clip(B, secs)
    cfg = Formants()
    x, xl = fe.resample(y, SR, None, sr_out=cfg.rate())
    res = fe.formants(x, xl, cfg, hop=176, sample_rate=cfg.rate(), return_iters=True)
    f0 = M.extract_f0(y)
    T = min(f0.shape[1], res["count"].shape[1])
    st = fe.formant_stats(res["freq"][:, :T], res["count"][:, :T], f0[:, :T]).cpu().numpy()
    it = res["iters"].cpu().numpy()
    alone = timed_ms(lambda: fe.formants(x, xl, cfg, hop=176, sample_rate=cfg.rate()))
    whole = timed_ms(lambda: M.extract_formants(y))
    stats = timed_ms(lambda: fe.formant_stats(res["freq"], res["count"]))
    pitch = timed_ms(lambda: M.extract_f0(y))
    frames = int(res["count"].shape[1])
    print(json.dumps({"metric": "formants ms per call (%d timed calls, 3 warm-up)" % K, "seconds": secs, "batch": B, "samples_11k": int(x.shape[1]),
                      "frames": frames, "empty_frames": int((it < 0).sum()), "mean_iterations": round(float(it[it > 0].mean()), 2),
                      "max_iterations": int(it.max()), "first_row": {"voiced_frames_used": int(st[0, 0]), "f1_f4_hz": [round(float(v), 1) for v in st[0, 2:6]],
                                                                      "vtl_cm": round(float(st[0, 11]), 2)},
                      "formants_ms": alone, "extract_ms": whole, "stats_ms": stats, "f0_ms_same_clip": pitch,
                      "frames_per_ms": round(B * frames / alone["median"], 1)}), flush=True)
