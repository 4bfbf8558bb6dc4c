"""Formant-track measurement: the Viterbi pass over the formant candidates (MelFrontEnd.formant_track, csrc/formant_track.hip) on the
GPU, next to the time of the candidates themselves (MelFrontEnd.formants, mt2_lpc_formants) on the same clips as the yardstick.
The clips are made as those of tools/bench_formants.py: 16 kHz, 110 - 220 Hz pulse trains through four resonators, a new vowel every 0.3 s,
over a noise floor; analysed at 11 kHz on the mel's frames.  track_ms is the handle call on candidates already on the device, between
two device events: ONE launch, a workgroup of one wave per utterance, so a single clip is latency, not throughput - the chain is T
steps long - and a batch runs its clips side by side.  lpc_ms is the candidates' call on the resampled audio; stats_ms is
mt2_formant_stats on the tracks.  Nobody has measured this kernel before and the parent has no tracker: the figures record what it is.
usage: python tools/bench_formant_track.py   -> one JSON line per case: a 30 s clip (1876 frames), 32 of them, a 5-minute clip
(18 751 frames) and a 10-minute clip (37 501 frames)"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd import megatts2 as M
from megatts2_amd.runtime import Formants, FormantTrack

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


RESP = [vowel_response(v) for v in VOWELS]


def clip(B, secs, seed=0):
    rng = np.random.default_rng(seed)
    L = int(secs * SR)
    wav = np.zeros((B, L), np.float32)
    seg = int(0.3 * SR)
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
            resp = RESP[int(rng.integers(len(VOWELS)))]
            for p0 in s0 + np.flatnonzero(src[s0:s0 + seg]):      # the convolution, pulse by pulse: a 10-minute clip in seconds
                y[p0:p0 + resp.size] += resp
        wav[b] = y[:L] / np.abs(y[:L]).max() * 0.5 + 1e-3 * rng.standard_normal(L)
    return torch.from_numpy(wav).cuda()


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


for B, secs in ((1, 30.0), (32, 30.0), (1, 300.0), (1, 600.0)):
    y = clip(B, secs)
    cfg, trk = Formants(), FormantTrack()
    x, xl = fe.resample(y, SR, None, sr_out=cfg.rate())
    T = 1 + y.shape[1] // 256                     # the mel's frames
    res = fe.formants(x, xl, cfg, hop=176, sample_rate=cfg.rate())
    freq, bw, count = (res[k][:, :T].contiguous() for k in ("freq", "bw", "count"))
    out = fe.formant_track(freq, bw, count, None, trk)
    on = out["track_count"] > 0
    moved = ((out["sel"][..., :4] != torch.arange(4, device="cuda", dtype=torch.int32)).any(-1) & on).sum()
    raw, st = fe.formant_stats(freq, count).cpu().numpy(), fe.formant_stats(out["track_freq"], out["track_count"]).cpu().numpy()
    track = timed_ms(lambda: fe.formant_track(freq, bw, count, None, trk))
    lpc = timed_ms(lambda: fe.formants(x, xl, cfg, hop=176, sample_rate=cfg.rate()))
    stats = timed_ms(lambda: fe.formant_stats(out["track_freq"], out["track_count"]))
    print(json.dumps({"metric": "formant_track ms per call (%d timed calls, 3 warm-up)" % K, "seconds": secs, "batch": B, "frames": T, "tracks": trk.tracks,
                      "tracked_frames": int(on.sum()), "gap_frames": int(B * T - on.sum()), "share_not_the_first_four": round(float(moved) / max(int(on.sum()), 1), 4),
                      "first_row": {"f1_f4_hz_tracked": [round(float(v), 1) for v in st[0, 2:6]], "f1_f4_hz_first_four": [round(float(v), 1) for v in raw[0, 2:6]],
                                    "vtl_cm_tracked": round(float(st[0, 11]), 2), "vtl_cm_first_four": round(float(raw[0, 11]), 2)},
                      "track_ms": track, "lpc_formants_ms_same_clip": lpc, "stats_ms": stats,
                      "track_us_per_frame_of_the_longest_row": round(1000.0 * track["median"] / T, 4)}), flush=True)
