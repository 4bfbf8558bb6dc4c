"""Row f4 measurement: the second F0 tracker (MelFrontEnd.f0_track, csrc/f0.hip: a Viterbi pass over YIN's lag costs) on the GPU, next to
the plain YIN call and the mel front-end on the same clips (bench_f0.py's: a vibrato harmonic stack at 16 kHz with pauses).
track_ms is the whole call between device events (one upload, two launches), median of 20 after 3 warm-up calls; cmnd_ms and
viterbi_ms are its two kernels between the call's own stage events (mt2_set_profiling: d' of every frame to scratch; recurrence,
backtrack and refinement by one workgroup per utterance), medians of 20 profiled calls.  terms: n^2 predecessor terms a frame, n = 225
states.  The numpy restatement (tests/f0_track_ref.py, float32) is timed once for one clip on the host, and its lag path compared.
usage: python tools/bench_f0_track.py [seconds]   -> one JSON line per B"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import f0_ref as R
import f0_track_ref as V
from megatts2_amd.runtime import MelFrontEnd, f0_track_query

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


def stage_medians(fn):
    fe.set_profiling(True)
    rows = []
    for _ in range(K):
        fn()
        rows.append(fe.last_stage_ms())
    fe.set_profiling(False)
    return {k: float(np.median([r[k] for r in rows])) for k in rows[0]}


L = int(secs * R.SR)
n = np.arange(L, dtype=np.float64)
rows = []
for b in range(8):
    f = (110.0 + 20.0 * b) * (1.0 + 0.03 * np.sin(2 * np.pi * 5.0 * n / R.SR))          # 5 Hz vibrato of +- 3 %
    ph = 2 * np.pi * np.cumsum(f) / R.SR
    x = sum(h * np.sin((k + 1) * ph) for k, h in enumerate((1.0, 0.5, 0.33, 0.25)))
    gate = (np.sin(2 * np.pi * 0.7 * n / R.SR + b) > -0.3).astype(np.float64)           # pauses: some frames are unvoiced
    rows.append((0.3 * x * gate + 1e-3 * np.random.default_rng(b).standard_normal(L)).astype(np.float32))

for B in (1, 8):
    x = torch.from_numpy(np.stack(rows[:B])).cuda()
    T, lo, hi, states, ws = f0_track_query(L, B, hop=fe.audio.hop_length)
    out = torch.empty(B, T, device="cuda", dtype=torch.float32)
    track_ms = median_ms(lambda: fe.f0_track(x, out=out))
    st = stage_medians(lambda: fe.f0_track(x, out=out))
    yin_ms = median_ms(lambda: fe.f0(x, out=out))
    mel_ms = median_ms(lambda: fe(x))
    rec = {"metric": "f0_track ms per call (median of %d)" % K, "seconds": secs, "batch": B, "frames": T, "states": states,
           "track_ms": round(track_ms, 4), "cmnd_ms": round(st["f0_cmnd"], 4), "viterbi_ms": round(st["f0_viterbi"], 4),
           "yin_ms_same_clip": round(yin_ms, 4), "mel_frontend_ms_same_clip": round(mel_ms, 4),
           "viterbi_us_per_frame": round(1e3 * st["f0_viterbi"] / T, 3), "gterms": round(1e-9 * B * T * states * states, 3),
           "workspace_mib": round(ws / 2 ** 20, 2)}
    if B == 1:
        f0, lag, d = fe.f0_track(x, return_lag=True, return_diff=True)
        t0 = time.perf_counter()
        ref = V.track(d[0].cpu().numpy(), dtype=np.float32)
        rec["host_restatement_ms_one_clip"] = round((time.perf_counter() - t0) * 1e3, 1)
        rec["lags_equal_restatement"] = bool(np.array_equal(lag[0].cpu().numpy(), ref[2]))
        stats = fe.f0_stats(f0).cpu().numpy()
        rec.update(voiced_fraction=round(float(stats[0, 1]), 4), mean_hz=round(float(stats[0, 2]), 2), std_hz=round(float(stats[0, 3]), 2))
    print(json.dumps(rec), flush=True)
