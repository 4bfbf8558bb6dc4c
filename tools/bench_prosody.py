"""Row f5 measurement: the per-phone prosody layer (csrc/prosody.hip) on the GPU - MelFrontEnd.energy, .phone_prosody and
.pitch_contour, and the whole megatts2.pitch_distance (two contours, one copy of the counts to the host, the DTW at D = 1) - next to
MelFrontEnd.f0 (YIN) and the mel front-end on the same clips.  The clips are bench_f0.py's vibrato harmonic stacks at 16 kHz with
pauses; the alignment gives about 400 phones to 30 s.  Every figure is the whole call between device events, median of 20 after 3
warm-up calls; pitch_distance_ms is wall time around the call (it waits for the device itself).  The numpy restatement
(tests/prosody_ref.py) is timed once for one clip on the host.
usage: python tools/bench_prosody.py [seconds]   -> one JSON line per B"""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch
import f0_ref as R
import prosody_ref as P
from megatts2_amd import megatts2 as M
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


def wall_ms(fn):
    for _ in range(3):
        fn()
    ms = []
    for _ in range(K):
        torch.cuda.synchronize()
        t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
        ms.append((time.perf_counter() - t0) * 1e3)
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
T = 1 + L // fe.audio.hop_length
Np = max(1, round(400 * secs / 30.0))
rng = np.random.default_rng(7)
cuts = np.sort(rng.integers(0, T + 1, Np - 1))
dur = np.diff(np.concatenate([[0], cuts, [T]])).astype(np.int32)                          # Np durations summing to T, zeros among them

for B in (1, 8):
    x = torch.from_numpy(np.stack(rows[:B])).cuda()
    d = torch.from_numpy(np.tile(dur, (B, 1))).cuda()
    f0 = fe.f0(x)
    en = fe.energy(x)
    out = torch.empty_like(en)
    energy_ms = median_ms(lambda: fe.energy(x, out=out))
    phones_ms = median_ms(lambda: fe.phone_prosody(f0, d, en))
    contour_ms = median_ms(lambda: fe.pitch_contour(f0))
    other = torch.roll(f0, 1, 0) if B > 1 else torch.flip(f0, (1,))
    dist_ms = wall_ms(lambda: M.pitch_distance(f0, other))
    dist = M.pitch_distance(f0, other)
    st, nv = fe.pitch_contour(f0)
    k, nvh = int(nv.max()), nv.cpu().numpy()
    X = st[:, :k].unsqueeze(2).contiguous()
    dtw_ms = median_ms(lambda: fe.dtw(X, X, nvh, nvh)) if B == 1 else None
    f0_ms = median_ms(lambda: fe.f0(x))
    mel_ms = median_ms(lambda: fe(x))
    line = {"metric": "prosody ms per call (median of %d)" % K, "seconds": secs, "batch": B, "frames": T, "phones": Np,
            "energy_ms": round(energy_ms, 4), "phone_prosody_ms": round(phones_ms, 4), "pitch_contour_ms": round(contour_ms, 4),
            "pitch_distance_ms": round(dist_ms, 4), "voiced_frames": int(nv[0]), "rms_semitones": round(float(dist["rms_semitones"][0]), 4),
            "f0_yin_ms_same_clip": round(f0_ms, 4), "mel_frontend_ms_same_clip": round(mel_ms, 4)}
    if B == 1:
        line["dtw_d1_ms_of_that"] = round(dtw_ms, 4)
        f0h, enh = f0[0].cpu().numpy(), en[0].cpu().numpy()
        t0 = time.perf_counter(); ref_e = P.energy32(rows[0]); t1 = time.perf_counter()
        ref_p = P.phone_prosody(f0h, dur, enh)[0]; t2 = time.perf_counter()
        ref_c = P.contour(f0h)[0]; t3 = time.perf_counter()
        line["host_restatement_ms_one_clip"] = {"energy": round((t1 - t0) * 1e3, 1), "phone_prosody": round((t2 - t1) * 1e3, 1),
                                                "pitch_contour": round((t3 - t2) * 1e3, 2)}
        line["energy_bits_equal_restatement"] = bool(np.array_equal(enh.view(np.uint32), ref_e.view(np.uint32)))
        got = fe.phone_prosody(f0, d, en).cpu().numpy()[0]
        line["phone_frames_equal_restatement"] = bool(np.array_equal(got[:, 1], ref_p[:, 1]))
    print(json.dumps(line), flush=True)
