"""Row f3 measurement: the prompt-audio silence trimmer (MelFrontEnd.trim, csrc/trim.hip) on the GPU, next to the resampler's and the
mel front-end's time for the same clips.  The clip is 44.1 kHz noise-floor + speech-like burst audio; the trimmer sees its 16 kHz
resampled, normalised form.  trim_ms is the whole call (four kernels, the copy of the bounds to the host and the wait for it).
Bytes: the audio is read twice (block sums, copy) and written once - 4 * B * (2 L + Lout_max); GB/s = those bytes over trim_ms.
usage: python tools/bench_trim.py [seconds]   -> one JSON line per B"""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from megatts2_amd.runtime import MelFrontEnd

secs = float(sys.argv[1]) if len(sys.argv) > 1 else 30.0
K = 20
SR_IN = 44100
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


for B in (1, 8):
    L = int(secs * SR_IN)
    rng = np.random.default_rng(0)
    wav = 1e-3 * rng.standard_normal((B, L))
    wav[:, L // 6:L - L // 6] += 0.1 * rng.standard_normal((B, L - 2 * (L // 6)))          # a sixth of "room tone" at either end
    x = torch.from_numpy(wav.astype(np.float32)).cuda()
    y, y_lens = fe.resample(x, SR_IN, normalize=True)
    Lo = y.shape[1]
    rs_out = torch.empty_like(y)
    resample_ms = median_ms(lambda: fe.resample(x, SR_IN, normalize=True, out=rs_out))
    out = torch.empty_like(y)
    trim_ms = median_ms(lambda: fe.trim(y, y_lens, 40.0, out=out))
    cut, cut_lens, bounds = fe.trim(y, y_lens, 40.0, out=out)
    mel_ms = median_ms(lambda: fe(y, y_lens))
    mel_cut_ms = median_ms(lambda: fe(cut, cut_lens))
    gbytes = 4e-9 * B * (2 * Lo + Lo)
    print(json.dumps({"metric": "trim ms per call (median of %d)" % K, "seconds": secs, "batch": B, "samples_16k": Lo,
                      "kept_samples": int(cut_lens[0]), "trim_ms": round(trim_ms, 4), "gbytes": round(gbytes, 5),
                      "gb_per_s": round(gbytes / (trim_ms * 1e-3), 1), "resample_normalize_ms_same_clip": round(resample_ms, 4),
                      "mel_frontend_ms_same_clip": round(mel_ms, 4), "mel_frontend_ms_trimmed_clip": round(mel_cut_ms, 4)}), flush=True)
