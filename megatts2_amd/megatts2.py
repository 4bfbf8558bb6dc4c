"""Drop-in mirror of the reference's `models/megatts2.py` object surface on the MI355X HIP engine.

Same class / method names, argument order and tensor layouts as the reference
(`MegaG`, `MegaPLM`, `MegaADM`, `Megatts`, `LengthRegulator`), so that
`infer.py`-style code switches with an import change.  Every numeric method
forwards to libmegatts2_hip through `runtime.NativeModel`; nothing here computes with torch ops.

Extensions over the reference (which is batch-1, CPU): every method takes optional per-utterance
length arguments and treats each utterance as an independent batch-1 run; `Megatts.synthesize`
runs a whole batch with activations resident in HBM between stages.
"""
from __future__ import annotations

import glob
import os
import warnings
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import config as cfgmod
from . import weights
from .config import HIFIGAN_HOP_LENGTH, HIFIGAN_SR
from .runtime import DECLIP_NAMES, DENOISE_NAMES, PAUSES_NAMES, WPE_NAMES, Declip, Denoise, Dereverb, Limiter, NativeError, NativeModel, Pauses  # noqa: F401  (Limiter, Denoise, Dereverb, Declip, Pauses: arguments of synthesize / forward)
from .runtime import FORMANT_STAT_NAMES, Formants, FormantTrack, resample_query
from .sampling import PLMSampling, seed_array


def _np_sd(sd) -> Dict[str, np.ndarray]:
    return {k: (v.detach().cpu().numpy() if hasattr(v, "detach") else np.asarray(v)) for k, v in sd.items()}


_FRONTEND = None


def _frontend():
    global _FRONTEND
    if _FRONTEND is None:
        from .runtime import MelFrontEnd
        _FRONTEND = MelFrontEnd()
    return _FRONTEND


def extract_mel_spec(samples, sample_rate: Optional[int] = None, trim_db: Optional[float] = None, denoise: Optional[Denoise] = None,
                     dereverb: Optional[Dereverb] = None, declip: Optional[Declip] = None, cut_pauses: Optional[Pauses] = None):
    """reference modules/tokenizer.py:107-125: 1-D waveform tensor (16 kHz) -> mel [80, T] (the reference
    returns channels first and `Megatts.forward` transposes it, models/megatts2.py:339).  Runs on the GPU
    (runtime.MelFrontEnd); a [B, L] input gives [B, 80, T].  sample_rate: the rate of `samples` when it is not
    16 kHz - they are resampled on the GPU first (MelFrontEnd.resample, not normalised).  trim_db: leading and
    trailing silence is cut off first (MelFrontEnd.trim, `librosa.effects.trim(y, top_db=trim_db)` of :337; a batch
    is cut per row, T follows the longest row and the frames behind a shorter row's own are zero).  denoise (None = off, exactly
    the call without it): a `Denoise`; stationary noise is suppressed behind the resampling and in front of the trim
    (MelFrontEnd.denoise, csrc/denoise.hip; the level is left as it comes out, up to hop - 1 tail samples are dropped).  dereverb (None
    = off, exactly the call without it): a `Dereverb`; late reverberation is removed by weighted prediction error behind the resampling
    and in front of the denoiser (MelFrontEnd.dereverb, csrc/wpe.hip; likewise).  declip (None = off, exactly the call without it): a
    `Declip`; clipped samples are restored first of all, at the samples' own rate and in front of the resampling, which would turn
    the flat tops into ripple (MelFrontEnd.declip, csrc/declip.hip; the level is left as it comes out and can exceed the input's).
    cut_pauses (None = off, exactly the call without it): a `Pauses`; where the trim would run, the pauses inside the audio are cut out
    as well as its ends (MelFrontEnd.cut_pauses, csrc/segments.hip), so it excludes trim_db (ValueError)."""
    import torch
    if cut_pauses is not None and trim_db is not None:
        raise ValueError("cut_pauses cuts the ends itself: it excludes trim_db")
    fe = _frontend()
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    batched = x.dim() == 2
    x = (x if batched else x.unsqueeze(0)).to("cuda", torch.float32)
    if declip is not None:
        x = fe.declip(x, None, declip)
    if sample_rate is not None and int(sample_rate) != fe.audio.sample_rate:
        x = fe.resample(x, int(sample_rate))[0]
    lens = None
    if dereverb is not None:
        x, lens = fe.dereverb(x, None, dereverb)
    if denoise is not None:
        x, lens = fe.denoise(x, lens, denoise)
    if trim_db is not None:
        x, lens, _ = fe.trim(x, lens, top_db=trim_db)
    if cut_pauses is not None:
        x, lens = fe.cut_pauses(x, lens, cut_pauses)
    mel = fe(x, lens).transpose(1, 2)
    return mel if batched else mel[0]


def extract_f0(samples, sample_rate: Optional[int] = None, trim_db: Optional[float] = None, method: str = "yin", **yin):
    """F0 track of a 1-D waveform (16 kHz) -> f0 [T] in Hz, 0 where a frame is unvoiced: YIN on the GPU by the rule of csrc/f0.hip
    (MelFrontEnd.f0; no reference counterpart, parity with librosa.yin / pyin and quality on real speech unpinned).  sample_rate and
    trim_db are extract_mel_spec's, applied first in the same way, so f0[t] belongs to mel frame t of the same call; a [B, L] input
    gives [B, T].  **yin: MelFrontEnd.f0's arguments (fmin, fmax, threshold, hop, return_cmnd, return_lag, return_diff); with an
    extra asked for the result is MelFrontEnd.f0's tuple.  method="viterbi": the second tracker (MelFrontEnd.f0_track, a Viterbi
    pass over YIN's lag costs that cures its octave-high frames), which also takes octave_cost and jump_cost."""
    import torch
    if method not in ("yin", "viterbi"):
        raise ValueError("method must be 'yin' or 'viterbi'")
    fe = _frontend()
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    batched = x.dim() == 2
    x = (x if batched else x.unsqueeze(0)).to("cuda", torch.float32)
    if sample_rate is not None and int(sample_rate) != fe.audio.sample_rate:
        x = fe.resample(x, int(sample_rate))[0]
    lens = None
    if trim_db is not None:
        x, lens, _ = fe.trim(x, top_db=trim_db)
    res = (fe.f0 if method == "yin" else fe.f0_track)(x, lens, **yin)
    if batched:
        return res
    return tuple(r[0] for r in res) if isinstance(res, tuple) else res[0]


PITCH_STATS = ("voiced_frames", "voiced_fraction", "mean_hz", "std_hz", "skewness", "kurtosis")


def pitch_stats(f0, frame_lens=None) -> Dict[str, np.ndarray]:
    """The per-utterance pitch moments by which prosody transfer is usually reported, over the voiced frames (f0 > 0) among the
    first frame_lens[b] of f0 [T] or [B, T] (MelFrontEnd.f0_stats: double sums on the GPU) -> dict of float64 numpy arrays [B]
    ([1] for a 1-D track): voiced_frames, voiced_fraction, mean_hz, std_hz, skewness, kurtosis (excess).  Without a voiced frame
    every entry is 0."""
    import torch
    x = f0 if hasattr(f0, "is_cuda") else torch.as_tensor(np.asarray(f0, np.float32))
    x = (x if x.dim() == 2 else x.unsqueeze(0)).to("cuda", torch.float32)
    st = _frontend().f0_stats(x, frame_lens).cpu().numpy()
    return {k: st[:, i].copy() for i, k in enumerate(PITCH_STATS)}


def extract_formants(samples, sample_rate: Optional[int] = None, lens=None, formants: Optional[Formants] = None,
                     track: Optional[FormantTrack] = None):
    """Formant candidates of a 1-D waveform (16 kHz, or at sample_rate) on the mel's frames: linear prediction on the GPU by the rule of
    csrc/formants.hip (MelFrontEnd.formants; no reference counterpart, parity with Praat's Burg fit and quality on real speech
    unpinned).  formants: a `Formants` (defaults: 5.5 kHz ceiling, order 10, 50 ms Hann, pre-emphasis from 50 Hz).  The audio is
    resampled on the GPU to 2 * max_formant_hz (11 kHz: MelFrontEnd.resample's rule) - not at all when that is its own rate - and
    analysed there with the hop hop_length * rate / 16000 (176), which must be a whole number of samples (ValueError otherwise, never
    rounded), so that frame t is centred where mel frame t of the same audio at 16 kHz is.  -> dict: "freq", "bw" f32 [T, 5] in Hz,
    "count" int32 [T] (device), T = 1 + L16 // hop_length for the L16 samples the audio has at 16 kHz - the mel's frame count, so
    freq[t], extract_f0's f0[t] and mel frame t coincide (the resampled audio can hold one frame more, which is dropped: the three tensors are then views of the wider rows, not
    contiguous); "frame_lens"
    (host int32 [B]), "rate", "hop".  A [B, L] input (lens: the rows' lengths) gives [B, T, ...]; frames behind a row's own are zeros.
    track: a `FormantTrack` adds "track_freq", "track_bw", "track_count" and "sel", `track_formants` of these candidates (ref_hz None at
    this call's max_formant_hz); None (the default) is the call of before, nothing tracked."""
    import torch
    fe = _frontend()
    cfg = formants or Formants()
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    batched = x.dim() == 2
    x = (x if batched else x.unsqueeze(0)).to("cuda", torch.float32)
    B, L = x.shape
    sr_in = fe.audio.sample_rate if sample_rate is None else int(sample_rate)
    ln = np.full(B, L, np.int32) if lens is None else np.asarray(lens, np.int32).reshape(-1)
    rate = cfg.rate()
    if (fe.audio.hop_length * rate) % fe.audio.sample_rate:
        raise ValueError(f"the mel's hop of {fe.audio.hop_length} samples at {fe.audio.sample_rate} Hz is not a whole number of samples at {rate} Hz: "
                         "choose max_formant_hz so that hop_length * 2 * max_formant_hz / 16000 is an integer (5500, 5000, 4000)")
    hop = fe.audio.hop_length * rate // fe.audio.sample_rate
    # the mel's frames: of the audio as it is at the mel's rate
    l16 = ln if sr_in == fe.audio.sample_rate else np.asarray([resample_query(sr_in, fe.audio.sample_rate, int(n))[0] for n in ln], np.int64)
    frame_lens = (1 + l16 // fe.audio.hop_length).astype(np.int32)
    if sr_in != rate:
        x, ln = fe.resample(x, sr_in, ln, sr_out=rate)
    T = int(frame_lens.max())
    # rows wide enough for both frame counts: the analysed audio can hold one frame more than the mel (L = 256 k - 1), and behind two
    # different resamplings one less, which then is an empty frame
    rows = max(T, 1 + int(np.max(ln)) // hop)
    res = fe.formants(x, ln, cfg, hop=hop, sample_rate=rate, out=torch.empty(B, rows, 5, device=x.device, dtype=torch.float32))
    out = {k: v[:, :T] for k, v in res.items()}
    if track is not None:
        out.update(fe.formant_track(out["freq"], out["bw"], out["count"], frame_lens, track, cfg.max_formant_hz))
    if not batched:
        out = {k: v[0] for k, v in out.items()}
    out.update(frame_lens=frame_lens, rate=rate, hop=hop)
    return out


def track_formants(freq, bw, count, frame_lens=None, track: Optional[FormantTrack] = None, max_formant_hz: float = 5500.0):
    """Formant tracks across frames of candidate rows freq, bw [T, 5] / [B, T, 5] and count [T] / [B, T] (extract_formants'): of every
    frame's candidates the `track.tracks` that form the cheapest smooth path through the utterance's first frame_lens[b] frames, by a
    Viterbi pass on the GPU (MelFrontEnd.formant_track; the rule is in include/megatts2_hip.h; parity with Praat's tracker and quality on
    real speech unpinned) -> dict of device tensors in the input's layout: "track_freq", "track_bw" f32 [.., T, 5] (track q in slot q,
    zeros behind), "track_count" int32 [.., T] (tracks, or 0 in a frame without that many sound candidates) and "sel" int32 [.., T, 5]
    (the candidate slot of every track, -1 behind).  formant_stats(track_freq, track_count) is the intended use: one spurious root no
    longer moves every formant above it.  track: a `FormantTrack` (None: its defaults; ref_hz None at max_formant_hz)."""
    import torch

    batched = (freq.dim() if hasattr(freq, "dim") else np.asarray(freq).ndim) == 3

    def dev(a, dims, dtype):
        t = a if hasattr(a, "is_cuda") else torch.as_tensor(np.asarray(a))
        return (t if t.dim() == dims else t.unsqueeze(0)).to("cuda", dtype).contiguous()
    out = _frontend().formant_track(dev(freq, 3, torch.float32), dev(bw, 3, torch.float32), dev(count, 2, torch.int32), frame_lens, track,
                                    max_formant_hz)
    return out if batched else {k: v[0] for k, v in out.items()}


def formant_stats(freq, count, f0=None, frame_lens=None) -> Dict[str, np.ndarray]:
    """The per-utterance formant figures of candidate tracks freq [T, 5] / [B, T, 5] and count [T] / [B, T] (extract_formants') over
    the frames with at least four candidates among the first frame_lens[b] - the voiced ones (f0 > 0) where an F0 track of the same
    frames is given (MelFrontEnd.formant_stats: double sums on the GPU) -> dict of float64 numpy arrays [B] (FORMANT_STAT_NAMES): frames,
    share, f1 .. f4 (means, Hz), f1_sigma .. f4_sigma, dispersion ((f4 - f1) / 3, Hz), vtl_cm (the length of a uniform tube closed at
    one end with these means; 17.5 for 500 / 1500 / 2500 / 3500 Hz).  Without such a frame every entry is 0.  Two voices compare by
    the ratio of their vtl_cm, whatever the text."""
    import torch

    def dev(a, dims, dtype):
        if a is None:
            return None
        t = a if hasattr(a, "is_cuda") else torch.as_tensor(np.asarray(a))
        return (t if t.dim() == dims else t.unsqueeze(0)).to("cuda", dtype).contiguous()
    st = _frontend().formant_stats(dev(freq, 3, torch.float32), dev(count, 2, torch.int32), dev(f0, 2, torch.float32), frame_lens).cpu().numpy()
    return {k: st[:, i].copy() for i, k in enumerate(FORMANT_STAT_NAMES)}


def extract_energy(samples, sample_rate: Optional[int] = None, trim_db: Optional[float] = None, **kw):
    """Energy contour of a 1-D waveform (16 kHz) -> f32 [T]: the mean square of the 1024 samples around each mel frame, on the GPU
    by the rule of csrc/prosody.hip (MelFrontEnd.energy; no reference counterpart, parity with librosa's rms unpinned).  sample_rate
    and trim_db are extract_f0's, applied first in exactly the same way, so energy[t], f0[t] and mel frame t of one call coincide; a
    [B, L] input gives [B, T].  **kw: MelFrontEnd.energy's hop and out."""
    import torch
    fe = _frontend()
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    batched = x.dim() == 2
    x = (x if batched else x.unsqueeze(0)).to("cuda", torch.float32)
    if sample_rate is not None and int(sample_rate) != fe.audio.sample_rate:
        x = fe.resample(x, int(sample_rate))[0]
    lens = None
    if trim_db is not None:
        x, lens, _ = fe.trim(x, top_db=trim_db)
    res = fe.energy(x, lens, **kw)
    return res if batched else res[0]


LOUDNESS_STATS = ("integrated_lufs", "blocks", "blocks_over_absolute_gate", "blocks_over_both_gates", "relative_gate_lufs", "sample_peak",
                  "max_momentary_lufs", "gain")


EBU_STATS = ("true_peak", "oversampling", "lra", "short_term_blocks", "short_term_blocks_over_absolute_gate",
             "short_term_blocks_over_both_gates", "lra_relative_gate_lufs", "lra_p10_lufs", "lra_p95_lufs", "short_term_max")


def measure_loudness(samples, sample_rate: Optional[int] = None, lens=None, ebu: bool = False) -> Dict[str, np.ndarray]:
    """Integrated loudness (ITU-R BS.1770-4, gated - the measure EBU R 128 builds on) of a 1-D waveform or a [B, L] batch, on the GPU
    by the rule of csrc/loudness.hip (MelFrontEnd.loudness; no reference counterpart, parity with pyloudnorm / libebur128 unpinned;
    true peak and loudness range with ebu=True) -> dict of float64 numpy arrays [B] ([1] for a 1-D waveform): integrated_lufs (-inf
    under 0.4 s or for silence), blocks, blocks_over_absolute_gate, blocks_over_both_gates, relative_gate_lufs, sample_peak (linear),
    max_momentary_lufs, gain (1).  sample_rate: the rate of `samples` (default 16 kHz), a multiple of 10 in [8000, 192000] - the
    audio is measured at its own rate, nothing is resampled.  lens: the real samples of each row.
    ebu (False = exactly the call above): the rest of an EBU-mode meter (EBU R 128 / Tech 3341; MelFrontEnd.loudness_ebu, csrc/ebu.hip)
    is added to the dict, the first eight entries keeping their bits: true_peak (linear, oversampled to at least 192 kHz),
    true_peak_dbtp, oversampling, lra (loudness range in LU by EBU Tech 3342; NaN under 3 s or for silence), short_term_blocks
    (3 s every 100 ms), short_term_blocks_over_absolute_gate, short_term_blocks_over_both_gates, lra_relative_gate_lufs,
    lra_p10_lufs, lra_p95_lufs, short_term_max."""
    import torch
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    x = (x if x.dim() == 2 else x.unsqueeze(0)).to("cuda", torch.float32)
    if ebu:
        st = _frontend().loudness_ebu(x, lens, sample_rate=sample_rate).cpu().numpy()
        res = {k: st[:, i].copy() for i, k in enumerate(LOUDNESS_STATS + EBU_STATS)}
        with np.errstate(divide="ignore"):
            res["true_peak_dbtp"] = 20.0 * np.log10(res["true_peak"])
        return res
    st = _frontend().loudness(x, lens, sample_rate=sample_rate).cpu().numpy()
    return {k: st[:, i].copy() for i, k in enumerate(LOUDNESS_STATS)}


def denoise_audio(samples, sample_rate: Optional[int] = None, lens=None, denoise: Optional[Denoise] = None, noise=None):
    """Stationary-noise suppression of a 1-D waveform or a [B, L] batch on the GPU, by the rule of csrc/denoise.hip (MelFrontEnd.denoise;
    no reference counterpart; parity with noisereduce / RNNoise / Audacity and audible quality on real speech unpinned): a per-bin
    noise floor - the `percentile`-th percentile of the power over time, turned into a mean - and a spectral gate between the STFT and
    its inverse.  A steady tone is stationary and is removed like hum; speech present in a bin for more than 100 - percentile % of
    the frames raises that bin's floor.  sample_rate: the rate of `samples` when it is not 16 kHz - they are resampled on the GPU first
    (not normalised), and the result is at 16 kHz.  lens: the real samples of each row.  denoise: a `Denoise` (None: its defaults).
    noise: a noise-only clip (1-D, or [B, L'] - one per row - at the same rate as `samples`) whose floor is used instead of each
    utterance's own.  -> (out float32 numpy [B, hop * (L // hop)] ([.] for a 1-D waveform), dict: out_lens int32 [B], floor float32
    [B, 513] and float64 [B] noise_db, snr_db, floored_share, reduction_db, frames, rank, mean_frame_power, noise_power)."""
    import torch
    fe = _frontend()
    dn = denoise or Denoise()

    def at_rate(a, ln):
        a = a if hasattr(a, "is_cuda") else torch.as_tensor(np.asarray(a, np.float32))
        a = (a.unsqueeze(0) if a.dim() == 1 else a).to("cuda", torch.float32)
        if sample_rate is not None and int(sample_rate) != fe.audio.sample_rate:
            return fe.resample(a, int(sample_rate), ln)
        return a, ln

    flat = (samples.dim() if hasattr(samples, "dim") else np.asarray(samples).ndim) == 1
    x, ln = at_rate(samples, lens)
    floor = None
    if noise is not None:
        nz, nl = at_rate(noise, None)
        floor = fe.noise_floor(fe.stft(nz, nl), None if nl is None else 1 + np.asarray(nl) // fe.audio.hop_length, dn)
        if floor.shape[0] == 1 and x.shape[0] > 1:
            floor = floor.expand(x.shape[0], -1)
    out, out_lens, used, fig = fe.denoise(x, ln, dn, noise_floor=floor, return_floor=True, return_figures=True)
    fig = fig.cpu().numpy()
    res = {k: fig[:, i].copy() for i, k in enumerate(DENOISE_NAMES)}
    res["out_lens"], res["floor"] = out_lens, used.cpu().numpy()
    out = out.cpu().numpy()
    return (out[0] if flat else out), res


def dereverb_audio(samples, sample_rate: Optional[int] = None, lens=None, dereverb: Optional[Dereverb] = None):
    """De-reverberation of a 1-D waveform or a [B, L] batch on the GPU by weighted prediction error, the rule of csrc/wpe.hip
    (MelFrontEnd.dereverb; no reference counterpart; parity with nara_wpe and audible quality on real speech unpinned): per bin a
    prediction filter estimated from the recording itself removes what is predictable from the frames at least `delay` back.  Discrete
    reflections go, diffuse tails are helped only modestly, and a steady tone is removed like a reflection.  sample_rate: the rate of
    `samples` when it is not 16 kHz - they are resampled on the GPU first (not normalised), and the result is at 16 kHz.  lens: the real
    samples of each row.  dereverb: a `Dereverb` (None: its defaults).  -> (out float32 numpy [B, hop * (L // hop)] ([.] for a 1-D
    waveform), dict: out_lens int32 [B] and float64 [B] power_in, power_out, reduction_db, frames, bins_filtered, bins_passed, max_tap,
    iterations)."""
    import torch
    fe = _frontend()
    flat = (samples.dim() if hasattr(samples, "dim") else np.asarray(samples).ndim) == 1
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    x = (x.unsqueeze(0) if x.dim() == 1 else x).to("cuda", torch.float32)
    ln = lens
    if sample_rate is not None and int(sample_rate) != fe.audio.sample_rate:
        x, ln = fe.resample(x, int(sample_rate), ln)
    out, out_lens, fig = fe.dereverb(x, ln, dereverb or Dereverb(), return_figures=True)
    fig = fig.cpu().numpy()
    res = {k: fig[:, i].copy() for i, k in enumerate(WPE_NAMES)}
    res["out_lens"] = out_lens
    out = out.cpu().numpy()
    return (out[0] if flat else out), res


def detect_clipping(samples, lens=None, declip: Optional[Declip] = None):
    """Clipping of a 1-D waveform or a [B, L] batch, detected on the GPU by step 1 of the rule of csrc/declip.hip (MelFrontEnd.clip_detect):
    nothing is restored.  -> dict of float64 [B]: clipped (0 / 1), hi, lo, share (of the samples at the two levels)."""
    import torch
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    x = (x.unsqueeze(0) if x.dim() == 1 else x).to("cuda", torch.float32)
    fig = _frontend().clip_detect(x, lens, declip or Declip()).cpu().numpy()
    return {k: fig[:, i].copy() for i, k in enumerate(DECLIP_NAMES[:4])}


def declip_audio(samples, lens=None, declip: Optional[Declip] = None):
    """Declipping of a 1-D waveform or a [B, L] batch on the GPU by sparsity, the rule of csrc/declip.hip (MelFrontEnd.declip, A-SPADE;
    no reference counterpart; parity with any outside declipper and audible quality on real speech unpinned).  The samples are taken at
    their OWN rate - nothing is resampled, because a resampler turns flat tops into ripple that is no longer recognised - so there is no
    sample_rate argument.  Samples within `tol` of the utterance's extremes count as clipped once there are enough of them; each frame
    that holds some is re-estimated as the signal of sparsest spectrum that keeps the reliable samples and lies beyond the level on the
    clipped ones.  An utterance that is not clipped comes back bit for bit; soft clipping is not detected; a steady full-scale tone
    reads as clipped.  The output can exceed the input's peak: normalise after.  lens: the real samples of each row.  declip: a
    `Declip` (None: its defaults).  -> (out float32 numpy [B, L] ([L] for a 1-D waveform), dict: iters int32 [B, T] and float64 [B]
    clipped, hi, lo, share, frames_iterated, mean_iterations, max_iterations, power_change_db)."""
    import torch
    fe = _frontend()
    flat = (samples.dim() if hasattr(samples, "dim") else np.asarray(samples).ndim) == 1
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    x = (x.unsqueeze(0) if x.dim() == 1 else x).to("cuda", torch.float32)
    out, fig, iters = fe.declip(x, lens, declip or Declip(), return_figures=True, return_iters=True)
    fig = fig.cpu().numpy()
    res = {k: fig[:, i].copy() for i, k in enumerate(DECLIP_NAMES)}
    res["iters"] = iters.cpu().numpy()
    out = out.cpu().numpy()
    return (out[0] if flat else out), res


def _pause_input(samples, sample_rate):
    import torch
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    flat = x.dim() == 1
    x = (x.unsqueeze(0) if flat else x).to("cuda", torch.float32)
    return x, flat, _frontend().audio.sample_rate if sample_rate is None else int(sample_rate)


def _segment_lists(seg, cnt):
    """ONE copy to the host: the segment table and the counts side by side -> per utterance [(start, end)]"""
    import torch
    B = seg.shape[0]
    t = torch.cat([seg.reshape(B, -1), cnt.reshape(B, 1)], dim=1).cpu().numpy()
    return [[(int(t[b, 2 * k]), int(t[b, 2 * k + 1])) for k in range(int(t[b, -1]))] for b in range(B)]


def speech_segments(samples, sample_rate: Optional[int] = None, lens=None, pauses: Optional[Pauses] = None):
    """The speech segments of a 1-D waveform or a [B, L] batch, found on the GPU by frame energy - the rule of csrc/segments.hip
    (MelFrontEnd.speech_segments; our own rule: parity with librosa.effects.split, webrtcvad or a model-based VAD and quality on real
    speech are unpinned).  The samples are taken at their OWN rate (sample_rate, default 16 kHz): nothing is resampled, and the
    durations of `pauses` (a `Pauses`; None: its defaults) become frames of 512 samples at that rate.  -> dict: segments, per utterance
    a list of (start, end) in samples, and float64 [B] for each of PAUSES_NAMES (segments negative: nothing was found and the utterance
    stayed whole)."""
    x, _, sr = _pause_input(samples, sample_rate)
    out = _frontend().speech_segments(x, lens, pauses, sample_rate=sr)
    fig = out["figures"].cpu().numpy()
    res = {k: fig[:, i].copy() for i, k in enumerate(PAUSES_NAMES)}
    res["n_segments"] = res.pop("segments")
    res["segments"] = _segment_lists(out["segments"], out["counts"])
    return res


def cut_pauses(samples, sample_rate: Optional[int] = None, lens=None, pauses: Optional[Pauses] = None, keep: str = "speech"):
    """A 1-D waveform or a [B, L] batch with its pauses cut out on the GPU (MelFrontEnd.cut_pauses, csrc/segments.hip), at the samples'
    own rate; keep="pauses" returns what is between the speech segments instead - a noise-only clip, e.g. for denoise_audio(noise=).
    Every kept sample is an exact copy; there is no cross-fade, and every join is a multiple of 512 samples.  -> (out float32 numpy
    [B, max out_lens] ([out_len] for a 1-D waveform), out_lens int32 [B], dict as `speech_segments`)."""
    x, flat, sr = _pause_input(samples, sample_rate)
    out, out_lens, seg, cnt, fig = _frontend().cut_pauses(x, lens, pauses, sample_rate=sr, keep=keep, return_segments=True, return_figures=True)
    fig = fig.cpu().numpy()
    res = {k: fig[:, i].copy() for i, k in enumerate(PAUSES_NAMES)}
    res["n_segments"] = res.pop("segments")
    res["segments"] = _segment_lists(seg, cnt)
    out = out[:, :max(int(out_lens.max()), 0)].cpu().numpy()
    return (out[0] if flat else out), out_lens, res


def split_on_pauses(samples, sample_rate: Optional[int] = None, lens=None, pauses: Optional[Pauses] = None):
    """A 1-D waveform or a [B, L] batch split at its pauses: per utterance a list of float32 numpy arrays, one per speech segment (the
    segments of `speech_segments`; one copy of the segment table to the host, the slices are taken from the host samples)."""
    x, flat, sr = _pause_input(samples, sample_rate)
    out = _frontend().speech_segments(x, lens, pauses, sample_rate=sr)
    segs = _segment_lists(out["segments"], out["counts"])
    host = (samples.detach().cpu().numpy() if hasattr(samples, "detach") else np.asarray(samples, np.float32)).reshape(x.shape)
    parts = [[host[b, s:e].copy() for s, e in segs[b]] for b in range(x.shape[0])]
    return parts[0] if flat else parts


LIMITER_STATS = ("half_window", "min_gain", "samples_limited", "true_peak_before_trim", "trim", "output_lufs")


def limit_true_peak(samples, sample_rate: Optional[int] = None, lens=None, pre_gain_db: float = 0.0, ceiling_dbtp: float = -1.0,
                    window_ms: float = 5.0):
    """True-peak look-ahead limiter on a 1-D waveform or a [B, L] batch, on the GPU by the rule of csrc/limiter.hip
    (MelFrontEnd.limit; offline and symmetric; parity with any outside limiter and audible quality on real speech unpinned): the audio
    is scaled by 10^(pre_gain_db / 20) and its crests are turned down by a smooth gain so that the true peak stays at or under
    ceiling_dbtp; audio further than 2 window_ms from any such crest keeps the plain gain exactly.  -> (out float32 numpy [B, L]
    ([L] for a 1-D waveform), dict of float64 numpy arrays [B]: measure_loudness(ebu=True)'s entries for the INPUT, with `gain` the
    linear pre-gain, and half_window (samples), min_gain, samples_limited, true_peak_before_trim, trim, output_lufs)."""
    import torch
    x = samples if hasattr(samples, "is_cuda") else torch.as_tensor(np.asarray(samples, np.float32))
    flat = x.dim() == 1
    x = (x.unsqueeze(0) if flat else x).to("cuda", torch.float32)
    out, st = _frontend().limit(x, lens, pre_gain_db, ceiling_dbtp, window_ms, sample_rate=sample_rate, return_stats=True)
    st = st.cpu().numpy()
    res = {k: st[:, i].copy() for i, k in enumerate(LOUDNESS_STATS + EBU_STATS + LIMITER_STATS)}
    out = out.cpu().numpy()
    return (out[0] if flat else out), res


PHONE_PROSODY = ("start", "frames", "voiced_frames", "mean_hz", "mean_semitones", "min_hz", "max_hz", "mean_energy")
DURATION_STATS = ("phones", "realised_fraction", "mean_frames", "std_frames", "skewness", "kurtosis")


def phone_prosody(f0, durations, energy=None, phone_lens=None, frame_lens=None, check_sum: bool = False) -> Dict[str, np.ndarray]:
    """Phone-level pitch and energy: the segment reduction of an F0 track f0 [T] or [B, T] over phone durations [Np] or [B, Np]
    (frames per phone: aux["dur"] of a synthesis call on the device, or a host alignment such as align_prompt's), on the GPU by
    the rule of csrc/prosody.hip (MelFrontEnd.phone_prosody) -> dict of float64 numpy arrays [B, Np]: start, frames,
    voiced_frames, mean_hz, mean_semitones (above 55 Hz), min_hz, max_hz (over the phone's voiced frames; 0 without one) and
    mean_energy (over all its frames; 0 without `energy`, a track of extract_energy).  Phone p owns the frames from the sum of the
    durations before it, clipped to frame_lens[b]; entries at or beyond phone_lens[b] are zeros.  check_sum: ValueError unless the
    durations of every row sum to its frame count exactly."""
    import torch

    def dev(a):
        a = a if hasattr(a, "is_cuda") else torch.as_tensor(np.asarray(a, np.float32))
        return (a if a.dim() == 2 else a.unsqueeze(0)).to("cuda", torch.float32)

    x = dev(f0)
    d = durations if hasattr(durations, "is_cuda") else torch.as_tensor(np.asarray(durations, np.int32))
    d = d if d.dim() == 2 else d.unsqueeze(0)
    fe = _frontend()
    out, total = fe.phone_prosody(x, d, None if energy is None else dev(energy), phone_lens, frame_lens, return_sum=True)
    if check_sum:
        want = fe._frame_lens(frame_lens, x.shape[0], x.shape[1])
        got = total.cpu().numpy()
        if not np.array_equal(got, want):
            raise ValueError(f"durations sum to {got.tolist()} frames, the tracks have {want.tolist()}")
    out = out.cpu().numpy()
    return {k: out[:, :, i].copy() for i, k in enumerate(PHONE_PROSODY)}


def duration_stats(durations, phone_lens=None) -> Dict[str, np.ndarray]:
    """The moments of phone duration by which rhythm is reported beside pitch_stats: over the realised phones (duration > 0) among
    the first phone_lens[b] of durations [Np] or [B, Np] (frames) -> dict of float64 numpy arrays [B]: phones, realised_fraction,
    mean_frames, std_frames, skewness, kurtosis (excess).  A composition, no kernel of its own: the durations as f32 (exact below
    2^24) go through MelFrontEnd.f0_stats, which already leaves zeros out and sums in double."""
    import torch
    d = durations if hasattr(durations, "is_cuda") else torch.as_tensor(np.asarray(durations, np.int32))
    d = (d if d.dim() == 2 else d.unsqueeze(0)).to("cuda", torch.float32)
    st = _frontend().f0_stats(d, phone_lens).cpu().numpy()
    return {k: st[:, i].copy() for i, k in enumerate(DURATION_STATS)}


def pitch_distance(f0_a, f0_b, lens_a=None, lens_b=None, center: bool = True) -> Dict[str, np.ndarray]:
    """The DTW distance between pitch contours: f0_a [Ta] or [B, Ta] and f0_b [Tb] or [B, Tb] -> dict of numpy arrays [B]:
    rms_semitones (float64) = sqrt(total / steps) of the warp of a's contour onto b's, steps, voiced_a, voiced_b (ints).  Each
    track's voiced frames are compacted to semitones (MelFrontEnd.pitch_contour), so unvoiced gaps do not count as pitch; center
    takes each contour's own mean off, which removes the speaker's register; the warp (MelFrontEnd.dtw with D = 1) removes the
    speaking rate.  One copy of the voiced counts to the host in between.  A pair where either side has no voiced frame gets NaN
    (steps 0) and is left out of the DTW call.  More than runtime.DTW_MAX_LEN = 4096 voiced frames on a side is the DTW's own
    refusal (NativeError), never clamped.  The rule is our own; no outside library's distance is matched."""
    import torch

    def dev(a):
        a = a if hasattr(a, "is_cuda") else torch.as_tensor(np.asarray(a, np.float32))
        return (a if a.dim() == 2 else a.unsqueeze(0)).to("cuda", torch.float32)

    fe = _frontend()
    xa, xb = dev(f0_a), dev(f0_b)
    B = xa.shape[0]
    assert xb.shape[0] == B
    sa, na = fe.pitch_contour(xa, lens_a, center=center)
    sb, nb = fe.pitch_contour(xb, lens_b, center=center)
    n = torch.stack([na, nb]).cpu().numpy()
    res = {"rms_semitones": np.full(B, np.nan), "steps": np.zeros(B, np.int64), "voiced_a": n[0].astype(np.int64),
           "voiced_b": n[1].astype(np.int64)}
    keep = np.nonzero((n[0] > 0) & (n[1] > 0))[0]
    if keep.size:
        rows = torch.as_tensor(keep, device=xa.device)
        ta, tb = int(n[0, keep].max()), int(n[1, keep].max())
        path = fe.dtw(sa[rows, :ta].unsqueeze(2), sb[rows, :tb].unsqueeze(2), n[0, keep], n[1, keep])
        steps = path["steps"].cpu().numpy().astype(np.int64)
        res["steps"][keep] = steps
        res["rms_semitones"][keep] = np.sqrt(path["total"].cpu().numpy().astype(np.float64) / steps)
    return res


def _mcd_dict(row) -> Dict[str, np.ndarray]:
    from .runtime import MCD_NAMES
    row = row.cpu().numpy()
    return {k: row[:, i].copy() for i, k in enumerate(MCD_NAMES)}


def mel_cepstral_distortion(mel_a, mel_b, lens_a=None, lens_b=None, f0_a=None, f0_b=None, order: int = 13) -> Dict[str, np.ndarray]:
    """Mel-cepstral distortion along the DTW path, on the GPU by the rule of csrc/mcd.hip (MelFrontEnd.mcd): mel_a [Ta, N] or
    [B, Ta, N] against mel_b [Tb, N] or [B, Tb, N], natural-log mels, TIME-major (extract_mel_spec(...).transpose(-1, -2)) -> dict of
    float64 numpy arrays [B]: cells (the path's length), mcd_db (the mean over the path of (10 / ln 10) sqrt(2 sum_k (c_k - c'_k)^2),
    k = 1 .. order; the level c0 is left out, so a gain change reads 0), max_db, and with F0 tracks f0_a [Ta] / f0_b [Tb] (Hz, 0 =
    unvoiced, frame-aligned to the mels as extract_f0 is to extract_mel_spec) along the SAME path: voiced_cells, f0_rmse_cents,
    f0_offset_cents (mean of 1200 log2(f0_a / f0_b): the register offset), vuv_cells and vuv_error (cells voiced on exactly one side,
    and their share).  The cepstrum is a DCT of the N-bin log-mel, not a mel-generalised cepstrum of a spectral envelope: the figures
    are comparable with themselves only, parity with SPTK / WORLD / ESPnet / Coqui MCD is unpinned."""
    import torch

    def dev(a, dims):
        a = a if hasattr(a, "is_cuda") else torch.as_tensor(np.asarray(a, np.float32))
        return (a if a.dim() == dims else a.unsqueeze(0)).to("cuda", torch.float32)

    fa = None if f0_a is None else dev(f0_a, 2)
    fb = None if f0_b is None else dev(f0_b, 2)
    return _mcd_dict(_frontend().mcd(dev(mel_a, 3), dev(mel_b, 3), lens_a, lens_b, fa, fb, order=order))


def compare_audio(wav_a, wav_b, sample_rate: Optional[int] = None, tracker: str = "yin", order: int = 13,
                  trim_db: Optional[float] = None) -> Dict[str, np.ndarray]:
    """The objective distance of two recordings of one sentence (1-D waveforms, e.g. generated audio and a reference recording):
    both are resampled from sample_rate (one rate, or a pair (rate_a, rate_b)) to 16 kHz where needed and optionally trimmed
    (trim_db), their mels and F0 tracks
    (tracker "yin" or "viterbi") are made by one front end, frame-aligned, and mel_cepstral_distortion compares a against b ->
    its dict (arrays [1])."""
    import torch
    if tracker not in ("yin", "viterbi"):
        raise ValueError("tracker must be 'yin' or 'viterbi'")
    fe = _frontend()
    mels, f0s = [], []
    rates = tuple(sample_rate) if isinstance(sample_rate, (tuple, list)) else (sample_rate, sample_rate)
    for w, sr in zip((wav_a, wav_b), rates):
        x = w if hasattr(w, "is_cuda") else torch.as_tensor(np.asarray(w, np.float32))
        assert x.dim() == 1, "compare_audio takes two 1-D waveforms"
        x = x.unsqueeze(0).to("cuda", torch.float32)
        if sr is not None and int(sr) != fe.audio.sample_rate:
            x = fe.resample(x, int(sr))[0]
        lens = None
        if trim_db is not None:
            x, lens, _ = fe.trim(x, top_db=trim_db)
        mel = fe(x, lens)
        f0 = (fe.f0 if tracker == "yin" else fe.f0_track)(x, lens)
        T = mel.shape[1] if lens is None else 1 + int(lens[0]) // fe.audio.hop_length
        mels.append(mel[:, :T])
        f0s.append(f0[:, :T])
    return _mcd_dict(fe.mcd(mels[0], mels[1], None, None, f0s[0], f0s[1], order=order))


class LengthRegulator:
    """reference modules/mrte.py:34-60 (FastSpeech length regulator) as a device gather."""

    def __init__(self, mel_frames, sample_rate, duration_token_ms, native: Optional[NativeModel] = None):
        assert (mel_frames / sample_rate * 1000 / duration_token_ms) == 1      # mrte.py:40
        self._native = native

    def bind(self, native: NativeModel) -> "LengthRegulator":
        self._native = native
        return self

    def __call__(self, x, duration_tokens, mel_max_length=None, lens=None):
        if self._native is None:
            raise NativeError("LengthRegulator is not bound to a native model")
        return self._native.length_regulate(x, duration_tokens, lens, mel_max_length)

    forward = __call__


class _MRTE:
    """reference modules/mrte.py:63-171 (the inference surface: `tc_latent`, `mel_encoder`)."""

    def __init__(self, owner: "MegaG"):
        self._o = owner
        self.hidden_size = owner.cfg.mrte.hidden_size
        self.mel_bins = owner.cfg.mrte.mel_bins

    def tc_latent(self, phone, *args, phone_lens=None, mel_lens=None):
        # the reference signature is (phone, mel) (mrte.py:154-158) but two of its own call sites pass
        # (phone, phone_lens, mel) (mrte.py:180, models/megatts2.py:83): accept both
        if len(args) == 1:
            mel = args[0]
        elif len(args) == 2:
            phone_lens, mel = args
        else:
            raise TypeError("tc_latent(phone, mel) or tc_latent(phone, phone_lens, mel)")
        return self._o.native.tc_latent(phone, mel, phone_lens, mel_lens)

    def mel_encoder(self, mel_bdt, mel_lens=None):
        """ConvNetDouble.forward on "B D T" input -> "B D T" (modules/convnet.py:202-210)."""
        return self._o.native.mel_context(mel_bdt.transpose(1, 2), mel_lens).transpose(1, 2)


class _RVQ:
    """reference modules/quantization/vq.py:100-113 (n_q = 1)."""

    def __init__(self, owner: "MegaG"):
        self._o = owner
        self.dimension = owner.cfg.vqpe.vq_dim
        self.n_q = 1
        self.bins = owner.cfg.vqpe.vq_bins

    def decode(self, codes):
        return self._o.native.vq_decode(codes)

    def encode(self, x, frame_rate=None, bandwidth=None):
        """x "b d n" -> codes [n_q, b, n] (EuclideanCodebook.encode, core_vq.py:192-200)."""
        b, d, n = x.shape
        idx = self._o.native.vq_quantize(x.transpose(1, 2).reshape(b * n, d))
        return idx.view(1, b, n)


class _VQPE:
    """reference modules/vqpe.py:13-62."""

    def __init__(self, owner: "MegaG"):
        self._o = owner
        self.stride = owner.cfg.vqpe.stride
        self.mel_bins = owner.cfg.vqpe.mel_bins
        self.vq = _RVQ(owner)

    def __call__(self, mel, lens=None):
        import torch
        zq, codes = self._o.native.vqpe_forward(mel, lens)
        zero = torch.zeros(1, 1, device=mel.device)       # losses are training-only (vqpe.py:57-58)
        return zq, zero, zero[0, 0], codes

    forward = __call__


class MegaG:
    """reference models/megatts2.py:30-117."""

    def __init__(self, cfg: cfgmod.GConfig, state_dict: Dict[str, np.ndarray], native: Optional[NativeModel] = None):
        self.cfg = cfg
        self.state = _np_sd(state_dict)
        weights.check_strict(self.state, weights.inventory_g(cfg))
        self._native = native
        self.mrte = _MRTE(self)
        self.vqpe = _VQPE(self)

    @property
    def native(self) -> NativeModel:
        if self._native is None:
            self._native = NativeModel(g_cfg=self.cfg, sd_g=self.state)
        return self._native

    def decoder(self, x, lens=None):
        """ConvNet.forward, "B D T" -> "B D T" (modules/convnet.py:115-119)."""
        return self.native.mel_decoder(x, lens)

    def s2_latent(self, phone, phone_lens, mel_mrte, mel_vqpe):
        """models/megatts2.py:75-84 (stage-2 latent extraction, prepare_ds.py:224-258)."""
        _, codes = self.native.vqpe_forward(mel_vqpe)
        return self.native.tc_latent(phone, mel_mrte, phone_lens), codes

    def extract_latent(self, path: str, phone, phone_lens, mel_mrte, mel_vqpe) -> None:
        """One item of `prepare_ds.py --stage 2` (prepare_ds.py:224-258): s2_latent of a batch-1 item saved as
        the reference's `{spk}/{id}.npy` pickle: {'tc_latent': [1, Np, 512] f32, 'p_code': [1, 1, Tq] int64}."""
        tc, codes = self.s2_latent(phone, phone_lens, mel_mrte, mel_vqpe)
        np.save(path, {"tc_latent": tc.cpu().numpy(), "p_code": codes.cpu().numpy()})

    def eval(self):
        return self

    def cuda(self):
        return self

    @classmethod
    def from_hparams(cls, config_path: str, seed: int = 0) -> "MegaG":
        """models/megatts2.py:87-104.  The reference returns randomly initialised modules; here the
        synthetic name-seeded weights are used."""
        cfg = cfgmod.g_config_from_yaml(config_path)
        return cls(cfg, weights.synth_state_dict(weights.inventory_g(cfg), seed, "G."))

    @classmethod
    def from_pretrained(cls, ckpt: str, config: str) -> "MegaG":
        cfg = cfgmod.g_config_from_yaml(config)
        return cls(cfg, weights.load_lightning_state_dict(ckpt, "G."))


class MegaPLM:
    """reference models/megatts2.py:120-198."""

    def __init__(self, cfg: cfgmod.PLMConfig, state_dict, native: Optional[NativeModel] = None):
        self.cfg = cfg
        self.state = _np_sd(state_dict)
        weights.check_strict(self.state, weights.inventory_plm(cfg))
        self._native = native

    @property
    def native(self) -> NativeModel:
        if self._native is None:
            self._native = NativeModel(plm_cfg=self.cfg, sd_plm=self.state)
        return self._native

    def infer(self, tc_latent, lens=None, prompt_tc_latent=None, prompt_codes=None, temperature=None, top_k: int = 0,
              top_p: float = 1.0, seed=None):
        """models/megatts2.py:165-181.  Optional prompt conditioning, in the layout the PLM is
        TRAINED on (modules/datamodule.py:201-212): `prompt_tc_latent` [B, P, tc] = the prompt utterance's
        length-regulated, max-pooled tc_latents, `prompt_codes` int64 [B, P] = its VQ-PE prosody codes
        (`generator.vqpe(prompt_mel)[3][0]`); both are put in front of the target's and decoding continues
        after them.  Returns the target's codes [B, Tq].
        `temperature` (None = the reference's greedy decoding): draw every code with temperature / top_k / top_p, seeded per
        utterance by `seed` (an int s - utterance b gets s + b - or one per utterance; sampling.PLMSampling)."""
        if (prompt_tc_latent is None) != (prompt_codes is None):
            raise ValueError("prompt_tc_latent and prompt_codes go together")
        kw = {}
        if temperature is not None:
            kw = dict(sampling=PLMSampling(temperature, top_k, top_p), seeds=seed)
        elif seed is not None or top_k or top_p != 1.0:
            raise ValueError("top_k / top_p / seed need a temperature (temperature=None is greedy decoding)")
        if prompt_codes is None:
            return self.native.plm_infer(tc_latent, lens, **kw)
        import torch
        if prompt_tc_latent.shape[1] != prompt_codes.shape[-1]:
            raise ValueError("prompt_tc_latent and prompt_codes must have the same length")   # datamodule.py:207 assert
        cond = torch.cat([prompt_tc_latent.to(tc_latent.device, torch.float32), tc_latent.to(torch.float32)], dim=1)
        return self.native.plm_infer(cond, lens, prefix_codes=prompt_codes.to(tc_latent.device), **kw)

    def infer_interpolated(self, tc_latent, prompt_a, prompt_b, gamma, lens=None, temperature=None, top_k: int = 0,
                           top_p: float = 1.0, seed=None):
        """Prosody interpolation (Mega-TTS 2, section 3.3): decode against two prosody prompts at once.  `prompt_a` / `prompt_b`
        are `(prompt_tc_latent [B, P, tc], prompt_codes int64 [B, P])` pairs as `infer` takes them, of one length P; at every step
        the two contexts' next-code distributions are mixed as (1 - gamma) * pA + gamma * pB (`gamma` one float or one per
        utterance in [0, 1]), and the code chosen on the mixture - greedy, or drawn with `temperature` / `top_k` / `top_p` /
        `seed` as in `infer` - is fed back to both.  Returns the target's codes [B, Tq]."""
        import torch
        kw = {}
        if temperature is not None:
            kw = dict(sampling=PLMSampling(temperature, top_k, top_p), seeds=seed)
        elif seed is not None or top_k or top_p != 1.0:
            raise ValueError("top_k / top_p / seed need a temperature (temperature=None is greedy decoding)")
        conds, prefixes = [], []
        for tc_p, codes_p in (prompt_a, prompt_b):
            if tc_p.shape[1] != codes_p.shape[-1]:
                raise ValueError("prompt_tc_latent and prompt_codes must have the same length")
            conds.append(torch.cat([tc_p.to(tc_latent.device, torch.float32), tc_latent.to(torch.float32)], dim=1))
            prefixes.append(codes_p.to(tc_latent.device))
        if conds[0].shape != conds[1].shape:
            raise ValueError("both prompts must have one pooled length P")
        return self.native.plm_infer_interpolated(conds[0], conds[1], lens, gamma, prefix_a=prefixes[0], prefix_b=prefixes[1], **kw)

    def eval(self):
        return self

    @classmethod
    def from_pretrained(cls, ckpt: str, config: str) -> "MegaPLM":
        return cls(cfgmod.plm_config_from_yaml(config), weights.load_lightning_state_dict(ckpt, "plm."))


class MegaADM:
    """reference models/megatts2.py:201-292."""

    def __init__(self, cfg: cfgmod.ADMConfig, state_dict, native: Optional[NativeModel] = None):
        self.cfg = cfg
        self.state = _np_sd(state_dict)
        weights.check_strict(self.state, weights.inventory_adm(cfg))
        self._native = native

    @property
    def native(self) -> NativeModel:
        if self._native is None:
            self._native = NativeModel(adm_cfg=self.cfg, sd_adm=self.state)
        return self._native

    def infer(self, tc_latents, lens=None):
        """-> int32 [B, Np, 1] like the reference (models/megatts2.py:275)."""
        return self.native.adm_infer(tc_latents, lens).unsqueeze(-1)

    def eval(self):
        return self

    @classmethod
    def from_pretrained(cls, ckpt: str, config: str) -> "MegaADM":
        return cls(cfgmod.adm_config_from_yaml(config), weights.load_lightning_state_dict(ckpt, "adm."))


class HIFIGAN:
    """`speechbrain.pretrained.HIFIGAN` (models/megatts2.py:25,321-323) on the HIP engine: HiFi-GAN V1 generator.

    `HIFIGAN.from_hparams(source=<local dir>)` reads a speechbrain model directory (`hyperparams.yaml` +
    `generator.ckpt`, weight norm folded at load); the hub name of the reference cannot be downloaded offline, so
    `source` must be a local copy (or `savedir` must already hold one).  A state dict named like
    transformers.SpeechT5HifiGan (weights.inventory_hifigan) is accepted by the constructor directly."""

    def __init__(self, cfg: cfgmod.HifiGanConfig, state_dict, native: Optional[NativeModel] = None):
        self.cfg = cfg
        self.state = _np_sd(state_dict)
        weights.check_strict(self.state, weights.inventory_hifigan(cfg))
        self._native = native

    @classmethod
    def from_hparams(cls, source: str, savedir: Optional[str] = None, run_opts=None, **_ignored) -> "HIFIGAN":
        """speechbrain's `Pretrained.from_hparams(source, savedir=...)`: `source` is a directory with the model files;
        when it is a hub id ("speechbrain/tts-hifigan-libritts-16kHz") the files must already be under `savedir`
        (default `pretrained_models/<name>`, where speechbrain caches them) or under $MEGATTS2_HIFIGAN_DIR."""
        cands = [source]
        if savedir:
            cands.append(savedir)
        if os.environ.get("MEGATTS2_HIFIGAN_DIR"):
            cands.append(os.environ["MEGATTS2_HIFIGAN_DIR"])
        cands.append(os.path.join("pretrained_models", os.path.basename(source.rstrip("/"))))
        # speechbrain's fetch() default cache: pretrained_models/<ClassName>-<md5(source)>
        import hashlib
        cands.append(os.path.join("pretrained_models", f"{cls.__name__}-{hashlib.md5(source.encode('UTF-8', errors='replace')).hexdigest()}"))
        for d in cands:
            if d and os.path.isfile(os.path.join(d, "hyperparams.yaml")):
                cfg, sd = weights.load_speechbrain_hifigan(d)
                return cls(cfg, sd)
        raise FileNotFoundError(f"HiFi-GAN model files (hyperparams.yaml, generator.ckpt) not found in any of {cands}: "
                                "there is no network here, place a local copy of the speechbrain model there")

    @property
    def native(self) -> NativeModel:
        if self._native is None:
            self._native = NativeModel(hg_cfg=self.cfg, sd_hifigan=self.state)
        return self._native

    def decode_batch(self, spectrogram, mel_lens=None, hop_len=None):
        """mel [B, 80, T] -> waveform [B, 1, hop * (T + 2 * inference_padding)] (speechbrain pads the mel by
        `inference_padding` replicated frames on both sides before the generator).  Every utterance is decoded as
        if alone (its own edge frames are replicated); samples beyond its length are zero - what speechbrain's
        `mask_noise` leaves when `mel_lens` and `hop_len` are given."""
        return self.native.hifigan(spectrogram, mel_lens)

    def eval(self):
        return self


class Megatts:
    """reference models/megatts2.py:295-375.  One native handle carries G + PLM + ADM (+ vocoder)."""

    def __init__(self, g_ckpt: str = None, g_config: str = None, plm_ckpt: str = None, plm_config: str = None,
                 adm_ckpt: str = None, adm_config: str = None, symbol_table: str = None, *,
                 models: Optional[tuple] = None, hifi_gan: Optional[HIFIGAN] = None,
                 hifigan_source: Optional[str] = "speechbrain/tts-hifigan-libritts-16kHz"):
        if models is not None:
            self.generator, self.plm, self.adm = models
        else:
            self.generator = MegaG.from_pretrained(g_ckpt, g_config)
            self.plm = MegaPLM.from_pretrained(plm_ckpt, plm_config)
            self.adm = MegaADM.from_pretrained(adm_ckpt, adm_config)
            if hifi_gan is None and hifigan_source:
                # :321-323  the reference ALWAYS builds the vocoder.  Offline the hub id resolves to a local copy
                # (savedir / $MEGATTS2_HIFIGAN_DIR / pretrained_models/<name>); without one there is no audio.
                try:
                    hifi_gan = HIFIGAN.from_hparams(source=hifigan_source)
                except FileNotFoundError as e:
                    warnings.warn(f"no vocoder: {e}")
        self.hifi_gan = hifi_gan
        self.native = NativeModel(self.generator.cfg, self.plm.cfg, self.adm.cfg,
                                  hifi_gan.cfg if hifi_gan else None, self.generator.state, self.plm.state,
                                  self.adm.state, hifi_gan.state if hifi_gan else None)
        for part in (self.generator, self.plm, self.adm) + ((hifi_gan,) if hifi_gan else ()):
            part._native = self.native
        self.lr = LengthRegulator(HIFIGAN_HOP_LENGTH, 16000, (HIFIGAN_HOP_LENGTH / HIFIGAN_SR * 1000), self.native)
        self.symbol_table = symbol_table
        self.tt = None                      # G2P (text -> phone symbols) is the reference's TextTokenizer, outside the path
        # :318  self.ttc = TokensCollector(symbol_table): native reader of the k2 symbol table (megatts2_amd/tokens.py)
        from .tokens import TokensCollector
        self.ttc = TokensCollector(symbol_table) if symbol_table else None
        if self.ttc is not None and self.ttc.vocab_size > self.generator.cfg.mrte.phone_vocab_size:
            warnings.warn(f"symbol table has {self.ttc.vocab_size} symbols, the phone embedding "
                          f"{self.generator.cfg.mrte.phone_vocab_size} rows")

    def eval(self):
        return self

    # -- batched tensor-level pipeline (the measured hot path)
    def synthesize(self, phone_tokens, mels, phone_lens=None, mel_lens=None, forced_durations=None,
                   forced_codes=None, vocoder: bool = False, return_aux: bool = False, sampling=None, seeds=None,
                   griffin_lim=None, loudness_lufs: Optional[float] = None, peak_ceiling: float = 0.0,
                   true_peak_ceiling_dbtp: Optional[float] = None, limiter=None):
        """phone_tokens int64 [B, Np], mels f32 [B, Tp, 80] -> (mel [B, Tm, 80], mel_lens) - the
        no_grad block of Megatts.forward (models/megatts2.py:353-368) for every utterance of the batch.
        `sampling` (sampling.PLMSampling; None = greedy) / `seeds` (int64 [B] or one int s -> s + b): sampled PLM codes.
        `griffin_lim` (None = off, exactly the call above; True or a dict of vocode_griffin_lim's keyword arguments): the generated
        mel is vocoded by Griffin-Lim instead of HiFi-GAN and the result is (mel, mel_lens, aux) with aux["wav"] f32
        [B, (max mel_lens - 1) * hop], utterance b holding (mel_lens[b] - 1) * hop samples - no inference padding, unlike
        decode_batch.
        `loudness_lufs` (None = off, exactly the call without it): aux["wav"] - HiFi-GAN's with vocoder=True and return_aux=True, or
        Griffin-Lim's - is brought to this integrated loudness per utterance over its real samples, in place on the device
        (MelFrontEnd.loudness_normalize; `peak_ceiling` > 0 caps the gain so that the sample peak stays under it; an utterance under
        0.4 s or silent keeps its level).  `true_peak_ceiling_dbtp` (None = off; needs loudness_lufs, excludes peak_ceiling > 0):
        the gain is capped so that the TRUE peak stays at or under this many dBTP (e.g. -1.0), which the sample-peak ceiling cannot
        promise - a 16 kHz signal has crests up to 3 dB over its samples.  `limiter` (None = off, exactly the call without it; a
        runtime.Limiter; needs true_peak_ceiling_dbtp): where that cap binds, one gain lands under loudness_lufs - with the
        limiter the crests alone are turned down (the look-ahead limiter of csrc/limiter.hip) and the audio reaches loudness_lufs
        under the same ceiling."""
        if true_peak_ceiling_dbtp is not None and loudness_lufs is None:
            raise ValueError("true_peak_ceiling_dbtp caps the gain of the loudness normalisation: it needs loudness_lufs")
        if limiter is not None and true_peak_ceiling_dbtp is None:
            raise ValueError("a limiter holds a true-peak ceiling: it needs true_peak_ceiling_dbtp (and loudness_lufs)")
        if loudness_lufs is not None:
            gl_on = not (griffin_lim is None or griffin_lim is False)
            if not gl_on and not (vocoder and return_aux):
                raise ValueError("loudness_lufs needs audio to normalise: vocoder=True with return_aux=True, or griffin_lim")
            mel, out_lens, aux = self.synthesize(phone_tokens, mels, phone_lens, mel_lens, forced_durations, forced_codes, vocoder,
                                                 True, sampling, seeds, griffin_lim)
            hg = self.native.hg_cfg
            n = np.asarray(out_lens, np.int64)
            n = (n - 1) * HIFIGAN_HOP_LENGTH if gl_on else (n + 2 * int(getattr(hg, "inference_padding", 0))) * hg.hop
            if limiter is not None:          # aux["limiter_stats"]: the f64 [B, 24] of MelFrontEnd.limit, on the device
                _, aux["limiter_stats"] = _frontend().loudness_normalize(
                    aux["wav"], np.maximum(n, 1).astype(np.int32), float(loudness_lufs), float(peak_ceiling), sample_rate=HIFIGAN_SR,
                    out=aux["wav"], return_stats=True, true_peak_ceiling_dbtp=true_peak_ceiling_dbtp, limiter=limiter)
                return mel, out_lens, aux
            _frontend().loudness_normalize(aux["wav"], np.maximum(n, 1).astype(np.int32), float(loudness_lufs), float(peak_ceiling),
                                           sample_rate=HIFIGAN_SR, out=aux["wav"], true_peak_ceiling_dbtp=true_peak_ceiling_dbtp)
            return mel, out_lens, aux
        if griffin_lim is None or griffin_lim is False:
            return self.native.synthesize_batch(phone_tokens, phone_lens, mels, mel_lens, forced_durations, forced_codes,
                                                run_plm=forced_codes is None, vocoder=vocoder, return_aux=return_aux,
                                                sampling=sampling, seeds=seeds)
        if vocoder:
            raise ValueError("vocoder=True (HiFi-GAN) and griffin_lim are two vocoders for one mel: pass one")
        mel, out_lens, aux = self.native.synthesize_batch(phone_tokens, phone_lens, mels, mel_lens, forced_durations, forced_codes,
                                                          run_plm=forced_codes is None, vocoder=False, return_aux=True,
                                                          sampling=sampling, seeds=seeds)
        aux["wav"] = self.vocode_griffin_lim(mel, out_lens, **(griffin_lim if isinstance(griffin_lim, dict) else {}))
        return mel, out_lens, aux

    def vocode_griffin_lim(self, mel, mel_lens=None, n_iter: int = 32, momentum: float = 0.99, seeds=0, return_resid: bool = False):
        """Audio from a log-mel with no vocoder weights: mel f32 [B, T, 80] (device) -> wav f32 [B, (T - 1) * hop] by the
        Griffin-Lim rule of csrc/griffinlim.hip (MelFrontEnd.griffin_lim), utterance b holding (mel_lens[b] - 1) * hop samples and
        zeros beyond: the exact inverse of the mel front-end's framing, without HiFi-GAN's inference padding.  Intelligible but
        buzzy - the fallback when the hub's HiFi-GAN weights are not on hand and a way to listen to a synthetic or partly trained
        model, not a replacement for HiFi-GAN.  Every utterance needs at least n_fft / (2 hop) + 2 = 4 frames."""
        return _frontend().griffin_lim(mel, mel_lens, n_iter=n_iter, momentum=momentum, seeds=seeds, return_resid=return_resid)

    def output_prosody(self, mel_lens, aux, tracker: str = "yin", phone_lens=None):
        """Phone-level prosody of a synthesis call's own output: `mel_lens` and `aux` as `synthesize(..., return_aux=True)` returned
        them with a vocoder on (aux["wav"] the audio, aux["dur"] the ADM's durations, device).  HiFi-GAN audio carries
        inference_padding * hop samples on both sides of every utterance, which are removed first; Griffin-Lim audio has none.
        Frame t of the tracks is then mel frame t.  F0 (tracker "yin" or "viterbi") and energy are tracked on the GPU and reduced
        over the durations with frame_lens = mel_lens -> dict: "phones" (phone_prosody's dict, [B, Np]), "durations"
        (duration_stats' dict, [B]), "f0" and "energy" (device f32 [B, T], T >= max mel_lens) and "frame_lens"."""
        if tracker not in ("yin", "viterbi"):
            raise ValueError("tracker must be 'yin' or 'viterbi'")
        wav, dur = aux.get("wav"), aux["dur"]
        if wav is None:
            raise ValueError("aux has no audio: synthesize with vocoder=True or griffin_lim=True")
        fe = _frontend()
        hop = fe.audio.hop_length
        ml = np.asarray(mel_lens, np.int32).reshape(-1)
        top = int(ml.max())
        pad = int(getattr(self.hifi_gan.cfg, "inference_padding", 0)) if self.hifi_gan is not None else 0
        if self.hifi_gan is not None and wav.shape[1] >= (top + 2 * pad) * hop:      # HiFi-GAN: (mel_lens + 2 pad) hop samples a row
            x, lens = wav[:, pad * hop:(pad + top) * hop].contiguous(), ml * hop
        else:                                                                         # Griffin-Lim: (mel_lens - 1) hop samples
            x, lens = wav, (ml - 1) * hop
        f0 = (fe.f0 if tracker == "yin" else fe.f0_track)(x, lens)
        energy = fe.energy(x, lens)
        return {"phones": phone_prosody(f0, dur, energy, phone_lens, ml), "durations": duration_stats(dur, phone_lens), "f0": f0,
                "energy": energy, "frame_lens": ml}

    def output_formants(self, mel_lens, aux, tracker: str = "yin", formants: Optional[Formants] = None, track: Optional[FormantTrack] = None):
        """The formant figures of a synthesis call's own output: `mel_lens` and `aux` as `synthesize(..., return_aux=True)` returned
        them with a vocoder on.  The inference padding is taken off as `output_prosody` takes it off; the audio is tracked for F0
        (tracker "yin" or "viterbi") and analysed by `extract_formants` (formants: a `Formants`), and the figures are taken over the
        voiced frames with four candidates among the first mel_lens[b] -> formant_stats' dict (FORMANT_STAT_NAMES, float64 [B]) with
        "freq", "bw", "count", "f0" (device, [B, T, ...]) and "frame_lens" beside it.  `aux` is not altered.  track: a `FormantTrack` has
        the candidates tracked across frames first (`track_formants`) and the figures taken over track_freq / track_count, which are
        returned too with track_bw and sel; None (the default) is the call of before."""
        if tracker not in ("yin", "viterbi"):
            raise ValueError("tracker must be 'yin' or 'viterbi'")
        wav = aux.get("wav")
        if wav is None:
            raise ValueError("aux has no audio: synthesize with vocoder=True or griffin_lim=True")
        fe = _frontend()
        hop = fe.audio.hop_length
        ml = np.asarray(mel_lens, np.int32).reshape(-1)
        top = int(ml.max())
        pad = int(getattr(self.hifi_gan.cfg, "inference_padding", 0)) if self.hifi_gan is not None else 0
        if self.hifi_gan is not None and wav.shape[1] >= (top + 2 * pad) * hop:      # HiFi-GAN: (mel_lens + 2 pad) hop samples a row
            x, lens = wav[:, pad * hop:(pad + top) * hop].contiguous(), ml * hop
        else:                                                                         # Griffin-Lim: (mel_lens - 1) hop samples
            x, lens = wav, (ml - 1) * hop
        f0 = (fe.f0 if tracker == "yin" else fe.f0_track)(x, lens)
        res = extract_formants(x, None, lens, formants, track)
        T = min(f0.shape[1], res["count"].shape[1])
        fl = np.minimum(np.minimum(ml, res["frame_lens"]), T).astype(np.int32)
        fk, ck = ("freq", "count") if track is None else ("track_freq", "track_count")
        out = formant_stats(res[fk][:, :T], res[ck][:, :T], f0[:, :T], fl)
        out.update(freq=res["freq"], bw=res["bw"], count=res["count"], f0=f0, frame_lens=fl)
        if track is not None:
            out.update({k: res[k] for k in ("track_freq", "track_bw", "track_count", "sel")})
        return out

    def align_prompt(self, prompt_phone_tokens, mels, prompt_phone_lens=None, mel_lens=None, return_aux: bool = False):
        """The phone-level alignment of a prompt utterance to its own phones, made by the model itself - the `prompt_durations` of
        `synthesize_prompt_conditioned` / `synthesize_prosody_interpolated` without the Montreal Forced Aligner TextGrids the
        reference reads during data preparation (prepare_ds.py, utils/textgrid.py).  `prompt_phone_tokens` int64 [B, Npp], `mels`
        f32 [B, Tp, 80] -> host int32 [B, Npp], row b summing to mel_lens[b] exactly (a phone may get 0).  Three steps: `synthesize`
        on the prompt's own phones under the prompt's own timbre (greedy PLM, no vocoder: the ADM's durations and a synthetic mel);
        `dtw` of that mel onto `mels` (csrc/dtw.hip); `align_durations`, which gives real frame j to the phone that owns the
        synthetic frame hi[j].  Always greedy, so the alignment is deterministic.  return_aux: (durations, dict) with the synthetic
        durations `syn_dur` (host int32 [B, Npp]), `syn_lens`, the path's lo, hi, steps, total (device), and `mcd`, the dict of
        mel_cepstral_distortion for the re-synthesis against the real prompt along the warp of their cepstra (`mcd_lo`, `mcd_hi`,
        device) - the one number that says whether the alignment is any good; the durations come from the 80-bin warp as
        before, and without return_aux nothing of this runs.  Both lengths of the
        warp are capped at runtime.DTW_MAX_LEN = 4096 frames (MT2_DTW_MAX_LEN): a prompt longer than that, or a synthesis of it that
        comes out longer (the ADM may give a phone up to 128 frames - untrained durations on many phones), is refused with a
        NativeError from mt2_dtw_align, never clamped.  Alignment quality on real speech is unpinned: there is no aligner here to
        compare with."""
        nat = self.native
        B = prompt_phone_tokens.shape[0]
        ml = nat._lens(mel_lens, B, mels.shape[1])
        ppl = nat._lens(prompt_phone_lens, B, prompt_phone_tokens.shape[1])
        syn, syn_lens, aux = nat.synthesize_batch(prompt_phone_tokens, ppl, mels, ml, return_aux=True)
        syn_lens = np.asarray(syn_lens, np.int32)
        syn_dur = aux["dur"].cpu().numpy().astype(np.int32)
        path = nat.dtw(syn[:, :max(int(syn_lens.max()), 1)], mels, syn_lens, ml)
        dur = nat.align_durations(path["hi"], ml, syn_dur, ppl)
        if not return_aux:
            return dur
        path.update(syn_dur=syn_dur, syn_lens=syn_lens)
        # how good the alignment is: the distortion of the re-synthesis against the real prompt along the warp of their cepstra
        row, lo, hi = nat.mcd(syn[:, :max(int(syn_lens.max()), 1)], mels, syn_lens, ml, return_path=True)
        path.update(mcd=_mcd_dict(row), mcd_lo=lo, mcd_hi=hi)
        return dur, path

    def synthesize_prompt_conditioned(self, phone_tokens, mels, prompt_phone_tokens, prompt_durations=None, phone_lens=None,
                                      mel_lens=None, prompt_phone_lens=None, forced_durations=None, vocoder: bool = False,
                                      return_aux: bool = False, sampling=None, seeds=None):
        """Synthesis with the PLM conditioned on the prompt's prosody - the layout the PLM is trained
        on (reference modules/datamodule.py:161-177,196-212) at inference: the prompt's length-regulated, max-pooled
        tc_latents in front of the target's, the prompt's VQ-PE codes behind the BOS, greedy decoding from there.
        `prompt_phone_tokens` int64 [B, Npp] / `prompt_durations` int32 [B, Npp] are the prompt utterance's own phones and
        alignment (sum = prompt frames); `prompt_durations=None` takes the alignment from `align_prompt` (the model's own synthesis
        of the prompt warped onto it by DTW), a given array exactly the path it always took.  A prompt whose silence was cut off (`MelFrontEnd.from_audio(trim_db=...,
        return_bounds=True)`) needs its alignment cut the same way: `audio_io.trim_alignment(prompt_phone_tokens,
        prompt_durations, start, end)`.  ONE native call (mt2_synthesize_prompt_conditioned): the MRTE mel encoder runs once
        for both phone sets, the prompt's VQ-PE beside the ADM on the handle's side stream, nothing leaves the device between
        the stages but the durations.  `synthesize_prompt_conditioned_staged` is the same computation as ten C-ABI stage
        calls (round 3's form; kept as the cross-check of the fused entry point)."""
        if prompt_durations is None:
            prompt_durations = self.align_prompt(prompt_phone_tokens, mels, prompt_phone_lens, mel_lens)
        out = self.native.synthesize_prompt_conditioned(phone_tokens, phone_lens, mels, mel_lens, prompt_phone_tokens,
                                                        prompt_phone_lens, prompt_durations, forced_dur=forced_durations,
                                                        vocoder=vocoder, sampling=sampling, seeds=seeds)
        return out if return_aux else (out[0], out[1])

    def synthesize_prompt_conditioned_staged(self, phone_tokens, mels, prompt_phone_tokens, prompt_durations=None, phone_lens=None,
                                             mel_lens=None, prompt_phone_lens=None, forced_durations=None, vocoder: bool = False,
                                             return_aux: bool = False):
        """The stage-call composition of `synthesize_prompt_conditioned`: tc_latent (prompt, target), vqpe_forward, adm_infer,
        length_regulate, max_pool, plm_infer_prompted, then synthesize_batch with the decoded codes forced.
        `prompt_durations=None`: `align_prompt`, as there."""
        import torch
        nat = self.native
        B = phone_tokens.shape[0]
        mel_lens = nat._lens(mel_lens, B, mels.shape[1])
        if prompt_durations is None:
            prompt_durations = self.align_prompt(prompt_phone_tokens, mels, prompt_phone_lens, mel_lens)
        pd = np.asarray(prompt_durations.detach().cpu().numpy() if hasattr(prompt_durations, "detach") else prompt_durations,
                        np.int32).reshape(B, -1)
        ppl = nat._lens(prompt_phone_lens, B, prompt_phone_tokens.shape[1])
        for b in range(B):
            if int(pd[b, :ppl[b]].sum()) != int(mel_lens[b]):
                raise ValueError("prompt durations must sum to the prompt's mel frames")      # datamodule.py:198 assert
        st = self.generator.cfg.vqpe.stride
        # prompt side: pooled tc_latents + prosody codes
        tc_p = nat.tc_latent(prompt_phone_tokens, mels, ppl, mel_lens)
        exp_p = nat.length_regulate(tc_p, pd, ppl)                               # [B, Tp, H]; row b holds mel_lens[b] frames
        cond_p = nat.max_pool_ceil(exp_p, st, mel_lens)                          # [B, ceil(Tp / 8), H]
        codes_p = nat.vqpe_forward(mels, mel_lens)[1][0]                         # [B, ceil(Tp / 8)]
        q_p = -(-mel_lens // st)
        P = int(q_p[0])
        if (q_p != P).any():
            raise ValueError("prompt-conditioned batches need prompts of one pooled length (pad-free prefix layout)")
        # target side: ADM, regulation, pooling
        pl = nat._lens(phone_lens, B, phone_tokens.shape[1])
        tc = nat.tc_latent(phone_tokens, mels, pl, mel_lens)
        dur = nat.adm_infer(tc, pl)
        use = np.asarray(dur.cpu().numpy() if forced_durations is None else forced_durations, np.int32).reshape(B, -1)
        len_t = np.asarray([int(use[b, :pl[b]].sum()) for b in range(B)], np.int32)
        exp_t = nat.length_regulate(tc, use, pl)
        cond_t = nat.max_pool_ceil(exp_t, st, len_t)
        q_t = -(-len_t // st)
        codes = nat.plm_infer(torch.cat([cond_p[:, :P], cond_t], dim=1), q_t, prefix_codes=codes_p[:, :P])
        out = nat.synthesize_batch(phone_tokens, pl, mels, mel_lens, forced_dur=use, forced_codes=codes, run_plm=False,
                                   vocoder=vocoder, return_aux=True)
        aux = out[2]
        aux["dur"], aux["prompt_codes"] = dur, codes_p[:, :P]
        return (out[0], out[1], aux) if return_aux else (out[0], out[1])

    def synthesize_prosody_interpolated(self, phone_tokens, mels, prompt_phone_tokens, prompt_durations=None, rhythm_mels=None,
                                        rhythm_phone_tokens=None, rhythm_durations=None, gamma=None, phone_lens=None, mel_lens=None,
                                        prompt_phone_lens=None, rhythm_mel_lens=None, rhythm_phone_lens=None,
                                        forced_durations=None, vocoder: bool = False, return_aux: bool = False, sampling=None,
                                        seeds=None):
        """Synthesis with the prosody interpolated between two prompts (Mega-TTS 2, section 3.3): the timbre prompt `mels` (with its
        own phones `prompt_phone_tokens` and alignment `prompt_durations`, as `synthesize_prompt_conditioned` takes them) and a
        rhythm prompt `rhythm_mels` / `rhythm_phone_tokens` / `rhythm_durations`.  The PLM runs two contexts in lock step
        (`plm_infer_interpolated`): both see the target's pooled tc_latents under the TIMBRE prompt; context A's prefix is the
        timbre prompt's pooled tc_latents and VQ-PE codes, context B's the rhythm prompt's (its phones and alignment through MRTE
        with its own mel, its own VQ-PE codes).  gamma = 0 is `synthesize_prompt_conditioned`; the timbre comes from `mels` at every
        gamma.  Composed from stage calls like `synthesize_prompt_conditioned_staged`; all prompts of the call must have one pooled
        length P (ValueError otherwise).  `prompt_durations=None` / `rhythm_durations=None`: that prompt's alignment comes from
        `align_prompt` (each prompt synthesised under its own timbre and warped onto itself by DTW); `rhythm_mels`,
        `rhythm_phone_tokens` and `gamma` have defaults only because they follow an optional parameter, and are required."""
        import torch
        nat = self.native
        B = phone_tokens.shape[0]
        st = self.generator.cfg.vqpe.stride
        if rhythm_mels is None or rhythm_phone_tokens is None or gamma is None:
            raise TypeError("synthesize_prosody_interpolated needs rhythm_mels, rhythm_phone_tokens and gamma")
        if prompt_durations is None:
            prompt_durations = self.align_prompt(prompt_phone_tokens, mels, prompt_phone_lens, mel_lens)
        if rhythm_durations is None:
            rhythm_durations = self.align_prompt(rhythm_phone_tokens, rhythm_mels, rhythm_phone_lens, rhythm_mel_lens)

        def prompt_side(pm, pm_lens, pp, pp_lens, pdur):
            pm_lens = nat._lens(pm_lens, B, pm.shape[1])
            pd = np.asarray(pdur.detach().cpu().numpy() if hasattr(pdur, "detach") else pdur, np.int32).reshape(B, -1)
            ppl = nat._lens(pp_lens, B, pp.shape[1])
            for b in range(B):
                if int(pd[b, :ppl[b]].sum()) != int(pm_lens[b]):
                    raise ValueError("prompt durations must sum to the prompt's mel frames")      # datamodule.py:198 assert
            tc_p = nat.tc_latent(pp, pm, ppl, pm_lens)
            cond_p = nat.max_pool_ceil(nat.length_regulate(tc_p, pd, ppl), st, pm_lens)
            codes_p = nat.vqpe_forward(pm, pm_lens)[1][0]
            return cond_p, codes_p, -(-pm_lens // st), pm_lens

        cond_a, codes_a, q_a, mel_lens = prompt_side(mels, mel_lens, prompt_phone_tokens, prompt_phone_lens, prompt_durations)
        cond_b, codes_b, q_b, _ = prompt_side(rhythm_mels, rhythm_mel_lens, rhythm_phone_tokens, rhythm_phone_lens, rhythm_durations)
        P = int(q_a[0])
        if (q_a != P).any() or (q_b != P).any():
            raise ValueError("prosody interpolation needs prompts of one pooled length (pad-free prefix layout)")
        # target side: ADM, regulation, pooling - under the timbre prompt
        pl = nat._lens(phone_lens, B, phone_tokens.shape[1])
        tc = nat.tc_latent(phone_tokens, mels, pl, mel_lens)
        dur = nat.adm_infer(tc, pl)
        use = np.asarray(dur.cpu().numpy() if forced_durations is None else forced_durations, np.int32).reshape(B, -1)
        len_t = np.asarray([int(use[b, :pl[b]].sum()) for b in range(B)], np.int32)
        cond_t = nat.max_pool_ceil(nat.length_regulate(tc, use, pl), st, len_t)
        q_t = -(-len_t // st)
        codes = nat.plm_infer_interpolated(torch.cat([cond_a[:, :P], cond_t], dim=1), torch.cat([cond_b[:, :P], cond_t], dim=1),
                                           q_t, gamma, prefix_a=codes_a[:, :P], prefix_b=codes_b[:, :P], sampling=sampling,
                                           seeds=seeds)
        out = nat.synthesize_batch(phone_tokens, pl, mels, mel_lens, forced_dur=use, forced_codes=codes, run_plm=False,
                                   vocoder=vocoder, return_aux=True)
        aux = out[2]
        aux["dur"], aux["prompt_codes"], aux["rhythm_codes"] = dur, codes_a[:, :P], codes_b[:, :P]
        return (out[0], out[1], aux) if return_aux else (out[0], out[1])

    def synthesize_list(self, utterances: Sequence, vocoder: bool = False, sampling=None, seeds=None):
        """List of utterance records (`.phone` int64 [Np], `.prompt_mel` f32 [Tp, 80], optional
        `.durations`, `.p_codes`) -> (mel [B, Tm_max, 80] device tensor, lens); pads to the batch
        maxima and forwards per-utterance lengths, so every utterance is computed as if alone.
        `sampling` (sampling.PLMSampling): the PLM's codes are drawn, utterance i seeded by its record's `.seed` when it has
        one, otherwise by `seeds` (one per record, or an int s -> s + i; default s = 0)."""
        import torch
        B = len(utterances)
        Np = max(u.phone.size for u in utterances)
        Tp = max(u.prompt_mel.shape[0] for u in utterances)
        phone = np.zeros((B, Np), np.int64)
        mel = np.zeros((B, Tp, utterances[0].prompt_mel.shape[1]), np.float32)
        pl, ml = np.zeros(B, np.int32), np.zeros(B, np.int32)
        have_d = all(getattr(u, "durations", None) is not None for u in utterances)
        have_c = all(getattr(u, "p_codes", None) is not None for u in utterances)
        dur = np.zeros((B, Np), np.int32) if have_d else None
        tq = max(u.p_codes.size for u in utterances) if have_c else 0
        codes = np.zeros((B, tq), np.int64) if have_c else None
        for i, u in enumerate(utterances):
            pl[i], ml[i] = u.phone.size, u.prompt_mel.shape[0]
            phone[i, :pl[i]] = u.phone
            mel[i, :ml[i]] = u.prompt_mel
            if have_d:
                dur[i, :pl[i]] = u.durations
            if have_c:
                codes[i, :u.p_codes.size] = u.p_codes
        dev = self.native.device
        kw = {}
        if sampling is not None:
            sd = seed_array(seeds, B)
            for i, u in enumerate(utterances):
                if getattr(u, "seed", None) is not None:
                    sd[i] = np.uint64(int(u.seed) & 0xFFFFFFFFFFFFFFFF)
            kw = dict(sampling=sampling, seeds=sd)
        elif seeds is not None:
            raise ValueError("seeds given without sampling")
        out = self.native.synthesize_batch(torch.from_numpy(phone).to(dev), pl, torch.from_numpy(mel).to(dev), ml,
                                           forced_dur=dur,
                                           forced_codes=torch.from_numpy(codes).to(dev) if have_c else None,
                                           run_plm=not have_c, vocoder=vocoder, **kw)
        return out[0], out[1]

    # -- the reference's entry point (models/megatts2.py:325-375).  Prompt audio: every *.wav of the directory
    # is loaded (mono), peak-normalised, turned into a mel by extract_mel_spec (on the GPU) and the mels
    # are concatenated along time (:332-344).  A file at another rate than 16 kHz is resampled as `librosa.load(wav,
    # sr=16000)` does it there (:335) - on the GPU (MelFrontEnd.from_audio; its own filter, parity with librosa's
    # unpinned); resample=False rejects such a file instead.  trim_db: the leading and trailing silence of every prompt
    # file is cut off behind the normalisation, `librosa.effects.trim(y, top_db=trim_db)` of :337 (commented out there:
    # its prompts are pre-cut) - on the GPU as well (MelFrontEnd.from_audio(trim_db=...), 16 kHz files included); None
    # leaves the audio whole.  Text -> phone ids is the reference's G2P (pypinyin + MFA
    # dictionary, host side, outside the hot path); when it is not importable pass `phone_tokens` instead.
    # vocoder: None is the reference's behaviour - HiFi-GAN when its weights were found, otherwise no audio and no file;
    # "griffin_lim" (or a dict of vocode_griffin_lim's keyword arguments) vocodes the first prompt mel and the generated mel by
    # Griffin-Lim, concatenates them as the HiFi-GAN branch does, sets aux["wav"] and writes out_path.  That audio has
    # (T - 1) * hop samples per mel of T frames and no inference padding, unlike decode_batch.
    # loudness_lufs: None leaves the levels as the vocoder produced them; a number brings the vocoded prompt and the generated audio
    # EACH to that integrated loudness (BS.1770, MelFrontEnd.loudness_normalize; peak_ceiling > 0 caps the gain by the sample peak)
    # before they are concatenated and written, with either vocoder - the two halves of the file then sound equally loud.
    # true_peak_ceiling_dbtp (None = off; needs loudness_lufs): each half's gain is capped so that its true peak stays under this many dBTP.
    # limiter (None = off; a runtime.Limiter; needs true_peak_ceiling_dbtp): each half reaches loudness_lufs under that ceiling, its
    # crests turned down by the look-ahead limiter, where one gain would land under it.
    # denoise (None = off; a runtime.Denoise): every prompt file, 16 kHz ones too, goes through MelFrontEnd.from_audio(denoise=...):
    # resample, peak-normalise, suppress stationary noise (csrc/denoise.hip), peak-normalise, trim.  aux["prompt_noise"] then holds
    # one dict per prompt file with the figures of the suppression (DENOISE_NAMES).
    # dereverb (None = off; a runtime.Dereverb): likewise through from_audio(dereverb=...): resample, peak-normalise, remove late
    # reverberation by weighted prediction error (csrc/wpe.hip), the denoiser behind it if asked for, peak-normalise, trim.
    # aux["prompt_reverb"] then holds one dict per prompt file with the figures of the stage (WPE_NAMES).
    # declip (None = off; a runtime.Declip): likewise through from_audio(declip=...), where it comes first of all, at the file's own
    # sample rate (csrc/declip.hip): declip, resample, peak-normalise, ...  aux["prompt_clipping"] then holds one dict per prompt file
    # with the figures of the stage (DECLIP_NAMES).
    # cut_pauses (None = off; a runtime.Pauses): likewise through from_audio(cut_pauses=...), where it comes last, in the trim's place
    # (csrc/segments.hip): the pauses inside every prompt file are cut out as well as its ends, so it excludes trim_db.
    # aux["prompt_pauses"] then holds one dict per prompt file with the figures of the stage (PAUSES_NAMES).
    def forward(self, wavs_dir: str, text: Optional[str] = None, phone_tokens=None, out_path: Optional[str] = "test.wav",
                phones: Optional[Sequence[str]] = None, resample: bool = True, trim_db: Optional[float] = None, vocoder=None,
                loudness_lufs: Optional[float] = None, peak_ceiling: float = 0.0, true_peak_ceiling_dbtp: Optional[float] = None,
                limiter=None, denoise: Optional[Denoise] = None, dereverb: Optional[Dereverb] = None, declip: Optional[Declip] = None,
                cut_pauses: Optional[Pauses] = None):
        import torch
        if cut_pauses is not None and trim_db is not None:
            raise ValueError("cut_pauses cuts the ends itself: it excludes trim_db")
        if true_peak_ceiling_dbtp is not None and loudness_lufs is None:
            raise ValueError("true_peak_ceiling_dbtp caps the gain of the loudness normalisation: it needs loudness_lufs")
        if limiter is not None and true_peak_ceiling_dbtp is None:
            raise ValueError("a limiter holds a true-peak ceiling: it needs true_peak_ceiling_dbtp (and loudness_lufs)")
        level = {} if loudness_lufs is None else {"loudness_lufs": float(loudness_lufs), "peak_ceiling": float(peak_ceiling)}
        if true_peak_ceiling_dbtp is not None:
            level["true_peak_ceiling_dbtp"] = float(true_peak_ceiling_dbtp)
        if limiter is not None:
            level["limiter"] = limiter

        def levelled(x):          # the vocoded prompt, a 1-D device tensor
            if loudness_lufs is None:
                return x
            return _frontend().loudness_normalize(x.unsqueeze(0), None, float(loudness_lufs), float(peak_ceiling), sample_rate=HIFIGAN_SR,
                                                  true_peak_ceiling_dbtp=true_peak_ceiling_dbtp,
                                                  **({} if limiter is None else {"limiter": limiter}))[0]

        if not (vocoder is None or vocoder == "griffin_lim" or isinstance(vocoder, dict)):
            raise ValueError(f"vocoder={vocoder!r}: None (HiFi-GAN when loaded) or 'griffin_lim'")
        from . import audio_io
        wavs = sorted(glob.glob(f"{wavs_dir}/*.wav"))
        if not wavs:
            raise NativeError(f"no *.wav under {wavs_dir}")

        prompt_noise, prompt_reverb, prompt_clipping, prompt_pauses = [], [], [], []

        def prompt_mel(w):
            y, sr = audio_io.read_wav(w)
            if denoise is not None or dereverb is not None or declip is not None or cut_pauses is not None:
                if sr != HIFIGAN_SR and not resample:
                    raise ValueError(f"{w}: {sr} Hz, expected {HIFIGAN_SR} Hz (resample=False)")
                more = {} if declip is None else {"declip": declip, "return_clipping": True}      # absent: exactly the call of before
                if cut_pauses is not None:
                    more.update(cut_pauses=cut_pauses, return_pauses=True)
                res = _frontend().from_audio(torch.from_numpy(y).unsqueeze(0).cuda(), sr, trim_db=trim_db, denoise=denoise,
                                             return_noise=denoise is not None, dereverb=dereverb, return_reverb=dereverb is not None, **more)
                figures = list(res[2:])      # in from_audio's order: noise, reverb, clipping, pauses - those that were asked for
                for on, names, sink in ((denoise, DENOISE_NAMES, prompt_noise), (dereverb, WPE_NAMES, prompt_reverb),
                                        (declip, DECLIP_NAMES, prompt_clipping), (cut_pauses, PAUSES_NAMES, prompt_pauses)):
                    if on is not None:
                        sink.append(dict(zip(names, figures.pop(0)[0].cpu().numpy().tolist())))
                return res[0][0]
            if sr == HIFIGAN_SR and trim_db is None:          # audio_io.load_audio's two steps
                return extract_mel_spec(torch.from_numpy(audio_io.normalize(y))).transpose(0, 1)
            if sr != HIFIGAN_SR and not resample:
                raise ValueError(f"{w}: {sr} Hz, expected {HIFIGAN_SR} Hz (resample=False)")
            return _frontend().from_audio(torch.from_numpy(y).unsqueeze(0).cuda(), sr, trim_db=trim_db)[0][0]

        mels = [prompt_mel(w) for w in wavs]
        mels_prompt = mels[0]
        mels = torch.cat(mels, dim=0).unsqueeze(0)
        if phone_tokens is None:
            if phones is None:          # text -> phone symbols: the reference's G2P (host side, out of scope), if importable
                try:
                    from modules.tokenizer import TextTokenizer
                except Exception as e:  # pragma: no cover - pypinyin / phonemizer absent in this image
                    raise NativeError("text input needs the reference's G2P (modules.tokenizer.TextTokenizer: pypinyin, "
                                      "phonemizer); pass phones=[...] (symbols) or phone_tokens=[...] (ids) instead") from e
                if self.tt is None:
                    self.tt = TextTokenizer()
                phones = self.tt.tokenize_lty(self.tt.tokenize(text))
            if self.ttc is None:
                raise NativeError("phone symbols given but no symbol_table was passed to Megatts(...)")
            phone_tokens = self.ttc.phone2token(phones)               # :350-351
        phone_tokens = torch.as_tensor(np.asarray(phone_tokens)).to(torch.int64).reshape(1, -1).cuda()
        if vocoder is not None:
            gl = vocoder if isinstance(vocoder, dict) else {}
            mel, mel_lens, aux = self.synthesize(phone_tokens, mels, return_aux=True, griffin_lim=gl or True, **level)
            if denoise is not None:
                aux["prompt_noise"] = prompt_noise
            if dereverb is not None:
                aux["prompt_reverb"] = prompt_reverb
            if declip is not None:
                aux["prompt_clipping"] = prompt_clipping
            if cut_pauses is not None:
                aux["prompt_pauses"] = prompt_pauses
            if out_path:
                prompt = levelled(self.vocode_griffin_lim(mels_prompt.unsqueeze(0).contiguous(), **gl)[0])
                audio = torch.cat([prompt, aux["wav"][0, :(int(mel_lens[0]) - 1) * HIFIGAN_HOP_LENGTH]])
                audio_io.write_wav(out_path, audio, HIFIGAN_SR)
            return mel, mel_lens, aux
        mel, mel_lens, aux = self.synthesize(phone_tokens, mels, vocoder=self.hifi_gan is not None, return_aux=True,
                                             **(level if self.hifi_gan is not None else {}))
        if denoise is not None:
            aux["prompt_noise"] = prompt_noise
        if dereverb is not None:
            aux["prompt_reverb"] = prompt_reverb
        if declip is not None:
            aux["prompt_clipping"] = prompt_clipping
        if cut_pauses is not None:
            aux["prompt_pauses"] = prompt_pauses
        if self.hifi_gan is not None and out_path:
            # :370-375  prompt audio (vocoded first prompt mel) followed by the generated audio; decode_batch output
            # includes the generator's inference padding on both sides, exactly as the reference concatenates it
            hg = self.hifi_gan.cfg
            prompt = levelled(self.hifi_gan.decode_batch(mels_prompt.transpose(0, 1).unsqueeze(0).contiguous())[0, 0])
            audio = torch.cat([prompt, aux["wav"][0, :(int(mel_lens[0]) + 2 * hg.inference_padding) * hg.hop]])
            audio_io.write_wav(out_path, audio, HIFIGAN_SR)
        return mel, mel_lens, aux

    __call__ = forward
