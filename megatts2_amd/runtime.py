"""ctypes binding of libmegatts2_hip.so (C ABI: include/megatts2_hip.h).

PyTorch-ROCm is used for plumbing only: device memory (`torch.empty(..., device='cuda')`), the
current HIP stream and `torch.distributed`.  Every numeric stage runs in the hand-written gfx950
kernels behind the C ABI; there is NO PyTorch / CPU fallback - if the shared library or a gfx950
device is missing, construction fails loudly.
"""
from __future__ import annotations

import ctypes as C
import dataclasses
import math
import os
from typing import Dict, Optional, Sequence

import numpy as np

from . import config as cfgmod
from . import sampling as sampmod

_LIB = None
MAX_POSITIONS = 8192       # rows of the sine tables (the reference builds 4000 and extends on demand)

MT2_RUN_PLM, MT2_RUN_VOCODER, MT2_SKIP_ADM, MT2_PROMPT_VQPE = 1, 2, 4, 8
ACT_NONE, ACT_RELU, ACT_LRELU, ACT_TANH = 0, 1, 2, 3
ACT_LOGCLAMP = 4          # epilogue only: log(max(v, pro_slope))
MT2_RESAMPLE_NORMALIZE = 1
TRIM_FRAME, TRIM_HOP = 2048, 512      # MT2_TRIM_FRAME, MT2_TRIM_HOP
F0_FRAME, F0_WINDOW, F0_MAX_LAG = 1024, 768, 256      # MT2_F0_FRAME, MT2_F0_WINDOW, MT2_F0_MAX_LAG
DTW_MAX_LEN, DTW_DIR_COLS = 4096, 16  # MT2_DTW_MAX_LEN, MT2_DTW_DIR_COLS
PROSODY_FIELDS = 8                    # MT2_PROSODY_FIELDS
MCD_FIELDS, MCD_MAX_ORDER = 8, 32     # MT2_MCD_FIELDS, MT2_MCD_MAX_ORDER
MCD_NAMES = ("cells", "mcd_db", "max_db", "voiced_cells", "f0_rmse_cents", "f0_offset_cents", "vuv_cells", "vuv_error")
LOUDNESS_FIELDS = 8                   # MT2_LOUDNESS_FIELDS
EBU_FIELDS, TP_ZERO_CROSSINGS, TP_TAPS, TP_TILE = 18, 12, 24, 1024      # MT2_EBU_FIELDS, MT2_TP_ZERO_CROSSINGS, MT2_TP_TAPS, MT2_TP_TILE
LIMITER_FIELDS, LIMITER_TILE, LIMITER_MAX_HALF_WINDOW, LIMITER_MAX_PASSES = 24, 1024, 1024, 4      # MT2_LIMITER_*


class NativeError(RuntimeError):
    pass


class Limiter:
    """The settings of the true-peak look-ahead limiter (csrc/limiter.hip): the half window in milliseconds (the gain looks that far
    ahead and behind; 5 ms is 80 samples at 16 kHz) and the passes of the normalising form (1 .. 4), each of which re-measures the
    loudness of the limited audio and corrects the gain in front of the limiter."""

    def __init__(self, window_ms: float = 5.0, passes: int = 2):
        self.window_ms, self.passes = float(window_ms), int(passes)

    def __repr__(self):
        return f"Limiter(window_ms={self.window_ms}, passes={self.passes})"


@dataclasses.dataclass(frozen=True)
class Denoise:
    """The settings of the stationary-noise suppression (csrc/denoise.hip; the rule is in include/megatts2_hip.h): the per-bin noise
    floor is the `percentile`-th percentile of the power over time (1 .. 99) times the factor that turns that quantile of an
    exponential distribution into its mean; a cell keeps max(floor_gain, (P - over_subtraction * floor) / P) of its amplitude, averaged
    over +-smooth_bins bins and +-smooth_frames frames (0 .. 8 each).  A steady tone is stationary and is removed like hum; speech
    present in a bin for more than 100 - percentile % of the frames raises that bin's floor."""
    percentile: int = 20
    over_subtraction: float = 3.0
    floor_gain: float = 0.1
    smooth_bins: int = 1
    smooth_frames: int = 1

    def c_struct(self) -> "MT2DenoiseConfig":
        return MT2DenoiseConfig(int(self.percentile), float(self.over_subtraction), float(self.floor_gain), int(self.smooth_bins),
                                int(self.smooth_frames), 0)


class MT2DenoiseConfig(C.Structure):
    _fields_ = [("percentile", C.c_int32), ("over_subtraction", C.c_float), ("floor_gain", C.c_float), ("smooth_bins", C.c_int32),
                ("smooth_frames", C.c_int32), ("reserved", C.c_int32)]


DENOISE_NAMES = ("noise_db", "snr_db", "floored_share", "reduction_db", "frames", "rank", "mean_frame_power", "noise_power")


@dataclasses.dataclass(frozen=True)
class Dereverb:
    """The settings of the de-reverberation by weighted prediction error (csrc/wpe.hip; the rule is in include/megatts2_hip.h): per bin a
    filter of `taps` frames (1 .. 16) predicts the late reverberation from the frames at least `delay` (1 .. 8) back and is subtracted;
    `iterations` (1 .. 8) passes alternate between the variance of the result, averaged over +-`context` frames (0 .. 4) and floored
    at `variance_floor` (in (0, 1]) of the bin's largest, and the filter; `loading` (0 .. 1e-2) is the diagonal loading of the normal
    equations.  Discrete reflections are removed well, diffuse tails only modestly; a steady tone is predictable from its own past and
    is removed like a reflection."""
    delay: int = 3
    taps: int = 10
    iterations: int = 3
    context: int = 1
    variance_floor: float = 1e-2
    loading: float = 1e-8

    def c_struct(self) -> "MT2WpeConfig":
        return MT2WpeConfig(int(self.delay), int(self.taps), int(self.iterations), int(self.context), float(self.variance_floor),
                            float(self.loading), 0)


class MT2WpeConfig(C.Structure):
    _fields_ = [("delay", C.c_int32), ("taps", C.c_int32), ("iterations", C.c_int32), ("context", C.c_int32),
                ("variance_floor", C.c_double), ("loading", C.c_double), ("reserved", C.c_int32)]


WPE_NAMES = ("power_in", "power_out", "reduction_db", "frames", "bins_filtered", "bins_passed", "max_tap", "iterations")


@dataclasses.dataclass(frozen=True)
class Declip:
    """The settings of the declipping by sparsity (csrc/declip.hip, A-SPADE; the rule is in include/megatts2_hip.h): frames of `frame`
    samples (256, 512, 1024 or 2048; the hop is a quarter).  A side of the waveform is clipped when at least max(`min_count`,
    ceil(`min_share` * length)) samples lie within `tol` (0 .. 0.1, relative) of the utterance's extreme - or of `level`, when the
    clipping level is known (NaN: detect).  Each frame with clipped samples is re-estimated as the signal whose spectrum is sparsest
    while the reliable samples stay and the clipped ones lie beyond the level: the sparsity grows by `step` bins every `every`
    iterations until the residual falls under `eps` of the frame's norm, or `max_iter` (0: every * ceil((frame / 2 + 1) / step)) is
    reached.  Soft clipping, and clipping followed by a resampler or a lossy codec, has no flat tops and is not detected; a steady
    full-scale tone reads as clipped."""
    frame: int = 1024
    tol: float = 1e-3
    min_share: float = 1e-4
    min_count: int = 4
    level: float = float("nan")
    step: int = 1
    every: int = 1
    eps: float = 0.02
    max_iter: int = 0

    def c_struct(self) -> "MT2DeclipConfig":
        return MT2DeclipConfig(int(self.frame), int(self.min_count), int(self.step), int(self.every), int(self.max_iter), 0, float(self.tol),
                               float(self.min_share), float(self.level), float(self.eps))

    def frames(self, length: int) -> int:
        """the frames of an utterance of `length` samples: ceil(length / hop) + 3"""
        hop = int(self.frame) // 4
        return -(-int(length) // hop) + 3


class MT2DeclipConfig(C.Structure):
    _fields_ = [("frame", C.c_int32), ("min_count", C.c_int32), ("step", C.c_int32), ("every", C.c_int32), ("max_iter", C.c_int32),
                ("reserved", C.c_int32), ("tol", C.c_double), ("min_share", C.c_double), ("level", C.c_double), ("eps", C.c_double)]


DECLIP_NAMES = ("clipped", "hi", "lo", "share", "frames_iterated", "mean_iterations", "max_iterations", "power_change_db")


class MT2FormantConfig(C.Structure):
    _fields_ = [("window", C.c_int32), ("order", C.c_int32), ("kind", C.c_int32), ("reserved", C.c_int32), ("preemphasis_hz", C.c_double),
                ("fmin_hz", C.c_double), ("max_bandwidth_hz", C.c_double)]


FORMANT_MAX, FORMANT_MAX_WINDOW, FORMANT_MAX_ORDER, FORMANT_MAX_ITERS, FORMANT_STAT_FIELDS = 5, 1024, 32, 64, 12      # MT2_FORMANT_*
FORMANT_WINDOWS = {"hann": 0, "rect": 1}      # MT2_FORMANT_HANN, MT2_FORMANT_RECT
FORMANT_STAT_NAMES = ("frames", "share", "f1", "f2", "f3", "f4", "f1_sigma", "f2_sigma", "f3_sigma", "f4_sigma", "dispersion", "vtl_cm")


@dataclasses.dataclass(frozen=True)
class Formants:
    """The settings of the formant candidates by linear prediction (csrc/formants.hip; the rule is in include/megatts2_hip.h): the audio
    is analysed at 2 * `max_formant_hz` (5500 for an adult female voice, 5000 for a male one, as Praat advises) in frames of `window_ms`
    under a `window` ("hann" or "rect"), behind a pre-emphasis from `preemphasis_hz` up (0: off), by an all-pole fit of `order`
    coefficients (even; two per expected formant and two to spare).  A root of the fit is a candidate when its frequency lies more than
    `fmin_hz` inside (0, rate / 2) and its bandwidth under `max_bandwidth_hz`.  The fit is the autocorrelation method, not Praat's
    Burg; on a voiced frame it is drawn to strong harmonics (a property of linear prediction)."""
    max_formant_hz: float = 5500.0
    order: int = 10
    window_ms: float = 50.0
    preemphasis_hz: float = 50.0
    fmin_hz: float = 50.0
    max_bandwidth_hz: float = 500.0
    window: str = "hann"

    def rate(self) -> int:
        """the rate the audio is analysed at, 2 * max_formant_hz, which must be a whole number of Hz"""
        r = 2.0 * float(self.max_formant_hz)
        if not (math.isfinite(r) and r >= 1.0 and r == int(r)):
            raise ValueError("2 * max_formant_hz must be a whole number of Hz, at least 1")
        return int(r)

    def window_samples(self, sample_rate: int) -> int:
        """W at sample_rate: window_ms * sample_rate / 1000 rounded down to even"""
        if not math.isfinite(float(self.window_ms)):
            raise ValueError("window_ms is not finite")
        return int(float(self.window_ms) * int(sample_rate) / 1000.0) // 2 * 2

    def c_struct(self, sample_rate: int) -> MT2FormantConfig:
        if self.window not in FORMANT_WINDOWS:
            raise ValueError('window must be "hann" or "rect"')
        return MT2FormantConfig(self.window_samples(sample_rate), int(self.order), FORMANT_WINDOWS[self.window], 0, float(self.preemphasis_hz),
                                float(self.fmin_hz), float(self.max_bandwidth_hz))


class MT2FormantTrackConfig(C.Structure):
    _fields_ = [("tracks", C.c_int32), ("reserved", C.c_int32), ("ref_hz", C.c_double * 5), ("freq_cost", C.c_double), ("bw_cost", C.c_double),
                ("jump_cost", C.c_double)]


FORMANT_TRACK_STATES = 10      # MT2_FORMANT_TRACK_STATES


@dataclasses.dataclass(frozen=True)
class FormantTrack:
    """The settings of the formant tracks across frames (csrc/formant_track.hip; the rule is in include/megatts2_hip.h): of the up to five
    candidates of every frame, the `tracks` that form the cheapest smooth path through the utterance.  A candidate on track q costs
    `freq_cost` per kHz it lies from `ref_hz[q]` plus `bw_cost` times its bandwidth over its frequency; a step between frames costs
    `jump_cost` times the relative change of every track.  ref_hz None: (2 q + 1) * max_formant_hz / 10, the formants of a uniform tube
    scaled to the ceiling - Praat's 550, 1650, 2750, ... at 5500 Hz.  In the manner of Praat's "Formant: Track" (Xia and Espy-Wilson
    2000) with a rule of our own; parity with Praat is unpinned."""
    tracks: int = 4
    ref_hz: Optional[Sequence[float]] = None
    freq_cost: float = 1.0
    bw_cost: float = 1.0
    jump_cost: float = 1.0

    def c_struct(self, max_formant_hz: float = 5500.0) -> MT2FormantTrackConfig:
        ref = [(2 * q + 1) * float(max_formant_hz) / 10.0 for q in range(FORMANT_MAX)] if self.ref_hz is None else [float(r) for r in self.ref_hz]
        if len(ref) < min(max(int(self.tracks), 0), FORMANT_MAX):
            raise ValueError("ref_hz is shorter than tracks")
        ref = (ref + [0.0] * FORMANT_MAX)[:FORMANT_MAX]
        return MT2FormantTrackConfig(int(self.tracks), 0, (C.c_double * 5)(*ref), float(self.freq_cost), float(self.bw_cost), float(self.jump_cost))


class MT2SegmentsConfig(C.Structure):
    _fields_ = [("top_db", C.c_float), ("min_pause", C.c_int32), ("min_speech", C.c_int32), ("pad", C.c_int32), ("keep", C.c_int32)]


SEGMENTS_HOP = 512
SEGMENTS_KEEP = {"speech": 0, "pauses": 1}
PAUSES_NAMES = ("frames", "raw_active", "kept_frames", "segments", "kept_samples", "longest_pause", "kept_energy", "dropped_energy")


def segments_config(top_db: float = 40.0, min_pause: int = 10, min_speech: int = 3, pad: int = 2, keep: str = "speech") -> MT2SegmentsConfig:
    """The rule of csrc/segments.hip in FRAMES of 512 samples, checked as the library checks it (ValueError)."""
    if keep not in SEGMENTS_KEEP:
        raise ValueError('keep must be "speech" or "pauses"')
    top_db, min_pause, min_speech, pad = float(top_db), int(min_pause), int(min_speech), int(pad)
    if not (math.isfinite(top_db) and top_db > 0.0):
        raise ValueError("top_db must be finite and > 0")
    if min_speech < 2:
        raise ValueError("min_speech < 2 frames")
    if pad < 0:
        raise ValueError("pad < 0")
    if min_pause <= 2 * pad:
        raise ValueError("min_pause <= 2 pad (padded segments could touch; no merge step exists)")
    if max(min_pause, min_speech, pad) > 2 ** 31 - 1:
        raise ValueError("a frame count beyond int32")
    return MT2SegmentsConfig(top_db, min_pause, min_speech, pad, SEGMENTS_KEEP[keep])


@dataclasses.dataclass(frozen=True)
class Pauses:
    """The settings of the speech segments by frame energy (csrc/segments.hip; the rule is in include/megatts2_hip.h): a frame of 2048
    samples every 512 is active while its energy is above the loudest frame's * 10^(-`top_db` / 10); pauses between active frames
    shorter than `min_pause_ms` are closed, runs shorter than `min_speech_ms` are dropped, and what is left is widened by `pad_ms` on
    both sides.  Each duration becomes frames by round(ms * rate / 512000) at the rate of the audio it is applied to.  The threshold is
    relative to the LOUDEST frame: room tone above -top_db of the peak reads as speech and nothing is cut; a breath is speech or pause
    by its level alone; a weak consonant at a segment's edge is protected only by the pad."""
    top_db: float = 40.0
    min_pause_ms: float = 320.0
    min_speech_ms: float = 96.0
    pad_ms: float = 64.0

    def frames(self, sample_rate: int):
        """(min_pause, min_speech, pad) in frames at sample_rate"""
        if int(sample_rate) < 1:
            raise ValueError("sample_rate < 1")
        return tuple(int(round(float(ms) * int(sample_rate) / (1000.0 * SEGMENTS_HOP))) for ms in (self.min_pause_ms, self.min_speech_ms, self.pad_ms))

    def c_struct(self, sample_rate: int, keep: str = "speech") -> MT2SegmentsConfig:
        for ms in (self.min_pause_ms, self.min_speech_ms, self.pad_ms):
            if not math.isfinite(float(ms)):
                raise ValueError("a duration that is not finite")
        mp, ms, pad = self.frames(sample_rate)
        return segments_config(self.top_db, mp, ms, pad, keep)


def segments_bound(F: int, min_pause: int, min_speech: int) -> int:
    """the most segments an utterance of F frames can have: max(1, (F + min_pause) // (min_speech + min_pause))"""
    return max(1, (int(F) + int(min_pause)) // (int(min_speech) + int(min_pause)))


class MT2Config(C.Structure):
    _fields_ = [
        ("mel_bins", C.c_int32), ("mrte_hidden", C.c_int32), ("mrte_kernel", C.c_int32), ("mrte_stride", C.c_int32),
        ("mrte_n_layer", C.c_int32), ("mrte_n_stack", C.c_int32), ("mrte_n_block", C.c_int32),
        ("content_ff_dim", C.c_int32), ("content_n_heads", C.c_int32), ("content_n_layers", C.c_int32),
        ("phone_vocab", C.c_int32),
        ("vq_mel_bins", C.c_int32), ("vq_stride", C.c_int32), ("vq_hidden", C.c_int32), ("vq_kernel", C.c_int32),
        ("vq_n_layers", C.c_int32), ("vq_n_stacks", C.c_int32), ("vq_n_blocks", C.c_int32), ("vq_bins", C.c_int32),
        ("vq_dim", C.c_int32),
        ("dec_kernel", C.c_int32), ("dec_hidden", C.c_int32), ("dec_n_stack", C.c_int32), ("dec_n_block", C.c_int32),
        ("plm_layers", C.c_int32), ("plm_heads", C.c_int32), ("plm_vq_dim", C.c_int32), ("plm_tc_dim", C.c_int32),
        ("plm_bins", C.c_int32),
        ("adm_layers", C.c_int32), ("adm_heads", C.c_int32), ("adm_emb_dim", C.c_int32), ("adm_tc_dim", C.c_int32),
        ("adm_tc_emb_dim", C.c_int32),
        ("hg_in_dim", C.c_int32), ("hg_init_channels", C.c_int32), ("hg_n_up", C.c_int32),
        ("hg_up_rates", C.c_int32 * 8), ("hg_up_kernels", C.c_int32 * 8),
        ("hg_n_res", C.c_int32), ("hg_res_kernels", C.c_int32 * 4), ("hg_res_dilations", (C.c_int32 * 3) * 4),
        ("hg_slope", C.c_float),
        ("max_positions", C.c_int32),
        ("hg_inference_padding", C.c_int32),
        ("hg_reflect_pad", C.c_int32),
    ]


class MT2AudioConfig(C.Structure):
    _fields_ = [("sample_rate", C.c_int32), ("n_fft", C.c_int32), ("hop_length", C.c_int32),
                ("win_length", C.c_int32), ("n_mels", C.c_int32),
                ("f_min", C.c_float), ("f_max", C.c_float), ("clip", C.c_float)]


def library_path() -> str:
    return os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib", "libmegatts2_hip.so")


def load_library():
    """dlopen the HIP library (building it with hipcc first if the .so is absent)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    # PyTorch-ROCm bundles its own HIP runtime: it must be the one already mapped when this library
    # resolves libamdhip64, otherwise two runtimes end up in the process (and the second sees no device).
    import torch  # noqa: F401
    path = library_path()
    if not os.path.exists(path):
        from .build import build
        build(verbose=False)
    if not os.path.exists(path):
        raise NativeError(f"{path} is missing: run `python -m megatts2_amd.build` (needs hipcc)")
    lib = C.CDLL(path)
    lib.mt2_last_error.restype = C.c_char_p
    lib.mt2_version.restype = C.c_char_p
    lib.mt2_model_create.restype = C.c_void_p
    lib.mt2_model_create.argtypes = [C.POINTER(MT2Config)]
    lib.mt2_model_destroy.argtypes = [C.c_void_p]
    lib.mt2_model_destroy.restype = None
    lib.mt2_resample_query.argtypes = [C.c_int, C.c_int, C.c_longlong] + [C.c_void_p] * 4
    lib.mt2_trim_query.argtypes = [C.c_longlong, C.c_float, C.c_void_p, C.c_void_p]
    lib.mt2_trim_silence.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_float, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.mt2_dtw_query.argtypes = [C.c_int] * 4 + [C.c_void_p]
    lib.mt2_dtw_align.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 6
    lib.mt2_align_durations.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_void_p]
    lib.mt2_mcd_table.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.mt2_mcd_query.argtypes = [C.c_int] * 5 + [C.c_void_p]
    lib.mt2_mel_cepstrum.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p]
    lib.mt2_path_distortion.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.mt2_mel_cepstral_distortion.argtypes = ([C.c_void_p] * 4 + [C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int]
                                                + [C.c_void_p] * 5)
    lib.mt2_denoise_query.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.mt2_noise_floor.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    lib.mt2_spectral_gain.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    lib.mt2_denoise.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 4 + [C.c_int]
    lib.mt2_dereverb_query.argtypes = [C.c_void_p] * 3 + [C.c_int, C.c_int] + [C.c_void_p] * 2
    lib.mt2_wpe_spectrum.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    lib.mt2_dereverb.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 2 + [C.c_int]
    lib.mt2_declip_query.argtypes = [C.c_void_p] * 2 + [C.c_int, C.c_int] + [C.c_void_p] * 3
    lib.mt2_clip_detect.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p]
    lib.mt2_declip.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.mt2_segments_query.argtypes = [C.c_void_p] * 2 + [C.c_int, C.c_int] + [C.c_void_p] * 4
    lib.mt2_segment_frames.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.mt2_speech_segments.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 3 + [C.c_int]
    lib.mt2_cut_pauses.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    lib.mt2_stft.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.mt2_istft.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.mt2_mel_to_linear.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_void_p]
    lib.mt2_griffin_lim_query.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_double, C.c_int, C.c_void_p, C.c_void_p]
    lib.mt2_griffin_lim.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
    lib.mt2_f0_query.argtypes = [C.c_int, C.c_int, C.c_float, C.c_float, C.c_longlong] + [C.c_void_p] * 4
    lib.mt2_f0_yin.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float] * 3 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    lib.mt2_f0_track_query.argtypes = [C.c_int, C.c_int] + [C.c_float] * 4 + [C.c_longlong, C.c_int] + [C.c_void_p] * 5
    lib.mt2_f0_track.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_float] * 5 + [C.c_void_p] * 3 + [C.c_int, C.c_void_p]
    lib.mt2_f0_stats.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p]
    lib.mt2_formant_query.argtypes = [C.c_int] * 4 + [C.c_longlong, C.c_void_p, C.c_void_p]
    lib.mt2_formant_window.argtypes = [C.c_int, C.c_int, C.c_void_p]
    lib.mt2_lpc_formants.argtypes = [C.c_void_p] * 4 + [C.c_int] * 4 + [C.c_void_p] * 4 + [C.c_int] + [C.c_void_p] * 5
    lib.mt2_formant_stats.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int, C.c_void_p]
    lib.mt2_formant_track_query.argtypes = [C.c_int, C.c_longlong, C.c_int, C.c_void_p, C.c_void_p]
    lib.mt2_formant_track.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_int] + [C.c_void_p] * 5
    lib.mt2_frame_energy.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int]
    lib.mt2_phone_prosody.argtypes = [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p]
    lib.mt2_pitch_contour.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int] + [C.c_void_p] * 3
    lib.mt2_loudness_query.argtypes = [C.c_int, C.c_longlong] + [C.c_void_p] * 4
    lib.mt2_loudness.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int]
    lib.mt2_loudness_normalize.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.mt2_ebu_query.argtypes = [C.c_int, C.c_longlong] + [C.c_void_p] * 5
    lib.mt2_true_peak_table.argtypes = [C.c_int, C.c_void_p]
    lib.mt2_loudness_ebu.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    lib.mt2_loudness_normalize_tp.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p]
    lib.mt2_limiter_query.argtypes = [C.c_int, C.c_longlong, C.c_double] + [C.c_void_p] * 3
    lib.mt2_limiter_window.argtypes = [C.c_int, C.c_double, C.c_void_p]
    lib.mt2_limit_true_peak.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int] + [C.c_double] * 3 + [C.c_void_p] * 4
    lib.mt2_loudness_normalize_limited.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_int] + [C.c_double] * 3 + [C.c_int] + [C.c_void_p] * 4
    lib.mt2_workspace_fill.argtypes = [C.c_void_p, C.c_int]
    lib.mt2_workspace_peek.argtypes = [C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t]
    _LIB = lib
    return lib


def _check(rc: int) -> None:
    if rc != 0:
        raise NativeError(load_library().mt2_last_error().decode(errors="replace"))


def device_check() -> None:
    _check(load_library().mt2_device_check())


def make_config(g: Optional[cfgmod.GConfig], plm: Optional[cfgmod.PLMConfig], adm: Optional[cfgmod.ADMConfig],
                hg: Optional[cfgmod.HifiGanConfig], max_positions: int = MAX_POSITIONS) -> MT2Config:
    g = g or cfgmod.production_g()
    plm = plm or cfgmod.production_plm()
    adm = adm or cfgmod.production_adm()
    hg = hg or cfgmod.production_hifigan()
    c = MT2Config()
    m, v = g.mrte, g.vqpe
    c.mel_bins, c.mrte_hidden, c.mrte_kernel, c.mrte_stride = m.mel_bins, m.hidden_size, m.mel_kernel_size, m.mel_stride
    c.mrte_n_layer, c.mrte_n_stack, c.mrte_n_block = m.mel_n_layer, m.mel_n_stack, m.mel_n_block
    c.content_ff_dim, c.content_n_heads, c.content_n_layers = m.content_ff_dim, m.content_n_heads, m.content_n_layers
    c.phone_vocab = m.phone_vocab_size
    c.vq_mel_bins, c.vq_stride, c.vq_hidden, c.vq_kernel = v.mel_bins, v.stride, v.hidden_size, v.kernel_size
    c.vq_n_layers, c.vq_n_stacks, c.vq_n_blocks, c.vq_bins, c.vq_dim = v.n_layers, v.n_stacks, v.n_blocks, v.vq_bins, v.vq_dim
    c.dec_kernel, c.dec_hidden, c.dec_n_stack, c.dec_n_block = g.kernel_size, g.hidden_size, g.decoder_n_stack, g.decoder_n_block
    c.plm_layers, c.plm_heads, c.plm_vq_dim, c.plm_tc_dim, c.plm_bins = plm.n_layers, plm.n_heads, plm.vq_dim, plm.tc_latent_dim, plm.vq_bins
    c.adm_layers, c.adm_heads, c.adm_emb_dim, c.adm_tc_dim, c.adm_tc_emb_dim = adm.n_layers, adm.n_heads, adm.emb_dim, adm.tc_latent_dim, adm.tc_emb_dim
    c.hg_in_dim, c.hg_init_channels, c.hg_n_up = hg.in_dim, hg.upsample_initial_channel, len(hg.upsample_rates)
    for i, (r, k) in enumerate(zip(hg.upsample_rates, hg.upsample_kernel_sizes)):
        c.hg_up_rates[i], c.hg_up_kernels[i] = r, k
    c.hg_n_res = len(hg.resblock_kernel_sizes)
    for j, (k, dils) in enumerate(zip(hg.resblock_kernel_sizes, hg.resblock_dilation_sizes)):
        c.hg_res_kernels[j] = k
        for n, d in enumerate(dils):
            c.hg_res_dilations[j][n] = d
    c.hg_slope = hg.leaky_relu_slope
    c.max_positions = max_positions
    c.hg_inference_padding = int(getattr(hg, "inference_padding", 0))
    c.hg_reflect_pad = 1 if getattr(hg, "pad_mode", "zeros") == "reflect" else 0
    return c


def sine_table(n: int, dim: int, alpha: float) -> np.ndarray:
    """alpha * pe[:n] of SinePositionalEmbedding (reference modules/embedding.py:68-98), computed with
    the same torch fp32 ops the reference uses so that the table is bit-identical to its `self.pe`."""
    import torch

    position = torch.arange(0, n, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, dim, 2, dtype=torch.float32) * -(math.log(10000.0) / dim))
    pe = torch.zeros(n, dim)
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return (float(alpha) * pe).numpy()


def _i32(a) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(a, dtype=np.int32))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _iptr(a: Optional[np.ndarray]):
    return a.ctypes.data_as(C.c_void_p) if a is not None else C.c_void_p(0)


def _stream() -> C.c_void_p:
    import torch
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _dtw(lib, h, X, Y, x_lens=None, y_lens=None, return_cost: bool = False, return_acc: bool = False):
    """mt2_dtw_align on the handle `h` (NativeModel.dtw and MelFrontEnd.dtw): X f32 [B, Tx, D] warped onto Y f32 [B, Ty, D] by the
    rule of csrc/dtw.hip -> dict of device tensors: lo, hi int32 [B, Ty] (the smallest / largest row of X on the path in each
    column of Y; -1 at or beyond y_lens[b]), steps int32 [B] (cells on the path), total f32 [B] (the DTW distance A[Tx-1, Ty-1]),
    and on request cost / acc f32 [B, Tx, Ty] (zeros outside an utterance's own cells).  Rows beyond the lengths are never read.
    The call only enqueues."""
    import torch
    assert X.is_cuda and Y.is_cuda and X.dim() == 3 and Y.dim() == 3 and X.shape[0] == Y.shape[0] and X.shape[2] == Y.shape[2]
    X, Y = X.contiguous().to(torch.float32), Y.contiguous().to(torch.float32)
    B, Tx, D = X.shape
    Ty = Y.shape[1]
    xl = np.full(B, Tx, np.int32) if x_lens is None else _i32(x_lens)
    yl = np.full(B, Ty, np.int32) if y_lens is None else _i32(y_lens)
    assert xl.shape == (B,) and yl.shape == (B,)
    dev = X.device
    out = {"lo": torch.empty(B, Ty, device=dev, dtype=torch.int32), "hi": torch.empty(B, Ty, device=dev, dtype=torch.int32),
           "steps": torch.empty(B, device=dev, dtype=torch.int32), "total": torch.empty(B, device=dev, dtype=torch.float32)}
    if return_cost:
        out["cost"] = torch.zeros(B, Tx, Ty, device=dev, dtype=torch.float32)
    if return_acc:
        out["acc"] = torch.zeros(B, Tx, Ty, device=dev, dtype=torch.float32)
    _check(lib.mt2_dtw_align(h, _stream(), _ptr(X), _iptr(xl), Tx, _ptr(Y), _iptr(yl), Ty, D, B, _ptr(out["lo"]), _ptr(out["hi"]),
                             _ptr(out["steps"]), _ptr(out["total"]), _ptr(out.get("cost")), _ptr(out.get("acc"))))
    return out


def _rows_lens(x, lens, what: str):
    """x f32 [B, T, W] on the device, lens int [B] or None (every row whole) -> (x contiguous f32, lens int32 [B])"""
    import torch
    assert x.is_cuda and x.dim() == 3, what
    x = x.contiguous().to(torch.float32)
    ln = np.full(x.shape[0], x.shape[1], np.int32) if lens is None else _i32(lens)
    assert ln.shape == (x.shape[0],), what
    return x, ln


def _f0_pair(f0_a, f0_b, B: int, Ta: int, Tb: int):
    import torch
    if f0_a is None and f0_b is None:
        return None, None
    if f0_a is not None:
        assert f0_a.is_cuda and tuple(f0_a.shape) == (B, Ta)
        f0_a = f0_a.contiguous().to(torch.float32)
    if f0_b is not None:      # one track without the other goes to the library, which refuses it
        assert f0_b.is_cuda and tuple(f0_b.shape) == (B, Tb)
        f0_b = f0_b.contiguous().to(torch.float32)
    return f0_a, f0_b


def _mel_cepstrum(lib, h, mel, frame_lens=None, order: int = 13):
    """mt2_mel_cepstrum on the handle `h`: mel f32 [B, T, N] (natural-log mel, time-major, device) -> cep f32 [B, T, order] by the
    rule of csrc/mcd.hip: c[t][k-1] = sum_m mel[t][m] cos(pi (m + 1/2) k / N) / N, one f32 fma chain; c0 is left out.  Rows at or beyond
    frame_lens[b] are never read and give zeros.  The call only enqueues."""
    import torch
    mel, fl = _rows_lens(mel, frame_lens, "mel f32 [B, T, N]")
    B, T, N = mel.shape
    cep = torch.empty(B, T, int(order), device=mel.device, dtype=torch.float32)
    _check(lib.mt2_mel_cepstrum(h, _stream(), _ptr(mel), _iptr(fl), T, B, N, int(order), _ptr(cep)))
    return cep


def _path_distortion(lib, h, ca, cb, lo, hi, a_lens=None, b_lens=None, f0_a=None, f0_b=None):
    """mt2_path_distortion on the handle `h`: cepstra ca f32 [B, Ta, K], cb f32 [B, Tb, K] and a path lo, hi int32 [B, Tb] (device, as
    `dtw` returns them) -> float64 [B, 8] (device): cells, MCD in dB, largest cell dB, cells voiced on both sides, F0 RMSE in cents,
    mean F0 difference in cents, cells voiced on one side, that over the cells; the last five are 0 without f0_a f32 [B, Ta] and f0_b
    f32 [B, Tb].  The call only enqueues."""
    import torch
    ca, al = _rows_lens(ca, a_lens, "ca f32 [B, Ta, K]")
    cb, bl = _rows_lens(cb, b_lens, "cb f32 [B, Tb, K]")
    B, Ta, K = ca.shape
    Tb = cb.shape[1]
    assert cb.shape[0] == B and cb.shape[2] == K
    lo, hi = (t.to(ca.device, torch.int32).contiguous() for t in (lo, hi))
    assert tuple(lo.shape) == (B, Tb) and tuple(hi.shape) == (B, Tb)
    f0_a, f0_b = _f0_pair(f0_a, f0_b, B, Ta, Tb)
    out = torch.empty(B, MCD_FIELDS, device=ca.device, dtype=torch.float64)
    _check(lib.mt2_path_distortion(h, _stream(), _ptr(ca), _iptr(al), Ta, _ptr(cb), _iptr(bl), Tb, K, B, _ptr(lo), _ptr(hi), _ptr(f0_a),
                                   _ptr(f0_b), _ptr(out)))
    return out


def _mcd(lib, h, mel_a, mel_b, a_lens=None, b_lens=None, f0_a=None, f0_b=None, order: int = 13, return_path: bool = False):
    """mt2_mel_cepstral_distortion on the handle `h`: the cepstra of mel_a f32 [B, Ta, N] and mel_b f32 [B, Tb, N], the DTW of
    csrc/dtw.hip on them and the path reduction, in one call -> float64 [B, 8] (device; the fields of `_path_distortion`), with
    return_path (row, lo, hi), the path int32 [B, Tb].  The call only enqueues."""
    import torch
    mel_a, al = _rows_lens(mel_a, a_lens, "mel_a f32 [B, Ta, N]")
    mel_b, bl = _rows_lens(mel_b, b_lens, "mel_b f32 [B, Tb, N]")
    B, Ta, N = mel_a.shape
    Tb = mel_b.shape[1]
    assert mel_b.shape[0] == B and mel_b.shape[2] == N
    f0_a, f0_b = _f0_pair(f0_a, f0_b, B, Ta, Tb)
    out = torch.empty(B, MCD_FIELDS, device=mel_a.device, dtype=torch.float64)
    lo = torch.empty(B, Tb, device=mel_a.device, dtype=torch.int32) if return_path else None
    hi = torch.empty(B, Tb, device=mel_a.device, dtype=torch.int32) if return_path else None
    _check(lib.mt2_mel_cepstral_distortion(h, _stream(), _ptr(mel_a), _iptr(al), Ta, _ptr(mel_b), _iptr(bl), Tb, N, int(order), B,
                                           _ptr(f0_a), _ptr(f0_b), _ptr(out), _ptr(lo), _ptr(hi)))
    return (out, lo, hi) if return_path else out


def _audio_struct(audio) -> MT2AudioConfig:
    a = audio or cfgmod.AudioConfig()
    return MT2AudioConfig(a.sample_rate, a.n_fft, a.hop_length, a.win_length, a.n_mels, a.f_min, a.f_max, a.clip)


def _packed_spec(spec, F: int):
    """A spectrum as mt2_stft lays it out: complex64 [B, T, F] -> a new f32 [B, T, S] = [re | im | zero pad];  f32 [B, T, S] as it is."""
    import torch
    S = (2 * F + 3) & ~3
    assert spec.is_cuda and spec.dim() == 3
    if spec.is_complex():
        assert spec.shape[2] == F
        packed = torch.zeros(spec.shape[0], spec.shape[1], S, device=spec.device, dtype=torch.float32)
        packed[..., :F] = spec.real
        packed[..., F:2 * F] = spec.imag
        return packed
    assert spec.dtype == torch.float32 and spec.shape[2] == S and spec.is_contiguous()
    return spec


def _noise_floor(lib, h, ac, spec, frame_lens=None, denoise: Optional[Denoise] = None):
    """mt2_noise_floor on the handle `h`: a spectrum (complex64 [B, T, F], or f32 [B, T, S] in mt2_stft's layout; device) -> the noise
    floor f32 [B, F] (device): per bin the `percentile`-th percentile of the power over the frames below frame_lens[b], selected
    exactly, times the quantile-to-mean factor.  On a noise-only clip this is a noise profile for `denoise(..., noise_floor=)`."""
    import torch
    F = ac.n_fft // 2 + 1
    packed = _packed_spec(spec, F)
    B, T, _ = packed.shape
    ln = np.full(B, T, np.int32) if frame_lens is None else _i32(frame_lens)
    assert ln.shape == (B,)
    dc = (denoise or Denoise()).c_struct()
    floor = torch.empty(B, (F + 3) & ~3, device=packed.device, dtype=torch.float32)
    _check(lib.mt2_noise_floor(h, _stream(), C.byref(ac), C.byref(dc), _ptr(packed), _iptr(ln), T, B, _ptr(floor)))
    return floor[:, :F]


def _floor_arg(floor, B: int, F: int):
    """A caller's floor f32 [B, F] or [B, Fp] (device) as the contiguous [B, Fp] the library reads."""
    import torch
    Fp = (F + 3) & ~3
    assert floor.is_cuda and floor.dim() == 2 and floor.shape[0] == B and floor.shape[1] in (F, Fp)
    if floor.shape[1] == Fp and floor.is_contiguous() and floor.dtype == torch.float32:
        return floor
    full = torch.zeros(B, Fp, device=floor.device, dtype=torch.float32)
    full[:, :floor.shape[1]] = floor
    return full


def _spectral_gain(lib, h, ac, spec, floor, frame_lens=None, denoise: Optional[Denoise] = None, return_gain: bool = True,
                   apply: bool = False, in_place: bool = False):
    """mt2_spectral_gain on the handle `h`: a spectrum (as `_noise_floor`) and a floor f32 [B, F] -> the smoothed gain f32 [B, T, F]
    (zeros in frames at or beyond frame_lens[b]) and / or, with apply, the gated spectrum in the form the spectrum came in (in_place:
    written over an f32 [B, T, S] spectrum itself).  -> gain, gated, or (gain, gated)."""
    import torch
    assert return_gain or apply
    F = ac.n_fft // 2 + 1
    packed = _packed_spec(spec, F)
    B, T, S = packed.shape
    ln = np.full(B, T, np.int32) if frame_lens is None else _i32(frame_lens)
    assert ln.shape == (B,)
    dc = (denoise or Denoise()).c_struct()
    fl = _floor_arg(floor, B, F)
    gain = torch.empty(B, T, (F + 3) & ~3, device=packed.device, dtype=torch.float32) if return_gain else None
    gated = None
    if apply:
        assert not in_place or packed is spec, "in_place needs the f32 [B, T, S] layout"
        gated = packed if in_place else torch.empty_like(packed)
    _check(lib.mt2_spectral_gain(h, _stream(), C.byref(ac), C.byref(dc), _ptr(packed), _iptr(ln), T, B, _ptr(fl), _ptr(gain), _ptr(gated)))
    if gated is not None and spec.is_complex():
        gated = torch.complex(gated[..., :F], gated[..., F:2 * F])
    res = tuple(x for x in (gain[..., :F] if gain is not None else None, gated) if x is not None)
    return res[0] if len(res) == 1 else res


def _denoise(lib, h, ac, wav, lens=None, denoise: Optional[Denoise] = None, noise_floor=None, return_floor: bool = False,
             return_figures: bool = False, out=None):
    """mt2_denoise on the handle `h`: wav f32 [B, L] (device) -> the denoised audio f32 [B, (T - 1) * hop] with T = 1 + max lens // hop,
    utterance b holding hop * (lens[b] // hop) samples (up to hop - 1 tail samples are dropped, the Griffin-Lim convention) and zeros
    beyond; samples at or beyond lens[b] are never read.  noise_floor: f32 [B, F] (device) to gate against instead of the utterance's
    own quantile floor, e.g. `noise_floor` of a noise-only clip.  return_floor: also the floor that was used, f32 [B, F];
    return_figures: also float64 [B, 8] (device; DENOISE_NAMES).  out: a contiguous f32 [B, >= (T - 1) * hop] device tensor to write
    into (not wav).  -> (out, out_lens int32 [B][, floor][, figures]).  The call only enqueues."""
    import torch
    wav, ln, B, L = _wav_lens(wav, lens)
    hop, F = ac.hop_length, ac.n_fft // 2 + 1
    out_lens = (hop * (ln // hop)).astype(np.int32)
    out = _out_rows(out, B, wav, lambda: max(int(out_lens.max()), 1))
    dc = (denoise or Denoise()).c_struct()
    fin = None if noise_floor is None else _floor_arg(noise_floor, B, F)
    fout = torch.empty(B, (F + 3) & ~3, device=wav.device, dtype=torch.float32) if return_floor else None
    fig = torch.empty(B, len(DENOISE_NAMES), device=wav.device, dtype=torch.float64) if return_figures else None
    _check(lib.mt2_denoise(h, _stream(), C.byref(ac), C.byref(dc), _ptr(wav), _iptr(ln), L, B, _ptr(fin), _ptr(fout), _ptr(fig), _ptr(out),
                           out.shape[1]))
    res = (out, out_lens)
    if return_floor:
        res += (fout[:, :F],)
    if return_figures:
        res += (fig,)
    return res


def _wpe_spectrum(lib, h, ac, spec, frame_lens=None, dereverb: Optional[Dereverb] = None, return_filters: bool = False,
                  return_figures: bool = False, in_place: bool = False):
    """mt2_wpe_spectrum on the handle `h`: steps 1-3 of the weighted-prediction-error rule on a spectrum (complex64 [B, T, F], or f32
    [B, T, S] in mt2_stft's layout; device), at any T >= 1 -> the de-reverberated spectrum in the form it came in (in_place: written
    over an f32 [B, T, S] spectrum itself; pad columns and frames at or beyond frame_lens[b] then stay as they were, else they are
    zero).  return_filters: also the prediction filters complex128 [B, F, K] (zeros for a bin that passed through); return_figures:
    also float64 [B, 8] (device; WPE_NAMES).  -> spectrum, or (spectrum[, filters][, figures])."""
    import torch
    F = ac.n_fft // 2 + 1
    packed = _packed_spec(spec, F)
    B, T, S = packed.shape
    ln = np.full(B, T, np.int32) if frame_lens is None else _i32(frame_lens)
    assert ln.shape == (B,)
    cfg = dereverb or Dereverb()
    wc = cfg.c_struct()
    assert not in_place or packed is spec, "in_place needs the f32 [B, T, S] layout"
    out = packed if in_place else torch.empty_like(packed)
    Fp = (F + 3) & ~3
    filt = torch.empty(B, Fp, int(cfg.taps), 2, device=packed.device, dtype=torch.float64) if return_filters else None
    fig = torch.empty(B, len(WPE_NAMES), device=packed.device, dtype=torch.float64) if return_figures else None
    _check(lib.mt2_wpe_spectrum(h, _stream(), C.byref(ac), C.byref(wc), _ptr(packed), _iptr(ln), T, B, _ptr(out), _ptr(filt), _ptr(fig)))
    if spec.is_complex():
        out = torch.complex(out[..., :F], out[..., F:2 * F])
    res = (out,)
    if return_filters:
        res += (torch.view_as_complex(filt[:, :F].contiguous()),)
    if return_figures:
        res += (fig,)
    return res[0] if len(res) == 1 else res


def _dereverb(lib, h, ac, wav, lens=None, dereverb: Optional[Dereverb] = None, return_figures: bool = False, out=None):
    """mt2_dereverb on the handle `h`: wav f32 [B, L] (device) -> the de-reverberated audio f32 [B, (T - 1) * hop] with T = 1 + max lens
    // hop, utterance b holding hop * (lens[b] // hop) samples (up to hop - 1 tail samples are dropped, as `_denoise` does) and zeros
    beyond; samples at or beyond lens[b] are never read.  An utterance of fewer than delay + 4 * taps frames passes through the two
    transforms unfiltered.  return_figures: also float64 [B, 8] (device; WPE_NAMES).  out: a contiguous f32 [B, >= (T - 1) * hop]
    device tensor to write into (not wav).  -> (out, out_lens int32 [B][, figures]).  The call only enqueues."""
    import torch
    wav, ln, B, L = _wav_lens(wav, lens)
    hop = ac.hop_length
    out_lens = (hop * (ln // hop)).astype(np.int32)
    out = _out_rows(out, B, wav, lambda: max(int(out_lens.max()), 1))
    wc = (dereverb or Dereverb()).c_struct()
    fig = torch.empty(B, len(WPE_NAMES), device=wav.device, dtype=torch.float64) if return_figures else None
    _check(lib.mt2_dereverb(h, _stream(), C.byref(ac), C.byref(wc), _ptr(wav), _iptr(ln), L, B, _ptr(fig), _ptr(out), out.shape[1]))
    return (out, out_lens, fig) if return_figures else (out, out_lens)


def _clip_detect(lib, h, wav, lens=None, declip: Optional[Declip] = None):
    """mt2_clip_detect on the handle `h`: wav f32 [B, L] (device, at its own sample rate) -> figures float64 [B, 8] (device;
    DECLIP_NAMES; the last four are zero: nothing is restored).  Samples at or beyond lens[b] are never read.  The call only enqueues."""
    import torch
    wav, ln, B, L = _wav_lens(wav, lens)
    dc = (declip or Declip()).c_struct()
    fig = torch.empty(B, len(DECLIP_NAMES), device=wav.device, dtype=torch.float64)
    _check(lib.mt2_clip_detect(h, _stream(), C.byref(dc), _ptr(wav), _iptr(ln), L, B, _ptr(fig)))
    return fig


def _declip(lib, h, wav, lens=None, declip: Optional[Declip] = None, return_figures: bool = False, return_iters: bool = False, out=None):
    """mt2_declip on the handle `h`: wav f32 [B, L] (device, at its own sample rate; nothing is resampled) -> the declipped audio f32
    [B, L]: reliable samples keep their bits, a clipped sample moves outward or stays, an utterance that is not clipped (or holds a
    non-finite sample) comes back bit for bit.  The output can exceed the input's peak; the caller normalises after.  Samples at or
    beyond lens[b] are never read; in a new `out` they are the input's, in a caller's they are left untouched.  out: a contiguous f32
    [B, >= max lens] device tensor to write into (NOT wav: in place is not offered).  return_figures: also float64 [B, 8] (device;
    DECLIP_NAMES); return_iters: also int32 [B, T] (device), T = ceil(max lens / hop) + 3: the iterations of every frame.
    -> out, or (out[, figures][, iters]).  The call only enqueues."""
    import torch
    wav, ln, B, L = _wav_lens(wav, lens)
    cfg = declip or Declip()
    dc = cfg.c_struct()
    if out is None:
        out = wav.clone()
    out = _out_rows(out, B, wav, lambda: L)
    fig = torch.empty(B, len(DECLIP_NAMES), device=wav.device, dtype=torch.float64) if return_figures else None
    T = cfg.frames(int(ln.max())) if int(cfg.frame) >= 4 and len(ln) else 1
    it = torch.empty(B, T, device=wav.device, dtype=torch.int32) if return_iters else None
    _check(lib.mt2_declip(h, _stream(), C.byref(dc), _ptr(wav), _iptr(ln), L, B, _ptr(out), out.shape[1], _ptr(fig), _ptr(it), T))
    res = (out,)
    if return_figures:
        res += (fig,)
    if return_iters:
        res += (it,)
    return res[0] if len(res) == 1 else res


def _segments_cfg(pauses, sample_rate: int, keep: str) -> MT2SegmentsConfig:
    """a `Pauses` (durations, turned into frames at sample_rate), None (its defaults) or an MT2SegmentsConfig in frames (segments_config),
    whose own `keep` then stands"""
    if isinstance(pauses, MT2SegmentsConfig):
        return pauses
    return (pauses or Pauses()).c_struct(sample_rate, keep)


def _segment_frames(lib, h, energy, frame_lens=None, pauses=None, sample_rate: int = 16000, keep: str = "speech"):
    """mt2_segment_frames on the handle `h`, the staged form of the rule: energy f32 [B, F] (device; any contour >= 0, e.g. from
    `frame_energy`), frame_lens int [B] (every row F by default) -> dict of device tensors: flags uint8 [B, F] (d; bytes at or beyond
    frame_lens[b] are zero), segments int32 [B, S, 2] (FRAMES [f0, f1 + 1); -1 behind counts[b]; S = the bound of the rule), counts
    int32 [B], figures float64 [B, 8] (PAUSES_NAMES).  The call only enqueues."""
    import torch
    assert energy.is_cuda and energy.dim() == 2
    energy = energy.contiguous().to(torch.float32)
    B, F = energy.shape
    fl = np.full(B, F, np.int32) if frame_lens is None else _i32(frame_lens)
    assert fl.shape == (B,)
    cfg = _segments_cfg(pauses, sample_rate, keep)
    S = segments_bound(int(fl.max()) if B else 1, cfg.min_pause, cfg.min_speech)
    dev = energy.device
    out = {"flags": torch.zeros(B, F, device=dev, dtype=torch.uint8), "segments": torch.empty(B, S, 2, device=dev, dtype=torch.int32),
           "counts": torch.empty(B, device=dev, dtype=torch.int32), "figures": torch.empty(B, len(PAUSES_NAMES), device=dev, dtype=torch.float64)}
    _check(lib.mt2_segment_frames(h, _stream(), C.byref(cfg), _ptr(energy), _iptr(fl), F, B, _ptr(out["flags"]), _ptr(out["segments"]), S,
                                  _ptr(out["counts"]), _ptr(out["figures"])))
    return out


def _speech_segments(lib, h, wav, lens=None, pauses=None, sample_rate: int = 16000, keep: str = "speech", return_energy: bool = False):
    """mt2_speech_segments on the handle `h`: wav f32 [B, L] (device, at sample_rate; nothing is resampled) -> dict of device tensors:
    segments int32 [B, S, 2] (SAMPLES [start, end); -1 behind counts[b]), counts int32 [B], figures float64 [B, 8] (PAUSES_NAMES) and,
    on request, energy f32 [B, 1 + max lens // 512].  Samples at or beyond lens[b] are never read.  The call only enqueues."""
    import torch
    wav, ln, B, L = _wav_lens(wav, lens)
    cfg = _segments_cfg(pauses, sample_rate, keep)
    F = 1 + max(int(ln.max()), 0) // SEGMENTS_HOP
    S = segments_bound(F, cfg.min_pause, cfg.min_speech)
    dev = wav.device
    out = {"segments": torch.empty(B, S, 2, device=dev, dtype=torch.int32), "counts": torch.empty(B, device=dev, dtype=torch.int32),
           "figures": torch.empty(B, len(PAUSES_NAMES), device=dev, dtype=torch.float64)}
    if return_energy:
        out["energy"] = torch.empty(B, F, device=dev, dtype=torch.float32)
    _check(lib.mt2_speech_segments(h, _stream(), C.byref(cfg), _ptr(wav), _iptr(ln), L, B, _ptr(out["segments"]), S, _ptr(out["counts"]),
                                   _ptr(out["figures"]), _ptr(out.get("energy")), F))
    return out


def _cut_pauses(lib, h, wav, lens=None, pauses=None, sample_rate: int = 16000, keep: str = "speech", out=None, return_segments: bool = False,
                return_figures: bool = False):
    """mt2_cut_pauses on the handle `h`: wav f32 [B, L] (device, at sample_rate) -> (out f32 [B, max lens], out_lens int32 [B]): the
    kept frames of each utterance - its speech segments, or with keep = "pauses" everything else: a noise-only clip - moved together,
    every sample an exact copy, zeros behind out_lens[b] (which may be 0 with keep = "pauses").  No cross-fade; every join is a multiple
    of 512 samples.  out: a contiguous f32 [B, >= max lens] device tensor to write into (not wav).  return_segments: also segments
    int32 [B, S, 2] (device; samples of the INPUT, -1 behind counts) and counts int32 [B] (device); return_figures: also float64 [B, 8]
    (device; PAUSES_NAMES).  The call waits for the device once, for out_lens."""
    import torch
    wav, ln, B, L = _wav_lens(wav, lens)
    cfg = _segments_cfg(pauses, sample_rate, keep)
    out = _out_rows(out, B, wav, lambda: max(int(ln.max()), 1))
    F = 1 + max(int(ln.max()), 0) // SEGMENTS_HOP
    S = segments_bound(F, cfg.min_pause, cfg.min_speech)
    seg = torch.empty(B, S, 2, device=wav.device, dtype=torch.int32) if return_segments else None
    cnt = torch.empty(B, device=wav.device, dtype=torch.int32) if return_segments else None
    fig = torch.empty(B, len(PAUSES_NAMES), device=wav.device, dtype=torch.float64) if return_figures else None
    out_lens = np.zeros(B, np.int32)
    _check(lib.mt2_cut_pauses(h, _stream(), C.byref(cfg), _ptr(wav), _iptr(ln), L, B, _ptr(out), out.shape[1], _iptr(out_lens), _ptr(seg), S,
                              _ptr(cnt), _ptr(fig)))
    res = (out, out_lens)
    if return_segments:
        res += (seg, cnt)
    if return_figures:
        res += (fig,)
    return res


def _formant_cfg(cfg, sample_rate: int) -> MT2FormantConfig:
    """a `Formants` (its window in samples at sample_rate; max_formant_hz is extract_formants' affair), None (its defaults) or an
    MT2FormantConfig as it stands"""
    if isinstance(cfg, MT2FormantConfig):
        return cfg
    return (cfg or Formants()).c_struct(sample_rate)


def _formants(lib, h, wav, lens=None, cfg=None, hop: int = 256, sample_rate: int = 16000, return_lpc: bool = False, return_err: bool = False,
              return_autocorr: bool = False, return_roots: bool = False, return_iters: bool = False, out=None):
    """mt2_lpc_formants on the handle `h`: wav f32 [B, L] (device, at sample_rate; nothing is resampled) -> dict of device tensors: freq
    and bw f32 [B, T, 5] (Hz; the candidates of every frame in ascending frequency, zeros behind count), count int32 [B, T], with T =
    1 + max lens // hop; frames behind an utterance's own 1 + lens[b] // hop hold zeros.  At the mel's hop and rate freq[b, t] belongs
    to mel frame t.  On request lpc f64 [B, T, P + 1], err f64 [B, T], autocorr f64 [B, T, P + 1], roots complex128 [B, T, P] and iters
    int32 [B, T] (-1: an empty frame).  out: a contiguous f32 [B, T', 5] (or [B, 5 T']) device tensor to write freq into, T' >= T; every
    other output then has T' rows.  Samples at or beyond lens[b] are never read.  The call only enqueues (the first one with a new
    window uploads its table)."""
    import torch
    wav, ln, B, L = _wav_lens(wav, lens)
    hop, sr = int(hop), int(sample_rate)
    c = _formant_cfg(cfg, sr)
    if out is not None:
        assert out.is_contiguous() and out.numel() % (B * FORMANT_MAX) == 0
        out = out.view(B, -1)
    freq = _out_rows(out, B, wav, lambda: FORMANT_MAX * (1 + max(int(ln.max()), 0) // max(hop, 1)))
    T, P, dev = freq.shape[1] // FORMANT_MAX, int(c.order), wav.device
    assert freq.shape[1] == T * FORMANT_MAX
    res = {"freq": freq.view(B, T, FORMANT_MAX), "bw": torch.empty(B, T, FORMANT_MAX, device=dev, dtype=torch.float32),
           "count": torch.empty(B, T, device=dev, dtype=torch.int32)}
    if return_lpc:
        res["lpc"] = torch.empty(B, T, P + 1, device=dev, dtype=torch.float64)
    if return_err:
        res["err"] = torch.empty(B, T, device=dev, dtype=torch.float64)
    if return_autocorr:
        res["autocorr"] = torch.empty(B, T, P + 1, device=dev, dtype=torch.float64)
    roots = torch.empty(B, T, max(P, 0), 2, device=dev, dtype=torch.float64) if return_roots else None
    if return_iters:
        res["iters"] = torch.empty(B, T, device=dev, dtype=torch.int32)
    _check(lib.mt2_lpc_formants(h, _stream(), _ptr(wav), _iptr(ln), L, B, sr, hop, C.byref(c), _ptr(res["freq"]), _ptr(res["bw"]),
                                _ptr(res["count"]), T, _ptr(res.get("lpc")), _ptr(res.get("err")), _ptr(res.get("autocorr")), _ptr(roots),
                                _ptr(res.get("iters"))))
    if roots is not None:
        res["roots"] = torch.view_as_complex(roots)
    return res


def _formant_stats(lib, h, freq, count, f0, ln):
    """mt2_formant_stats on the handle `h`: freq f32 [B, T, 5], count int32 [B, T][, f0 f32 [B, T]] (device), ln int32 [B] -> float64
    [B, 12] (device; FORMANT_STAT_NAMES)."""
    import torch
    assert freq.is_cuda and freq.dim() == 3 and freq.shape[2] == FORMANT_MAX and count.is_cuda and count.shape == freq.shape[:2]
    freq, count = freq.contiguous().to(torch.float32), count.contiguous().to(torch.int32)
    B, T = count.shape
    if f0 is not None:
        assert f0.is_cuda and f0.shape == count.shape
        f0 = f0.contiguous().to(torch.float32)
    stats = torch.empty(B, FORMANT_STAT_FIELDS, device=freq.device, dtype=torch.float64)
    _check(lib.mt2_formant_stats(h, _stream(), _ptr(freq), _ptr(count), _ptr(f0), _iptr(ln), T, B, _ptr(stats)))
    return stats


def _formant_track_cfg(track, max_formant_hz: float) -> MT2FormantTrackConfig:
    """a `FormantTrack` (its ref_hz at max_formant_hz), None (its defaults) or an MT2FormantTrackConfig as it stands"""
    if isinstance(track, MT2FormantTrackConfig):
        return track
    return (track or FormantTrack()).c_struct(max_formant_hz)


def _formant_track(lib, h, freq, bw, count, ln, track=None, max_formant_hz: float = 5500.0, return_sel: bool = True):
    """mt2_formant_track on the handle `h`: freq, bw f32 [B, T, 5], count int32 [B, T] (device, as `_formants` returned them), ln int32
    [B] -> dict of device tensors: track_freq, track_bw f32 [B, T, 5], track_count int32 [B, T] - the candidates' own layout, so
    `_formant_stats` reads them unchanged - and sel int32 [B, T, 5] (the candidate slot of every track, -1 behind; None when not asked
    for).  A frame without `tracks` sound candidates, and every frame behind ln[b], has zeros, count 0 and sel -1.  The call only
    enqueues."""
    import torch
    assert freq.is_cuda and freq.dim() == 3 and freq.shape[2] == FORMANT_MAX and bw.is_cuda and bw.shape == freq.shape
    assert count.is_cuda and count.shape == freq.shape[:2]
    freq, bw, count = freq.contiguous().to(torch.float32), bw.contiguous().to(torch.float32), count.contiguous().to(torch.int32)
    B, T = count.shape
    c = _formant_track_cfg(track, max_formant_hz)
    res = {"track_freq": torch.empty_like(freq), "track_bw": torch.empty_like(bw), "track_count": torch.empty_like(count),
           "sel": torch.empty(B, T, FORMANT_MAX, device=freq.device, dtype=torch.int32) if return_sel else None}
    _check(lib.mt2_formant_track(h, _stream(), _ptr(freq), _ptr(bw), _ptr(count), _iptr(ln), T, B, C.byref(c), _ptr(res["track_freq"]),
                                 _ptr(res["track_bw"]), _ptr(res["track_count"]), _ptr(res["sel"])))
    return res


def _workspace_fill(lib, h, byte: int) -> None:
    """mt2_workspace_fill (test hook): every byte of the handle's arena := byte, after the handle's pending call; waits."""
    _check(lib.mt2_workspace_fill(h, int(byte)))


def _workspace_peek(lib, h, offset: int, nbytes: int) -> np.ndarray:
    """mt2_workspace_peek (test hook): `nbytes` arena bytes from `offset` (over the chunks in allocation order) -> np.uint8 array."""
    out = np.empty(int(nbytes), np.uint8)
    _check(lib.mt2_workspace_peek(h, C.c_size_t(int(offset)), out.ctypes.data_as(C.c_void_p), C.c_size_t(int(nbytes))))
    return out


class NativeModel:
    """Owns one `mt2_model*`: packed weights in HBM + the activation workspace."""

    def __init__(self, g_cfg=None, plm_cfg=None, adm_cfg=None, hg_cfg=None,
                 sd_g: Optional[Dict[str, np.ndarray]] = None, sd_plm: Optional[Dict[str, np.ndarray]] = None,
                 sd_adm: Optional[Dict[str, np.ndarray]] = None, sd_hifigan: Optional[Dict[str, np.ndarray]] = None,
                 max_positions: int = MAX_POSITIONS):
        import torch

        self.lib = load_library()
        device_check()
        if not torch.cuda.is_available():
            raise NativeError("PyTorch-ROCm sees no GPU")
        self.g_cfg = g_cfg or cfgmod.production_g()
        self.plm_cfg = plm_cfg or cfgmod.production_plm()
        self.adm_cfg = adm_cfg or cfgmod.production_adm()
        self.hg_cfg = hg_cfg or cfgmod.production_hifigan()
        self.max_positions = max_positions
        self.ccfg = make_config(self.g_cfg, self.plm_cfg, self.adm_cfg, self.hg_cfg, max_positions)
        self.h = C.c_void_p(self.lib.mt2_model_create(C.byref(self.ccfg)))
        if not self.h:
            raise NativeError(self.lib.mt2_last_error().decode())
        self.device = torch.device("cuda", torch.cuda.current_device())
        try:
            if sd_g is not None:
                self._push(sd_g, "G.")
                self._push_one("pe.mrte", sine_table(max_positions, self.g_cfg.mrte.hidden_size,
                                                     float(np.asarray(sd_g["mrte.phone_pos_embedding.alpha"]).reshape(-1)[0])))
            if sd_plm is not None:
                self._push(sd_plm, "plm.")
                self._push_one("pe.plm", sine_table(max_positions, self.plm_cfg.d_model,
                                                    float(np.asarray(sd_plm["pos.alpha"]).reshape(-1)[0])))
            if sd_adm is not None:
                self._push(sd_adm, "adm.")
                self._push_one("pe.adm", sine_table(max_positions, self.adm_cfg.d_model,
                                                    float(np.asarray(sd_adm["pos_emb.alpha"]).reshape(-1)[0])))
            if sd_hifigan is not None:
                self._push(sd_hifigan, "hifigan.")
            _check(self.lib.mt2_model_finalize(self.h))
        except Exception:
            self.close()
            raise
        self.has_g, self.has_plm, self.has_adm = sd_g is not None, sd_plm is not None, sd_adm is not None
        self.has_vocoder = sd_hifigan is not None
        self.range_fallbacks = 0        # calls repeated on the bf16 path because the fp16 range guard tripped (_guarded)

    # ---- lifetime
    def _push_one(self, name: str, arr) -> None:
        a = np.ascontiguousarray(np.asarray(arr, dtype=np.float32))
        shape = (C.c_int64 * max(a.ndim, 1))(*(a.shape if a.ndim else (1,)))
        _check(self.lib.mt2_model_load_tensor(self.h, name.encode(), a.ctypes.data_as(C.c_void_p), shape,
                                              max(a.ndim, 1)))

    def _push(self, sd: Dict[str, np.ndarray], prefix: str) -> None:
        for k, v in sd.items():
            if hasattr(v, "detach"):
                v = v.detach().cpu().numpy()
            self._push_one(prefix + k, v)

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.mt2_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def memory(self):
        w, s = C.c_size_t(0), C.c_size_t(0)
        _check(self.lib.mt2_model_memory(self.h, C.byref(w), C.byref(s)))
        return w.value, s.value

    # ---- helpers
    def _f32(self, t):
        import torch
        assert t.is_cuda, "device tensor expected"
        return t.contiguous().to(torch.float32)

    def _lens(self, lens, B: int, full: int) -> np.ndarray:
        if lens is None:
            return np.full(B, full, np.int32)
        if hasattr(lens, "detach"):
            lens = lens.detach().cpu().numpy()
        a = _i32(lens)
        assert a.shape == (B,)
        return a

    # ---- range guard of the fp16-pipe GEMMs (csrc/gemm_x3h.hip; option "x3h")
    def range_guard(self) -> bool:
        """Waits for this handle's last call; True when one of its fp16-pipe GEMMs saw an activation outside the fp16 range (the
        guard is re-armed).  The outputs of that call are then to be discarded and the call repeated with option x3h = 0."""
        t = C.c_int(0)
        _check(self.lib.mt2_x3h_guard(self.h, C.byref(t)))
        return bool(t.value)

    def _guarded(self, call, check_range: bool = True):
        """Run one native call (a callable returning its status); with check_range, wait for it and - should the range guard have
        tripped - repeat it on the bf16 six-product path, which has f32's exponent range.  Costs one event wait per call;
        check_range = False leaves the call asynchronous and the check (`range_guard()`) to the caller."""
        _check(call())
        if check_range and self.range_guard():
            prev = self.get_option("x3h")        # (a bit mask of the fp16-pipe forms in use)
            self.set_option("x3h", 0)
            try:
                _check(call())
                self.range_fallbacks += 1
            finally:
                self.set_option("x3h", prev)

    # ---- stages (C ABI one-to-one)
    def tc_latent(self, phone, mel, phone_lens=None, mel_lens=None):
        import torch
        B, Np = phone.shape
        Tp = mel.shape[1]
        phone = phone.contiguous().to(torch.int64)
        mel = self._f32(mel)
        pl, ml = self._lens(phone_lens, B, Np), self._lens(mel_lens, B, Tp)
        out = torch.empty(B, Np, self.g_cfg.mrte.hidden_size, device=mel.device, dtype=torch.float32)
        self._guarded(lambda: self.lib.mt2_mrte_tc_latent(self.h, _stream(), _ptr(phone), _iptr(pl), Np, _ptr(mel), _iptr(ml), Tp, B,
                                           _ptr(out)))
        return out

    def mel_context(self, mel, mel_lens=None):
        import torch
        B, Tp = mel.shape[0], mel.shape[1]
        mel = self._f32(mel)
        ml = self._lens(mel_lens, B, Tp)
        s = self.g_cfg.mrte.mel_stride
        Tc = (int(ml.max()) - 1) // s + 1
        out = torch.empty(B, Tc, self.g_cfg.mrte.hidden_size, device=mel.device, dtype=torch.float32)
        self._guarded(lambda: self.lib.mt2_mrte_mel_context(self.h, _stream(), _ptr(mel), _iptr(ml), Tp, B, _ptr(out), Tc))
        return out

    def adm_infer(self, tc_latent, lens=None, return_float=False, p_prefix=None, max_steps: int = 0):
        """MegaADM.infer.  `p_prefix` f32 [B, P] (test hook): forced un-rounded predictions of the first P
        positions - the loop continues from position P for `max_steps` positions (0 = to the end)."""
        import torch
        B, Np = tc_latent.shape[0], tc_latent.shape[1]
        tc = self._f32(tc_latent)
        ln = self._lens(lens, B, Np)
        dur = torch.empty(B, Np, device=tc.device, dtype=torch.int32)
        flt = torch.empty(B, Np, device=tc.device, dtype=torch.float32) if return_float else None
        P = 0
        if p_prefix is not None:
            p_prefix = self._f32(p_prefix).reshape(B, -1)
            P = p_prefix.shape[1]
        self._guarded(lambda: self.lib.mt2_adm_infer_forced(self.h, _stream(), _ptr(tc), _iptr(ln), Np, B, _ptr(p_prefix), P,
                                             int(max_steps), _ptr(dur), _ptr(flt)))
        return (dur, flt) if return_float else dur

    def length_regulate(self, x, dur, lens=None, mel_max_length=None):
        import torch
        B, Np, D = x.shape
        x = self._f32(x)
        d = _i32(dur.detach().cpu().numpy() if hasattr(dur, "detach") else dur).reshape(B, Np)
        ln = self._lens(lens, B, Np)
        tm = int(max(int(d[b, :ln[b]].sum()) for b in range(B)))
        cap = max(tm, int(mel_max_length)) if mel_max_length else tm
        out = torch.empty(B, cap, D, device=x.device, dtype=torch.float32)
        _check(self.lib.mt2_length_regulate(self.h, _stream(), _ptr(x), _iptr(d), _iptr(ln), Np, D, B, _ptr(out), cap))
        return out

    def max_pool_ceil(self, x, k: int = 8, lens=None):
        import torch
        B, T, D = x.shape
        x = self._f32(x)
        ln = self._lens(lens, B, T)
        Tq = -(-T // k)
        out = torch.zeros(B, Tq, D, device=x.device, dtype=torch.float32)
        _check(self.lib.mt2_max_pool_ceil(self.h, _stream(), _ptr(x), _iptr(ln), T, D, B, k, _ptr(out), Tq))
        return out

    @staticmethod
    def _sampling(sampling, seeds, B: int):
        """(pointer to the mt2_sampling struct, its seed array) of a sampled call, or (None, None) - the NULL the `_sampled` entry
        points take for greedy decoding (the greedy C symbols forward to them with NULL themselves)."""
        sampling = sampmod.as_sampling(sampling)
        if sampling is None:
            if seeds is not None:
                raise ValueError("seeds given without sampling")
            return None, None
        sd = sampmod.seed_array(seeds, B)
        return C.byref(sampling.to_c(sd)), sd

    def plm_infer(self, cond, lens=None, return_logits=False, prefix_codes=None, max_steps: int = 0, sampling=None,
                  seeds=None):
        """MegaPLM.infer.  With `prefix_codes` int64 [B, P] the first P rows of `cond` [B, P + Tq, tc] are the
        prompt's pooled tc_latents and decoding is conditioned on the prompt's prosody codes (training layout of
        reference modules/datamodule.py:201-212); `lens` are the TARGET lengths, the result covers the target.
        `sampling` (a sampling.PLMSampling; None = greedy) draws every code instead of the argmax, with `seeds` = an int64
        array [B] or one int s (utterance b gets s + b): mt2_plm_infer_sampled."""
        import torch
        B = cond.shape[0]
        cond = self._f32(cond)
        P = 0
        if prefix_codes is not None:
            prefix_codes = prefix_codes.contiguous().to(torch.int64).reshape(B, -1)
            P = prefix_codes.shape[1]
        Tq = cond.shape[1] - P
        assert Tq >= 1, "cond must hold the prompt rows followed by at least one target row"
        ln = self._lens(lens, B, Tq)
        codes = torch.empty(B, Tq, device=cond.device, dtype=torch.int64)
        logits = torch.zeros(B, Tq, self.plm_cfg.vq_bins, device=cond.device, dtype=torch.float32) if return_logits else None
        smp, _sd = self._sampling(sampling, seeds, B)      # counter-based draws: the range guard's repeat of the call draws the same u
        self._guarded(lambda: self.lib.mt2_plm_infer_sampled(self.h, _stream(), _ptr(cond), _iptr(ln), Tq, B, _ptr(prefix_codes),
                                                             P, int(max_steps), _ptr(codes), _ptr(logits), smp))
        return (codes, logits) if return_logits else codes

    def plm_infer_interpolated(self, cond_a, cond_b, lens, gamma, prefix_a=None, prefix_b=None, return_logits=False,
                               max_steps: int = 0, sampling=None, seeds=None):
        """Prosody interpolation (mt2_plm_infer_interpolated): the PLM decoded against two contexts in lock step, every code drawn
        from the mixture (1 - gamma) * pA + gamma * pB of their next-code distributions and fed back to both.  cond_a / cond_b f32
        [B, P + Tq, tc] (P prompt rows, then the target rows), prefix_a / prefix_b int64 [B, P] (both or neither), `gamma` one
        float or one per utterance in [0, 1], `lens` the TARGET lengths.  `sampling` None = greedy on the mixture.  Returns the
        codes [B, Tq] (and, with return_logits, the logits of both contexts f32 [2, B, Tq, bins])."""
        import torch
        if (prefix_a is None) != (prefix_b is None):
            raise ValueError("prefix_a and prefix_b go together")
        if cond_a.shape != cond_b.shape:
            raise ValueError("cond_a and cond_b must have one shape")
        B = cond_a.shape[0]
        cond = torch.stack([self._f32(cond_a), self._f32(cond_b)])
        P, prefix = 0, None
        if prefix_a is not None:
            prefix_a, prefix_b = (p.contiguous().to(torch.int64).reshape(B, -1) for p in (prefix_a, prefix_b))
            if prefix_a.shape != prefix_b.shape:
                raise ValueError("prefix_a and prefix_b must have one length")
            P = prefix_a.shape[1]
            prefix = torch.stack([prefix_a, prefix_b]) if P else None
        Tq = cond.shape[2] - P
        assert Tq >= 1, "cond must hold the prompt rows followed by at least one target row"
        ln = self._lens(lens, B, Tq)
        gm = sampmod.gamma_array(gamma, B)
        codes = torch.empty(B, Tq, device=cond.device, dtype=torch.int64)
        logits = torch.zeros(2, B, Tq, self.plm_cfg.vq_bins, device=cond.device, dtype=torch.float32) if return_logits else None
        smp, _sd = self._sampling(sampling, seeds, B)      # counter-based draws: the range guard's repeat draws the same codes
        self._guarded(lambda: self.lib.mt2_plm_infer_interpolated(self.h, _stream(), _ptr(cond), _iptr(ln), Tq, B, _ptr(prefix), P,
                                                                  _iptr(gm), int(max_steps), _ptr(codes), _ptr(logits), smp))
        return (codes, logits) if return_logits else codes

    def vq_decode(self, codes):
        import torch
        nq, B, Tq = codes.shape
        assert nq == 1, "n_q = 1 (reference modules/vqpe.py:45)"
        codes = codes.contiguous().to(torch.int64)
        out = torch.empty(B, self.g_cfg.vqpe.vq_dim, Tq, device=codes.device, dtype=torch.float32)
        _check(self.lib.mt2_vq_decode(self.h, _stream(), _ptr(codes), B, Tq, _ptr(out)))
        return out

    def vq_quantize(self, x):
        import torch
        x = self._f32(x)
        M = x.shape[0]
        idx = torch.empty(M, device=x.device, dtype=torch.int64)
        self._guarded(lambda: self.lib.mt2_vq_quantize(self.h, _stream(), _ptr(x), M, _ptr(idx)))
        return idx

    def vqpe_forward(self, mel, lens=None, return_ze=False):
        import torch
        B, T, ld = mel.shape
        mel = self._f32(mel)
        ln = self._lens(lens, B, T)
        st = self.g_cfg.vqpe.stride
        Tq = -(-T // st)
        zq = torch.empty(B, T, self.g_cfg.vqpe.vq_dim, device=mel.device, dtype=torch.float32)
        codes = torch.empty(1, B, Tq, device=mel.device, dtype=torch.int64)
        ze = torch.empty(B, Tq, self.g_cfg.vqpe.vq_dim, device=mel.device, dtype=torch.float32) if return_ze else None
        self._guarded(lambda: self.lib.mt2_vqpe_forward(self.h, _stream(), _ptr(mel), _iptr(ln), T, ld, B, _ptr(zq), _ptr(codes), Tq,
                                         _ptr(ze)))
        return (zq, codes, ze) if return_ze else (zq, codes)

    def mel_decoder(self, x, lens=None):
        import torch
        B, D, T = x.shape
        x = self._f32(x)
        ln = self._lens(lens, B, T)
        mel = torch.empty(B, self.g_cfg.mrte.mel_bins, T, device=x.device, dtype=torch.float32)
        self._guarded(lambda: self.lib.mt2_mel_decoder(self.h, _stream(), _ptr(x), _iptr(ln), T, B, _ptr(mel)))
        return mel

    def hifigan(self, mel, lens=None):
        import torch
        B, D, T = mel.shape
        mel = self._f32(mel)
        ln = self._lens(lens, B, T)
        pad = int(getattr(self.hg_cfg, "inference_padding", 0))
        wav = torch.empty(B, 1, self.hg_cfg.hop * (T + 2 * pad), device=mel.device, dtype=torch.float32)
        self._guarded(lambda: self.lib.mt2_hifigan(self.h, _stream(), _ptr(mel), _iptr(ln), T, B, _ptr(wav)))
        return wav

    def _synth_buffers(self, forced_dur, pl, Np: int, tm_cap: Optional[int], vocoder: bool, dev, mel_out=None):
        """The part the synthesis methods share: forced durations on the host (or None), the frame / code capacities they imply
        and the output tensors -> (fd, tm_cap, tq_cap, mel, mel_lens, dur_out, codes_out, wav)."""
        import torch
        B = len(pl)
        fd = None
        if forced_dur is not None:
            fd = _i32(forced_dur.detach().cpu().numpy() if hasattr(forced_dur, "detach") else forced_dur).reshape(B, Np)
            tm_cap = max(tm_cap or 0, int(max(int(fd[b, :pl[b]].sum()) for b in range(B))))
        if tm_cap is None:
            tm_cap = 128 * Np          # clamp(1, 128) bounds every duration (models/megatts2.py:275)
        tq_cap = -(-tm_cap // self.g_cfg.vqpe.stride)
        nm = self.g_cfg.mrte.mel_bins
        if mel_out is not None:
            if (tuple(mel_out.shape) != (B, tm_cap, nm) or mel_out.dtype != torch.float32
                    or not mel_out.is_contiguous() or mel_out.device != dev):
                raise ValueError(f"mel_out must be a contiguous f32 [{B}, {tm_cap}, {nm}] tensor on {dev}")
            mel = mel_out
        else:
            mel = torch.empty(B, tm_cap, nm, device=dev, dtype=torch.float32)
        mel_lens = np.zeros(B, np.int32)
        dur_out = torch.empty(B, Np, device=dev, dtype=torch.int32)
        codes_out = torch.empty(B, tq_cap, device=dev, dtype=torch.int64)
        pad = int(getattr(self.hg_cfg, "inference_padding", 0))
        wav = torch.empty(B, self.hg_cfg.hop * (tm_cap + 2 * pad), device=dev, dtype=torch.float32) if vocoder else None
        return fd, tm_cap, tq_cap, mel, mel_lens, dur_out, codes_out, wav

    def synthesize_batch(self, phone, phone_lens, prompt_mel, prompt_lens, forced_dur=None, forced_codes=None,
                         run_plm=True, vocoder=False, skip_adm=False, tm_cap: Optional[int] = None,
                         return_aux=False, prompt_vqpe=False, mel_out=None, check_range=True, sampling=None, seeds=None):
        """Megatts.forward's no_grad block for a batch; returns (mel [B, Tm_cap, 80], mel_lens[, aux]).
        `mel_out`: a caller-owned contiguous f32 [B, tm_cap, mel_bins] device tensor the mels are written into (the native call
        zero-fills it first) - e.g. `dist.MelExchange.mel_view(B)`, so that a multi-GPU step gathers without a copy.
        `sampling` / `seeds`: the PLM's codes drawn instead of decoded greedily (as plm_infer; mt2_synthesize_batch_sampled)."""
        import torch
        B, Np = phone.shape
        Tp = prompt_mel.shape[1]
        phone = phone.contiguous().to(torch.int64)
        prompt_mel = self._f32(prompt_mel)
        pl, ml = self._lens(phone_lens, B, Np), self._lens(prompt_lens, B, Tp)
        dev = prompt_mel.device
        fd, tm_cap, tq_cap, mel, mel_lens, dur_out, codes_out, wav = self._synth_buffers(forced_dur, pl, Np, tm_cap, vocoder, dev,
                                                                                        mel_out)
        if forced_codes is not None:
            forced_codes = forced_codes.contiguous().to(torch.int64)
            assert forced_codes.shape[0] == B
            if forced_codes.shape[1] != tq_cap:
                fc = torch.zeros(B, tq_cap, device=phone.device, dtype=torch.int64)
                n = min(tq_cap, forced_codes.shape[1])
                fc[:, :n] = forced_codes[:, :n]
                forced_codes = fc
        flags = ((MT2_RUN_PLM if run_plm else 0) | (MT2_RUN_VOCODER if vocoder else 0) | (MT2_SKIP_ADM if skip_adm else 0)
                 | (MT2_PROMPT_VQPE if prompt_vqpe else 0))
        pcodes = torch.empty(B, -(-Tp // self.g_cfg.vqpe.stride), device=dev, dtype=torch.int64) if prompt_vqpe else None
        smp, _sd = self._sampling(sampling, seeds, B)
        self._guarded(lambda: self.lib.mt2_synthesize_batch_sampled(
            self.h, _stream(), _ptr(phone), _iptr(pl), Np, _ptr(prompt_mel), _iptr(ml), Tp, B, _iptr(fd), _ptr(forced_codes),
            tq_cap, flags, _ptr(mel), tm_cap, _iptr(mel_lens), _ptr(dur_out), _ptr(codes_out), _ptr(wav), _ptr(pcodes), smp),
            check_range)
        if return_aux:
            return mel, mel_lens, {"dur": dur_out, "codes": codes_out, "wav": wav, "prompt_codes": pcodes}
        return mel, mel_lens

    def synthesize_prompt_conditioned(self, phone, phone_lens, prompt_mel, prompt_lens, prompt_phone, prompt_phone_lens,
                                      prompt_dur, forced_dur=None, vocoder=False, tm_cap: Optional[int] = None, check_range=True,
                                      sampling=None, seeds=None):
        """mt2_synthesize_prompt_conditioned: prompt-conditioned synthesis (the PLM continued from the prompt's prosody codes,
        modules/datamodule.py:161-177,196-212) as ONE native call -> (mel, mel_lens, aux) with aux["dur"] the ADM's own
        durations, aux["codes"] the decoded target codes, aux["prompt_codes"] [B, P] the prompt's VQ-PE codes.
        `sampling` / `seeds`: the target's codes drawn instead of decoded greedily (mt2_synthesize_prompt_conditioned_sampled)."""
        import torch
        B, Np = phone.shape
        Tp, Npp = prompt_mel.shape[1], prompt_phone.shape[1]
        phone = phone.contiguous().to(torch.int64)
        prompt_phone = prompt_phone.contiguous().to(torch.int64)
        prompt_mel = self._f32(prompt_mel)
        pl, ml, ppl = self._lens(phone_lens, B, Np), self._lens(prompt_lens, B, Tp), self._lens(prompt_phone_lens, B, Npp)
        pd = _i32(prompt_dur.detach().cpu().numpy() if hasattr(prompt_dur, "detach") else prompt_dur).reshape(B, Npp)
        for b in range(B):
            if int(pd[b, :ppl[b]].sum()) != int(ml[b]):
                raise ValueError("prompt durations must sum to the prompt's mel frames")      # datamodule.py:198 assert
        st = self.g_cfg.vqpe.stride
        if len({-(-int(v) // st) for v in ml}) != 1:
            raise ValueError("prompt-conditioned batches need prompts of one pooled length (pad-free prefix layout)")
        dev = prompt_mel.device
        fd, tm_cap, tq_cap, mel, mel_lens, dur_out, codes_out, wav = self._synth_buffers(forced_dur, pl, Np, tm_cap, vocoder, dev)
        pcodes = torch.empty(B, -(-Tp // st), device=dev, dtype=torch.int64)
        smp, _sd = self._sampling(sampling, seeds, B)
        self._guarded(lambda: self.lib.mt2_synthesize_prompt_conditioned_sampled(
            self.h, _stream(), _ptr(phone), _iptr(pl), Np, _ptr(prompt_mel), _iptr(ml), Tp, B, _ptr(prompt_phone), _iptr(ppl),
            Npp, _iptr(pd), _iptr(fd), tq_cap, MT2_RUN_VOCODER if vocoder else 0, _ptr(mel), tm_cap, _iptr(mel_lens),
            _ptr(dur_out), _ptr(codes_out), _ptr(wav), _ptr(pcodes), smp), check_range)
        P = -(-int(ml[0]) // st)
        return mel, mel_lens, {"dur": dur_out, "codes": codes_out, "wav": wav, "prompt_codes": pcodes[:, :P]}

    # ---- alignment of a prompt to its phones without an external aligner (csrc/dtw.hip)
    def dtw(self, X, Y, x_lens=None, y_lens=None, return_cost: bool = False, return_acc: bool = False):
        """Dynamic time warping of X f32 [B, Tx, D] onto Y f32 [B, Ty, D] (`_dtw`): dict of device tensors lo, hi, steps, total
        [, cost, acc]."""
        return _dtw(self.lib, self.h, X, Y, x_lens, y_lens, return_cost, return_acc)

    # ---- mel-cepstral distortion along the DTW path (csrc/mcd.hip)
    def mel_cepstrum(self, mel, frame_lens=None, order: int = 13):
        """Mel cepstra c1 .. c_order of a log-mel f32 [B, T, N] (`_mel_cepstrum`) -> f32 [B, T, order] (device)."""
        return _mel_cepstrum(self.lib, self.h, mel, frame_lens, order)

    def path_distortion(self, ca, cb, lo, hi, a_lens=None, b_lens=None, f0_a=None, f0_b=None):
        """The distortion row float64 [B, 8] of two cepstra along a given path (`_path_distortion`; the fields are MCD_NAMES)."""
        return _path_distortion(self.lib, self.h, ca, cb, lo, hi, a_lens, b_lens, f0_a, f0_b)

    def mcd(self, mel_a, mel_b, a_lens=None, b_lens=None, f0_a=None, f0_b=None, order: int = 13, return_path: bool = False):
        """Mel-cepstral distortion of mel_a f32 [B, Ta, N] against mel_b f32 [B, Tb, N] along the DTW path of their cepstra, with the F0
        error and the voicing error along the same path where both tracks are given (`_mcd`) -> float64 [B, 8] (device)."""
        return _mcd(self.lib, self.h, mel_a, mel_b, a_lens, b_lens, f0_a, f0_b, order, return_path)

    # ---- stationary-noise suppression (csrc/denoise.hip) on the model's handle, as MelFrontEnd's;  audio: the AudioConfig (default 16 kHz)
    def denoise(self, wav, lens=None, denoise: Optional[Denoise] = None, noise_floor=None, return_floor: bool = False,
                return_figures: bool = False, out=None, audio=None):
        """Denoised audio of wav f32 [B, L] (`_denoise`)."""
        return _denoise(self.lib, self.h, _audio_struct(audio), wav, lens, denoise, noise_floor, return_floor, return_figures, out)

    def noise_floor(self, spec, frame_lens=None, denoise: Optional[Denoise] = None, audio=None):
        """The quantile noise floor f32 [B, F] of a spectrum (`_noise_floor`)."""
        return _noise_floor(self.lib, self.h, _audio_struct(audio), spec, frame_lens, denoise)

    def spectral_gain(self, spec, floor, frame_lens=None, denoise: Optional[Denoise] = None, return_gain: bool = True, apply: bool = False,
                      in_place: bool = False, audio=None):
        """The smoothed gain and / or the gated spectrum of a spectrum and a floor (`_spectral_gain`)."""
        return _spectral_gain(self.lib, self.h, _audio_struct(audio), spec, floor, frame_lens, denoise, return_gain, apply, in_place)

    # ---- declipping by sparsity (csrc/declip.hip) on the model's handle, as MelFrontEnd's
    def clip_detect(self, wav, lens=None, declip: Optional[Declip] = None):
        """The clipping figures float64 [B, 8] of wav f32 [B, L] (`_clip_detect`)."""
        return _clip_detect(self.lib, self.h, wav, lens, declip)

    def declip(self, wav, lens=None, declip: Optional[Declip] = None, return_figures: bool = False, return_iters: bool = False, out=None):
        """Declipped audio of wav f32 [B, L] (`_declip`)."""
        return _declip(self.lib, self.h, wav, lens, declip, return_figures, return_iters, out)

    # ---- speech segments by frame energy and the cut of the pauses (csrc/segments.hip) on the model's handle, as MelFrontEnd's
    def segment_frames(self, energy, frame_lens=None, pauses=None, sample_rate: int = 16000, keep: str = "speech"):
        """The staged form of the rule on any energy contour (`_segment_frames`)."""
        return _segment_frames(self.lib, self.h, energy, frame_lens, pauses, sample_rate, keep)

    def speech_segments(self, wav, lens=None, pauses=None, sample_rate: int = 16000, keep: str = "speech", return_energy: bool = False):
        """The speech segments of wav f32 [B, L] in samples (`_speech_segments`)."""
        return _speech_segments(self.lib, self.h, wav, lens, pauses, sample_rate, keep, return_energy)

    def cut_pauses(self, wav, lens=None, pauses=None, sample_rate: int = 16000, keep: str = "speech", out=None, return_segments: bool = False,
                   return_figures: bool = False):
        """wav f32 [B, L] with its pauses (or with keep = "pauses" its speech) cut out (`_cut_pauses`)."""
        return _cut_pauses(self.lib, self.h, wav, lens, pauses, sample_rate, keep, out, return_segments, return_figures)

    # ---- formant candidates by linear prediction and the formant figures (csrc/formants.hip) on the model's handle, as MelFrontEnd's
    def formants(self, wav, lens=None, cfg=None, hop: Optional[int] = None, sample_rate: Optional[int] = None, return_lpc: bool = False,
                 return_err: bool = False, return_autocorr: bool = False, return_roots: bool = False, return_iters: bool = False, out=None):
        """The formant candidates of wav f32 [B, L] at sample_rate (default 16000; hop default 256) (`_formants`) -> dict: freq, bw, count
        [, lpc, err, autocorr, roots, iters]."""
        return _formants(self.lib, self.h, wav, lens, cfg, 256 if hop is None else hop, 16000 if sample_rate is None else sample_rate,
                         return_lpc, return_err, return_autocorr, return_roots, return_iters, out)

    def formant_stats(self, freq, count, f0=None, frame_lens=None):
        """The formant figures float64 [B, 12] (device; FORMANT_STAT_NAMES) of candidate tracks (`_formant_stats`)."""
        return _formant_stats(self.lib, self.h, freq, count, f0, self._lens(frame_lens, count.shape[0], count.shape[1]))

    def formant_track(self, freq, bw, count, frame_lens=None, track=None, max_formant_hz: float = 5500.0, return_sel: bool = True):
        """The formant tracks across frames of candidate rows (`_formant_track`) -> dict: track_freq, track_bw, track_count, sel."""
        return _formant_track(self.lib, self.h, freq, bw, count, self._lens(frame_lens, count.shape[0], count.shape[1]), track, max_formant_hz,
                              return_sel)

    # ---- de-reverberation by weighted prediction error (csrc/wpe.hip) on the model's handle, as MelFrontEnd's
    def dereverb(self, wav, lens=None, dereverb: Optional[Dereverb] = None, return_figures: bool = False, out=None, audio=None):
        """De-reverberated audio of wav f32 [B, L] (`_dereverb`)."""
        return _dereverb(self.lib, self.h, _audio_struct(audio), wav, lens, dereverb, return_figures, out)

    def wpe_spectrum(self, spec, frame_lens=None, dereverb: Optional[Dereverb] = None, return_filters: bool = False, in_place: bool = False,
                     return_figures: bool = False, audio=None):
        """Steps 1-3 of the rule on a spectrum (`_wpe_spectrum`)."""
        return _wpe_spectrum(self.lib, self.h, _audio_struct(audio), spec, frame_lens, dereverb, return_filters, return_figures, in_place)

    def align_durations(self, hi, y_lens, syn_dur, phone_lens=None):
        """mt2_align_durations: the path's `hi` int32 [B, Ty] (device, from `dtw` with these y_lens) and the synthetic durations
        `syn_dur` int32 [B, Np] (sum over phone_lens[b] = the x-length of utterance b) -> host int32 [B, Np]: the frames of Y that
        each phone owns, row sums = y_lens.  Waits for the device once."""
        import torch
        assert hi.is_cuda and hi.dim() == 2
        hi = hi.contiguous().to(torch.int32)
        B, Ty = hi.shape
        sd = _i32(syn_dur.detach().cpu().numpy() if hasattr(syn_dur, "detach") else syn_dur).reshape(B, -1)
        Np = sd.shape[1]
        yl, pl = self._lens(y_lens, B, Ty), self._lens(phone_lens, B, Np)
        out = np.zeros((B, Np), np.int32)
        _check(self.lib.mt2_align_durations(self.h, _stream(), _ptr(hi), _iptr(yl), Ty, _iptr(sd), _iptr(pl), Np, B, _iptr(out)))
        return out

    # ---- tuning / measurement (every switch lives in THIS handle; the library has no mutable globals)
    def set_option(self, name: str, value: int) -> None:
        _check(self.lib.mt2_set_option(self.h, name.encode(), int(value)))

    def get_option(self, name: str) -> int:
        v = C.c_int(0)
        _check(self.lib.mt2_get_option(self.h, name.encode(), C.byref(v)))
        return v.value

    def set_ar_groups(self, groups: int) -> None:
        self.set_option("ar_groups", groups)

    def workspace_query(self, B: int, Np_max: int, Tp_max: int, Tm_cap: int, run_plm=True, vocoder=False,
                        skip_adm=False, prompt_vqpe=False) -> int:
        """Upper bound (bytes) of the arena one synthesize_batch call of this geometry needs."""
        flags = ((MT2_RUN_PLM if run_plm else 0) | (MT2_RUN_VOCODER if vocoder else 0) | (MT2_SKIP_ADM if skip_adm else 0)
                 | (MT2_PROMPT_VQPE if prompt_vqpe else 0))
        n = C.c_size_t(0)
        _check(self.lib.mt2_workspace_query(self.h, B, Np_max, Tp_max, Tm_cap, flags, C.byref(n)))
        return n.value

    def workspace_reserve(self, nbytes: int) -> None:
        _check(self.lib.mt2_workspace_reserve(self.h, C.c_size_t(int(nbytes))))

    def workspace_high_water(self) -> int:
        n = C.c_size_t(0)
        _check(self.lib.mt2_workspace_high_water(self.h, C.byref(n)))
        return n.value

    def workspace_fill(self, byte: int) -> None:
        """Test hook: set every byte of the activation arena (`_workspace_fill`); results must not depend on it."""
        _workspace_fill(self.lib, self.h, byte)

    def workspace_peek(self, offset: int, nbytes: int) -> np.ndarray:
        """Test hook: arena bytes as a np.uint8 array (`_workspace_peek`)."""
        return _workspace_peek(self.lib, self.h, offset, nbytes)

    def gemm_trace_begin(self) -> None:
        _check(self.lib.mt2_gemm_trace_begin(self.h))

    def gemm_trace_shapes(self, top: int = 16):
        """Traced launches grouped by (config, M, N, K, groups), slowest first - call before gemm_trace_end()."""
        buf = C.create_string_buffer(1 << 14)
        n = self.lib.mt2_gemm_trace_shapes(self.h, buf, len(buf), int(top))
        if n < 0:
            raise NativeError("gemm trace failed")
        out = []
        for line in buf.value.decode().splitlines():
            c, M, N, K, g, cnt, ms, tf = line.split()
            out.append({"config": c, "M": int(M), "N": int(N), "K": int(K), "groups": int(g), "launches": int(cnt),
                        "ms": float(ms), "tflops": float(tf)})
        return out

    def gemm_trace_end(self):
        """-> list of dicts {config, launches, flops, ms} for this handle's GEMM launches since gemm_trace_begin()."""
        cap = 48
        names = (C.c_char_p * cap)()
        launches = (C.c_int64 * cap)()
        flops = (C.c_double * cap)()
        ms = (C.c_double * cap)()
        n = self.lib.mt2_gemm_trace_end(self.h, cap, names, launches, flops, ms)
        if n < 0:
            raise NativeError("gemm trace failed")
        return [{"config": names[i].decode(), "launches": int(launches[i]), "flops": float(flops[i]), "ms": float(ms[i])}
                for i in range(n)]

    def form_log_begin(self) -> None:
        """Start recording the decisions of the AR step wiring, the vocoder wiring and the parallel stages (mt2_form_log_begin):
        observation only, off by default."""
        _check(self.lib.mt2_form_log_begin(self.h))

    def form_log_end(self):
        """-> list of tuples (kind, point, form, attrs) in call order since form_log_begin(): the layer kind (first-fill, first-incr,
        mid, last-skinny, last-split, last-fused; voc-pre, voc-stage<i>, voc-post; mel-encoder, phone-encoder, cross, vqpe, decoder), the
        decision point (ln_linear, residual, ln_pending, attention, tail; pre, upsample, mean, pair, halo, streams, post; conv, linear, ln), the form
        taken there and a dict of the entry's key=value fields (ints where they parse as ints) - include/megatts2_hip.h."""
        buf = C.create_string_buffer(1 << 20)
        n = self.lib.mt2_form_log_end(self.h, buf, len(buf))
        if n < 0:
            raise NativeError("form log failed (or longer than the buffer)")
        out = []
        for line in buf.value.decode().splitlines():
            kind, point, form, *kv = line.split()
            attrs = {}
            for item in kv:
                k, v = item.split("=", 1)
                attrs[k] = int(v) if v.lstrip("-").isdigit() else v
            out.append((kind, point, form, attrs))
        return out

    def set_profiling(self, on: bool) -> None:
        _check(self.lib.mt2_set_profiling(self.h, 1 if on else 0))

    def last_stage_ms(self) -> Dict[str, float]:
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = self.lib.mt2_last_stage_ms(self.h, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(max(n, 0))}


def _wav_lens(wav, lens):
    """What every waveform call of MelFrontEnd starts with: wav as a contiguous f32 [B, L] device tensor and lens as int32 [B] (every
    row L by default) -> (wav, lens, B, L)."""
    import torch
    assert wav.is_cuda and wav.dim() == 2
    wav = wav.contiguous().to(torch.float32)
    B, L = wav.shape
    ln = np.full(B, L, np.int32) if lens is None else _i32(lens)
    assert ln.shape == (B,)
    return wav, ln, B, L


def _out_rows(out, B: int, like, width):
    """The `out` of a call: the caller's contiguous f32 [B, >= what the call needs] device tensor, or a new [B, width()] beside `like`."""
    import torch
    if out is None:
        out = torch.empty(B, width(), device=like.device, dtype=torch.float32)
    assert out.is_cuda and out.is_contiguous() and out.dtype == torch.float32 and out.dim() == 2 and out.shape[0] == B
    return out


def _out_like(out, wav):
    """The `out` of a call that keeps wav's shape: the caller's contiguous f32 [B, L] device tensor, which may be wav itself, or a new one."""
    out = _out_rows(out, wav.shape[0], wav, lambda: wav.shape[1])
    assert out.shape == wav.shape
    return out


def _loudness_blocks(ln, sr: int, momentary: bool, short_term: bool):
    """(NB, NST), a loudness call's momentary and short-term output widths: the longest utterance's blocks, at least 1; 0 if not asked for."""
    ns = max(int(ln.max()), 0) // max(sr // 10, 1)
    return max(1, ns - 3) if momentary else 0, max(1, ns - 29) if short_term else 0


class MelFrontEnd:
    """extract_mel_spec on the GPU (reference modules/tokenizer.py:107-125): STFT as an implicit conv on the
    GEMM engine, magnitude, slaney mel filterbank, log(clamp(., 1e-5)).  Owns a bare handle (no weights)."""

    def __init__(self, audio: Optional[cfgmod.AudioConfig] = None):
        import torch
        self.lib = load_library()
        device_check()
        if not torch.cuda.is_available():
            raise NativeError("PyTorch-ROCm sees no GPU")
        self.audio = audio or cfgmod.AudioConfig()
        a = self.audio
        self.ac = MT2AudioConfig(a.sample_rate, a.n_fft, a.hop_length, a.win_length, a.n_mels, a.f_min, a.f_max, a.clip)
        ccfg = make_config(None, None, None, None)
        self.h = C.c_void_p(self.lib.mt2_model_create(C.byref(ccfg)))
        if not self.h:
            raise NativeError(self.lib.mt2_last_error().decode())

    def close(self) -> None:
        if getattr(self, "h", None):
            self.lib.mt2_model_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __call__(self, wav, lens=None):
        """wav f32 [B, L] (device) -> mel f32 [B, 1 + L // hop, n_mels]; rows beyond 1 + lens[b] // hop are zero."""
        import torch
        assert wav.is_cuda and wav.dim() == 2
        wav = wav.contiguous().to(torch.float32)
        B, L = wav.shape
        ln = np.full(B, L, np.int32) if lens is None else _i32(lens)
        T = 1 + int(ln.max()) // self.audio.hop_length
        mel = torch.empty(B, T, self.audio.n_mels, device=wav.device, dtype=torch.float32)
        _check(self.lib.mt2_mel_spectrogram(self.h, _stream(), C.byref(self.ac), _ptr(wav), _iptr(ln), L, B, _ptr(mel), T))
        return mel

    def resample(self, wav, sr_in: int, lens=None, normalize: bool = False, out=None, sr_out: Optional[int] = None):
        """`librosa.load(wav, sr=audio.sample_rate)` of the reference (models/megatts2.py:335) for a ragged batch on the device, by the
        rule of csrc/resample.hip (parity with librosa's soxr filter is unpinned): wav f32 [B, L] (device) at sr_in ->
        (f32 [B, max L_out], out_lens int32 [B]) with L_out = ceil(n * L / o), zeros beyond out_lens[b]; samples beyond lens[b] are
        never read.  normalize: each utterance divided by its peak as well (:336).  out: a contiguous f32 [B, >= max L_out] device
        tensor to write into.  sr_in == audio.sample_rate is an error: there is nothing to resample.  sr_out (None: audio.sample_rate):
        another rate to resample to, by the same rule - the formant analysis runs at 11 kHz."""
        wav, ln, B, L = _wav_lens(wav, lens)
        sr_out = self._rate(sr_out)
        out = _out_rows(out, B, wav, lambda: resample_query(sr_in, sr_out, int(ln.max()))[0])
        out_lens = np.zeros(B, np.int32)
        _check(self.lib.mt2_resample(self.h, _stream(), _ptr(wav), _iptr(ln), L, B, int(sr_in), sr_out,
                                     MT2_RESAMPLE_NORMALIZE if normalize else 0, _ptr(out), out.shape[1], _iptr(out_lens)))
        return out, out_lens

    def trim(self, wav, lens=None, top_db: float = 60.0, out=None, return_energy: bool = False):
        """`librosa.effects.trim(y, top_db)` of the reference (models/megatts2.py:337; top_db defaults to librosa's 60, the reference
        writes 20) for a ragged batch on the device, by the rule of csrc/trim.hip - frames of 2048 samples every 512, a frame kept
        while its energy is above max energy * 10^(-top_db / 10); parity with librosa is unpinned.  wav f32 [B, L] (device) ->
        (out f32 [B, max lens], out_lens int32 [B], bounds int32 [B, 2]) with out[b, :out_lens[b]] = wav[b, start:end] exactly and
        zeros behind; an all-zero utterance is left whole.  Samples beyond lens[b] are never read.  out: a contiguous f32
        [B, >= max lens] device tensor to write into (not wav).  return_energy: a fourth result, the frame energies f32
        [B, 1 + max lens // 512] (device).  The call waits for the device once, for the bounds."""
        import torch
        wav, ln, B, L = _wav_lens(wav, lens)
        out = _out_rows(out, B, wav, lambda: max(int(ln.max()), 1))
        F = 1 + max(int(ln.max()), 0) // TRIM_HOP
        energy = torch.empty(B, F, device=wav.device, dtype=torch.float32) if return_energy else None
        bounds = np.zeros((B, 2), np.int32)
        _check(self.lib.mt2_trim_silence(self.h, _stream(), _ptr(wav), _iptr(ln), L, B, float(top_db), _ptr(out), out.shape[1],
                                         _iptr(bounds), _ptr(energy), F))
        res = (out, bounds[:, 1] - bounds[:, 0], bounds)
        return res + (energy,) if return_energy else res

    def _rate(self, sample_rate: Optional[int]) -> int:
        return self.audio.sample_rate if sample_rate is None else int(sample_rate)

    def loudness(self, wav, lens=None, sample_rate: Optional[int] = None, return_momentary: bool = False):
        """Integrated loudness (ITU-R BS.1770-4, gated; what EBU R 128 builds on) of a ragged batch of mono utterances on the device, by
        the rule of csrc/loudness.hip / include/megatts2_hip.h; parity with pyloudnorm / libebur128 is unpinned; true peak and
        loudness range are `loudness_ebu`'s.  wav f32 [B, L] (device) at sample_rate (default audio.sample_rate; a multiple of 10 in
        [8000, 192000]) -> stats f64 [B, 8] (device): integrated LUFS (-inf for an utterance under 0.4 s or silent, NaN behind a
        non-finite sample), blocks, blocks over the absolute gate, blocks over both gates, the relative gate, the sample peak, the
        maximum momentary loudness, 1.0.  return_momentary: also f64 [B, max(1, blocks of the longest)] with the loudness of every
        400 ms block (every 100 ms), -inf behind an utterance's own blocks.  Samples beyond lens[b] are never read.  The call only
        enqueues."""
        import torch
        wav, ln, B, L = _wav_lens(wav, lens)
        sr = self._rate(sample_rate)
        stats = torch.empty(B, LOUDNESS_FIELDS, device=wav.device, dtype=torch.float64)
        NB = _loudness_blocks(ln, sr, return_momentary, False)[0]
        mom = torch.empty(B, NB, device=wav.device, dtype=torch.float64) if NB else None
        _check(self.lib.mt2_loudness(self.h, _stream(), _ptr(wav), _iptr(ln), L, B, sr, _ptr(stats), _ptr(mom), NB))
        return (stats, mom) if return_momentary else stats

    def loudness_ebu(self, wav, lens=None, sample_rate: Optional[int] = None, return_momentary: bool = False, return_short_term: bool = False):
        """The figures of an EBU-mode meter (EBU R 128 / Tech 3341) for a ragged batch of mono utterances on the device, by the rules of
        csrc/loudness.hip and csrc/ebu.hip (include/megatts2_hip.h); parity with libebur128 / pyloudnorm is unpinned.  wav f32 [B, L]
        (device) at sample_rate (default audio.sample_rate; a multiple of 10 in [8000, 192000]) -> stats f64 [B, 18] (device): fields
        0-7 are `loudness`'s row bit for bit; 8 the true peak (linear; oversampled ceil(192000 / sample_rate) times, never under the
        sample peak), 9 the oversampling factor, 10 the loudness range in LU (EBU Tech 3342; NaN under 3 s or for silence), 11 the
        short-term blocks (3 s, every 100 ms), 12 those over -70 LUFS, 13 those over both gates, 14 the relative gate (20 LU under
        the gated mean), 15 / 16 the 10th / 95th percentile, 17 the maximum short-term loudness.  return_momentary: also f64
        [B, max(1, blocks of the longest)] as `loudness` returns it.  return_short_term: also f64 [B, max(1, short-term blocks of the
        longest)], -inf behind an utterance's own blocks.  Samples beyond lens[b] are never read.  The call only enqueues."""
        import torch
        wav, ln, B, L = _wav_lens(wav, lens)
        sr = self._rate(sample_rate)
        stats = torch.empty(B, EBU_FIELDS, device=wav.device, dtype=torch.float64)
        NB, NST = _loudness_blocks(ln, sr, return_momentary, return_short_term)
        mom = torch.empty(B, NB, device=wav.device, dtype=torch.float64) if NB else None
        sht = torch.empty(B, NST, device=wav.device, dtype=torch.float64) if NST else None
        _check(self.lib.mt2_loudness_ebu(self.h, _stream(), _ptr(wav), _iptr(ln), L, B, sr, _ptr(stats), _ptr(mom), NB, _ptr(sht), NST))
        res = (stats,) + ((mom,) if return_momentary else ()) + ((sht,) if return_short_term else ())
        return res if len(res) > 1 else stats

    def loudness_normalize(self, wav, lens=None, target_lufs: float = -23.0, peak_ceiling: float = 0.0, sample_rate: Optional[int] = None,
                           out=None, return_stats: bool = False, true_peak_ceiling_dbtp: Optional[float] = None,
                           limiter: Optional[Limiter] = None):
        """Each utterance of a ragged batch brought to target_lufs by one gain g = 10^((target - I) / 20), I its integrated loudness
        (`loudness`): wav f32 [B, L] (device) -> out f32 [B, L] with out[b, :lens[b]] = wav[b, :lens[b]] * g_b (one f32 product) and
        zeros behind.  peak_ceiling > 0: g is capped so that the sample peak stays at or below it (the sample peak, not the true
        peak).  true_peak_ceiling_dbtp (None = off, exactly the call without it; e.g. -1.0): g is capped so that the true peak
        (`loudness_ebu`) stays at or below 10^(dBTP / 20) - what a delivery specification means by a ceiling; it cannot be combined
        with peak_ceiling > 0, and return_stats then gives the f64 [B, 18] of `loudness_ebu`.  An utterance whose loudness is not finite - under 0.4 s, silent, holding a non-finite sample - is copied unchanged
        (g = 1).  out: a contiguous f32 [B, L] device tensor to write into; it may be wav itself.  return_stats: also the f64
        [B, 8] of `loudness` for the INPUT, with g in the last field.  The gain is formed and read on the device: the call only
        enqueues, with no copy to the host and no wait.
        limiter (None = off, exactly the call without it; needs true_peak_ceiling_dbtp): a `Limiter`.  One gain under a ceiling stops
        at the utterance's largest crest and lands under the target; with the limiter the crests alone are turned down by the
        look-ahead gain of csrc/limiter.hip (`limit`), the gain in front of it is corrected over limiter.passes passes until the
        limited audio reads target_lufs, and the ceiling holds as before.  return_stats then gives the f64 [B, 24] of `limit`."""
        import torch
        wav, ln, B, L = _wav_lens(wav, lens)
        sr = self._rate(sample_rate)
        if limiter is not None and true_peak_ceiling_dbtp is None:
            raise ValueError("a limiter holds a true-peak ceiling: state true_peak_ceiling_dbtp")
        out = _out_like(out, wav)
        if true_peak_ceiling_dbtp is not None and peak_ceiling > 0:
            raise ValueError("peak_ceiling and true_peak_ceiling_dbtp exclude each other: state the ceiling one way")
        fields = LOUDNESS_FIELDS if true_peak_ceiling_dbtp is None else EBU_FIELDS if limiter is None else LIMITER_FIELDS
        stats = torch.empty(B, fields, device=wav.device, dtype=torch.float64) if return_stats else None
        head = (self.h, _stream(), _ptr(wav), _iptr(ln), L, B, sr, float(target_lufs))
        if true_peak_ceiling_dbtp is None:
            _check(self.lib.mt2_loudness_normalize(*head, float(peak_ceiling), _ptr(out), _ptr(stats)))
        elif limiter is None:
            _check(self.lib.mt2_loudness_normalize_tp(*head, float(true_peak_ceiling_dbtp), _ptr(out), _ptr(stats)))
        else:
            _check(self.lib.mt2_loudness_normalize_limited(*head, float(true_peak_ceiling_dbtp), float(limiter.window_ms), int(limiter.passes),
                                                           _ptr(out), None, None, _ptr(stats)))
        return (out, stats) if return_stats else out

    def limit(self, wav, lens=None, pre_gain_db: float = 0.0, ceiling_dbtp: float = -1.0, window_ms: float = 5.0,
              sample_rate: Optional[int] = None, out=None, return_stats: bool = False, return_gain: bool = False, return_need: bool = False):
        """True-peak look-ahead limiter, one pass (the rule of csrc/limiter.hip / include/megatts2_hip.h; offline and symmetric; parity
        with any outside limiter and audible quality on real speech are unpinned): wav f32 [B, L] (device) -> out f32 [B, L] with
        out[b, i] = wav[b, i] * G * s[b, i] * t_b, G = 10^(pre_gain_db / 20), s <= 1 the smoothed gain that keeps every oversampled
        value of G wav at or under 10^(ceiling_dbtp / 20) - 1 exactly further than 2 window_ms from any crest over the ceiling - and
        t_b <= 1 a last trim that makes the re-measured true peak hold the ceiling; zeros behind lens[b].  out: a contiguous f32
        [B, L] device tensor to write into; it may be wav itself.  The extras follow out in this order, device tensors:
        return_stats f64 [B, 24] (0-17 `loudness_ebu`'s row of the INPUT with G in field 7, 18 the half window in samples, 19 min s,
        20 the samples with s < 1, 21 the true peak before the trim, 22 t, 23 the integrated loudness of out), return_gain f32 [B, L]
        (s, 1 behind lens[b]), return_need f32 [B, L] (the gain each sample needs by itself).  Samples beyond lens[b] are never read.
        The call only enqueues."""
        import torch
        wav, ln, B, L = _wav_lens(wav, lens)
        sr = self._rate(sample_rate)
        out = _out_like(out, wav)
        stats = torch.empty(B, LIMITER_FIELDS, device=wav.device, dtype=torch.float64) if return_stats else None
        gain = torch.empty_like(wav) if return_gain else None
        need = torch.empty_like(wav) if return_need else None
        _check(self.lib.mt2_limit_true_peak(self.h, _stream(), _ptr(wav), _iptr(ln), L, B, sr, float(pre_gain_db), float(ceiling_dbtp),
                                            float(window_ms), _ptr(out), _ptr(gain), _ptr(need), _ptr(stats)))
        res = (out,) + tuple(x for x in (stats, gain, need) if x is not None)
        return res if len(res) > 1 else out

    def f0(self, wav, lens=None, fmin: float = 62.5, fmax: float = 500.0, threshold: float = 0.15, hop: Optional[int] = None,
           return_cmnd: bool = False, return_lag: bool = False, return_diff: bool = False, out=None):
        """F0 track of a ragged batch by YIN, the rule of csrc/f0.hip (no reference counterpart; parity with librosa.yin / pyin and
        quality on real speech are unpinned): wav f32 [B, L] (device) at audio.sample_rate -> f0 f32 [B, 1 + max lens // hop] in Hz,
        0 where a frame is unvoiced or lies behind its utterance's own 1 + lens[b] // hop.  hop defaults to the mel front-end's, so
        f0[b, t] belongs to mel frame t.  Samples beyond lens[b] are never read.  The extras follow f0 in this order, device tensors:
        return_cmnd f32 [B, T] (the normalised difference at the chosen lag; voiced iff < threshold), return_lag int32 [B, T],
        return_diff f32 [B, T, 257] (the difference function).  out: a contiguous f32 [B, >= T] device tensor to write f0 into (the
        extras then have its width).  The call only enqueues."""
        return self._f0(None, wav, lens, fmin, fmax, threshold, hop, return_cmnd, return_lag, return_diff, out)

    def _f0(self, costs, wav, lens, fmin, fmax, threshold, hop, return_cmnd, return_lag, return_diff, out):
        """`f0` (costs None) and `f0_track` (costs = (octave_cost, jump_cost)): the two differ in the entry point alone."""
        import torch
        wav, ln, B, L = _wav_lens(wav, lens)
        hop = self.audio.hop_length if hop is None else int(hop)
        out = _out_rows(out, B, wav, lambda: 1 + max(int(ln.max()), 0) // max(hop, 1))
        T = out.shape[1]
        cmnd = torch.empty(B, T, device=wav.device, dtype=torch.float32) if return_cmnd else None
        lag = torch.empty(B, T, device=wav.device, dtype=torch.int32) if return_lag else None
        diff = torch.empty(B, T, F0_MAX_LAG + 1, device=wav.device, dtype=torch.float32) if return_diff else None
        head = (self.h, _stream(), _ptr(wav), _iptr(ln), L, B, self.audio.sample_rate, hop, float(fmin), float(fmax), float(threshold))
        tail = (_ptr(out), _ptr(cmnd), _ptr(lag), T, _ptr(diff))
        if costs is None:
            _check(self.lib.mt2_f0_yin(*head, *tail))
        else:
            _check(self.lib.mt2_f0_track(*head, float(costs[0]), float(costs[1]), *tail))
        extras = tuple(x for x in (cmnd, lag, diff) if x is not None)
        return (out,) + extras if extras else out

    def f0_track(self, wav, lens=None, fmin: float = 62.5, fmax: float = 500.0, threshold: float = 0.15, hop: Optional[int] = None,
                 octave_cost: float = 0.02, jump_cost: float = 0.5, return_cmnd: bool = False, return_lag: bool = False,
                 return_diff: bool = False, out=None):
        """F0 track of a ragged batch by the second tracker, a Viterbi pass over YIN's lag costs (mt2_f0_track; the rule is in
        include/megatts2_hip.h and csrc/f0.hip): one lag per frame by the frame's whole d' curve plus jump_cost per octave jumped
        between frames and octave_cost per octave of lag, which cures YIN's octave-high frames on signals with dominant even
        harmonics.  A frame is voiced iff d' at the tracked lag < threshold.  Arguments, outputs and extras as MelFrontEnd.f0.  A
        non-finite sample may change frames anywhere in its utterance (the path is global), never another utterance's.  The call
        only enqueues."""
        return self._f0((octave_cost, jump_cost), wav, lens, fmin, fmax, threshold, hop, return_cmnd, return_lag, return_diff, out)

    def f0_stats(self, f0, frame_lens=None):
        """Pitch moments of f0 f32 [B, T] (device) over the voiced frames (f0 > 0) among the first frame_lens[b] of each row ->
        float64 [B, 6] (device): n, n / T_b, mean, sigma, skewness, excess kurtosis - all zeros without a voiced frame.  Sums in
        double, two passes (csrc/f0.hip).  The call only enqueues."""
        import torch
        assert f0.is_cuda and f0.dim() == 2
        f0 = f0.contiguous().to(torch.float32)
        B, T = f0.shape
        ln = self._frame_lens(frame_lens, B, T)
        stats = torch.empty(B, 6, device=f0.device, dtype=torch.float64)
        _check(self.lib.mt2_f0_stats(self.h, _stream(), _ptr(f0), _iptr(ln), T, B, _ptr(stats)))
        return stats

    # ---- formant candidates by linear prediction and the formant figures (csrc/formants.hip)
    def formants(self, wav, lens=None, cfg=None, hop: Optional[int] = None, sample_rate: Optional[int] = None, return_lpc: bool = False,
                 return_err: bool = False, return_autocorr: bool = False, return_roots: bool = False, return_iters: bool = False, out=None):
        """Formant candidates of a ragged batch by linear prediction, the rule of csrc/formants.hip / include/megatts2_hip.h (no reference
        counterpart; parity with Praat's Burg fit and quality on real speech are unpinned): wav f32 [B, L] (device) at sample_rate
        (default audio.sample_rate; nothing is resampled - `megatts2.extract_formants` does that) -> dict of device tensors (`_formants`):
        freq and bw f32 [B, T, 5] in Hz, the candidates of every frame in ascending frequency with zeros behind count int32 [B, T]; T = 1 +
        max lens // hop, hop defaulting to the mel front-end's, so that at the mel's rate freq[b, t] belongs to mel frame t.  cfg: a
        `Formants` (defaults: order 10, 50 ms Hann, pre-emphasis from 50 Hz) or an MT2FormantConfig in samples.  The extras on request:
        lpc, err, autocorr (float64), roots (complex128 [B, T, order]), iters (int32; -1 marks an empty frame).  out: a contiguous f32
        [B, T', 5] device tensor for freq, T' >= T.  Candidates are per frame; nothing tracks a formant across frames.  The call only
        enqueues."""
        return _formants(self.lib, self.h, wav, lens, cfg, self.audio.hop_length if hop is None else hop, self._rate(sample_rate), return_lpc,
                         return_err, return_autocorr, return_roots, return_iters, out)

    def formant_stats(self, freq, count, f0=None, frame_lens=None):
        """The formant figures of candidate tracks freq f32 [B, T, 5], count int32 [B, T] (device, from `formants`) over the frames with
        at least four candidates among the first frame_lens[b] - and, where an F0 track f0 f32 [B, T] of the same frames is given, the
        voiced ones (f0 > 0) among them -> float64 [B, 12] (device; FORMANT_STAT_NAMES): frames used, their share, the means and sigmas
        of F1 .. F4 in Hz, the formant dispersion (F4 - F1) / 3 of the means, and the vocal-tract length in cm of a uniform tube closed
        at one end with these means (17.5 cm for 500 / 1500 / 2500 / 3500 Hz).  All zeros without such a frame.  Sums in double, two
        passes.  The call only enqueues."""
        return _formant_stats(self.lib, self.h, freq, count, f0, self._frame_lens(frame_lens, count.shape[0], count.shape[1]))

    def formant_track(self, freq, bw, count, frame_lens=None, track=None, max_formant_hz: float = 5500.0, return_sel: bool = True):
        """Formant tracks across frames, the rule of csrc/formant_track.hip / include/megatts2_hip.h (no reference counterpart; parity with
        Praat's "Formant: Track" and quality on real speech are unpinned): of the candidates freq, bw f32 [B, T, 5], count int32 [B, T]
        (device, from `formants`) the `track.tracks` per frame that form the cheapest smooth path through the first frame_lens[b] frames,
        by a Viterbi pass on the GPU, a workgroup per utterance -> dict of device tensors (`_formant_track`): track_freq, track_bw f32
        [B, T, 5] (track q in slot q, zeros behind), track_count int32 [B, T] (`tracks`, or 0 in a frame without that many sound
        candidates: a gap, which cuts the path) and sel int32 [B, T, 5] (the candidate slot each track took, -1 behind).  `formant_stats`
        reads track_freq and track_count as it reads freq and count.  track: a `FormantTrack` (defaults: four tracks, all costs 1; its
        ref_hz None is taken at max_formant_hz) or an MT2FormantTrackConfig.  The call only enqueues."""
        return _formant_track(self.lib, self.h, freq, bw, count, self._frame_lens(frame_lens, count.shape[0], count.shape[1]), track,
                              max_formant_hz, return_sel)

    # ---- per-phone prosody (csrc/prosody.hip)
    def energy(self, wav, lens=None, hop: Optional[int] = None, out=None):
        """Energy contour of a ragged batch on the mel's frames (mt2_frame_energy; the rule is in include/megatts2_hip.h): wav f32
        [B, L] (device) -> f32 [B, 1 + max lens // hop], the mean square of the 1024 samples [hop t - 512, hop t + 512) - exactly
        the F0 frames, so energy[b, t], f0[b, t] and mel frame t coincide; zeros behind an utterance's own 1 + lens[b] // hop.
        Samples beyond lens[b] are never read.  hop defaults to the mel front-end's.  out: a contiguous f32 [B, >= T] device tensor
        to write into.  No reference counterpart; parity with librosa's rms is unpinned.  The call only enqueues."""
        wav, ln, B, L = _wav_lens(wav, lens)
        hop = self.audio.hop_length if hop is None else int(hop)
        out = _out_rows(out, B, wav, lambda: 1 + max(int(ln.max()), 0) // max(hop, 1))
        _check(self.lib.mt2_frame_energy(self.h, _stream(), _ptr(wav), _iptr(ln), L, B, hop, _ptr(out), out.shape[1]))
        return out

    def phone_prosody(self, f0, dur, energy=None, phone_lens=None, frame_lens=None, return_sum: bool = False):
        """The segment reduction of an F0 track over phone durations (mt2_phone_prosody): f0 f32 [B, T] (device), dur int [B, Np] (a
        device tensor as aux["dur"] is, or a host array such as align_prompt's, which is uploaded here), optionally energy f32
        [B, T] -> float64 [B, Np, 8] (device): start, frames, voiced frames, mean Hz, mean semitones above 55 Hz, min Hz, max Hz,
        mean energy of every phone, phone p owning the frames [sum of the durations before it, + its own) clipped to
        frame_lens[b]; a negative duration counts as 0; rows at or beyond phone_lens[b] are zeros.  return_sum: (out, int64 [B]
        device) with the unclipped sum of the durations of each row.  The call only enqueues."""
        import torch
        assert f0.is_cuda and f0.dim() == 2
        f0 = f0.contiguous().to(torch.float32)
        B, T = f0.shape
        dur = dur if hasattr(dur, "is_cuda") else torch.from_numpy(_i32(dur))
        assert dur.dim() == 2 and dur.shape[0] == B
        dur = dur.to(f0.device, torch.int32).contiguous()
        Np = dur.shape[1]
        if energy is not None:
            assert energy.is_cuda and energy.shape == f0.shape
            energy = energy.contiguous().to(torch.float32)
        pl = np.full(B, Np, np.int32) if phone_lens is None else _i32(phone_lens)
        assert pl.shape == (B,)
        fl = self._frame_lens(frame_lens, B, T)
        out = torch.empty(B, Np, PROSODY_FIELDS, device=f0.device, dtype=torch.float64)
        total = torch.empty(B, device=f0.device, dtype=torch.int64) if return_sum else None
        _check(self.lib.mt2_phone_prosody(self.h, _stream(), _ptr(f0), _ptr(energy), _ptr(dur), _iptr(pl), Np, _iptr(fl), T, B, _ptr(out),
                                          _ptr(total)))
        return (out, total) if return_sum else out

    def pitch_contour(self, f0, frame_lens=None, center: bool = True, return_index: bool = False):
        """The voiced frames (f0 > 0) among the first frame_lens[b] of f0 f32 [B, T] (device), kept in order, as semitones
        12 log2 f0 (mt2_pitch_contour) -> (st f32 [B, T], n_voiced int32 [B]) on the device, zeros behind the n_voiced[b] entries of
        a row.  center: the mean of the row's own entries (a double sum) is taken off, which removes the speaker's register.
        return_index: a third result int32 [B, T], the frame each entry came from (-1 behind).  Two such contours through `dtw`
        with D = 1 give the pitch-contour distance sqrt(total / steps).  The call only enqueues."""
        import torch
        assert f0.is_cuda and f0.dim() == 2
        f0 = f0.contiguous().to(torch.float32)
        B, T = f0.shape
        fl = self._frame_lens(frame_lens, B, T)
        st = torch.empty(B, T, device=f0.device, dtype=torch.float32)
        n = torch.empty(B, device=f0.device, dtype=torch.int32)
        index = torch.empty(B, T, device=f0.device, dtype=torch.int32) if return_index else None
        _check(self.lib.mt2_pitch_contour(self.h, _stream(), _ptr(f0), _iptr(fl), T, B, 1 if center else 0, _ptr(st), _ptr(n), _ptr(index)))
        return (st, n, index) if return_index else (st, n)

    def dtw(self, X, Y, x_lens=None, y_lens=None, return_cost: bool = False, return_acc: bool = False):
        """Dynamic time warping of X f32 [B, Tx, D] onto Y f32 [B, Ty, D] on the bare handle (`_dtw`, as NativeModel.dtw): e.g. the
        DTW mel distance `total` between two utterances of different length."""
        return _dtw(self.lib, self.h, X, Y, x_lens, y_lens, return_cost, return_acc)

    # ---- mel-cepstral distortion along the DTW path (csrc/mcd.hip)
    def mel_cepstrum(self, mel, frame_lens=None, order: int = 13):
        """Mel cepstra c1 .. c_order of a log-mel f32 [B, T, N] (`_mel_cepstrum`) -> f32 [B, T, order] (device)."""
        return _mel_cepstrum(self.lib, self.h, mel, frame_lens, order)

    def path_distortion(self, ca, cb, lo, hi, a_lens=None, b_lens=None, f0_a=None, f0_b=None):
        """The distortion row float64 [B, 8] of two cepstra along a given path (`_path_distortion`; the fields are MCD_NAMES)."""
        return _path_distortion(self.lib, self.h, ca, cb, lo, hi, a_lens, b_lens, f0_a, f0_b)

    def mcd(self, mel_a, mel_b, a_lens=None, b_lens=None, f0_a=None, f0_b=None, order: int = 13, return_path: bool = False):
        """Mel-cepstral distortion of mel_a f32 [B, Ta, N] against mel_b f32 [B, Tb, N] along the DTW path of their cepstra, with the F0
        error and the voicing error along the same path where both tracks are given (`_mcd`) -> float64 [B, 8] (device)."""
        return _mcd(self.lib, self.h, mel_a, mel_b, a_lens, b_lens, f0_a, f0_b, order, return_path)

    # ---- stationary-noise suppression (csrc/denoise.hip): quantile noise floor, spectral gate
    def denoise(self, wav, lens=None, denoise: Optional[Denoise] = None, noise_floor=None, return_floor: bool = False,
                return_figures: bool = False, out=None):
        """Denoised audio of wav f32 [B, L] at audio.sample_rate (`_denoise`) -> (out f32 [B, hop * (max lens // hop)], out_lens
        int32 [B][, floor f32 [B, F]][, figures float64 [B, 8]])."""
        return _denoise(self.lib, self.h, self.ac, wav, lens, denoise, noise_floor, return_floor, return_figures, out)

    def noise_floor(self, spec, frame_lens=None, denoise: Optional[Denoise] = None):
        """The quantile noise floor f32 [B, F] of a spectrum, e.g. `stft` of a noise-only clip (`_noise_floor`)."""
        return _noise_floor(self.lib, self.h, self.ac, spec, frame_lens, denoise)

    def spectral_gain(self, spec, floor, frame_lens=None, denoise: Optional[Denoise] = None, return_gain: bool = True, apply: bool = False,
                      in_place: bool = False):
        """The smoothed gain f32 [B, T, F] and / or the gated spectrum of a spectrum and a floor (`_spectral_gain`)."""
        return _spectral_gain(self.lib, self.h, self.ac, spec, floor, frame_lens, denoise, return_gain, apply, in_place)

    # ---- declipping by sparsity (csrc/declip.hip, A-SPADE): detection of flat tops and their restoration, at the audio's own rate
    def clip_detect(self, wav, lens=None, declip: Optional[Declip] = None):
        """The clipping figures float64 [B, 8] (device; DECLIP_NAMES) of wav f32 [B, L] at any sample rate (`_clip_detect`): clipped or
        not, the two levels, the share of samples clipped; nothing is restored."""
        return _clip_detect(self.lib, self.h, wav, lens, declip)

    def declip(self, wav, lens=None, declip: Optional[Declip] = None, return_figures: bool = False, return_iters: bool = False, out=None):
        """Declipped audio of wav f32 [B, L] at any sample rate (`_declip`) -> out f32 [B, L][, figures float64 [B, 8]][, iters int32
        [B, T]]."""
        return _declip(self.lib, self.h, wav, lens, declip, return_figures, return_iters, out)

    # ---- speech segments by frame energy and the cut of the pauses (csrc/segments.hip), at the audio's own rate
    def segment_frames(self, energy, frame_lens=None, pauses=None, sample_rate: Optional[int] = None, keep: str = "speech"):
        """The staged form of the rule on any energy contour f32 [B, F] (`_segment_frames`) -> dict: flags, segments (frames), counts,
        figures.  pauses: a `Pauses` (frames at sample_rate, default audio.sample_rate) or a `segments_config` in frames."""
        return _segment_frames(self.lib, self.h, energy, frame_lens, pauses, self._rate(sample_rate), keep)

    def speech_segments(self, wav, lens=None, pauses=None, sample_rate: Optional[int] = None, keep: str = "speech", return_energy: bool = False):
        """The speech segments of wav f32 [B, L] at sample_rate (default audio.sample_rate) in samples (`_speech_segments`) -> dict:
        segments int32 [B, S, 2], counts int32 [B], figures float64 [B, 8] (PAUSES_NAMES)[, energy]."""
        return _speech_segments(self.lib, self.h, wav, lens, pauses, self._rate(sample_rate), keep, return_energy)

    def cut_pauses(self, wav, lens=None, pauses=None, sample_rate: Optional[int] = None, keep: str = "speech", out=None,
                   return_segments: bool = False, return_figures: bool = False):
        """wav f32 [B, L] with its pauses - or with keep = "pauses" its speech - cut out (`_cut_pauses`) -> (out, out_lens int32 [B][,
        segments, counts][, figures])."""
        return _cut_pauses(self.lib, self.h, wav, lens, pauses, self._rate(sample_rate), keep, out, return_segments, return_figures)

    # ---- de-reverberation by weighted prediction error (csrc/wpe.hip): a per-bin prediction filter between the STFT and its inverse
    def dereverb(self, wav, lens=None, dereverb: Optional[Dereverb] = None, return_figures: bool = False, out=None):
        """De-reverberated audio of wav f32 [B, L] at audio.sample_rate (`_dereverb`) -> (out f32 [B, hop * (max lens // hop)], out_lens
        int32 [B][, figures float64 [B, 8]])."""
        return _dereverb(self.lib, self.h, self.ac, wav, lens, dereverb, return_figures, out)

    def wpe_spectrum(self, spec, frame_lens=None, dereverb: Optional[Dereverb] = None, return_filters: bool = False, in_place: bool = False,
                     return_figures: bool = False):
        """Steps 1-3 of the rule on a spectrum, e.g. `stft` of a recording, at any T >= 1 (`_wpe_spectrum`) -> the spectrum[, the
        filters complex128 [B, F, K]][, figures float64 [B, 8]]."""
        return _wpe_spectrum(self.lib, self.h, self.ac, spec, frame_lens, dereverb, return_filters, return_figures, in_place)

    # ---- Griffin-Lim vocoder (csrc/griffinlim.hip): the STFT, its inverse, mel -> linear and the iteration
    def _frame_lens(self, lens, B: int, T: int) -> np.ndarray:
        ln = np.full(B, T, np.int32) if lens is None else _i32(lens)
        assert ln.shape == (B,)
        return ln

    def stft(self, wav, lens=None):
        """wav f32 [B, L] (device) -> complex64 [B, 1 + L // hop, n_fft // 2 + 1]: the STFT the mel front-end takes its magnitude of
        (torch.stft with center=True, reflect padding, periodic Hann); frames beyond 1 + lens[b] // hop are zero."""
        import torch
        assert wav.is_cuda and wav.dim() == 2
        wav = wav.contiguous().to(torch.float32)
        B, L = wav.shape
        ln = self._frame_lens(lens, B, L)
        T, F = 1 + int(ln.max()) // self.audio.hop_length, self.audio.n_fft // 2 + 1
        S = (2 * F + 3) & ~3
        spec = torch.empty(B, T, S, device=wav.device, dtype=torch.float32)
        _check(self.lib.mt2_stft(self.h, _stream(), C.byref(self.ac), _ptr(wav), _iptr(ln), L, B, _ptr(spec), T))
        return torch.complex(spec[..., :F], spec[..., F:2 * F])

    def istft(self, spec, frame_lens=None, out=None):
        """complex64 [B, T, n_fft // 2 + 1] (device) -> wav f32 [B, (T - 1) * hop]: `torch.istft(center=True, length=(T - 1) * hop)` by
        the rule of csrc/griffinlim.hip, utterance b holding (frame_lens[b] - 1) * hop samples and zeros beyond; frames at or beyond
        frame_lens[b] are never read.  out: a contiguous f32 [B, >= (max T_b - 1) * hop] device tensor to write into."""
        import torch
        assert spec.is_cuda and spec.dim() == 3 and spec.is_complex()
        B, T, F = spec.shape
        assert F == self.audio.n_fft // 2 + 1
        ln = self._frame_lens(frame_lens, B, T)
        S = (2 * F + 3) & ~3
        packed = torch.zeros(B, T, S, device=spec.device, dtype=torch.float32)
        packed[..., :F] = spec.real
        packed[..., F:2 * F] = spec.imag
        out = _out_rows(out, B, spec, lambda: max((int(ln.max()) - 1) * self.audio.hop_length, 1))
        _check(self.lib.mt2_istft(self.h, _stream(), C.byref(self.ac), _ptr(packed), _iptr(ln), T, B, _ptr(out), out.shape[1]))
        return out

    def mel_to_linear(self, mel, mel_lens=None):
        """log-mel f32 [B, T, n_mels] (device) -> linear magnitude f32 [B, T, n_fft // 2 + 1] = max(0, exp(mel) @ P^T), P the
        pseudo-inverse of the front-end's filterbank; zeros in frames at or beyond mel_lens[b], which are never read."""
        import torch
        assert mel.is_cuda and mel.dim() == 3 and mel.shape[2] == self.audio.n_mels
        mel = mel.contiguous().to(torch.float32)
        B, T, _ = mel.shape
        ln = self._frame_lens(mel_lens, B, T)
        F = self.audio.n_fft // 2 + 1
        mag = torch.empty(B, T, (F + 3) & ~3, device=mel.device, dtype=torch.float32)
        _check(self.lib.mt2_mel_to_linear(self.h, _stream(), C.byref(self.ac), _ptr(mel), _iptr(ln), T, B, _ptr(mag)))
        return mag[..., :F]

    def griffin_lim(self, mel, mel_lens=None, n_iter: int = 32, momentum: float = 0.99, seeds=0, return_resid: bool = False, out=None,
                    resid_out=None):
        """Griffin-Lim vocoder by the rule of csrc/griffinlim.hip: log-mel f32 [B, T, n_mels] (device) -> wav f32 [B, (T - 1) * hop],
        utterance b holding (mel_lens[b] - 1) * hop samples - the exact inverse of the front-end's framing, with no inference padding
        (unlike HiFi-GAN's decode_batch) - and zeros beyond.  No weights: intelligible but buzzy audio, a fallback and a debugging
        aid, not a replacement for HiFi-GAN.  seeds: as sampling.seed_array (an int s means s + b); the initial phase depends on
        (seed, frame, bin) alone, so a batch gives what its utterances give alone, bit for bit.  return_resid: also f32
        [B, n_iter + 1, T] with sum_f (|STFT(x_k)| - A)^2 per frame (one extra STFT).  out / resid_out: contiguous f32 device tensors
        [B, >= (max T_b - 1) * hop] / [B, n_iter + 1, T] to write into.  The call only enqueues."""
        import torch
        from .sampling import seed_array
        assert mel.is_cuda and mel.dim() == 3 and mel.shape[2] == self.audio.n_mels
        mel = mel.contiguous().to(torch.float32)
        B, T, _ = mel.shape
        ln = self._frame_lens(mel_lens, B, T)
        sd = seed_array(seeds, B)
        out = _out_rows(out, B, mel, lambda: max((int(ln.max()) - 1) * self.audio.hop_length, 1))
        resid = resid_out
        if resid is None and return_resid:
            resid = torch.empty(B, max(int(n_iter), 0) + 1, T, device=mel.device, dtype=torch.float32)
        if resid is not None:
            assert resid.is_cuda and resid.is_contiguous() and resid.dtype == torch.float32 and resid.shape == (B, int(n_iter) + 1, T)
        _check(self.lib.mt2_griffin_lim(self.h, _stream(), C.byref(self.ac), _ptr(mel), _iptr(ln), T, B, int(n_iter), float(momentum),
                                        sd.ctypes.data_as(C.c_void_p), _ptr(out), out.shape[1], _ptr(resid)))
        return (out, resid) if resid is not None else out

    def set_profiling(self, on: bool) -> None:
        _check(self.lib.mt2_set_profiling(self.h, 1 if on else 0))

    def last_stage_ms(self) -> Dict[str, float]:
        names = (C.c_char_p * 16)()
        ms = (C.c_float * 16)()
        n = self.lib.mt2_last_stage_ms(self.h, names, ms, 16)
        return {names[i].decode(): float(ms[i]) for i in range(max(n, 0))}

    def workspace_high_water(self) -> int:
        n = C.c_size_t(0)
        _check(self.lib.mt2_workspace_high_water(self.h, C.byref(n)))
        return n.value

    def workspace_fill(self, byte: int) -> None:
        """Test hook: set every byte of the activation arena (`_workspace_fill`); results must not depend on it."""
        _workspace_fill(self.lib, self.h, byte)

    def workspace_peek(self, offset: int, nbytes: int) -> np.ndarray:
        """Test hook: arena bytes as a np.uint8 array (`_workspace_peek`)."""
        return _workspace_peek(self.lib, self.h, offset, nbytes)

    def workspace_reserve(self, nbytes: int) -> None:
        _check(self.lib.mt2_workspace_reserve(self.h, C.c_size_t(int(nbytes))))

    def memory(self):
        """(weight bytes, workspace bytes) of the bare handle, as NativeModel.memory."""
        w, s = C.c_size_t(0), C.c_size_t(0)
        _check(self.lib.mt2_model_memory(self.h, C.byref(w), C.byref(s)))
        return w.value, s.value

    def from_audio(self, wav, sr_in: int, lens=None, trim_db: Optional[float] = None, return_bounds: bool = False,
                   denoise: Optional[Denoise] = None, return_noise: bool = False, dereverb: Optional[Dereverb] = None,
                   return_reverb: bool = False, declip: Optional[Declip] = None, return_clipping: bool = False,
                   cut_pauses: Optional[Pauses] = None, return_segments: bool = False, return_pauses: bool = False):
        """Prompt audio at any sample rate -> (mel [B, T, n_mels], mel_lens): resample to audio.sample_rate, peak-normalise and
        extract the mel (models/megatts2.py:335-336,339) with no host round trip.  Audio that already has that rate is only
        normalised, by the same kernels.  trim_db: leading / trailing silence is cut off between the normalisation and the mel
        (`trim`, :337 - the reference's order); None leaves the audio whole.  return_bounds: a third result, int32 [B, 2] = the
        (start, end) of each utterance within its resampled audio.  denoise (None = off, exactly the call without it): a `Denoise`;
        the normalised audio goes through `denoise` and is peak-normalised again before the trim, so that the trim's threshold and the
        mel see the level a clean prompt would have; up to hop - 1 tail samples are dropped.  return_noise (needs denoise): a last
        result, the figures float64 [B, 8] of the suppression (device; DENOISE_NAMES).  dereverb (None = off, exactly the call
        without it): a `Dereverb`; the normalised audio goes through `dereverb` in FRONT of the denoiser - WPE is a linear filter and
        must see the recording before a non-linear gate breaks the linear relation it estimates - and is peak-normalised again once, behind
        the last of the two stages (resample -> normalise -> dereverb -> denoise -> normalise -> trim);
        return_reverb (needs dereverb): a last result, its figures float64 [B, 8] (device; WPE_NAMES).  declip (None = off, exactly
        the call without it): a `Declip`; clipped samples are restored FIRST, at sr_in - the resampler and the normalisation turn flat
        tops into ripple that nothing can recognise as clipping (declip -> resample -> normalise -> dereverb -> denoise -> normalise ->
        trim); return_clipping (needs declip): a last result, its figures float64 [B, 8] (device; DECLIP_NAMES).  cut_pauses (None =
        off, exactly the call without it): a `Pauses`; where the trim would run, behind the last normalisation, the pauses INSIDE the
        audio are cut out as well as its ends (`cut_pauses`; the pad included), so it excludes trim_db and return_bounds (ValueError).
        return_segments (needs cut_pauses): two more results, segments int32 [B, S, 2] (device; samples of the normalised audio, -1
        behind counts) and counts int32 [B] (device); return_pauses (needs cut_pauses): the very last result, its figures float64
        [B, 8] (device; PAUSES_NAMES)."""
        import torch
        if cut_pauses is not None and (trim_db is not None or return_bounds):
            raise ValueError("cut_pauses cuts the ends itself: it excludes trim_db and return_bounds")
        if cut_pauses is None and (return_segments or return_pauses):
            raise ValueError("return_segments and return_pauses need cut_pauses")
        assert wav.is_cuda and wav.dim() == 2
        assert denoise is not None or not return_noise
        assert dereverb is not None or not return_reverb
        assert declip is not None or not return_clipping
        wav = wav.contiguous().to(torch.float32)
        B, L = wav.shape
        clipping = None
        if declip is not None:
            d = self.declip(wav, lens, declip, return_figures=return_clipping)
            wav, clipping = (d[0], d[1]) if return_clipping else (d, None)
        if int(sr_in) == self.audio.sample_rate:
            ln = np.full(B, L, np.int32) if lens is None else _i32(lens)
            y = torch.empty_like(wav)
            _check(self.lib.mt2_peak_normalize(self.h, _stream(), _ptr(wav), _iptr(ln), L, B, _ptr(y)))
        else:
            y, ln = self.resample(wav, sr_in, lens, normalize=True)
        reverb = None
        if dereverb is not None:
            d = self.dereverb(y, ln, dereverb, return_figures=return_reverb)
            y, ln = d[0], d[1]
            reverb = d[2] if return_reverb else None
            if denoise is None:      # with the denoiser behind it, its own normalisation is the one in front of the trim
                _check(self.lib.mt2_peak_normalize(self.h, _stream(), _ptr(y), _iptr(ln), y.shape[1], B, _ptr(y)))
        figures = None
        if denoise is not None:
            d = self.denoise(y, ln, denoise, return_figures=return_noise)
            y, ln = d[0], d[1]
            figures = d[2] if return_noise else None
            _check(self.lib.mt2_peak_normalize(self.h, _stream(), _ptr(y), _iptr(ln), y.shape[1], B, _ptr(y)))
        bounds = None
        if trim_db is not None:
            y, ln, bounds = self.trim(y, ln, trim_db)
        cut = None
        if cut_pauses is not None:
            cut = self.cut_pauses(y, ln, cut_pauses, return_segments=return_segments, return_figures=return_pauses)
            y, ln = cut[0], cut[1]
        res = (self(y, ln), 1 + ln // self.audio.hop_length)
        if return_bounds:
            res += (np.stack([np.zeros_like(ln), ln], axis=1) if bounds is None else bounds,)
        if return_noise:
            res += (figures,)
        if return_reverb:
            res += (reverb,)
        if return_clipping:
            res += (clipping,)
        if cut is not None:
            res += cut[2:]
        return res


# ---- kernel-level entry points -------------------------------------------------------------------------

def op_gemm(X, W, bias=None, R=None, valid=None, rowbase=None, a_mul=1, shift0=0, taps=1, dil=1, Cin=None,
            M=None, N=None, pro_act=ACT_NONE, pro_slope=0.0, epi_act=ACT_NONE, out_scale=1.0, force_cfg=-1,
            out=None, ldx=None):
    import torch
    lib = load_library()
    ldx = ldx or X.shape[1]
    Cin = Cin or ldx
    N = N or W.shape[0]
    M = M or X.shape[0]
    if out is None:
        out = torch.empty(M, N, device=X.device, dtype=torch.float32)
    _check(lib.mt2_op_gemm(_stream(), _ptr(X), ldx, X.shape[0], _ptr(rowbase), a_mul, shift0, taps, dil, Cin, _ptr(W),
                           W.shape[1], _ptr(bias), _ptr(R), R.shape[1] if R is not None else 0, _ptr(valid), _ptr(out),
                           out.shape[1], M, N, pro_act, C.c_float(pro_slope), epi_act, C.c_float(out_scale), force_cfg))
    return out


def op_tile_major(W):
    """row-major [N, K] -> the tile-major block layout of gemm_skinny_tm_kernel (include/megatts2_hip.h)."""
    import torch
    lib = load_library()
    out = torch.empty_like(W)
    _check(lib.mt2_op_tile_major(_stream(), _ptr(W), W.shape[0], W.shape[1], _ptr(out)))
    return out


def op_gemm_tm(X, Wtm, Kw, N, K, n0=0, k0=0, groups=1, x_gstride=0, w_gstride=0, bias=None, R=None, valid=None, M=None,
               a_mul=1, shift0=0, pro_act=ACT_NONE, pro_slope=0.0, epi_act=ACT_NONE, ln=None, eps=1e-5, ldx=None, waves8=False):
    """Linear layer of at most 64 rows on tile-major weights; groups > 1 -> out [groups, M, N] (split-K slabs, ...);
    ln = (gamma, beta): LayerNorm prologue; waves8: the eight-wave form (default: sixteen / twelve waves at M <= 32)."""
    import torch
    lib = load_library()
    ldx = ldx or X.shape[-1]
    M = M or X.shape[-2]
    out = torch.empty(groups, M, N, device=X.device, dtype=torch.float32)
    g_, b_ = ln if ln is not None else (None, None)
    _check(lib.mt2_op_gemm_tm(_stream(), _ptr(X), C.c_longlong(x_gstride), ldx, X.shape[-2], a_mul, shift0, _ptr(Wtm), Kw, n0, k0,
                              C.c_longlong(w_gstride), groups, _ptr(bias), _ptr(R), R.shape[-1] if R is not None else 0,
                              _ptr(valid), _ptr(out), C.c_longlong(M * N), N, M, N, K, pro_act | (0x100 if waves8 else 0), C.c_float(pro_slope), epi_act,
                              _ptr(g_), _ptr(b_), C.c_float(eps)))
    return out[0] if groups == 1 else out


def op_gemm_tm_pairs(X, Wtm, Kw, N, K, bias=None, R=None, M=None, a_mul=1, shift0=0, epi_act=ACT_NONE, ln=None, want_stats=False,
                     pairs=None, eps=1e-5):
    """mt2_op_gemm_tm_pairs: the <= 64-row kernel with the statistics epilogue (want_stats -> (out, pairs [M, N / 16, 2])) and / or
    the pair-fed LayerNorm prologue (ln = (gamma, beta), pairs = [rows, K / 16, 2] of the source rows)."""
    import torch
    lib = load_library()
    M = M or X.shape[0]
    out = torch.empty(M, N, device=X.device, dtype=torch.float32)
    stat = torch.zeros(M, N // 16, 2, device=X.device, dtype=torch.float32) if want_stats else None
    g_, b_ = ln if ln is not None else (None, None)
    _check(lib.mt2_op_gemm_tm_pairs(_stream(), _ptr(X), X.shape[1], X.shape[0], a_mul, shift0, _ptr(Wtm), Kw, _ptr(bias), _ptr(R),
                                    R.shape[1] if R is not None else 0, _ptr(out), N, M, N, K, epi_act, _ptr(g_), _ptr(b_),
                                    C.c_float(eps), _ptr(stat), _ptr(pairs), pairs.shape[1] if pairs is not None else 0))
    return (out, stat) if want_stats else out


def split_bf16x3(W):
    """f32 tensor -> three bf16 planes (uint16 bit patterns, [3, *W.shape]) by truncation; their sum is W exactly."""
    import torch
    r = W.detach().to(torch.float32).cpu().clone()
    planes = []
    for _ in range(3):
        bits = r.view(torch.int32) & -65536          # 0xffff0000
        planes.append((bits >> 16).to(torch.int16))
        r = r - bits.view(torch.float32)
    return torch.stack(planes).contiguous()


def op_conv_x6(X, W, bias=None, R=None, valid=None, shift0=0, taps=1, dil=1, Cin=None, pro_act=ACT_NONE, pro_slope=0.0,
               epi_act=ACT_NONE, force_cfg=-1, out=None):
    """Window convolution with bf16 weight planes (mt2_op_gemm_x6): X [rows, Cin] f32, W [N, taps*Cin] f32; out [rows, N] f32 when given."""
    import torch
    lib = load_library()
    Cin = Cin or X.shape[1]
    N, M = W.shape[0], X.shape[0]
    W3 = split_bf16x3(W).to(X.device)
    if out is None:
        out = torch.empty(M, N, device=X.device, dtype=torch.float32)
    _check(lib.mt2_op_gemm_x6(_stream(), _ptr(X), X.shape[1], M, shift0, taps, dil, Cin, _ptr(W), _ptr(W3), _ptr(bias),
                              _ptr(R), R.shape[1] if R is not None else 0, _ptr(valid), _ptr(out), N, M, N, pro_act,
                              C.c_float(pro_slope), epi_act, force_cfg))
    return out


def split_f16x2_rows(W):
    """f32 matrix [N, K] -> the x3h operand format, written independently of csrc/x3h_planes.h (numpy float16 rounds to nearest
    even with gradual underflow): (planes int16 [N, Kp / 32, 2, 32] = fp16 bit patterns, per row and 32-k chunk the hi values then the
    lo * 2^11 values of the row-scaled matrix, K zero-padded to Kp = ceil32(K); inv f32 [N] = the inverse power-of-two row scales)."""
    import torch
    w = W.detach().to(torch.float32).cpu().numpy()
    N, K = w.shape
    mx = np.abs(np.where(np.isfinite(w), w, 0)).max(axis=1)
    e = np.zeros(N, np.int32)
    nz = mx > 0
    e[nz] = np.clip(15 - np.frexp(mx[nz])[1], -100, 100)
    s = np.ldexp(np.float32(1), e).astype(np.float32)
    v = (w * s[:, None]).astype(np.float32)
    hi = v.astype(np.float16)
    lo = ((v - hi.astype(np.float32)) * np.float32(2048)).astype(np.float16)
    Kp = -(-K // 32) * 32
    planes = np.zeros((N, Kp // 32, 2, 32), np.int16)
    pad = np.zeros((N, Kp), np.int16)
    pad[:, :K] = hi.view(np.int16)
    planes[:, :, 0, :] = pad.reshape(N, Kp // 32, 32)
    pad[:, :K] = lo.view(np.int16)
    planes[:, :, 1, :] = pad.reshape(N, Kp // 32, 32)
    return torch.from_numpy(planes), torch.from_numpy(np.ldexp(np.float32(1), -e).astype(np.float32))


def x3h_split_native(W):
    """The library's own host splitter (mt2_x3h_split) on a CPU f32 matrix: (planes int16 [N, Kp / 32, 2, 32], inv f32 [N])."""
    import torch
    lib = load_library()
    w = W.detach().to(torch.float32).cpu().contiguous()
    kp = -(-w.shape[1] // 32) * 32
    planes = torch.empty(w.shape[0], kp // 32, 2, 32, dtype=torch.int16)
    inv = torch.empty(w.shape[0], dtype=torch.float32)
    _check(lib.mt2_x3h_split(C.c_void_p(w.data_ptr()), C.c_longlong(w.shape[0]), C.c_longlong(w.shape[1]),
                             C.c_void_p(planes.data_ptr()), C.c_void_p(inv.data_ptr())))
    return planes, inv


def op_conv_x3h(X, W, bias=None, R=None, valid=None, shift0=0, taps=1, dil=1, Cin=None, pro_act=ACT_NONE, pro_slope=0.0,
                epi_act=ACT_NONE, force_cfg=-1, want_flag=False, out=None):
    """mt2_op_gemm_x3h: one GEMM / convolution launch with the weights given as f32, as bf16 planes and as fp16 planes (so that
    every tile configuration can be forced): X [rows, Cin] f32, W [N, taps*Cin] f32.  want_flag -> (out, range flag).
    Test conventions of the entry point: force_cfg + 1000 = the same launch with the loaders' 64-bit address form; + 2000 = X holds
    fp16 planes written by op_layernorm(..., act=100) (GemmP::a_planes); + 4000 = the OUTPUT is stored as such planes (GemmP::c_planes:
    same bytes per row as f32; the x3h loader tile only)."""
    import torch
    lib = load_library()
    Cin = Cin or X.shape[1]
    N, M = W.shape[0], X.shape[0]
    W3 = split_bf16x3(W).to(X.device)
    ph, inv = split_f16x2_rows(W)
    ph, inv = ph.to(X.device), inv.to(X.device)
    if out is None:
        out = torch.empty(M, N, device=X.device, dtype=torch.float32)
    flag = torch.zeros(4, device=X.device, dtype=torch.int32)
    _check(lib.mt2_op_gemm_x3h(_stream(), _ptr(X), X.shape[1], M, shift0, taps, dil, Cin, _ptr(W), _ptr(W3), _ptr(ph), _ptr(inv),
                               _ptr(bias), _ptr(R), R.shape[1] if R is not None else 0, _ptr(valid), _ptr(out), N, M, N, pro_act,
                               C.c_float(pro_slope), epi_act, force_cfg, _ptr(flag)))
    return (out, int(flag[0].item())) if want_flag else out


def op_conv_pair(X, W1, b1, W2, b2, taps, dil, slope, valid=None, channels=None, out=None, pair_fuse=7, want_flag=False):
    """mt2_op_conv_pair: out = X + conv2(lrelu(conv1(lrelu(X)))) on the fused pair kernel.  X [R, ldx] f32 of which the first `channels`
    columns are the channels (all when None), W1 / W2 [C, taps * C] f32 (split into fp16 planes here), conv1 dilation dil, conv2 dilation 1, rows with
    valid == 0 written as zeros.  out [R, ldy >= C] (allocated [R, C] when None) receives the C columns.  want_flag -> (out, flag)."""
    import torch
    lib = load_library()
    Cc = channels or X.shape[1]
    R = X.shape[0]
    p1, i1 = (t.to(X.device) for t in split_f16x2_rows(W1))
    p2, i2 = (t.to(X.device) for t in split_f16x2_rows(W2))
    if out is None:
        out = torch.empty(R, Cc, device=X.device, dtype=torch.float32)
    flag = torch.zeros(4, device=X.device, dtype=torch.int32)
    _check(lib.mt2_op_conv_pair(_stream(), _ptr(X), X.shape[1], R, Cc, taps, dil, C.c_float(slope), _ptr(p1), _ptr(i1), _ptr(b1),
                                _ptr(p2), _ptr(i2), _ptr(b2), _ptr(valid), _ptr(out), out.shape[1], pair_fuse, _ptr(flag)))
    return (out, int(flag[0].item())) if want_flag else out


def op_conv_pair_route(R, Cn, taps, dil, flags=0, pair_fuse=7, x3h=15):
    """mt2_conv_pair_route (no device needed) -> dict(err, lds, grid, block, bm, bmo) of the launch launch_conv_pair would make.
    flags: 1 reflect padding, 2 no fp16 planes, 4 an operand of 2 GiB, 8 an operand off its alignment."""
    err, lds, grid, block, bm, bmo = C.c_int(0), C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0)
    load_library().mt2_conv_pair_route(R, Cn, taps, dil, flags, pair_fuse, x3h, C.byref(err), C.byref(lds), C.byref(grid), C.byref(block),
                                       C.byref(bm), C.byref(bmo))
    return {"err": err.value, "lds": lds.value, "grid": grid.value, "block": block.value, "bm": bm.value, "bmo": bmo.value}


def op_up_mrf(X0, X1, X2, Wcat, bias, slope, scale=1.0 / 3.0, valid=None, channels=None, out=None, up_fuse=3, want_flag=False):
    """mt2_op_up_mrf: out [R, ldy >= ch] = stride-2 transposed convolution of lrelu(((X0 + X1) + X2) * scale) on the fused kernel.  X0 / X1 /
    X2 [R, ldx] f32 of which the first `channels` columns are the ch channels (all when None), Wcat [ch, 2 ch] f32 = [wlo rows | whi rows]
    (split into fp16 planes here), bias [ch / 2], rows with valid == 0 written as zeros.  want_flag -> (out, range flag)."""
    import torch
    lib = load_library()
    ch = channels or X0.shape[1]
    R = X0.shape[0]
    assert X1.shape == X0.shape and X2.shape == X0.shape
    ph, inv = (t.to(X0.device) for t in split_f16x2_rows(Wcat))
    if out is None:
        out = torch.empty(R, ch, device=X0.device, dtype=torch.float32)
    flag = torch.zeros(4, device=X0.device, dtype=torch.int32)
    _check(lib.mt2_op_up_mrf(_stream(), _ptr(X0), _ptr(X1), _ptr(X2), X0.shape[1], R, ch, C.c_float(scale), C.c_float(slope), _ptr(ph),
                             _ptr(inv), _ptr(bias), _ptr(valid), _ptr(out), out.shape[1], up_fuse, _ptr(flag)))
    return (out, int(flag[0].item())) if want_flag else out


def op_up_mrf_route(R, ch, stride=2, flags=0, up_fuse=3, x3h=15, off=0):
    """mt2_up_mrf_route (no device needed) -> dict(err, lds, grid, block, bm) of the launch launch_up_mrf would make.  flags: 1 no fp16
    planes, 2 an operand of 2 GiB, 4 output off 16 bytes, 8 planes off 128 bytes, 16 ldx no multiple of 4, 32 a null input, 64 ldy below the
    width, 128 bias off 16 bytes; off: 1 win_conv off, 2 x6_conv off, 4 forced configuration, 8 ldr64."""
    err, lds, grid, block, bm = C.c_int(0), C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0)
    load_library().mt2_up_mrf_route(R, ch, stride, flags, up_fuse, x3h, off, C.byref(err), C.byref(lds), C.byref(grid), C.byref(block),
                                    C.byref(bm))
    return {"err": err.value, "lds": lds.value, "grid": grid.value, "block": block.value, "bm": bm.value}


def op_gemm_x6_ln(X, W, bias=None, R=None, M=None, a_mul=1, shift0=0, epi_act=ACT_NONE, force_cfg=-1, want_stats=False,
                  ln=None, eps=1e-5, x3h=False):
    """mt2_op_gemm_x6_ln: one linear launch on an x6 tile.  want_stats -> also returns (pairs [M, nt, 2], pair width) written by
    the epilogue (nt = 0 rows when the tile has none).  ln = (gamma, beta, pairs [rows, nt, 2], pair width): LayerNorm(X) @ W^T + b
    in the pair-fed algebraic form - gamma / beta are folded into the operands here (float64 sums, as the model loader does)."""
    import torch
    lib = load_library()
    K, N = X.shape[1], W.shape[0]
    M = M or X.shape[0]
    dev = X.device
    out = torch.empty(M, N, device=dev, dtype=torch.float32)
    stat = torch.zeros(M, 32, 2, device=dev, dtype=torch.float32) if want_stats else None
    nt, pw = C.c_int32(0), C.c_int32(0)
    ln_stat, ln_nt, ln_w, ln_s = None, 0, 0, None
    if ln is not None:
        gamma, beta, pairs, ln_w = ln
        Wd = W.double().cpu()
        Wl = (W.cpu() * gamma.cpu()[None, :]).to(torch.float32)
        ln_s = Wl.double().sum(1).to(torch.float32).to(dev)
        bias = (Wd @ beta.double().cpu() + (bias.double().cpu() if bias is not None else 0.0)).to(torch.float32).to(dev)
        W = Wl.to(dev)
        ln_stat = pairs.contiguous()
        ln_nt = pairs.shape[1]
    W = W.contiguous()
    W3 = split_bf16x3(W).to(dev)
    if x3h:      # the same launch with the fp16 planes as well (mt2_op_gemm_x3h_ln): the fp16-pipe tiles 103 / 95-97
        ph, inv = split_f16x2_rows(W)
        ph, inv = ph.to(dev), inv.to(dev)
        _check(lib.mt2_op_gemm_x3h_ln(_stream(), _ptr(X), K, X.shape[0], a_mul, shift0, _ptr(W), _ptr(W3), _ptr(ph), _ptr(inv),
                                      _ptr(bias), _ptr(R), R.shape[1] if R is not None else 0, _ptr(out), N, M, N, K, epi_act,
                                      force_cfg, _ptr(stat), C.byref(nt), C.byref(pw), _ptr(ln_stat), ln_nt, int(ln_w), _ptr(ln_s),
                                      C.c_float(eps)))
    else:
        _check(lib.mt2_op_gemm_x6_ln(_stream(), _ptr(X), K, X.shape[0], a_mul, shift0, _ptr(W), _ptr(W3), _ptr(bias), _ptr(R),
                                     R.shape[1] if R is not None else 0, _ptr(out), N, M, N, K, epi_act, force_cfg, _ptr(stat),
                                     C.byref(nt), C.byref(pw), _ptr(ln_stat), ln_nt, int(ln_w), _ptr(ln_s), C.c_float(eps)))
    if want_stats:
        return out, stat.view(-1)[:M * nt.value * 2].reshape(M, nt.value, 2).clone(), pw.value      # dense [M][nt][2]
    return out


def op_sample_rows(logits, sampling, seeds, positions):
    """mt2_op_sample_rows: the PLM's sampling draw on every row of `logits` f32 [A, N] (device) with per-row seeds (int64 /
    uint64 values [A], device tensor) and target positions (int32 [A], device) -> int64 [A]."""
    import torch
    lib = load_library()
    A, N = logits.shape
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.stride(1) == 1
    seeds = seeds.contiguous().to(torch.int64)
    positions = positions.contiguous().to(torch.int32)
    assert seeds.shape == (A,) and positions.shape == (A,)
    out = torch.empty(A, device=logits.device, dtype=torch.int64)
    s = sampmod.as_sampling(sampling).to_c(np.zeros(1, np.uint64))
    s.seeds = C.cast(C.c_void_p(0), C.POINTER(C.c_uint64))      # the op reads seeds_dev only
    _check(lib.mt2_op_sample_rows(_stream(), _ptr(logits), logits.stride(0), N, A, C.byref(s), _ptr(seeds), _ptr(positions),
                                  _ptr(out)))
    return out


def op_sample_mix_rows(logits, sampling, seeds, positions, gamma):
    """mt2_op_sample_mix_rows: the interpolated draw on the A row pairs of `logits` f32 [2 A, N] (device; pair j = rows 2j,
    2j + 1) with per-pair seeds (int64 / uint64 values [A]), target positions (int32 [A]) and gamma (f32 [A]), all device tensors
    -> int64 [2 A] (the pair's code at 2j and 2j + 1).  `sampling` None = greedy on the mixture (seeds / positions may be None)."""
    import torch
    lib = load_library()
    A, N = logits.shape[0] // 2, logits.shape[1]
    assert logits.is_cuda and logits.dtype == torch.float32 and logits.stride(1) == 1 and logits.shape[0] == 2 * A
    gamma = gamma.contiguous().to(torch.float32)
    assert gamma.shape == (A,)
    s = None
    if sampling is not None:
        seeds = seeds.contiguous().to(torch.int64)
        positions = positions.contiguous().to(torch.int32)
        assert seeds.shape == (A,) and positions.shape == (A,)
        s = sampmod.as_sampling(sampling).to_c(np.zeros(1, np.uint64))
        s.seeds = C.cast(C.c_void_p(0), C.POINTER(C.c_uint64))      # the op reads seeds_dev only
    else:
        seeds = positions = None
    out = torch.empty(2 * A, device=logits.device, dtype=torch.int64)
    _check(lib.mt2_op_sample_mix_rows(_stream(), _ptr(logits), logits.stride(0), N, A, C.byref(s) if s is not None else None,
                                      _ptr(seeds), _ptr(positions), _ptr(gamma), _ptr(out)))
    return out


def op_layernorm(x, gamma, beta, R1=None, valid=None, eps=1e-5, act=ACT_NONE):
    import torch
    lib = load_library()
    M, Cc = x.shape
    out = torch.empty_like(x)
    _check(lib.mt2_op_layernorm(_stream(), _ptr(x), Cc, _ptr(gamma), _ptr(beta), _ptr(R1), Cc, _ptr(valid), _ptr(out),
                                Cc, M, Cc, C.c_float(eps), act))
    return out


# ---- test-only entries into the row kernels (csrc/rowops.hip).  The caller owns every buffer, outputs included (a test pre-fills
# them with a sentinel), and passes the launcher's arguments in the launcher's order (csrc/mt2_kernels.h).

def op_layernorm_ex(x, ldx, gamma, beta, rows_per_group, R1, ldr1, r1_rows, R2, ldr2, valid, valid_rows, out, ldo, M, Cc, eps=1e-5,
                    act=ACT_NONE, out_planes=0, x3h_flag=None):
    """mt2_op_layernorm_ex: one LayerNorm launch with every field of LnP."""
    _check(load_library().mt2_op_layernorm_ex(_stream(), _ptr(x), ldx, _ptr(gamma), _ptr(beta), rows_per_group, _ptr(R1), ldr1,
                                              r1_rows, _ptr(R2), ldr2, _ptr(valid), valid_rows, _ptr(out), ldo, M, Cc,
                                              C.c_float(eps), act, out_planes, _ptr(x3h_flag)))


def op_ln_reduce(parts, pstride, S, bias, R, ldr, gamma, beta, xout, ldx, hout, ldh, M, Cc, eps=1e-5, h_planes=0, x3h_flag=None):
    """mt2_op_ln_reduce: the split-K consumer with every field of LnReduceP, through the launcher's own kernel choice."""
    _check(load_library().mt2_op_ln_reduce(_stream(), _ptr(parts), C.c_longlong(pstride), S, _ptr(bias), _ptr(R), ldr, _ptr(gamma),
                                           _ptr(beta), _ptr(xout), ldx, _ptr(hout), ldh, M, Cc, C.c_float(eps), h_planes,
                                           _ptr(x3h_flag)))


def op_row(op, *args, stream=None):
    """mt2_op_row: launch_<op> with `args` in the launcher's order.  Marshalling is by kind: a tensor (or None = NULL) is a pointer,
    an int an integer, a float a float."""
    ptrs, ints, flts = [], [], []
    for a in args:
        if isinstance(a, float):
            flts.append(a)
        elif isinstance(a, (int, np.integer)) and not isinstance(a, bool):
            ints.append(int(a))
        else:
            ptrs.append(a.data_ptr() if a is not None else 0)
    _check(load_library().mt2_op_row(stream if stream is not None else _stream(), op.encode(), (C.c_void_p * len(ptrs))(*ptrs), len(ptrs),
                                     (C.c_longlong * len(ints))(*ints), len(ints), (C.c_float * len(flts))(*flts), len(flts)))


def op_embed_pe(table, Cc, ids, idmap, pos, pe, out, ldo, R, vocab): op_row("embed_pe", table, Cc, ids, idmap, pos, pe, out, ldo, R, vocab)
def op_gather_rows(src, lds_, map_, out, ldo, Cc, R): op_row("gather_rows", src, lds_, map_, out, ldo, Cc, R)
def op_pool_max(src, lds_, first, cnt, out, ldo, Cc, R): op_row("pool_max", src, lds_, first, cnt, out, ldo, Cc, R)
def op_sum_groups(x, strideG, groups, ld, out, ldo, Cc, R): op_row("sum_groups", x, strideG, groups, ld, out, ldo, Cc, R)
def op_avg3(a, b, d, scale, out, n): op_row("avg3", a, b, d, float(scale), out, n)
def op_conv_post(x0, x1, x2, scale, R, ch, k, w, bias, slope, valid, out): op_row("conv_post", x0, x1, x2, float(scale), R, ch, k, w, bias, float(slope), valid, out)
def op_fill_reflect(x, ld, Cc, start, len_, B, scale, G): op_row("fill_reflect", x, ld, Cc, start, len_, B, scale, G)
def op_pack_rows(src, Cc, Tmax, cmajor, rowmap, dst, ldd, R): op_row("pack_rows", src, Cc, Tmax, cmajor, rowmap, dst, ldd, R)
def op_unpack_rows(src, lds_, Cc, Tmax, cmajor, rowmap, dst, R): op_row("unpack_rows", src, lds_, Cc, Tmax, cmajor, rowmap, dst, R)
def op_adm_step_input(tc_emb, ld_tc, tc_row, w_dt, p, pstride, pe, x, Dc, De, n, A): op_row("adm_step_input", tc_emb, ld_tc, tc_row, w_dt, p, pstride, pe, x, Dc, De, n, A)
def op_plm_step_input(cond, ld_c, cond_row, emb, codes, cstride, pe, x, Dc, De, n, A, emb_rows): op_row("plm_step_input", cond, ld_c, cond_row, emb, codes, cstride, pe, x, Dc, De, n, A, emb_rows)
def op_adm_predict(x, D, w, p, pstride, n, xn, A): op_row("adm_predict", x, D, w, p, pstride, n, xn, A)
def op_adm_finalize(p, pstride, lens, slot_b, dur, flt, dstride, A, nmax): op_row("adm_finalize", p, pstride, lens, slot_b, dur, flt, dstride, A, nmax)
def op_plm_finalize(codes, cstride, lens, slot_b, out, ostride, A, nmax, skip): op_row("plm_finalize", codes, cstride, lens, slot_b, out, ostride, A, nmax, skip)
def op_adm_init_hist(p, pstride, prefix, P, slot_b, A): op_row("adm_init_hist", p, pstride, prefix, P, slot_b, A)
def op_plm_init_hist(codes, cstride, bos, prefix, P, pstride, slot_b, A): op_row("plm_init_hist", codes, cstride, bos, prefix, P, pstride, slot_b, A)
def op_check_ids(ids, map_, R, hi, flag, bit): op_row("check_ids", ids, map_, R, hi, flag, bit)
def op_copy_2d(src, spitch, dst, dpitch, width, rows): op_row("copy_2d", src, spitch, dst, dpitch, width, rows)
def op_scatter_i64(src, map_, out, R): op_row("scatter_i64", src, map_, out, R)
def op_expand_mask(in_, factor, out, n): op_row("expand_mask", in_, factor, out, n)
def op_unpack_wav(src, start, len_, out, out_stride, max_len, B): op_row("unpack_wav", src, start, len_, out, out_stride, max_len, B)
def op_argmax_rows(x, ldx, N, out, ostride, ooff, A): op_row("argmax_rows", x, ldx, N, out, ostride, ooff, A)
def op_vq_argmin(x, ldx, D, xe, ldxe, ee, N, valid, idx, M): op_row("vq_argmin", x, ldx, D, xe, ldxe, ee, N, valid, idx, M)
def op_row_sqnorm(E, D, ee, N): op_row("row_sqnorm", E, D, ee, N)
def op_codebook_rows(E, codes, codemap, out, ldo, Dq, R, bins): op_row("codebook_rows", E, codes, codemap, out, ldo, Dq, R, bins)
def op_reflect_pad_blocks(wav, wstride, blk_b, blk_t, len_, hop, pad, out, R): op_row("reflect_pad_blocks", wav, wstride, blk_b, blk_t, len_, hop, pad, out, R)
def op_magnitude(spec, lds_, F, out, ldo, M): op_row("magnitude", spec, lds_, F, out, ldo, M)
def op_gl_exp_rows(mel, Cc, rowmap, out, R): op_row("gl_exp_rows", mel, Cc, rowmap, out, R)
def op_gl_phase_init(A, lda, row_b, row_t, seeds, S, lds_, F, R): op_row("gl_phase_init", A, lda, row_b, row_t, seeds, S, lds_, F, R)
def op_istft_ola_blocks(frames, N, hop, w2, blk_b, blk_t, row0, T, out, Rb): op_row("istft_ola_blocks", frames, N, hop, w2, blk_b, blk_t, row0, T, out, Rb)
def op_istft_ola_wav(frames, N, hop, w2, row0, T, wav, L_max, B): op_row("istft_ola_wav", frames, N, hop, w2, row0, T, wav, L_max, B)
def op_gl_phase_update(R, Rprev, A, lda, S, lds_, F, c, resid, rmap, rows, update): op_row("gl_phase_update", R, Rprev, A, lda, S, lds_, F, float(c), resid, rmap, rows, update)


# ---- test-only entry into GROUPED launches of the GEMM engine (tests/test_gpu_gemm_groups.py, tests/test_gemm_groups_host.py): the
# descriptor mirror, the model's plane-stride rule, a weight buffer in every operand form, and the launch itself

class MT2GemmDesc(C.Structure):
    """ctypes mirror of mt2_gemm_desc (include/megatts2_hip.h): one engine launch with every operand and stride explicit."""
    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("X", C.c_void_p), ("strideX", C.c_longlong), ("ldx", C.c_int32), ("Rx", C.c_int32),
        ("rowbase", C.c_void_p), ("a_mul", C.c_int32), ("shift0", C.c_int32), ("taps", C.c_int32), ("dil", C.c_int32),
        ("Cin", C.c_int32),
        ("W", C.c_void_p), ("strideW", C.c_longlong), ("ldw", C.c_int32),
        ("W3", C.c_void_p), ("w3_plane", C.c_longlong),
        ("Wh", C.c_void_p), ("wh_inv", C.c_void_p), ("wh_ldb", C.c_longlong), ("wh_gstride", C.c_longlong),
        ("wh_inv_stride", C.c_longlong),
        ("a_planes", C.c_int32),
        ("bias", C.c_void_p), ("strideB", C.c_longlong),
        ("R", C.c_void_p), ("strideR", C.c_longlong), ("ldr", C.c_int32),
        ("valid", C.c_void_p),
        ("C", C.c_void_p), ("strideC", C.c_longlong), ("ldc", C.c_int32),
        ("M", C.c_int32), ("N", C.c_int32), ("groups", C.c_int32),
        ("pro_act", C.c_int32), ("pro_slope", C.c_float), ("epi_act", C.c_int32), ("out_scale", C.c_float),
        ("force_cfg", C.c_int32),
        ("range_flag", C.c_void_p),
        ("cfg_out", C.POINTER(C.c_int32)),
        ("ks_epi4", C.c_int32),
        ("epi4_out", C.POINTER(C.c_int32)),
    ]


def x3h_group_planes(row_len, w_off, ldw, strideW, groups):
    """mt2_x3h_group_planes (host only): how a launch walks the fp16 planes of a buffer split as [rows][row_len] - the rule the model
    applies to its own launches.  -> None (no planes) or a dict: form ("whole" / "slices"), wh_off (bytes), wh_ldb, wh_gstride (bytes),
    inv_off (elements), wh_inv_stride."""
    lib = load_library()
    form = C.c_int32(0)
    v = [C.c_longlong(0) for _ in range(5)]
    _check(lib.mt2_x3h_group_planes(C.c_longlong(row_len), C.c_longlong(w_off), C.c_longlong(ldw), C.c_longlong(strideW),
                                    C.c_longlong(groups), C.byref(form), *[C.byref(x) for x in v]))
    if form.value == 0:
        return None
    return {"form": {1: "whole", 2: "slices"}[form.value], "wh_off": v[0].value, "wh_ldb": v[1].value, "wh_gstride": v[2].value,
            "inv_off": v[3].value, "wh_inv_stride": v[4].value}


class GemmWeights:
    """Test helper: a weight buffer [rows, row_len] on the device in every operand form of the engine, as the model loader keeps it: f32, three
    bf16 planes (plane stride = the whole buffer) and two fp16 planes with one scale per row."""

    def __init__(self, W, device="cuda"):
        W = W.detach().to("cpu").contiguous()
        assert W.dim() == 2
        self.rows, self.row_len = W.shape
        self.f32 = W.to(device)
        self.w3 = split_bf16x3(W).to(device)
        ph, inv = split_f16x2_rows(W)
        self.ph, self.inv = ph.to(device), inv.to(device)


def op_gemm_grouped(X, wts, out, *, M, N, Cin, ldx, Rx, ldw, ldc, groups=1, strideX=0, strideW=0, strideC=0, w_off=0, taps=1, dil=1,
                    a_mul=1, shift0=0, rowbase=None, bias=None, strideB=0, R=None, strideR=0, ldr=0, valid=None, pro_act=ACT_NONE,
                    pro_slope=0.0, epi_act=ACT_NONE, out_scale=1.0, force_cfg=-1, x6=True, x3h=True, a_planes=0, wh_gstride=None,
                    flag=None, ks_epi4=1, want_epi4=False):
    """mt2_op_gemm_grouped: one launch of the engine with `groups` groups.  X / out / bias / R: device tensors whose data pointer is
    the operand of group 0 (a view into a larger buffer moves it); wts: GemmWeights, the launch's W starts w_off elements into it.
    x6 / x3h: attach the bf16 / fp16 planes - the fp16 strides come from x3h_group_planes, i.e. from the model's own rule (no planes
    when it says so); wh_gstride overrides its group stride (rejection tests).  flag: device int32 range-guard word.  Writes `out`
    in place and returns the configuration index the routing chose.  ks_epi4: the option of that name for this launch; want_epi4: return
    (configuration, 1 when the launch finished its tiles with 16-byte loads and stores) instead."""
    lib = load_library()
    d = MT2GemmDesc()
    d.struct_bytes = C.sizeof(MT2GemmDesc)
    d.X, d.strideX, d.ldx, d.Rx = X.data_ptr(), strideX, ldx, Rx
    d.rowbase = rowbase.data_ptr() if rowbase is not None else None
    d.a_mul, d.shift0, d.taps, d.dil, d.Cin = a_mul, shift0, taps, dil, Cin
    d.W, d.strideW, d.ldw = wts.f32.data_ptr() + 4 * w_off, strideW, ldw
    if x6:
        d.W3, d.w3_plane = wts.w3.data_ptr() + 2 * w_off, wts.rows * wts.row_len
    if x3h:
        g = x3h_group_planes(wts.row_len, w_off, ldw, strideW, groups)
        if g is not None:
            d.Wh, d.wh_inv = wts.ph.data_ptr() + g["wh_off"], wts.inv.data_ptr() + 4 * g["inv_off"]
            d.wh_ldb, d.wh_gstride, d.wh_inv_stride = g["wh_ldb"], g["wh_gstride"], g["wh_inv_stride"]
            if wh_gstride is not None:
                d.wh_gstride = wh_gstride
    d.a_planes = a_planes
    d.bias, d.strideB = (bias.data_ptr() if bias is not None else None), strideB
    d.R, d.strideR, d.ldr = (R.data_ptr() if R is not None else None), strideR, ldr
    d.valid = valid.data_ptr() if valid is not None else None
    d.C, d.strideC, d.ldc = out.data_ptr(), strideC, ldc
    d.M, d.N, d.groups = M, N, groups
    d.pro_act, d.pro_slope, d.epi_act, d.out_scale = pro_act, pro_slope, epi_act, out_scale
    d.force_cfg = force_cfg
    d.range_flag = flag.data_ptr() if flag is not None else None
    cfg, epi4 = C.c_int32(-1), C.c_int32(0)
    d.cfg_out = C.pointer(cfg)
    d.ks_epi4, d.epi4_out = ks_epi4, C.pointer(epi4)
    _check(lib.mt2_op_gemm_grouped(_stream(), C.byref(d)))
    return (cfg.value, epi4.value) if want_epi4 else cfg.value


def op_attention(Q, K, V, q_start, q_len, kv_start, kv_len, H, D, scale, lds_min_qlen=-1, lds_waves=0, out=None, x6_min_qlen=-1):
    """mt2_op_attention_tuned: one attention launch with the kernel choice exposed.  lds_waves: 0 / 4 / 8 query tiles per workgroup of
    the LDS-tiled and matrix-pipe kernels; + 32 = the register kernel instead of the head-dim-split one; + 64 = the output rows as fp16
    planes (AttnP::o_planes); + 128 = the fp16-pipe form of the long-sequence kernel (with x6_min_qlen >= 1)."""
    import torch
    lib = load_library()
    O = out if out is not None else torch.zeros(Q.shape[0], H * D, device=Q.device, dtype=torch.float32)
    B = q_start.shape[0]
    _check(lib.mt2_op_attention_tuned(_stream(), _ptr(Q), Q.stride(0), _ptr(K), K.stride(0), _ptr(V), V.stride(0), _ptr(O),
                                      O.stride(0), _ptr(q_start), _ptr(q_len), _ptr(kv_start), _ptr(kv_len), B, H, D,
                                      int(q_len.max().item()), C.c_float(scale), lds_min_qlen, lds_waves, x6_min_qlen,
                                      int(kv_len.max().item())))
    return O


def op_attention_x3h(Q, K, V, q_start, q_len, kv_start, kv_len, H, D, scale, lds_waves=0):
    """mt2_op_attention_x3h: the fp16-pipe form of the long-sequence attention kernel -> (O, range flag)."""
    import torch
    lib = load_library()
    O = torch.zeros(Q.shape[0], H * D, device=Q.device, dtype=torch.float32)
    flag = torch.zeros(4, device=Q.device, dtype=torch.int32)
    _check(lib.mt2_op_attention_x3h(_stream(), _ptr(Q), Q.stride(0), _ptr(K), K.stride(0), _ptr(V), V.stride(0), _ptr(O), O.stride(0),
                                    _ptr(q_start), _ptr(q_len), _ptr(kv_start), _ptr(kv_len), q_start.shape[0], H, D,
                                    int(q_len.max().item()), C.c_float(scale), lds_waves, int(kv_len.max().item()), _ptr(flag)))
    return O, int(flag[0].item())


# ---- test-only entry into the attention launches' geometry (tests/test_gpu_attention_geometry.py, tests/test_attention_route_host.py)

ATTN_KERNELS = ("none", "generic", "reg", "ds", "lds", "x6", "x3h")      # MT2_ATTN_* of include/megatts2_hip.h, by id


class MT2AttnDesc(C.Structure):
    """ctypes mirror of mt2_attn_desc (include/megatts2_hip.h): one attention launch with every field of its parameter block explicit."""
    _fields_ = [
        ("struct_bytes", C.c_int32),
        ("Q", C.c_void_p), ("ldq", C.c_int32),
        ("K", C.c_void_p), ("ldk", C.c_int32),
        ("V", C.c_void_p), ("ldv", C.c_int32),
        ("O", C.c_void_p), ("ldo", C.c_int32),
        ("q_start", C.c_void_p), ("q_len", C.c_void_p), ("kv_start", C.c_void_p), ("kv_len", C.c_void_p), ("o_start", C.c_void_p),
        ("u_qstride", C.c_int32), ("u_qlen", C.c_int32), ("u_kvstride", C.c_int32), ("u_kvlen", C.c_int32), ("u_ostride", C.c_int32),
        ("B", C.c_int32), ("H", C.c_int32), ("D", C.c_int32), ("max_qlen", C.c_int32), ("max_kvlen", C.c_int32), ("scale", C.c_float),
        ("lds_min_qlen", C.c_int32), ("x6_min_qlen", C.c_int32), ("lds_waves", C.c_int32), ("ds_short", C.c_int32),
        ("x3h", C.c_int32), ("o_planes", C.c_int32),
        ("range_flag", C.c_void_p),
        ("kernel_out", C.POINTER(C.c_int32)),
    ]


def _attn_desc(Q, ldq, K, ldk, V, ldv, O, ldo, *, B, H, D, max_qlen, scale, q_start=None, q_len=None, kv_start=None, kv_len=None,
               o_start=None, u_qstride=0, u_qlen=0, u_kvstride=0, u_kvlen=0, u_ostride=0, max_kvlen=0, lds_min_qlen, x6_min_qlen,
               lds_waves, ds_short, x3h, o_planes, flag=None):
    """Q / K / V / O, the start / len arrays and flag: device tensors (their data pointer is the operand: a view into a larger buffer
    moves it), plain integer addresses (the route query never dereferences them) or None."""
    def addr(x):
        return None if x is None else (int(x) if isinstance(x, int) else x.data_ptr())
    d = MT2AttnDesc()
    d.struct_bytes = C.sizeof(MT2AttnDesc)
    d.Q, d.ldq, d.K, d.ldk, d.V, d.ldv, d.O, d.ldo = addr(Q), ldq, addr(K), ldk, addr(V), ldv, addr(O), ldo
    d.q_start, d.q_len, d.kv_start, d.kv_len, d.o_start = addr(q_start), addr(q_len), addr(kv_start), addr(kv_len), addr(o_start)
    d.u_qstride, d.u_qlen, d.u_kvstride, d.u_kvlen, d.u_ostride = u_qstride, u_qlen, u_kvstride, u_kvlen, u_ostride
    d.B, d.H, d.D, d.max_qlen, d.max_kvlen, d.scale = B, H, D, max_qlen, max_kvlen, scale
    d.lds_min_qlen, d.x6_min_qlen, d.lds_waves, d.ds_short, d.x3h, d.o_planes = lds_min_qlen, x6_min_qlen, lds_waves, ds_short, x3h, o_planes
    d.range_flag = addr(flag)
    return d


def op_attention_desc(Q, ldq, K, ldk, V, ldv, O, ldo, **geometry):
    """mt2_op_attention_desc: one attention launch in the ragged (q_start, q_len, kv_start, kv_len[, o_start]) or the uniform (u_*)
    geometry, nothing defaulted: B, H, D, max_qlen, scale, lds_min_qlen, x6_min_qlen, lds_waves, ds_short, x3h and o_planes are required
    keywords.  Writes O in place and returns the name of the kernel the routing chose (ATTN_KERNELS)."""
    d = _attn_desc(Q, ldq, K, ldk, V, ldv, O, ldo, **geometry)
    kernel = C.c_int32(0)
    d.kernel_out = C.pointer(kernel)
    _check(load_library().mt2_op_attention_desc(_stream(), C.byref(d)))
    return ATTN_KERNELS[kernel.value]


def attention_route(ldq, ldk, ldv, ldo, *, Q=128, K=128, V=128, O=128, **geometry):
    """mt2_attention_route (no device needed): what launch_attention would do with the launch -> dict: err (hipError_t; 0 with kernel
    "none": nothing to launch), kernel (ATTN_KERNELS), d (template head dim; generic kernel: 32-column tiles per wave), nwq (query tiles
    per workgroup), nkv (key tiles: ds), nwv (split-KV waves: reg; waves across the head dim: generic), grid (x, y, z), block, lds (bytes).
    Pointers are addresses that are never dereferenced: pass any non-zero integer for a start / len array that exists."""
    d = _attn_desc(Q, ldq, K, ldk, V, ldv, O, ldo, **geometry)
    err, kernel, lds = C.c_int32(0), C.c_int32(0), C.c_longlong(0)
    tmpl, launch = (C.c_int32 * 4)(), (C.c_int32 * 4)()
    if load_library().mt2_attention_route(C.byref(d), C.byref(err), C.byref(kernel), tmpl, launch, C.byref(lds)) != 0:
        raise NativeError("mt2_attention_route: null or mis-sized descriptor")
    return {"err": err.value, "kernel": ATTN_KERNELS[kernel.value], "d": tmpl[0], "nwq": tmpl[1], "nkv": tmpl[2], "nwv": tmpl[3],
            "grid": (launch[0], launch[1], launch[2]), "block": launch[3], "lds": lds.value}


def op_gemm_route(M, N, K, taps=1, dil=1, groups=1, pro_act=ACT_NONE, operands=0, misaligned=0, force_cfg=-1, x3h=15):
    """mt2_gemm_route (no device needed) -> (hipError_t, config index, variant, LDS bytes, planes bits) of the launch launch_gemm would make."""
    out = [C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0), C.c_int(0)]
    _check(load_library().mt2_gemm_route(M, N, K, taps, dil, groups, pro_act, operands, misaligned, force_cfg, x3h, *map(C.byref, out)))
    return tuple(v.value for v in out)


def op_gemm_route_ex(M, N, K, taps=1, dil=1, groups=1, pro_act=ACT_NONE, operands=0, misaligned=0, force_cfg=-1, x3h=15, ld_pad=0, ks_epi4=1):
    """mt2_gemm_route_ex (no device needed): op_gemm_route with ldc = ldr = N + ld_pad and the option ks_epi4 -> its tuple + (1 when an
    x3h K-split tile would finish the launch with 16-byte loads and stores,)."""
    out = [C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0), C.c_int(0), C.c_int(0)]
    _check(load_library().mt2_gemm_route_ex(M, N, K, taps, dil, groups, pro_act, operands, misaligned, force_cfg, x3h, ld_pad, ks_epi4,
                                            *map(C.byref, out)))
    return tuple(v.value for v in out)


def resample_query(sr_in: int, sr_out: int, L: int = 0):
    """mt2_resample_query (no device needed) -> (L_out, o, n, taps) of resampling L samples from sr_in to sr_out."""
    lo, o, n, k = C.c_longlong(0), C.c_int(0), C.c_int(0), C.c_int(0)
    _check(load_library().mt2_resample_query(int(sr_in), int(sr_out), int(L), C.byref(lo), C.byref(o), C.byref(n), C.byref(k)))
    return lo.value, o.value, n.value, k.value


def trim_query(L: int, top_db: float):
    """mt2_trim_query (no device needed) -> (frames, factor): F = 1 + L // 512 and the f32 factor 10^(-top_db / 10) a frame's
    energy is compared with, as a numpy float32."""
    f, c = C.c_int(0), C.c_float(0)
    _check(load_library().mt2_trim_query(int(L), float(top_db), C.byref(f), C.byref(c)))
    return f.value, np.float32(c.value)


def loudness_query(sample_rate: int, L: int):
    """mt2_loudness_query (no device needed) -> (sub_block, blocks, coeffs, workspace_bytes): h = sample_rate // 10, nb =
    max(0, L // h - 3), the ten K-weighting coefficients as float64 (b0 b1 b2 a1 a2 of the shelf, then of the high-pass) and the arena
    bytes of a MelFrontEnd.loudness / loudness_normalize call with one utterance of L samples; NativeError where the rule refuses."""
    h, nb, ws = C.c_int(0), C.c_int(0), C.c_longlong(0)
    c = np.zeros(10, np.float64)
    _check(load_library().mt2_loudness_query(int(sample_rate), int(L), C.byref(h), C.byref(nb), c.ctypes.data_as(C.c_void_p), C.byref(ws)))
    return h.value, nb.value, c, ws.value


def ebu_query(sample_rate: int, L: int):
    """mt2_ebu_query (no device needed) -> (oversample, taps, tile, short_term_blocks, workspace_bytes): o = ceil(192000 / sample_rate),
    the taps of one phase of the true-peak filter (24), the positions one workgroup of the true-peak kernel takes (tile t holds
    i in [tile * t - 12, tile * (t + 1) - 12)), nst = max(0, L // h - 29) and the arena bytes of a MelFrontEnd.loudness_ebu /
    loudness_normalize(true_peak_ceiling_dbtp=) call with one utterance of L samples; NativeError where the rule refuses."""
    o, taps, tile, nst, ws = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
    _check(load_library().mt2_ebu_query(int(sample_rate), int(L), C.byref(o), C.byref(taps), C.byref(tile), C.byref(nst), C.byref(ws)))
    return o.value, taps.value, tile.value, nst.value, ws.value


def limiter_query(sample_rate: int, L: int, window_ms: float = 5.0):
    """mt2_limiter_query (no device needed) -> (half_window, tile, workspace_bytes): H = round(sample_rate * window_ms / 1000), the
    samples one workgroup of the limiter kernels takes (tile t holds i in [tile * t, tile * (t + 1))) and the arena bytes of a
    MelFrontEnd.limit / loudness_normalize(limiter=) call with one utterance of L samples; NativeError where the rule refuses."""
    h, tile, ws = C.c_int(0), C.c_int(0), C.c_longlong(0)
    _check(load_library().mt2_limiter_query(int(sample_rate), int(L), float(window_ms), C.byref(h), C.byref(tile), C.byref(ws)))
    return h.value, tile.value, ws.value


def limiter_window(sample_rate: int, window_ms: float = 5.0):
    """mt2_limiter_window (no device needed) -> the 2 H + 1 smoothing weights of the limiter rule, float32; they add up to 1."""
    H = limiter_query(sample_rate, 1, window_ms)[0]
    w = np.zeros(2 * H + 1, np.float32)
    _check(load_library().mt2_limiter_window(int(sample_rate), float(window_ms), w.ctypes.data_as(C.c_void_p)))
    return w


def true_peak_table(sample_rate: int):
    """mt2_true_peak_table (no device needed) -> the interpolation table of the true-peak rule, float32 [o, 24]; row 0 is the unit
    sample."""
    o = ebu_query(sample_rate, 1)[0]
    table = np.zeros((o, TP_TAPS), np.float32)
    _check(load_library().mt2_true_peak_table(int(sample_rate), table.ctypes.data_as(C.c_void_p)))
    return table


def f0_query(L: int, sample_rate: int = 16000, hop: int = 256, fmin: float = 62.5, fmax: float = 500.0):
    """mt2_f0_query (no device needed) -> (frames, lag_min, lag_max, workspace_bytes): T = 1 + L // hop, tau_min = ceil(sr / fmax),
    tau_max = floor(sr / fmin) and the arena bytes of one MelFrontEnd.f0 call; NativeError where the rule refuses."""
    f, lo, hi, ws = C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
    _check(load_library().mt2_f0_query(int(sample_rate), int(hop), float(fmin), float(fmax), int(L), C.byref(f), C.byref(lo), C.byref(hi),
                                       C.byref(ws)))
    return f.value, lo.value, hi.value, ws.value


def formant_query(L: int, sample_rate: int = 11000, hop: int = 176, window: int = 550, order: int = 10):
    """mt2_formant_query (no device needed) -> (frames, workspace_bytes): T = 1 + L // hop and the arena bytes of one `formants` call
    (4 * 65535 rounded up to 256, whatever the batch); NativeError where the rule refuses."""
    f, ws = C.c_int(0), C.c_longlong(0)
    _check(load_library().mt2_formant_query(int(sample_rate), int(hop), int(window), int(order), int(L), C.byref(f), C.byref(ws)))
    return f.value, ws.value


def formant_track_query(tracks: int = 4, T_max: int = 1, B: int = 1):
    """mt2_formant_track_query (no device needed) -> (states, workspace_bytes): C(5, tracks) and the arena bytes of one `formant_track`
    call, r(4 * 65535) + r(16 * B * T_max) with r rounding up to 256; NativeError where the rule refuses."""
    st, ws = C.c_int(0), C.c_longlong(0)
    _check(load_library().mt2_formant_track_query(int(tracks), int(T_max), int(B), C.byref(st), C.byref(ws)))
    return st.value, ws.value


def formant_window(window: int, kind: str = "hann") -> np.ndarray:
    """mt2_formant_window (no device needed) -> float64 [window]: the table the device applies; NativeError where the rule refuses."""
    w = np.empty(max(int(window), 1), np.float64)
    _check(load_library().mt2_formant_window(int(window), FORMANT_WINDOWS.get(kind, -1), w.ctypes.data_as(C.c_void_p)))
    return w


def f0_track_query(L: int, B: int = 1, sample_rate: int = 16000, hop: int = 256, fmin: float = 62.5, fmax: float = 500.0,
                   octave_cost: float = 0.02, jump_cost: float = 0.5):
    """mt2_f0_track_query (no device needed) -> (frames, lag_min, lag_max, states, workspace_bytes) of one MelFrontEnd.f0_track call
    with B utterances, the longest of L samples: T = 1 + L // hop, n = lag_max - lag_min + 1 and, with r(x) = x rounded up to 256,
    r(4 (4 ceil(B / 4) + 256)) + r(4 B T 257) + r(256 B T) arena bytes; NativeError where the rule refuses."""
    f, lo, hi, n, ws = C.c_int(0), C.c_int(0), C.c_int(0), C.c_int(0), C.c_longlong(0)
    _check(load_library().mt2_f0_track_query(int(sample_rate), int(hop), float(fmin), float(fmax), float(octave_cost), float(jump_cost),
                                             int(L), int(B), C.byref(f), C.byref(lo), C.byref(hi), C.byref(n), C.byref(ws)))
    return f.value, lo.value, hi.value, n.value, ws.value


def dtw_query(Tx_max: int, Ty_max: int, D: int = 80, B: int = 1) -> int:
    """mt2_dtw_query (no device needed) -> the arena bytes one dtw call of this geometry takes at most: with r(n) = n rounded up to
    256, r(4 B ceil(Tx / 64) 64 ceil((Ty + 63) / 64) 64) for the skewed costs + r(4 B Tx ceil(Ty / 16)) for the packed directions +
    r(4 (2 B + 8)) for the lengths."""
    n = C.c_longlong(0)
    _check(load_library().mt2_dtw_query(int(Tx_max), int(Ty_max), int(D), int(B), C.byref(n)))
    return n.value


def mcd_query(Ta_max: int, Tb_max: int, n_mels: int = 80, order: int = 13, B: int = 1) -> int:
    """mt2_mcd_query (no device needed) -> the arena bytes of one `mcd` call of this geometry, which is exactly its high water: what
    dtw_query states for the skewed costs and the packed directions, and with r(n) = n rounded up to 256, r(4 (4 ceil(B / 4) + B)) for
    the lengths + r(4 B Ta K) + r(4 B Tb K) for the cepstra + 2 r(4 B Tb) for lo and hi + 2 r(4 B) for steps and total."""
    n = C.c_longlong(0)
    _check(load_library().mt2_mcd_query(int(Ta_max), int(Tb_max), int(n_mels), int(order), int(B), C.byref(n)))
    return n.value


def mcd_table(n_mels: int = 80, order: int = 13) -> np.ndarray:
    """mt2_mcd_table (no device needed) -> the cepstrum table float32 [order, n_mels]: cos(pi (m + 1/2) k / n_mels) / n_mels, k = 1 .. order."""
    table = np.zeros((max(int(order), 0), max(int(n_mels), 0)), np.float32)
    _check(load_library().mt2_mcd_table(int(n_mels), int(order), table.ctypes.data_as(C.c_void_p)))
    return table


def denoise_query(audio=None, lens=None, L_max: Optional[int] = None, B: Optional[int] = None, denoise: Optional[Denoise] = None):
    """mt2_denoise_query (no device needed) -> (arena bytes, L_out, rank k, factor c) of one `denoise` call: lens int [B] (or L_max and
    B: every utterance L_max samples).  The bytes are exactly the call's high water; L_out = hop * (max lens // hop); k and c are the
    rank and the quantile-to-mean factor of the longest utterance.  It refuses what the call refuses."""
    ac = _audio_struct(audio)
    ln = None if lens is None else _i32(lens)
    if ln is not None:
        B, L_max = len(ln), int(ln.max()) if L_max is None else L_max
    dc = (denoise or Denoise()).c_struct()
    nbytes, lout, rank, c = C.c_longlong(0), C.c_longlong(0), C.c_int(0), C.c_float(0)
    _check(load_library().mt2_denoise_query(C.byref(ac), C.byref(dc), _iptr(ln), int(L_max or 0), int(B or 0), C.byref(nbytes),
                                            C.byref(lout), C.byref(rank), C.byref(c)))
    return nbytes.value, lout.value, rank.value, c.value


def dereverb_query(audio=None, lens=None, L_max: Optional[int] = None, B: Optional[int] = None, dereverb: Optional[Dereverb] = None):
    """mt2_dereverb_query (no device needed) -> (arena bytes, L_out) of one `dereverb` call: lens int [B] (or L_max and B: every
    utterance L_max samples).  The bytes are exactly the call's high water; L_out = hop * (max lens // hop).  It refuses what the call
    refuses."""
    ac = _audio_struct(audio)
    ln = None if lens is None else _i32(lens)
    if ln is not None:
        B, L_max = len(ln), int(ln.max()) if L_max is None else L_max
    wc = (dereverb or Dereverb()).c_struct()
    nbytes, lout = C.c_longlong(0), C.c_longlong(0)
    _check(load_library().mt2_dereverb_query(C.byref(ac), C.byref(wc), _iptr(ln), int(L_max or 0), int(B or 0), C.byref(nbytes),
                                             C.byref(lout)))
    return nbytes.value, lout.value


def segments_query(lens=None, L_max: Optional[int] = None, B: Optional[int] = None, pauses=None, sample_rate: int = 16000):
    """mt2_segments_query (no device needed) -> (frames of the longest utterance, the f32 factor 10^(-top_db / 10), the most segments an
    utterance can have - the S of `speech_segments` -, arena bytes of one `speech_segments` or `cut_pauses` call): lens int [B] in
    samples, or every utterance L_max samples.  pauses: a `Pauses` at sample_rate, or a `segments_config` in frames."""
    ln = None if lens is None else _i32(lens)
    if ln is not None:
        L_max = int(ln.max()) if L_max is None and ln.size else L_max
        B = ln.size
    cfg = _segments_cfg(pauses, sample_rate, "speech")
    F, c, S, nbytes = C.c_int(0), C.c_float(0.0), C.c_longlong(0), C.c_longlong(0)
    _check(load_library().mt2_segments_query(C.byref(cfg), _iptr(ln), int(L_max or 0), int(B or 0), C.byref(F), C.byref(c), C.byref(S), C.byref(nbytes)))
    return F.value, c.value, S.value, nbytes.value


def declip_query(lens=None, L_max: Optional[int] = None, B: Optional[int] = None, declip: Optional[Declip] = None):
    """mt2_declip_query (no device needed) -> (arena bytes of one `declip` call, arena bytes of one `clip_detect` call, T): lens int [B]
    (or L_max and B: every utterance L_max samples).  The bytes are exactly the calls' high water; T = ceil(max lens / hop) + 3, the
    width of `iters`.  It refuses what the calls refuse."""
    ln = None if lens is None else _i32(lens)
    if ln is not None:
        B, L_max = len(ln), (int(ln.max()) if len(ln) else 0) if L_max is None else L_max
    dc = (declip or Declip()).c_struct()
    nbytes, dbytes, T = C.c_longlong(0), C.c_longlong(0), C.c_longlong(0)
    _check(load_library().mt2_declip_query(C.byref(dc), _iptr(ln), int(L_max or 0), int(B or 0), C.byref(nbytes), C.byref(dbytes), C.byref(T)))
    return nbytes.value, dbytes.value, T.value


def griffin_lim_query(audio, mel_lens=None, T_max: Optional[int] = None, B: Optional[int] = None, n_iter: int = 32,
                      momentum: float = 0.99, return_resid: bool = False):
    """mt2_griffin_lim_query (no device needed) -> (arena bytes, L_out) of one MelFrontEnd.griffin_lim call: mel_lens int [B] (or
    None with T_max and B: every utterance T_max frames), L_out = (max T_b - 1) * hop.  It refuses what the call refuses, the
    rank-deficient filterbank included.  The closed form is in include/megatts2_hip.h."""
    ac = MT2AudioConfig(audio.sample_rate, audio.n_fft, audio.hop_length, audio.win_length, audio.n_mels, audio.f_min, audio.f_max,
                        audio.clip)
    ln = None if mel_lens is None else _i32(mel_lens)
    if ln is not None:
        B = int(ln.size) if B is None else B
        T_max = int(ln.max()) if T_max is None and ln.size else T_max
    n, lo = C.c_longlong(0), C.c_longlong(0)
    _check(load_library().mt2_griffin_lim_query(C.byref(ac), _iptr(ln), int(T_max or 0), int(B or 0), int(n_iter), float(momentum),
                                                1 if return_resid else 0, C.byref(n), C.byref(lo)))
    return n.value, lo.value


def resample_table(sr_in: int, sr_out: int) -> np.ndarray:
    """mt2_resample_table (no device needed) -> the f32 filter [n, taps] the device applies for this pair of rates."""
    _, _, n, k = resample_query(sr_in, sr_out)
    h = np.empty((n, k), np.float32)
    _check(load_library().mt2_resample_table(int(sr_in), int(sr_out), h.ctypes.data_as(C.c_void_p)))
    return h


def bench_gemm(M, N, K, taps=1, force_cfg=-1, iters=20, w_copies=1, dil=1, flags=0):
    lib = load_library()
    ms = C.c_float(0)
    name = C.create_string_buffer(64)
    ghz = C.c_double(0.0)
    _check(lib.mt2_bench_gemm(_stream(), M, N, K, taps, dil, flags, force_cfg, iters, w_copies, C.byref(ms), name, 64,
                              C.byref(ghz)))
    if flags & 4:
        return ms.value, name.value.decode(), ghz.value
    return ms.value, name.value.decode()
