"""Seeded sampling of the PLM's prosody codes (temperature / top-k / top-p): the host side of `mt2_sampling`.

The reference decodes the PLM greedily (models/megatts2.py:165-181) and greedy stays the default here; a `PLMSampling`
passed to `NativeModel.plm_infer / synthesize_batch / synthesize_prompt_conditioned` (or the mirror's `sampling=`) makes
each step draw its code instead, on the GPU (csrc/sampling.hip), by the rule documented in include/megatts2_hip.h.  The
draw of utterance b at target position j uses u = (x0 >> 8) * 2^-24, x0 = the first word of Philox4x32-10 with key =
seed_b and counter = (j, 0, 0, 0) - `philox4x32_10` / `uniform` below compute the same numbers on the host.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass
from typing import Optional, Sequence, Union

import numpy as np

VQ_BINS = 1024

PHILOX_M0, PHILOX_M1 = 0xD2511F53, 0xCD9E8D57
PHILOX_W0, PHILOX_W1 = 0x9E3779B9, 0xBB67AE85
_MASK32 = 0xFFFFFFFF


class MT2Sampling(C.Structure):
    """ctypes mirror of `mt2_sampling` (include/megatts2_hip.h)."""
    _fields_ = [("temperature", C.c_float), ("top_k", C.c_int32), ("top_p", C.c_float), ("reserved", C.c_int32),
                ("seeds", C.POINTER(C.c_uint64))]


@dataclass(frozen=True)
class PLMSampling:
    """Decoding control of the PLM: temperature > 0, top_k in [0, vq_bins] (0 = all), top_p in (0, 1] (1 = off)."""
    temperature: float
    top_k: int = 0
    top_p: float = 1.0

    def __post_init__(self):
        t, p = float(self.temperature), float(self.top_p)
        if not (math.isfinite(t) and t > 0.0):
            raise ValueError(f"temperature must be finite and > 0, got {self.temperature!r}")
        if isinstance(self.top_k, bool) or int(self.top_k) != self.top_k or not 0 <= int(self.top_k) <= VQ_BINS:
            raise ValueError(f"top_k must be an integer in [0, {VQ_BINS}], got {self.top_k!r}")
        if not (p > 0.0 and p <= 1.0):
            raise ValueError(f"top_p must be in (0, 1], got {self.top_p!r}")
        object.__setattr__(self, "temperature", t)
        object.__setattr__(self, "top_k", int(self.top_k))
        object.__setattr__(self, "top_p", p)

    def to_c(self, seeds: np.ndarray) -> MT2Sampling:
        """The C struct over `seeds` (uint64 [B], host; the caller keeps the array alive during the call)."""
        assert seeds.dtype == np.uint64 and seeds.flags.c_contiguous
        return MT2Sampling(C.c_float(self.temperature), self.top_k, C.c_float(self.top_p), 0,
                           seeds.ctypes.data_as(C.POINTER(C.c_uint64)))


def seed_array(seeds: Union[None, int, Sequence[int], np.ndarray], B: int) -> np.ndarray:
    """uint64 [B] seeds: an int s means utterance b gets s + b; an array-like gives one per utterance; None = 0 + b."""
    if seeds is None:
        seeds = 0
    if hasattr(seeds, "detach"):
        seeds = seeds.detach().cpu().numpy()
    if np.ndim(seeds) == 0:
        s = int(seeds)
        return np.asarray([(s + b) & 0xFFFFFFFFFFFFFFFF for b in range(B)], np.uint64)
    a = np.asarray(seeds).reshape(-1)
    if a.size != B:
        raise ValueError(f"{a.size} seeds for {B} utterances")
    return np.ascontiguousarray([int(v) & 0xFFFFFFFFFFFFFFFF for v in a.tolist()], np.uint64)


def gamma_array(gamma, B: int) -> np.ndarray:
    """float32 [B] interpolation weights of `plm_infer_interpolated`: one float for every utterance or one per utterance, each
    in [0, 1] (0 = context A's prosody alone, 1 = context B's)."""
    if hasattr(gamma, "detach"):
        gamma = gamma.detach().cpu().numpy()
    a = np.asarray(gamma, np.float64)
    if a.ndim == 0:
        a = np.full(B, float(a))
    a = a.reshape(-1)
    if a.size != B:
        raise ValueError(f"{a.size} gamma values for {B} utterances")
    if not bool(np.all((a >= 0.0) & (a <= 1.0))):       # (False for NaN)
        raise ValueError(f"gamma must be in [0, 1], got {a.tolist()!r}")
    return np.ascontiguousarray(a, np.float32)


def philox4x32_10(ctr: Sequence[int], key: Sequence[int]):
    """Philox4x32-10 (Salmon et al., SC'11) on one counter block: 4 x u32 counter, 2 x u32 key -> 4 x u32."""
    c0, c1, c2, c3 = (int(v) & _MASK32 for v in ctr)
    k0, k1 = (int(v) & _MASK32 for v in key)
    for _ in range(10):
        p0, p1 = PHILOX_M0 * c0, PHILOX_M1 * c2
        c0, c1, c2, c3 = ((p1 >> 32) ^ c1 ^ k0, p1 & _MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & _MASK32)
        k0, k1 = (k0 + PHILOX_W0) & _MASK32, (k1 + PHILOX_W1) & _MASK32
    return c0, c1, c2, c3


def uniform(seed: int, position: int) -> float:
    """The u of utterance `seed` at target position `position` (exact: a multiple of 2^-24 in [0, 1))."""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    x0 = philox4x32_10((position, 0, 0, 0), (s & _MASK32, s >> 32))[0]
    return (x0 >> 8) * 2.0 ** -24


def as_sampling(sampling: Optional[PLMSampling]) -> Optional[PLMSampling]:
    if sampling is None or isinstance(sampling, PLMSampling):
        return sampling
    raise TypeError("sampling must be a PLMSampling (or None for greedy decoding)")
