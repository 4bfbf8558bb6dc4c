"""The noise-suppression calls read no workspace bytes that they did not write (GPU): the three-step protocol of
tests/test_gpu_workspace_poison.py (its docstring; its helpers, by import) on mt2_denoise, mt2_noise_floor and mt2_spectral_gain - an
arena of 0x00 against one of 0xFF gives bit-equal outputs, a call of another geometry in front changes nothing, the arena beyond the
high water keeps its fill - and the high water of mt2_denoise is mt2_denoise_query's answer exactly.

Arena buffers the kernels read, from the code before the first run: the packed spectrum is memset whole before the per-utterance STFT
GEMMs write its 2 F columns (the pad columns meet zero basis columns in the inverse GEMM); dn_power_kernel writes all Fp columns of
every row of P below T_b, and nothing reads a row at or beyond it; the floor's pad columns are written by the select; the tile sums
of the tiles below T_b are written by the gain kernel and only those are read by the figures kernel.  No buffer of integers is written
by the device."""
import numpy as np
import pytest

import denoise_ref as D
from test_gpu_workspace_poison import MiB, dev, one_chunk, protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RESERVE = 16 * MiB
SHAPES = {"B": (37, 130, 4), "A": (5, 64, 65, 17, 257)}      # frame counts


def audio():
    from megatts2_amd.config import AudioConfig
    return AudioConfig(sample_rate=16000, n_fft=128, hop_length=32, win_length=128, n_mels=8, f_min=0.0, f_max=8000.0)


def waves(which):
    xs = [(D.tone((T - 1) * 32 + 3 * i, 16000, hz=1000.0) + D.white_noise((T - 1) * 32 + 3 * i, seed=T)).astype(np.float32)
          for i, T in enumerate(SHAPES[which])]
    lens = np.asarray([len(x) for x in xs], np.int32)
    w = np.full((len(xs), int(lens.max()) + 5), np.nan, np.float32)
    for b, x in enumerate(xs):
        w[b, :len(x)] = x
    return dev(w), lens


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    h = one_chunk(MelFrontEnd(audio()), RESERVE)
    yield h
    h.close()


def call(h, name, which):
    w, lens = waves(which)
    if name == "denoise":
        return lambda: h.denoise(w, lens, return_floor=True, return_figures=True)
    Ts = 1 + lens // 32
    spec = torch.view_as_real(h.stft(w, lens))                                 # inputs of the calls below, made once
    packed = torch.full((len(Ts), int(Ts.max()) + 2, 132), float("nan"), device="cuda", dtype=torch.float32)
    for b, T in enumerate(Ts):
        packed[b, :T, :65] = spec[b, :T, :, 0]
        packed[b, :T, 65:130] = spec[b, :T, :, 1]
    if name == "noise_floor":
        return lambda: h.noise_floor(packed, Ts)
    floor = h.noise_floor(packed, Ts)
    return lambda: h.spectral_gain(packed, floor, Ts, return_gain=True, apply=True)


def test_high_water_of_denoise_is_the_query():
    """first, on a handle nothing else has used: the high-water mark is the most any call took since the handle was made"""
    from megatts2_amd import runtime as rt
    for which in ("B", "A"):
        h = rt.MelFrontEnd(audio())
        try:
            w, lens = waves(which)
            h.denoise(w, lens, return_figures=True)
            torch.cuda.synchronize()
            assert h.workspace_high_water() == rt.denoise_query(audio(), lens=lens)[0]
        finally:
            h.close()


@pytest.mark.parametrize("name", ["denoise", "noise_floor", "spectral_gain"])
def test_denoise_calls(fe, name):
    protocol(fe, call(fe, name, "B"), call(fe, name, "A"), f"front end {name}")
