"""The de-reverberation calls read no workspace bytes that they did not write (GPU): the three-step protocol of
tests/test_gpu_workspace_poison.py (its docstring; its helpers, by import) on mt2_dereverb and mt2_wpe_spectrum - an arena of 0x00
against one of 0xFF gives bit-equal outputs, a call of another geometry in front changes nothing, the arena beyond the high water
keeps its fill - and the high water of mt2_dereverb is mt2_dereverb_query's answer exactly.

Arena buffers the kernels read, from the code before the first run: the packed spectrum is memset whole before the per-utterance STFT
GEMMs write its 2 F columns; wpe_to_bins_kernel writes every cell of the columns of Y, the frames T_b .. Tp - 1 as zeros;
wpe_bin_kernel writes every cell of the columns of D (the same pad frames as zeros) and the five sums of every bin, and only those are
read by the way back and by the figures kernel.  No buffer of integers is written by the device."""
import numpy as np
import pytest

import wpe_ref as W
from test_gpu_workspace_poison import MiB, dev, one_chunk, protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RESERVE = 16 * MiB
SHAPES = {"B": (64, 130, 30), "A": (45, 64, 65, 17, 257)}      # frame counts; 30 and 17 are under delay + 4 taps: passed through


def audio():
    from megatts2_amd.config import AudioConfig
    return AudioConfig(sample_rate=16000, n_fft=128, hop_length=32, win_length=128, n_mels=8, f_min=0.0, f_max=8000.0)


def waves(which):
    xs = [W.spectrum_signal(audio(), T, seed=T, tail=(3 * i) % 32) for i, T in enumerate(SHAPES[which])]
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
    if name == "dereverb":
        return lambda: h.dereverb(w, lens, return_figures=True)
    Ts = 1 + lens // 32
    spec = torch.view_as_real(h.stft(w, lens))                                 # the input of the call below, made once
    packed = torch.full((len(Ts), int(Ts.max()) + 2, 132), float("nan"), device="cuda", dtype=torch.float32)
    for b, T in enumerate(Ts):
        packed[b, :T, :65] = spec[b, :T, :, 0]
        packed[b, :T, 65:130] = spec[b, :T, :, 1]
    return lambda: h.wpe_spectrum(packed, Ts, return_filters=True, return_figures=True)


def test_high_water_of_dereverb_is_the_query():
    """first, on a handle nothing else has used: the high-water mark is the most any call took since the handle was made"""
    from megatts2_amd import runtime as rt
    for which in ("B", "A"):
        h = rt.MelFrontEnd(audio())
        try:
            w, lens = waves(which)
            h.dereverb(w, lens, return_figures=True)
            torch.cuda.synchronize()
            assert h.workspace_high_water() == rt.dereverb_query(audio(), lens=lens)[0]
        finally:
            h.close()


@pytest.mark.parametrize("name", ["dereverb", "wpe_spectrum"])
def test_dereverb_calls(fe, name):
    protocol(fe, call(fe, name, "B"), call(fe, name, "A"), f"front end {name}")
