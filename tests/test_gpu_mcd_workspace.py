"""The mel-cepstral-distortion calls read no workspace bytes that they did not write (GPU): the three-step protocol of
tests/test_gpu_workspace_poison.py (its docstring; its helpers, by import) on mt2_mel_cepstrum, mt2_path_distortion and
mt2_mel_cepstral_distortion - an arena of 0x00 against one of 0xFF gives bit-equal outputs, a call of another geometry in front
changes nothing, the arena beyond the high water keeps its fill - and the whole chain's high water is mt2_mcd_query's answer exactly.

Arena buffers of integers that the device writes: the DTW's packed directions (see that file) and, new here, the chain's lo | hi |
steps: dtw_backtrack_kernel writes lo[j] / hi[j] of every column, -1 beyond the length, before mcd_path_kernel reads them, and that
kernel cuts every run to the rows of the cepstra whatever the words hold."""
import numpy as np
import pytest

import mcd_ref as R
from test_gpu_workspace_poison import MiB, dev, one_chunk, pad_stack, protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RESERVE = 16 * MiB
SHAPES = {"B": ((40, 50), (17, 9), (64, 65)), "A": ((9, 30), (70, 20), (1, 5), (33, 33), (2, 1))}


def inputs(which, N=80):
    mels_a, mels_b, f0_a, f0_b = [], [], [], []
    for n, (Ta, Tb) in enumerate(SHAPES[which]):
        rng = np.random.default_rng(10 * n + len(which))
        A = R.log_mel(Ta, N, seed=50 + n)
        mels_a.append(A)
        mels_b.append((A[np.minimum(np.arange(Tb) * Ta // Tb, Ta - 1)] + 0.2 * rng.standard_normal((Tb, N))).astype(np.float32))
        fa, fb = (100.0 + 50.0 * rng.random(Ta)).astype(np.float32), (100.0 + 50.0 * rng.random(Tb)).astype(np.float32)
        fa[::5], fb[::7] = 0.0, np.nan
        f0_a.append(fa), f0_b.append(fb)
    (A, al), (Bm, bl) = pad_stack(mels_a, fill=np.nan), pad_stack(mels_b, fill=np.nan)
    return dev(A), dev(Bm), al, bl, dev(pad_stack(f0_a, fill=np.nan)[0]), dev(pad_stack(f0_b, fill=np.nan)[0])


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    h = one_chunk(MelFrontEnd(), RESERVE)
    yield h
    h.close()


def call(h, name, which):
    A, Bm, al, bl, fa, fb = inputs(which)
    if name == "mcd":
        return lambda: h.mcd(A, Bm, al, bl, fa, fb, order=13, return_path=True)
    if name == "mel_cepstrum":
        return lambda: h.mel_cepstrum(A, al, 13)
    ca, cb = h.mel_cepstrum(A, al, 13), h.mel_cepstrum(Bm, bl, 13)      # inputs of the call below, made once
    path = h.dtw(ca, cb, al, bl)
    return lambda: h.path_distortion(ca, cb, path["lo"], path["hi"], al, bl, fa, fb)


def test_high_water_of_the_whole_chain_is_the_query():
    """first, on a handle nothing else has used: the high-water mark is the most any call took since the handle was made"""
    from megatts2_amd import runtime as rt
    for which in ("B", "A"):
        h = rt.MelFrontEnd()
        try:
            A, Bm, al, bl, fa, fb = inputs(which)
            h.mcd(A, Bm, al, bl, fa, fb, order=13)
            torch.cuda.synchronize()
            assert h.workspace_high_water() == rt.mcd_query(A.shape[1], Bm.shape[1], 80, 13, A.shape[0])
        finally:
            h.close()


@pytest.mark.parametrize("name", ["mcd", "mel_cepstrum", "path_distortion"])
def test_mcd_calls(fe, name):
    protocol(fe, call(fe, name, "B"), call(fe, name, "A"), f"front end {name}")
