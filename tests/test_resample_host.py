"""Host side of the prompt-audio resampler (no GPU): the float64 restatement of the rule (tests/resample_ref.py) against analytic
tones, and the library's host-only entry points - filter table, length rule, rejections - against that restatement."""
import ctypes
import math
import os

import numpy as np
import pytest

import resample_ref as R

SR_OUT = 16000


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


@pytest.mark.parametrize("sr_in", R.RATES)
def test_reference_reproduces_tones_at_the_new_rate(sr_in):
    """Away from the edges (the filter reaches 2 * width input samples = 2 * width * n / o output samples) the resampled
    three-tone signal is the same three tones sampled at 16 kHz, to 1e-7 (measured 1.4e-8 .. 3.2e-8 at amplitude 3)."""
    o, n, width, _ = R.rule(sr_in, SR_OUT)
    L = sr_in // 4 + 37
    y = R.resample(R.tones(sr_in, L, sr_in), sr_in, SR_OUT)
    assert y.size == math.ceil(n * L / o)
    edge = math.ceil(2 * width * n / o) + 4
    assert y.size > 2 * edge + 1000
    err = np.abs(y - R.tones(SR_OUT, y.size, sr_in))[edge:-edge].max()
    print(sr_in, "max abs error against the analytic tones", err)
    assert err <= 1e-7


@pytest.mark.parametrize("sr_in", R.RATES)
def test_table_matches_reference(rt, sr_in):
    """one f32 rounding of the float64 filter, plus room for another double-precision I0"""
    h32, h64 = rt.resample_table(sr_in, SR_OUT), R.table(sr_in, SR_OUT)
    assert h32.shape == h64.shape and h32.dtype == np.float32
    assert (np.abs(h32.astype(np.float64) - h64) <= 2.0 ** -23 * np.abs(h64) + 1e-12).all()
    assert np.abs(h64).sum(axis=1).max() <= 2.59


@pytest.mark.parametrize("sr_in", R.RATES)
def test_query_matches_reference(rt, sr_in):
    o, n, _, K = R.rule(sr_in, SR_OUT)
    for L in (1, o - 1, o, o + 1, 1000, 2 ** 31 - 1):
        assert rt.resample_query(sr_in, SR_OUT, L) == (R.out_len(sr_in, SR_OUT, L), o, n, K)


def test_rule_table_of_the_issue():
    assert [R.rule(sr, SR_OUT)[:2] + R.rule(sr, SR_OUT)[3:] for sr in R.RATES] == [
        (3, 1, 409), (441, 160, 815), (441, 320, 629), (3, 2, 207), (1, 2, 137), (2, 1, 274), (441, 640, 577)]


def test_exports(rt):
    lib = rt.load_library()
    for name in ("mt2_resample_query", "mt2_resample_table", "mt2_resample"):
        assert hasattr(lib, name)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_resample_query", "mt2_resample_table", "mt2_resample", "MT2_RESAMPLE_NORMALIZE"):
        assert name in header


@pytest.mark.parametrize("sr_in, sr_out", [(0, 16000), (-44100, 16000), (44100, 0), (16000, -1), (16000, 16000), (16001, 16000)])
def test_host_entries_reject(rt, sr_in, sr_out):
    with pytest.raises(rt.NativeError):
        rt.resample_query(sr_in, sr_out, 1000)
    lib, word = rt.load_library(), np.full(4, 7.0, np.float32)
    assert lib.mt2_resample_table(sr_in, sr_out, word.ctypes.data_as(ctypes.c_void_p)) != 0
    assert (word == 7.0).all() and lib.mt2_last_error()


def test_load_audio_still_rejects_another_rate(tmp_path):
    from megatts2_amd import audio_io
    path = str(tmp_path / "p22050.wav")
    audio_io.write_wav(path, 0.5 * R.tones(22050, 2205, 22050).astype(np.float32) / 3, 22050)
    assert audio_io.read_wav(path)[1] == 22050
    with pytest.raises(ValueError):
        audio_io.load_audio(path)
    with pytest.raises(ValueError):
        audio_io.load_audio(path, 16000)
