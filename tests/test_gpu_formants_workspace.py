"""The formant calls read no workspace bytes that they did not write (GPU): the three-step protocol of
tests/test_gpu_workspace_poison.py (its docstring; its helpers, by import) on mt2_lpc_formants with every optional output, on
mt2_formant_stats and on megatts2.extract_formants - an arena of 0x00 against one of 0xFF gives bit-equal outputs, a call of another
geometry in front changes nothing, the arena beyond the high water keeps its fill.  (That the high water of mt2_lpc_formants is
mt2_formant_query's answer: tests/test_gpu_formants.py.)

Arena buffers the kernels read, from the code before the first run: formants_kernel reads len[b] for b < B - the first B words of the
call's plan, which formant_run sends in the call's one upload before the launch; the room behind them, up to the 65535 words the plan
is given whatever B, is never read.  The window table is not in the arena: it lies in an allocation of the handle's own, written once
by a synchronous copy before the first launch that reads it.  formant_stats_kernel reads frame_len[b] for b < B, the plan of its call,
likewise.  extract_formants adds the resampler in front: its plan (the tile lists, the lengths in and out) is uploaded whole before
resample_rows_kernel reads it, and no peak words are used without normalisation.  Both batches are ragged, so rows that are never
written lie between rows that are."""
import numpy as np
import pytest

import formant_ref as F
from test_gpu_workspace_poison import MiB, dev, one_chunk, protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RESERVE = 16 * MiB


def waves(which):
    xs = {"B": [F.voiced_signal(5000), np.zeros(700, np.float32), np.array([0.25], np.float32), F.noise_signal(2307, 2)],
          "A": [F.noise_signal(275, 3), F.voiced_signal(9000, period=55), F.noise_signal(176, 4)]}[which]
    lens = np.asarray([len(v) for v in xs], np.int32)
    w = np.full((len(xs), int(lens.max()) + 5), np.nan, np.float32)
    for b, v in enumerate(xs):
        w[b, :len(v)] = v
    return dev(w), lens


def tracks(which):
    rng = np.random.default_rng(3 if which == "B" else 4)
    fl = np.asarray([700, 1, 257, 64] if which == "B" else [65, 1030, 300], np.int32)
    T = int(fl.max()) + 2
    freq = np.full((len(fl), T, 5), np.nan, np.float32)
    count = np.full((len(fl), T), 5, np.int32)
    f0 = np.full((len(fl), T), np.nan, np.float32)
    for b, n in enumerate(fl):
        freq[b, :n] = np.sort(rng.uniform(200.0, 5000.0, (n, 5)), axis=1)
        count[b, :n] = rng.integers(3, 6, n)
        f0[b, :n] = rng.uniform(80.0, 300.0, n) * (rng.random(n) < 0.7)
    return dev(freq), dev(count), dev(f0), fl


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    h = one_chunk(MelFrontEnd(), RESERVE)
    yield h
    h.close()


def call(h, name, which, monkeypatch):
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime as rt
    if name == "formant_stats":
        freq, count, f0, fl = tracks(which)
        return lambda: h.formant_stats(freq, count, f0, fl)
    w, lens = waves(which)
    if name == "formants":
        cfg = rt.Formants(order=12 if which == "B" else 8, window_ms=50.0 if which == "B" else 20.0)
        return lambda: h.formants(w, lens, cfg, hop=176, sample_rate=11000, return_lpc=True, return_err=True, return_autocorr=True,
                                  return_roots=True, return_iters=True)
    monkeypatch.setattr(M, "_FRONTEND", h)                    # extract_formants runs on the module's front end: this handle
    return lambda: M.extract_formants(w, 16000 if which == "B" else 22050, lens)


@pytest.mark.parametrize("name", ["formants", "formant_stats", "extract_formants"])
def test_formant_calls(fe, name, monkeypatch):
    protocol(fe, call(fe, name, "B", monkeypatch), call(fe, name, "A", monkeypatch), f"front end {name}")
