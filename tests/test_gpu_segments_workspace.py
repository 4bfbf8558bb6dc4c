"""The segment calls read no workspace bytes that they did not write (GPU): the three-step protocol of
tests/test_gpu_workspace_poison.py (its docstring; its helpers, by import) on mt2_segment_frames, mt2_speech_segments and
mt2_cut_pauses - an arena of 0x00 against one of 0xFF gives bit-equal outputs, a call of another geometry in front changes nothing, the
arena beyond the high water keeps its fill.  (That the high water is mt2_segments_query's answer: tests/test_gpu_segments.py.)

Arena buffers the kernels read, from the code before the first run: the trim's block sums s[j] are written for every block of an
utterance and read behind the same bound; its peak words are memset.  segments_smooth_kernel writes prv[f] in passes 1, 3 and 5 and
fb, fc, fd, dst in passes 2, 4, 6 and 7 for every f < F_b before a later pass reads them, and reads no entry at or beyond F_b; it
writes all eight words of every utterance, which the figures and copy kernels read.  Both batches are ragged, so rows that are never
written lie between rows that are."""
import numpy as np
import pytest

import segments_ref as S
import trim_ref as T
from test_gpu_workspace_poison import MiB, dev, one_chunk, protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RESERVE = 16 * MiB


def waves(which):
    xs = {"B": [S.plan_signal(seed=1), np.zeros(3000, np.float32), np.array([0.25], np.float32), T.burst_signal(20000, "interior", seed=2)],
          "A": [T.burst_signal(700, "end"), S.plan_signal(plan=S.PLAN * 3, seed=2), T.burst_signal(32768, "start")]}[which]
    lens = np.asarray([len(v) for v in xs], np.int32)
    w = np.full((len(xs), int(lens.max()) + 5), np.nan, np.float32)
    for b, v in enumerate(xs):
        w[b, :len(v)] = v
    return dev(w), lens


def contours(which):
    rng = np.random.default_rng(3 if which == "B" else 4)
    fl = np.asarray([700, 1, 257, 64] if which == "B" else [65, 1030, 300], np.int32)
    e = np.full((len(fl), int(fl.max()) + 2), np.nan, np.float32)
    for b, F in enumerate(fl):
        e[b, :F] = rng.random(F) < 0.6
    return dev(e), fl


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    h = one_chunk(MelFrontEnd(), RESERVE)
    yield h
    h.close()


def call(h, name, which):
    from megatts2_amd import runtime as rt
    if name == "segment_frames":
        e, fl = contours(which)
        return lambda: h.segment_frames(e, fl, rt.segments_config(10.0, 3, 2, 1))
    w, lens = waves(which)
    if name == "speech_segments":
        return lambda: h.speech_segments(w, lens, rt.Pauses(), return_energy=True)
    out = torch.zeros_like(w)
    return lambda: h.cut_pauses(w, lens, rt.Pauses(), keep=name.split()[1], out=out, return_segments=True, return_figures=True)


@pytest.mark.parametrize("name", ["segment_frames", "speech_segments", "cut speech", "cut pauses"])
def test_segment_calls(fe, name):
    protocol(fe, call(fe, name, "B"), call(fe, name, "A"), f"front end {name}")
