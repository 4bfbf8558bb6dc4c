"""The formant tracker reads no workspace bytes that it did not write (GPU): the three-step protocol of
tests/test_gpu_workspace_poison.py (its docstring; its helpers, by import) on mt2_formant_track with sel and on
megatts2.track_formants - an arena of 0x00 against one of 0xFF gives bit-equal outputs, a call of another geometry in front changes
nothing, the arena beyond the high water keeps its fill.  (That the high water is mt2_formant_track_query's answer:
tests/test_gpu_formant_track.py.)

Arena bytes formant_track_kernel reads, from the code before the first run.  (1) len[b] for b < B: the first B words of the room of
65535 that formant_track_run carves first and fills by the call's one upload, enqueued on the stream before the launch; the words
behind them are never read.  (2) psi, 16 bytes a frame: the workgroup of utterance b writes the rows of its frames t < len[b] in its
forward pass - each of the 16 bytes, the ten predecessors and the six zeros behind them, staged in LDS (cleared per tile) and stored as
one uint4 per frame - and its backward pass, behind a barrier of the same workgroup, reads exactly those rows back, a tile at a time; the
rows of the frames in [len[b], T_max) are neither written nor read, and no workgroup touches another utterance's rows.  Both batches are
ragged, so psi rows that are never written lie between rows that are."""
import numpy as np
import pytest

import formant_track_ref as R
from test_gpu_workspace_poison import MiB, dev, one_chunk, protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RESERVE = 16 * MiB


def candidates(which):
    """two ragged geometries: scene rows cut across the 64-frame tile, NaN behind every row and behind count"""
    cuts = (130, 1, 64, 257) if which == "B" else (65, 300, 63)
    T = max(cuts) + 2
    freq = np.full((len(cuts), T, 5), np.nan, np.float32)
    bw = np.full((len(cuts), T, 5), np.nan, np.float32)
    count = np.full((len(cuts), T), 5, np.int32)
    for b, n in enumerate(cuts):
        f, w, c, _, _ = R.scene(10 + b, max(n, 2))
        behind = np.arange(5)[None, :] >= c[:, None]
        f[behind], w[behind] = np.nan, np.nan
        freq[b, :n], bw[b, :n], count[b, :n] = f[:n], w[:n], c[:n]
    return dev(freq), dev(bw), dev(count), np.asarray(cuts, np.int32)


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    h = one_chunk(MelFrontEnd(), RESERVE)
    yield h
    h.close()


def call(h, name, which, monkeypatch):
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime as rt
    freq, bw, count, fl = candidates(which)
    track = rt.FormantTrack(tracks=4 if which == "B" else 3, jump_cost=1.0 if which == "B" else 2.0)
    if name == "formant_track":
        return lambda: h.formant_track(freq, bw, count, fl, track, return_sel=True)
    monkeypatch.setattr(M, "_FRONTEND", h)                    # track_formants runs on the module's front end: this handle
    return lambda: M.track_formants(freq, bw, count, fl, track)


@pytest.mark.parametrize("name", ["formant_track", "track_formants"])
def test_formant_track_calls(fe, name, monkeypatch):
    protocol(fe, call(fe, name, "B", monkeypatch), call(fe, name, "A", monkeypatch), f"front end {name}")
