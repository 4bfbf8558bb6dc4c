"""The declipping calls read no workspace bytes that they did not write (GPU): the three-step protocol of
tests/test_gpu_workspace_poison.py (its docstring; its helpers, by import) on mt2_declip and mt2_clip_detect - an arena of 0x00 against
one of 0xFF gives bit-equal outputs, a call of another geometry in front changes nothing, the arena beyond the high water keeps its
fill - and the high water of either call is mt2_declip_query's answer exactly.

Arena buffers the kernels read, from the code before the first run: dc_detect_kernel writes all eight detection words of every
utterance; dc_frame_kernel writes the whole frame row and the iteration count of every frame t < T_b of an utterance with a clipped
side, and the overlap and figures kernels read the rows and counts of those utterances only.  Both batches mix clipped, unclipped and
non-finite utterances, so rows that are never written lie between rows that are."""
import numpy as np
import pytest

import declip_ref as D
from test_gpu_workspace_poison import MiB, dev, one_chunk, protocol

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RESERVE = 16 * MiB
N = 256


def waves(which):
    x = D.make_signal(N, 3, length=3000)
    nan = D.clip(x[:700], 0.3)
    nan[5] = np.nan
    xs = {"B": [D.clip(x[:1500], 0.3), x[:999].copy(), D.clip(x[:64], 0.2), nan],
          "A": [x[:130].copy(), D.clip(x, 0.5), D.clip(x[:65], 0.2)]}[which]
    lens = np.asarray([len(v) for v in xs], np.int32)
    w = np.full((len(xs), int(lens.max()) + 5), np.nan, np.float32)
    for b, v in enumerate(xs):
        w[b, :len(v)] = v
    return dev(w), lens


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    h = one_chunk(MelFrontEnd(), RESERVE)
    yield h
    h.close()


def call(h, name, which):
    from megatts2_amd.runtime import Declip
    w, lens = waves(which)
    if name == "clip_detect":
        return lambda: (h.clip_detect(w, lens, Declip(frame=N)),)
    out = torch.zeros_like(w)
    return lambda: h.declip(w, lens, Declip(frame=N), return_figures=True, return_iters=True, out=out)


def test_high_water_is_the_query():
    """first, on a handle nothing else has used: the high-water mark is the most any call took since the handle was made"""
    from megatts2_amd import runtime as rt
    for name, col in (("clip_detect", 1), ("declip", 0)):
        for which in ("B", "A"):
            h = rt.MelFrontEnd()
            try:
                call(h, name, which)()
                torch.cuda.synchronize()
                assert h.workspace_high_water() == rt.declip_query(lens=waves(which)[1], declip=rt.Declip(frame=N))[col]
            finally:
                h.close()


@pytest.mark.parametrize("name", ["declip", "clip_detect"])
def test_declip_calls(fe, name):
    protocol(fe, call(fe, name, "B"), call(fe, name, "A"), f"front end {name}")
