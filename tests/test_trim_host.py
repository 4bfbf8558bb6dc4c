"""Host side of the prompt-audio silence trimmer (no GPU): the float64 restatement of the rule (tests/trim_ref.py) on hand cases,
the library's host-only entry point mt2_trim_query against it, and audio_io.trim_alignment."""
import os

import numpy as np
import pytest

import trim_ref as T


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


@pytest.mark.parametrize("L", [1, 511, 512, 513, 2047, 2048, 2049, 5000, 16000])
def test_block_form_is_the_centred_frame_sum(L):
    x = T.burst_signal(L, "interior", seed=1)
    e, d = T.energies(x), T.energies_direct(x)
    assert e.shape == d.shape == (1 + L // 512,)
    assert np.abs(e - d).max() <= 1e-14 * d.max()


def test_burst_between_zeros_is_cut_to_multiples_of_the_hop():
    """zeros [0, 4096), a unit tone on [4096, 8192), zeros up to 16000: a frame's energy is the count of burst samples in its
    window (times 1/2), the threshold at 20 dB is 1 % of a full window: frames 7 .. 17 hold more than 20.48 burst samples"""
    x = np.zeros(16000)
    x[4096:8192] = np.sin(2 * np.pi * 1000.0 * np.arange(4096) / 16000.0)
    e = T.energies(x)
    assert e[:7].max() == 0.0 and e[18:].max() == 0.0 and e[7] > 0.01 * e.max() and e[17] > 0.01 * e.max()
    assert T.bounds(x, 20) == (7 * 512, 18 * 512)
    assert T.bounds(x, 40) == (7 * 512, 18 * 512)
    x += 1e-3                                         # a floor whose frames hold 2e-3 against the burst's 1e3: cut at 40 dB, kept at 100
    assert T.bounds(x, 40) == (7 * 512, 18 * 512)
    assert T.bounds(x, 100) == (0, 16000)


def test_silent_utterance_is_left_whole():
    assert T.bounds(np.zeros(5000), 20) == (0, 5000)
    assert T.bounds(np.full(5000, 1e-25), 20) == (0, 5000)          # squares underflow FLT_MIN
    assert T.margin(np.zeros(5000), 20) == np.inf


def test_single_click():
    """a click at sample 3000 lies in the windows of frames 4 .. 7 (512 f - 1024 <= 3000 < 512 f + 1024)"""
    x = np.zeros(8000)
    x[3000] = 1.0
    assert np.nonzero(T.energies(x))[0].tolist() == [4, 5, 6, 7]
    assert T.bounds(x, 20) == (4 * 512, 8 * 512)
    x = np.zeros(3500)                                # ... and the end is clamped to L
    x[3000] = 1.0
    assert T.bounds(x, 20) == (4 * 512, 3500)


def test_one_sample():
    assert T.energies(np.array([0.5])).tolist() == [0.25]
    assert T.bounds(np.array([0.5]), 20) == (0, 1)
    assert T.bounds(np.array([0.0]), 20) == (0, 1)


@pytest.mark.parametrize("L", [1, 511, 512, 513, 2048, 16000])
def test_query_matches_reference(rt, L):
    for top_db in (20, 40, 60, 33.5):
        frames, c = rt.trim_query(L, top_db)
        assert frames == 1 + L // 512 == T.energies(np.zeros(L)).size
        assert isinstance(c, np.float32) and c == np.float32(10 ** (-top_db / 10)) == T.factor(top_db)


@pytest.mark.parametrize("L, top_db", [(0, 20.0), (-5, 20.0), (2 ** 31, 20.0), (1000, 0.0), (1000, -20.0), (1000, float("nan")),
                                       (1000, float("inf"))])
def test_query_rejects(rt, L, top_db):
    with pytest.raises(rt.NativeError):
        rt.trim_query(L, top_db)
    assert rt.load_library().mt2_last_error()


def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_trim_query", "mt2_trim_silence"):
        assert hasattr(lib, name) and name in header
    assert "MT2_TRIM_FRAME 2048" in header and "MT2_TRIM_HOP 512" in header
    assert (rt.TRIM_FRAME, rt.TRIM_HOP) == (T.FRAME, T.HOP)


# ---- trim_alignment ----------------------------------------------------------------------------------------------------------

def align(tok, dur, start, end, hop=256):
    from megatts2_amd import audio_io
    t, d = audio_io.trim_alignment(np.asarray(tok), np.asarray(dur, np.int32), start, end, hop)
    assert d.dtype == np.int32
    return t.tolist(), d.tolist()


def test_alignment_hand_example():
    """5 phones over 20 frames (5120 samples at hop 256, T = 1 + 5120 // 256 = 21 with the centred last frame on phone 9's
    account); the audio cut to [1024, 3584): frames [4, 4 + 11) = 4 .. 14"""
    tok, dur = [5, 6, 7, 8, 9], [3, 4, 5, 2, 7]            # spans [0,3) [3,7) [7,12) [12,14) [14,21)
    assert align(tok, dur, 1024, 3584) == ([6, 7, 8, 9], [3, 5, 2, 1])
    assert align(tok, dur, 1024, 3584) == T.trim_alignment(tok, dur, 1024, 3584)


def test_alignment_sums_to_the_cut_frames_and_drops_phones():
    rng = np.random.default_rng(3)
    for _ in range(50):
        dur = rng.integers(0, 9, rng.integers(1, 12)).tolist()
        total = sum(dur)
        if total < 1:
            continue
        tok = list(range(100, 100 + len(dur)))
        L = (total - 1) * 256 + int(rng.integers(0, 256))           # a length with 1 + L // 256 == total
        start = 512 * int(rng.integers(0, L // 512 + 1))
        end = int(rng.integers(start, L + 1))
        got = align(tok, dur, start, end)
        assert got == T.trim_alignment(tok, dur, start, end)
        assert sum(got[1]) == 1 + (end - start) // 256 and min(got[1]) >= 1
        assert got[0] == sorted(got[0]) and set(got[0]) <= set(tok)


def test_alignment_cut_inside_a_phone_and_dropped_phones():
    tok, dur = [1, 2, 3], [10, 10, 10]                       # 30 frames: L in [7424, 7680)
    assert align(tok, dur, 12 * 256, 14 * 256 + 7) == ([2], [3])          # frames 12, 13, 14: phones 1 and 3 are gone
    assert align(tok, dur, 5 * 256, 7500) == ([1, 2, 3], [5, 10, 10])     # 1 + (7500 - 1280) // 256 = 25 frames from frame 5


def test_alignment_without_a_cut_is_its_input():
    tok, dur = [4, 2, 9, 2], [6, 1, 8, 5]                    # 20 frames = 1 + L // 256 for L = 5000
    assert align(tok, dur, 0, 5000) == (tok, dur)


def test_alignment_errors():
    from megatts2_amd import audio_io
    tok, dur = np.array([4, 2, 9]), np.array([6, 1, 8], np.int32)          # 15 frames
    with pytest.raises(ValueError):
        audio_io.trim_alignment(tok, dur, 100, 3000)                       # start inside a mel frame
    with pytest.raises(ValueError):
        audio_io.trim_alignment(tok, dur, 0, 15 * 256)                     # 16 frames wanted, 15 aligned
    with pytest.raises(ValueError):
        audio_io.trim_alignment(tok, dur, 1024, 1024 + 12 * 256)           # frames [4, 17) reach beyond 15
    for bad in ((100, 3000), (0, 15 * 256)):
        with pytest.raises(ValueError):
            T.trim_alignment(tok.tolist(), dur.tolist(), *bad)
