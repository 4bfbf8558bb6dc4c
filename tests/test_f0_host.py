"""Host side of the F0 tracker (no GPU): the restatement of the YIN rule (tests/f0_ref.py) against ground truth - the pitch of an
analytic tone is known -, on hand cases, its moments against plain numpy formulas, and the library's host-only entry point
mt2_f0_query against the rule.

The tones: a sum of harmonics with phases 0.3 k, peak 0.5, plus 1e-3 Gaussian noise, in f32, at L = 8000.  Observed over the
8 frequencies x 3 harmonic sets: 0.04 .. 0.73 cents from the truth on interior frames, cmnd <= 0.018; 0.1-rms white noise has
cmnd >= 0.78 everywhere."""
import math
import os

import numpy as np
import pytest

import f0_ref as R

L_TONE = 8000


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


@pytest.mark.parametrize("harm", range(len(R.HARMONICS)))
@pytest.mark.parametrize("f", R.FREQS)
def test_tones_are_within_a_cent_of_the_truth(f, harm):
    x = R.tone(f, L_TONE, R.HARMONICS[harm])
    f0, cmnd, lag, d = R.yin(x)
    inner = R.interior(L_TONE)
    assert inner == list(range(2, 30))
    assert (f0[inner] > 0).all() and (cmnd[inner] < 0.15).all()
    c = np.abs(R.cents(f0[inner], f))
    print(f"{f} Hz {R.HARMONICS[harm]}: {c.min():.3g} .. {c.max():.3g} cents, cmnd <= {cmnd[inner].max():.3g}")
    assert c.max() <= 1.0
    assert cmnd[inner].max() <= 0.018
    assert (d[:, 0] == 0).all()


def test_noise_and_silence_are_unvoiced():
    f0, cmnd, _, _ = R.yin(R.white(L_TONE, 0.1))
    print(f"white noise: min cmnd {cmnd.min():.3g}")
    assert not f0.any() and cmnd.min() >= 0.15
    f0, cmnd, lag, d = R.yin(np.zeros(L_TONE, np.float32))
    assert not f0.any() and (cmnd == 1.0).all() and not d.any()
    assert (lag == R.lags()[0]).all()                      # every d' is 1: the first lag attains the minimum


@pytest.mark.parametrize("P", [37, 100, 181, 256])
def test_table_periodic_signal_has_a_zero_at_its_period(P):
    """x[n] = tab[n % P]: every term of d[P] is a difference of equal samples"""
    tab = np.random.default_rng(P).standard_normal(P).astype(np.float32)
    x = tab[np.arange(L_TONE) % P]
    f0, cmnd, lag, d = R.yin(x)
    inner = R.interior(L_TONE)
    assert (d[inner, P] == 0).all()
    assert (lag[inner] == P).all() and (cmnd[inner] == 0).all()
    if P < 256:                                            # refined: with b = 0 and a, c >= 0, |delta| = |a - c| / (2 (a + c)) <= 1 / 2
        assert (f0[inner] >= R.SR / (P + 0.5)).all() and (f0[inner] <= R.SR / (P - 0.5)).all()
    else:                                                  # no right neighbour: delta = 0
        assert (f0[inner] == R.SR / P).all()
    g0, gm, gl = R.decide(d, dtype=np.float32)
    assert (gl[inner] == P).all() and g0.dtype == np.float32


def test_one_sample():
    f0, cmnd, lag, d = R.yin(np.array([0.5], np.float32))
    assert f0.shape == (1,) and f0[0] == 0 and not cmnd[0] < 0.15
    assert d[0, 0] == 0 and d.shape == (1, 257)


def test_float32_steps_follow_float64():
    x = R.mixed()
    d = R.difference(x)
    f64, c64, l64 = R.decide(d)
    f32, c32, l32 = R.decide(d, dtype=np.float32)
    assert f32.dtype == c32.dtype == np.float32 and len(f64) == 63
    clear = (c64 < 0.075) | (c64 > 0.3)
    assert (~clear).sum() <= 8
    assert np.array_equal((f32 > 0)[clear], (f64 > 0)[clear])
    assert np.abs(c32 - c64).max() <= 1e-4


def test_nan_never_wins_the_minimum():
    dp = np.full(257, np.nan)
    assert R.choose(dp, 32, 256, 0.15) == 32
    dp[100], dp[200] = 0.5, 0.5
    assert R.choose(dp, 32, 256, 0.15) == 100
    dp[150] = 0.1
    dp[151], dp[152], dp[153] = 0.05, np.nan, 0.01        # the walk stops in front of a NaN
    assert R.choose(dp, 32, 256, 0.15) == 151


# ---- moments -------------------------------------------------------------------------------------------------------------------

def test_moments_against_numpy_formulas():
    rng = np.random.default_rng(5)
    f = np.where(rng.random(300) < 0.6, rng.uniform(80, 400, 300), 0.0).astype(np.float32)
    m = R.moments(f, 250)
    v = f[:250][f[:250] > 0].astype(np.float64)
    assert m[0] == v.size and m[1] == v.size / 250
    assert m[2] == pytest.approx(v.mean(), rel=1e-14) and m[3] == pytest.approx(v.std(), rel=1e-13)
    z = (v - v.mean()) / v.std()
    assert m[4] == pytest.approx(np.mean(z ** 3), rel=1e-11) and m[5] == pytest.approx(np.mean(z ** 4) - 3, rel=1e-11)
    assert not R.moments(np.zeros(10)).any()
    assert R.moments(np.array([0, 220.0, 0])).tolist() == [1, 1 / 3, 220.0, 0, 0, 0]
    assert R.moments(np.full(7, 220.0)).tolist() == [7, 1, 220.0, 0, 0, 0]


# ---- exports and query ---------------------------------------------------------------------------------------------------------

def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_f0_query", "mt2_f0_yin", "mt2_f0_stats"):
        assert hasattr(lib, name) and name in header
    assert "MT2_F0_FRAME 1024" in header and "MT2_F0_WINDOW 768" in header and "MT2_F0_MAX_LAG 256" in header
    assert (rt.F0_FRAME, rt.F0_WINDOW, rt.F0_MAX_LAG) == (R.FRAME, R.WINDOW, R.MAX_LAG)
    assert hasattr(rt.MelFrontEnd, "f0") and hasattr(rt.MelFrontEnd, "f0_stats")
    from megatts2_amd import megatts2 as M
    assert callable(M.extract_f0) and callable(M.pitch_stats)
    unit = open(os.path.join(root, "megatts2_amd", "csrc", "f0.hip")).read()
    assert "Cheveign" in unit and "__fdiv_rn" in unit


@pytest.mark.parametrize("hop", [256, 80])
@pytest.mark.parametrize("L", [1, 255, 256, 257, 8000])
def test_query_matches_the_rule(rt, L, hop):
    frames, lo, hi, ws = rt.f0_query(L, hop=hop)
    assert frames == 1 + L // hop == R.frames(L, hop) == R.difference(np.zeros(L), hop).shape[0]
    assert (lo, hi) == (32, 256) == R.lags()
    assert ws >= 4
    for fmin, fmax in ((80.0, 400.0), (62.5, 1000.0), (100.0, 8000.0), (70.0, 493.9)):
        assert rt.f0_query(L, hop=hop, fmin=fmin, fmax=fmax)[1:3] == R.lags(R.SR, fmin, fmax) == \
            (math.ceil(R.SR / fmax), math.floor(R.SR / fmin))


@pytest.mark.parametrize("kw", [
    dict(hop=0), dict(hop=1025), dict(hop=-256),
    dict(fmin=0.0), dict(fmin=-62.5), dict(fmin=float("nan")), dict(fmin=float("inf")),
    dict(fmax=0.0), dict(fmax=-500.0), dict(fmax=float("nan")), dict(fmax=float("inf")),
    dict(fmin=62.0),                     # tau_max = 258 > 256
    dict(fmin=30.0),
    dict(fmax=16000.0),                  # tau_min = 1
    dict(fmin=500.0, fmax=500.0),        # tau_min == tau_max
    dict(fmin=500.0, fmax=62.5),         # tau_min > tau_max
    dict(L=0), dict(L=-1), dict(L=2 ** 31),
])
def test_query_rejects(rt, kw):
    assert rt.f0_query(8000, fmin=62.5, fmax=8000.0)[1:3] == (2, 256)          # the widest range the rule takes
    kw = dict(kw)
    L = kw.pop("L", 8000)
    with pytest.raises(rt.NativeError):
        rt.f0_query(L, **kw)
    assert rt.load_library().mt2_last_error()
    if L == 8000 and "hop" not in kw:
        with pytest.raises(ValueError):
            R.lags(R.SR, kw.get("fmin", 62.5), kw.get("fmax", 500.0))
