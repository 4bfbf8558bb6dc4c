"""Host side of the second F0 tracker (no GPU): the restatement of its rule (tests/f0_track_ref.py: a Viterbi pass over YIN's lag
costs) on hand cases and against ground truth - the pitch of an analytic signal is known -, in float64 and in float32, and the
library's host-only entry point mt2_f0_track_query against the documented byte formula.

Observed with the default costs (octave 0.02, jump 0.5): the 24 tones 0.733 cents from the truth at worst (YIN's own figure); the nine
H signals - even harmonics dominant, plain YIN an exact octave high on 25 .. 59 of 59 interior frames - 0.12 cents at worst; the
continuity signals (odd harmonics vanishing periodically) 19 .. 24 interior frames an octave up with jump_cost 0, none with 0.5; the
float32 lag path equal to float64's on all 42 signals, no frame excluded.

The defaults are not knife-edge.  A sweep of the ground-truth checks over octave_cost {0.005, 0.01, 0.014, 0.02, 0.028, 0.04, 0.06}
x jump_cost {0.125, 0.25, 0.35, 0.5, 0.7, 1, 2} (float64) passes everywhere on [0.014, 0.028] x [0.35, 0.7] - a factor sqrt(2) either
way of each default, the corners tested below - and also at octave 0.01 .. 0.014 with jump 0.25 .. 0.7, octave 0.02 with jump
0.25 .. 1 and octave 0.04 with jump 0.5 .. 1.  It is not a rectangle: [0.01, 0.04] x [0.25, 1] fails at its corners (jump 0.25 with
octave >= 0.028 leaves continuity frames an octave up; jump 1 with octave <= 0.014 changes two voicing flags of mixed()).  Outside:
octave 0.005 puts the 493.9 Hz weak-fundamental tone an octave down, octave 0.06 the a = 0.2 signals an octave up, jump 0.125 loses
the continuity case and jump 2 changes voicing flags of mixed()."""
import functools
import os

import numpy as np
import pytest

import f0_ref as R
import f0_track_ref as V

L_TONE, L_H = 8000, 16000
DTYPES = (np.float64, np.float32)
TONES = tuple(("tone", f, h) for f in R.FREQS for h in range(len(R.HARMONICS)))
HS = tuple(("H", f, a) for a in V.H_WEAK for f in V.H_FREQS)
CONT = tuple(("Hv", f, a) for a in (0.3, 0.4) for f in V.H_FREQS)
OTHER = (("noise",), ("zeros",), ("mixed",))
ALL = TONES + HS + CONT + OTHER


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


@functools.lru_cache(maxsize=None)
def signal(key):
    kind = key[0]
    if kind == "tone":
        return R.tone(key[1], L_TONE, R.HARMONICS[key[2]], seed=int(key[1]) + key[2])          # the seeds of test_gpu_f0.py
    if kind == "H":
        return V.H(key[1], key[2], L_H)
    if kind == "Hv":
        return V.H(key[1], key[2], L_H, vanishing=True)
    if kind == "noise":
        return R.white(L_TONE, 0.1)
    if kind == "zeros":
        return np.zeros(L_TONE, np.float32)
    return R.mixed()


@functools.lru_cache(maxsize=None)
def diff(key):
    d = R.difference(signal(key))
    d.setflags(write=False)
    return d


@functools.lru_cache(maxsize=None)
def tracked(key, dtype=np.float64, octave_cost=V.OCTAVE_COST, jump_cost=V.JUMP_COST):
    return V.track(diff(key), octave_cost=octave_cost, jump_cost=jump_cost, dtype=dtype)


def truth(key):
    return key[1]


# ---- hand cases ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("dtype", DTYPES)
def test_one_frame_is_the_arg_min_of_o(dtype):
    rng = np.random.default_rng(1)
    for n in (2, 64, 225, 255):
        o = rng.random((1, n)).astype(dtype)
        o[0, n // 3] = o[0, n // 2] = o.min() / 2              # two states attain the minimum: the smaller wins
        assert V.path(o, V.transitions(2, n + 1, 0.5, dtype)).tolist() == [n // 3]
    f0, cm, lag, d = V.viterbi_track(np.array([0.5], np.float32), dtype=dtype)
    assert f0.shape == (1,) and f0[0] == 0 and lag[0] == 32 and d.shape == (1, 257)


@pytest.mark.parametrize("dtype", DTYPES)
def test_jump_cost_zero_makes_the_frames_independent(dtype):
    rng = np.random.default_rng(2)
    o = rng.random((40, 225)).astype(dtype)
    o[7, 100] = o[7, 30] = 0.0                                 # a tie inside a frame: its first arg-min
    tr = V.transitions(32, 256, 0.0, dtype)
    assert not tr.any()
    assert np.array_equal(V.path(o, tr), np.argmin(o, axis=1)) and V.path(o, tr)[7] == 30
    key = ("Hv", 146.83, 0.3)
    dp = R.cmnd(diff(key), dtype)
    lag = tracked(key, dtype, jump_cost=0.0)[2]
    assert np.array_equal(lag - 32, np.argmin(V.observations(dp, 32, 256), axis=1))


@pytest.mark.parametrize("dtype", DTYPES)
def test_an_all_equal_o_takes_state_zero_throughout(dtype):
    o = np.full((30, 225), 0.25, dtype)
    assert not V.path(o, V.transitions(32, 256, 0.5, dtype)).any()
    assert not V.path(o, V.transitions(32, 256, 0.0, dtype)).any()
    f0, cm, lag = V.track(np.zeros((12, 257)), dtype=dtype)[:3]          # silence: every d' is 1, o = 1 + bias, state 0 is cheapest
    assert (lag == 32).all() and (cm == 1).all() and not f0.any()


def test_a_non_finite_d_counts_as_one_and_the_lag_stays_in_range():
    d = diff(("tone", 146.83, 1)).copy()
    d[10, 90:120] = np.nan
    d[11] = np.inf
    for dtype in DTYPES:
        o = V.observations(R.cmnd(d, dtype), 32, 256)
        assert np.isfinite(o).all()
        f0, cm, lag = V.track(d, dtype=dtype)
        assert ((lag >= 32) & (lag <= 256)).all() and np.isfinite(f0).all()


def test_costs_are_refused_like_the_library_refuses_them():
    for bad in (-0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            V.track(diff(("zeros",)), octave_cost=bad)
        with pytest.raises(ValueError):
            V.track(diff(("zeros",)), jump_cost=bad)


# ---- ground truth ----------------------------------------------------------------------------------------------------------------

def within_a_cent(keys, L, **costs):
    inner = R.interior(L)
    worst = 0.0
    for dtype in DTYPES:
        for key in keys:
            f0, cm, _ = tracked(key, dtype, **costs)
            assert (f0[inner] > 0).all() and (cm[inner] < 0.15).all(), (key, dtype)
            c = float(np.abs(R.cents(f0[inner], truth(key))).max())
            assert c <= 1.0, (key, dtype, c)
            worst = max(worst, c)
    return worst


def test_tones_are_within_a_cent_of_the_truth():
    assert R.interior(L_TONE) == list(range(2, 30))
    print(f"tones: worst {within_a_cent(TONES, L_TONE):.3g} cents")


def test_dominant_even_harmonics_are_within_a_cent_where_yin_is_an_octave_high():
    inner = R.interior(L_H)
    assert len(inner) == 59
    for key in HS:
        y = R.decide(diff(key))[0][inner]
        off = np.abs(R.cents(np.where(y > 0, y, 1e-9), truth(key))) > 50
        print(key, "plain YIN more than 50 cents off on", int(off.sum()), "of 59 interior frames")
        assert off.sum() >= 25                                 # the signals exercise the failure
        assert octave_up(y, truth(key))[off].all()             # ... and every such frame is an octave up
    print(f"H: worst {within_a_cent(HS, L_H):.3g} cents")


def octave_up(f0, f):
    return np.abs(R.cents(np.where(f0 > 0, f0, 1e-9), 2 * f)) <= 50


def test_continuity_the_time_dimension_does_something():
    """the odd harmonics vanish periodically: frame by frame (jump_cost 0) those frames come out an octave up; f stays a true period
    throughout, and with the default jump_cost the path stays on it"""
    inner = R.interior(L_H)
    for dtype in DTYPES:
        for key in CONT:
            alone = tracked(key, dtype, jump_cost=0.0)[0][inner]
            up = int(octave_up(alone, truth(key)).sum())
            print(key, dtype.__name__, "jump_cost 0:", up, "interior frames an octave up")
            assert up >= 15
            f0 = tracked(key, dtype)[0][inner]
            assert not octave_up(f0, truth(key)).any()
    within_a_cent(CONT, L_H)


def test_noise_and_silence_are_unvoiced():
    for dtype in DTYPES:
        for key in (("noise",), ("zeros",)):
            f0, cm, lag = tracked(key, dtype)
            assert not f0.any() and (cm >= 0.15).all() and ((lag >= 32) & (lag <= 256)).all()


def test_mixed_voicing_flags_are_yins():
    for dtype in DTYPES:
        want = R.decide(diff(("mixed",)), dtype=dtype)[0] > 0
        got = tracked(("mixed",), dtype)[0] > 0
        assert want.size == 63 and 0 < want.sum() < 63
        assert np.array_equal(got, want)


def test_float32_path_is_the_float64_path():
    """zero frames excluded, over every signal above and both jump costs of the continuity case"""
    assert len(ALL) == 42
    for key in ALL:
        assert np.array_equal(tracked(key, np.float32)[2], tracked(key, np.float64)[2]), key
    for key in CONT:
        assert np.array_equal(tracked(key, np.float32, jump_cost=0.0)[2], tracked(key, np.float64, jump_cost=0.0)[2]), key


@pytest.mark.parametrize("octave_cost", [0.014, 0.028])
@pytest.mark.parametrize("jump_cost", [0.35, 0.7])
def test_the_defaults_are_not_knife_edge(octave_cost, jump_cost):
    """the ground-truth checks a factor sqrt(2) either way of each default (float64); the whole sweep is in the module's docstring"""
    costs = dict(octave_cost=octave_cost, jump_cost=jump_cost)
    for keys, L in ((TONES, L_TONE), (HS, L_H), (CONT, L_H)):
        inner = R.interior(L)
        for key in keys:
            f0, cm, _ = tracked(key, np.float64, **costs)
            assert (f0[inner] > 0).all() and np.abs(R.cents(f0[inner], truth(key))).max() <= 1.0, key
    for key in (("noise",), ("zeros",)):
        assert not tracked(key, np.float64, **costs)[0].any()
    assert np.array_equal(tracked(("mixed",), np.float64, **costs)[0] > 0, R.decide(diff(("mixed",)))[0] > 0)


# ---- exports and query ---------------------------------------------------------------------------------------------------------

def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_f0_track_query", "mt2_f0_track"):
        assert hasattr(lib, name) and name in header
    assert hasattr(rt.MelFrontEnd, "f0_track") and callable(rt.f0_track_query)
    unit = open(os.path.join(root, "megatts2_amd", "csrc", "f0.hip")).read()
    assert "f0_viterbi_kernel" in unit and "octave_cost" in header and "jump_cost" in header


def r256(x):
    return (x + 255) // 256 * 256


@pytest.mark.parametrize("hop", [256, 80])
@pytest.mark.parametrize("L, B", [(1, 1), (255, 3), (256, 4), (8000, 5), (480000, 8), (2 ** 31 - 1, 65535)])
def test_query_matches_the_rule_and_the_byte_formula(rt, L, B, hop):
    frames, lo, hi, n, ws = rt.f0_track_query(L, B, hop=hop)
    assert frames == 1 + L // hop and (lo, hi) == R.lags() and n == 225 == V.table(lo, hi).size
    assert ws == r256(4 * ((B + 3) // 4 * 4 + 256)) + r256(4 * B * frames * 257) + r256(256 * B * frames)
    assert rt.f0_track_query(L, B, hop=hop)[:3] == rt.f0_query(L, hop=hop)[:3]
    for fmin, fmax, states in ((62.5, 8000.0, 255), (5333.0, 8000.0, 2), (240.6, 4000.0, 63), (237.0, 4000.0, 64),
                               (233.6, 4000.0, 65)):
        got = rt.f0_track_query(L, B, hop=hop, fmin=fmin, fmax=fmax)
        assert got[3] == states == got[2] - got[1] + 1 and got[1:3] == R.lags(R.SR, fmin, fmax)


@pytest.mark.parametrize("kw", [
    dict(hop=0), dict(hop=1025), dict(hop=-256),
    dict(fmin=0.0), dict(fmin=-62.5), dict(fmin=float("nan")), dict(fmin=float("inf")),
    dict(fmax=0.0), dict(fmax=-500.0), dict(fmax=float("nan")), dict(fmax=float("inf")),
    dict(fmin=62.0), dict(fmin=30.0), dict(fmax=16000.0), dict(fmin=500.0, fmax=500.0), dict(fmin=500.0, fmax=62.5),
    dict(L=0), dict(L=-1), dict(L=2 ** 31),
    dict(B=0), dict(B=-1), dict(B=65536),
    dict(sample_rate=0),
    dict(octave_cost=-0.01), dict(octave_cost=float("nan")), dict(octave_cost=float("inf")),
    dict(jump_cost=-0.5), dict(jump_cost=float("nan")), dict(jump_cost=float("inf")), dict(jump_cost=float("-inf")),
])
def test_query_rejects(rt, kw):
    assert rt.f0_track_query(8000, 2, octave_cost=0.0, jump_cost=0.0)[3] == 225           # zero costs are legal
    kw = dict(kw)
    L = kw.pop("L", 8000)
    with pytest.raises(rt.NativeError):
        rt.f0_track_query(L, **kw)
    assert rt.load_library().mt2_last_error()
