"""The stationary-noise suppression rule without a GPU: its float64 restatement (tests/denoise_ref.py) against analytic ground truth at
the 16 kHz configuration, the restatement's pieces against statements that do not call the rule, and the library's host-only entry
point mt2_denoise_query - with the refusals of the three device calls, which are decided on the host before the handle is looked at.

Ground truth (the figures are this file's own prints):
  white noise, sigma 0.05, defaults   mean Nf[f] / (sigma^2 sum w^2) over 0 < f < N/2: 1.009 at 5 s, 1.027 at 2 s -> within 5 % of 1;
                                      output 18.18 dB under the input at 5 s, 18.09 dB at 2 s (floor -20 dB) -> at least 15 dB
  440 Hz tone gated on for alternate half-seconds, 7 dB over that noise
                                      SNR against the clean gated tone 7.00 dB -> 17.69 dB at percentile 20 -> a rise of at least 8 dB;
                                      0.996 dB at percentile 50: the tone sits in its bin half the time, the median is no longer noise
                                      -> no improvement.  This pins the stated limit.
  a steady tone of the same level     amplitude 0.2238 -> 0.0227 (-19.9 dB): removed like hum -> at least 15 dB"""
import ctypes as C
import math
import os
from fractions import Fraction

import numpy as np
import pytest

import denoise_ref as D
import griffinlim_ref as G

SR = 16000


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


@pytest.fixture(scope="module")
def audio():
    from megatts2_amd.config import AudioConfig
    return AudioConfig()


# ---- ground truth ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("seconds", [5, 2])
def test_white_noise_floor_is_the_noise_power_and_the_output_sits_at_the_floor_gain(audio, seconds):
    x = D.white_noise(seconds * SR, seed=0)
    r = D.denoise(x, audio)
    F = audio.n_fft // 2 + 1
    ratio = float((r["Nf"][1:F - 1] / (D.SIGMA ** 2 * D.window_energy(audio))).mean())
    drop = -D.level_db(r["y"], x)
    print(f"white noise {seconds} s: mean Nf / (sigma^2 sum w^2) = {ratio:.4f}, output {drop:.2f} dB under the input")
    if seconds == 5:
        assert abs(ratio - 1.0) < 0.05
    assert drop >= 15.0


def test_gated_tone_is_cleaned_at_20_and_not_at_50(audio):
    L = 5 * SR
    clean = D.tone(L, SR, gated=True)
    x = (clean + D.white_noise(L, seed=0)).astype(np.float32)
    before = D.snr_db(x, clean)
    at20 = D.snr_db(D.denoise(x, audio, D.Config(percentile=20))["y"], clean)
    at50 = D.snr_db(D.denoise(x, audio, D.Config(percentile=50))["y"], clean)
    print(f"gated tone: SNR {before:.2f} dB -> {at20:.2f} dB at percentile 20, {at50:.2f} dB at percentile 50")
    assert abs(before - 7.0) < 0.1
    assert at20 - before >= 8.0
    assert at50 <= before


def test_a_steady_tone_is_removed_like_hum(audio):
    L = 5 * SR
    x = (D.tone(L, SR, gated=False) + D.white_noise(L, seed=0)).astype(np.float32)
    y = D.denoise(x, audio)["y"]
    a0, a1 = D.tone_amplitude(x, SR), D.tone_amplitude(y, SR)
    print(f"steady tone: amplitude {a0:.4f} -> {a1:.4f} ({20 * math.log10(a1 / a0):.1f} dB)")
    assert abs(a0 - D.TONE_AMP) < 0.01 and 20 * math.log10(a1 / a0) <= -15.0


@pytest.mark.parametrize("dt", [np.float64, np.float32])
def test_floor_gain_one_is_the_round_trip(audio, dt):
    x = (D.tone(6000, SR) + D.white_noise(6000, seed=3)).astype(np.float32)
    r = D.denoise(x, audio, D.Config(floor_gain=1.0), dt)
    assert (r["g0"] == 1).all() and (r["g"] == 1).all()
    assert np.array_equal(r["y"], G.istft(G.stft(x, audio, dt), audio, dt))


def test_figures_follow_rule_7(audio):
    x = (D.tone(2 * SR, SR) + D.white_noise(2 * SR, seed=1)).astype(np.float32)
    r = D.denoise(x, audio)
    f = dict(zip(D.FIELDS, r["figures"]))
    T = 1 + len(x) // audio.hop_length
    assert f["frames"] == T and f["rank"] == D.rank(T, 20)
    assert f["noise_db"] == pytest.approx(10 * math.log10(r["Nf"].sum()))
    assert f["snr_db"] == pytest.approx(10 * math.log10((r["P"].sum() / T - r["Nf"].sum()) / r["Nf"].sum()))
    assert f["floored_share"] == pytest.approx((r["g0"] == np.float32(0.1)).mean()) and 0.5 < f["floored_share"] < 1.0
    assert f["reduction_db"] == pytest.approx(10 * math.log10((r["g"] ** 2 * r["P"]).sum() / r["P"].sum())) and f["reduction_db"] < 0


# ---- pinned to restatements that do not call the rule --------------------------------------------------------------------------------

def test_fma_f32_is_one_rounding():
    """against exact rational arithmetic, on operands chosen to land near f32 midpoints and on squares, the rule's use"""
    rng = np.random.default_rng(0)
    a = rng.standard_normal(1500).astype(np.float32)
    b = np.where(np.arange(1500) % 2 == 0, a, rng.standard_normal(1500).astype(np.float32))
    c = (np.abs(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, 1500) * 2.0 ** -24)).astype(np.float32)
    c[::3] = (rng.standard_normal(c[::3].size) ** 2).astype(np.float32) * 1e-3
    got = D.fma_f32(a, b, c)
    for x, y, z, g in zip(a, b, c, got):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        err = abs(exact - Fraction(float(g)))
        assert err <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))
        if err == abs(exact - Fraction(float(lo))) or err == abs(exact - Fraction(float(hi))):       # a tie goes to the even mantissa
            assert int(np.float32(g).view(np.uint32)) & 1 == 0


@pytest.mark.parametrize("percentile", [1, 20, 50, 99])
def test_rank_and_factor(rt, audio, percentile):
    for T in (4, 5, 255, 256, 257, 4100, 16384):
        k = D.rank(T, percentile)
        assert k == math.floor(Fraction((T - 1) * percentile, 100) + Fraction(1, 2)) and 0 <= k < T
        L = (T - 1) * audio.hop_length
        _, lout, rank, c = rt.denoise_query(audio, L_max=L, B=1, denoise=rt.Denoise(percentile=percentile))
        assert (lout, rank) == (L, k)
        assert np.float32(c) == D.factor(percentile)
    # the quantile of an exponential distribution with mean 1 is -ln(1 - p): c times it is the mean
    assert float(D.factor(percentile)) * -math.log1p(-percentile / 100.0) == pytest.approx(1.0, abs=2.0 ** -23)
    e = np.random.default_rng(percentile).exponential(1.0, 200001)
    assert float(D.factor(percentile)) * np.sort(e)[D.rank(e.size, percentile)] == pytest.approx(1.0, rel=0.05)


@pytest.mark.parametrize("T, F, bf, bt", [(4, 65, 1, 1), (4, 65, 8, 8), (9, 5, 8, 0), (40, 65, 0, 8), (3, 2, 1, 1), (20, 30, 3, 2)])
def test_smoothing_counts_the_existing_cells(T, F, bf, bt):
    cfg = D.Config(smooth_bins=bf, smooth_frames=bt)
    assert np.array_equal(D.smooth(np.ones((T, F)), cfg), np.ones((T, F)))
    rng = np.random.default_rng(T * F)
    g0 = rng.random((T, F))
    want = np.zeros((T, F))
    g1 = np.zeros((T, F))
    for t in range(T):
        for f in range(F):
            cells = [g0[t, q] for q in range(f - bf, f + bf + 1) if 0 <= q < F]
            g1[t, f] = sum(cells) / len(cells)
    for t in range(T):
        for f in range(F):
            cells = [g1[q, f] for q in range(t - bt, t + bt + 1) if 0 <= q < T]
            want[t, f] = sum(cells) / len(cells)
    assert np.allclose(D.smooth(g0, cfg), want, rtol=1e-14, atol=0)
    one = np.zeros((T, F))
    one[0, 0] = 1.0      # a corner: min(F, bf + 1) bins and min(T, bt + 1) frames exist
    assert D.smooth(one, cfg)[0, 0] == pytest.approx(1.0 / (min(F, bf + 1) * min(T, bt + 1)))


@pytest.mark.parametrize("L", [1024, 1279, 1280, 4000, 80000])
def test_output_length(rt, audio, L):
    y = D.denoise(D.white_noise(L, seed=L), audio)["y"]
    h = audio.hop_length
    assert len(y) == h * (L // h) == D.out_len(L, audio) and L - len(y) < h
    assert rt.denoise_query(audio, L_max=L, B=3)[1] == len(y)


# ---- the library without a device ------------------------------------------------------------------------------------------------

def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_denoise_query", "mt2_noise_floor", "mt2_spectral_gain", "mt2_denoise"):
        assert hasattr(lib, name) and name in header
    assert "MT2_DENOISE_FIELDS 8" in header and "MT2_DENOISE_MAX_FRAMES 16384" in header
    assert rt.DENOISE_NAMES == D.FIELDS
    d = rt.Denoise()
    assert dataclass_fields(d) == dataclass_fields(D.Config())
    from megatts2_amd import megatts2 as M
    assert hasattr(M, "denoise_audio")
    for cls in (rt.NativeModel, rt.MelFrontEnd):
        assert all(hasattr(cls, n) for n in ("denoise", "noise_floor", "spectral_gain"))


def dataclass_fields(d):
    import dataclasses
    return {f.name: getattr(d, f.name) for f in dataclasses.fields(d)}


def carve(audio, lens):
    """denoise_layout by hand: every piece rounded up to 256 bytes, never none"""
    r = lambda n: max(256, (n + 255) // 256 * 256)
    q = lambda n: (n + 3) // 4 * 4
    N, h = audio.n_fft, audio.hop_length
    F = N // 2 + 1
    Fp, S, B = q(F), q(2 * F), len(lens)
    T = [1 + L // h for L in lens]
    Fr, Rb = sum(T), sum(t - 1 + N // h for t in T)
    tiles = ((max(T) + 15) // 16) * ((F + 63) // 64)
    return (r(4 * (2 * q(Rb) + q(B) + 2 * q(Fr) + q(B) + B)) + r(4 * Rb * h) + r(4 * Fr * S) + r(4 * Fr * Fp) + r(4 * B * Fp) + r(24 * B * tiles)
            + r(4 * Fr * N))


@pytest.mark.parametrize("lens", [(1024,), (480000,), (1024, 99999, 5000), (8000,) * 32, (770, 1279)])
def test_query_is_the_carve(rt, audio, lens):
    assert rt.denoise_query(audio, lens=np.asarray(lens))[0] == carve(audio, lens)


def test_query_refuses(rt, audio):
    def why(L_max=8000, B=1, lens=None, **kw):
        with pytest.raises(rt.NativeError) as e:
            rt.denoise_query(audio, lens=lens, L_max=L_max, B=B, denoise=rt.Denoise(**kw))
        return str(e.value)

    assert rt.denoise_query(audio, L_max=8000, B=1)[1] == 7936
    assert "percentile" in why(percentile=0)
    assert "percentile" in why(percentile=100)
    for bad in (0.0, -1.0, math.nan, math.inf):
        assert "over_subtraction" in why(over_subtraction=bad)
    for bad in (0.0, -0.1, 1.0001, math.nan, math.inf):
        assert "floor_gain" in why(floor_gain=bad)
    assert "smooth_bins" in why(smooth_bins=-1) and "smooth_bins" in why(smooth_bins=9)
    assert "smooth_frames" in why(smooth_frames=-1) and "smooth_frames" in why(smooth_frames=9)
    assert "B outside" in why(B=0) and "B outside" in why(B=65536)
    assert "fewer frames" in why(L_max=767)                                   # T = 3 < n_fft / (2 hop) + 2 = 4
    assert rt.denoise_query(audio, L_max=768, B=1)[1] == 768
    assert "fewer frames" in why(lens=np.asarray([8000, 700]))
    assert "MT2_DENOISE_MAX_FRAMES" in why(L_max=16384 * 256)
    assert rt.denoise_query(audio, L_max=16384 * 256 - 1, B=1)[2] == D.rank(16384, 20)
    assert "outside [1, L_max]" in why(lens=np.asarray([8000, 9000]), L_max=8000)


SENT = -77.25


def test_device_calls_refuse_on_the_host(rt, audio):
    """host arrays stand in for device buffers: a refused call never reads or writes them, and the handle is looked at last"""
    lib = rt.load_library()
    ac = rt._audio_struct(audio)
    F = audio.n_fft // 2 + 1
    Fp, S = (F + 3) & ~3, (2 * F + 3) & ~3

    def run(name, lens, T_or_L, B=None, cfg=None, overlap=False, null=None, Lout=None, floor_in=False):
        lens = np.asarray(lens, np.int32)
        n = lens.size if B is None else B
        dc = (cfg or rt.Denoise()).c_struct()
        rows = max(min(n, 2), 1)
        bufs = {"floor": np.full((rows, Fp), SENT, np.float32), "fig": np.full((rows, 8), SENT, np.float64)}
        p = lambda k: None if null == k else rt._iptr(bufs[k])
        if name == "denoise":
            bufs["wav"] = np.full((rows, max(T_or_L, 1)), SENT, np.float32)
            bufs["out"] = np.full((rows, max(T_or_L, 1)), SENT, np.float32)
            rc = lib.mt2_denoise(None, None, C.byref(ac), C.byref(dc), p("wav"), rt._iptr(lens), T_or_L, n, p("floor") if floor_in else None,
                                 None, p("fig"), p("wav") if overlap else p("out"), T_or_L if Lout is None else Lout)
        else:
            bufs["spec"] = np.full((rows, 4, S), SENT, np.float32)
            bufs["gain"] = np.full((rows, 4, Fp), SENT, np.float32)
            if name == "noise_floor":
                rc = lib.mt2_noise_floor(None, None, C.byref(ac), C.byref(dc), p("spec"), rt._iptr(lens), T_or_L, n,
                                         p("spec") if overlap else p("floor"))
            else:
                rc = lib.mt2_spectral_gain(None, None, C.byref(ac), C.byref(dc), p("spec"), rt._iptr(lens), T_or_L, n, p("floor"),
                                           p("spec") if overlap else p("gain"), None)
        assert rc != 0 and all((v == SENT).all() for v in bufs.values())
        return lib.mt2_last_error().decode()

    for name, lens, size in (("denoise", [8000, 4000], 8000), ("noise_floor", [4, 2], 4), ("spectral_gain", [4, 2], 4)):
        assert "null model handle" in run(name, lens, size)
        assert "percentile" in run(name, lens, size, cfg=rt.Denoise(percentile=0))
        assert "over_subtraction" in run(name, lens, size, cfg=rt.Denoise(over_subtraction=math.nan))
        assert "floor_gain" in run(name, lens, size, cfg=rt.Denoise(floor_gain=0.0))
        assert "smooth_bins" in run(name, lens, size, cfg=rt.Denoise(smooth_bins=9))
        assert "smooth_frames" in run(name, lens, size, cfg=rt.Denoise(smooth_frames=-1))
        assert "B outside" in run(name, lens, size, B=0)
        assert "overlapping" in run(name, lens, size, overlap=True)
    assert "fewer frames" in run("denoise", [8000, 767], 8000)
    assert "outside [1, L_max]" in run("denoise", [8000, 8001], 8000)
    assert "MT2_DENOISE_MAX_FRAMES" in run("denoise", [16384 * 256], 16384 * 256, Lout=1)
    assert "Lout_max" in run("denoise", [8000, 4000], 8000, Lout=7935)
    assert "bad buffers" in run("denoise", [8000], 8000, null="wav")
    assert "bad buffers" in run("denoise", [8000], 8000, null="out")
    assert "overlapping" not in run("denoise", [8000], 8000, floor_in=True)
    for name in ("noise_floor", "spectral_gain"):
        assert "frame count" in run(name, [4, 5], 4)
        assert "frame count" in run(name, [0, 4], 4)
        assert "T_max" in run(name, [4], 0)
        assert "T_max" in run(name, [4], 16385)
        assert "bad buffers" in run(name, [4], 4, null="spec")
    assert "bad floor" in run("noise_floor", [4], 4, null="floor")
    assert "null floor" in run("spectral_gain", [4], 4, null="floor")
    assert "neither output" in run("spectral_gain", [4], 4, null="gain")
