"""Host side of the per-phone prosody layer (no GPU): the numpy restatement of the three rules of csrc/prosody.hip
(tests/prosody_ref.py) on hand cases and against ground truth, and the library's refusals, which are decided on the host.

Ground truth for phone-level pitch: tone A (110 Hz), tone B (220 Hz), silence and tone C (329.63 Hz), 24 hops each, harmonics
(1, .5, .33, .25), tracked by the restatement of YIN (f0_ref.yin); every segment border sits in its own 4-frame phone.  Observed:
the interior phones' mean_hz 0.018 .. 0.104 cents from the truth, min_hz / max_hz within 0.144 cents (bar 1 cent); 4-frame border
phones suffice, every window of an interior frame lies wholly inside its segment.

Ground truth for the distance: contour b is contour a with every voiced frame repeated twice, transposed by 3 semitones, with
other unvoiced gaps; a steps between four levels 7.02 semitones apart (prosody_ref.warped_pair says why levels).  The bar 4 * 2^-24 * max|st| stands for the two f32 roundings of the contour values (half an ulp each, an ulp
at most 2^-23 max|st|); the f32 rounding of the transposed F0 itself adds up to 12 / ln 2 * 2^-24 = 17.3 * 2^-24 semitones, which
the contour's span (+-11.1 semitones centred, so a bar of 44 * 2^-24 against 16 + 17.3 at worst) leaves room for.  Observed in
float64 DTW on the f32 contours: centred 3.3e-07 semitones (bar 2.65e-06), uncentred |rms - 3| 0 (bar 2.47e-05: in one binade x and
x + 3 round alike), reversed 3.9 semitones."""
import math
import os

import numpy as np
import pytest

import f0_ref as F
import prosody_ref as P


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


# ---- energy ------------------------------------------------------------------------------------------------------------------------

def test_constant_signal_has_energy_c_squared():
    c = np.float32(0.375)                                     # c^2 and every partial sum are exact in f32
    x = np.full(4000, c, np.float32)
    e32, e64 = P.energy32(x), P.energy64(x)
    inner = F.interior(4000)
    assert inner and (e32[inner] == c * c).all() and (e64[inner] == float(c) ** 2).all()
    assert e32[0] == c * c / 2 and e64[0] == float(c) ** 2 / 2      # frame 0 of a long signal: the left half is zeros
    assert e32.dtype == np.float32 and e32.shape == (1 + 4000 // 256,)


@pytest.mark.parametrize("hop", [256, 80])
def test_sine_is_at_half_its_squared_amplitude(hop):
    A = 0.7
    x = (A * np.sin(2 * np.pi * np.arange(6000) / 64 + 0.4)).astype(np.float32)
    e32, e64 = P.energy32(x, hop), P.energy64(x, hop)
    inner = F.interior(6000, hop)
    rel = np.abs(e32[inner].astype(np.float64) - e64[inner]) / e64[inner]
    print(f"hop {hop}: f32 chain against float64 {rel.max():.3g} (bar {P.EPS_E:.3g}); float64 against A^2 / 2 "
          f"{np.abs(e64[inner] / (A * A / 2) - 1).max():.3g}")
    assert rel.max() <= P.EPS_E
    assert np.abs(e32[inner].astype(np.float64) / (A * A / 2) - 1).max() <= P.EPS_E + 2.0 ** -22      # + the f32 samples' own rounding


def test_one_sample_is_one_frame():
    e = P.energy32(np.array([0.5], np.float32))
    assert e.shape == (1,) and e[0] == np.float32(0.25 / 1024)
    assert P.energy64(np.array([0.5], np.float32))[0] == 0.25 / 1024


def test_fma32_is_correctly_rounded():
    """against exact rational arithmetic, on operands chosen to sit near rounding ties"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    x = rng.standard_normal(4000).astype(np.float32)
    acc = (rng.standard_normal(4000) * 2.0 ** rng.integers(-30, 30, 4000)).astype(np.float32)
    x[:50], acc[:50] = np.float32(1 + 2.0 ** -12), np.float32(2.0 ** 24) * np.arange(1, 51, dtype=np.float32)
    got = P.fma32(x, acc)
    for i in range(x.size):
        exact = Fraction(float(x[i])) ** 2 + Fraction(float(acc[i]))
        lo = np.float32(float(exact))                          # float(Fraction) is correctly rounded to f64; bracket in f32
        cands = {float(lo), float(np.nextafter(lo, np.float32(np.inf))), float(np.nextafter(lo, np.float32(-np.inf)))}
        best = min(cands, key=lambda v: (abs(Fraction(v) - exact), int(np.float32(v).view(np.uint32)) & 1))
        assert float(got[i]) == best, i


# ---- phone prosody -----------------------------------------------------------------------------------------------------------------

def test_durations_are_clipped_to_the_frames():
    f0 = np.array([100, 0, 200, 400, 0, 0, 110, 220], np.float32)
    en = np.arange(8, dtype=np.float32)
    out, total = P.phone_prosody(f0, [3, 0, -2, 4, 5, 2], en)       # sum 14 > T = 8
    assert total == 14
    assert out[:, 0].tolist() == [0, 3, 3, 3, 7, 8] and out[:, 1].tolist() == [3, 0, 0, 4, 1, 0]
    assert out[:, 2].tolist() == [2, 0, 0, 2, 1, 0]
    assert out[0, 3] == 150 and out[0, 5] == 100 and out[0, 6] == 200 and out[0, 7] == 1.0
    assert out[0, 4] == pytest.approx(6 * (math.log2(100 / 55) + math.log2(200 / 55)), rel=1e-15)
    assert not out[1, 1:].any() and not out[2, 1:].any() and not out[5, 1:].any()      # a zero, a negative, one beyond T
    assert out[3, 3] == 255 and out[3, 7] == 4.5 and out[4, 3] == 220 and out[4, 7] == 7
    short, total = P.phone_prosody(f0, [2, 3])                # sum 5 < T: the last frames belong to no phone
    assert total == 5 and short[:, 1].tolist() == [2, 3] and not short[:, 7].any()
    cut, _ = P.phone_prosody(f0, [3, 4, 5], T=5)              # frame_lens below the track's width
    assert cut[:, 1].tolist() == [3, 2, 0] and cut[:, 0].tolist() == [0, 3, 5]
    nan = f0.copy()
    nan[2] = np.nan                                           # a NaN is not voiced
    assert P.phone_prosody(nan, [3])[0][0, 2] == 1


def test_an_unvoiced_track_gives_zero_fields_and_an_empty_contour():
    out, _ = P.phone_prosody(np.zeros(10, np.float32), [4, 6], np.ones(10, np.float32))
    assert not out[:, 2:7].any() and out[:, 7].tolist() == [1, 1] and out[:, 1].tolist() == [4, 6]
    for center in (True, False):
        s, index = P.contour(np.zeros(10, np.float32), center=center)
        assert s.size == 0 and index.size == 0


def test_the_compaction_is_stable():
    f0 = np.array([0, 110, 0, 0, 220, 55, np.nan, 440, 0], np.float32)
    s, index = P.contour(f0, center=False)
    assert index.tolist() == [1, 4, 5, 7]
    assert np.array_equal(s, (12 * np.log2(np.array([110, 220, 55, 440.0]))).astype(np.float32))
    c, _ = P.contour(f0, center=True)
    assert np.allclose(c, [-6, 6, -18, 18], atol=1e-6) and P.contour(f0, T=5)[1].tolist() == [1, 4]


def test_duration_moments_against_numpy_formulas():
    d = np.array([3, 0, 7, 12, 0, 5, 5, 1, 30], np.int32)
    m = P.duration_moments(d)
    v = d[d > 0].astype(np.float64)
    assert m[0] == 7 and m[1] == 7 / 9 and m[2] == v.mean() and m[3] == pytest.approx(v.std(), rel=1e-15)
    assert np.allclose(m, F.moments(d.astype(np.float32)), rtol=1e-13, atol=0)      # what duration_stats composes on the device
    assert not P.duration_moments([0, 0]).any()


# ---- ground truth: phone-level pitch ----------------------------------------------------------------------------------------------

def test_interior_phones_are_within_a_cent_of_the_known_pitch():
    x = P.truth_signal()
    f0 = F.yin(x)[0].astype(np.float32)
    assert f0.size == 97
    dur, inner = P.truth_alignment(f0.size)
    assert dur.tolist() == [2, 20, 4, 20, 4, 20, 4, 20, 3] and inner == [1, 3, 5, 7]
    out, total = P.phone_prosody(f0, dur, P.energy64(x).astype(np.float32))
    assert total == 97
    for p, f in zip(inner, P.TRUTH):
        if f == 0:
            assert out[p, 2] == 0 and not out[p, 3:7].any() and out[p, 7] == 0
            continue
        c = [abs(float(F.cents(out[p, k], f))) for k in (3, 5, 6)]
        print(f"{f} Hz: mean {c[0]:.3g}, min {c[1]:.3g}, max {c[2]:.3g} cents; mean energy {out[p, 7]:.4g}")
        assert out[p, 1] == out[p, 2] == 20 and max(c) <= 1.0
        assert out[p, 4] == pytest.approx(12 * math.log2(f / 55), abs=0.01) and out[p, 7] > 0.01


# ---- ground truth: the distance -----------------------------------------------------------------------------------------------------

def test_a_warped_transposed_contour_is_at_distance_zero_centred_and_three_semitones_not():
    a, b = P.warped_pair()
    assert (a > 0).sum() == 53 and (b > 0).sum() == 106 and b.size == 120
    ca, cb = P.contour(a)[0], P.contour(b)[0]
    top = float(max(np.abs(ca).max(), np.abs(cb).max()))
    rms, steps = P.dtw_rms(ca, cb)
    print(f"centred: {rms:.3g} semitones over {steps} steps (bar {4 * 2.0 ** -24 * top:.3g}, max |st| {top:.3g})")
    assert top >= 9 and steps >= 106 and rms <= 4 * 2.0 ** -24 * top
    ua, ub = P.contour(a, center=False)[0], P.contour(b, center=False)[0]
    utop = float(max(np.abs(ua).max(), np.abs(ub).max()))
    urms, usteps = P.dtw_rms(ua, ub)
    print(f"uncentred: |rms - 3| {abs(urms - 3):.3g} over {usteps} steps (bar {4 * 2.0 ** -24 * utop:.3g})")
    assert usteps == 106 and abs(urms - 3.0) <= 4 * 2.0 ** -24 * utop
    back, _ = P.dtw_rms(ca[::-1].copy(), cb)
    print(f"reversed: {back:.3g} semitones")
    assert back > rms


# ---- refusals and exports ----------------------------------------------------------------------------------------------------------

FAKE = 0x10000          # a well-aligned address that is never dereferenced: every call below is refused on the host


def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_frame_energy", "mt2_phone_prosody", "mt2_pitch_contour"):
        assert hasattr(lib, name) and name in header
    assert "MT2_PROSODY_FIELDS 8" in header and rt.PROSODY_FIELDS == 8 == len(P.FIELDS)
    for name in ("energy", "phone_prosody", "pitch_contour"):
        assert hasattr(rt.MelFrontEnd, name)
    from megatts2_amd import megatts2 as M
    for name in ("extract_energy", "phone_prosody", "duration_stats", "pitch_distance"):
        assert callable(getattr(M, name))
    assert callable(M.Megatts.output_prosody) and M.PHONE_PROSODY == P.FIELDS
    from megatts2_amd import build
    assert "prosody.hip" in build.UNITS


def test_frame_energy_refuses_on_the_host(rt):
    lib = rt.load_library()

    def why(lens, L_max=3000, hop=256, T_max=12, B=None, wav=FAKE, energy=FAKE + (1 << 20)):
        lens = np.asarray(lens, np.int32)
        keep = lens.copy()
        rc = lib.mt2_frame_energy(None, None, wav, rt._iptr(lens), L_max, lens.size if B is None else B, hop, energy, T_max)
        assert rc != 0 and np.array_equal(lens, keep)
        return lib.mt2_last_error().decode()

    assert "null model handle" in why([3000, 2000])
    assert "B outside" in why([3000], B=0) and "B outside" in why([3000], B=65536)
    assert "length outside" in why([3000, 0]) and "length outside" in why([3001, 5]) and "length outside" in why([-1])
    for hop in (0, -1, 1025):
        assert "hop outside" in why([3000], hop=hop)
    assert "T_max smaller" in why([3000], T_max=11) and "T_max smaller" in why([3000], hop=80, T_max=37)
    assert "overlaps" in why([3000, 3000], energy=FAKE + 4 * 2990) and "overlaps" in why([3000, 3000], energy=FAKE + 4 * 5999)
    assert "bad buffers" in why([3000], wav=None) and "bad buffers" in why([3000], energy=None)
    assert "misaligned" in why([3000], energy=FAKE + (1 << 20) + 2)


def test_phone_prosody_refuses_on_the_host(rt):
    lib = rt.load_library()
    f0, en, dur, out, tot = FAKE, FAKE + (1 << 20), FAKE + (2 << 20), FAKE + (3 << 20), FAKE + (5 << 20)

    def why(pl, fl, Np_max=40, T_max=100, B=None, **kw):
        pl, fl = np.asarray(pl, np.int32), np.asarray(fl, np.int32)
        a = dict(f0=f0, en=en, dur=dur, out=out, tot=tot)
        a.update(kw)
        rc = lib.mt2_phone_prosody(None, None, a["f0"], a["en"], a["dur"], rt._iptr(pl), Np_max, rt._iptr(fl), T_max,
                                   pl.size if B is None else B, a["out"], a["tot"])
        assert rc != 0
        return lib.mt2_last_error().decode()

    assert "null model handle" in why([40, 7], [100, 1])
    assert "null model handle" in why([40], [100], en=None, tot=None)
    assert "B outside" in why([40], [100], B=0) and "B outside" in why([40], [100], B=65536)
    assert "phone count" in why([41], [100]) and "phone count" in why([40, 0], [100, 100])
    assert "frame count" in why([40], [101]) and "frame count" in why([40, 40], [100, 0])
    assert "bad buffers" in why([40], [100], f0=None) and "bad buffers" in why([40], [100], dur=None)
    assert "bad buffers" in why([40], [100], out=None)
    assert "misaligned" in why([40], [100], out=out + 8) and "misaligned" in why([40], [100], tot=tot + 4)
    for kw in (dict(out=f0 + 4 * 48), dict(out=en), dict(out=dur + 4 * 36), dict(tot=f0), dict(tot=en + 8), dict(tot=dur),
               dict(tot=out + 64 * 40 - 8)):
        assert "overlapping" in why([40], [100], **kw), kw


def test_pitch_contour_refuses_on_the_host(rt):
    lib = rt.load_library()
    f0, st, n, index = FAKE, FAKE + (1 << 20), FAKE + (2 << 20), FAKE + (3 << 20)

    def why(fl, T_max=100, B=None, center=1, **kw):
        fl = np.asarray(fl, np.int32)
        a = dict(f0=f0, st=st, n=n, index=index)
        a.update(kw)
        rc = lib.mt2_pitch_contour(None, None, a["f0"], rt._iptr(fl), T_max, fl.size if B is None else B, center, a["st"], a["n"],
                                   a["index"])
        assert rc != 0
        return lib.mt2_last_error().decode()

    assert "null model handle" in why([100, 1]) and "null model handle" in why([100], index=None, center=0)
    assert "B outside" in why([100], B=0) and "B outside" in why([100], B=65536)
    assert "frame count" in why([101]) and "frame count" in why([100, 0])
    assert "center" in why([100], center=2) and "center" in why([100], center=-1)
    assert "bad buffers" in why([100], f0=None) and "bad buffers" in why([100], st=None) and "bad buffers" in why([100], n=None)
    assert "misaligned" in why([100], st=st + 2)
    for kw in (dict(st=f0 + 4 * 99), dict(index=f0), dict(n=f0 + 4 * 50), dict(index=st), dict(n=st), dict(n=index + 4 * 99)):
        assert "overlapping" in why([100], **kw), kw
