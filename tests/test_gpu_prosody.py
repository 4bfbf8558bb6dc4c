"""The per-phone prosody layer on the GPU (csrc/prosody.hip: mt2_frame_energy, mt2_phone_prosody, mt2_pitch_contour) against the
restatement of its rules (tests/prosody_ref.py) and against ground truth.

Bars.  Energy: BIT-EQUAL to the float32 restatement (the lane / butterfly order spelled out), and within (1024 + 7) * 2^-24 * e of
the float64 mean square.  Phone prosody: the integer fields, min and max exactly the float64 restatement's, the means within 1e-12
relative (the bar test_gpu_f0.py holds the double moments to), dur_sum exact.  Contour: n_voiced, index and the zero tail exact, st
within 2^-23 * max(1, |ref|) of the float64 restatement (the device's double log2 may differ from numpy's in the last place before
the one rounding to f32).  A ragged batch: bit-identical to its rows alone, whatever the slot, the max dimensions or repetition.

In every case the input padding beyond the lengths is NaN (f0, energy, wav) or garbage (dur), the outputs are wider than needed,
pre-filled with a sentinel and followed by guard words."""
import dataclasses
import functools

import numpy as np
import pytest

import f0_ref as F
import prosody_ref as P
from conftest import synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT, ISENT, GUARD = -77.25, -7777, 11
LENGTHS = (1, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 1500, 4000)
HOPS = (256, 80)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


def rt():
    from megatts2_amd import runtime
    return runtime


@functools.lru_cache(maxsize=None)
def signals():
    rows = [F.tone(220.5, L, F.HARMONICS[1], seed=L) for L in LENGTHS]
    rows += [F.white(4000, 0.1, seed=5), np.zeros(1500, np.float32), F.tone(110.0, 1025, F.HARMONICS[2], seed=9)]
    return tuple(rows)


@functools.lru_cache(maxsize=None)
def energy_refs(hop):
    """(float32 restatement, float64 mean square) of every signal, computed once"""
    return tuple((P.energy32(x, hop), P.energy64(x, hop)) for x in signals())


# ---- 1. energy ---------------------------------------------------------------------------------------------------------------------

def energy_run(rows, hop=256, extra_L=7, extra_T=3, shift=0, expect_error=False, lens=None, T_w=None):
    """mt2_frame_energy on `rows` as one batch -> (energy [B, T_w], T [B]); `shift` floats in front of the wav buffer move every
    row's address"""
    R = rt()
    fe = frontend()
    B = len(rows)
    true_lens = np.asarray([r.size for r in rows], np.int32)
    L_max = int(true_lens.max()) + extra_L
    host = np.full(shift + B * L_max, np.nan, np.float32)
    for b, r in enumerate(rows):
        host[shift + b * L_max:shift + b * L_max + r.size] = r
    base = dev(host)
    wav = base[shift:]
    lens = true_lens if lens is None else np.asarray(lens, np.int32)
    if T_w is None:
        T_w = 1 + int(true_lens.max()) // max(hop, 1) + extra_T
    n = B * T_w
    out = torch.full((n + GUARD,), SENT, device="cuda", dtype=torch.float32)
    rc = fe.lib.mt2_frame_energy(fe.h, R._stream(), R._ptr(wav), R._iptr(lens), L_max, B, hop, R._ptr(out), T_w)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    if expect_error:
        assert rc != 0 and fe.lib.mt2_last_error() and (got == np.float32(SENT)).all()
        return None
    assert rc == 0, fe.lib.mt2_last_error().decode()
    assert (got[n:] == np.float32(SENT)).all()
    e, T = got[:n].reshape(B, T_w), 1 + lens // hop
    for b in range(B):
        assert not e[b, int(T[b]):].any()                     # frames behind the utterance's own are written 0
    return e, T


@pytest.mark.parametrize("shift", [0, 1])
@pytest.mark.parametrize("hop", HOPS)
def test_energy_is_the_float32_restatement_bit_for_bit(hop, shift):
    """Observed on an MI355X: worst error against float64 0.0018 of the bound."""
    rows = signals()
    e, T = energy_run(rows, hop, shift=shift, extra_L=7 if shift == 0 else 6)      # L_max odd / even: row addresses of every class
    worst = 0.0
    for b, (r32, r64) in enumerate(energy_refs(hop)):
        t = int(T[b])
        assert r32.shape == (t,)
        assert np.array_equal(e[b, :t].view(np.uint32), r32.view(np.uint32)), (b, rows[b].size)
        err = np.abs(e[b, :t].astype(np.float64) - r64)
        assert (err <= P.EPS_E * r64).all()
        worst = max(worst, float(np.max(err / np.maximum(P.EPS_E * r64, 1e-300))))
    print(f"hop {hop} shift {shift}: worst energy error / bound {worst:.3g}")


@pytest.mark.parametrize("hop", HOPS)
def test_a_nan_sample_changes_only_the_energy_frames_that_hold_it(hop):
    x = F.tone(146.83, 4000, F.HARMONICS[1], seed=2)
    y = x.copy()
    y[2000] = np.nan
    e, T = energy_run([x, y], hop)
    t = int(T[0])
    clean = np.array([not (hop * k - 512 <= 2000 < hop * k + 512) for k in range(t)])
    assert 0 < clean.sum() < t
    assert np.array_equal(e[0, :t][clean].view(np.uint32), e[1, :t][clean].view(np.uint32))
    assert np.isnan(e[1, :t][~clean]).all() and np.isfinite(e[0, :t]).all()


# ---- 2. phone prosody -----------------------------------------------------------------------------------------------------------

def prosody_run(f0_rows, dur_rows, en_rows=None, frame_lens=None, extra_T=5, extra_Np=3, expect_error=False, phone_lens=None,
                want_sum=True):
    """mt2_phone_prosody on one batch -> (out [B, Np_w, 8] float64, dur_sum [B] or None)"""
    R = rt()
    fe = frontend()
    B = len(f0_rows)
    T_w = max(r.size for r in f0_rows) + extra_T
    Np_w = max(len(d) for d in dur_rows) + extra_Np
    f0 = np.full((B, T_w), np.nan, np.float32)
    en = np.full((B, T_w), np.nan, np.float32)
    dur = np.full((B, Np_w), 1 << 20, np.int32)               # garbage behind phone_lens: a read would move every later start
    dur[:, 1::2] = -5
    for b in range(B):
        f0[b, :f0_rows[b].size] = f0_rows[b]
        dur[b, :len(dur_rows[b])] = dur_rows[b]
        if en_rows is not None:
            en[b, :en_rows[b].size] = en_rows[b]
    fl = np.asarray([r.size for r in f0_rows] if frame_lens is None else frame_lens, np.int32)
    pl = np.asarray([len(d) for d in dur_rows] if phone_lens is None else phone_lens, np.int32)
    n = B * Np_w * 8
    out = torch.full((n + GUARD,), SENT, device="cuda", dtype=torch.float64)
    tot = torch.full((B + GUARD,), ISENT, device="cuda", dtype=torch.int64) if want_sum else None
    d_f0, d_en, d_dur = dev(f0), dev(en) if en_rows is not None else None, dev(dur)
    rc = fe.lib.mt2_phone_prosody(fe.h, R._stream(), R._ptr(d_f0), R._ptr(d_en), R._ptr(d_dur), R._iptr(pl), Np_w, R._iptr(fl), T_w, B,
                                  R._ptr(out), R._ptr(tot))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    s = tot.cpu().numpy() if want_sum else None
    if expect_error:
        assert rc != 0 and (got == SENT).all() and (s is None or (s == ISENT).all())
        return None
    assert rc == 0, fe.lib.mt2_last_error().decode()
    assert (got[n:] == SENT).all() and (s is None or (s[B:] == ISENT).all())
    o = got[:n].reshape(B, Np_w, 8)
    for b in range(B):
        assert not o[b, int(pl[b]):].any()                    # rows at or beyond phone_lens are zeros
    return o, (s[:B] if want_sum else None)


NPS = (1, 2, 255, 256, 257, 600)


@functools.lru_cache(maxsize=None)
def prosody_case():
    """six utterances, one per phone count: zero durations, one phone of 300 frames, a negative entry, sums below and above T_b"""
    rng = np.random.default_rng(21)
    f0s, ens, durs = [], [], []
    for k, Np in enumerate(NPS):
        d = rng.integers(0, 5, Np).astype(np.int32)
        d[rng.random(Np) < 0.2] = 0
        if Np >= 255:
            d[Np // 2] = 300
            d[7] = -3
        if Np == 1:
            d[0] = 9
        total = int(np.maximum(d, 0).sum())
        T = max(1, total + (-40 if k % 2 else 25) if Np >= 255 else total + (3 if k % 2 else -2))
        f = np.where(rng.random(T) < 0.7, rng.uniform(70, 450, T), 0.0).astype(np.float32)
        f[rng.integers(0, T)] = np.nan                        # not voiced
        f0s.append(f)
        ens.append(rng.uniform(0, 0.3, T).astype(np.float32))
        durs.append(d)
    refs = [(P.phone_prosody(f0s[b], durs[b], ens[b]), P.phone_prosody(f0s[b], durs[b], None)) for b in range(len(NPS))]
    return f0s, ens, durs, refs


def assert_prosody(got, want, where):
    for k in (0, 1, 2, 5, 6):
        assert np.array_equal(got[:, k], want[:, k]), (where, k)
    for k in (3, 4, 7):
        err = np.abs(got[:, k] - want[:, k])
        assert (err <= 1e-12 * np.abs(want[:, k])).all(), (where, k, float(err.max()))


@pytest.mark.parametrize("with_energy", [True, False])
def test_phone_prosody_equals_the_float64_restatement(with_energy):
    f0s, ens, durs, refs = prosody_case()
    o, s = prosody_run(f0s, durs, ens if with_energy else None)
    sums = []
    for b, Np in enumerate(NPS):
        want, total = refs[b][0 if with_energy else 1]
        assert s[b] == total
        sums.append((total, f0s[b].size))
        assert_prosody(o[b, :Np], want, Np)
        assert with_energy or not o[b, :, 7].any()
        assert o[b, :Np, 1].sum() == min(total, f0s[b].size)
    assert any(t < T for t, T in sums) and any(t > T for t, T in sums)
    assert o[3, :, 1].max() == 300 and (o[..., 2] > 0).any()
    bare, none = prosody_run(f0s, durs, ens if with_energy else None, want_sum=False)      # without dur_sum: the same bits
    assert none is None and np.array_equal(bare, o)


def test_frame_lens_below_the_track_clip_the_phones():
    f0s, ens, durs, _ = prosody_case()
    fl = [max(1, f.size // 2) for f in f0s]
    o, s = prosody_run(f0s, durs, ens, frame_lens=fl)
    for b, Np in enumerate(NPS):
        want, total = P.phone_prosody(f0s[b], durs[b], ens[b], T=fl[b])
        assert s[b] == total
        assert_prosody(o[b, :Np], want, Np)


def test_ground_truth_end_to_end_on_the_device():
    """f0 -> energy -> phone_prosody on tones of known pitch.  Observed on an MI355X: interior phones 0.018 .. 0.104 cents from the
    truth in the mean, min / max within 0.144."""
    fe = frontend()
    x = P.truth_signal()
    wav = dev(x[None])
    f0, en = fe.f0(wav), fe.energy(wav)
    assert f0.shape == en.shape == (1, 97)
    dur, inner = P.truth_alignment(97)
    out, total = fe.phone_prosody(f0, dur[None], en, return_sum=True)
    assert int(total[0]) == 97
    out = out.cpu().numpy()[0]
    assert_prosody(out, P.phone_prosody(f0.cpu().numpy()[0], dur, en.cpu().numpy()[0])[0], "truth")
    for p, f in zip(inner, P.TRUTH):
        if f == 0:
            assert out[p, 2] == 0 and not out[p, 3:].any()
            continue
        c = [abs(float(F.cents(out[p, k], f))) for k in (3, 5, 6)]
        print(f"{f} Hz: mean {c[0]:.3g}, min {c[1]:.3g}, max {c[2]:.3g} cents")
        assert out[p, 1] == out[p, 2] == 20 and max(c) <= 1.0 and out[p, 7] > 0.01


# ---- 3. contour ------------------------------------------------------------------------------------------------------------------

TS = (1, 63, 64, 65, 255, 256, 257, 1000)


def contour_run(rows, center=True, extra_T=4, frame_lens=None, want_index=True, expect_error=False):
    """mt2_pitch_contour on one batch -> (st [B, T_w], n [B], index [B, T_w] or None)"""
    R = rt()
    fe = frontend()
    B = len(rows)
    T_w = max(r.size for r in rows) + extra_T
    f0 = np.full((B, T_w), np.nan, np.float32)
    for b, r in enumerate(rows):
        f0[b, :r.size] = r
    f0[:, -1] = 300.0                                         # a voiced frame behind every utterance: never read
    fl = np.asarray([r.size for r in rows] if frame_lens is None else frame_lens, np.int32)
    m = B * T_w
    st = torch.full((m + GUARD,), SENT, device="cuda", dtype=torch.float32)
    n = torch.full((B + GUARD,), ISENT, device="cuda", dtype=torch.int32)
    index = torch.full((m + GUARD,), ISENT, device="cuda", dtype=torch.int32) if want_index else None
    d_f0 = dev(f0)
    rc = fe.lib.mt2_pitch_contour(fe.h, R._stream(), R._ptr(d_f0), R._iptr(fl), T_w, B, int(center), R._ptr(st), R._ptr(n), R._ptr(index))
    torch.cuda.synchronize()
    g_st, g_n = st.cpu().numpy(), n.cpu().numpy()
    g_ix = index.cpu().numpy() if want_index else None
    if expect_error:
        assert rc != 0 and (g_st == np.float32(SENT)).all() and (g_n == ISENT).all() and (g_ix is None or (g_ix == ISENT).all())
        return None
    assert rc == 0, fe.lib.mt2_last_error().decode()
    assert (g_st[m:] == np.float32(SENT)).all() and (g_n[B:] == ISENT).all() and (g_ix is None or (g_ix[m:] == ISENT).all())
    return g_st[:m].reshape(B, T_w), g_n[:B], (g_ix[:m].reshape(B, T_w) if want_index else None)


def contour_rows(pattern):
    rng = np.random.default_rng(31)
    rows = []
    for T in TS:
        f = rng.uniform(70, 450, T).astype(np.float32)
        if pattern == "none":
            f[:] = 0
        elif pattern == "alternating":
            f[::2] = 0
        elif pattern == "one":
            keep = f[T // 2]
            f[:] = 0
            f[T // 2] = keep
        elif pattern == "mixed":
            f[rng.random(T) < 0.4] = 0
            f[rng.integers(0, T)] = np.nan
        rows.append(f)
    return rows


@pytest.mark.parametrize("center", [True, False])
@pytest.mark.parametrize("pattern", ["all", "none", "alternating", "one", "mixed"])
def test_contour_equals_the_float64_restatement(pattern, center):
    rows = contour_rows(pattern)
    st, n, index = contour_run(rows, center)
    worst = 0.0
    for b, f in enumerate(rows):
        want, widx = P.contour64(f, center=center)
        k = widx.size
        assert n[b] == k and np.array_equal(index[b, :k], widx)
        assert not st[b, k:].any() and (index[b, k:] == -1).all()
        err = np.abs(st[b, :k].astype(np.float64) - want)
        bar = 2.0 ** -23 * np.maximum(1.0, np.abs(want))
        assert (err <= bar).all(), (pattern, f.size)
        if k:
            worst = max(worst, float((err / bar).max()))
        if pattern == "one" and center:
            assert k == 1 and st[b, 0] == 0
    print(f"{pattern} center={center}: worst st error / bound {worst:.3g}")
    bare = contour_run(rows, center, want_index=False)
    assert bare[2] is None and np.array_equal(bare[0].view(np.uint32), st.view(np.uint32)) and np.array_equal(bare[1], n)


# ---- 4. a ragged batch is its rows alone --------------------------------------------------------------------------------------------

def test_energy_of_a_ragged_batch_is_its_rows_alone():
    rows = [signals()[0], signals()[3], signals()[10], F.mixed()]
    assert [r.size for r in rows] == [1, 257, 1500, 16000]
    e, T = energy_run(rows)
    again, wider, turned = energy_run(rows)[0], energy_run(rows, extra_L=20, extra_T=9, shift=3)[0], energy_run(rows[::-1])[0]
    for b, r in enumerate(rows):
        t = int(T[b])
        alone = energy_run([r])[0]
        for other, slot in ((again, b), (wider, b), (turned, 3 - b), (alone, 0)):
            assert np.array_equal(e[b, :t].view(np.uint32), other[slot, :t].view(np.uint32)), b


def test_prosody_of_a_ragged_batch_is_its_rows_alone():
    f0s, ens, durs, _ = prosody_case()
    pick = (0, 1, 4, 5)                                       # 1, 2, 257 and 600 phones: lengths 1, short, straddling 256, long
    f0s, ens, durs = [f0s[i] for i in pick], [ens[i] for i in pick], [durs[i] for i in pick]
    o, s = prosody_run(f0s, durs, ens)
    again = prosody_run(f0s, durs, ens)
    wider = prosody_run(f0s, durs, ens, extra_T=40, extra_Np=300)
    turned = prosody_run(f0s[::-1], durs[::-1], ens[::-1])
    for b in range(4):
        Np = len(durs[b])
        alone = prosody_run([f0s[b]], [durs[b]], [ens[b]])
        for other, slot in ((again, b), (wider, b), (turned, 3 - b), (alone, 0)):
            assert np.array_equal(o[b, :Np].view(np.uint64), other[0][slot, :Np].view(np.uint64)), b
            assert s[b] == other[1][slot]


@pytest.mark.parametrize("center", [True, False])
def test_contour_of_a_ragged_batch_is_its_rows_alone(center):
    rows = [contour_rows("mixed")[i] for i in (0, 1, 6, 7)]   # 1, 63, 257 and 1000 frames
    st, n, index = contour_run(rows, center)
    again, wider, turned = contour_run(rows, center), contour_run(rows, center, extra_T=300), contour_run(rows[::-1], center)
    for b, r in enumerate(rows):
        alone = contour_run([r], center)
        for other, slot in ((again, b), (wider, b), (turned, 3 - b), (alone, 0)):
            k = int(n[b])
            assert other[1][slot] == k and np.array_equal(index[b, :k], other[2][slot, :k])
            assert np.array_equal(st[b, :k].view(np.uint32), other[0][slot, :k].view(np.uint32)), b


# ---- 5. composed -----------------------------------------------------------------------------------------------------------------

def test_pitch_distance_on_the_warped_transposed_pair():
    """Observed on an MI355X: centred 3.3e-07 semitones (bar 2.65e-06), uncentred |rms - 3| 0 (bar 2.47e-05), reversed 3.9."""
    from megatts2_amd import megatts2 as M
    a, b = P.warped_pair()
    Ta, Tb = a.size, b.size
    A = np.zeros((4, Ta + 2), np.float32)
    Bm = np.zeros((4, Tb + 3), np.float32)
    A[:, Ta:], Bm[:, Tb:] = 250.0, 250.0                      # voiced frames behind the lengths: never read
    A[0, :Ta], Bm[0, :Tb] = a, b
    A[2, :Ta], Bm[2, :Tb] = a, b                              # row 1: a has no voiced frame; row 3: b has none
    Bm[1, :Tb], A[3, :Ta] = b, a
    la, lb = np.full(4, Ta, np.int32), np.full(4, Tb, np.int32)
    top = float(max(np.abs(P.contour(a)[0]).max(), np.abs(P.contour(b)[0]).max()))
    got = M.pitch_distance(A, Bm, la, lb)
    print(f"centred: {got['rms_semitones'][0]:.3g} semitones over {got['steps'][0]} steps (bar {4 * 2.0 ** -24 * top:.3g})")
    assert got["voiced_a"].tolist() == [53, 0, 53, 53] and got["voiced_b"].tolist() == [106, 106, 106, 0]
    assert np.isnan(got["rms_semitones"][[1, 3]]).all() and got["steps"][[1, 3]].tolist() == [0, 0]
    assert got["rms_semitones"][0] <= 4 * 2.0 ** -24 * top and got["steps"][0] >= 106
    assert got["rms_semitones"][2] == got["rms_semitones"][0] and got["steps"][2] == got["steps"][0]
    alone = M.pitch_distance(a, b)                            # the unvoiced neighbours did not disturb the pair
    assert alone["rms_semitones"][0] == got["rms_semitones"][0] and alone["steps"].tolist() == [got["steps"][0]]
    raw = M.pitch_distance(a, b, center=False)
    utop = float(np.abs(P.contour(b, center=False)[0]).max())
    print(f"uncentred: |rms - 3| {abs(raw['rms_semitones'][0] - 3):.3g} (bar {4 * 2.0 ** -24 * utop:.3g})")
    assert abs(raw["rms_semitones"][0] - 3.0) <= 4 * 2.0 ** -24 * utop and raw["steps"][0] == 106
    rev = np.concatenate([a[a > 0][::-1], np.zeros(2, np.float32)])
    back = M.pitch_distance(rev, b)["rms_semitones"][0]
    print(f"reversed: {back:.3g} semitones")
    assert back > got["rms_semitones"][0]
    assert np.isnan(M.pitch_distance(np.zeros(5, np.float32), b)["rms_semitones"][0])


@functools.lru_cache(maxsize=None)
def tiny_tts(padding):
    """the tiny model with synthetic weights; padding None: no vocoder weights, else HiFi-GAN with that inference padding"""
    from megatts2_amd import megatts2 as M
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    voc = None if padding is None else M.HIFIGAN(dataclasses.replace(h, inference_padding=padding), sd_h)
    return M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)), hifi_gan=voc)


def synth_inputs():
    (g, _, _, _), _ = synth_models("tiny")
    rng = np.random.default_rng(77)
    phone = rng.integers(1, g.mrte.phone_vocab_size, (2, 6))
    prompt = rng.standard_normal((2, 40, 80)).astype(np.float32)
    return dev(phone.astype(np.int64)), dev(prompt), np.array([6, 4], np.int32), np.array([40, 33], np.int32)


def check_output_prosody(tts, mel_lens, aux, pl):
    from megatts2_amd import megatts2 as M
    out = tts.output_prosody(mel_lens, aux, phone_lens=pl)
    dur = aux["dur"].cpu().numpy()
    ml = np.asarray(mel_lens, np.int32)
    for b in range(2):
        n = int(pl[b])
        assert dur[b, :n].sum() == ml[b]
        assert np.array_equal(out["phones"]["frames"][b, :n], dur[b, :n]) and not out["phones"]["frames"][b, n:].any()
        want = P.duration_moments(dur[b, :n])
        got = np.array([out["durations"][k][b] for k in M.DURATION_STATS])
        assert np.allclose(got, want, rtol=1e-12, atol=0)
    assert out["f0"].shape == out["energy"].shape and out["f0"].shape[1] >= ml.max()
    again = M.phone_prosody(out["f0"], aux["dur"], out["energy"], pl, ml, check_sum=True)
    assert all(np.array_equal(again[k], out["phones"][k]) for k in M.PHONE_PROSODY)
    with pytest.raises(ValueError):
        M.phone_prosody(out["f0"], aux["dur"], out["energy"], pl, ml - 1, check_sum=True)
    assert np.array_equal(M.duration_stats(dur, pl)["mean_frames"], out["durations"]["mean_frames"])
    return out


def test_output_prosody_of_a_griffin_lim_synthesis():
    tts = tiny_tts(None)
    phone, prompt, pl, ml = synth_inputs()
    mel, mel_lens, aux = tts.synthesize(phone, prompt, pl, ml, griffin_lim={"n_iter": 2}, return_aux=True)
    out = check_output_prosody(tts, mel_lens, aux, pl)
    fe = frontend()
    lens = (np.asarray(mel_lens, np.int32) - 1) * 256
    assert torch.equal(out["f0"], fe.f0(aux["wav"], lens)) and torch.equal(out["energy"], fe.energy(aux["wav"], lens))
    assert out["f0"].shape[1] == int(np.max(mel_lens))
    assert torch.equal(tts.output_prosody(mel_lens, aux, "viterbi", pl)["f0"], fe.f0_track(aux["wav"], lens))


def test_output_prosody_of_a_hifigan_synthesis_takes_the_padding_off():
    pad = 5
    tts = tiny_tts(pad)
    phone, prompt, pl, ml = synth_inputs()
    mel, mel_lens, aux = tts.synthesize(phone, prompt, pl, ml, vocoder=True, return_aux=True)
    out = check_output_prosody(tts, mel_lens, aux, pl)
    fe = frontend()
    ml_out = np.asarray(mel_lens, np.int32)
    top = int(ml_out.max())
    cut = aux["wav"][:, pad * 256:(pad + top) * 256].contiguous()
    assert torch.equal(out["energy"], fe.energy(cut, ml_out * 256)) and torch.equal(out["f0"], fe.f0(cut, ml_out * 256))
    wrong = fe.energy(aux["wav"][:, :top * 256].contiguous(), ml_out * 256)       # offset 0: the padding still in front
    assert not torch.equal(out["energy"], wrong)
    assert out["energy"].shape[1] == top + 1


def test_surface():
    from megatts2_amd import megatts2 as M
    fe = M._frontend()
    x = P.truth_signal().copy()                               # writable: torch.as_tensor warns about a read-only array
    e = M.extract_energy(x)
    f = M.extract_f0(x)
    assert e.dim() == 1 and e.shape == f.shape == (97,)
    assert np.array_equal(e.cpu().numpy().view(np.uint32), P.energy32(x).view(np.uint32))
    both = M.extract_energy(np.stack([x, x]), trim_db=40)
    assert both.shape == M.extract_f0(np.stack([x, x]), trim_db=40).shape and both.shape[0] == 2
    x44 = np.concatenate([np.zeros(9000, np.float32), 0.5 * np.sin(2 * np.pi * 196.0 * np.arange(22050) / 44100).astype(np.float32)])
    assert M.extract_energy(x44, 44100).shape[0] == M.extract_mel_spec(x44, 44100).shape[1]
    dur, inner = P.truth_alignment(97)
    pp = M.phone_prosody(f, dur, e, check_sum=True)
    assert list(pp) == list(M.PHONE_PROSODY) and all(v.shape == (1, 9) and v.dtype == np.float64 for v in pp.values())
    assert abs(float(F.cents(pp["mean_hz"][0, 1], 110.0))) <= 1.0 and pp["voiced_frames"][0, 5] == 0
    with pytest.raises(ValueError):
        M.phone_prosody(f, dur[:-1], e, check_sum=True)
    on_device = M.phone_prosody(f, dev(dur), e)
    assert all(np.array_equal(on_device[k], pp[k]) for k in pp)
    ds = M.duration_stats(dur)
    assert list(ds) == list(M.DURATION_STATS) and np.allclose([ds[k][0] for k in ds], P.duration_moments(dur), rtol=1e-12, atol=0)
    st, n, index = fe.pitch_contour(f.unsqueeze(0), return_index=True)
    want, widx = P.contour(f.cpu().numpy())
    assert int(n[0]) == widx.size and np.array_equal(index[0, :widx.size].cpu().numpy(), widx)
    out = torch.full((1, 120), 5.0, device="cuda")
    assert fe.energy(dev(x[None]), out=out) is out and torch.equal(out[0, :97], e) and not out[0, 97:].any()


# ---- 6. refusals -------------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_device_outputs_untouched():
    rows = [signals()[10], signals()[3]]                      # 1500 and 257 samples
    for kw in (dict(lens=[1500, 0]), dict(lens=[1508, 257]), dict(lens=[-1, 257]), dict(hop=0), dict(hop=-1), dict(hop=1025),
               dict(T_w=1 + 1500 // 256 - 1), dict(hop=80, T_w=1 + 1500 // 80 - 1)):
        assert energy_run(rows, expect_error=True, **kw) is None
    f0s, ens, durs, _ = prosody_case()
    f0s, ens, durs = f0s[:2], ens[:2], durs[:2]
    Np_w, T_w = 2 + 3, max(f.size for f in f0s) + 5
    for kw in (dict(phone_lens=[1, 0]), dict(phone_lens=[Np_w + 1, 2]), dict(frame_lens=[0, 5]), dict(frame_lens=[9, T_w + 1])):
        assert prosody_run(f0s, durs, ens, expect_error=True, **kw) is None
    crows = contour_rows("mixed")[:3]
    for kw in (dict(frame_lens=[1, 63, 0]), dict(frame_lens=[1, 63, 64 + 5]), dict(center=2)):
        assert contour_run(crows, expect_error=True, **kw) is None
    # B outside [1, 65535] and overlapping buffers: the C entry points themselves
    R = rt()
    fe = frontend()
    base = torch.zeros(4096, device="cuda", dtype=torch.float32)
    before = base.clone()
    ok = torch.full((64,), SENT, device="cuda", dtype=torch.float32)
    ok64 = torch.full((64,), SENT, device="cuda", dtype=torch.float64)
    oki = torch.full((64,), ISENT, device="cuda", dtype=torch.int32)
    one = np.array([1000, 900], np.int32)
    fl, pl = np.array([10, 9], np.int32), np.array([4, 3], np.int32)
    dur = torch.ones(8, device="cuda", dtype=torch.int32)

    def energy(B, out, wav=base):
        return fe.lib.mt2_frame_energy(fe.h, R._stream(), R._ptr(wav), R._iptr(one), 1000, B, 256, R._ptr(out), 4)

    def phones(B, out, f0=base, en=None, tot=None):
        return fe.lib.mt2_phone_prosody(fe.h, R._stream(), R._ptr(f0), R._ptr(en), R._ptr(dur), R._iptr(pl), 4, R._iptr(fl), 10, B,
                                        R._ptr(out), R._ptr(tot))

    def contour(B, st, n, index=None, f0=base):
        return fe.lib.mt2_pitch_contour(fe.h, R._stream(), R._ptr(f0), R._iptr(fl), 10, B, 1, R._ptr(st), R._ptr(n), R._ptr(index))

    for B in (0, -1, 65536):
        assert energy(B, ok) != 0 and phones(B, ok64) != 0 and contour(B, ok, oki) != 0
    assert energy(2, base[1996:]) != 0 and energy(2, base[8:]) != 0
    inside = base[16:].view(torch.float64)
    assert phones(2, inside) != 0 and phones(2, ok64, en=ok64.view(torch.float32)) != 0
    assert phones(2, ok64, tot=base[4:].view(torch.int64)) != 0 and phones(2, ok64, tot=ok64[8:].view(torch.int64)) != 0
    assert contour(2, base[12:], oki) != 0 and contour(2, ok, base[16:].view(torch.int32)) != 0
    assert contour(2, ok, oki, index=base[4:].view(torch.int32)) != 0 and contour(2, ok, oki, index=ok.view(torch.int32)[8:]) != 0
    torch.cuda.synchronize()
    assert torch.equal(base, before) and (ok == SENT).all() and (ok64 == SENT).all() and (oki == ISENT).all()
    assert energy(2, ok) == 0 and phones(2, ok64) == 0 and contour(2, ok, oki[32:], index=oki) == 0      # valid calls go through
    torch.cuda.synchronize()
    assert torch.equal(base, before) and not (ok[:8] == SENT).any() and not (ok64[:64] == SENT).any() and (oki[:20] == -1).all()
