"""Stationary-noise suppression on the GPU (csrc/denoise.hip: mt2_noise_floor, mt2_spectral_gain, mt2_denoise) against the restatement
of its rule (tests/denoise_ref.py): the select and the gain chain bit for bit on the device's own spectrum, the whole call against
float64 and against analytic ground truth, then batches, ranges, refusals and the Python surface.

Conventions: outputs are wider than needed, pre-filled with a sentinel and followed by guard words; samples at or beyond an
utterance's length, spectrum frames at or beyond its frame count and the pad columns of a spectrum are NaN (a read of one poisons the
output).  Two audio configurations: a small one (n_fft 128, hop 32: F = 65, Fp = 68, S = 132, so that both pads exist) and the
model's (1024 / 256).  Frame counts 4 (the smallest mt2_istft accepts), 5, 255, 256, 257 (around the 64 rows a select step takes and
the 16 of a gain tile) and 4100 (over 4096: more than one select step per thread many times over, 257 gain tiles).

Bars.  Bit equality wherever the rule fixes the arithmetic.  The whole call against float64: WAV_BAR below."""
import ctypes as C
import functools

import numpy as np
import pytest

import denoise_ref as D
from conftest import synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = np.float32(-777.25)
GUARD = 64
SR = 16000
FRAMES = (4, 5, 255, 256, 257, 4100)
# The closed loop istft(stft(x)) holds 5e-7 relative L2 against x (tests/test_gpu_griffinlim.py, RT_OBSERVED).  The denoiser puts a gain
# between the two transforms.  With eps the relative error of a spectrum cell, P and Nf each carry 2 eps, and g0 = 1 - beta Nf / P moves
# by beta Nf / P (2 eps + 2 eps) <= 0.9 x 4 eps = 3.6 eps wherever it is above g_min = 0.1 (below, it is g_min exactly; max() and the
# order statistic are continuous, so a cell that changes branch moves no further).  The gated cell g S then carries at most 3.6 eps
# / g + eps; weighted by the energy g^2 P the cells near the floor count for little, and on the cells that carry the output (g near 1)
# that is 4.6 eps, plus the inverse transform's own share of the loop.  Margin 8 covers 4.6 + 1 with room for the means' roundings.
# The restatement's own f32 run on these inputs sits at 1.3e-7 .. 4.2e-7.
RT_HOLDS = 5.0e-7
WAV_BAR = 8 * RT_HOLDS
# a cell within the gain's error of the branch edge may take the other branch: q's density near g_min is about 0.1 per unit for
# exponentially distributed P, the error under 1e-5, so about 1e-6 of the cells - the cap is 1e-3.  The f32 restatement differs from
# float64 in none of the cells of these inputs.
BRANCH_CAP = 1e-3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint64)


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


@functools.lru_cache(maxsize=None)
def audio(name):
    from megatts2_amd.config import AudioConfig
    if name == "prod":
        return AudioConfig()
    return AudioConfig(sample_rate=SR, n_fft=128, hop_length=32, win_length=128, n_mels=8, f_min=0.0, f_max=8000.0)


@functools.lru_cache(maxsize=None)
def frontend(name):
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd(audio(name))


def geometry(name):
    F = audio(name).n_fft // 2 + 1
    return F, (F + 3) & ~3, (2 * F + 3) & ~3


@functools.lru_cache(maxsize=None)
def signal(name, T, tail=7):
    """noise under a tone gated on for alternate half-seconds (both branches of the gain), T frames and `tail` samples more"""
    a = audio(name)
    L = (T - 1) * a.hop_length + tail
    return (D.tone(L, SR, gated=True, hz=1000.0) + D.white_noise(L, seed=T)).astype(np.float32)


def wav_batch(xs, extra=5):
    """[B, L_max + extra] with NaN at and beyond every utterance's length"""
    lens = np.asarray([len(x) for x in xs], np.int32)
    w = np.full((len(xs), int(lens.max()) + extra), np.nan, np.float32)
    for b, x in enumerate(xs):
        w[b, :len(x)] = x
    return w, lens


@functools.lru_cache(maxsize=None)
def device_spectrum(name, T):
    """mt2_stft of signal(name, T) alone, as the packed f32 [T, S] rows the library writes (host copy); computed once and shared"""
    from megatts2_amd import runtime as rt
    fe = frontend(name)
    x = dev(signal(name, T)[None])
    S = geometry(name)[2]
    spec = torch.empty(1, T, S, device="cuda", dtype=torch.float32)
    ln = np.asarray([x.shape[1]], np.int32)
    rt._check(fe.lib.mt2_stft(fe.h, rt._stream(), C.byref(fe.ac), rt._ptr(x), rt._iptr(ln), x.shape[1], 1, rt._ptr(spec), T))
    return spec[0].cpu().numpy()


def spec_batch(rows, extra=3):
    """packed spectra [T_b, S] -> [B, T_max + extra, S] with NaN in the pad columns and in the frames at or beyond T_b"""
    Ts = np.asarray([r.shape[0] for r in rows], np.int32)
    S = rows[0].shape[1]
    F = (S // 2) if (S // 2) % 2 else S // 2 - 1      # S = 2 F rounded up to 4 and F is odd
    out = np.full((len(rows), int(Ts.max()) + extra, S), np.nan, np.float32)
    for b, r in enumerate(rows):
        out[b, :Ts[b], :2 * F] = r[:, :2 * F]
    return out, Ts


def power_of(rows, F):
    """the device's own P: the f32 fma of the rule on the spectrum the device made"""
    return D.fma_f32(rows[:, F:2 * F], rows[:, F:2 * F], rows[:, :F] * rows[:, :F])


def crafted(name, T):
    """the device's spectrum with a constant segment (many equal powers in every bin) and one bin zero in every frame"""
    F = geometry(name)[0]
    r = device_spectrum(name, T).copy()
    if T >= 5:
        r[T // 4:T // 2] = r[T // 4]
    r[:, 7] = 0.0
    r[:, F + 7] = 0.0
    return r


# ---- 1. the select, exact -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("percentile", [1, 20, 50, 99])
def test_noise_floor_is_the_exact_order_statistic(percentile):
    from megatts2_amd.runtime import Denoise
    fe = frontend("small")
    F, Fp, _ = geometry("small")
    rows = [crafted("small", T) for T in FRAMES]
    spec, Ts = spec_batch(rows)
    cfg = Denoise(percentile=percentile)
    got = fe.noise_floor(dev(spec), Ts, cfg).cpu().numpy()
    c = D.factor(percentile)
    for b, r in enumerate(rows):
        P = power_of(r, F)
        k = D.rank(Ts[b], percentile)
        want = (np.partition(P, k, axis=0)[k] * c).astype(np.float32)
        assert same(got[b], want), (percentile, int(Ts[b]), int((bits(got[b]) != bits(want)).sum()))
        assert want[7] == 0.0 and (np.sort(P, axis=0)[k] == np.partition(P, k, axis=0)[k]).all()
    alone = fe.noise_floor(dev(spec_batch([rows[4]], extra=0)[0]), None, cfg).cpu().numpy()      # T = 257 alone, no spare frame
    assert same(alone[0], got[4])


def test_noise_floor_at_the_model_configuration():
    fe = frontend("prod")
    F = geometry("prod")[0]
    rows = [crafted("prod", 130), crafted("prod", 40)]
    spec, Ts = spec_batch(rows)
    got = fe.noise_floor(dev(spec), Ts).cpu().numpy()
    for b, r in enumerate(rows):
        P = power_of(r, F)
        k = D.rank(Ts[b], 20)
        assert same(got[b], (np.partition(P, k, axis=0)[k] * D.factor(20)).astype(np.float32))


# ---- 2. gain, smoothing and apply, bit for bit on the device's own P and Nf ------------------------------------------------------------

GAIN_FRAMES = (4, 5, 37, 130)


@pytest.mark.parametrize("bf", [0, 1, 8])
@pytest.mark.parametrize("bt", [0, 1, 8])
def test_gain_chain_is_the_f32_restatement(bf, bt):
    from megatts2_amd.runtime import Denoise
    fe = frontend("small")
    F, Fp, S = geometry("small")
    rows = [device_spectrum("small", T) for T in GAIN_FRAMES]      # bt = 8 >= T for the first two; bf = 8 is clipped at both edges
    spec, Ts = spec_batch(rows)
    cfg = Denoise(smooth_bins=bf, smooth_frames=bt)
    rc = D.Config(smooth_bins=bf, smooth_frames=bt)
    sd = dev(spec)
    floor = fe.noise_floor(sd, Ts, cfg)
    gain, gated = fe.spectral_gain(sd, floor, Ts, cfg, return_gain=True, apply=True)
    nf, gain, gated = floor.cpu().numpy(), gain.cpu().numpy(), gated.cpu().numpy()
    inplace = sd.clone()
    fe.spectral_gain(inplace, floor, Ts, cfg, return_gain=False, apply=True, in_place=True)
    inplace = inplace.cpu().numpy()
    for b, r in enumerate(rows):
        T = int(Ts[b])
        P = power_of(r, F)
        g = D.smooth(D.gain0(P, nf[b], rc, np.float32), rc, np.float32)
        assert g.dtype == np.float32 and same(gain[b, :T], g), (bf, bt, T, int((bits(gain[b, :T]) != bits(g)).sum()))
        assert (gain[b, T:] == 0).all()
        want = np.concatenate([g * r[:, :F], g * r[:, F:2 * F]], axis=1).astype(np.float32)
        assert same(gated[b, :T, :2 * F], want) and (gated[b, :T, 2 * F:] == 0).all() and (gated[b, T:] == 0).all()
        assert same(inplace[b, :T, :2 * F], want)
    keep = np.ones_like(spec, bool)
    for b, T in enumerate(Ts):
        keep[b, :T, :2 * F] = False
    assert np.isnan(inplace[keep]).all()                                      # pad columns and spare frames are left as they were
    if (bf, bt) == (1, 1):
        m = np.concatenate([(D.gain0(power_of(r, F), nf[b], rc, np.float32) == np.float32(0.1)).ravel() for b, r in enumerate(rows)])
        assert 0.5 < m.mean() < 0.999                                         # both branches of the gain are in play


# ---- 3. g_min = 1 is the round trip of the existing calls ------------------------------------------------------------------------------

@pytest.mark.parametrize("name, T", [("small", 4), ("small", 37), ("small", 257), ("prod", 40)])
def test_floor_gain_one_is_istft_of_stft(name, T):
    from megatts2_amd.runtime import Denoise
    fe = frontend(name)
    x = dev(signal(name, T)[None])
    want = fe.istft(fe.stft(x))
    got, lens = fe.denoise(x, None, Denoise(floor_gain=1.0))
    assert lens[0] == (T - 1) * audio(name).hop_length == want.shape[1]
    assert same(got.cpu().numpy(), want.cpu().numpy())


@pytest.mark.parametrize("name, T", [("small", 65), ("prod", 45)])
def test_the_call_is_the_composition_of_the_public_calls(name, T):
    """one utterance, default configuration (the gate at work): mt2_denoise gives the bits of mt2_stft -> mt2_noise_floor ->
    mt2_spectral_gain (apply) -> mt2_istft"""
    fe = frontend(name)
    x = dev(signal(name, T)[None])
    spec = fe.stft(x)
    want = fe.istft(fe.spectral_gain(spec, fe.noise_floor(spec), return_gain=False, apply=True))
    got, lens = fe.denoise(x)
    assert lens[0] == (T - 1) * audio(name).hop_length == want.shape[1]
    assert same(got.cpu().numpy(), want.cpu().numpy())
    assert not same(got.cpu().numpy(), fe.istft(spec).cpu().numpy())


# ---- 4. the whole call against float64 --------------------------------------------------------------------------------------------------

def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


@pytest.mark.parametrize("name, T", [("small", 4), ("small", 37), ("small", 130), ("small", 257), ("prod", 40), ("prod", 130)])
def test_whole_call_against_float64(name, T):
    from megatts2_amd.runtime import Denoise
    fe, a = frontend(name), audio(name)
    F = geometry(name)[0]
    x = signal(name, T)
    ref = D.denoise(x, a)
    got, lens, floor, fig = fe.denoise(dev(x[None]), None, return_floor=True, return_figures=True)
    y = got.cpu().numpy()[0]
    err = rel_l2(y[:lens[0]], ref["y"])
    # the branch of every cell, with the smoothing off so that the gain IS g0
    flat = Denoise(smooth_bins=0, smooth_frames=0)
    g0 = fe.spectral_gain(dev(device_spectrum(name, T)[None]), floor, None, flat).cpu().numpy()[0]
    share = float(((g0 == np.float32(0.1)) != (ref["g0"] == np.float32(0.1))).mean())
    print(f"{name} T={T}: waveform relative L2 {err:.3e} (bar {WAV_BAR:.1e}), cells on the other branch {share:.2e} (cap {BRANCH_CAP:.0e})")
    assert lens[0] == len(ref["y"]) and err <= WAV_BAR
    assert share <= BRANCH_CAP
    # looser companions of the waveform bar: a bin beside the tone carries the transform's error relative to the FRAME, not to itself
    assert np.allclose(floor.cpu().numpy()[0], ref["Nf"], rtol=1e-4, atol=0)
    f, r = fig.cpu().numpy()[0], ref["figures"]
    assert f[4] == T and f[5] == D.rank(T, 20) and f[4] == r[4] and f[5] == r[5]
    assert np.allclose(f[[0, 1, 3]], r[[0, 1, 3]], rtol=0, atol=1e-3) and abs(f[2] - r[2]) <= BRANCH_CAP
    assert np.allclose(f[[6, 7]], r[[6, 7]], rtol=1e-4, atol=0)


# ---- 5. ground truth on the device: the host tests' signals, held to the same assertions --------------------------------------------

def device_denoise(x, cfg=None):
    y, lens = frontend("prod").denoise(dev(np.asarray(x, np.float32)[None]), None, cfg)
    return y.cpu().numpy()[0, :lens[0]]


@pytest.mark.parametrize("seconds", [5, 2])
def test_white_noise_on_the_device(seconds):
    a = audio("prod")
    F = geometry("prod")[0]
    x = D.white_noise(seconds * SR, seed=0)
    y, lens, floor = frontend("prod").denoise(dev(x[None]), None, return_floor=True)
    ratio = float((floor.cpu().numpy()[0, 1:F - 1].astype(np.float64) / (D.SIGMA ** 2 * D.window_energy(a))).mean())
    drop = -D.level_db(y.cpu().numpy()[0, :lens[0]], x)
    print(f"white noise {seconds} s on the device: mean Nf / (sigma^2 sum w^2) = {ratio:.4f}, output {drop:.2f} dB under the input")
    if seconds == 5:
        assert abs(ratio - 1.0) < 0.05
    assert drop >= 15.0


def test_gated_and_steady_tone_on_the_device():
    from megatts2_amd.runtime import Denoise
    L = 5 * SR
    noise = D.white_noise(L, seed=0)
    clean = D.tone(L, SR, gated=True)
    x = (clean + noise).astype(np.float32)
    before = D.snr_db(x, clean)
    at20, at50 = D.snr_db(device_denoise(x, Denoise(percentile=20)), clean), D.snr_db(device_denoise(x, Denoise(percentile=50)), clean)
    print(f"gated tone on the device: SNR {before:.2f} dB -> {at20:.2f} dB at percentile 20, {at50:.2f} dB at percentile 50")
    assert at20 - before >= 8.0 and at50 <= before
    x = (D.tone(L, SR, gated=False) + noise).astype(np.float32)
    a0, a1 = D.tone_amplitude(x, SR), D.tone_amplitude(device_denoise(x), SR)
    print(f"steady tone on the device: amplitude {a0:.4f} -> {a1:.4f}")
    assert 20 * np.log10(a1 / a0) <= -15.0


# ---- 6. batch and ranges --------------------------------------------------------------------------------------------------------

def run(fe, xs, cfg=None, floor=None, width=None):
    """one mt2_denoise call on the ragged batch xs -> (out rows [B, W], out_lens, floor, figures, guards intact)"""
    w, lens = wav_batch(xs)
    B = len(xs)
    hop = fe.audio.hop_length
    W = width or hop * (int(lens.max()) // hop) + 9
    buf = torch.full((B * W + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
    out, out_lens, used, fig = fe.denoise(dev(w), lens, cfg, noise_floor=floor, return_floor=True, return_figures=True, out=buf[:B * W].view(B, W))
    h = buf.cpu().numpy()
    return h[:B * W].reshape(B, W), out_lens, used.cpu().numpy(), fig.cpu().numpy(), bool((h[B * W:] == SENT).all())


@pytest.mark.parametrize("name, Ts", [("small", (37, 4, 257, 130, 5)), ("prod", (40, 130, 4))])
def test_batch_is_its_utterances_alone(name, Ts):
    fe, a = frontend(name), audio(name)
    xs = [signal(name, T, tail=(3 * i) % a.hop_length) for i, T in enumerate(Ts)]
    out, lens, floor, fig, ok = run(fe, xs)
    assert ok
    for b, x in enumerate(xs):
        n = (Ts[b] - 1) * a.hop_length
        assert lens[b] == n and (out[b, n:] == 0).all() and np.isfinite(out[b, :n]).all()
        o1, l1, f1, g1, ok1 = run(fe, [x])
        assert ok1 and l1[0] == n
        assert same(out[b, :n], o1[0, :n]) and same(floor[b], f1[0]) and same(fig[b], g1[0]), (name, Ts[b])


def test_a_floor_passed_in_gives_the_bits_of_the_call_that_made_it():
    fe = frontend("small")
    xs = [signal("small", T) for T in (37, 130)]
    out, _, floor, fig, _ = run(fe, xs)
    out2, _, floor2, fig2, ok = run(fe, xs, floor=dev(floor))
    assert ok and same(out, out2) and same(floor, floor2) and same(fig, fig2)
    # a profile from a noise-only clip: mt2_noise_floor on mt2_stft of the clip, through the same argument
    noise = D.white_noise(130 * 32, seed=9)
    profile = fe.noise_floor(fe.stft(dev(noise[None])))
    out3, _, used, _, ok = run(fe, xs, floor=profile.expand(2, -1))
    assert ok and same(used[0], profile.cpu().numpy()[0]) and not same(out3, out)


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------

def test_refusals_launch_nothing_and_leave_the_output():
    from megatts2_amd import runtime as rt
    fe = rt.MelFrontEnd(audio("small"))      # a handle nothing has used: a refused call leaves its arena untouched
    try:
        x = signal("small", 37)
        w, lens = wav_batch([x, x[:500]])
        W = 32 * (len(x) // 32)
        big = torch.zeros(2 * w.shape[1] + 2 * W, device="cuda", dtype=torch.float32)
        wd = big[:2 * w.shape[1]].view(2, w.shape[1])
        wd.copy_(dev(w))
        over = big[w.shape[1]:w.shape[1] + 2 * W].view(2, W)                                   # a buffer that lies across the second row of wav
        out = torch.full((2, W), float(SENT), device="cuda", dtype=torch.float32)
        floor = torch.full((2, 68), float(SENT), device="cuda", dtype=torch.float32)

        def refused(cfg=None, ln=lens, o=out, **kw):
            with pytest.raises(rt.NativeError) as e:
                fe.denoise(wd, ln, cfg, out=o, **kw)
            torch.cuda.synchronize()
            assert (out == float(SENT)).all() and fe.workspace_high_water() == 0 and fe.memory()[1] == 0
            return str(e.value)

        assert "percentile" in refused(rt.Denoise(percentile=0)) and "percentile" in refused(rt.Denoise(percentile=100))
        assert "over_subtraction" in refused(rt.Denoise(over_subtraction=0.0))
        assert "over_subtraction" in refused(rt.Denoise(over_subtraction=float("nan")))
        assert "floor_gain" in refused(rt.Denoise(floor_gain=1.5)) and "floor_gain" in refused(rt.Denoise(floor_gain=0.0))
        assert "smooth_bins" in refused(rt.Denoise(smooth_bins=9)) and "smooth_frames" in refused(rt.Denoise(smooth_frames=9))
        assert "fewer frames" in refused(ln=np.asarray([len(x), 95], np.int32))                # T = 3
        assert "Lout_max" in refused(o=out[:, :W - 1].contiguous())
        assert "overlapping" in refused(o=over)
        assert same(wd.cpu().numpy(), w)
        assert "outside [1, L_max]" in refused(ln=np.asarray([len(x), w.shape[1] + 1], np.int32))
        with pytest.raises(rt.NativeError):                                                      # B < 1
            dc = rt.Denoise().c_struct()
            rt._check(fe.lib.mt2_denoise(fe.h, rt._stream(), C.byref(fe.ac), C.byref(dc), rt._ptr(wd), rt._iptr(lens), w.shape[1], 0, None, None,
                                         None, rt._ptr(out), W))
        assert (out == float(SENT)).all() and fe.workspace_high_water() == 0
        spec = torch.full((2, 6, 132), float(SENT), device="cuda", dtype=torch.float32)
        for call in (lambda: fe.noise_floor(spec, [6, 7]), lambda: fe.spectral_gain(spec, floor, [0, 6]),
                     lambda: fe.noise_floor(spec, None, rt.Denoise(percentile=0)), lambda: fe.spectral_gain(spec, floor, None, rt.Denoise(smooth_bins=-1))):
            with pytest.raises(rt.NativeError):
                call()
        torch.cuda.synchronize()
        assert fe.workspace_high_water() == 0 and (spec == float(SENT)).all() and (floor == float(SENT)).all()
        got, ln = fe.denoise(wd, lens, out=out)                                                  # and the accepted call writes it
        assert fe.workspace_high_water() > 0 and ln.tolist() == [W, 480] and bool((out[1, 480:] == 0).all())
    finally:
        fe.close()


# ---- 8. the surface -------------------------------------------------------------------------------------------------------------------

def test_non_finite_input_does_not_fault():
    fe = frontend("small")
    x = signal("small", 130).copy()
    x[100], x[700], x[2000] = np.nan, np.inf, -np.inf
    out, lens, floor, fig, ok = run(fe, [x, signal("small", 37)])
    assert ok and lens.tolist() == [129 * 32, 36 * 32]
    alone = run(fe, [signal("small", 37)])
    assert same(out[1, :lens[1]], alone[0][0, :lens[1]])                       # the other utterance is untouched by it


def peak_normalized(fe, x, ln):
    """mt2_peak_normalize as MelFrontEnd.from_audio calls it -> a new tensor"""
    from megatts2_amd import runtime as rt
    y = torch.empty_like(x)
    rt._check(fe.lib.mt2_peak_normalize(fe.h, rt._stream(), rt._ptr(x), rt._iptr(ln), x.shape[1], x.shape[0], rt._ptr(y)))
    return y


def test_prompt_paths_without_the_argument_keep_their_bits():
    from megatts2_amd import megatts2 as M
    from megatts2_amd.runtime import Denoise
    fe = M._frontend()
    x = signal("prod", 40)
    x48 = np.interp(np.arange(3 * len(x)) / 3.0, np.arange(len(x)), x).astype(np.float32)
    for wav, sr in ((x, SR), (x48, 48000)):
        xd = dev(wav[None])
        mel0, n0 = fe.from_audio(xd, sr, trim_db=30.0)
        mel1, n1 = fe.from_audio(xd, sr, trim_db=30.0, denoise=None)
        assert same(mel0.cpu().numpy(), mel1.cpu().numpy()) and n0.tolist() == n1.tolist()
        if sr == SR:      # ... and they are what the primitives give, as before
            t, tl, _ = fe.trim(peak_normalized(fe, xd, np.asarray([len(wav)], np.int32)), None, 30.0)
            assert same(fe(t, tl).cpu().numpy(), mel0.cpu().numpy())
        # with the argument: resample (+ normalise) -> denoise -> normalise -> trim -> mel, by the same primitives
        mel2, n2, fig = fe.from_audio(xd, sr, trim_db=30.0, denoise=Denoise(), return_noise=True)
        if sr != SR:
            y, ln = fe.resample(xd, sr, normalize=True)
        else:
            ln = np.asarray([len(wav)], np.int32)
            y = peak_normalized(fe, xd, ln)
        d, dl, dfig = fe.denoise(y, ln, Denoise(), return_figures=True)
        d = peak_normalized(fe, d, dl)
        t, tl, _ = fe.trim(d, dl, 30.0)
        assert same(fe(t, tl).cpu().numpy(), mel2.cpu().numpy()) and same(dfig.cpu().numpy(), fig.cpu().numpy())
        assert abs(float(d.abs().max()) - 1.0) < 1e-6
    m0 = M.extract_mel_spec(torch.from_numpy(x))
    assert same(m0.cpu().numpy(), M.extract_mel_spec(torch.from_numpy(x), denoise=None).cpu().numpy())
    assert same(m0.cpu().numpy(), fe(dev(x[None]))[0].transpose(0, 1).contiguous().cpu().numpy())
    md = M.extract_mel_spec(torch.from_numpy(x), denoise=Denoise())
    assert md.shape == (80, 40) and not same(md.cpu().numpy(), m0.cpu().numpy())
    out, st = M.denoise_audio(x)
    assert same(out, fe.denoise(dev(x[None]))[0].cpu().numpy()[0]) and st["frames"][0] == 40 and st["floor"].shape == (1, 513)
    out_n, st_n = M.denoise_audio(x, noise=D.white_noise(8000, seed=4))
    assert out_n.shape == out.shape and not same(st_n["floor"], st["floor"])


def test_forward_denoises_every_prompt_file(tmp_path):
    """Megatts.forward(denoise=...): every prompt file, the 16 kHz one too, goes through from_audio(denoise=...); without the argument
    the call is what it was"""
    from megatts2_amd import audio_io, megatts2 as M
    from megatts2_amd.runtime import Denoise
    (g, p, a, _), (sd_g, sd_p, sd_a, _) = synth_models("tiny")
    tts = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)))
    wavs = tmp_path / "prompts"
    wavs.mkdir()
    x = signal("prod", 40)
    x48 = np.interp(np.arange(3 * len(x)) / 3.0, np.arange(len(x)), x).astype(np.float32)
    audio_io.write_wav(str(wavs / "a.wav"), x, SR)
    audio_io.write_wav(str(wavs / "b.wav"), x48, 48000)
    phone = np.random.default_rng(13).integers(0, g.mrte.phone_vocab_size, 6)
    mel0, lens0, aux0 = tts.forward(str(wavs), phone_tokens=phone, out_path=None)
    mel1, lens1, aux1 = tts.forward(str(wavs), phone_tokens=phone, out_path=None, denoise=None)
    assert torch.equal(mel0, mel1) and "prompt_noise" not in aux0 and "prompt_noise" not in aux1
    mel2, lens2, aux2 = tts.forward(str(wavs), phone_tokens=phone, out_path=None, denoise=Denoise())
    fe = M._frontend()
    noise = aux2["prompt_noise"]
    assert len(noise) == 2 and all(set(n) == set(D.FIELDS) for n in noise)
    for (path, n) in zip(("a.wav", "b.wav"), noise):
        y, sr = audio_io.read_wav(str(wavs / path))
        fig = fe.from_audio(dev(y[None]), sr, denoise=Denoise(), return_noise=True)[2].cpu().numpy()[0]
        assert [n[k] for k in D.FIELDS] == fig.tolist() and n["frames"] == 40 and -25.0 < n["reduction_db"] < 0.0
    assert mel2.shape[0] == mel0.shape[0] and np.isfinite(mel2.cpu().numpy()).all()
