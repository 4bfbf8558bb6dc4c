"""De-reverberation by weighted prediction error on the GPU (csrc/wpe.hip: mt2_wpe_spectrum, mt2_dereverb) against the float64
restatement of its rule (tests/wpe_ref.py) on the device's own spectrum, against ground truth (a known prediction filter, a hop-aligned
echo; the bars of tests/test_wpe_host.py), then batches, the write set and the Python surface.

Conventions (those of tests/test_gpu_denoise.py): outputs are wider than needed, pre-filled with a sentinel and followed by guard words;
samples at or beyond an utterance's length, spectrum frames at or beyond its frame count and the pad columns of a spectrum are NaN.  Two
audio configurations: a small one (n_fft 128, hop 32: F = 65, Fp = 68, S = 132) and the model's (1024 / 256).

Frame counts of the spectrum call: 1, 3, 4 (T <= delay and T = delay + 1: one non-zero regressor), 13 and 14 (around delay + taps),
63 / 64 / 65 and 255 / 256 / 257 (around a wave's stride over t and the 32-frame tiles of the transpositions; 512, a workgroup's stride,
lies inside 4100) and 4100 (past kWpeLdsFrames = 4096: the column streams from the bin-major scratch instead of sitting in LDS).

The bar.  The device and the restatement differ in the order of their sums and in where a product and a sum are one fma; both are
relative perturbations of R and p of the size of a rounding, which cond(R) turns into the error of g and D.  Measured on the CPU, on
these inputs (G.stft of the same signals), as the restatement against itself with the t-sums in the kernel's lane order and in ascending
order, relative L2 per bin, the largest over every frame count and configuration:  D (f32 parts) 2.2e-8 (T = 14, K 16),
g 6.8e-9 (T = 14, K 16).  The bars are 16 times these.  The device against the restatement read, on an MI355X, at most 5.4e-9 for D and
5.9e-9 for g (both at T = 14, K 16), and 0 for D wherever R is well conditioned (the f32 rounding of the output hides the rest)."""
import ctypes as C
import functools

import numpy as np
import pytest

import wpe_ref as W
from conftest import synth_models
from test_wpe_host import ECHO, KNOWN

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = np.float32(-777.25)
GUARD = 64
SR = 16000
ORDER_NOISE_D, ORDER_NOISE_G = 2.2e-8, 6.8e-9
D_BAR, G_BAR = 16 * ORDER_NOISE_D, 16 * ORDER_NOISE_G
FRAMES = (1, 3, 4, 13, 14, 63, 64, 65, 255, 256, 257, 4100)
CONFIGS = {"default": {}, "long": dict(taps=16, delay=1, context=4, iterations=8), "short": dict(taps=1, delay=8, context=0, iterations=1)}


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({4: np.uint32, 8: np.uint64, 16: np.uint64}[a.dtype.itemsize])


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
def device_spectrum(name, T):
    """mt2_stft of W.spectrum_signal alone, as the packed f32 [T, S] rows the library writes (host copy); computed once and shared"""
    from megatts2_amd import runtime as rt
    fe = frontend(name)
    x = dev(W.spectrum_signal(audio(name), T)[None])
    S = geometry(name)[2]
    spec = torch.empty(1, T, S, device="cuda", dtype=torch.float32)
    ln = np.asarray([x.shape[1]], np.int32)
    rt._check(fe.lib.mt2_stft(fe.h, rt._stream(), C.byref(fe.ac), rt._ptr(x), rt._iptr(ln), x.shape[1], 1, rt._ptr(spec), T))
    return spec[0].cpu().numpy()


def rows_of(name, T):
    """the first T frames of the longest spectrum of the configuration: any T >= 1, which mt2_stft itself does not give"""
    return device_spectrum(name, 4100 if name == "small" else 257)[:T]


def spec_batch(rows, extra=3):
    """packed spectra [T_b, S] -> [B, T_max + extra, S] with NaN in the pad columns and in the frames at or beyond T_b"""
    Ts = np.asarray([r.shape[0] for r in rows], np.int32)
    S = rows[0].shape[1]
    F = (S // 2) if (S // 2) % 2 else S // 2 - 1      # S = 2 F rounded up to 4 and F is odd
    out = np.full((len(rows), int(Ts.max()) + extra, S), np.nan, np.float32)
    for b, r in enumerate(rows):
        out[b, :Ts[b], :2 * F] = r[:, :2 * F]
    return out, Ts


def rel_bins(a, b):
    """relative L2 per bin (axis 0 = frames or taps), 0 where the reference is zero and so is the other"""
    n = np.linalg.norm(b, axis=0)
    d = np.linalg.norm(a - b, axis=0)
    return np.where(n > 0, d / np.where(n > 0, n, 1.0), d)


def wpe_call(fe, rows, cfg, **kw):
    """one mt2_wpe_spectrum call on a ragged batch of packed spectra -> (spec_out host [B, T_max + 3, S], filters [B, F, K], figures, Ts, spec)"""
    spec, Ts = spec_batch(rows)
    out, filt, fig = fe.wpe_spectrum(dev(spec), Ts, cfg, return_filters=True, return_figures=True, **kw)
    return out.cpu().numpy(), filt.cpu().numpy(), fig.cpu().numpy(), Ts, spec


# ---- 1. the spectrum call against float64 on the device's own spectrum, and exact pass-through -------------------------------------

@pytest.mark.parametrize("cfg_name", sorted(CONFIGS))
@pytest.mark.parametrize("name, frames", [("small", FRAMES[:-1]), ("small", FRAMES[-1:]), ("prod", (4, 65, 257))])
def test_spectrum_call_is_the_rule(name, frames, cfg_name):
    from megatts2_amd.runtime import Dereverb
    fe = frontend(name)
    F, Fp, S = geometry(name)
    cfg, rc = Dereverb(**CONFIGS[cfg_name]), W.Config(**CONFIGS[cfg_name])
    rows = []
    for T in frames:
        r = rows_of(name, T).copy()
        r[:, 7] = 0.0          # a column of zeros: it passes through, bit for bit
        r[:, F + 7] = 0.0
        rows.append(r)
    out, filt, fig, Ts, spec = wpe_call(fe, rows, cfg)
    worst_d = worst_g = 0.0
    for b, r in enumerate(rows):
        T = int(Ts[b])
        pick = np.arange(F) if T < 4100 else np.unique(np.concatenate([np.arange(0, F, 4), [7, F - 1]]))     # the bins are independent
        ref = W.wpe(W.unpack(r, F)[:, pick], rc)
        got = W.unpack(out[b, :T], F)[:, pick]
        # the counts, on every input: a condition, not a tolerance
        filtered = np.abs(filt[b][pick]).max(axis=1) > 0
        assert np.array_equal(filtered, ref["filtered"]), (name, T, cfg_name)
        if T < 4100:                                                           # every bin was restated: the figures too
            whole = ref["figures"]
            assert fig[b, 3] == T and fig[b, 4] == whole[4] and fig[b, 5] == whole[5] and fig[b, 7] == whole[7]
            assert np.allclose(fig[b, [0, 1, 6]], whole[[0, 1, 6]], rtol=1e-6, atol=0)
        assert not ref["filtered"][list(pick).index(7)]
        # pass-through is exact
        keep = ~ref["filtered"]
        assert same(out[b, :T][:, pick[keep]], r[:, pick[keep]]) and same(out[b, :T][:, F + pick[keep]], r[:, F + pick[keep]])
        if T <= rc.delay:
            assert not ref["filtered"].any() and same(out[b, :T, :2 * F], r[:, :2 * F])
        ed, eg = rel_bins(got, ref["D"]), rel_bins(filt[b][pick].T, ref["g"].T)
        print(f"{name} {cfg_name} T={T}: {int(ref['filtered'].sum())} of {len(pick)} bins filtered, worst bin D {ed.max():.3e} (bar {D_BAR:.1e}), "
              f"g {eg.max():.3e} (bar {G_BAR:.1e})")
        worst_d, worst_g = max(worst_d, ed.max()), max(worst_g, eg.max())
        # out of place: zeros in the pad columns and in the frames at or beyond T
        assert (out[b, :T, 2 * F:] == 0).all() and (out[b, T:] == 0).all()
    assert worst_d <= D_BAR and worst_g <= G_BAR


def test_in_place_is_out_of_place_and_two_runs_agree():
    from megatts2_amd.runtime import Dereverb
    fe = frontend("small")
    F, Fp, S = geometry("small")
    rows = [rows_of("small", T) for T in (257, 14, 65)]
    out, filt, fig, Ts, spec = wpe_call(fe, rows, Dereverb())
    out2, filt2, fig2, _, _ = wpe_call(fe, rows, Dereverb())
    assert same(out, out2) and same(filt, filt2) and same(fig, fig2)
    sd = dev(spec)
    got = fe.wpe_spectrum(sd, Ts, Dereverb(), in_place=True)
    assert got.data_ptr() == sd.data_ptr()
    inplace = sd.cpu().numpy()
    keep = np.ones_like(spec, bool)
    for b, T in enumerate(Ts):
        assert same(inplace[b, :T, :2 * F], out[b, :T, :2 * F])
        keep[b, :T, :2 * F] = False
    assert np.isnan(inplace[keep]).all()                                      # pad columns and spare frames are left as they were
    cplx = torch.complex(dev(rows[0][None, :, :F]), dev(rows[0][None, :, F:2 * F]))
    d = fe.wpe_spectrum(cplx)                                                  # the complex form of the same utterance, alone
    assert same(torch.view_as_real(d)[0].cpu().numpy()[..., 0], out[0, :257, :F])


# ---- 2. ground truth on the device -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name, K, delay, T", [("small", 10, 3, 256), ("small", 10, 3, 4100), ("small", 16, 1, 4100), ("prod", 10, 3, 1024)])
def test_a_known_prediction_filter_is_removed_on_the_device(name, K, delay, T):
    from megatts2_amd.runtime import Dereverb
    fe = frontend(name)
    F = geometry(name)[0]
    g = W.known_filter(K, 0)
    Y, S = W.ar_columns(T, F, g, delay, 0)
    D, filt, fig = fe.wpe_spectrum(dev(W.pack(Y)[None]), None, Dereverb(delay=delay, taps=K), return_filters=True, return_figures=True)
    D = W.unpack(D.cpu().numpy()[0], F)
    before = 10 * np.log10((np.abs(Y - S) ** 2).sum() / (np.abs(S) ** 2).sum())
    after = 10 * np.log10((np.abs(D - S) ** 2).sum() / (np.abs(S) ** 2).sum())
    gerr = float(np.abs(filt.cpu().numpy()[0] - g[None]).max())
    f = fig.cpu().numpy()[0]
    print(f"{name} K {K} delay {delay} T {T}: ||D - S||^2 / ||S||^2 {before:.1f} -> {after:.1f} dB (bar {KNOWN[(K, delay, T)][1]}), max |g^ - g| {gerr:.4f}")
    assert after <= KNOWN[(K, delay, T)][1]
    assert f[3] == T and f[4] == F and f[5] == 0 and f[7] == 3 and 0.15 < f[6] < 0.35        # the largest tap is 0.2, estimated


def device_dereverb(name, x, cfg=None):
    y, lens = frontend(name).dereverb(dev(np.asarray(x, np.float32)[None]), None, cfg)
    return y.cpu().numpy()[0, :lens[0]]


@pytest.mark.parametrize("name, hops, L", sorted(ECHO))
def test_a_hop_aligned_echo_is_removed_on_the_device(name, hops, L):
    a = audio(name)
    for seed in (0, 1):
        x = W.gated_bursts(L, seed)
        y = W.echo(x, hops, a.hop_length)
        d = device_dereverb(name, y)
        ref = W.dereverb(y, a)["y"]
        after, err = W.error_db(d, x), np.linalg.norm(d - ref) / np.linalg.norm(ref)
        print(f"{name} echo at {hops} hops, T {1 + L // a.hop_length}, seed {seed}: {W.error_db(y, x):.2f} -> {after:.2f} dB (bar {ECHO[(name, hops, L)][1]}); "
              f"from the float64 call {err:.2e}")
        assert len(d) == len(ref) and after <= ECHO[(name, hops, L)][1]


@pytest.mark.parametrize("name, T", [("small", 65), ("prod", 45)])
def test_the_call_is_the_composition_of_the_public_calls(name, T):
    """one utterance of at least delay + 4 taps = 43 frames, default configuration (the filter at work): mt2_dereverb gives the bits of
    mt2_stft -> mt2_wpe_spectrum -> mt2_istft"""
    fe, a = frontend(name), audio(name)
    x = dev(W.spectrum_signal(a, T, seed=31)[None])
    spec = fe.stft(x)
    want = fe.istft(fe.wpe_spectrum(spec))
    got, lens = fe.dereverb(x)
    assert lens[0] == (T - 1) * a.hop_length == want.shape[1]
    assert same(got.cpu().numpy(), want.cpu().numpy())
    assert not same(got.cpu().numpy(), fe.istft(spec).cpu().numpy())


# ---- 3. batches and the write set --------------------------------------------------------------------------------------------------

def wav_batch(xs, extra=5):
    """[B, L_max + extra] with NaN at and beyond every utterance's length"""
    lens = np.asarray([len(x) for x in xs], np.int32)
    w = np.full((len(xs), int(lens.max()) + extra), np.nan, np.float32)
    for b, x in enumerate(xs):
        w[b, :len(x)] = x
    return w, lens


def run(fe, xs, cfg=None):
    """one mt2_dereverb call on the ragged batch xs -> (out rows [B, W], out_lens, figures, guards intact)"""
    w, lens = wav_batch(xs)
    B = len(xs)
    hop = fe.audio.hop_length
    W_ = hop * (int(lens.max()) // hop) + 9
    buf = torch.full((B * W_ + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
    out, out_lens, fig = fe.dereverb(dev(w), lens, cfg, return_figures=True, out=buf[:B * W_].view(B, W_))
    h = buf.cpu().numpy()
    return h[:B * W_].reshape(B, W_), out_lens, fig.cpu().numpy(), bool((h[B * W_:] == SENT).all())


@pytest.mark.parametrize("name, Ts", [("small", (257, 30, 4100, 43, 64, 42)), ("prod", (60, 20, 130))])
def test_batch_is_its_utterances_alone(name, Ts):
    """a clip too short for the filter (T < delay + 4 taps = 43) beside long ones; at 4100 frames the batch streams its columns while
    the shorter utterances alone keep theirs in LDS: the same bits"""
    fe, a = frontend(name), audio(name)
    xs = [W.spectrum_signal(a, T, seed=20 + i, tail=(3 * i) % a.hop_length) for i, T in enumerate(Ts)]
    out, lens, fig, ok = run(fe, xs)
    assert ok
    F = geometry(name)[0]
    for b, x in enumerate(xs):
        n = (Ts[b] - 1) * a.hop_length
        assert lens[b] == n and (out[b, n:] == 0).all() and np.isfinite(out[b, :n]).all()
        o1, l1, g1, ok1 = run(fe, [x])
        assert ok1 and l1[0] == n
        assert same(out[b, :n], o1[0, :n]) and same(fig[b], g1[0]), (name, Ts[b])
        short = Ts[b] < 43
        assert fig[b, 3] == Ts[b] and fig[b, 4] == (0 if short else F) and fig[b, 5] == (F if short else 0) and fig[b, 7] == (0 if short else 3)
        if short:                                                              # unfiltered: the two transforms alone
            assert same(out[b, :n], fe.istft(fe.stft(dev(x[None]))).cpu().numpy()[0]) and fig[b, 0] == fig[b, 1]
    again = run(fe, xs)
    assert same(out, again[0]) and same(fig, again[2])


def test_non_finite_input_does_not_fault():
    fe = frontend("small")
    x = W.spectrum_signal(audio("small"), 130).copy()
    x[100], x[700], x[2000] = np.nan, np.inf, -np.inf
    other = W.spectrum_signal(audio("small"), 64, seed=5)
    out, lens, fig, ok = run(fe, [x, other])
    assert ok and lens.tolist() == [129 * 32, 63 * 32]
    alone = run(fe, [other])
    assert same(out[1, :lens[1]], alone[0][0, :lens[1]]) and same(fig[1], alone[2][0])      # the other utterance is untouched by it
    assert np.isfinite(out[1, :lens[1]]).all() and (out[1, lens[1]:] == 0).all()


def test_refusals_launch_nothing_and_leave_the_output():
    from megatts2_amd import runtime as rt
    fe = rt.MelFrontEnd(audio("small"))      # a handle nothing has used: a refused call leaves its arena untouched
    try:
        x = W.spectrum_signal(audio("small"), 64)
        w, lens = wav_batch([x, x[:500]])
        W_ = 32 * (len(x) // 32)
        big = torch.zeros(2 * w.shape[1] + 2 * W_, device="cuda", dtype=torch.float32)
        wd = big[:2 * w.shape[1]].view(2, w.shape[1])
        wd.copy_(dev(w))
        over = big[w.shape[1]:w.shape[1] + 2 * W_].view(2, W_)                 # a buffer that lies across the second row of wav
        out = torch.full((2, W_), float(SENT), device="cuda", dtype=torch.float32)

        def refused(cfg=None, ln=lens, o=out):
            with pytest.raises(rt.NativeError) as e:
                fe.dereverb(wd, ln, cfg, out=o)
            torch.cuda.synchronize()
            assert (out == float(SENT)).all() and fe.workspace_high_water() == 0 and fe.memory()[1] == 0
            return str(e.value)

        assert "delay" in refused(rt.Dereverb(delay=0)) and "taps" in refused(rt.Dereverb(taps=17))
        assert "iterations" in refused(rt.Dereverb(iterations=0)) and "context" in refused(rt.Dereverb(context=5))
        assert "variance_floor" in refused(rt.Dereverb(variance_floor=0.0)) and "loading" in refused(rt.Dereverb(loading=float("nan")))
        assert "fewer frames" in refused(ln=np.asarray([len(x), 95], np.int32))
        assert "Lout_max" in refused(o=out[:, :W_ - 1].contiguous())
        assert "overlapping" in refused(o=over)
        assert same(wd.cpu().numpy(), w)
        spec = torch.full((2, 6, 132), float(SENT), device="cuda", dtype=torch.float32)
        for call in (lambda: fe.wpe_spectrum(spec, [6, 7]), lambda: fe.wpe_spectrum(spec, [0, 6]),
                     lambda: fe.wpe_spectrum(spec, None, rt.Dereverb(taps=0)), lambda: fe.wpe_spectrum(spec, None, rt.Dereverb(delay=9), in_place=True)):
            with pytest.raises(rt.NativeError):
                call()
        torch.cuda.synchronize()
        assert fe.workspace_high_water() == 0 and (spec == float(SENT)).all()
        got, ln = fe.dereverb(wd, lens, out=out)                               # and the accepted call writes it
        assert fe.workspace_high_water() > 0 and ln.tolist() == [W_, 480] and bool((out[1, 480:] == 0).all())
    finally:
        fe.close()


# ---- 4. the surface -------------------------------------------------------------------------------------------------------------------

def peak_normalized(fe, x, ln):
    """mt2_peak_normalize as MelFrontEnd.from_audio calls it -> a new tensor"""
    from megatts2_amd import runtime as rt
    y = torch.empty_like(x)
    rt._check(fe.lib.mt2_peak_normalize(fe.h, rt._stream(), rt._ptr(x), rt._iptr(ln), x.shape[1], x.shape[0], rt._ptr(y)))
    return y


def test_prompt_paths_without_the_argument_keep_their_bits():
    from megatts2_amd import megatts2 as M
    from megatts2_amd.runtime import Denoise, Dereverb
    fe = M._frontend()
    clean = W.gated_bursts(100 * 256 + 7, 2)
    x = W.echo(clean, 4, 256)
    x48 = np.interp(np.arange(3 * len(x)) / 3.0, np.arange(len(x)), x).astype(np.float32)
    for wav, sr in ((x, SR), (x48, 48000)):
        xd = dev(wav[None])
        for dn in (None, Denoise()):
            mel0, n0 = fe.from_audio(xd, sr, trim_db=30.0, denoise=dn)
            mel1, n1 = fe.from_audio(xd, sr, trim_db=30.0, denoise=dn, dereverb=None)
            assert same(mel0.cpu().numpy(), mel1.cpu().numpy()) and n0.tolist() == n1.tolist()
        # with the argument: resample (+ normalise) -> dereverb -> denoise -> normalise -> trim -> mel, by the same primitives
        mel2, n2, nfig, rfig = fe.from_audio(xd, sr, trim_db=30.0, denoise=Denoise(), return_noise=True, dereverb=Dereverb(), return_reverb=True)
        if sr != SR:
            y, ln = fe.resample(xd, sr, normalize=True)
        else:
            ln = np.asarray([len(wav)], np.int32)
            y = peak_normalized(fe, xd, ln)
        r, rl, rf = fe.dereverb(y, ln, Dereverb(), return_figures=True)
        d, dl, df = fe.denoise(r, rl, Denoise(), return_figures=True)
        d = peak_normalized(fe, d, dl)
        t, tl, _ = fe.trim(d, dl, 30.0)
        assert same(fe(t, tl).cpu().numpy(), mel2.cpu().numpy()) and same(df.cpu().numpy(), nfig.cpu().numpy())
        assert same(rf.cpu().numpy(), rfig.cpu().numpy())
    # the echo is reduced in the mel: the de-reverberated prompt's log-mel is nearer the clean one's than the recording's is
    mc = fe.from_audio(dev(clean[None]), SR)[0].cpu().numpy()[0]
    me = fe.from_audio(dev(x[None]), SR)[0].cpu().numpy()[0]
    md, _, fig = fe.from_audio(dev(x[None]), SR, dereverb=Dereverb(), return_reverb=True)
    yn = peak_normalized(fe, dev(x[None]), np.asarray([len(x)], np.int32))      # alone: dereverb -> normalise -> mel
    r, rl = fe.dereverb(yn, None, Dereverb())
    assert same(fe(peak_normalized(fe, r, rl), rl).cpu().numpy(), md.cpu().numpy())
    md = md.cpu().numpy()[0]
    n = md.shape[0]

    def mel_error(m):
        """the mel magnitudes against the clean prompt's, after the best common scale (each prompt is peak-normalised on its own)"""
        a, c = np.exp(m[:n].astype(np.float64)), np.exp(mc[:n].astype(np.float64))
        return float(np.linalg.norm(a * ((a * c).sum() / (a * a).sum()) - c) / np.linalg.norm(c))

    e_before, e_after = mel_error(me), mel_error(md)
    print(f"mel magnitude error against the clean prompt: {e_before:.3f} with the echo, {e_after:.3f} de-reverberated; power "
          f"{fig.cpu().numpy()[0, 2]:.2f} dB")
    assert e_after < 0.6 * e_before and fig.cpu().numpy()[0, 2] < -0.3
    m0 = M.extract_mel_spec(torch.from_numpy(x))
    assert same(m0.cpu().numpy(), M.extract_mel_spec(torch.from_numpy(x), dereverb=None).cpu().numpy())
    m1 = M.extract_mel_spec(torch.from_numpy(x), dereverb=Dereverb())
    assert m1.shape == (80, 101) and not same(m1.cpu().numpy(), m0.cpu().numpy())
    out, st = M.dereverb_audio(x)
    assert same(out, fe.dereverb(dev(x[None]))[0].cpu().numpy()[0]) and st["frames"][0] == 101 and st["bins_filtered"][0] == 513
    out48, st48 = M.dereverb_audio(x48, 48000)                                 # another rate: resampled first, the result at 16 kHz
    y16, l16 = fe.resample(dev(x48[None]), 48000)
    assert same(out48, fe.dereverb(y16, l16)[0].cpu().numpy()[0]) and abs(len(out48) - len(out)) <= 256


def test_forward_dereverberates_every_prompt_file(tmp_path):
    from megatts2_amd import audio_io, megatts2 as M
    from megatts2_amd.runtime import Denoise, Dereverb
    (g, p, a, _), (sd_g, sd_p, sd_a, _) = synth_models("tiny")
    tts = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)))
    wavs = tmp_path / "prompts"
    wavs.mkdir()
    x = W.echo(W.gated_bursts(60 * 256, 4), 4, 256)
    x48 = np.interp(np.arange(3 * len(x)) / 3.0, np.arange(len(x)), x).astype(np.float32)
    audio_io.write_wav(str(wavs / "a.wav"), x, SR)
    audio_io.write_wav(str(wavs / "b.wav"), x48, 48000)
    phone = np.random.default_rng(13).integers(0, g.mrte.phone_vocab_size, 6)
    mel0, lens0, aux0 = tts.forward(str(wavs), phone_tokens=phone, out_path=None)
    mel1, lens1, aux1 = tts.forward(str(wavs), phone_tokens=phone, out_path=None, dereverb=None)
    assert torch.equal(mel0, mel1) and "prompt_reverb" not in aux0 and "prompt_reverb" not in aux1
    mel2, lens2, aux2 = tts.forward(str(wavs), phone_tokens=phone, out_path=None, dereverb=Dereverb())
    fe = M._frontend()
    rev = aux2["prompt_reverb"]
    assert len(rev) == 2 and all(set(n) == set(W.FIELDS) for n in rev) and "prompt_noise" not in aux2
    for (path, n) in zip(("a.wav", "b.wav"), rev):
        y, sr = audio_io.read_wav(str(wavs / path))
        fig = fe.from_audio(dev(y[None]), sr, dereverb=Dereverb(), return_reverb=True)[2].cpu().numpy()[0]
        assert [n[k] for k in W.FIELDS] == fig.tolist() and n["frames"] == 61 and n["bins_filtered"] == 513 and n["reduction_db"] < 0.0
    assert mel2.shape[0] == mel0.shape[0] and np.isfinite(mel2.cpu().numpy()).all()
    _, _, aux3 = tts.forward(str(wavs), phone_tokens=phone, out_path=None, dereverb=Dereverb(), denoise=Denoise())
    assert len(aux3["prompt_reverb"]) == 2 and len(aux3["prompt_noise"]) == 2
