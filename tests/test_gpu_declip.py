"""Declipping on the GPU (csrc/declip.hip) against its float64 restatement (tests/declip_ref.py), on the same f32 input.

mt2_clip_detect is held bit for bit: f32 comparisons and integer counts.  mt2_declip: `iters` equal on every frame that the RESTATEMENT
does not report as a near-tie (the relative gap between the k-th and (k + 1)-th |v|^2, or the relative distance of |d| from eps |F|, under
1e-9 in some iteration; at most 2 % of frames, and the seeds used here have none), and the output's relative L2 against the float64
output under a bar derived here: 2^-24, the one f32 rounding, plus 16 x the difference between the restatement run with numpy's FFT and
with the kernel-order FFT (1e-15 .. 5e-15: the bar is 5.96e-8 at every size).  Observed on an MI355X: see the figures the tests print."""
import math

import numpy as np
import pytest

import declip_ref as D

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

NEAR_TIE_SHARE = 0.02
# (N, theta, seed, rule parameters): N 256 at three settings, one case each at 1024 and 2048
CASES = [(256, 0.3, 1, {}), (256, 0.6, 1, {}), (256, 0.3, 0, {"step": 4, "every": 2}), (256, 0.6, 0, {"step": 4, "every": 2}),
         (256, 0.3, 1, {"max_iter": 3}), (256, 0.6, 1, {"max_iter": 3}), (1024, 0.6, 1, {}), (2048, 0.3, 0, {})]


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    h = MelFrontEnd()
    yield h
    h.close()


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def bits(a):
    return np.asarray(a, np.float32).view(np.int32)


def batch(xs, fill=np.nan, extra=5):
    lens = np.asarray([len(x) for x in xs], np.int32)
    w = np.full((len(xs), int(lens.max()) + extra), fill, np.float32)
    for b, x in enumerate(xs):
        w[b, :len(x)] = x
    return w, lens


def run(fe, rt, xs, **kw):
    """-> (out numpy [B, L] over an out buffer filled with -7.5, figures [B, 8], iters [B, T]) of one ragged call"""
    w, lens = batch(xs)
    out = torch.full(w.shape, -7.5, device="cuda", dtype=torch.float32)
    o, fig, it = fe.declip(dev(w), lens, rt.Declip(**kw), return_figures=True, return_iters=True, out=out)
    return o.cpu().numpy(), fig.cpu().numpy(), it.cpu().numpy()


# ---- detection -----------------------------------------------------------------------------------------------------------------------

def test_clip_detect_is_bit_equal_to_numpy(fe, rt):
    x = D.make_signal(256, 4, length=16001)
    sigs = {1: np.asarray([0.25], np.float32), 63: D.clip(x[:63], 0.2), 64: D.clip(x[100:164], 0.2), 65: x[:65].copy(),
            1000: np.minimum(x[:1000], np.float32(0.3)).astype(np.float32), 16001: D.clip(x, 0.4)}
    nan = D.clip(x[:1000], 0.3)
    nan[17] = np.nan
    xs = [sigs[1], sigs[63], nan, sigs[64], sigs[65], sigs[1000], sigs[16001]]
    w, lens = batch(xs)
    for tol in (0.0, 1e-3):
        rule = D.Rule(frame=256, tol=tol)
        fig = fe.clip_detect(dev(w), lens, rt.Declip(frame=256, tol=tol)).cpu().numpy()
        want = np.stack([D.detect_figures(x, rule) for x in xs])
        print(tol, fig[:, :4].tolist())
        assert np.array_equal(fig.view(np.int64)[~np.isnan(want)], want.view(np.int64)[~np.isnan(want)])
        assert np.isnan(fig[2, 1]) and np.isnan(fig[2, 2]) and fig[2, 0] == 0
        assert fig[5, 0] == 1 and fig[5, 3] > 0 and fig[4, 0] == 0 and fig[6, 0] == 1      # one side only; unclipped; both
        alone = np.stack([fe.clip_detect(dev(x[None]), None, rt.Declip(frame=256, tol=tol)).cpu().numpy()[0] for x in xs])
        assert np.array_equal(alone.view(np.int64), fig.view(np.int64))         # the NaN utterance's neighbours keep their bits


# ---- the rule ------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N, theta, seed, kw", CASES)
def test_declip_against_the_restatement(fe, rt, N, theta, seed, kw):
    x = D.make_signal(N, seed)
    y = D.clip(x, theta)
    rule = D.Rule(frame=N, **kw)
    ref, refk = D.declip(y, rule), D.declip(y, rule, fft="kernel")
    fft_diff = np.linalg.norm(ref["out64"] - refk["out64"]) / np.linalg.norm(ref["out64"])
    bar = 2.0 ** -24 + 16.0 * fft_diff
    exempt = ref["near_tie"] | refk["near_tie"]
    assert not exempt.any()                                                    # the seeds were chosen so: checked without a GPU as well
    out, fig, it = run(fe, rt, [y], frame=N, **kw)
    out, fig, it = out[0, :len(y)], fig[0], it[0]
    err = np.linalg.norm(out - ref["out64"]) / np.linalg.norm(ref["out64"])
    print(f"N {N} theta {theta} {kw}: relative L2 {err:.3e} (bar {bar:.3e}, transforms {fft_diff:.2e}), frames iterated {int(fig[4])}, mean "
          f"{fig[5]:.1f}, most {int(fig[6])}, SDR {D.sdr_db(x, y, N):.2f} -> {D.sdr_db(x, out, N):.2f} dB (restatement {D.sdr_db(x, ref['out'], N):.2f})")
    assert exempt.mean() <= NEAR_TIE_SHARE
    assert np.array_equal(it[~exempt], ref["iters"][~exempt])
    assert err < bar
    assert np.array_equal(fig[:4], ref["figures"][:4]) and np.array_equal(fig[4:7], ref["figures"][4:7])
    assert abs(fig[7] - ref["figures"][7]) < 1e-6
    H, L = ref["det"]["H"], ref["det"]["L"]
    assert np.array_equal(bits(out[~(H | L)]), bits(y[~(H | L)]))
    assert (out[H] >= y[H]).all() and (out[L] <= y[L]).all()


@pytest.mark.parametrize("N, theta", sorted(__import__("test_declip_host").TRUTH))
def test_ground_truth_on_the_device(fe, rt, N, theta):
    """the host tests' SDRs, read on the device inside the same bars"""
    from test_declip_host import RISE, SEEDS, TRUTH
    xs = [D.make_signal(N, s) for s in SEEDS]
    ys = [D.clip(x, theta) for x in xs]
    out, fig, _ = run(fe, rt, ys, frame=N)
    before = np.array([D.sdr_db(x, y, N) for x, y in zip(xs, ys)])
    after = np.array([D.sdr_db(x, o[:len(x)], N) for x, o in zip(xs, out)])
    print(f"N {N} theta {theta}: before {before.min():.2f} .. {before.max():.2f} dB, after {after.min():.2f} .. {after.max():.2f} dB "
          f"(bar {TRUTH[(N, theta)][1]}), rise {(after - before).min():.2f} dB at least")
    assert after.min() >= TRUTH[(N, theta)][1] and (after - before).min() >= RISE and (fig[:, 0] == 1).all()


def test_what_passes_through_bit_for_bit_and_the_square_wave(fe, rt):
    x = D.make_signal(256, 0)
    nan = x.copy()
    nan[100] = np.nan
    square = np.where((np.arange(256 + 24 * 64) // 40) % 2 == 0, 0.5, -0.5).astype(np.float32)
    xs = [x, nan, np.zeros(700, np.float32), square]
    out, fig, it = run(fe, rt, xs, frame=256)
    for b, y in enumerate(xs):
        assert np.array_equal(bits(out[b, :len(y)]), bits(y)), b
        assert (it[b] == 0).all() and (bits(out[b, len(y):]) == bits(np.float32(-7.5))).all()
    assert fig[:, 0].tolist() == [0, 0, 0, 1] and fig[3, 3] == 1.0 and np.isnan(fig[1, 1]) and (fig[:, 4:] == 0).all()


def test_an_explicit_level_reproduces_the_detected_one(fe, rt):
    y = D.clip(D.make_signal(256, 2), 0.6)
    a, b = run(fe, rt, [y], frame=256), run(fe, rt, [y], frame=256, level=float(np.float32(0.6)))
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip(a, b))


def test_a_ragged_batch_is_its_utterances_alone_and_two_runs_agree(fe, rt):
    x = D.make_signal(256, 6)
    xs = [D.clip(x, 0.3), x[:900].copy(), D.clip(x[200:264], 0.2), D.clip(x[:1111], 0.5)]      # clipped, unclipped, one hop long, clipped
    out, fig, it = run(fe, rt, xs, frame=256)
    again = run(fe, rt, xs, frame=256)
    assert all(np.array_equal(p.view(np.uint8), q.view(np.uint8)) for p, q in zip((out, fig, it), again))
    assert fig[:, 0].tolist() == [1, 0, 1, 1] and (it[0] > 0).any()
    for b, y in enumerate(xs):
        o1, f1, i1 = run(fe, rt, [y], frame=256)
        T = D.frames_of(len(y), 256)
        assert np.array_equal(bits(o1[0, :len(y)]), bits(out[b, :len(y)])), b
        assert np.array_equal(f1[0].view(np.int64), fig[b].view(np.int64)), b
        assert np.array_equal(i1[0, :T], it[b, :T]) and (it[b, T:] == 0).all(), b
        # NaN beyond lens[b] is never read; the output beyond it is left untouched
        assert (bits(out[b, len(y):]) == bits(np.float32(-7.5))).all()


def test_guard_words_stay_intact(fe, rt):
    y = D.clip(D.make_signal(256, 7), 0.4)
    L, T = len(y), D.frames_of(len(y), 256)
    G = 64
    wav = torch.full((L + 2 * G,), float("nan"), device="cuda", dtype=torch.float32)
    wav[G:G + L] = dev(y)
    out = torch.full((L + 2 * G,), 3.25, device="cuda", dtype=torch.float32)
    fig = torch.full((8 + 2 * G,), 3.25, device="cuda", dtype=torch.float64)
    it = torch.full((T + 2 * G,), -9, device="cuda", dtype=torch.int32)
    dc = rt.Declip(frame=256).c_struct()
    import ctypes as C
    lens = np.asarray([L], np.int32)
    p = lambda t, off, size: C.c_void_p(t.data_ptr() + off * size)
    rt._check(fe.lib.mt2_declip(fe.h, rt._stream(), C.byref(dc), p(wav, G, 4), rt._iptr(lens), L, 1, p(out, G, 4), L, p(fig, G, 8), p(it, G, 4), T))
    torch.cuda.synchronize()
    o, f, i = out.cpu().numpy(), fig.cpu().numpy(), it.cpu().numpy()
    assert (o[:G] == 3.25).all() and (o[G + L:] == 3.25).all() and (f[:G] == 3.25).all() and (f[G + 8:] == 3.25).all()
    assert (i[:G] == -9).all() and (i[G + T:] == -9).all() and (i[G:G + T] >= 0).all() and f[G] == 1.0
    assert np.array_equal(bits(o[G:G + L]), bits(run(fe, rt, [y], frame=256)[0][0, :L]))


def test_refusals_leave_the_outputs_and_the_arena(fe, rt):
    y = D.clip(D.make_signal(256, 7), 0.4)
    w = dev(y[None])
    fe.declip(w, None, rt.Declip(frame=256))                                    # the arena exists
    torch.cuda.synchronize()
    rt._workspace_fill(fe.lib, fe.h, 0x5A)
    before = fe.workspace_high_water()
    out = torch.full_like(w, -7.5)
    for bad in (dict(frame=300), dict(tol=0.5), dict(eps=0.0), dict(level=-1.0), dict(step=0), dict(every=99), dict(min_count=0), dict(max_iter=-1)):
        with pytest.raises(rt.NativeError):
            fe.declip(w, None, rt.Declip(**{"frame": 256, **bad}), return_figures=True, return_iters=True, out=out)
        with pytest.raises(rt.NativeError):
            fe.clip_detect(w, None, rt.Declip(**{"frame": 256, **bad}))
    with pytest.raises(rt.NativeError):
        fe.declip(w, np.asarray([len(y) + 1]), rt.Declip(frame=256), out=out)
    with pytest.raises(rt.NativeError):
        fe.declip(w, None, rt.Declip(frame=256), out=w)                         # in place is not offered
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -7.5).all() and fe.workspace_high_water() == before
    peek = rt._workspace_peek(fe.lib, fe.h, 0, min(before, 1 << 16))
    assert (np.frombuffer(peek, np.uint8) == 0x5A).all()


# ---- the application layer -----------------------------------------------------------------------------------------------------------

def test_the_front_end_without_the_argument_keeps_its_bits(fe, rt):
    from megatts2_amd import megatts2 as M
    x = D.make_signal(1024, 2, sr=48000, length=48000)
    w = dev(x[None])
    for kw in ({}, {"denoise": rt.Denoise()}, {"dereverb": rt.Dereverb()}, {"denoise": rt.Denoise(), "dereverb": rt.Dereverb()}):
        a, b = fe.from_audio(w, 48000, **kw), fe.from_audio(w, 48000, declip=None, return_clipping=False, **kw)
        assert torch.equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        c = fe.from_audio(w, 48000, declip=rt.Declip(), return_clipping=True, **kw)      # unclipped: passed through bit for bit
        assert torch.equal(a[0], c[0]) and c[-1][0, 0].item() == 0.0
    x16 = D.make_signal(1024, 2, length=16000)
    for kw in ({}, {"denoise": rt.Denoise()}, {"dereverb": rt.Dereverb()}):
        assert torch.equal(M.extract_mel_spec(x16, **kw), M.extract_mel_spec(x16, declip=None, **kw))
        assert torch.equal(M.extract_mel_spec(x16, **kw), M.extract_mel_spec(x16, declip=rt.Declip(), **kw))


def test_from_audio_declip_brings_the_mel_nearer_the_clean_one(fe, rt):
    """the clipped test signal at 48 kHz: the mel of from_audio(declip=) against the clean signal's, beside the mel without it"""
    x = D.make_signal(1024, 3, sr=48000, length=48000)
    y = D.clip(x, 0.3)
    clean = fe.from_audio(dev(x[None]), 48000)[0]
    plain = fe.from_audio(dev(y[None]), 48000)[0]
    mel, lens, fig = fe.from_audio(dev(y[None]), 48000, declip=rt.Declip(), return_clipping=True)
    d_plain, d_declip = float((plain - clean).abs().mean()), float((mel - clean).abs().mean())
    print(f"mean |log-mel - clean|: clipped {d_plain:.4f}, declipped {d_declip:.4f};  figures {fig[0].cpu().numpy().tolist()}")
    assert fig[0, 0].item() == 1.0 and d_declip < d_plain
    from megatts2_amd import megatts2 as M
    out, res = M.declip_audio(y)
    assert res["clipped"][0] == 1.0 and out.shape == y.shape and res["iters"].shape[1] == rt.Declip().frames(len(y))
    assert np.array_equal(bits(out), bits(fe.declip(dev(y[None])).cpu().numpy()[0]))
