"""The Griffin-Lim vocoder on the GPU (csrc/griffinlim.hip: mt2_stft, mt2_istft, mt2_mel_to_linear, mt2_griffin_lim) against the
restatement of its rule (tests/griffinlim_ref.py), one launch at a time where the row-op table allows it, then whole runs.

Conventions: outputs are wider than needed, pre-filled with a sentinel and followed by guard words; mel frames at or beyond an
utterance's length are NaN (a read of one poisons the output).  Two audio configurations: production (1024 / 256 / 80 mels) and a
small one (64 / 16 / 8 mels, 16 kHz, f_max 8000), so that no constant is hard-coded.  Frame counts 4 (the minimum), 5 (the first with
an interior sample), 37, 65, 130 (around the 64-row GEMM tile) and the ragged batch {4, 37, 65, 130}.

Bars.  The engine's existing bar for a convolution (tests/test_gpu_gemm_groups.py), 3e-6 relative L2, holds the STFT, the inverse
STFT and mel -> linear to the float64 restatement.  The measured bars - the round trip, and the whole run's spectral convergence and
waveform - are 4 x the larger of the value observed on an MI355X and the restatement's own f32 run (constants below, with what was
observed)."""
import functools

import numpy as np
import pytest

import griffinlim_ref as G
from conftest import synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = np.float32(-777.25)
GUARD = 64
U = 2.0 ** -24
CONV_BAR = 3e-6
FRAMES = (4, 5, 37, 65, 130)
RAGGED = (4, 37, 65, 130)
# Observed on an MI355X (this file's own prints); in brackets the restatement's own f32 run on the same cases - every transform one f32
# dot per output value, as the rule states it (its single STFT / inverse STFT sit 1.5e-7 .. 3.1e-7 from float64, like the kernels'):
#   round trip istft(stft(x)) vs x, relative L2: production 3.5e-7 .. 5.0e-7, small 1.3e-7 .. 1.5e-7             -> bar 4 x 5.0e-7
#   whole run, n_iter = 4, all 20 cases: max_k |sc_gpu - sc_ref| 5.9e-9 .. 1.95e-7 (f32 restatement 7.7e-9 .. 2.85e-7) -> 4 x 2.85e-7
#                                        waveform relative L2 1.9e-7 .. 1.01e-5 (f32 restatement 1.2e-7 .. 1.9e-5)    -> 4 x 1.9e-5
# (single launches: phase init 0.43 of 2^-20; phase update 0.36 of its component bound, 0.20 of its residual bound; STFT 0.9e-7 ..
# 3.0e-7, inverse STFT 1.8e-7 .. 7.9e-7, mel -> linear 7e-8 .. 1e-7 relative L2)
RT_OBSERVED = 5.0e-7
SC_BAR = 4 * 2.85e-7
WAV_BAR = 4 * 1.9e-5


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def audio(name):
    from megatts2_amd.config import AudioConfig
    if name == "prod":
        return AudioConfig()
    return AudioConfig(sample_rate=16000, n_fft=64, hop_length=16, win_length=64, n_mels=8, f_min=0.0, f_max=8000.0)


@functools.lru_cache(maxsize=None)
def frontend(name):
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd(audio(name))


@functools.lru_cache(maxsize=None)
def signal(name, T, kind=None):
    a = audio(name)
    L = (T - 1) * a.hop_length
    kind = kind or ("tone" if T in (4, 37, 130) else "vib")
    return G.two_tone_noise(L, a.sample_rate, seed=T) if kind == "tone" else G.vibrato_stack(L, a.sample_rate)


@functools.lru_cache(maxsize=None)
def mel_of(name, T, kind=None):
    return G.log_mel(signal(name, T, kind), audio(name))


@functools.lru_cache(maxsize=None)
def reference(name, T, n_iter, momentum, seed, f32=False, kind=None):
    """(x, sc [n_iter + 1], A, resid) of the restatement; computed once and shared"""
    x, resid, A = G.griffin_lim(mel_of(name, T, kind), seed, audio(name), n_iter, momentum, np.float32 if f32 else np.float64)
    return x, G.spectral_convergence(resid, A), A, resid


def rel_l2(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / np.linalg.norm(b))


def run_gl(name, mels, seeds, n_iter, momentum, T_max=None, slots=None, B=None, resid=True, fe=None):
    """Griffin-Lim of the log-mels `mels` (list of [T_b, n_mels]) as one batch; slots[i] = the batch row of mels[i] (other rows are
    filled with the first utterance).  -> (wav [B, Lw], resid [B, n_iter + 1, T_max] or None, guards_ok)"""
    fe, a = fe or frontend(name), audio(name)
    slots = list(range(len(mels))) if slots is None else slots
    B = B or (max(slots) + 1)
    Ts = np.full(B, mels[0].shape[0], np.int32)
    T_max = T_max or max(m.shape[0] for m in mels) + 3
    mel = np.full((B, T_max, a.n_mels), np.nan, np.float32)
    sd = np.zeros(B, np.uint64)
    mel[:, :mels[0].shape[0]] = mels[0]
    sd[:] = seeds[0]
    for i, s in enumerate(slots):
        Ts[s] = mels[i].shape[0]
        mel[s] = np.nan
        mel[s, :Ts[s]] = mels[i]
        sd[s] = seeds[i]
    Lw = (int(Ts.max()) - 1) * a.hop_length + 9
    wbuf = torch.full((B * Lw + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
    rn = B * (n_iter + 1) * T_max
    rbuf = torch.full((rn + GUARD,), float(SENT), device="cuda", dtype=torch.float32) if resid else None
    fe.griffin_lim(dev(mel), Ts, n_iter=n_iter, momentum=momentum, seeds=sd, out=wbuf[:B * Lw].view(B, Lw),
                   resid_out=rbuf[:rn].view(B, n_iter + 1, T_max) if resid else None)
    w = wbuf.cpu().numpy()
    ok = bool((w[B * Lw:] == SENT).all())
    r = None
    if resid:
        r = rbuf.cpu().numpy()
        ok = ok and bool((r[rn:] == SENT).all())
        r = r[:rn].reshape(B, n_iter + 1, T_max)
    return w[:B * Lw].reshape(B, Lw), r, ok


def gpu_stats(name, T, wav_row, resid_row, n_iter, momentum, seed, kind=None):
    """(max_k |sc_gpu - sc_ref|, waveform relative L2, the same two for the restatement's f32 run)"""
    x, sc, A, _ = reference(name, T, n_iter, momentum, seed, False, kind)
    x32, sc32, _, _ = reference(name, T, n_iter, momentum, seed, True, kind)
    L = (T - 1) * audio(name).hop_length
    sc_gpu = G.spectral_convergence(resid_row[:, :T], A)
    return float(np.abs(sc_gpu - sc).max()), rel_l2(wav_row[:L], x), float(np.abs(sc32 - sc).max()), rel_l2(x32, x)


# ---- 1. phase init, one launch ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["prod", "small"])
def test_phase_init_one_launch(name):
    """every component within 2^-20 of float64 cos / sin(2 pi u) for A = 1 (rounding 2 pi u in f32 costs at most 2^-21, cosf / sinf a
    few ulp), pad columns zero, guards intact, and a batch's rows equal the utterance's alone bit for bit"""
    from megatts2_amd import runtime as rt
    a = audio(name)
    F = a.n_fft // 2 + 1
    lds = (2 * F + 3) & ~3
    Ts, seeds = (5, 37), np.asarray([11, 2 ** 40 + 5], np.uint64)
    row_b = np.concatenate([np.full(t, b, np.int32) for b, t in enumerate(Ts)])
    row_t = np.concatenate([np.arange(t, dtype=np.int32) for t in Ts])
    R = row_b.size

    def launch(rb, rt_, sd):
        n = rb.size
        buf = torch.full((n * lds + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
        rt.op_gl_phase_init(None, 0, dev(rb), dev(rt_), dev(sd.view(np.int64)), buf, lds, F, n)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        assert (got[n * lds:] == SENT).all()
        return got[:n * lds].reshape(n, lds)

    S = launch(row_b, row_t, seeds)
    assert (S[:, 2 * F:] == 0).all()
    for b, t in enumerate(Ts):
        theta = 2.0 * np.pi * G.phase_uniform(seeds[b], t, F)
        rows = S[row_b == b]
        err = max(np.abs(rows[:, :F] - np.cos(theta)).max(), np.abs(rows[:, F:2 * F] - np.sin(theta)).max())
        print(f"phase_init {name} T={t}: max error {err / 2.0 ** -20:.3f} x 2^-20")
        assert err <= 2.0 ** -20
        alone = launch(np.zeros(t, np.int32), np.arange(t, dtype=np.int32), seeds[b:b + 1])
        assert np.array_equal(alone, rows)
    assert R == sum(Ts)


# ---- 2. STFT and inverse STFT, one call each ------------------------------------------------------------------------------------

def stft_batch(name, Ts):
    fe, a = frontend(name), audio(name)
    xs = [signal(name, T) for T in Ts]
    lens = np.asarray([x.size for x in xs], np.int32)
    wav = np.full((len(Ts), int(lens.max()) + 5), np.nan, np.float32)
    for b, x in enumerate(xs):
        wav[b, :x.size] = x
    return xs, fe.stft(dev(wav), lens).cpu().numpy()


@pytest.mark.parametrize("name", ["prod", "small"])
@pytest.mark.parametrize("Ts", [(T,) for T in FRAMES] + [RAGGED])
def test_stft_against_float64(name, Ts):
    xs, S = stft_batch(name, Ts)
    for b, (T, x) in enumerate(zip(Ts, xs)):
        ref = G.stft(x, audio(name))
        assert ref.shape[0] == T
        err = rel_l2(np.concatenate([S[b, :T].real, S[b, :T].imag]), np.concatenate([ref.real, ref.imag]))
        print(f"stft {name} T={T}: rel L2 {err:.3g}")
        assert err <= CONV_BAR
        assert (S[b, T:] == 0).all()


def istft_batch(name, specs, extra=7):
    """inverse STFT of the float64 spectra `specs` (rounded to complex64) as one batch, NaN padding frames, sentinel-filled output"""
    fe, a = frontend(name), audio(name)
    Ts = np.asarray([s.shape[0] for s in specs], np.int32)
    B, F = len(specs), a.n_fft // 2 + 1
    S = np.full((B, int(Ts.max()) + 2, F), np.nan + 1j * np.nan, np.complex64)
    for b, s in enumerate(specs):
        S[b, :Ts[b]] = s
    Lw = (int(Ts.max()) - 1) * a.hop_length + extra
    buf = torch.full((B * Lw + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
    fe.istft(dev(S), Ts, out=buf[:B * Lw].view(B, Lw))
    got = buf.cpu().numpy()
    assert (got[B * Lw:] == SENT).all()
    return got[:B * Lw].reshape(B, Lw)


@pytest.mark.parametrize("name", ["prod", "small"])
@pytest.mark.parametrize("Ts", [(T,) for T in FRAMES] + [RAGGED])
def test_istft_against_float64(name, Ts):
    """a random-phase spectrum (not a consistent one: the overlap-add has to do real work) against the restatement; at T = 4 and 5
    every sample lies in the edge region, where e differs from its interior value: held per sample there"""
    a = audio(name)
    rng = np.random.default_rng(sum(Ts))
    specs = []
    for T in Ts:
        S = G.stft(signal(name, T), a)
        specs.append((np.abs(S) * np.exp(2j * np.pi * rng.random(S.shape))).astype(np.complex64))
    out = istft_batch(name, specs)
    for b, T in enumerate(Ts):
        L = (T - 1) * a.hop_length
        ref = G.istft(specs[b].astype(np.complex128), a)
        err = rel_l2(out[b, :L], ref)
        print(f"istft {name} T={T}: rel L2 {err:.3g}")
        assert err <= CONV_BAR
        assert (out[b, L:] == 0).all()
        if T <= 5:
            assert np.abs(out[b, :L] - ref).max() <= CONV_BAR * np.abs(ref).max()
            wrong = G.istft(specs[b].astype(np.complex128), a, edge_interior=True)      # the mutation this test must catch
            assert np.abs(wrong - ref).max() > 100 * CONV_BAR * np.abs(ref).max()


@pytest.mark.parametrize("name", ["prod", "small"])
def test_round_trip(name):
    """istft(stft(x)) against x itself, no reference involved; each half is held to 3e-6, the observed round trip is far below"""
    xs, S = stft_batch(name, RAGGED)
    out = istft_batch(name, [S[b, :T] for b, T in enumerate(RAGGED)])
    for b, (T, x) in enumerate(zip(RAGGED, xs)):
        err = rel_l2(out[b, :x.size], x)
        print(f"round trip {name} T={T}: rel L2 {err:.3g}")
        assert err <= 4 * RT_OBSERVED


# ---- 3. phase update, one launch ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["prod", "small"])
@pytest.mark.parametrize("momentum", [0.0, 0.99])
def test_phase_update_one_launch(name, momentum):
    """S within 8 * 2^-24 * A * (|R| + c |Rprev|) / |D| of float64 per component (six roundings and the cancellation of the
    difference), Rprev out bit-equal to R in, and the residual rows within
        2^-24 * (4 sum |d_f| |R_f| + (ceil(F / 64) + 8) sum d_f^2),  d_f = |R_f| - A_f:
    |R| carries 2 u |R| (two squares, a sum, a root), so d errs by 2 u |R| + u |d| and d^2 by 4 u |d| |R| + 3 u d^2; a lane adds
    ceil(F / 64) terms in order and the butterfly adds 6 levels: (ceil(F / 64) + 5) u sum d^2."""
    from megatts2_amd import runtime as rt
    a = audio(name)
    F = a.n_fft // 2 + 1
    lds, lda, rows = (2 * F + 3) & ~3, (F + 3) & ~3, 70
    rng = np.random.default_rng(int(momentum * 100) + F)
    R = np.zeros((rows, lds), np.float32)
    Rp = np.zeros((rows, lds), np.float32)
    R[:, :2 * F] = rng.standard_normal((rows, 2 * F)) * rng.uniform(0.1, 30.0, (rows, 1))
    Rp[:, :2 * F] = R[:, :2 * F] * rng.uniform(0.7, 1.3, (rows, 2 * F)) + 0.05 * rng.standard_normal((rows, 2 * F))
    A = np.zeros((rows, lda), np.float32)
    A[:, :F] = np.abs(rng.standard_normal((rows, F))) * 5.0
    c = G.momentum_c(momentum)
    rmap = rng.permutation(rows).astype(np.int32)
    Sbuf = torch.full((rows * lds + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
    rbuf = torch.full((rows + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
    Rp_d = dev(Rp)
    rt.op_gl_phase_update(dev(R), Rp_d, dev(A), lda, Sbuf, lds, F, float(c), rbuf, dev(rmap), rows, 1)
    torch.cuda.synchronize()
    S, res = Sbuf.cpu().numpy(), rbuf.cpu().numpy()
    assert (S[rows * lds:] == SENT).all() and (res[rows:] == SENT).all()
    S = S[:rows * lds].reshape(rows, lds)
    assert np.array_equal(Rp_d.cpu().numpy()[:, :2 * F], R[:, :2 * F])
    Rc = R[:, :F].astype(np.float64) + 1j * R[:, F:2 * F]
    Rpc = Rp[:, :F].astype(np.float64) + 1j * Rp[:, F:2 * F]
    A64 = A[:, :F].astype(np.float64)
    want = G.phase_update(Rc, Rpc, A64, c)
    D = Rc - float(c) * Rpc
    bound = 8 * U * A64 * (np.abs(Rc) + float(c) * np.abs(Rpc)) / np.abs(D)
    worst = max((np.abs(S[:, :F] - want.real) / bound).max(), (np.abs(S[:, F:2 * F] - want.imag) / bound).max())
    print(f"phase_update {name} momentum={momentum}: worst component at {worst:.3f} of its bound")
    assert worst <= 1.0
    if momentum > 0:      # the mutation "Rprev updated before D is formed" is far outside the bound
        wrong = G.phase_update(Rc, Rpc, A64, c, rprev_first=True)
        assert (np.abs(wrong.real - want.real) / bound).max() > 100
    d = np.abs(Rc) - A64
    rbound = U * (4 * (np.abs(d) * np.abs(Rc)).sum(1) + (-(-F // 64) + 8) * (d * d).sum(1))
    rworst = (np.abs(res[:rows][rmap] - G.residual(Rc, A64)) / rbound).max()
    print(f"phase_update {name} momentum={momentum}: worst residual at {rworst:.3f} of its bound")
    assert rworst <= 1.0


# ---- 4. mel -> linear -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["prod", "small"])
def test_mel_to_linear(name):
    fe, a = frontend(name), audio(name)
    Ts = RAGGED
    mel = np.full((len(Ts), max(Ts) + 2, a.n_mels), np.nan, np.float32)
    for b, T in enumerate(Ts):
        mel[b, :T] = mel_of(name, T)
    mel[1, 3] = np.log(a.clip)                       # a frame at the compression floor
    got = fe.mel_to_linear(dev(mel), np.asarray(Ts, np.int32)).cpu().numpy()
    assert np.isfinite(got).all()
    P = G.pinv_cholesky(G.filterbank(a)).astype(np.float32).astype(np.float64)
    for b, T in enumerate(Ts):
        raw = np.exp(mel[b, :T].astype(np.float64)) @ P.T
        ref = np.maximum(raw, 0.0)
        err = rel_l2(got[b, :T], ref)
        print(f"mel_to_linear {name} T={T}: rel L2 {err:.3g}, {int((raw < 0).sum())} clamped")
        assert err <= CONV_BAR
        assert (got[b, :T][raw < -1e-6 * ref.max()] == 0).all() and (got[b, :T] >= 0).all()
        assert (got[b, T:] == 0).all()


# ---- 5. whole run against the restatement -------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["prod", "small"])
@pytest.mark.parametrize("momentum", [0.0, 0.99])
@pytest.mark.parametrize("T", FRAMES)
def test_whole_run_matches_restatement(name, momentum, T):
    seed = 7 + T
    wav, resid, ok = run_gl(name, [mel_of(name, T)], [seed], 4, momentum)
    assert ok
    sc_err, wav_err, sc32, wav32 = gpu_stats(name, T, wav[0], resid[0], 4, momentum, seed)
    print(f"whole run {name} T={T} momentum={momentum}: sc {sc_err:.3g} (f32 restatement {sc32:.3g}), wav {wav_err:.3g} ({wav32:.3g})")
    assert sc_err <= SC_BAR and wav_err <= WAV_BAR


@pytest.mark.parametrize("T", [4, 5])
def test_the_restatement_tells_the_mutations_apart(T):
    """the two deliberate mutations, applied to the restatement, leave the bars of the whole-run test by orders of magnitude: the
    edge envelope replaced by its interior value (T = 4, 5), and Rprev updated before D is formed (momentum 0.99)"""
    a, M = audio("small"), mel_of("small", T)
    x, r, A = G.griffin_lim(M, 3, a, 4, 0.99)
    for kw in ({"edge_interior": True}, {"rprev_first": True}):
        xm, rm, _ = G.griffin_lim(M, 3, a, 4, 0.99, **kw)
        assert rel_l2(xm, x) > 100 * WAV_BAR
        assert np.abs(G.spectral_convergence(rm, A) - G.spectral_convergence(r, A)).max() > 100 * SC_BAR


# ---- 6. the defaults ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["prod", "small"])
@pytest.mark.parametrize("T", [37, 130])
def test_defaults_32_iterations(name, T):
    """finite, exactly (T - 1) hop samples, sc within the whole-run bar of the restatement, scaled by nothing; the waveform is not
    compared at 32 iterations (f32 and float64 may drift apart).

    Observed: 1.1e-7 .. 2.0e-7 on three cases and 1.12e-6 at production T = 37, whose deviation peaks at k = 18 (the first five steps
    stay within 2.5e-8): the iteration amplifies rounding differences there, in the restatement's f32 run as well."""
    a = audio(name)
    wav, resid, ok = run_gl(name, [mel_of(name, T)], [0], 32, 0.99)
    L = (T - 1) * a.hop_length
    assert ok and np.isfinite(wav[0, :L]).all() and (wav[0, L:] == 0).all() and np.abs(wav[0, :L]).max() > 0
    _, sc, A, _ = reference(name, T, 32, 0.99, 0)
    dev_k = np.abs(G.spectral_convergence(resid[0, :, :T], A) - sc)
    err = dev_k.max()
    print(f"defaults {name} T={T}: sc {err:.3g} at k = {int(dev_k.argmax())} (first five steps {dev_k[:5].max():.3g}), sc[0] {sc[0]:.3f} -> sc[32] {sc[32]:.3f}")
    assert err <= SC_BAR


# ---- 7. monotone at momentum 0 ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["prod", "small"])
@pytest.mark.parametrize("T", [37, 65, 130])
def test_monotone_without_momentum(name, T):
    """T = 4 and 5 are excluded on purpose: with reflect padding the step is no exact projection there"""
    _, sc, A, _ = reference(name, T, 32, 0.0, 1)
    assert ((sc[:-1] - sc[1:]) / sc[:-1]).min() >= 1e-3, "precondition: the restatement itself decreases by 1e-3 a step"
    _, resid, ok = run_gl(name, [mel_of(name, T)], [1], 32, 0.0)
    got = G.spectral_convergence(resid[0, :, :T], A)
    print(f"monotone {name} T={T}: sc[0] {got[0]:.3f} -> sc[32] {got[32]:.3f}")
    assert ok and (got[1:] < got[:-1]).all() and got[32] < 0.6 * got[0]


# ---- 8. batch and determinism -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["prod", "small"])
def test_batch_is_its_utterances_alone(name):
    from megatts2_amd.runtime import MelFrontEnd, griffin_lim_query
    a = audio(name)
    mels, seeds = [mel_of(name, T) for T in RAGGED], [5, 6, 2 ** 63 + 9, 8]
    fresh = MelFrontEnd(a)
    wav, resid, ok = run_gl(name, mels, seeds, 4, 0.99, fe=fresh)
    assert ok
    assert fresh.workspace_high_water() == griffin_lim_query(a, np.asarray(RAGGED), T_max=max(RAGGED) + 3, n_iter=4, return_resid=True)[0]
    again, resid2, _ = run_gl(name, mels, seeds, 4, 0.99)
    assert np.array_equal(wav, again) and np.array_equal(resid, resid2)
    for b, T in enumerate(RAGGED):
        L = (T - 1) * a.hop_length
        assert (wav[b, L:] == 0).all() and np.isfinite(wav[b]).all()
        assert (resid[b, :, T:] == 0).all() and np.isfinite(resid[b]).all()
        alone, r1, ok1 = run_gl(name, [mels[b]], [seeds[b]], 4, 0.99, T_max=T + (b % 2))
        assert ok1 and np.array_equal(alone[0, :L], wav[b, :L]) and np.array_equal(r1[0, :, :T], resid[b, :, :T])
    # another slot and another T_max
    moved, r2, ok2 = run_gl(name, [mels[1], mels[3]], [seeds[1], seeds[3]], 4, 0.99, T_max=140, slots=[2, 0], B=3)
    assert ok2
    for src, slot in ((1, 2), (3, 0)):
        T = RAGGED[src]
        L = (T - 1) * a.hop_length
        assert np.array_equal(moved[slot, :L], wav[src, :L]) and np.array_equal(r2[slot, :, :T], resid[src, :, :T])
    other, _, _ = run_gl(name, [mels[1]], [seeds[1] + 1], 4, 0.99)
    L = (RAGGED[1] - 1) * a.hop_length
    assert not np.array_equal(other[0, :L], wav[1, :L])
    no_resid, none, ok3 = run_gl(name, mels, seeds, 4, 0.99, resid=False)
    assert ok3 and none is None and np.array_equal(no_resid, wav)


def test_zero_iterations_is_the_inverse_stft_of_the_random_phase():
    a, T = audio("small"), 37
    wav, resid, ok = run_gl("small", [mel_of("small", T)], [4], 0, 0.99)
    A = G.mel_to_linear(mel_of("small", T), a)
    ref = G.istft(G.phase_init(A, 4), a)
    assert ok and resid.shape[1] == 1 and rel_l2(wav[0, :ref.size], ref) <= WAV_BAR


# ---- 9. range -------------------------------------------------------------------------------------------------------------------

def test_values_beyond_the_fp16_range():
    """one frame of log-mel 12 (exp = 1.6e5 > 65504): the two GEMMs run on f32 tiles, so the audio is finite and within the bars;
    the call after it on a normal input is bit-identical to that input's run before"""
    name, T = "prod", 37
    before, rb, _ = run_gl(name, [mel_of(name, T)], [3], 4, 0.99)
    M = mel_of(name, T).copy()
    M[9] = 12.0
    wav, resid, ok = run_gl(name, [M], [3], 4, 0.99)
    x, r, A = G.griffin_lim(M, 3, audio(name), 4, 0.99)
    L = (T - 1) * audio(name).hop_length
    assert ok and np.isfinite(wav).all() and A.max() > 65504
    sc_err = np.abs(G.spectral_convergence(resid[0, :, :T], A) - G.spectral_convergence(r, A)).max()
    print(f"range: sc {sc_err:.3g}, wav {rel_l2(wav[0, :L], x):.3g}")
    assert sc_err <= SC_BAR and rel_l2(wav[0, :L], x) <= WAV_BAR
    after, ra, _ = run_gl(name, [mel_of(name, T)], [3], 4, 0.99)
    assert np.array_equal(before, after) and np.array_equal(rb, ra)


# ---- 10. refusals -------------------------------------------------------------------------------------------------------------

def test_refusals_leave_the_outputs_untouched():
    from megatts2_amd.config import AudioConfig
    from megatts2_amd.runtime import MelFrontEnd, NativeError
    fe, a = frontend("small"), audio("small")
    T, B = 9, 2
    mel = dev(np.tile(mel_of("small", 37)[:T], (B, 1, 1)))
    L = (T - 1) * a.hop_length

    def refused(fe_, mel_, lens, out_w=L, **kw):
        wbuf = torch.full((B * out_w + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
        n_iter = max(kw.get("n_iter", 2), 0)
        rbuf = torch.full((B, n_iter + 1, T), float(SENT), device="cuda", dtype=torch.float32)
        with pytest.raises(NativeError):
            fe_.griffin_lim(mel_, lens, out=wbuf[:B * out_w].view(B, out_w), resid_out=rbuf if "n_iter" not in kw or kw["n_iter"] >= 0 else None,
                            **{"n_iter": 2, **kw})
        torch.cuda.synchronize()
        assert (wbuf == float(SENT)).all() and (rbuf == float(SENT)).all()

    refused(fe, mel, [T, T], n_iter=-1)
    refused(fe, mel, [T, T], momentum=1.0)
    refused(fe, mel, [T, T], momentum=-0.1)
    refused(fe, mel, [T, 3])                        # below n_fft / (2 hop) + 2 = 4
    refused(fe, mel, [T, T + 1])                    # beyond T_max
    refused(fe, mel, [T, T], out_w=L - 1)           # L_max < (max T - 1) hop
    deficient = MelFrontEnd(AudioConfig(sample_rate=16000, n_fft=64, hop_length=16, win_length=64, n_mels=80, f_min=0.0, f_max=8000.0))
    refused(deficient, dev(np.zeros((B, T, 80), np.float32)), [T, T])
    import ctypes
    from megatts2_amd import runtime as rt
    wbuf = torch.full((L + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
    with pytest.raises(NativeError):                # B < 1
        rt._check(fe.lib.mt2_griffin_lim(fe.h, None, ctypes.byref(fe.ac), rt._ptr(mel), rt._iptr(np.asarray([T], np.int32)), T, 0, 2, 0.5,
                                         rt._iptr(np.zeros(1, np.uint64)), rt._ptr(wbuf), L, None))
    assert (wbuf == float(SENT)).all()
    good, _, ok = run_gl("small", [mel_of("small", 37)], [1], 2, 0.5)      # the handle still works
    assert ok and np.isfinite(good).all()


# ---- 11. closed loop ------------------------------------------------------------------------------------------------------------

def test_closed_loop_mel_of_griffin_lim_of_mel():
    """mel(griffin_lim(mel(x))) against mel(x), production configuration, T = 130, defaults: the mel path is invertible to within
    what the restatement reaches on the same input, times 1.25 for f32 drift over 32 iterations"""
    fe, a, T = frontend("prod"), audio("prod"), 130
    x = G.vibrato_stack((T - 1) * a.hop_length, a.sample_rate)
    mel = fe(dev(x[None]))
    assert mel.shape == (1, T, a.n_mels)
    wav = fe.griffin_lim(mel)
    assert wav.shape == (1, (T - 1) * a.hop_length)
    back = fe(wav)
    assert back.shape == mel.shape
    got = rel_l2(back.cpu().numpy(), mel.cpu().numpy())
    M = mel_of("prod", T, "vib")
    y, _, _ = G.griffin_lim(M, 0, a, 32, 0.99)
    ref = rel_l2(G.log_mel(y, a), M)
    print(f"closed loop: log-mel rel L2 {got:.4f} (restatement {ref:.4f})")
    assert got <= 1.25 * ref


# ---- 12. the model: tiny synthetic weights --------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny_tts():
    from megatts2_amd import megatts2 as M
    (g, p, a, _), (sd_g, sd_p, sd_a, _) = synth_models("tiny")
    return M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a))), g


def test_synthesize_with_griffin_lim():
    tts, g = tiny_tts()
    rng = np.random.default_rng(12)
    B, Np, Tp = 2, 5, 24
    phone = dev(rng.integers(0, g.mrte.phone_vocab_size, (B, Np)).astype(np.int64))
    mels = dev((0.5 * rng.standard_normal((B, Tp, 80)) - 4.0).astype(np.float32))
    dur = np.asarray([[2, 3, 1, 2, 4], [1, 2, 2, 3, 1]], np.int32)
    plain = tts.synthesize(phone, mels, forced_durations=dur, return_aux=True)
    assert plain[2].get("wav") is None                                  # the default: no audio without HiFi-GAN, as before
    mel, mel_lens, aux = tts.synthesize(phone, mels, forced_durations=dur, griffin_lim={"n_iter": 3, "seeds": 5})
    assert torch.equal(mel, plain[0]) and np.array_equal(np.asarray(mel_lens), np.asarray(plain[1]))
    assert aux["wav"].shape == (B, (int(np.max(mel_lens)) - 1) * 256)
    assert torch.equal(aux["wav"], tts.vocode_griffin_lim(mel, mel_lens, n_iter=3, seeds=5))
    for b in range(B):
        L = (int(mel_lens[b]) - 1) * 256
        w = aux["wav"][b].cpu().numpy()
        assert np.isfinite(w).all() and np.abs(w[:L]).max() > 0 and (w[L:] == 0).all()


def test_forward_writes_a_file_only_with_griffin_lim(tmp_path):
    from megatts2_amd import audio_io
    tts, g = tiny_tts()
    wavs = tmp_path / "prompts"
    wavs.mkdir()
    x = G.vibrato_stack(16000 // 2)
    audio_io.write_wav(str(wavs / "p.wav"), x, 16000)
    phone = np.random.default_rng(13).integers(0, g.mrte.phone_vocab_size, 6)
    out = tmp_path / "out.wav"
    mel0, lens0, aux0 = tts.forward(str(wavs), phone_tokens=phone, out_path=str(out))
    assert not out.exists() and aux0.get("wav") is None                  # as today
    mel, lens, aux = tts.forward(str(wavs), phone_tokens=phone, out_path=str(out), vocoder={"n_iter": 2})
    assert torch.equal(mel, mel0) and out.exists()
    y, sr = audio_io.read_wav(str(out))
    Tp = 1 + x.size // 256
    assert sr == 16000 and y.size == (Tp - 1) * 256 + (int(lens[0]) - 1) * 256 and np.isfinite(y).all()
