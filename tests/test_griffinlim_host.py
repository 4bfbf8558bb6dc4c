"""Host side of the Griffin-Lim vocoder (no GPU): the restatement of the rule (tests/griffinlim_ref.py) against torch.istft, numpy's
pseudo-inverse and itself, and the library's host-only entry point mt2_griffin_lim_query against its closed form and the listed
refusals."""
import os

import numpy as np
import pytest

import griffinlim_ref as G

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


def audio(n_fft=1024, hop=256, n_mels=80):
    from megatts2_amd.config import AudioConfig
    return AudioConfig(sample_rate=16000, n_fft=n_fft, hop_length=hop, win_length=n_fft, n_mels=n_mels, f_min=0.0, f_max=8000.0)


PROD, SMALL = (1024, 256, 80), (64, 16, 8)


@pytest.mark.parametrize("cfg", [PROD, SMALL])
@pytest.mark.parametrize("T", [4, 5, 37])
def test_istft_is_torch_istft(cfg, T):
    a = audio(*cfg)
    N, h = a.n_fft, a.hop_length
    rng = np.random.default_rng(T + N)
    S = rng.standard_normal((T, N // 2 + 1)) + 1j * rng.standard_normal((T, N // 2 + 1))
    want = torch.istft(torch.from_numpy(S.T.copy()), N, h, N, window=torch.hann_window(N, periodic=True, dtype=torch.float64),
                       center=True, length=(T - 1) * h).numpy()
    assert np.abs(G.window(a) - torch.hann_window(N, periodic=True, dtype=torch.float64).numpy()).max() < 1e-15
    got = G.istft(S, a)
    assert got.shape == want.shape == ((T - 1) * h,)
    assert np.abs(got - want).max() <= 1e-10


@pytest.mark.parametrize("cfg", [PROD, SMALL])
@pytest.mark.parametrize("T", [4, 5, 37])
def test_round_trip_in_float64(cfg, T):
    a = audio(*cfg)
    x = G.two_tone_noise((T - 1) * a.hop_length, seed=T).astype(np.float64)
    S = G.stft(x, a)
    assert S.shape == (T, a.n_fft // 2 + 1)
    assert np.abs(G.istft(S, a) - x).max() <= 1e-12


@pytest.mark.parametrize("cfg", [PROD, SMALL])
def test_pseudo_inverse_by_cholesky_is_pinv(cfg):
    fb = G.filterbank(audio(*cfg))
    assert fb.dtype == np.float32 and fb.shape == (cfg[2], cfg[0] // 2 + 1)
    want = np.linalg.pinv(fb.astype(np.float64))
    assert np.abs(G.pinv_cholesky(fb) - want).max() <= 1e-12 * np.abs(want).max()
    assert np.linalg.cond(fb.astype(np.float64)) < 10


def test_rank_deficient_filterbank_is_refused(rt):
    """n_fft 64 with 80 mels: 33 bins cannot carry 80 filters (many cover no bin)"""
    a = audio(64, 16, 80)
    fb = G.filterbank(a)
    assert (np.abs(fb).sum(1) == 0).sum() >= 32
    with pytest.raises(np.linalg.LinAlgError):
        G.pinv_cholesky(fb)
    with pytest.raises(rt.NativeError, match="rank deficient"):
        rt.griffin_lim_query(a, [9, 9])
    assert rt.griffin_lim_query(audio(64, 16, 8), [9, 9])[1] == 8 * 16


def closed_form(a, lens, resid):
    up = lambda n: (n + 255) & ~255          # noqa: E731
    q = lambda n: (n + 3) & ~3               # noqa: E731
    N, h = a.n_fft, a.hop_length
    F = N // 2 + 1
    Fp, S, B = q(F), q(2 * F), len(lens)
    Fr, Rb = sum(lens), sum(t - 1 + N // h for t in lens)
    ints = 2 * q(Rb) + 4 * q(Fr) + 2 * q(B) + (q(2 * B) + Fr if resid else 2 * B)
    return up(4 * ints) + up(4 * Fr * a.n_mels) + up(4 * Fr * Fp) + 3 * up(4 * Fr * S) + up(4 * Fr * N) + up(4 * Rb * h)


@pytest.mark.parametrize("cfg", [PROD, SMALL])
@pytest.mark.parametrize("lens", [[4], [5], [37], [130], [4, 37, 65, 130], [431] * 8])
def test_query_matches_closed_form(rt, cfg, lens):
    a = audio(*cfg)
    for resid in (False, True):
        nbytes, L = rt.griffin_lim_query(a, lens, T_max=max(lens) + 3, return_resid=resid)
        assert nbytes == closed_form(a, lens, resid) and L == (max(lens) - 1) * a.hop_length
    assert rt.griffin_lim_query(a, None, T_max=37, B=3) == rt.griffin_lim_query(a, [37] * 3)


def test_query_refusals(rt):
    a = audio(*PROD)
    ok = dict(mel_lens=[9, 9])
    rt.griffin_lim_query(a, **ok)
    for kw in (dict(mel_lens=None, T_max=9, B=0), dict(mel_lens=[9, 9], n_iter=-1), dict(mel_lens=[9, 9], momentum=1.0),
               dict(mel_lens=[9, 9], momentum=-0.01), dict(mel_lens=[9, 9], momentum=float("nan")), dict(mel_lens=[9, 3]),
               dict(mel_lens=[9, 10], T_max=9), dict(mel_lens=[0, 9])):
        with pytest.raises(rt.NativeError):
            rt.griffin_lim_query(a, **kw)
        assert rt.load_library().mt2_last_error()
    assert rt.griffin_lim_query(a, [4])[1] == 3 * 256                  # the minimum at 1024 / 256
    with pytest.raises(rt.NativeError):                                # one window per hop: the overlap-add has zeros
        rt.griffin_lim_query(audio(64, 64, 8), [9])


def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_stft", "mt2_istft", "mt2_mel_to_linear", "mt2_griffin_lim", "mt2_griffin_lim_query"):
        assert hasattr(lib, name) and name + "(" in header


def test_phase_draw_is_the_sampling_generator():
    from sampling_ref import uniform_np
    u = G.phase_uniform(2 ** 40 + 5, 3, 33)
    assert u.shape == (3, 33) and u[2, 7] == uniform_np(np.uint64(2 ** 40 + 5), 2 * 33 + 7) and (0 <= u).all() and (u < 1).all()


@pytest.mark.parametrize("T", [37, 65, 130])
def test_restatement_is_monotone_without_momentum(T):
    """the precondition of the GPU test: at momentum 0 every one of 32 steps lowers the spectral convergence by at least 1e-3
    relative (smallest decrease seen: 1.2e-3), and the last value is below 0.6 of the first"""
    a = audio(*SMALL)
    for sig in (G.two_tone_noise((T - 1) * a.hop_length, seed=T), G.vibrato_stack((T - 1) * a.hop_length)):
        _, resid, A = G.griffin_lim(G.log_mel(sig, a), 1, a, 32, 0.0)
        sc = G.spectral_convergence(resid, A)
        assert ((sc[:-1] - sc[1:]) / sc[:-1]).min() >= 1e-3 and sc[32] < 0.6 * sc[0]


def test_f32_restatement_stays_near_float64():
    a = audio(*SMALL)
    M = G.log_mel(G.vibrato_stack(36 * a.hop_length), a)
    x, r, A = G.griffin_lim(M, 7, a, 4, 0.99)
    x32, r32, _ = G.griffin_lim(M, 7, a, 4, 0.99, np.float32)
    assert np.linalg.norm(x32 - x) / np.linalg.norm(x) < 1e-4
    assert np.abs(G.spectral_convergence(r32, A) - G.spectral_convergence(r, A)).max() < 1e-5
