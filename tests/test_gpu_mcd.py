"""Mel-cepstral distortion along the DTW path on the GPU (csrc/mcd.hip: mt2_mel_cepstrum, mt2_path_distortion,
mt2_mel_cepstral_distortion) against the restatement of its rule (tests/mcd_ref.py), compare_audio on analytic tones and
Megatts.align_prompt's `mcd` on the tiny synthetic-weight model.

Bars, none of them chosen from what the kernels give:
  cepstrum   every coefficient within mcd_ref.coefficient_bound, (N + 2) 2^-24 sum_m |M[m]| |tab[m]|, of the float64 sum; rows at or
             beyond the length exactly 0; padding rows are NaN (a read of one poisons a coefficient); a ragged batch bit-identical to
             its utterances alone.
  path row   on paths the test builds: the three counts exactly; the double fields within cells 2^-53, relative to the mean of the
             terms' magnitudes (the bound of a recursive sum of `cells` terms, u = 2^-53: |error| <= cells u sum |term|), of the
             restatement run in the kernel's order on the kernel's own inputs with the cost chain restated bit for bit.
  whole      lo / hi bit-equal to dtw_ref.align on the bit-for-bit costs of the kernel's own cepstra; the row bit-equal to
             mt2_path_distortion on that path; the analytic cases of test_mcd_host.py inside mcd_ref.db_bound; a copy with repeated
             frames exactly 0.0.
Shapes: T in {1, 2, 63, 64, 65, 257} around the cepstrum kernel's tile of 32 frames and more than one workgroup; N in {2, 80, 128},
K in {1, 13, 32}; paths at Tb in {1, 255, 256, 257, 600}, where a thread's column count changes from 0 to 1 to 2 to 3.

Observed on an MI355X: the cepstrum at most 0.064 of its bound at N >= 80 (0.207 at N = 2) and bit-equal to the fma restatement; every
double field of the path rows equal to the restatement's, log2 included, but one that is an ulp off (0.005 of the bar); the analytic
cases at most 0.0053 of db_bound; compare_audio reads 50.053 cents for tones 50 cents apart.  The file takes 3 s."""
import functools
import math

import numpy as np
import pytest

import dtw_ref
import f0_ref as F0
import mcd_ref as R
from conftest import load_golden, synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U53 = 2.0 ** -53
TS = (1, 2, 63, 64, 65, 257)
NK = [(2, 1), (80, 1), (80, 13), (80, 32), (128, 1), (128, 13), (128, 32)]
SENT = -77.25
GUARD = 11


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


def nan_stack(rows, extra):
    """rows [T_b, W] -> (f32 [B, max T + extra, W] with NaN beyond every length, lens)"""
    lens = np.asarray([r.shape[0] for r in rows], np.int32)
    out = np.full((len(rows), int(lens.max()) + extra) + rows[0].shape[1:], np.nan, np.float32)
    for b, r in enumerate(rows):
        out[b, :r.shape[0]] = r
    return out, lens


# ---- cepstrum ------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def cep_mels(N):
    return tuple(R.log_mel(T, N, seed=100 * N + T) for T in TS)


@pytest.mark.parametrize("N, K", NK)
def test_cepstrum_is_inside_the_bound_of_float64_and_zero_beyond_the_length(N, K):
    from megatts2_amd import runtime as rt
    fe, mels = frontend(), cep_mels(N)
    mel, lens = nan_stack(mels, 3)
    B, T_max = mel.shape[:2]
    buf = torch.full((B * T_max * K + GUARD,), SENT, device="cuda", dtype=torch.float32)
    md = dev(mel)
    rt._check(fe.lib.mt2_mel_cepstrum(fe.h, rt._stream(), rt._ptr(md), rt._iptr(lens), T_max, B, N, K, rt._ptr(buf)))
    host = buf.cpu().numpy()
    assert (host[B * T_max * K:] == np.float32(SENT)).all()
    cep = host[:B * T_max * K].reshape(B, T_max, K)
    worst = 0.0
    for b, m in enumerate(mels):
        T = m.shape[0]
        assert (cep[b, T:] == 0).all() and np.isfinite(cep[b, :T]).all()
        err, bound = np.abs(cep[b, :T].astype(np.float64) - R.cepstrum64(m, K)), R.coefficient_bound(m, K)
        worst = max(worst, float((err / bound).max()))
        assert (err <= bound).all(), (T, float((err / bound).max()))
        assert np.array_equal(cep[b, :T], R.cepstrum32_chain(m, K)), T            # and the chain itself, bit for bit
    print(f"N={N} K={K}: worst coefficient error {worst:.3f} of the bound")
    assert torch.equal(fe.mel_cepstrum(md, lens, K), buf[:B * T_max * K].view(B, T_max, K))


@pytest.mark.parametrize("N, K", [(80, 13), (128, 32), (2, 1)])
def test_cepstrum_of_a_ragged_batch_is_its_utterances_alone(N, K):
    fe, mels = frontend(), cep_mels(N)
    alone = [fe.mel_cepstrum(dev(m[None]), None, K)[0].cpu().numpy() for m in mels]
    order = (5, 0, 3, 2, 4)                                                      # B = 5, other slots, another T_max
    mel, lens = nan_stack([mels[i] for i in order], 40)
    got = fe.mel_cepstrum(dev(mel), lens, K).cpu().numpy()
    for slot, i in enumerate(order):
        assert np.array_equal(got[slot, :lens[slot]], alone[i]) and (got[slot, lens[slot]:] == 0).all()


# ---- the path reduction on paths the test builds ---------------------------------------------------------------------------------

def f0_tracks(Ta, Tb, rng):
    """voiced contours with unvoiced (0), negative and NaN frames among them"""
    fa = (120.0 * 2.0 ** rng.uniform(-0.5, 0.5, Ta)).astype(np.float32)
    fb = (140.0 * 2.0 ** rng.uniform(-0.5, 0.5, Tb)).astype(np.float32)
    for f in (fa, fb):
        k = rng.random(f.size)
        f[k < 0.2] = 0.0
        f[(k >= 0.2) & (k < 0.25)] = np.nan
        f[(k >= 0.25) & (k < 0.28)] = -50.0
    return fa, fb


def build_case(name, K=13):
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "diagonal":
        Ta = Tb = 100
        lo = hi = np.arange(Tb, dtype=np.int32)
    elif name == "column":                                                       # one vertical run over a strip boundary
        Ta, Tb = 70, 1
        lo, hi = np.zeros(1, np.int32), np.full(1, Ta - 1, np.int32)
    elif name == "row":
        Ta, Tb = 1, 40
        lo = hi = np.zeros(Tb, np.int32)
    else:
        Tb = int(name.split("-")[1])
        Ta = max(1, (2 * Tb) // 3 + 2)
        lo, hi = R.monotone_path(Ta, Tb, rng)
    ca = rng.standard_normal((Ta, K)).astype(np.float32)
    cb = (ca[np.minimum(np.arange(Tb) * Ta // Tb, Ta - 1)] + 0.1 * rng.standard_normal((Tb, K))).astype(np.float32)
    fa, fb = f0_tracks(Ta, Tb, rng)
    return ca, cb, lo, hi, fa, fb


PATHS = ("diagonal", "column", "row", "random-1", "random-255", "random-256", "random-257", "random-600")


def run_paths(cases, extra=(3, 5), f0=True):
    fe = frontend()
    (ca, al), (cb, bl) = nan_stack([c[0] for c in cases], extra[0]), nan_stack([c[1] for c in cases], extra[1])
    (fa, _), (fb, _) = nan_stack([c[4] for c in cases], extra[0]), nan_stack([c[5] for c in cases], extra[1])
    lo = np.full(cb.shape[:2], -1, np.int32)
    hi = np.full(cb.shape[:2], -1, np.int32)
    for b, c in enumerate(cases):
        lo[b, :bl[b]], hi[b, :bl[b]] = c[2], c[3]
    out = fe.path_distortion(dev(ca), dev(cb), dev(lo), dev(hi), al, bl, dev(fa) if f0 else None, dev(fb) if f0 else None)
    return out.cpu().numpy()


def check_row(got, want, mean_abs, what):
    cells = want[0]
    assert got[0] == want[0] and got[3] == want[3] and got[6] == want[6], (what, got, want)
    tol = cells * U53
    scale = {1: want[1], 2: want[2], 4: want[4], 5: mean_abs, 7: want[7]}          # the mean magnitude of each field's terms
    for f, s in scale.items():
        err = abs(got[f] - want[f])
        print(f"{what} field {f}: {got[f]!r} against {want[f]!r}, off by {err:.3g} = {err / (tol * s) if s else 0.0:.3g} of cells 2^-53 relative")
        assert err <= tol * s, (what, f, got[f], want[f])


@functools.lru_cache(maxsize=None)
def path_results():
    cases = {n: build_case(n) for n in PATHS}
    rows = {n: run_paths([c])[0] for n, c in cases.items()}
    return cases, rows


@pytest.mark.parametrize("name", PATHS)
def test_path_row_is_the_restatement_in_the_kernels_order(name):
    cases, rows = path_results()
    ca, cb, lo, hi, fa, fb = cases[name]
    want, mean_abs = R.path_row(R.cost32_fma(ca, cb), lo, hi, fa, fb, return_abs=True)
    assert want[0] == dtw_ref.check_path(lo, hi, ca.shape[0], cb.shape[0])
    check_row(rows[name], want, mean_abs, name)
    bare = run_paths([cases[name]], f0=False)[0]
    assert np.array_equal(bare[:3], rows[name][:3]) and (bare[3:] == 0).all()


def test_path_rows_of_a_ragged_batch_are_its_utterances_alone():
    cases, rows = path_results()
    order = ("random-257", "column", "random-600", "row", "random-255", "diagonal")
    got = run_paths([cases[n] for n in order], extra=(17, 40))
    for slot, n in enumerate(order):
        assert np.array_equal(got[slot], rows[n]), n


@pytest.mark.parametrize("K", [1, 32])
def test_path_row_at_the_ends_of_the_order(K):
    c = build_case("random-257", K)
    want, mean_abs = R.path_row(R.cost32_fma(c[0], c[1]), c[2], c[3], c[4], c[5], return_abs=True)
    check_row(run_paths([c])[0], want, mean_abs, f"K={K}")


@pytest.mark.parametrize("cents", [35.0, -120.0])
@pytest.mark.parametrize("name", ["row", "random-257"])
def test_tracks_a_known_number_of_cents_apart_read_it(name, cents):
    ca, cb, lo, hi, _, _ = path_results()[0][name]
    fb = np.full(cb.shape[0], 155.0, np.float32)
    fa = np.full(ca.shape[0], np.float32(155.0 * 2.0 ** (cents / 1200)), np.float32)
    c = 1200.0 * math.log2(float(fa[0]) / float(fb[0]))                           # what the two f32 values are apart
    assert abs(c - cents) < 1e-3
    got = run_paths([(ca, cb, lo, hi, fa, fb)])[0]
    cells = got[0]
    print(f"{name} {cents}: rmse {got[4]!r}, offset {got[5]!r}, {c!r} expected over {int(cells)} cells")
    assert got[3] == cells and got[6] == 0 and got[7] == 0
    assert abs(got[4] - abs(c)) <= cells * U53 * abs(c) and abs(got[5] - c) <= cells * U53 * abs(c)


def test_lo_hi_outside_the_matrix_are_cut_not_followed():
    """not a path the DTW leaves, but one the call must survive: runs reaching below 0 and beyond Ta read nothing outside ca"""
    ca, cb, _, _, fa, fb = build_case("random-255")
    Ta, Tb = ca.shape[0], cb.shape[0]
    lo, hi = np.full(Tb, -5, np.int32), np.full(Tb, Ta + 1000, np.int32)
    got = run_paths([(ca, cb, lo, hi, fa, fb)])[0]
    assert got[0] == Ta * Tb and np.isfinite(got).all()


# ---- the whole chain -------------------------------------------------------------------------------------------------------------

PAIRS = ((37, 50), (130, 100), (1, 1), (64, 65), (70, 1))


@functools.lru_cache(maxsize=None)
def chain_inputs():
    out = []
    for n, (Ta, Tb) in enumerate(PAIRS):
        rng = np.random.default_rng(500 + n)
        A = R.log_mel(Ta, 80, seed=600 + n)
        Bm = (A[np.minimum(np.arange(Tb) * Ta // Tb, Ta - 1)] + 0.2 * rng.standard_normal((Tb, 80))).astype(np.float32)
        out.append((A, Bm) + f0_tracks(Ta, Tb, rng))
    return tuple(out)


def run_chain(items, extra=(3, 5), K=13):
    fe = frontend()
    (A, al), (Bm, bl) = nan_stack([c[0] for c in items], extra[0]), nan_stack([c[1] for c in items], extra[1])
    (fa, _), (fb, _) = nan_stack([c[2] for c in items], extra[0]), nan_stack([c[3] for c in items], extra[1])
    row, lo, hi = fe.mcd(dev(A), dev(Bm), al, bl, dev(fa), dev(fb), order=K, return_path=True)
    return row, lo, hi, (dev(A), dev(Bm), al, bl, dev(fa), dev(fb))


def test_whole_chain_is_its_pieces_bit_for_bit():
    fe, items = frontend(), chain_inputs()
    row, lo, hi, (A, Bm, al, bl, fa, fb) = run_chain(items)
    ca, cb = fe.mel_cepstrum(A, al, 13), fe.mel_cepstrum(Bm, bl, 13)
    lo_h, hi_h = lo.cpu().numpy(), hi.cpu().numpy()
    for b, (Ta, Tb) in enumerate(PAIRS):
        ref = dtw_ref.align(R.cost32_fma(ca[b, :Ta].cpu().numpy(), cb[b, :Tb].cpu().numpy()))
        assert np.array_equal(lo_h[b, :Tb], ref["lo"]) and np.array_equal(hi_h[b, :Tb], ref["hi"]), (Ta, Tb)
        assert (lo_h[b, Tb:] == -1).all() and (hi_h[b, Tb:] == -1).all()
        assert row[b, 0].item() == ref["steps"]
    assert torch.equal(row, fe.path_distortion(ca, cb, lo, hi, al, bl, fa, fb))
    bare = fe.mcd(A, Bm, al, bl, order=13)
    assert torch.equal(bare[:, :3], row[:, :3]) and (bare[:, 3:] == 0).all()
    # a ragged batch is its utterances alone, whatever the slot and the padded lengths
    order = (3, 0, 4, 1)
    again = run_chain([items[i] for i in order], extra=(20, 9))[0]
    for slot, i in enumerate(order):
        assert torch.equal(again[slot], row[i]), i
        alone = run_chain([items[i]], extra=(0, 0))[0]
        assert torch.equal(alone[0], row[i]), i


@pytest.mark.parametrize("T", [1, 2, 37, 130])
def test_ground_truth_on_the_device(T):
    """the three analytic cases of test_mcd_host.py, inside the same derived bound"""
    fe, K = frontend(), 13
    A = R.log_mel(T, 80, seed=10 + T)
    rng = np.random.default_rng(30 + T)
    cases = [(R.cos_mel(A, 0.5, 1), R.DB * 0.5 / math.sqrt(2.0), 0.25, 1), (R.cos_mel(A, 1.0, 13), R.DB / math.sqrt(2.0), 0.5, 13),
             (R.cos_mel(A, 0.7, 0), 0.0, 0.0, 1), (R.cos_mel(A, 1.0, K + 1), 0.0, 0.0, 1)]
    for Bm, want, d, k0 in cases:
        delta = np.zeros(K)
        delta[k0 - 1] = d
        bound = R.db_bound(A, Bm, K, delta)
        row, lo, hi = fe.mcd(dev(A[None]), dev(Bm[None]), order=K, return_path=True)
        row = row[0].cpu().numpy()
        print(f"T={T}: mcd {row[1]:.9f}, {want:.9f} expected, off by {abs(row[1] - want):.3g} = {abs(row[1] - want) / bound:.4f} of the bound {bound:.3g}")
        assert row[0] == T and lo[0].cpu().tolist() == hi[0].cpu().tolist() == list(range(T))
        assert abs(row[1] - want) <= bound and abs(row[2] - want) <= bound
    Bm = dtw_ref.warp_rows(A, rng.integers(1, 4, T))
    row = fe.mcd(dev(A[None]), dev(Bm[None]), order=K)[0].cpu().numpy()
    assert row[0] == Bm.shape[0] and row[1] == 0.0 and row[2] == 0.0


def test_compare_audio_reads_the_cents_between_two_tones():
    """harmonic stacks (so that the mel is not degenerate) 50 cents apart: the F0 RMSE within the tracker's pinned 0.73 cents of
    that; a clip against itself reads exactly 0"""
    from megatts2_amd import megatts2 as M
    cents, f = 50.0, 150.0
    a = F0.tone(f * 2.0 ** (cents / 1200), 8192, F0.HARMONICS[1], seed=1)
    b = F0.tone(f, 8192, F0.HARMONICS[1], seed=2)
    st = M.compare_audio(a, b)
    print({k: float(v[0]) for k, v in st.items()})
    assert st["voiced_cells"][0] > 0 and st["cells"][0] >= 33
    assert abs(st["f0_rmse_cents"][0] - cents) <= 0.73 and abs(st["f0_offset_cents"][0] - cents) <= 0.73
    same = M.compare_audio(a, a)
    assert same["mcd_db"][0] == 0.0 and same["max_db"][0] == 0.0 and same["cells"][0] == 33
    assert same["f0_rmse_cents"][0] == 0.0 and same["vuv_cells"][0] == 0
    d = M.mel_cepstral_distortion(M.extract_mel_spec(a).transpose(0, 1), M.extract_mel_spec(b).transpose(0, 1), f0_a=M.extract_f0(a), f0_b=M.extract_f0(b))
    assert all(np.array_equal(d[k], st[k]) for k in st)


# ---- the model: tiny synthetic weights -------------------------------------------------------------------------------------------

def test_align_prompt_reports_the_distortion_and_keeps_its_durations():
    from megatts2_amd import megatts2 as M
    (g, p, a, _), (sd_g, sd_p, sd_a, _) = synth_models("tiny")
    tts = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)))
    z = load_golden("tiny_prompted.npz")
    mels, pps = dev(z["prompt_mel"][None]).repeat(2, 1, 1), dev(z["prompt_phone"][None]).repeat(2, 3)
    mels[1] = torch.flip(mels[1], dims=[0])
    plain = tts.align_prompt(pps, mels)
    dur, aux = tts.align_prompt(pps, mels, return_aux=True)
    assert np.array_equal(plain, dur)
    Tp = mels.shape[1]
    lo, hi = aux["mcd_lo"].cpu().numpy(), aux["mcd_hi"].cpu().numpy()
    assert set(aux["mcd"]) == set(R.NAMES)
    for b in range(2):
        assert aux["mcd"]["cells"][b] == dtw_ref.check_path(lo[b], hi[b], int(aux["syn_lens"][b]), Tp)
        assert np.isfinite(aux["mcd"]["mcd_db"][b]) and 0 <= aux["mcd"]["mcd_db"][b] <= aux["mcd"]["max_db"][b]
