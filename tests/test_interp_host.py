"""Prosody interpolation, host side (no GPU): properties of the float64 rule (tests/interp_ref.py), the exported entry points
and their parameter checks, `gamma_array`, and the cap on the reference's own ambiguous share for the inputs of the kernel test."""
import ctypes

import numpy as np
import pytest

import interp_ref as I
from interp_ref import mix_draw, mix_draw_many, mix_greedy, mix_rule, mixture
from sampling_ref import draw, rule, uniform_np


def _rows(rng, n=1024):
    return (rng.standard_normal(n) * 3).astype(np.float32), (rng.standard_normal(n) * 3).astype(np.float32)


def test_mixture_sums_to_one():
    rng = np.random.default_rng(0)
    for tau in (0.3, 1.0, 2.5):
        for g in (0.0, 0.1, 0.5, 1.0):
            zA, zB = _rows(rng)
            assert abs(mixture(zA, zB, tau, g).sum() - 1.0) < 1e-12
            R, pr, K, _ = mix_rule(zA, zB, g, tau, 40, 0.8)
            assert abs(pr.sum() - 1.0) < 1e-12 and np.isin(R, K).all() and (np.diff(R) > 0).all()


def test_top1_and_greedy_are_the_argmax_of_the_mixture_with_planted_ties():
    rng = np.random.default_rng(1)
    for r in range(100):
        zA, zB = _rows(rng)
        if r % 2:       # an exact tie of the maximum of m: the same values at the same indices of both rows
            top = np.sort(rng.choice(1024, 2 + r % 4, replace=False))
            zA[top] = zA.max() + 1.0
            zB[top] = zB.max() + 2.0
        g = (0.0, 0.25, 0.5, 1.0)[r % 4]
        u = float(rng.random())
        for tau in (0.5, 1.0, 2.0):
            m = mixture(zA, zB, tau, g)
            want = int(np.flatnonzero(m == m.max())[0])
            if r % 2:
                assert want == top[0]
            assert mix_draw(zA, zB, g, tau, 1, 1.0, u)[0] == want
            assert mix_draw(zA, zB, g, tau, 1, 0.4, u)[0] == want
            assert mix_draw(zA, zB, g, tau, 0, 1e-7, u)[0] == want
        m1 = mixture(zA, zB, 1.0, g)
        assert mix_greedy(zA, zB, g)[0] == int(np.flatnonzero(m1 == m1.max())[0]) == mix_draw(zA, zB, g, None, 0, 1.0, u)[0]


@pytest.mark.parametrize("tau,k,p", [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (0.9, 30, 0.8)])
def test_end_points_are_the_single_row_rule(tau, k, p):
    rng = np.random.default_rng(2)
    checked = 0
    for r in range(30):
        zA, zB = _rows(rng)
        us = rng.random(16)
        for g, z in ((0.0, zA), (1.0, zB)):
            R1, pr1, _, amb1 = rule(z, tau, k, p)
            R2, pr2, _, amb2 = mix_rule(zA, zB, g, tau, k, p)
            if amb1 or amb2:
                continue
            assert np.array_equal(R1, R2) and np.allclose(pr1, pr2, rtol=1e-12, atol=0)
            for u in us:
                c1, a1 = draw(z, tau, k, p, u)
                c2, a2 = mix_draw(zA, zB, g, tau, k, p, u)
                if not (a1 or a2):
                    checked += 1
                    assert c1 == c2
    assert checked > 300


@pytest.mark.parametrize("g", [0.25, 0.5, 0.75])
def test_swapping_the_contexts_with_the_complementary_weight_is_the_same_decision(g):
    rng = np.random.default_rng(3)
    for r in range(20):
        zA, zB = _rows(rng)
        us = rng.random(64)
        for tau, k, p in ((1.0, 0, 1.0), (0.7, 50, 0.9)):
            c1, a1, R1, pr1 = mix_draw_many(zA, zB, g, tau, k, p, us)
            c2, a2, R2, pr2 = mix_draw_many(zB, zA, 1.0 - g, tau, k, p, us)
            assert np.array_equal(R1, R2) and np.allclose(pr1, pr2, rtol=1e-12, atol=0)
            ok = ~(a1 | a2)
            assert np.array_equal(c1[ok], c2[ok])
        assert mix_greedy(zA, zB, g)[0] == mix_greedy(zB, zA, 1.0 - g)[0]


def test_ambiguity_flags_of_the_cuts():
    zA = np.asarray([2.0, 2.0 + 2e-5, 0.0, -1.0], np.float32)        # two nearly equal m at the top
    assert mix_greedy(zA, zA, 0.5)[1]
    assert mix_rule(zA, zA, 0.5, 1.0, top_k=1)[3]
    assert not mix_rule(zA, zA, 0.5, 1.0, top_k=2)[3]
    zT = np.asarray([2.0, 2.0, 0.0, -1.0], np.float32)               # an exact tie is ordered by index, not flagged
    assert mix_greedy(zT, zT, 0.5) == (0, False)
    assert not mix_rule(zT, zT, 0.5, 1.0, top_k=1)[3]


def test_interpolated_entry_points_are_exported_and_check_their_parameters():
    from megatts2_amd.build import build
    from megatts2_amd.sampling import MT2Sampling
    lib = ctypes.CDLL(build(verbose=False))
    for n in ("mt2_plm_infer_interpolated", "mt2_op_sample_mix_rows"):
        assert hasattr(lib, n), n
    lib.mt2_last_error.restype = ctypes.c_char_p
    dummy = ctypes.c_void_p(16)          # never dereferenced: the parameter check comes first
    for t, k, p, r, msg in ((0.0, 0, 1.0, 0, b"temperature"), (float("nan"), 0, 1.0, 0, b"temperature"),
                            (float("inf"), 0, 1.0, 0, b"temperature"), (1.0, -1, 1.0, 0, b"top_k"), (1.0, 1025, 1.0, 0, b"top_k"),
                            (1.0, 0, 0.0, 0, b"top_p"), (1.0, 0, 1.5, 0, b"top_p"), (1.0, 0, 1.0, 3, b"reserved")):
        s = MT2Sampling(t, k, p, r, None)
        rc = lib.mt2_op_sample_mix_rows(None, dummy, 1024, 1024, 4, ctypes.byref(s), dummy, dummy, dummy, dummy)
        assert rc != 0 and msg in lib.mt2_last_error(), (t, k, p, r, lib.mt2_last_error())
    assert lib.mt2_op_sample_mix_rows(None, dummy, 1024, 1024, 4, None, None, None, None, dummy) != 0      # no gamma
    lens = (ctypes.c_int32 * 1)(4)
    call = lib.mt2_plm_infer_interpolated
    for gm in (-0.1, 1.5, float("nan"), 0.5):        # without a handle even a valid gamma is an error
        g = (ctypes.c_float * 1)(gm)
        assert call(None, None, dummy, lens, 4, 1, None, 0, g, 0, dummy, None, None) != 0
    assert call(None, None, dummy, lens, 4, 1, None, 0, None, 0, dummy, None, None) != 0


def test_gamma_array_validates_and_broadcasts():
    from megatts2_amd.sampling import gamma_array
    a = gamma_array(0.25, 3)
    assert a.dtype == np.float32 and a.tolist() == [0.25, 0.25, 0.25] and a.flags.c_contiguous
    assert gamma_array([0.0, 1.0], 2).tolist() == [0.0, 1.0]
    assert gamma_array(np.asarray([0.5], np.float64), 1).dtype == np.float32
    assert gamma_array(1, 2).tolist() == [1.0, 1.0]
    for bad, B in ((-0.1, 1), (1.5, 1), (float("nan"), 2), ([0.2, 1.01], 2), ([0.5, float("nan")], 2), ([0.1, 0.2, 0.3], 2)):
        with pytest.raises(ValueError):
            gamma_array(bad, B)


def test_ambiguous_share_of_the_kernel_tests_inputs_is_capped():
    """The kernel test excuses a mismatch only where the float64 rule calls the decision ambiguous: that excuse may cover at most
    10 % of its decisions.  A condition on the inputs - should it fail after a change of inputs, change the inputs, not the cap."""
    zA, zB = I.kernel_rows()
    for n, A, cases in ((1024, I.KERNEL_PAIRS, I.KERNEL_CASES), (I.TAIL_N, I.TAIL_PAIRS, I.TAIL_CASES)):
        us = uniform_np(I.KERNEL_SEED, I.kernel_positions(A))
        for tau, k, p, g in cases:
            _, amb, _, _ = mix_draw_many(zA[:n], zB[:n], g, tau, k, p, us)
            print(f"N={n} tau={tau} top_k={k} top_p={p} gamma={g}: ambiguous share {amb.mean():.4f}")
            assert amb.mean() <= 0.10, (n, tau, k, p, g, float(amb.mean()))
            assert not mix_rule(zA[:n], zB[:n], g, tau, k, p)[3], "a cut of the kernel test's inputs is ambiguous"
        assert not mix_greedy(zA[:n], zB[:n], 0.5)[1]


def test_reference_loop_end_points_reproduce_the_greedy_fixtures():
    from conftest import load_golden, synth_models
    (_, p, _, _), (_, sd_p, _, _) = synth_models("tiny")
    for i in (1, 2):
        z = load_golden(f"tiny_utt{i}.npz")
        c, r = z["plm_cond"], np.ascontiguousarray(z["plm_cond"][::-1])
        assert np.array_equal(I.plm_infer_interpolated_ref(sd_p, p, c, r, 0.0)[0], z["p_codes"])
        assert np.array_equal(I.plm_infer_interpolated_ref(sd_p, p, r, c, 1.0)[0], z["p_codes"])
        codes, amb = I.plm_infer_interpolated_ref(sd_p, p, c, r, 0.5, 0.8, 40, 1.0, seed=7)
        assert codes.shape == z["p_codes"].shape == amb.shape and (codes >= 0).all() and (codes < 1024).all()
