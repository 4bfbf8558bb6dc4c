"""The float64 AR-step reference of tests/ar_step_ref.py (host only): it is pinned to the float32 oracle - which
tests/test_oracle_golden.py pins to the live reference modules - and the PLM cases are shown to have a safe arg-max.

  * the float32 oracle is within 5e-6 of the float64 step on every (model, case, slot, step): relative L2 of the logits (PLM),
    |p - p64| / max(1, |p64|) (ADM).  On production weights the float32 numpy oracle measures 5.1e-7 .. 1.0e-6 (PLM) and
    1.4e-8 .. 2.0e-6 (ADM) against the float64 step on these cases: the bound leaves a factor of 5 over the PLM's worst step and
    of 2.5 over the ADM's (one scalar per step, so a single unlucky rounding shows undamped; most steps are at a few 1e-7).  A reference
    that restated the step wrongly - a causal mask, a history shifted by one, a missing residual - misses it by orders of
    magnitude;
  * the top-2 gap of every PLM step's float64 logits is at least 100 x BAR x max |logit| (BAR = 8 x E32, the device bar of
    tests/test_gpu_ar_step_forms.py): a device within BAR of the reference cannot pick another code, which is what lets the
    device test feed the device's own code to the next step and still compare with logits computed here in advance.  The seeds of
    ar_step_ref were kept because this holds for them.
Every figure is printed before it is asserted (pytest -s).
"""
import numpy as np
import pytest

import ar_step_ref as R
import megatts2_oracle as O

F32_BOUND = 5e-6
PLM_CASES = [(m, c) for m in R.MODELS if not R.is_adm(m) for c in R.MODEL_CASES[m]]


@pytest.mark.parametrize("case", R.MODEL_CASES["adm"])
def test_f32_oracle_is_within_f32_arithmetic_of_the_f64_adm_step(case):
    lens, P, _ = R.CASES[case]
    for b, r in enumerate(R.adm_reference(case)):
        assert r["p64"].size == R.steps_of(case, b) and np.isfinite(r["p64"]).all()
        for k, (p32, p64) in enumerate(zip(r["p32"], r["p64"])):
            err = R.adm_err(p32, p64)
            print(f"adm {case} slot {b} n {P + k + 1}: p64 {p64:+.9f} p32 {p32:+.9f} err {err:.3e}")
            assert err <= F32_BOUND, (case, b, k, p32, p64)


@pytest.mark.parametrize("model,case", PLM_CASES)
def test_f32_oracle_is_within_f32_arithmetic_of_the_f64_plm_step(model, case):
    lens, P, _ = R.CASES[case]
    for b, r in enumerate(R.plm_reference(model, case)):
        assert r["logits64"].shape == (R.steps_of(case, b), R.model_of(model)[0].vq_bins) and r["logits64"].dtype == np.float64
        assert np.array_equal(r["codes32"], r["codes64"]) and np.array_equal(r["codes64"], r["logits64"].argmax(axis=1))
        for k, (l32, l64) in enumerate(zip(r["logits32"], r["logits64"])):
            err = O.rel_l2(l32, l64)
            print(f"{model} {case} slot {b} n {P + k + 1}: rel-L2 {err:.3e}")
            assert err <= F32_BOUND, (model, case, b, k)


@pytest.mark.parametrize("model", [m for m in R.MODELS if not R.is_adm(m)])
def test_plm_argmax_margins_are_a_hundred_bars_wide(model):
    need = 100.0 * R.bar(model)
    print(f"E32({model}) {R.e32(model):.3e}  BAR {R.bar(model):.3e}  needed top-2 gap {need:.3e} x max|logit|")
    for case in R.MODEL_CASES[model]:
        for b, r in enumerate(R.plm_reference(model, case)):
            for k, l64 in enumerate(r["logits64"]):
                gap = R.top2_gap(l64)
                print(f"{model} {case} slot {b} step {k}: gap {gap:.3e}")
                assert gap >= need, (model, case, b, k, gap, need)


def test_e32_is_the_largest_error_of_the_cases():
    for model in R.MODELS:
        e = R.e32(model)
        print(f"E32({model}) = {e:.3e}")
        assert 0.0 < e <= F32_BOUND
    # the float64 module is a second instance of the oracle, not the oracle itself re-typed
    assert R.O64 is not O and O.F32 is np.float32 and R.O64.F32 is np.float64
