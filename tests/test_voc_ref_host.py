"""tests/voc_ref.py against independent evaluations (host only): the float64 generator equals torch in float64 - primitive by
primitive, in reflect mode, and as a whole against transformers.SpeechT5HifiGan carrying the same weights; the pinned E32 is the
recomputed one; and the judge of tests/test_gpu_voc_forms.py (per-frame max abs error against 8 x E32) catches a wiring defect that
the whole-wave relative L2 of the stage tests (< 1e-3) lets through."""
import numpy as np
import pytest

import megatts2_oracle as O
import voc_ref as V

torch = pytest.importorskip("torch")
Fn = torch.nn.functional


def t64(a):         # [T, C] -> [1, C, T]
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).T.unsqueeze(0)


def back(y):
    return y[0].T.numpy()


@pytest.mark.parametrize("T,cin,cout,k,dil", [(1, 8, 12, 3, 1), (2, 8, 12, 11, 5), (37, 12, 8, 7, 3), (50, 4, 4, 11, 5), (9, 80, 16, 7, 1)])
def test_convolutions_equal_torch_double(T, cin, cout, k, dil):
    """Each convolution equals F.conv1d in float64 to 1e-12, zero mode and (where F.pad accepts the padding) reflect mode."""
    rng = np.random.default_rng(k * 100 + T)
    x, w, b = rng.standard_normal((T, cin)), rng.standard_normal((cout, cin, k)), rng.standard_normal(cout)
    g = (k - 1) // 2 * dil
    want = back(Fn.conv1d(t64(x), torch.from_numpy(w), torch.from_numpy(b), padding=g, dilation=dil))
    assert np.abs(V.same64(x, w, b, dil) - want).max() <= 1e-12
    assert np.abs(V.conv1d64(x, w, b, g, dil) - want).max() <= 1e-12
    if g < T:
        want = back(Fn.conv1d(Fn.pad(t64(x), (g, g), mode="reflect"), torch.from_numpy(w), torch.from_numpy(b), dilation=dil))
        assert np.abs(V.same64(x, w, b, dil, reflect=True) - want).max() <= 1e-12
    else:
        with pytest.raises(AssertionError):         # F.pad raises: so does the reference
            V.same64(x, w, b, dil, reflect=True)


@pytest.mark.parametrize("T,cin,cout,k,stride", [(1, 8, 4, 16, 8), (5, 8, 4, 16, 8), (33, 12, 6, 4, 2), (7, 6, 3, 4, 2)])
def test_transposed_convolutions_equal_torch_double(T, cin, cout, k, stride):
    rng = np.random.default_rng(k * 100 + T)
    x, w, b = rng.standard_normal((T, cin)), rng.standard_normal((cin, cout, k)), rng.standard_normal(cout)
    want = back(Fn.conv_transpose1d(t64(x), torch.from_numpy(w), torch.from_numpy(b), stride=stride, padding=(k - stride) // 2))
    got = V.conv_transpose1d64(x, w, b, stride, (k - stride) // 2)
    assert got.shape == (T * stride, cout) and np.abs(got - want).max() <= 1e-12


def generator_torch64(sd, cfg, mel):
    """The generator as torch modules would run it, float64 throughout (the slopes too, rounded to float32 like the device's):
    F.conv1d / F.conv_transpose1d / F.pad(mode="reflect") - independent of every helper of voc_ref."""
    w = {k: torch.from_numpy(np.asarray(v, np.float32)).double() for k, v in sd.items()}
    slope, slope_post = float(np.float32(cfg.leaky_relu_slope)), float(np.float32(0.01))
    reflect = cfg.pad_mode == "reflect"

    def same(x, name, k, d=1):
        g = (k - 1) // 2 * d
        if reflect:
            return Fn.conv1d(Fn.pad(x, (g, g), mode="reflect"), w[name + ".weight"], w[name + ".bias"], dilation=d)
        return Fn.conv1d(x, w[name + ".weight"], w[name + ".bias"], padding=g, dilation=d)
    pad = cfg.inference_padding
    x = t64(np.pad(mel, ((pad, pad), (0, 0)), mode="edge"))
    x = same(x, "conv_pre", 7)
    nk = len(cfg.resblock_kernel_sizes)
    for i, (r, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        x = Fn.conv_transpose1d(Fn.leaky_relu(x, slope), w[f"upsampler.{i}.weight"], w[f"upsampler.{i}.bias"], stride=r, padding=(k - r) // 2)
        hs = []
        for j, (rk, dils) in enumerate(zip(cfg.resblock_kernel_sizes, cfg.resblock_dilation_sizes)):
            h = x
            for n, d in enumerate(dils):
                y = same(Fn.leaky_relu(h, slope), f"resblocks.{i * nk + j}.convs1.{n}", rk, d)
                h = h + same(Fn.leaky_relu(y, slope), f"resblocks.{i * nk + j}.convs2.{n}", rk)
            hs.append(h)
        x = (hs[0] + hs[1] + hs[2]) / 3
    return torch.tanh(same(Fn.leaky_relu(x, slope_post), "conv_post", 7))[0, 0].numpy()


@pytest.mark.parametrize("gen,case,slot", [("prod-reflect", "reflect", 0), ("prod-pad5", "pad5", 0), ("wide-tail", "edges", 4), ("prod", "edges", 0)])
def test_generator_equals_torch_double(gen, case, slot):
    """Reflect mode equals F.pad(mode="reflect") in front of every 'same' convolution, inference_padding equals np.pad(mode="edge"),
    through the whole generator: 1e-12 on a tanh of rms 0.2."""
    cfg, sd = V.generator(gen)
    with torch.no_grad():
        want = generator_torch64(sd, cfg, V.mels(case)[slot])
    got = V.reference(gen, case)[slot]
    assert got.size == V.out_frames(gen, case, slot) * cfg.hop
    assert np.abs(got - want).max() <= 1e-12


def test_generator_equals_transformers_double():
    """hifigan64 (zero mode) equals transformers.SpeechT5HifiGan(...).double() carrying the same weights to 1e-8: the residue (3e-9
    measured) is the module's slope 0.1 against the device's float32(0.1)."""
    tr = pytest.importorskip("transformers")
    h, sd = V.generator("prod")
    tcfg = tr.SpeechT5HifiGanConfig(model_in_dim=h.in_dim, upsample_initial_channel=h.upsample_initial_channel,
                                    upsample_rates=h.upsample_rates, upsample_kernel_sizes=h.upsample_kernel_sizes,
                                    resblock_kernel_sizes=h.resblock_kernel_sizes, resblock_dilation_sizes=h.resblock_dilation_sizes,
                                    leaky_relu_slope=h.leaky_relu_slope, normalize_before=False)
    ref = tr.SpeechT5HifiGan(tcfg).eval()
    full = {k: torch.from_numpy(v) for k, v in sd.items()}
    full["mean"], full["scale"] = torch.zeros(h.in_dim), torch.ones(h.in_dim)
    ref.load_state_dict(full, strict=True)
    ref = ref.double()
    for slot in (1, 4):          # 1 and 9 frames
        with torch.no_grad():
            want = ref(torch.from_numpy(V.mels("edges")[slot]).double()).numpy()
        err = np.abs(V.reference("prod", "edges")[slot] - want).max()
        print(f"edges[{slot}]: max abs to SpeechT5HifiGan.double() {err:.2e}")
        assert err <= 1e-8


def test_cases_are_what_the_wiring_needs():
    assert all(c in V.CASES for cases in V.GEN_CASES.values() for c in cases) and set(V.GEN_CASES) == set(V.GENERATORS)
    assert V.CASES["edges"] == (5, 1, 24, 2, 9) and list(V.CASES["edges"]) != sorted(V.CASES["edges"])
    assert max(max(v) for v in V.CASES.values()) <= 40
    assert min(V.CASES["reflect"]) * 8 > 25 and min(V.CASES["reflect"]) > 3       # stage 0's widest halo; conv_pre's
    for case in ("edges", "equal", "reflect", "pad5"):       # every utterance differs from every other
        m = V.mels(case)
        assert [a.shape[0] for a in m] == list(V.CASES[case])
        assert len({a[:1].tobytes() for a in m}) == len(m)
    assert V.mels("alone-2")[0] is V.mels("edges")[2]
    assert V.generator("wide-tail")[0].upsample_initial_channel // 2 == 256       # the last stage's width: above conv_post's 128
    assert V.generator("prod-reflect")[0].pad_mode == "reflect" and V.generator("prod-pad5")[0].inference_padding == 5
    for g, case in (("prod", "edges"), ("wide-tail", "edges")):      # the absolute measure: a tanh of rms 0.15 - 0.85 here
        for w in V.reference(g, case):
            assert 0.1 < np.sqrt((w * w).mean()) < 0.9 and np.abs(w).max() < 1.0


def test_pinned_e32():
    """The pinned E32 of each generator family is at least the recomputed one and at most 1.5 times it."""
    for family in V.FAMILIES:
        got = V.e32_measured(family)
        print(f"{family}: recomputed E32 {got:.3e}, pinned {V.E32[family[0]]:.3e}")
        for g in family:
            assert got <= V.E32[g] <= 1.5 * got, (g, got, V.E32[g])
            assert V.bar(g) == 8.0 * V.E32[g]
    assert O.hifigan is O._NUMPY_PRIMS.get("hifigan", O.hifigan)      # the oracle's numpy primitives are back


@pytest.mark.parametrize("mutant", [(1, 0, 0), (3, 2, 2)])
@pytest.mark.parametrize("slot", [4, 2])          # 9 and 24 frames
def test_the_judge_has_teeth(mutant, slot):
    """One convs2 (stage, resblock, pair) reading one extra copy of its last row behind the utterance's end fails the per-frame
    judge by a factor of 100 - in the last frame only - while its whole-wave relative L2 passes the stage tests' 1e-3."""
    cfg, sd = V.generator("prod")
    good = V.reference("prod", "edges")[slot]
    bad = V.hifigan64(sd, cfg, V.mels("edges")[slot], mutant=mutant)
    err = V.frame_err(bad, good, cfg.hop)
    moved = int((np.abs(bad - good) > V.bar("prod")).sum())
    print(f"mutant {mutant} at {err.size} frames: worst frame {err.max():.2e} = {err.max() / V.bar('prod'):.0f} x the bar, {moved} samples moved, "
          f"whole-wave rel-L2 {O.rel_l2(bad, good):.2e}")
    assert err.max() >= 100 * V.bar("prod")
    assert int(err.argmax()) == err.size - 1 and (err[:-2] <= V.bar("prod")).all()       # an edge frame, not the interior
    assert O.rel_l2(bad, good) < 1e-3
