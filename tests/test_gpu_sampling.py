"""Seeded PLM sampling on the GPU (csrc/sampling.hip, the mt2_*_sampled entry points, the Python surfaces): the kernel
against the float64 rule (tests/sampling_ref.py), greedy equivalence of the limits, the draws inside the AR loop, the
sampled oracle, batch / call invariance, pipeline consistency and the range guard's repeat.

A decision is "ambiguous" when u * S lies within 1e-4 * S of a cumulative boundary (or the top-p cut within 1e-4 of
sum_K w): float64 and the kernel's f32 may then disagree; every other decision must match exactly, and the disagreements
themselves stay at or below 0.1 % of the decisions."""
import math
import os

import numpy as np
import pytest

import megatts2_oracle as O
from conftest import load_golden, synth_models
from sampling_ref import draw, draw_many, plm_infer_sampled, uniform_np

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

_MODELS = {}


def model(kind):
    if kind not in _MODELS:
        from megatts2_amd import megatts2 as M
        (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models(kind)
        _MODELS[kind] = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)), hifi_gan=M.HIFIGAN(h, sd_h))
    return _MODELS[kind]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pad_stack(arrs):
    n = max(a.shape[0] for a in arrs)
    out = np.zeros((len(arrs), n) + arrs[0].shape[1:], arrs[0].dtype)
    for i, a in enumerate(arrs):
        out[i, :a.shape[0]] = a
    return out, np.asarray([a.shape[0] for a in arrs], np.int32)


def S(t, k=0, p=1.0):
    from megatts2_amd.sampling import PLMSampling
    return PLMSampling(t, k, p)


def chi2_isf_1e6(df):
    try:
        from scipy.stats import chi2
        return float(chi2.isf(1e-6, df))
    except ImportError:           # Wilson-Hilferty; z = the 1e-6 upper normal quantile
        z = 4.753424
        return df * (1 - 2 / (9 * df) + z * math.sqrt(2 / (9 * df))) ** 3


# ---------------------------------------------------------------------------------------------------
# 1. the kernel alone


@pytest.mark.parametrize("tau,k,p", [(1.0, 0, 1.0), (0.7, 50, 1.0), (1.3, 0, 0.9), (1.0, 1, 1.0)])
def test_op_sample_rows_against_the_float64_rule(tau, k, p):
    from megatts2_amd.runtime import op_sample_rows
    rng = np.random.default_rng(1234)
    z = (rng.standard_normal(1024) * 3).astype(np.float32)
    A = 65536
    seed = 0x5EED_0000_1234
    pos = np.arange(A, dtype=np.int32) * 3 + 7
    got = op_sample_rows(dev(np.tile(z, (A, 1))), S(tau, k, p), dev(np.full(A, seed, np.int64)), dev(pos)).cpu().numpy()
    us = uniform_np(seed, pos)
    want, amb, R, pr = draw_many(z, tau, k, p, us)
    assert np.isin(got, R).all(), "a choice outside K / R"
    bad = (got != want) & ~amb
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8])
    # with 1024 index-order boundaries a few % of the u land within 1e-4 of one, so the budget is on the disagreements
    # themselves (which can only be such rows): at most 0.1 %
    assert (got != want).mean() <= 1e-3, int((got != want).sum())
    # chi-square of the histogram over R against the float64 probabilities (bins with < 5 expected pooled)
    exp = pr * A
    obs = np.asarray([(got == r).sum() for r in R], np.float64)
    small = exp < 5
    e2 = np.concatenate([exp[~small], [exp[small].sum()]]) if small.any() else exp
    o2 = np.concatenate([obs[~small], [obs[small].sum()]]) if small.any() else obs
    keep = e2 > 0
    e2, o2 = e2[keep], o2[keep]
    if e2.size > 1:
        chi = float(((o2 - e2) ** 2 / e2).sum())
        assert chi < chi2_isf_1e6(e2.size - 1), (chi, e2.size)
    else:
        assert (got == R[0]).all()


def test_op_sample_rows_top1_picks_the_lowest_index_of_planted_ties():
    from megatts2_amd.runtime import op_sample_rows
    rng = np.random.default_rng(7)
    A = 512
    z = (rng.standard_normal((A, 1024)) * 3).astype(np.float32)
    for r in range(A):
        idx = np.sort(rng.choice(1024, 2 + r % 4, replace=False))
        z[r, idx] = z[r].max() + float(r % 3)
    z[::7] = np.round(z[::7])
    want = z.argmax(1)
    for tau, p in ((1.0, 1.0), (0.2, 0.3), (5.0, 1.0)):
        got = op_sample_rows(dev(z), S(tau, 1, p), dev(rng.integers(0, 2 ** 62, A)), dev(np.arange(A, dtype=np.int32))).cpu().numpy()
        assert np.array_equal(got, want)
        got = op_sample_rows(dev(z), S(tau, 0, 1e-7), dev(rng.integers(0, 2 ** 62, A)), dev(np.arange(A, dtype=np.int32))).cpu().numpy()
        assert np.array_equal(got, want)


# ---------------------------------------------------------------------------------------------------
# 2. the greedy limits are the greedy path, bit for bit


GREEDY_LIMITS = [S(0.8, 1, 0.5), S(1.7, 0, 1e-7)]


def test_greedy_limits_tiny_ragged_batch():
    tts = model("tiny")
    zs = [load_golden(f"tiny_utt{i}.npz") for i in range(4)]
    cond, ln = pad_stack([z["plm_cond"] for z in zs])
    want = tts.native.plm_infer(dev(cond), ln)
    for smp in GREEDY_LIMITS:
        got = tts.native.plm_infer(dev(cond), ln, sampling=smp, seeds=np.arange(4) * 977 + 5)
        assert torch.equal(got, want)
    for i, z in enumerate(zs):
        assert np.array_equal(want[i, :ln[i]].cpu().numpy(), z["p_codes"])


def test_greedy_limits_prod_c1_and_prompted():
    tts = model("prod")
    z = load_golden("prod_utt0.npz")
    args = (dev(z["phone"][None]), dev(z["prompt_mel"][None]))
    mel0, l0, aux0 = tts.synthesize(*args, forced_durations=z["forced_dur"][None], return_aux=True)
    assert np.array_equal(aux0["codes"][0, :33].cpu().numpy(), z["p_codes"])
    for smp in GREEDY_LIMITS:
        mel, l1, aux = tts.synthesize(*args, forced_durations=z["forced_dur"][None], return_aux=True, sampling=smp, seeds=99)
        assert torch.equal(aux["codes"], aux0["codes"]) and torch.equal(mel, mel0) and l1.tolist() == l0.tolist()
    zp = load_golden("prod_prompted.npz")
    pargs = (dev(zp["phone"][None]), dev(zp["prompt_mel"][None]), dev(zp["prompt_phone"][None]), zp["prompt_dur"][None])
    pm0, _, pa0 = tts.synthesize_prompt_conditioned(*pargs, forced_durations=zp["forced_dur"][None], return_aux=True)
    assert np.array_equal(pa0["codes"][0, :zp["p_codes"].size].cpu().numpy(), zp["p_codes"])
    for smp in GREEDY_LIMITS:
        pm, _, pa = tts.synthesize_prompt_conditioned(*pargs, forced_durations=zp["forced_dur"][None], return_aux=True,
                                                      sampling=smp, seeds=[12345])
        assert torch.equal(pa["codes"], pa0["codes"]) and torch.equal(pm, pm0)


# ---------------------------------------------------------------------------------------------------
# 3. the sampler inside the AR loop: every step against the rule on the GPU's own logits


@pytest.mark.parametrize("P", [0, 5])
def test_sampled_plm_steps_follow_the_rule_under_every_grouping(P):
    tts = model("prod")
    nat = tts.native
    rng = np.random.default_rng(31 + P)
    lens = np.asarray([21, 13, 7, 21, 1, 16, 9, 12], np.int32)
    B, T = lens.size, int(lens.max())
    cond = np.maximum(rng.standard_normal((B, P + T, 512)), 0).astype(np.float32)
    prefix = dev(rng.integers(0, 1024, (B, P))) if P else None
    seeds = rng.integers(0, 2 ** 63, B).astype(np.uint64)
    prev = nat.get_option("ar_groups")
    try:
        for groups in (1, 2, 4):
            nat.set_ar_groups(groups)
            codes, logits = nat.plm_infer(dev(cond), lens, return_logits=True, prefix_codes=prefix, sampling=S(1.0),
                                          seeds=seeds.astype(np.int64))
            codes, logits = codes.cpu().numpy(), logits.cpu().numpy()
            n_diff = 0
            for b in range(B):
                us = uniform_np(seeds[b], np.arange(lens[b]))
                for j in range(lens[b]):
                    want, amb = draw(logits[b, j], 1.0, 0, 1.0, us[j])
                    n_diff += int(codes[b, j]) != want
                    assert amb or int(codes[b, j]) == want, (groups, b, j, int(codes[b, j]), want)
                assert not codes[b, lens[b]:].any()
            assert n_diff <= 1
    finally:
        nat.set_ar_groups(prev)


# ---------------------------------------------------------------------------------------------------
# 4. against the sampled oracle


def test_sampled_plm_against_the_oracle():
    tts = model("tiny")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    zs = [load_golden(f"tiny_utt{i}.npz") for i in range(4)]
    cond, ln = pad_stack([z["plm_cond"] for z in zs])
    seeds = np.asarray([3, 1 << 40, 77, 2 ** 63 + 5], np.uint64)
    for tau, k, pp in ((1.0, 0, 1.0), (0.8, 0, 0.95)):
        got = tts.native.plm_infer(dev(cond), ln, sampling=S(tau, k, pp), seeds=seeds.astype(np.int64)).cpu().numpy()
        for b, z in enumerate(zs):
            want, amb = plm_infer_sampled(sd_p, p, z["plm_cond"], tau, k, pp, int(seeds[b]))
            n = int(np.argmax(amb)) if amb.any() else want.size          # compared up to the first ambiguous step
            assert np.array_equal(got[b, :n], want[:n]), (tau, b, got[b, :n], want[:n])


# ---------------------------------------------------------------------------------------------------
# 5. invariance: batch vs alone, call vs call, and the draw is random


def test_sampled_batch_equals_each_utterance_alone_and_repeats():
    from megatts2_amd import synth
    tts = model("tiny")
    (g, *_), _ = synth_models("tiny")
    rng = np.random.Generator(np.random.PCG64(2024))
    utts = [synth.make_utterance(rng, n, t, f, g.mrte.phone_vocab_size)
            for n, t, f in ((7, 40, 29), (3, 19, 11), (11, 70, 45), (1, 17, 4), (9, 33, 30), (5, 50, 22), (13, 64, 60), (2, 20, 9))]
    phone, pl = pad_stack([u.phone for u in utts])
    mel, ml = pad_stack([u.prompt_mel for u in utts])
    dur, _ = pad_stack([u.durations for u in utts])
    seeds = np.arange(8, dtype=np.int64) * 1_000_003 + 11
    smp = S(1.2, 0, 0.97)
    out, lens, aux = tts.synthesize(dev(phone), dev(mel), pl, ml, forced_durations=dur, return_aux=True, sampling=smp, seeds=seeds)
    out2, _, aux2 = tts.synthesize(dev(phone), dev(mel), pl, ml, forced_durations=dur, return_aux=True, sampling=smp, seeds=seeds)
    assert torch.equal(out, out2) and torch.equal(aux["codes"], aux2["codes"])
    for i, u in enumerate(utts):
        m1, l1, a1 = tts.synthesize(dev(u.phone[None]), dev(u.prompt_mel[None]), forced_durations=u.durations[None],
                                    return_aux=True, sampling=smp, seeds=[int(seeds[i])])
        nq = -(-int(l1[0]) // 8)
        assert l1[0] == lens[i]
        assert torch.equal(a1["codes"][0, :nq], aux["codes"][i, :nq]), i
        assert O.rel_l2(m1[0, :l1[0]].cpu().numpy(), out[i, :lens[i]].cpu().numpy()) < 2e-6


def test_many_seeds_give_distinct_codes_where_the_distribution_is_flat():
    tts = model("tiny")
    rng = np.random.default_rng(5)
    conds = [load_golden(f"tiny_utt{i}.npz")["plm_cond"] for i in range(4)]
    conds += [np.maximum(rng.standard_normal((6, 64)), 0).astype(np.float32) * s for s in (0.5, 1.0, 2.0)]
    checked = 0
    tau = 4.0
    for c in conds:
        B = 256
        cb = dev(np.stack([c] * B))
        codes, logits = tts.native.plm_infer(cb, np.full(B, c.shape[0], np.int32), return_logits=True, max_steps=1,
                                             sampling=S(tau), seeds=np.arange(B, dtype=np.int64) * 7919)
        z = logits[0, 0].cpu().numpy().astype(np.float64)
        pr = np.exp((z - z.max()) / tau)
        pr /= pr.sum()
        if pr.max() < 0.99:            # the condition comes from the logits (position 0 does not depend on the seed)
            checked += 1
            assert len(set(codes[:, 0].cpu().numpy().tolist())) >= 2
    assert checked >= 1


# ---------------------------------------------------------------------------------------------------
# 6. pipeline consistency


def test_sampled_synthesis_codes_equal_the_sampled_plm_on_the_same_conditioning():
    tts = model("tiny")
    nat = tts.native
    zs = [load_golden(f"tiny_utt{i}.npz") for i in range(4)]
    phone, pl = pad_stack([z["phone"] for z in zs])
    mel, ml = pad_stack([z["prompt_mel"] for z in zs])
    dur, _ = pad_stack([z["forced_dur"] for z in zs])
    seeds = np.asarray([8, 6, 7, 5], np.int64)
    smp = S(0.9, 200, 0.9)
    out, lens, aux = nat.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, return_aux=True, sampling=smp, seeds=seeds)
    tc = nat.tc_latent(dev(phone), dev(mel), pl, ml)
    cond = nat.max_pool_ceil(nat.length_regulate(tc, dur, pl), 8, lens)
    tq = -(-lens // 8)
    codes = nat.plm_infer(cond, tq, sampling=smp, seeds=seeds)
    for b in range(4):
        assert torch.equal(codes[b, :tq[b]], aux["codes"][b, :tq[b]]), b
    forced, flens = nat.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, forced_codes=aux["codes"], run_plm=False)
    assert torch.equal(forced, out) and flens.tolist() == lens.tolist()


# ---------------------------------------------------------------------------------------------------
# 7. the range guard repeats a sampled call with the same draws


def test_range_guard_repeat_of_a_sampled_call():
    tts = model("prod")
    nat = tts.native
    z = load_golden("prod_utt0.npz")
    B = 8
    phone = dev(np.stack([z["phone"]] * B))
    big = dev(np.stack([z["prompt_mel"]] * B).astype(np.float32) * np.float32(3e4))
    fd = np.stack([z["forced_dur"]] * B)
    kw = dict(forced_dur=fd, skip_adm=True, return_aux=True, sampling=S(1.0, 0, 0.95), seeds=np.arange(B, dtype=np.int64) + 40)
    x3h = nat.get_option("x3h")
    n0 = nat.range_fallbacks
    got, gl, ga = nat.synthesize_batch(phone, None, big, None, **kw)
    assert nat.range_fallbacks == n0 + 1 and nat.get_option("x3h") == x3h
    nat.set_option("x3h", 0)
    try:
        want, wl, wa = nat.synthesize_batch(phone, None, big, None, **kw)
    finally:
        nat.set_option("x3h", x3h)
    assert torch.equal(got, want) and torch.equal(ga["codes"], wa["codes"]) and gl.tolist() == wl.tolist()
