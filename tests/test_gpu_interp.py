"""Prosody interpolation on the GPU (sample_mix_rows_kernel, the pair mode of the AR driver, mt2_plm_infer_interpolated and the
Python surfaces): the kernel against the float64 rule (tests/interp_ref.py), planted ties, the end points gamma = 0 / 1, every
step of the AR loop against the rule on the GPU's own logits, the interpolated oracle loop, batch / call invariance, the
synthesis pipeline and the errors of the entry point.

A decision is "ambiguous" where interp_ref flags it (within 1e-4 relative of a draw boundary, a cut or - greedy - of the
runner-up): float64 and the kernel's f32 may then disagree.  Every other decision must match exactly; in the kernel test the
disagreements themselves stay at or below 0.1 % (tests/test_interp_host.py caps the ambiguous share of its inputs at 10 %)."""
import ctypes

import numpy as np
import pytest

import interp_ref as I
import megatts2_oracle as O
from conftest import load_golden, synth_models
from interp_ref import mix_draw, mix_draw_many, plm_infer_interpolated_ref
from sampling_ref import draw, uniform_np
from test_gpu_sampling import S, chi2_isf_1e6, dev, model, pad_stack

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


def first_true(mask):
    return int(np.argmax(mask)) if mask.any() else mask.size


# ---------------------------------------------------------------------------------------------------
# 1. the kernel alone


def _kernel_case(zA, zB, ld, A, tau, k, p, g):
    from megatts2_amd.runtime import op_sample_mix_rows
    N = zA.size
    rows = np.full((2 * A, ld), 1e30, np.float32)          # columns behind N hold a value that would win every draw if read
    rows[0::2, :N] = zA
    rows[1::2, :N] = zB
    pos = I.kernel_positions(A)
    buf = dev(rows)
    got2 = op_sample_mix_rows(buf[:, :N] if ld != N else buf, S(tau, k, p), dev(np.full(A, I.KERNEL_SEED, np.int64)), dev(pos),
                              dev(np.full(A, g, np.float32))).cpu().numpy()
    assert np.array_equal(got2[0::2], got2[1::2]), "the two histories of a pair received different codes"
    got = got2[0::2]
    want, amb, R, pr = mix_draw_many(zA, zB, g, tau, k, p, uniform_np(I.KERNEL_SEED, pos))
    assert np.isin(got, R).all(), "a choice outside K / R"
    bad = (got != want) & ~amb
    print(f"N={N} ld={ld} tau={tau} k={k} p={p} gamma={g}: {int((got != want).sum())} of {A} differ, {int(amb.sum())} ambiguous")
    assert not bad.any(), (int(bad.sum()), np.flatnonzero(bad)[:8])
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


@pytest.mark.parametrize("tau,k,p,g", I.KERNEL_CASES)
def test_op_sample_mix_rows_against_the_float64_rule(tau, k, p, g):
    zA, zB = I.kernel_rows()
    _kernel_case(zA, zB, 1024, I.KERNEL_PAIRS, tau, k, p, g)


@pytest.mark.parametrize("ld", [41, 44])        # unaligned rows: scalar loads; aligned rows: lanes 0-1 load float4, lane 2 the tail
def test_op_sample_mix_rows_tail_and_row_stride(ld):
    from megatts2_amd.runtime import op_sample_mix_rows
    zA, zB = (z[:I.TAIL_N] for z in I.kernel_rows())
    for tau, k, p, g in I.TAIL_CASES:
        _kernel_case(zA, zB, ld, I.TAIL_PAIRS, tau, k, p, g)
    rows = np.full((2, ld), 1e30, np.float32)
    rows[0, :I.TAIL_N], rows[1, :I.TAIL_N] = zA, zB
    got = op_sample_mix_rows(dev(rows)[:, :I.TAIL_N], None, None, None, dev(np.asarray([0.5], np.float32))).cpu().numpy()
    assert got.tolist() == [I.mix_greedy(zA, zB, 0.5)[0]] * 2


# ---------------------------------------------------------------------------------------------------
# 2. planted ties


def test_op_sample_mix_rows_lowest_index_wins_planted_ties():
    from megatts2_amd.runtime import op_sample_mix_rows
    rng = np.random.default_rng(7)
    A = 512
    z = (rng.standard_normal((2 * A, 1024)) * 3).astype(np.float32)
    want = np.zeros(A, np.int64)
    for r in range(A):      # the same values at the same indices of both rows: exact ties of the maximum of m at every tau
        idx = np.sort(rng.choice(1024, 2 + r % 4, replace=False))
        z[2 * r, idx] = z[2 * r].max() + 1.0 + float(r % 3)
        z[2 * r + 1, idx] = z[2 * r + 1].max() + 2.0
        want[r] = idx[0]
    gm = dev(np.full(A, 0.5, np.float32))
    zd = dev(z)
    got = op_sample_mix_rows(zd, None, None, None, gm).cpu().numpy()
    assert np.array_equal(got[0::2], want) and np.array_equal(got[1::2], want)
    pos = dev(np.arange(A, dtype=np.int32))
    for tau in (1.0, 0.2, 5.0):
        for smp in (S(tau, 1, 1.0), S(tau, 1, 0.3), S(tau, 0, 1e-7)):
            got = op_sample_mix_rows(zd, smp, dev(rng.integers(0, 2 ** 62, A)), pos, gm).cpu().numpy()
            assert np.array_equal(got[0::2], want) and np.array_equal(got[1::2], want), (tau, smp)


# ---------------------------------------------------------------------------------------------------
# 3. the end points leave the other context out


def test_end_points_decode_one_context_alone():
    tts = model("tiny")
    nat = tts.native
    zs = [load_golden(f"tiny_utt{i}.npz") for i in range(4)]
    cond, ln = pad_stack([z["plm_cond"] for z in zs])
    other = np.maximum(np.random.default_rng(11).standard_normal(cond.shape), 0).astype(np.float32)
    a, b = dev(cond), dev(other)
    for got in (nat.plm_infer_interpolated(a, b, ln, 0.0), nat.plm_infer_interpolated(b, a, ln, 1.0)):
        got = got.cpu().numpy()
        for i, z in enumerate(zs):
            assert np.array_equal(got[i, :ln[i]], z["p_codes"]), i
            assert not got[i, ln[i]:].any()
    # sampled: the same codes as the single-context sampler up to the first step either float64 rule calls ambiguous.  No top-p cut
    # here: over ~1000 near-flat bins the weight AT a top-p cut (~1.7e-4 of the mass) is of the order of the ambiguity margin itself,
    # so the reference would flag the cut at every step and nothing would be compared.
    seeds = np.arange(4, dtype=np.int64) * 977 + 5
    for tau, k in ((1.1, 0), (0.8, 40)):
        smp = S(tau, k, 1.0)
        one, lg1 = nat.plm_infer(a, ln, return_logits=True, sampling=smp, seeds=seeds)
        two, lg2 = nat.plm_infer_interpolated(a, b, ln, 0.0, return_logits=True, sampling=smp, seeds=seeds)
        one, lg1, two, lg2 = (t.cpu().numpy() for t in (one, lg1, two, lg2))
        compared = 0
        for i in range(4):
            us = uniform_np(np.uint64(seeds[i]), np.arange(ln[i]))
            amb = np.asarray([draw(lg1[i, j], tau, k, 1.0, us[j])[1] or mix_draw(lg2[0, i, j], lg2[1, i, j], 0.0, tau, k, 1.0, us[j])[1]
                              for j in range(ln[i])])
            n = first_true(amb)
            compared += n
            assert np.array_equal(one[i, :n], two[i, :n]), (tau, k, i, n, one[i, :n], two[i, :n])
        print(f"tau={tau} top_k={k}: {compared} of {int(ln.sum())} steps compared")
        assert compared > 0, "every utterance is ambiguous at its first step: nothing was compared"


# ---------------------------------------------------------------------------------------------------
# 4. every step of the pair-mode AR loop follows the rule on the GPU's own logits


@pytest.mark.parametrize("P", [0, 5])
def test_interpolated_plm_steps_follow_the_rule_under_every_grouping(P):
    tts = model("prod")
    nat = tts.native
    rng = np.random.default_rng(41 + P)
    lens = np.asarray([21, 13, 7, 21, 1, 16, 9, 12], np.int32)
    gamma = np.asarray([0, 1, 0.5, 0.25, 0.75, 0.5, 0.1, 0.9], np.float32)
    B, T = lens.size, int(lens.max())
    ca, cb = (dev(np.maximum(rng.standard_normal((B, P + T, 512)), 0).astype(np.float32)) for _ in range(2))
    pa, pb = (dev(rng.integers(0, 1024, (B, P))) for _ in range(2)) if P else (None, None)
    seeds = rng.integers(0, 2 ** 63, B).astype(np.uint64)
    prev = nat.get_option("ar_groups")
    try:
        for groups in (1, 2, 4):
            nat.set_ar_groups(groups)
            for tau in (1.0, None):
                kw = dict(sampling=S(tau), seeds=seeds.astype(np.int64)) if tau else {}
                codes, logits = nat.plm_infer_interpolated(ca, cb, lens, gamma, prefix_a=pa, prefix_b=pb, return_logits=True, **kw)
                codes, logits = codes.cpu().numpy(), logits.cpu().numpy()
                n_diff = 0
                for b in range(B):
                    us = uniform_np(seeds[b], np.arange(lens[b]))
                    for j in range(lens[b]):
                        want, amb = mix_draw(logits[0, b, j], logits[1, b, j], gamma[b], tau, 0, 1.0, us[j])
                        n_diff += int(codes[b, j]) != want
                        assert amb or int(codes[b, j]) == want, (groups, tau, b, j, int(codes[b, j]), want)
                    assert not codes[b, lens[b]:].any() and not logits[:, b, lens[b]:].any()
                    assert not np.array_equal(logits[0, b, :lens[b]], logits[1, b, :lens[b]]), "one context, not two"
                assert n_diff <= 1
    finally:
        nat.set_ar_groups(prev)


# ---------------------------------------------------------------------------------------------------
# 5. against the interpolated oracle loop


def test_interpolated_plm_against_the_oracle_loop():
    tts = model("tiny")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    zs = [load_golden(f"tiny_utt{i}.npz") for i in range(4)]
    cond, ln = pad_stack([z["plm_cond"] for z in zs])
    rev, _ = pad_stack([z["plm_cond"][::-1] for z in zs])
    seeds = np.asarray([3, 1 << 40, 77, 2 ** 63 + 5], np.uint64)
    for smp in (None, (0.8, 0, 0.95), (0.8, 40, 1.0)):      # (the last: no top-p cut, whose own ambiguity ends most comparisons early)
        kw = dict(sampling=S(*smp), seeds=seeds.astype(np.int64)) if smp else {}
        got = tts.native.plm_infer_interpolated(dev(cond), dev(rev), ln, 0.5, **kw).cpu().numpy()
        tau, k, pp = smp if smp else (None, 0, 1.0)
        for b, z in enumerate(zs):
            want, amb = plm_infer_interpolated_ref(sd_p, p, z["plm_cond"], np.ascontiguousarray(z["plm_cond"][::-1]), 0.5, tau, k, pp,
                                                   int(seeds[b]))
            n = first_true(amb)          # compared up to the first ambiguous step
            assert np.array_equal(got[b, :n], want[:n]), (smp, b, got[b, :n], want[:n])


# ---------------------------------------------------------------------------------------------------
# 6. invariance: batch vs alone, call vs call


def test_interpolated_batch_equals_each_utterance_alone_and_repeats():
    tts = model("tiny")
    nat = tts.native
    rng = np.random.default_rng(2025)
    lens = np.asarray([9, 4, 1, 7, 9, 3, 6, 2], np.int32)
    B, T, P = lens.size, int(lens.max()), 3
    ca, cb = (dev(np.maximum(rng.standard_normal((B, P + T, 64)), 0).astype(np.float32)) for _ in range(2))
    pa, pb = (dev(rng.integers(0, 1024, (B, P))) for _ in range(2))
    gamma = np.asarray([0.5, 0.2, 0.9, 0.0, 1.0, 0.35, 0.65, 0.5], np.float32)
    seeds = np.arange(B, dtype=np.int64) * 1_000_003 + 11
    for smp in (None, S(1.2, 0, 0.97)):
        kw = lambda sd: dict(sampling=smp, seeds=sd) if smp else {}
        full = nat.plm_infer_interpolated(ca, cb, lens, gamma, prefix_a=pa, prefix_b=pb, **kw(seeds))
        again = nat.plm_infer_interpolated(ca, cb, lens, gamma, prefix_a=pa, prefix_b=pb, **kw(seeds))
        assert torch.equal(full, again)
        for i in range(B):
            n = P + int(lens[i])
            one = nat.plm_infer_interpolated(ca[i:i + 1, :n], cb[i:i + 1, :n], lens[i:i + 1], gamma[i:i + 1], prefix_a=pa[i:i + 1],
                                             prefix_b=pb[i:i + 1], **kw(seeds[i:i + 1]))
            assert torch.equal(one[0], full[i, :lens[i]]), (i, one[0], full[i])


# ---------------------------------------------------------------------------------------------------
# 7. the synthesis pipeline


@pytest.mark.parametrize("kind", ["tiny", "prod"])
def test_synthesize_prosody_interpolated(kind):
    tts = model(kind)
    nat = tts.native
    z = load_golden(f"{kind}_prompted.npz")
    phone, mel = dev(z["phone"][None]), dev(z["prompt_mel"][None])
    pp, pd = dev(z["prompt_phone"][None]), z["prompt_dur"][None]
    # the rhythm prompt: the same prompt with its mel reversed in time, its phones and alignment reversed with it (same P)
    rmel = dev(np.ascontiguousarray(z["prompt_mel"][::-1])[None])
    rp, rd = dev(np.ascontiguousarray(z["prompt_phone"][::-1])[None]), np.ascontiguousarray(z["prompt_dur"][::-1])[None]
    fd = z["forced_dur"][None]
    args = (phone, mel, pp, pd, rmel, rp, rd)
    out, lens, aux = tts.synthesize_prosody_interpolated(*args, 0.0, forced_durations=fd, return_aux=True)
    n = z["mel"].shape[0]
    assert int(lens[0]) == n
    assert np.array_equal(aux["codes"][0, :z["p_codes"].size].cpu().numpy(), z["p_codes"])
    assert np.array_equal(aux["prompt_codes"][0].cpu().numpy(), z["prompt_codes"])
    assert O.rel_l2(out[0, :n].cpu().numpy(), z["mel"]) < 1e-3
    # sampled at gamma = 0.5: the codes are those of plm_infer_interpolated on the staged conditioning, the mel that of those codes
    smp, seeds = S(0.9, 200, 0.95), np.asarray([4242], np.int64)
    out, lens, aux = tts.synthesize_prosody_interpolated(*args, 0.5, forced_durations=fd, return_aux=True, sampling=smp, seeds=seeds)
    st = tts.generator.cfg.vqpe.stride
    ml = np.asarray([z["prompt_mel"].shape[0]], np.int32)

    def pooled(ph, m, d):
        tc = nat.tc_latent(ph, m)
        return nat.max_pool_ceil(nat.length_regulate(tc, d), st, ml), nat.vqpe_forward(m)[1][0]

    cond_a, codes_a = pooled(pp, mel, pd)
    cond_b, codes_b = pooled(rp, rmel, rd)
    len_t = np.asarray([int(fd.sum())], np.int32)
    cond_t = nat.max_pool_ceil(nat.length_regulate(nat.tc_latent(phone, mel), fd), st, len_t)
    q_t = -(-len_t // st)
    codes = nat.plm_infer_interpolated(torch.cat([cond_a, cond_t], 1), torch.cat([cond_b, cond_t], 1), q_t, 0.5, prefix_a=codes_a,
                                       prefix_b=codes_b, sampling=smp, seeds=seeds)
    assert torch.equal(codes[0, :q_t[0]], aux["codes"][0, :q_t[0]])
    assert not torch.equal(codes_a, codes_b), "the rhythm prompt's codes equal the timbre prompt's: the test has one context"
    forced, flens = nat.synthesize_batch(phone, None, mel, None, forced_dur=fd, forced_codes=aux["codes"], run_plm=False)
    assert torch.equal(forced, out) and flens.tolist() == lens.tolist()
    # a rhythm prompt of another pooled length: 8 more frames, given to its last phone
    longer = dev(np.concatenate([z["prompt_mel"][::-1], z["prompt_mel"][:st]])[None])
    rd2 = rd.copy()
    rd2[0, -1] += st
    with pytest.raises(ValueError, match="pooled length"):
        tts.synthesize_prosody_interpolated(phone, mel, pp, pd, longer, rp, rd2, 0.5, forced_durations=fd)


# ---------------------------------------------------------------------------------------------------
# 8. errors through the handle


def test_interpolated_errors_name_the_field_and_leave_the_handle_usable():
    from megatts2_amd.runtime import NativeError, _iptr, _ptr, _stream
    tts = model("tiny")
    nat = tts.native
    z = load_golden("tiny_utt0.npz")
    cond = dev(z["plm_cond"][None])
    T = cond.shape[1]
    want = nat.plm_infer_interpolated(cond, cond, None, 0.5)
    both = torch.stack([cond, cond])
    ln = np.asarray([T], np.int32)
    codes = torch.zeros(1, T, device=cond.device, dtype=torch.int64)

    def raw(gamma, prefix, P, Tq):
        g = np.asarray([gamma], np.float32)
        lq = np.asarray([Tq], np.int32)
        return nat.lib.mt2_plm_infer_interpolated(nat.h, _stream(), _ptr(both), _iptr(lq), Tq, 1, _ptr(prefix), P, _iptr(g), 0,
                                                  _ptr(codes), None, None)

    for gm in (-0.1, 1.5, float("nan")):
        assert raw(gm, None, 0, T) != 0 and b"gamma" in nat.lib.mt2_last_error()
    assert nat.lib.mt2_plm_infer_interpolated(nat.h, _stream(), _ptr(both), _iptr(ln), T, 1, None, 0, None, 0, _ptr(codes), None,
                                              None) != 0 and b"gamma" in nat.lib.mt2_last_error()
    assert raw(0.5, None, 2, T - 2) != 0 and b"prefix_codes" in nat.lib.mt2_last_error()
    with pytest.raises(ValueError, match="gamma"):
        nat.plm_infer_interpolated(cond, cond, None, 1.5)
    ok = dev(np.full((1, T - 1), 5, np.int64))
    bad = dev(np.full((1, T - 1), 1026, np.int64))          # vq_bins + 2: one past the last row of pc_embedding
    for pa, pb in ((bad, ok), (ok, bad)):
        with pytest.raises(NativeError, match="prompt prosody code"):
            nat.plm_infer_interpolated(cond, cond, np.asarray([1], np.int32), 0.5, prefix_a=pa, prefix_b=pb)
    assert torch.equal(nat.plm_infer_interpolated(cond, cond, None, 0.5), want)
