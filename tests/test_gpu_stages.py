"""Stage-level parity (GPU): the HIP path, called through the C ABI via the drop-in mirror classes,
against (a) the committed golden fixtures produced by the LIVE reference modules and (b) the CPU
oracle on seeded ragged batches.  Stage-wise with teacher forcing, then end to end.

Tolerances: floating-point outputs 1e-3 relative L2 as BASELINE.json's north_star states (the HIP
path actually lands around 1e-6, asserted at 2e-5 where nothing is amplified); VQ indices, PLM codes
and integer durations bit-exact.
"""
import os
import numpy as np
import pytest

import megatts2_oracle as O
from conftest import GOLDEN, load_golden, synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

TIGHT = 2e-5
NORTH_STAR = 1e-3


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pad_stack(arrs, dtype=None):
    n = max(a.shape[0] for a in arrs)
    out = np.zeros((len(arrs), n) + arrs[0].shape[1:], dtype or arrs[0].dtype)
    for i, a in enumerate(arrs):
        out[i, :a.shape[0]] = a
    return out, np.asarray([a.shape[0] for a in arrs], np.int32)


_MODELS = {}


def model(kind):
    """One combined native handle (G + PLM + ADM + vocoder) per model size, with the mirror classes."""
    if kind not in _MODELS:
        from megatts2_amd import megatts2 as M
        (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models(kind)
        tts = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)),
                        hifi_gan=M.HIFIGAN(h, sd_h))
        # MT2_TEST_OPTS="x6_ks=5,attn_x6_min=448": run the whole parity suite under non-default engine options (A/B of a
        # candidate default before it is made one - every discrete output must stay bit-exact under it)
        for kv in filter(None, os.environ.get("MT2_TEST_OPTS", "").split(",")):
            k, v = kv.split("=")
            tts.native.set_option(k, int(v))
        _MODELS[kind] = tts
    return _MODELS[kind]


@pytest.fixture(scope="module")
def tiny_batch():
    return [load_golden(f"tiny_utt{i}.npz") for i in range(4)]


# ---------------------------------------------------------------------------------------------------
# golden fixtures (reference modules), ragged batch of 4 tiny utterances incl. a 1-phone utterance


def test_tiny_tc_latent_batch(tiny_batch):
    tts = model("tiny")
    phone, pl = pad_stack([z["phone"] for z in tiny_batch])
    mel, ml = pad_stack([z["prompt_mel"] for z in tiny_batch])
    out = tts.generator.mrte.tc_latent(dev(phone), dev(mel), phone_lens=pl, mel_lens=ml).cpu().numpy()
    for i, z in enumerate(tiny_batch):
        assert O.rel_l2(out[i, :pl[i]], z["tc_latent"]) < TIGHT
        assert not out[i, pl[i]:].any()
    ctx = tts.native.mel_context(dev(mel), ml).cpu().numpy()
    for i, z in enumerate(tiny_batch):
        n = z["mel_context"].shape[0]
        assert O.rel_l2(ctx[i, :n], z["mel_context"]) < TIGHT


def test_tiny_each_utterance_alone_equals_batched(tiny_batch):
    """Batch semantics N1: an utterance computed alone == the same utterance inside a ragged batch."""
    tts = model("tiny")
    phone, pl = pad_stack([z["phone"] for z in tiny_batch])
    mel, ml = pad_stack([z["prompt_mel"] for z in tiny_batch])
    batched = tts.native.tc_latent(dev(phone), dev(mel), pl, ml).cpu().numpy()
    for i, z in enumerate(tiny_batch):
        alone = tts.generator.mrte.tc_latent(dev(z["phone"][None]), dev(z["prompt_mel"][None])).cpu().numpy()[0]
        assert O.rel_l2(alone, batched[i, :pl[i]]) < 2e-6


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_tiny_random_ragged_batches_against_oracle(seed):
    """Seeded random ragged batches (1-phone utterances, minimum-length prompts, equal lengths, up to 9
    utterances): the whole pipeline with forced durations and the vocoder, every utterance against the
    oracle run alone - mel within tolerance, ADM durations and PLM codes bit-exact, padding zero."""
    from megatts2_amd import synth
    tts = model("tiny")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    rng = np.random.Generator(np.random.PCG64(100 + seed))
    B = int(rng.integers(2, 10))
    utts = []
    for i in range(B):
        n_ph = 1 if i == 0 else int(rng.integers(1, 14))
        n_pr = 17 if i == 1 else int(rng.integers(17, 80))          # >= 17 frames: one stride-16 window + 1
        n_fr = n_ph * int(rng.integers(1, 6)) + int(rng.integers(0, n_ph))
        utts.append(synth.make_utterance(rng, n_ph, n_pr, max(n_fr, n_ph), g.mrte.phone_vocab_size))
    if B > 3:
        utts[3] = synth.make_utterance(rng, utts[2].phone.size, utts[2].prompt_mel.shape[0], int(utts[2].durations.sum()),
                                       g.mrte.phone_vocab_size)    # two utterances of identical geometry
    phone, pl = pad_stack([u.phone for u in utts])
    mel, ml = pad_stack([u.prompt_mel for u in utts])
    dur, _ = pad_stack([u.durations for u in utts])
    out, lens, aux = tts.native.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, vocoder=True,
                                                 return_aux=True)
    out = out.cpu().numpy()
    for i, u in enumerate(utts):
        ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, u.phone, u.prompt_mel, forced_durations=u.durations)
        n = ref["mel"].shape[0]
        assert lens[i] == n
        assert np.array_equal(aux["dur"][i, :pl[i]].cpu().numpy(), ref["adm_dur"])
        assert np.array_equal(aux["codes"][i, :ref["p_codes"].size].cpu().numpy(), ref["p_codes"])
        assert O.rel_l2(out[i, :n], ref["mel"]) < NORTH_STAR
        assert not out[i, n:].any()
        wav = O.hifigan(sd_h, h, ref["mel"])
        assert O.rel_l2(aux["wav"][i, :wav.size].cpu().numpy(), wav) < NORTH_STAR


def test_tiny_adm(tiny_batch):
    tts = model("tiny")
    tc, ln = pad_stack([z["tc_latent"] for z in tiny_batch])
    dur, flt = tts.native.adm_infer(dev(tc), ln, return_float=True)
    dur, flt = dur.cpu().numpy(), flt.cpu().numpy()
    for i, z in enumerate(tiny_batch):
        assert np.allclose(flt[i, :ln[i]], z["adm_float"], rtol=1e-4, atol=1e-4)
        assert np.array_equal(dur[i, :ln[i]], z["adm_dur"])
        assert not dur[i, ln[i]:].any()
    # mirror surface: int32 [B, Np, 1]
    d3 = tts.adm.infer(dev(tiny_batch[0]["tc_latent"][None]))
    assert d3.shape == (1, tiny_batch[0]["tc_latent"].shape[0], 1) and d3.dtype == torch.int32


@pytest.mark.parametrize("groups", [1, 2, 3])
def test_tiny_ar_stream_groups_do_not_change_results(tiny_batch, groups):
    """The AR loops split the batch into independent kernel chains on internal streams (mt2_set_ar_groups);
    every grouping must give the reference's discrete outputs and the same floats."""
    tts = model("tiny")
    tts.native.set_ar_groups(groups)
    try:
        tc, ln = pad_stack([z["tc_latent"] for z in tiny_batch])
        dur, flt = tts.native.adm_infer(dev(tc), ln, return_float=True)
        cond, lq = pad_stack([z["plm_cond"] for z in tiny_batch])
        codes = tts.native.plm_infer(dev(cond), lq)
        torch.cuda.synchronize()
        for i, z in enumerate(tiny_batch):
            assert np.allclose(flt[i, :ln[i]].cpu().numpy(), z["adm_float"], rtol=1e-4, atol=1e-4)
            assert np.array_equal(dur[i, :ln[i]].cpu().numpy(), z["adm_dur"])
            assert np.array_equal(codes[i, :lq[i]].cpu().numpy(), z["p_codes"])
    finally:
        tts.native.set_ar_groups(2)


def test_tiny_regulate_and_pool(tiny_batch):
    tts = model("tiny")
    tc, ln = pad_stack([z["tc_latent"] for z in tiny_batch])
    dur, _ = pad_stack([z["forced_dur"] for z in tiny_batch])
    out = tts.lr(dev(tc), dur, lens=ln).cpu().numpy()
    for i, z in enumerate(tiny_batch):
        ref = O.length_regulate(z["tc_latent"], z["forced_dur"])
        assert np.array_equal(out[i, :ref.shape[0]], ref)          # gather: bit-exact
        assert not out[i, ref.shape[0]:].any()
        cond = tts.native.max_pool_ceil(dev(ref[None]), 8).cpu().numpy()[0]
        assert np.array_equal(cond, z["plm_cond"])
    # the reference's only hot-path assertion (modules/mrte.py:186-194) and the SURVEY KAT
    x = torch.randn(2, 10, 128).cuda()
    d = np.asarray([[1, 2, 3, 4] + [0] * 6, [1, 2, 3, 5] + [0] * 6], np.int32)
    assert tuple(tts.lr(x, d).shape) == (2, 11, 128)
    kat = tts.lr(dev(np.arange(8, dtype=np.float32).reshape(1, 4, 2)), np.asarray([[1, 2, 0, 3]], np.int32))
    assert kat[0].cpu().tolist() == [[0, 1], [2, 3], [2, 3], [6, 7], [6, 7], [6, 7]]      # odd width: scalar path


def test_tiny_plm(tiny_batch):
    tts = model("tiny")
    cond, ln = pad_stack([z["plm_cond"] for z in tiny_batch])
    codes, logits = tts.native.plm_infer(dev(cond), ln, return_logits=True)
    codes, logits = codes.cpu().numpy(), logits.cpu().numpy()
    for i, z in enumerate(tiny_batch):
        assert np.array_equal(codes[i, :ln[i]], z["p_codes"])
        assert O.rel_l2(logits[i, :ln[i]], z["plm_logits"]) < 1e-4


def test_tiny_decoder_and_vq_decode(tiny_batch):
    tts = model("tiny")
    x, ln = pad_stack([z["decoder_in"] for z in tiny_batch])
    mel = tts.generator.decoder(dev(x).transpose(1, 2).contiguous(), lens=ln).cpu().numpy()     # "B D T"
    for i, z in enumerate(tiny_batch):
        assert O.rel_l2(mel[i, :, :ln[i]].T, z["mel"]) < TIGHT
        assert not mel[i, :, ln[i]:].any()
    z = tiny_batch[0]
    zq = tts.generator.vqpe.vq.decode(dev(z["p_codes"][None, None])).cpu().numpy()[0]            # [256, T]
    (g, *_), (sd_g, *_) = synth_models("tiny")
    assert np.array_equal(zq.T, O.vq_decode(sd_g[O.CODEBOOK], z["p_codes"]))


def test_tiny_vqpe(tiny_batch):
    tts = model("tiny")
    mel, ln = pad_stack([z["target_mel"] for z in tiny_batch])
    zq, codes, ze = tts.native.vqpe_forward(dev(mel), ln, return_ze=True)
    zq, codes, ze = zq.cpu().numpy(), codes.cpu().numpy(), ze.cpu().numpy()
    for i, z in enumerate(tiny_batch):
        tq = z["vqpe_codes"].shape[0]
        assert O.rel_l2(ze[i, :tq], z["vqpe_ze"]) < TIGHT
        assert np.array_equal(codes[0, i, :tq], z["vqpe_codes"])            # bit-exact VQ indices
        assert np.array_equal(zq[i, :ln[i]], z["vqpe_zq"])
    # mirror surface: (zq, commit_loss, vq_loss, codes)
    r = tts.generator.vqpe(dev(tiny_batch[0]["target_mel"][None]))
    assert len(r) == 4 and r[3].shape[0] == 1


def test_tiny_mirror_surfaces_of_the_reference_classes(tiny_batch):
    """The drop-in classes expose the reference's sub-surfaces with its layouts: MRTE.mel_encoder ("B D T"),
    MRTE.tc_latent with 2 or 3 positional arguments, RVQ encode/decode ([n_q, B, T] <-> "B D T")."""
    tts = model("tiny")
    (g, p, a, h), (sd_g, *_) = synth_models("tiny")
    z = tiny_batch[2]
    mel_bdt = dev(z["prompt_mel"].T[None].copy())
    ctx = tts.generator.mrte.mel_encoder(mel_bdt).cpu().numpy()[0].T
    assert O.rel_l2(ctx, z["mel_context"]) < TIGHT
    phone, pm = dev(z["phone"][None]), dev(z["prompt_mel"][None])
    t2 = tts.generator.mrte.tc_latent(phone, pm)
    t3 = tts.generator.mrte.tc_latent(phone, np.asarray([z["phone"].size], np.int32), pm)
    assert torch.equal(t2, t3) and O.rel_l2(t2[0].cpu().numpy(), z["tc_latent"]) < TIGHT
    ze = dev(z["vqpe_ze"].T[None].copy())                                  # "b d n"
    codes = tts.generator.vqpe.vq.encode(ze)
    assert tuple(codes.shape) == (1, 1, z["vqpe_codes"].size) and codes.dtype == torch.int64
    assert np.array_equal(codes[0, 0].cpu().numpy(), z["vqpe_codes"])
    zq = tts.generator.vqpe.vq.decode(codes).cpu().numpy()[0].T            # [B, D, T] -> [T, D]
    assert np.array_equal(zq, sd_g[O.CODEBOOK][z["vqpe_codes"]])
    w, ws = tts.native.memory()
    assert w > 0 and ws > 0


@pytest.mark.parametrize("kind", ["tiny", "prod"])
def test_vq_quantize_near_ties_against_the_live_reference(kind):
    """L2-argmin (EuclideanCodebook.quantize, core_vq.py:175-183) pinned to the LIVE reference: the fixture
    tests/golden/{kind}_vq_near_ties.npz holds the reference's own indices on 512 exact hits, 512 engineered near-ties and random
    rows (tiny: 4 096 rows, prod: 10^5; oracle/make_golden.py --extra-vq).  Three counts are reported - HIP vs reference, HIP vs
    the numpy port, port vs reference.  Exact hits and random rows: 0 flips against the reference.  Engineered near-ties: the
    argmax lies inside the f32 round-off of the expanded distance (the reference itself disagrees with float64 arithmetic and
    with the numpy port there), so a flip is legitimate only if the two picks' float64 scores differ by less than 16 f32 roundings
    of the distance's terms (asserted for EVERY flip against the reference, not only for those beyond the port's count) - and the
    HIP kernel may not sit further from exact arithmetic than the reference itself does (flips against the float64 argmax: the
    reference 8 / 163, the HIP kernel 14 / 168 on the tiny / production rows when the fixture was made)."""
    import hashlib
    tts = model(kind)
    z = load_golden(f"{kind}_vq_near_ties.npz")
    E = np.load(os.path.join(GOLDEN, f"codebook_{kind}.npy"))
    x = O.vq_near_tie_rows(E, int(z["n_rows"]), int(z["seed"]))
    assert hashlib.sha256(x.tobytes()).digest() == z["x_sha256"].tobytes()
    ref = z["ref_idx"].astype(np.int64)
    got = tts.native.vq_quantize(dev(x)).cpu().numpy()
    port = O.vq_quantize(E, x)
    hip_ref, hip_port, port_ref = (np.nonzero(a != b)[0] for a, b in ((got, ref), (got, port), (port, ref)))
    if os.path.isdir("gpurun_out"):      # the observed counts are quoted in DESIGN.md
        with open(f"gpurun_out/vq_near_tie_flips_{kind}.txt", "w") as fh:
            fh.write(f"{kind}: rows {x.shape[0]} (512 exact hits, 512 engineered near-ties): index flips HIP vs live reference = "
                     f"{hip_ref.size}, HIP vs numpy port = {hip_port.size}, numpy port vs live reference = {port_ref.size}; "
                     f"live reference vs float64 argmax = {int((ref != z['best64'].astype(np.int64)).sum())}, HIP vs float64 argmax = "
                     f"{int((got != z['best64'].astype(np.int64)).sum())}\n")
    assert np.array_equal(got[:512], ref[:512]), "exact hits: the row itself (or an earlier identical row) is returned"
    assert np.array_equal(got[1024:], ref[1024:]), "flip on a row that is not an engineered near-tie"
    assert O.vq_flips_within_roundoff(E, x[hip_ref], got[hip_ref], ref[hip_ref]).all()
    b64 = z["best64"].astype(np.int64)
    assert int((got != b64).sum()) <= 1.25 * int((ref != b64).sum()) + 8


def test_fp16_range_guard_repeats_the_call_on_the_bf16_path():
    """Round 6 (gemm_x3h.hip): activations are split into fp16 planes at run time, so a value at or beyond 65 504 cannot be
    represented - every x3h launch tracks max |a| and raises the handle's guard word, and the host layer (`NativeModel._guarded`,
    `mt2_x3h_guard`) REPEATS the call with x3h off (the bf16 six-product form has f32's exponent range).  A prompt mel scaled by
    3e4 drives the mel encoder's first activations to ~1e5: the guarded call must (1) notice, (2) return exactly what a handle
    with x3h = 0 returns, (3) stay quiet on ordinary input, (4) leave the option as it found it."""
    tts = model("prod")
    nat = tts.native
    z = load_golden("prod_utt0.npz")
    B = 8
    phone = dev(np.stack([z["phone"]] * B))
    mel = np.stack([z["prompt_mel"]] * B).astype(np.float32)
    big = dev(mel * np.float32(3e4))
    x3h = nat.get_option("x3h")
    assert x3h != 0, "the fp16-pipe forms are the default"
    n0 = nat.range_fallbacks
    got = nat.tc_latent(phone, big)
    assert nat.range_fallbacks == n0 + 1 and nat.get_option("x3h") == x3h
    nat.set_option("x3h", 0)
    try:
        want = nat.tc_latent(phone, big)
    finally:
        nat.set_option("x3h", x3h)
    assert torch.isfinite(got).all() and torch.equal(got, want)
    ok = nat.tc_latent(phone, dev(mel))
    assert nat.range_fallbacks == n0 + 1 and not nat.range_guard()
    assert O.rel_l2(ok[0].cpu().numpy(), z["tc_latent"]) < NORTH_STAR


def test_tiny_end_to_end(tiny_batch):
    """Whole pipeline on the ragged batch: forced durations (the fixtures' frame counts), free-running PLM."""
    tts = model("tiny")
    phone, pl = pad_stack([z["phone"] for z in tiny_batch])
    mel, ml = pad_stack([z["prompt_mel"] for z in tiny_batch])
    dur, _ = pad_stack([z["forced_dur"] for z in tiny_batch])
    out, lens, aux = tts.synthesize(dev(phone), dev(mel), pl, ml, forced_durations=dur, return_aux=True)
    out = out.cpu().numpy()
    for i, z in enumerate(tiny_batch):
        n = z["mel"].shape[0]
        assert lens[i] == n
        assert np.array_equal(aux["dur"][i, :pl[i]].cpu().numpy(), z["adm_dur"])        # the ADM's own durations
        assert np.array_equal(aux["codes"][i, :z["p_codes"].shape[0]].cpu().numpy(), z["p_codes"])
        assert O.rel_l2(out[i, :n], z["mel"]) < NORTH_STAR
        assert not out[i, n:].any()


def test_tiny_end_to_end_own_durations(tiny_batch):
    """No forced durations: the ADM's integer durations size the output (one D2H sync)."""
    tts = model("tiny")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    z = tiny_batch[0]
    out, lens = tts.synthesize(dev(z["phone"][None]), dev(z["prompt_mel"][None]))
    ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, z["phone"], z["prompt_mel"])
    assert lens[0] == ref["mel"].shape[0] == int(z["adm_dur"].sum())
    assert O.rel_l2(out[0, :lens[0]].cpu().numpy(), ref["mel"]) < NORTH_STAR


@pytest.mark.parametrize("kind", ["tiny", "prod"])
def test_hifigan_stand_in(kind):
    tts = model(kind)
    z = load_golden(f"{kind}_hifigan.npz")
    mels = []
    i = 0
    while f"mel{i}" in z:
        mels.append(z[f"mel{i}"])
        i += 1
    mel, ln = pad_stack(mels)
    wav = tts.hifi_gan.decode_batch(dev(mel).transpose(1, 2).contiguous(), mel_lens=ln).cpu().numpy()
    hop = tts.hifi_gan.cfg.hop
    for i, m in enumerate(mels):
        n = m.shape[0] * hop
        assert O.rel_l2(wav[i, 0, :n], z[f"wav{i}"]) < NORTH_STAR
        assert not wav[i, 0, n:].any()


# ---------------------------------------------------------------------------------------------------
# production shapes: config C1 golden (BASELINE.json configs[0])


def test_prod_c1_stages():
    tts = model("prod")
    z = load_golden("prod_utt0.npz")
    tc = tts.generator.mrte.tc_latent(dev(z["phone"][None]), dev(z["prompt_mel"][None])).cpu().numpy()[0]
    assert O.rel_l2(tc, z["tc_latent"]) < TIGHT
    dur, flt = tts.native.adm_infer(dev(z["tc_latent"][None]), return_float=True)
    assert np.allclose(flt[0].cpu().numpy(), z["adm_float"], rtol=1e-4, atol=1e-4)
    assert np.array_equal(dur[0].cpu().numpy(), z["adm_dur"])
    codes, logits = tts.native.plm_infer(dev(z["plm_cond"][None]), return_logits=True)
    assert np.array_equal(codes[0].cpu().numpy(), z["p_codes"])
    assert O.rel_l2(logits[0].cpu().numpy(), z["plm_logits"]) < 1e-4
    mel = tts.generator.decoder(dev(z["decoder_in"].T[None].copy())).cpu().numpy()[0].T
    assert O.rel_l2(mel, z["mel"]) < TIGHT
    zq, codes_v, ze = tts.native.vqpe_forward(dev(z["target_mel"][None]), return_ze=True)
    assert O.rel_l2(ze[0].cpu().numpy(), z["vqpe_ze"]) < TIGHT
    assert np.array_equal(codes_v[0, 0].cpu().numpy(), z["vqpe_codes"])
    assert np.array_equal(zq[0].cpu().numpy(), z["vqpe_zq"])


def test_prod_c1_end_to_end():
    tts = model("prod")
    z = load_golden("prod_utt0.npz")
    out, lens, aux = tts.synthesize(dev(z["phone"][None]), dev(z["prompt_mel"][None]),
                                    forced_durations=z["forced_dur"][None], return_aux=True)
    assert lens[0] == 260
    assert np.array_equal(aux["dur"][0].cpu().numpy(), z["adm_dur"])
    assert np.array_equal(aux["codes"][0, :33].cpu().numpy(), z["p_codes"])
    assert O.rel_l2(out[0, :260].cpu().numpy(), z["mel"]) < NORTH_STAR


def test_prod_c2_properties():
    """Config C2 at full size (B=32, 70 phones, 431 frames): size-independent properties - every
    utterance of the batch equals its stand-alone computation; one of them equals the oracle."""
    from megatts2_amd import synth
    tts = model("prod")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    utts = synth.make_batch(synth.C2, seed=1002, jitter=0.3)
    phone, pl = pad_stack([u.phone for u in utts])
    mel, ml = pad_stack([u.prompt_mel for u in utts])
    dur, _ = pad_stack([u.durations for u in utts])
    codes, _ = pad_stack([u.p_codes for u in utts])
    out, lens = tts.native.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, forced_codes=dev(codes),
                                            run_plm=False)
    out = out.cpu().numpy()
    for i in (0, 17, 31):
        u = utts[i]
        o1, l1 = tts.native.synthesize_batch(dev(u.phone[None]), None, dev(u.prompt_mel[None]), None,
                                             forced_dur=u.durations[None], forced_codes=dev(u.p_codes[None]),
                                             run_plm=False)
        assert l1[0] == lens[i] == int(u.durations.sum())
        assert O.rel_l2(out[i, :lens[i]], o1[0, :l1[0]].cpu().numpy()) < 1e-5
    u = utts[5]
    ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, u.phone, u.prompt_mel, forced_durations=u.durations,
                       forced_codes=u.p_codes)
    assert O.rel_l2(out[5, :lens[5]], ref["mel"]) < NORTH_STAR


def test_prod_plm_batched_vs_alone_decisions():
    """Free-running PLM at production size, ragged batch: every sequence of the batch must take the same
    greedy decisions as when it runs alone.  Tile configurations (hence fp32 summation orders) differ between
    the two runs, so a divergence is tolerated only where the stand-alone run's top-2 logit margin is below
    1e-4 of the logit range (a genuine near-tie); none is expected with these seeds."""
    tts = model("prod")
    rng = np.random.default_rng(21)
    lens = np.asarray([54, 41, 54, 7, 33, 1], np.int32)
    cond = np.zeros((len(lens), 54, 512), np.float32)
    for i, n in enumerate(lens):
        cond[i, :n] = np.maximum(rng.standard_normal((n, 512)), 0).astype(np.float32)     # tc_latent is post-ReLU
    codes_b, logits_b = tts.native.plm_infer(dev(cond), lens, return_logits=True)
    codes_b = codes_b.cpu().numpy()
    for i in (0, 1, 3, 5):
        n = int(lens[i])
        c1, l1 = tts.native.plm_infer(dev(cond[i:i + 1, :n]), return_logits=True)
        c1, l1 = c1.cpu().numpy()[0], l1.cpu().numpy()[0]
        diff = np.nonzero(c1 != codes_b[i, :n])[0]
        if diff.size:
            t = int(diff[0])
            top = np.sort(l1[t])[-2:]
            assert (top[1] - top[0]) < 1e-4 * (l1[t].max() - l1[t].min()), f"seq {i} diverges at step {t} without a near-tie"
        else:
            assert O.rel_l2(logits_b[i, :n].cpu().numpy(), l1) < 1e-4
        assert not codes_b[i, n:].any()


# ---------------------------------------------------------------------------------------------------
# row f3: mel front-end on the GPU (extract_mel_spec, modules/tokenizer.py:107-125)


def test_mel_frontend_matches_oracle():
    from megatts2_amd.runtime import MelFrontEnd
    from megatts2_amd import megatts2 as M
    rng = np.random.default_rng(11)
    lens = np.asarray([16000, 5000, 777, 12345], np.int32)
    wav = np.zeros((4, 16000), np.float32)
    for i, n in enumerate(lens):
        t = np.arange(n) / 16000.0
        wav[i, :n] = (0.3 * np.sin(2 * np.pi * (220.0 * (i + 1)) * t) + 0.05 * rng.standard_normal(n)).astype(np.float32)
    fe = MelFrontEnd()
    mel = fe(dev(wav), lens).cpu().numpy()
    assert mel.shape == (4, 1 + 16000 // 256, 80)
    for i, n in enumerate(lens):
        ref = O.mel_spectrogram(wav[i, :n])
        T = 1 + n // 256
        assert ref.shape == (T, 80)
        assert np.abs(mel[i, :T] - ref).max() < 2e-3            # log-mel, absolute
        assert O.rel_l2(np.exp(mel[i, :T]), np.exp(ref)) < 1e-4  # linear mel
        assert not mel[i, T:].any()
    # mirror of the reference function: 1-D samples -> [80, T]
    one = M.extract_mel_spec(torch.from_numpy(wav[1, :5000]))
    assert tuple(one.shape) == (80, 1 + 5000 // 256)
    assert np.abs(one.cpu().numpy().T - O.mel_spectrogram(wav[1, :5000])).max() < 2e-3
    # silence hits the clamp floor exactly
    z = fe(dev(np.zeros((1, 2048), np.float32))).cpu().numpy()
    assert np.allclose(z, np.log(np.float32(1e-5)))


def test_tiny_forward_from_wav_dir(tmp_path):
    """Megatts.forward(wavs_dir, ...) (models/megatts2.py:325-375) with the in-repo front-end: *.wav ->
    normalise -> GPU mel -> concatenated prompt -> synthesis -> prompt audio + generated audio -> test.wav."""
    from megatts2_amd import audio_io as A
    tts = model("tiny")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    rng = np.random.default_rng(5)
    mels = []
    for i, n in enumerate((6000, 4321)):
        t = np.arange(n) / 16000.0
        y = (0.4 * np.sin(2 * np.pi * 330.0 * (i + 1) * t) + 0.02 * rng.standard_normal(n)).astype(np.float32)
        A.write_wav(str(tmp_path / f"p{i}.wav"), y, 16000, "PCM_S16")
        mels.append(O.mel_spectrogram(A.load_audio(str(tmp_path / f"p{i}.wav"))))
    prompt = np.concatenate(mels, axis=0)
    phone = rng.integers(0, g.mrte.phone_vocab_size, 6)
    out_wav = str(tmp_path / "test.wav")
    mel, lens, aux = tts.forward(str(tmp_path), phone_tokens=phone, out_path=out_wav)
    ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, phone.astype(np.int64), prompt)
    assert lens[0] == ref["mel"].shape[0]
    assert O.rel_l2(mel[0, :lens[0]].cpu().numpy(), ref["mel"]) < NORTH_STAR
    y, sr = A.read_wav(out_wav)
    assert sr == 16000 and y.size == (mels[0].shape[0] + int(lens[0])) * h.hop


def test_tiny_s2_latent_extraction(tiny_batch, tmp_path):
    """Row f2: MegaG.s2_latent (models/megatts2.py:75-84) and the latents/{spk}/{id}.npy record of
    prepare_ds.py:224-258 - tc_latent within tolerance, prosody codes bit-exact."""
    tts = model("tiny")
    z = tiny_batch[1]
    phone, pm, tm = dev(z["phone"][None]), dev(z["prompt_mel"][None]), dev(z["target_mel"][None])
    tc, codes = tts.generator.s2_latent(phone, np.asarray([z["phone"].size], np.int32), pm, tm)
    assert O.rel_l2(tc[0].cpu().numpy(), z["tc_latent"]) < TIGHT
    assert np.array_equal(codes[0, 0].cpu().numpy(), z["vqpe_codes"])
    f = str(tmp_path / "utt.npy")
    tts.generator.extract_latent(f, phone, np.asarray([z["phone"].size], np.int32), pm, tm)
    rec = np.load(f, allow_pickle=True).item()
    assert set(rec) == {"tc_latent", "p_code"} and rec["p_code"].dtype == np.int64
    assert np.array_equal(rec["p_code"][0, 0], z["vqpe_codes"]) and rec["tc_latent"].shape == (1,) + z["tc_latent"].shape


def test_error_behaviour_matches_reference_exceptions(tiny_batch):
    """The C ABI never throws and never falls back: conditions on which the reference asserts / raises come
    back as an error code + message (NativeError), and the handle stays usable afterwards."""
    from megatts2_amd.runtime import NativeError, NativeModel
    from megatts2_amd import config as C, weights
    tts = model("tiny")
    z = tiny_batch[0]
    phone, mel = dev(z["phone"][None]), dev(z["prompt_mel"][None])
    with pytest.raises(NativeError, match="length"):                       # length beyond the padded tensor
        tts.native.tc_latent(phone, mel, phone_lens=np.asarray([phone.shape[1] + 1], np.int32))
    with pytest.raises(NativeError, match="length"):
        tts.native.adm_infer(dev(z["tc_latent"][None]), np.asarray([0], np.int32))
    dur = z["forced_dur"][None].astype(np.int32)
    with pytest.raises(NativeError, match="Tm_max"):                       # output smaller than sum(durations)
        B, Np, D = 1, dur.shape[1], 64
        out = torch.empty(1, 3, D, device="cuda")
        from megatts2_amd import runtime as rt
        x = dev(z["tc_latent"][None])
        rt._check(tts.native.lib.mt2_length_regulate(tts.native.h, rt._stream(), rt._ptr(x), rt._iptr(dur),
                                                     rt._iptr(np.asarray([Np], np.int32)), Np, D, 1, rt._ptr(out), 3))
    with pytest.raises(NativeError, match="PLM"):                          # component not loaded into the handle
        g = C.tiny_g()
        only_g = NativeModel(g_cfg=g, plm_cfg=C.tiny_plm(), adm_cfg=C.tiny_adm(), hg_cfg=C.tiny_hifigan(),
                             sd_g=synth_models("tiny")[1][0])
        only_g.plm_infer(dev(z["plm_cond"][None]))
    with pytest.raises(NativeError, match="missing tensor|shape mismatch"):  # load_state_dict(strict=True)
        bad = dict(synth_models("tiny")[1][2])
        bad.pop("adm.layers.0.norm1.weight")
        NativeModel(g_cfg=C.tiny_g(), plm_cfg=C.tiny_plm(), adm_cfg=C.tiny_adm(), hg_cfg=C.tiny_hifigan(), sd_adm=bad)
    # the shared handle still works
    out = tts.native.tc_latent(phone, mel).cpu().numpy()
    assert O.rel_l2(out[0], z["tc_latent"]) < TIGHT


# ---------------------------------------------------------------------------------------------------
# round 2: production-size parity beyond C1 - C3 batch (free-running PLM + vocoder), C5-length stages and
# single AR steps, prompt-conditioned PLM, vocoder boundary, index validation, handle hygiene


def _c3_batch():
    """32 utterances at the C2/C3/C4 geometry; slot 0 is the utterance of the live-reference fixture prod_utt1."""
    from megatts2_amd import synth
    z = load_golden("prod_utt1.npz")
    utts = synth.make_batch(synth.C3, seed=1003)
    utts[0] = synth.Utterance(z["phone"], z["prompt_mel"], z["forced_dur"], utts[0].p_codes)
    return z, utts


def test_prod_c3_batch_free_running_plm_and_vocoder():
    """BASELINE configs[2] at full size (B=32, 70 phones, 431-frame prompt, 431 frames): the whole path with the ADM and
    the PLM free-running and the vocoder.  Utterance 0 against the fixture made by the LIVE reference modules,
    utterances 7 and 31 against the oracle run alone (ATen backend): durations and prosody codes bit-exact, mel and
    waveform within 1e-3."""
    tts = model("prod")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    z, utts = _c3_batch()
    phone, pl = pad_stack([u.phone for u in utts])
    mel, ml = pad_stack([u.prompt_mel for u in utts])
    dur, _ = pad_stack([u.durations for u in utts])
    out, lens, aux = tts.native.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, vocoder=True, return_aux=True,
                                                 prompt_vqpe=True)
    out = out.cpu().numpy()
    assert lens.tolist() == [431] * 32
    # the prompt's VQ-PE codes (modules/vqpe.py:50-62) at the benchmark's batch geometry (32 x 431 frames through the x6
    # conv stacks): bit-exact against the oracle for utterances 0 / 7 / 31
    pc = aux["prompt_codes"].cpu().numpy()
    assert pc.shape == (32, 54)
    O.enable_torch_kernels()
    try:
        for i in (0, 7, 31):
            want = O.vqpe_forward(sd_g, g, utts[i].prompt_mel)[1]
            assert np.array_equal(pc[i, :want.size], want), f"prompt VQ-PE codes of utterance {i}"
    finally:
        O.disable_torch_kernels()
    assert np.array_equal(aux["dur"][0].cpu().numpy(), z["adm_dur"])
    assert np.array_equal(aux["codes"][0, :54].cpu().numpy(), z["p_codes"])
    assert O.rel_l2(out[0, :431], z["mel"]) < NORTH_STAR
    O.enable_torch_kernels()
    try:
        for i in (7, 31):
            u = utts[i]
            ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, u.phone, u.prompt_mel, forced_durations=u.durations)
            assert np.array_equal(aux["dur"][i].cpu().numpy(), ref["adm_dur"]), f"durations of utterance {i}"
            assert np.array_equal(aux["codes"][i, :54].cpu().numpy(), ref["p_codes"]), f"prosody codes of utterance {i}"
            assert O.rel_l2(out[i, :431], ref["mel"]) < NORTH_STAR
            wav = O.hifigan(sd_h, h, ref["mel"])
            assert O.rel_l2(aux["wav"][i, :wav.size].cpu().numpy(), wav) < NORTH_STAR
    finally:
        O.disable_torch_kernels()


def test_prod_strong_scaling_shard_geometry_b96_ragged():
    """BASELINE configs[3] as `bench.py --scaling strong` runs it on one rank: ONE synthesize_batch call over a large RAGGED
    shard (C4 utterances with lengths U(0.7, 1): 96 here, up to 256 in the bench) - workspace query, row maps and the AR slot
    ordering at B = 96, every length different.  Three utterances (the longest, the shortest, one in between) against the
    oracle run alone: the ADM's own durations and the free-running PLM's codes bit-exact, mel within 1e-3; padding zero."""
    from megatts2_amd import synth
    tts = model("prod")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    utts = synth.make_batch(synth.C4, seed=1004, jitter=0.3, batch=96)
    phone, pl = pad_stack([u.phone for u in utts])
    mel, ml = pad_stack([u.prompt_mel for u in utts])
    dur, _ = pad_stack([u.durations for u in utts])
    frames = np.asarray([int(u.durations.sum()) for u in utts])
    assert len(set(pl.tolist())) > 10 and len(set(frames.tolist())) > 30           # really ragged
    nat = tts.native
    nat.workspace_reserve(nat.workspace_query(96, int(pl.max()), int(ml.max()), synth.C4.Tm, run_plm=True, vocoder=False))
    out, lens, aux = nat.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, tm_cap=synth.C4.Tm, return_aux=True)
    assert lens.tolist() == frames.tolist()
    order = np.argsort(frames)
    picks = [int(order[-1]), int(order[0]), int(order[len(order) // 2])]
    out = out.cpu().numpy()
    O.enable_torch_kernels()
    try:
        for i in picks:
            u = utts[i]
            ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, u.phone, u.prompt_mel, forced_durations=u.durations)
            nq = ref["p_codes"].size
            assert np.array_equal(aux["dur"][i, :pl[i]].cpu().numpy(), ref["adm_dur"]), f"durations of utterance {i}"
            assert not aux["dur"][i, pl[i]:].any()
            assert np.array_equal(aux["codes"][i, :nq].cpu().numpy(), ref["p_codes"]), f"prosody codes of utterance {i}"
            assert O.rel_l2(out[i, :frames[i]], ref["mel"]) < NORTH_STAR
            assert not out[i, frames[i]:].any()
    finally:
        O.disable_torch_kernels()


def test_prod_strong_scaling_the_exact_256_utterance_call():
    """What `bench.py --gpus 1 --scaling strong` (and `bench.py --full`'s `workloads.C4_strong_n1`) TIMES: the 256 ragged
    utterances of BASELINE configs[3] (C4 geometry, lengths U(0.7, 1), seed 1004) in ONE synthesize_batch call with the prompt's
    VQ-PE and the vocoder, exactly as the bench issues it (that call was parity-checked at B = 96 only).
    The longest, the shortest and a middle utterance against the oracle run alone: the ADM's own durations, the free-running
    PLM's codes and the prompt's VQ-PE codes bit-exact, mel and waveform within 1e-3; padding zero."""
    from megatts2_amd import synth
    tts = model("prod")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    utts = synth.make_batch(synth.C4, seed=1004, jitter=0.3, batch=256)
    assert len(utts) == 256
    phone, pl = pad_stack([u.phone for u in utts])
    mel, ml = pad_stack([u.prompt_mel for u in utts])
    dur, _ = pad_stack([u.durations for u in utts])
    frames = np.asarray([int(u.durations.sum()) for u in utts])
    nat = tts.native
    nat.workspace_reserve(nat.workspace_query(256, int(pl.max()), int(ml.max()), synth.C4.Tm, run_plm=True, vocoder=True,
                                              prompt_vqpe=True))
    out, lens, aux = nat.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, tm_cap=synth.C4.Tm, vocoder=True,
                                          prompt_vqpe=True, return_aux=True)
    assert lens.tolist() == frames.tolist()
    order = np.argsort(frames)
    picks = [int(order[-1]), int(order[0]), int(order[len(order) // 2])]
    out = out.cpu().numpy()
    hop = h.hop
    O.enable_torch_kernels()
    try:
        for i in picks:
            u = utts[i]
            ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, u.phone, u.prompt_mel, forced_durations=u.durations)
            nq = ref["p_codes"].size
            assert np.array_equal(aux["dur"][i, :pl[i]].cpu().numpy(), ref["adm_dur"]), f"durations of utterance {i}"
            assert not aux["dur"][i, pl[i]:].any()
            assert np.array_equal(aux["codes"][i, :nq].cpu().numpy(), ref["p_codes"]), f"prosody codes of utterance {i}"
            assert O.rel_l2(out[i, :frames[i]], ref["mel"]) < NORTH_STAR
            assert not out[i, frames[i]:].any()
            want_pc = O.vqpe_forward(sd_g, g, u.prompt_mel)[1]
            assert np.array_equal(aux["prompt_codes"][i, :want_pc.size].cpu().numpy(), want_pc), f"prompt VQ-PE codes of utterance {i}"
            wav = O.hifigan(sd_h, h, ref["mel"])
            got = aux["wav"][i].cpu().numpy()
            assert O.rel_l2(got[:wav.size], wav) < NORTH_STAR and wav.size == frames[i] * hop
            assert not got[wav.size:].any()
    finally:
        O.disable_torch_kernels()


def test_prod_three_batches_in_flight_equal_three_sequential_calls():
    """`bench.py --inflight 3` (`bench.py --full`'s `workloads.C3_inflight3`) at production size: three handles, each with its
    own weights and arena, three HIP streams, three DIFFERENT C3 batches enqueued back to back without a host synchronisation -
    mels, waveforms, prosody codes, durations and prompt VQ-PE codes bit-identical to the same three batches run one after
    the other on one handle (exercised on the tiny model only)."""
    from megatts2_amd import megatts2 as M, synth
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    first = model("prod")
    handles = [first.native] + [M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)),
                                          hifi_gan=M.HIFIGAN(h, sd_h)).native for _ in range(2)]
    for kv in filter(None, os.environ.get("MT2_TEST_OPTS", "").split(",")):
        k, v = kv.split("=")
        for nat in handles[1:]:
            nat.set_option(k, int(v))
    batches = []
    for seed in (1003, 1013, 1023):
        utts = synth.make_batch(synth.C3, seed=seed)
        phone, pl = pad_stack([u.phone for u in utts])
        mel, ml = pad_stack([u.prompt_mel for u in utts])
        dur, _ = pad_stack([u.durations for u in utts])
        batches.append((dev(phone), pl, dev(mel), ml, dur))

    def call(nat, b):
        out, lens, aux = nat.synthesize_batch(b[0], b[1], b[2], b[3], forced_dur=b[4], vocoder=True, prompt_vqpe=True,
                                              tm_cap=synth.C3.Tm, return_aux=True)
        return out, lens, aux
    want = []
    for b in batches:                                         # sequential, one handle, default stream
        out, lens, aux = call(handles[0], b)
        torch.cuda.synchronize()
        want.append((out.cpu().numpy(), lens.copy(), {k: v.cpu().numpy() for k, v in aux.items()}))
    lanes = [torch.cuda.Stream() for _ in handles]
    got = [None] * 3
    for rep in range(2):                                      # twice: the second round reuses warm arenas on every handle
        for i, b in enumerate(batches):
            with torch.cuda.stream(lanes[i]):
                got[i] = call(handles[i], b)
        torch.cuda.synchronize()
    for i in range(3):
        out, lens, aux = got[i]
        w_out, w_lens, w_aux = want[i]
        assert lens.tolist() == w_lens.tolist()
        assert np.array_equal(out.cpu().numpy(), w_out), f"mel of batch {i}"
        for k in ("dur", "codes", "wav", "prompt_codes"):
            assert np.array_equal(aux[k].cpu().numpy(), w_aux[k]), f"{k} of batch {i}"
    assert not np.array_equal(want[0][0], want[1][0])         # really three different batches
    for nat in handles[1:]:
        nat.close()


def test_prod_c3_batch_own_durations_end_to_end():
    """The real control flow at production size (the default line's `workloads.C3_own_durations`): the C3 batch with NOTHING
    forced - the ADM's own durations leave the device (one D2H + stream synchronisation, as the reference's
    modules/mrte.py:51-56 does), the host re-plans the frame rows, the PLM and the decoder run on the lengths the ADM chose.
    Two utterances against the oracle run alone, un-forced too: durations and prosody codes bit-exact, mel within 1e-3, the
    frame count equal to the sum of the durations (VERDICT r4 missing 5 / weak 1)."""
    tts = model("prod")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    z, utts = _c3_batch()
    phone, pl = pad_stack([u.phone for u in utts])
    mel, ml = pad_stack([u.prompt_mel for u in utts])
    out, lens, aux = tts.native.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=None, vocoder=False, return_aux=True,
                                                 tm_cap=24 * int(pl.max()))
    out = out.cpu().numpy()
    durs = aux["dur"].cpu().numpy()
    assert lens.tolist() == durs.sum(axis=1).tolist() and durs.min() >= 1 and durs.max() <= 128       # :275 clamp(1, 128)
    O.enable_torch_kernels()
    try:
        for i in (3, 29):
            u = utts[i]
            ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, u.phone, u.prompt_mel)
            assert np.array_equal(durs[i], ref["adm_dur"]), f"durations of utterance {i}"
            n = int(ref["adm_dur"].sum())
            assert lens[i] == n == ref["mel"].shape[0]
            nq = -(-n // 8)
            assert np.array_equal(aux["codes"][i, :nq].cpu().numpy(), ref["p_codes"]), f"prosody codes of utterance {i}"
            assert O.rel_l2(out[i, :n], ref["mel"]) < NORTH_STAR
            assert not out[i, n:].any()
    finally:
        O.disable_torch_kernels()


def test_prod_c2_durations_of_the_batched_adm():
    """C2 at full size: the ADM's own integer durations (not the forced ones) of a ragged batch equal the oracle's."""
    from megatts2_amd import synth
    tts = model("prod")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    utts = synth.make_batch(synth.C2, seed=1002, jitter=0.3)
    phone, pl = pad_stack([u.phone for u in utts])
    mel, ml = pad_stack([u.prompt_mel for u in utts])
    dur, _ = pad_stack([u.durations for u in utts])
    codes, _ = pad_stack([u.p_codes for u in utts])
    out, lens, aux = tts.native.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, forced_codes=dev(codes),
                                                 run_plm=False, return_aux=True)
    O.enable_torch_kernels()
    try:
        for i in (5, 22):
            u = utts[i]
            tc = O.mrte_tc_latent(sd_g, g, u.phone, u.prompt_mel)
            assert np.array_equal(aux["dur"][i, :pl[i]].cpu().numpy(), O.adm_infer(sd_a, a, tc))
            assert not aux["dur"][i, pl[i]:].any()
    finally:
        O.disable_torch_kernels()


def test_prod_long_shapes_c5_geometry():
    """C5 geometry against the live-reference fixture prod_long.npz: mel encoder on a 2584-frame prompt, decoder and
    VQ-PE on 5168 frames (VQ indices bit-exact), single AR steps on forced histories at n = 71 / 417 / 834 (ADM:
    13-27 key tiles per head, PE rows > 260) and n = 128 / 646 (PLM: the 256x128 tile regime of its feed-forward)."""
    import fixtures
    tts = model("prod")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    z = load_golden("prod_long.npz")
    li = fixtures.long_inputs(sd_g[O.CODEBOOK], int(z["seed"]))
    ctx = tts.native.mel_context(dev(li["prompt_mel"][None])).cpu().numpy()[0]
    assert ctx.shape == z["mel_context"].shape and O.rel_l2(ctx, z["mel_context"]) < TIGHT
    mel = tts.generator.decoder(dev(li["decoder_in"].T[None].copy())).cpu().numpy()[0].T
    assert O.rel_l2(mel, z["mel"]) < TIGHT
    zq, codes, ze = tts.native.vqpe_forward(dev(li["target_mel"][None]), return_ze=True)
    assert O.rel_l2(ze[0].cpu().numpy(), z["vqpe_ze"]) < TIGHT
    assert np.array_equal(codes[0, 0].cpu().numpy(), z["vqpe_codes"])
    for n in fixtures.ADM_STEPS:
        _, flt = tts.native.adm_infer(dev(li["adm_tc"][None, :n]), return_float=True, p_prefix=dev(li["adm_hist"][None, :n - 1]),
                                      max_steps=1)
        flt = flt[0].cpu().numpy()
        assert np.array_equal(flt[:n - 1], li["adm_hist"][:n - 1])                 # the forced history comes back untouched
        want = float(z[f"adm_pred_{n}"])
        assert abs(float(flt[n - 1]) - want) < 1e-4 * max(1.0, abs(want)), (n, flt[n - 1], want)
    for n in fixtures.PLM_STEPS:
        c, lg = tts.native.plm_infer(dev(li["plm_cond"][None, :n]), np.asarray([1], np.int32), return_logits=True,
                                     prefix_codes=dev(li["plm_hist"][None, :n - 1]), max_steps=1)
        assert O.rel_l2(lg[0, 0].cpu().numpy(), z[f"plm_logits_{n}"]) < 1e-4
        assert int(c[0, 0]) == int(z[f"plm_logits_{n}"].argmax())
    # two sequences of different length stepping from the same forced-history length in ONE call
    tcs, ln = pad_stack([li["adm_tc"][:300], li["adm_tc"][200:480]])
    hist = np.stack([li["adm_hist"][:250], li["adm_hist"][200:450]])
    _, flt = tts.native.adm_infer(dev(tcs), ln, return_float=True, p_prefix=dev(hist), max_steps=2)
    O.enable_torch_kernels()
    try:
        for b, (lo, hi) in enumerate(((0, 300), (200, 480))):
            _, want = O.adm_infer(sd_a, a, li["adm_tc"][lo:hi], return_float=True, p_prefix=hist[b], steps=2)
            assert np.allclose(flt[b, :252].cpu().numpy(), want[:252], rtol=1e-4, atol=1e-4)
    finally:
        O.disable_torch_kernels()


def test_prod_c5_utterance_free_running():
    """BASELINE configs[4] end to end: ONE 834-phone / 2584-frame-prompt / 5168-frame utterance through MRTE -> ADM (834
    float-feedback steps) -> regulate (forced durations) -> PLM (646 greedy steps) -> decoder, against the fixture made by
    the LIVE reference modules (oracle/make_golden.py --extra-long).  Alone and as slot 0 of the B = 8 C5 batch:
    durations and prosody codes bit-exact, ADM float trajectory 1e-4, mel within 1e-3."""
    import fixtures
    from megatts2_amd import synth
    tts = model("prod")
    z = load_golden("prod_c5_utt.npz")
    u = fixtures.c5_utterance()
    assert u.phone.size == 834 and u.prompt_mel.shape[0] == 2584 and int(u.durations.sum()) == 5168

    def check(out, lens, aux, slot, what):
        assert int(lens[slot]) == 5168
        dur = aux["dur"][slot, :834].cpu().numpy()
        codes = aux["codes"][slot, :646].cpu().numpy()
        bad = np.nonzero(codes != z["p_codes"])[0]
        first = int(bad[0]) if bad.size else -1
        assert np.array_equal(dur, z["adm_dur"]), f"{what}: durations differ at {np.nonzero(dur != z['adm_dur'])[0][:8]}"
        assert bad.size == 0, (f"{what}: {bad.size} prosody codes differ, first at step {first} "
                               f"(reference arg-max margin there {float(z['plm_margin'][first]):.3g})")
        assert O.rel_l2(out[slot, :5168].cpu().numpy(), z["mel"]) < NORTH_STAR

    out, lens, aux = tts.native.synthesize_batch(dev(u.phone[None]), None, dev(u.prompt_mel[None]), None,
                                                 forced_dur=u.durations[None], return_aux=True)
    check(out, lens, aux, 0, "alone")
    # the float trajectory of the ADM and a spot check of tc_latent rows, through the stage calls
    tc = tts.generator.mrte.tc_latent(dev(u.phone[None]), dev(u.prompt_mel[None]))
    assert O.rel_l2(tc[0, ::64].cpu().numpy(), z["tc_latent_rows"]) < TIGHT
    _, flt = tts.native.adm_infer(tc, return_float=True)
    assert np.allclose(flt[0].cpu().numpy(), z["adm_float"], rtol=1e-4, atol=1e-4)
    del out, aux, tc
    utts = synth.make_batch(synth.C5, seed=1005)
    utts[0] = u
    phone, pl = pad_stack([v.phone for v in utts])
    mel, ml = pad_stack([v.prompt_mel for v in utts])
    dur, _ = pad_stack([v.durations for v in utts])
    # ... with the vocoder, as bench.py times C5 (the only timed leg without a comparison).  The last stage
    # holds 8 x 5168 x 256 = 10.6 M rows of 32 channels = 1.35 GB: byte offsets beyond 2^31 - the LAST utterance's tail
    # lives there, so slot 7 is compared too, and the last 64 frames of both explicitly.
    out, lens, aux = tts.native.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, vocoder=True, return_aux=True)
    check(out, lens, aux, 0, "slot 0 of the B = 8 batch")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    hop = int(np.prod(h.upsample_rates))
    O.enable_torch_kernels()
    try:
        for slot, mel_ref, tol in ((0, z["mel"], NORTH_STAR), (7, out[7, :int(lens[7])].cpu().numpy(), 1e-4)):
            T = int(lens[slot])
            want = O.hifigan(sd_h, h, mel_ref)              # slot 0: from the LIVE reference's mel (end to end); slot 7: the
            got = aux["wav"][slot, :T * hop].cpu().numpy()  # vocoder alone, on the mel the device produced
            assert want.size == T * hop
            assert O.rel_l2(got, want) < tol, (slot, O.rel_l2(got, want))
            tail = slice((T - 64) * hop, T * hop)
            assert O.rel_l2(got[tail], want[tail]) < max(tol, 2e-4) * 3, (slot, "last 64 frames", O.rel_l2(got[tail], want[tail]))
            assert not aux["wav"][slot, T * hop:].any()
    finally:
        O.disable_torch_kernels()


def test_prod_plm_prompt_conditioned():
    """Row f1: PLM decoding conditioned on a prompt's prosody codes (training layout, modules/datamodule.py:201-212)
    against the live-reference fixture; through the mirror `MegaPLM.infer(..., prompt_tc_latent, prompt_codes)`."""
    tts = model("prod")
    z = load_golden("prod_plm_prefix.npz")
    P = z["prefix"].size
    codes, logits = tts.native.plm_infer(dev(z["cond"][None]), return_logits=True, prefix_codes=dev(z["prefix"][None]))
    assert np.array_equal(codes[0].cpu().numpy(), z["codes"])
    assert O.rel_l2(logits[0].cpu().numpy(), z["logits"]) < 1e-4
    got = tts.plm.infer(dev(z["cond"][None, P:]), prompt_tc_latent=dev(z["cond"][None, :P]), prompt_codes=dev(z["prefix"][None]))
    assert np.array_equal(got[0].cpu().numpy(), z["codes"])
    # a ragged batch: the fixture's sequence beside a shorter one with another prompt of the same length
    rng = np.random.default_rng(9)
    cond2 = np.maximum(rng.standard_normal((P + 11, 512)), 0).astype(np.float32)
    pre2 = rng.integers(0, 1024, P).astype(np.int64)
    cb, _ = pad_stack([z["cond"], cond2])
    both = tts.native.plm_infer(dev(cb), np.asarray([z["codes"].size, 11], np.int32), prefix_codes=dev(np.stack([z["prefix"], pre2])))
    assert np.array_equal(both[0].cpu().numpy(), z["codes"])
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    O.enable_torch_kernels()
    try:
        assert np.array_equal(both[1, :11].cpu().numpy(), O.plm_infer(sd_p, p, cond2, prefix_codes=pre2))
    finally:
        O.disable_torch_kernels()
    assert not both[1, 11:].any()
    with pytest.raises(ValueError):
        tts.plm.infer(dev(z["cond"][None, P:]), prompt_codes=dev(z["prefix"][None]))


def test_hifigan_production_length_ragged_and_inference_padding():
    """Vocoder at C3 size (431 + 187 frames, ragged) against transformers.SpeechT5HifiGan carrying the same weights
    (stand-in: parity unpinned, speechbrain absent), and speechbrain's `inference_padding` behaviour both ways:
    padding 5 = the generator applied to the mel with its own edge frames replicated 5x on both sides."""
    from megatts2_amd import megatts2 as M, synth
    import dataclasses
    tr = pytest.importorskip("transformers")
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    tts = model("prod")
    rng = np.random.Generator(np.random.PCG64(78))
    mels = [synth.make_utterance(rng, 2, T, T).prompt_mel for T in (431, 187)]
    tcfg = tr.SpeechT5HifiGanConfig(model_in_dim=h.in_dim, upsample_initial_channel=h.upsample_initial_channel,
                                    upsample_rates=h.upsample_rates, upsample_kernel_sizes=h.upsample_kernel_sizes,
                                    resblock_kernel_sizes=h.resblock_kernel_sizes,
                                    resblock_dilation_sizes=h.resblock_dilation_sizes,
                                    leaky_relu_slope=h.leaky_relu_slope, normalize_before=False)
    ref = tr.SpeechT5HifiGan(tcfg).eval()
    full = {k: torch.from_numpy(v) for k, v in sd_h.items()}
    full["mean"], full["scale"] = torch.zeros(h.in_dim), torch.ones(h.in_dim)
    ref.load_state_dict(full, strict=True)
    mel, ln = pad_stack(mels)
    wav = tts.hifi_gan.decode_batch(dev(mel).transpose(1, 2).contiguous(), mel_lens=ln).cpu().numpy()
    for i, m in enumerate(mels):
        with torch.no_grad():
            want = ref(torch.from_numpy(m)).numpy()
        n = m.shape[0] * h.hop
        assert O.rel_l2(wav[i, 0, :n], want) < NORTH_STAR
        assert not wav[i, 0, n:].any()
    # inference_padding = 5 (speechbrain's default): tiny model, both ways against the oracle
    (gt, pt, at, ht), (_, _, _, sd_ht) = synth_models("tiny")
    hp = dataclasses.replace(ht, inference_padding=5)
    voc = M.HIFIGAN(hp, sd_ht)
    small = [synth.make_utterance(rng, 1, T, T).prompt_mel for T in (23, 9, 1)]
    mel, ln = pad_stack(small)
    wav = voc.decode_batch(dev(mel).transpose(1, 2).contiguous(), mel_lens=ln).cpu().numpy()
    assert wav.shape == (3, 1, (23 + 10) * ht.hop)
    for i, m in enumerate(small):
        want = O.hifigan(sd_ht, ht, np.pad(m, ((5, 5), (0, 0)), mode="edge"))
        assert want.size == (m.shape[0] + 10) * ht.hop
        assert O.rel_l2(wav[i, 0, :want.size], want) < NORTH_STAR
        assert not wav[i, 0, want.size:].any()
        plain = tiny_voc().decode_batch(dev(m.T[None].copy())).cpu().numpy()[0, 0]
        assert O.rel_l2(plain, O.hifigan(sd_ht, ht, m)) < NORTH_STAR      # padding 0: plain forward


def tiny_voc():
    return model("tiny").hifi_gan


def test_index_range_errors_instead_of_out_of_bounds_reads(tiny_batch):
    """nn.Embedding / F.embedding raise IndexError in the reference; here an out-of-range phone id or prosody code is
    reported as an error by the call that received it (never used as a gather offset), and the handle stays usable."""
    from megatts2_amd.runtime import NativeError
    tts = model("tiny")
    (g, *_), _ = synth_models("tiny")
    z = tiny_batch[0]
    phone, mel = z["phone"][None].copy(), dev(z["prompt_mel"][None])
    bad = phone.copy()
    bad[0, 3] = g.mrte.phone_vocab_size
    with pytest.raises(NativeError, match="phone id"):
        tts.native.tc_latent(dev(bad), mel)
    bad[0, 3] = -1
    with pytest.raises(NativeError, match="phone id"):
        tts.synthesize(dev(bad), mel, forced_durations=z["forced_dur"][None])
    padded = np.concatenate([phone, np.full((1, 4), 10 ** 6, np.int64)], axis=1)      # garbage BEYOND the true length is fine
    ok = tts.native.tc_latent(dev(padded), mel, phone_lens=np.asarray([phone.shape[1]], np.int32)).cpu().numpy()
    assert O.rel_l2(ok[0, :phone.shape[1]], z["tc_latent"]) < TIGHT
    codes = z["p_codes"][None].copy()
    codes[0, 1] = g.vqpe.vq_bins
    with pytest.raises(NativeError, match="prosody code"):
        tts.synthesize(dev(phone), mel, forced_durations=z["forced_dur"][None], forced_codes=dev(codes))
    with pytest.raises(NativeError, match="prosody code"):
        tts.generator.vqpe.vq.decode(dev(codes[None]))
    with pytest.raises(NativeError, match="prompt prosody code"):
        tts.native.plm_infer(dev(z["plm_cond"][None]), np.asarray([1], np.int32),
                             prefix_codes=dev(np.full((1, z["plm_cond"].shape[0] - 1), 5000, np.int64)))
    out, lens = tts.synthesize(dev(phone), mel, forced_durations=z["forced_dur"][None])
    assert O.rel_l2(out[0, :lens[0]].cpu().numpy(), z["mel"]) < NORTH_STAR


def test_handles_threads_and_streams_do_not_interfere(tiny_batch):
    """Library hygiene: (a) two handles driven from two host threads at once, each with its own options; (b) one
    handle called from two threads (serialised by the handle) and on two different streams back to back (the second
    call waits for the first one's end before reusing the arena) - every result equals the single-threaded one."""
    import threading
    from megatts2_amd import megatts2 as M
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    tts1 = model("tiny")
    tts2 = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)), hifi_gan=M.HIFIGAN(h, sd_h))
    tts2.native.set_option("ar_groups", 1)
    tts2.native.set_option("splitk", 0)
    assert tts1.native.get_option("ar_groups") == 2 and tts2.native.get_option("ar_groups") == 1   # per handle, no globals
    phone, pl = pad_stack([z["phone"] for z in tiny_batch])
    mel, ml = pad_stack([z["prompt_mel"] for z in tiny_batch])
    dur, _ = pad_stack([z["forced_dur"] for z in tiny_batch])
    dphone, dmel = dev(phone), dev(mel)
    want, _ = tts1.synthesize(dphone, dmel, pl, ml, forced_durations=dur)
    want = want.cpu().numpy()
    res, errs = {}, []

    def work(tag, tts, reps):
        try:
            s = torch.cuda.Stream()
            with torch.cuda.stream(s):
                for r in range(reps):
                    out, _ = tts.synthesize(dphone, dmel, pl, ml, forced_durations=dur)
                s.synchronize()
                res[tag] = out.cpu().numpy()
        except Exception as e:  # pragma: no cover
            errs.append(e)

    th = [threading.Thread(target=work, args=("h1", tts1, 3)), threading.Thread(target=work, args=("h2", tts2, 3)),
          threading.Thread(target=work, args=("h1b", tts1, 3))]
    for t in th:
        t.start()
    for t in th:
        t.join()
    assert not errs, errs
    for tag in ("h1", "h2", "h1b"):
        assert O.rel_l2(res[tag], want) < 2e-6, tag
    # one handle, two streams, no host synchronisation in between
    s1, s2 = torch.cuda.Stream(), torch.cuda.Stream()
    with torch.cuda.stream(s1):
        o1, _ = tts1.synthesize(dphone, dmel, pl, ml, forced_durations=dur)
    with torch.cuda.stream(s2):
        o2, _ = tts1.synthesize(dphone[:2], dmel[:2], pl[:2], ml[:2], forced_durations=dur[:2])
    torch.cuda.synchronize()
    assert O.rel_l2(o1.cpu().numpy(), want) < 2e-6
    assert O.rel_l2(o2.cpu().numpy()[:, :want.shape[1]], want[:2, :o2.shape[1]]) < 2e-6
    tts2.native.close()


def test_workspace_query_bounds_the_arena():
    """mt2_workspace_query is an upper bound of what a synthesize_batch call of that geometry really takes, and a
    reserved arena is not grown by the call."""
    from megatts2_amd import megatts2 as M, synth
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    for B, Np, Tp, Tm, voc in ((3, 12, 60, 50, True), (1, 5, 33, 17, False), (6, 9, 97, 61, True)):
        tts = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)), hifi_gan=M.HIFIGAN(h, sd_h))
        nat = tts.native
        utts = synth.make_batch(synth.Shape("t", B, Np, Tp, Tm), seed=3, phone_vocab=g.mrte.phone_vocab_size)
        bound = nat.workspace_query(B, Np, Tp, Tm, run_plm=True, vocoder=voc)
        nat.workspace_reserve(bound)
        cap0 = nat.memory()[1]
        phone, pl = pad_stack([u.phone for u in utts])
        mel, ml = pad_stack([u.prompt_mel for u in utts])
        dur, _ = pad_stack([u.durations for u in utts])
        nat.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, vocoder=voc, tm_cap=Tm)
        torch.cuda.synchronize()
        assert nat.workspace_high_water() <= bound, (B, Np, Tp, Tm, nat.workspace_high_water(), bound)
        assert nat.memory()[1] == cap0                                    # no allocation on the hot path
        nat.close()


def test_megatts_seven_argument_constructor_writes_wav(tmp_path, monkeypatch):
    """The import-swap of INTEGRATION.md: `Megatts(g_ckpt, g_config, plm_ckpt, plm_config, adm_ckpt, adm_config,
    symbol_table)` (reference models/megatts2.py:296-323) builds the vocoder from a local speechbrain model directory
    and `forward` writes test.wav = vocoded prompt + generated audio (:370-375), inference padding included."""
    import dataclasses
    import yaml
    from megatts2_amd import audio_io as A, config as C, megatts2 as M
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    ck = {}
    for name, pre, sd in (("g", "G.", sd_g), ("plm", "plm.", sd_p), ("adm", "adm.", sd_a)):
        ck[name] = str(tmp_path / f"{name}.ckpt")
        torch.save({"state_dict": {pre + k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}}, ck[name])
    gy = {"model": {"G": {"class_path": "models.megatts2.MegaG", "init_args": {
        "mrte": {"class_path": "modules.mrte.MRTE", "init_args": dict(dataclasses.asdict(g.mrte), mel_activation="ReLU", dropout=0.1)},
        "vqpe": {"class_path": "modules.vqpe.VQProsodyEncoder", "init_args": dict(dataclasses.asdict(g.vqpe), activation="ReLU")},
        "kernel_size": g.kernel_size, "activation": "ReLU", "hidden_size": g.hidden_size,
        "decoder_n_stack": g.decoder_n_stack, "decoder_n_block": g.decoder_n_block}}}}
    cfgs = {"g": gy, "plm": {"model": {"plm": {"init_args": dict(dataclasses.asdict(p), dropout=0.1)}}},
            "adm": {"model": {"adm": {"init_args": dict(dataclasses.asdict(a), dropout=0.1)}}}}
    ypath = {}
    for k, tree in cfgs.items():
        ypath[k] = str(tmp_path / f"config_{k}.yaml")
        open(ypath[k], "w").write(yaml.safe_dump(tree))
    voc = tmp_path / "tts-hifigan-libritts-16kHz"
    voc.mkdir()
    raw = {}
    for k, v in sd_h.items():
        base, leaf = k.rsplit(".", 1)
        raw[f"{base.replace('upsampler.', 'ups.')}.conv.{leaf}"] = torch.from_numpy(v)     # weight norm already removed
    torch.save(raw, str(voc / "generator.ckpt"))
    (voc / "hyperparams.yaml").write_text(yaml.safe_dump({
        "in_channels": 80, "out_channels": 1, "resblock_type": "1", "upsample_initial_channel": h.upsample_initial_channel,
        "upsample_factors": h.upsample_rates, "upsample_kernel_sizes": h.upsample_kernel_sizes,
        "resblock_kernel_sizes": h.resblock_kernel_sizes, "resblock_dilation_sizes": h.resblock_dilation_sizes,
        "inference_padding": 5, "cond_channels": 0, "conv_post_bias": True}))
    monkeypatch.setenv("MEGATTS2_HIFIGAN_DIR", str(voc))
    rng = np.random.default_rng(6)
    n = 5000
    y = (0.4 * np.sin(2 * np.pi * 300.0 * np.arange(n) / 16000.0) + 0.02 * rng.standard_normal(n)).astype(np.float32)
    wdir = tmp_path / "prompts"
    wdir.mkdir()
    A.write_wav(str(wdir / "p0.wav"), y, 16000, "PCM_S16")
    # symbol table (k2 format, ids deliberately NOT in sorted-symbol order): token id = rank among the sorted symbols
    syms = ["sil", "a1", "zh", "b", "ang4", "AA0", "_", "n", "i3"]
    stab = tmp_path / "unique_text_tokens.k2symbols"
    stab.write_text("".join(f"{s_} {i + 1}\n" for i, s_ in enumerate(syms)), encoding="utf-8")
    tts = M.Megatts(ck["g"], ypath["g"], ck["plm"], ypath["plm"], ck["adm"], ypath["adm"], str(stab))
    tts.eval()
    assert tts.hifi_gan is not None and tts.hifi_gan.cfg.inference_padding == 5 and tts.hifi_gan.cfg.pad_mode == "reflect"
    phones = ["n", "i3", "sil", "zh", "ang4"]
    rank = {s_: i for i, s_ in enumerate(sorted(syms + ["<eps>"]))}
    phone = np.asarray([rank[s_] for s_ in phones])
    assert tts.ttc.phone2token(phones).tolist() == phone.tolist()
    out_wav = str(tmp_path / "test.wav")
    mel, lens, aux = tts(str(wdir), None, phones=phones, out_path=out_wav)
    prompt = O.mel_spectrogram(A.load_audio(str(wdir / "p0.wav")))
    ref = O.synthesize(sd_g, sd_p, sd_a, g, p, a, phone.astype(np.int64), prompt)
    assert lens[0] == ref["mel"].shape[0] and O.rel_l2(mel[0, :lens[0]].cpu().numpy(), ref["mel"]) < NORTH_STAR
    audio, sr = A.read_wav(out_wav)
    want_gen = O.hifigan(sd_h, tts.hifi_gan.cfg, np.pad(ref["mel"], ((5, 5), (0, 0)), mode="edge"))   # reflect edge mode
    assert sr == 16000 and audio.size == (prompt.shape[0] + 10 + int(lens[0]) + 10) * h.hop
    assert O.rel_l2(audio[-want_gen.size:], want_gen) < 5e-3       # mel round-off amplified by the (random-weight) vocoder


def test_synthesize_list_and_sharded_world1_rccl(tiny_batch):
    """The real `Megatts.synthesize_list` (ragged list -> padded batch) and `dist.synthesize_sharded` on a world-1
    "nccl" (= RCCL) process group: same mels as the padded-tensor entry point, original order kept."""
    import socket
    import torch.distributed as dist
    from megatts2_amd import dist as D, synth
    tts = model("tiny")
    (g, *_), _ = synth_models("tiny")
    rng = np.random.Generator(np.random.PCG64(17))
    utts = [synth.make_utterance(rng, n, t, f, g.mrte.phone_vocab_size) for n, t, f in ((7, 40, 29), (3, 19, 11), (11, 70, 35), (1, 17, 4))]
    mel, lens = tts.synthesize_list(utts)
    mel = mel.cpu().numpy()
    for i, u in enumerate(utts):
        alone, l1 = tts.native.synthesize_batch(dev(u.phone[None]), None, dev(u.prompt_mel[None]), None, forced_dur=u.durations[None],
                                                forced_codes=dev(u.p_codes[None]), run_plm=False)   # records carry p_codes -> forced
        assert lens[i] == l1[0] == int(u.durations.sum())
        assert O.rel_l2(mel[i, :lens[i]], alone[0, :l1[0]].cpu().numpy()) < 2e-6
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    dist.init_process_group("nccl", init_method=f"tcp://127.0.0.1:{port}", rank=0, world_size=1)
    try:
        outs = D.synthesize_sharded(tts, utts)
        assert len(outs) == len(utts)
        for i, o in enumerate(outs):
            assert o.is_cuda and o.shape[0] == lens[i] and O.rel_l2(o.cpu().numpy(), mel[i, :lens[i]]) < 2e-6
    finally:
        dist.destroy_process_group()


def test_prompt_vqpe_inside_the_synthesis_call(tiny_batch):
    """MT2_PROMPT_VQPE: the VQ prosody encoder of the prompt mel on an internal stream beside the ADM gives the same
    codes as the stand-alone call, and leaves every other output of the call unchanged."""
    tts = model("tiny")
    phone, pl = pad_stack([z["phone"] for z in tiny_batch])
    mel, ml = pad_stack([z["prompt_mel"] for z in tiny_batch])
    dur, _ = pad_stack([z["forced_dur"] for z in tiny_batch])
    a, la, auxa = tts.native.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, vocoder=True, return_aux=True)
    b, lb, auxb = tts.native.synthesize_batch(dev(phone), pl, dev(mel), ml, forced_dur=dur, vocoder=True, return_aux=True,
                                              prompt_vqpe=True)
    assert torch.equal(a, b) and torch.equal(auxa["wav"], auxb["wav"]) and torch.equal(auxa["codes"], auxb["codes"])
    _, codes = tts.native.vqpe_forward(dev(mel), ml)
    assert torch.equal(auxb["prompt_codes"], codes[0])
    for i, z in enumerate(tiny_batch):
        want = O.vqpe_forward(synth_models("tiny")[1][0], synth_models("tiny")[0][0], z["prompt_mel"])[1]
        assert np.array_equal(auxb["prompt_codes"][i, :want.size].cpu().numpy(), want)


@pytest.mark.parametrize("kind", ["tiny", "prod"])
def test_prompt_conditioned_synthesis_as_one_call(kind):
    """Row f1 end to end through the mirror: `Megatts.synthesize_prompt_conditioned` (prompt tc_latents length-regulated by
    the prompt's own durations and max-pooled in front of the target's, the prompt's VQ-PE codes behind the BOS) against
    the fixture made by the LIVE reference modules - prompt codes, durations and target codes bit-exact, mel 1e-3; and the
    same utterance twice in one batch."""
    tts = model(kind)
    z = load_golden(f"{kind}_prompted.npz")
    args = (dev(z["phone"][None]), dev(z["prompt_mel"][None]), dev(z["prompt_phone"][None]), z["prompt_dur"][None])
    mel, lens, aux = tts.synthesize_prompt_conditioned(*args, forced_durations=z["forced_dur"][None], return_aux=True)
    n = z["mel"].shape[0]
    assert int(lens[0]) == n
    assert np.array_equal(aux["prompt_codes"][0].cpu().numpy(), z["prompt_codes"])
    assert np.array_equal(aux["dur"][0].cpu().numpy(), z["adm_dur"])
    assert np.array_equal(aux["codes"][0, :z["p_codes"].size].cpu().numpy(), z["p_codes"])
    assert O.rel_l2(mel[0, :n].cpu().numpy(), z["mel"]) < NORTH_STAR
    two = [torch.cat([a, a]) if hasattr(a, "shape") and not isinstance(a, np.ndarray) else np.concatenate([a, a]) for a in args]
    mel2, lens2, aux2 = tts.synthesize_prompt_conditioned(*two, forced_durations=np.concatenate([z["forced_dur"][None]] * 2),
                                                          return_aux=True)
    for b in range(2):
        assert np.array_equal(aux2["codes"][b, :z["p_codes"].size].cpu().numpy(), z["p_codes"])
        assert O.rel_l2(mel2[b, :n].cpu().numpy(), z["mel"]) < NORTH_STAR
    with pytest.raises(ValueError, match="sum to the prompt"):
        tts.synthesize_prompt_conditioned(args[0], args[1], args[2], z["prompt_dur"][None] + 1)
    # round 4: the call above is ONE native entry point (mt2_synthesize_prompt_conditioned: one mel-encoder pass for both phone
    # sets, VQ-PE beside the ADM).  Against round 3's composition of ten stage calls: same discrete outputs, same mel; on a
    # RAGGED pair too (the fixture's utterance beside one with fewer target phones and another split of the prompt alignment),
    # with the vocoder.
    st_mel, st_lens, st_aux = tts.synthesize_prompt_conditioned_staged(*args, forced_durations=z["forced_dur"][None], return_aux=True)
    assert torch.equal(st_aux["codes"][0, :z["p_codes"].size], aux["codes"][0, :z["p_codes"].size])
    assert torch.equal(st_aux["dur"], aux["dur"]) and torch.equal(st_aux["prompt_codes"], aux["prompt_codes"])
    assert O.rel_l2(mel[0, :n].cpu().numpy(), st_mel[0, :n].cpu().numpy()) < TIGHT
    ph2, pd2 = z["phone"][: max(1, z["phone"].size // 2)], z["prompt_dur"].copy()
    pph2 = z["prompt_phone"][:-1] if z["prompt_phone"].size > 1 else z["prompt_phone"]
    pd2 = pd2[:pph2.size].copy()
    pd2[-1] += int(z["prompt_dur"].sum()) - int(pd2.sum())                      # same prompt frames, one phone fewer
    fd2 = z["forced_dur"][:ph2.size]
    phone_b, pl_b = pad_stack([z["phone"], ph2])
    pph_b, ppl_b = pad_stack([z["prompt_phone"], pph2])
    pd_b, _ = pad_stack([z["prompt_dur"], pd2])
    fd_b, _ = pad_stack([z["forced_dur"], fd2])
    mels_b = dev(np.stack([z["prompt_mel"], z["prompt_mel"]]))
    kw = dict(phone_lens=pl_b, prompt_phone_lens=ppl_b, forced_durations=fd_b, vocoder=True, return_aux=True)
    fm, fl, fa = tts.synthesize_prompt_conditioned(dev(phone_b), mels_b, dev(pph_b), pd_b, **kw)
    sm, sl, sa = tts.synthesize_prompt_conditioned_staged(dev(phone_b), mels_b, dev(pph_b), pd_b, **kw)
    assert fl.tolist() == sl.tolist() == [int(z["forced_dur"].sum()), int(fd2.sum())]
    assert np.array_equal(fa["codes"][0, :z["p_codes"].size].cpu().numpy(), z["p_codes"])
    for b in range(2):
        nq = -(-int(fl[b]) // 8)
        assert torch.equal(fa["codes"][b, :nq], sa["codes"][b, :nq]) and torch.equal(fa["dur"][b], sa["dur"][b])
        assert O.rel_l2(fm[b, :fl[b]].cpu().numpy(), sm[b, :fl[b]].cpu().numpy()) < TIGHT
        hop = tts.hifi_gan.cfg.hop
        assert O.rel_l2(fa["wav"][b, :fl[b] * hop].cpu().numpy(), sa["wav"][b, :fl[b] * hop].cpu().numpy()) < 1e-4
        assert not fm[b, fl[b]:].any()


def test_hifigan_reflect_edge_mode():
    """The speechbrain generator's edge mode (`HifiGanConfig.pad_mode = "reflect"`: every 'same' convolution mirrors its
    input at the utterance ends - speechbrain.nnet.CNN.Conv1d's default - instead of zero padding), per utterance inside
    ragged batches, with and without `inference_padding`, against the oracle's reflect form (itself checked against
    torch's F.pad(mode="reflect") in the CPU suite): tiny model on short utterances (edge-dominated) and the production
    generator at 187 + 64 frames.  The two modes differ by > 1e-2 on a short utterance."""
    from megatts2_amd import megatts2 as M, synth
    import dataclasses
    rng = np.random.Generator(np.random.PCG64(79))
    (gt, pt, at, ht), (_, _, _, sd_ht) = synth_models("tiny")
    for pad in (0, 5):
        hr = dataclasses.replace(ht, pad_mode="reflect", inference_padding=pad)
        voc = M.HIFIGAN(hr, sd_ht)
        small = [synth.make_utterance(rng, 1, T, T).prompt_mel for T in (23, 9, 40, 7)]
        mel, ln = pad_stack(small)
        wav = voc.decode_batch(dev(mel).transpose(1, 2).contiguous(), mel_lens=ln).cpu().numpy()
        for i, m in enumerate(small):
            want = O.hifigan(sd_ht, hr, np.pad(m, ((pad, pad), (0, 0)), mode="edge"))
            assert O.rel_l2(wav[i, 0, :want.size], want) < NORTH_STAR, (pad, i)
            assert not wav[i, 0, want.size:].any()
        zero = O.hifigan(sd_ht, ht, np.pad(small[1], ((pad, pad), (0, 0)), mode="edge"))
        assert O.rel_l2(wav[1, 0, :zero.size], zero) > 1e-2
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("prod")
    hr = dataclasses.replace(h, pad_mode="reflect", inference_padding=5)
    voc = M.HIFIGAN(hr, sd_h)
    mels = [synth.make_utterance(rng, 2, T, T).prompt_mel for T in (187, 64)]
    mel, ln = pad_stack(mels)
    wav = voc.decode_batch(dev(mel).transpose(1, 2).contiguous(), mel_lens=ln).cpu().numpy()
    O.enable_torch_kernels()
    try:
        for i, m in enumerate(mels):
            want = O.hifigan(sd_h, hr, np.pad(m, ((5, 5), (0, 0)), mode="edge"))
            assert O.rel_l2(wav[i, 0, :want.size], want) < NORTH_STAR
    finally:
        O.disable_torch_kernels()
