"""No call reads workspace bytes that it did not write (GPU).

Every API call takes its activations from the handle's bump arena (csrc/mt2_model.h, Arena).  A call resets the arena to offset 0
and never clears it: what it finds there is what the previous call left.  Gap rows, pad columns between C and ld, unwritten cache
slots, split-K slabs and statistics pairs are, by convention, either written by their producer or masked by a select in their
consumer - and below the front end model_stages.hip has no memset of an arena buffer, so the convention is all there is.  This file
decides what the arena holds (mt2_workspace_fill) and looks at what a call left (mt2_workspace_peek).

Protocol for one call with inputs B (protocol()), on a handle this file owns, whose arena is ONE chunk reserved up front:
  1  fill 0x00, call -> out0; fill 0xFF, call -> outF.  Every output, on the whole caller buffer (where the binding takes a caller
     buffer it is wider than needed and pre-filled with a sentinel), has the same bits in both; range_fallbacks and the state of
     the fp16 range guard are the same.
  2  fill 0x00, a call of ANOTHER geometry A (more utterances, other ragged lengths: every internal offset moves), then B with no
     fill in between: the bits of out0.  Stale but finite values - a max or a comparison over them - are what the NaN run cannot see.
  3  after every call the capacity is what it was (no allocation escaped the poisoned chunk), high_water > 0, and the arena bytes
     in [high_water, capacity) still hold the fill pattern (the call did not write beyond what it reports).
0xFF bytes are NaN as f32 and -1 as int32 / int64, which the row kernels treat as "no row" (idmap / rowmap / map < 0: zeros;
kInvalidRow < 0; check_ids flags a negative id).  No pattern that reads as a large positive integer is used: a stale index would
address memory that nobody owns.  No tolerance appears in this file: every bar is bit equality.

Arena buffers of integers that the DEVICE writes, read from the code before the first run: each is written whole, or memset, before a
kernel uses it as an index (host-built index arrays go up whole through IntPlan::upload):
  durations       capi.inc mt2_synthesize_batch: `dur_dev` is memset whole before the ADM runs; adm_finalize_kernel (rowops.hip)
                  writes every [slot, t < nmax]; the host reads them back to plan the frames (plan_frames refuses a negative one).
  codes           model_stages.hip PlmStage::begin `codes_all`: plm_init_hist_kernel writes all [A, cstride] words of every group
                  (BOS, prefix, zeros) before the first step; plm_step_input_kernel reads positions < n through clamp_id; capi.inc
                  `cdev` is memset whole before plm_finalize_kernel writes [slot, t < nt].
  VQ indices      model_stages.hip vqpe_rows `r.idx`: vq_argmin_kernel writes every row m < Q.R (0 in a gap row); gathered through
                  the host-built code map only.
  vocoder masks   hifigan_rows `v2`: expand_mask_kernel writes all R x s words from the previous (host-built) mask.
  DTW directions  dtw_run `p.dirs`: the accumulate kernel writes the words of every cell of the matrix; the backtrack loads words of
                  rows r >= 0, c >= 0 that may be unwritten but uses only those of cells on the path, and forces the move at i == 0 /
                  j == 0 ("whatever the word says, the walk stays inside the matrix").
  Viterbi psi     f0_track_run `q.psi`: row 0 and every (t, k) of the utterance's frames are written; the backward walk clamps
                  every state to n - 1.
  trim words      trim_run `words` (peak | first | last): memset (0, then 0xFF = UINT_MAX / -1) before launch_trim; trim_bounds
                  clamps on the host.
  arg-max / draws launch_argmax_rows / launch_sample_rows / launch_sample_mix_rows write codes[j, n] of every active sequence j, the
                  one position the next step reads beyond those already written.
  align durations align_durations_run `p.dur | p.last`: dtw_durations_kernel writes every [b, ph < Np_max] and last[b]; read on the host.

Measured on an MI355X: every case passes; no call was found to read bytes it had not written.  By hand, not committed: without
the hipMemsetAsync(Rprev, ...) of griffin_lim_run the `griffin_lim` case fails (640 of 1181 samples NaN on the 0xFF arena);
with pack_rows_kernel leaving its gap rows unwritten 15 cases fail (tc_latent, mel_context, vqpe_forward, mel_decoder, both
synthesis calls, every zero-padded vocoder case; reflect mode mirrors into its gaps and passes).  Without the
hipMemsetAsync(S, ...) of istft_run - "0 x garbage must not be NaN" - `istft` and `griffin_lim` still pass: launch_pack_rows
behind it writes all lds columns of every row of S, gap rows and pad columns included, so that memset guards nothing today.

Geometry partners: the AR cases `tiled` <-> `first` and `around-64` <-> `long-q`; the vocoder's `equal` before `edges` and `edges`
before `pad5`; prod-reflect takes `equal` too, because reflect mode refuses the one-frame utterance of `edges` (as F.pad does).
Reserves: AR_RESERVE, VOC_RESERVE, FE_RESERVE, SMALL_RESERVE below for the stage calls; the tiny handle max(TINY_RESERVE, the
mt2_workspace_query bound of its largest synthesis call).
"""
import contextlib
import ctypes

import numpy as np
import pytest

import ar_step_ref as AR
import f0_ref as F0
import griffinlim_ref as GL
import megatts2_oracle as O
import resample_ref as RS
import trim_ref as TR
import voc_ref as VR
from conftest import load_golden, synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MiB = 1 << 20
AR_RESERVE = 64 * MiB           # adm_infer / plm_infer at production size, up to 4 x 71 and 1 x 192 positions
VOC_RESERVE = 256 * MiB         # mt2_hifigan, production widths, up to 79 frames in 4 utterances (reflect: gaps of 8 frames)
TINY_RESERVE = 64 * MiB         # the stage calls of the tiny model
FE_RESERVE = 64 * MiB           # MelFrontEnd, production audio config
SMALL_RESERVE = 16 * MiB        # MelFrontEnd, the "small" config of test_gpu_griffinlim.py
SENT = -77.25
GUARD = 11


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def pad_stack(arrs, fill=0):
    n = max(a.shape[0] for a in arrs)
    out = np.full((len(arrs), n) + arrs[0].shape[1:], fill, arrs[0].dtype)
    for i, a in enumerate(arrs):
        out[i, :a.shape[0]] = a
    return out, np.asarray([a.shape[0] for a in arrs], np.int32)


def sentinel(*shape, dtype=torch.float32):
    """(the whole buffer, its [shape] view): a caller buffer with GUARD words behind it, pre-filled with the sentinel"""
    n = int(np.prod(shape))
    buf = torch.full((n + GUARD,), SENT, device="cuda", dtype=dtype)
    return buf, buf[:n].view(*shape)


@contextlib.contextmanager
def options(nat, opts):
    prev = {k: nat.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            nat.set_option(k, v)
        yield
    finally:
        for k, v in prev.items():
            nat.set_option(k, v)


# ---------------------------------------------------------------------------------------------------
# the protocol

def flat(out, name="out"):
    """every array of a call's result, as (name, host array), in a fixed order"""
    if out is None:
        return []
    if isinstance(out, dict):
        return [x for k in sorted(out) for x in flat(out[k], f"{name}.{k}")]
    if isinstance(out, (tuple, list)):
        return [x for i, v in enumerate(out) for x in flat(v, f"{name}[{i}]")]
    if hasattr(out, "detach"):
        out = out.detach()
        out = (torch.view_as_real(out) if out.is_complex() else out).cpu().numpy()
    return [(name, np.ascontiguousarray(np.asarray(out)).copy())]


def same_bits(a, b, what):
    assert [n for n, _ in a] == [n for n, _ in b], what
    for (n, x), (_, y) in zip(a, b):
        assert x.shape == y.shape and x.dtype == y.dtype, (what, n)
        xb, yb = x.reshape(-1).view(np.uint8), y.reshape(-1).view(np.uint8)
        if not np.array_equal(xb, yb):
            bad = np.flatnonzero(xb != yb) // x.dtype.itemsize
            where = np.unravel_index(int(bad[0]), x.shape) if x.ndim else ()
            raise AssertionError(f"{what}: {n} {x.shape} differs in {np.unique(bad).size} of {x.size} elements, first at {where}: "
                                 f"{x.reshape(-1)[bad[0]]!r} against {y.reshape(-1)[bad[0]]!r}")


def guard_state(h):
    t = ctypes.c_int(0)
    assert h.lib.mt2_x3h_guard(h.h, ctypes.byref(t)) == 0
    return t.value


def arena_after(h, cap, fill, what):
    """step 3: the capacity is unchanged, the high-water mark is set, the bytes behind it still hold the fill pattern"""
    assert h.memory()[1] == cap, f"{what}: the arena grew from {cap} to {h.memory()[1]} bytes: an allocation escaped the poisoned chunk"
    hw = h.workspace_high_water()
    assert 0 < hw <= cap, (what, hw, cap)
    for off in range(hw, cap, 64 * MiB):
        tail = h.workspace_peek(off, min(64 * MiB, cap - off))
        assert (tail == fill).all(), f"{what}: bytes behind the high-water mark {hw} were written (first at {off + int(np.flatnonzero(tail != fill)[0])})"


def protocol(h, call_b, call_a, what, log=False):
    """Steps 1 - 3 of the docstring for the call `call_b`, with `call_a` the call of another geometry -> the form log of the 0xFF run"""
    cap = h.memory()[1]

    def one(call, fill, tag, want_log=False):
        fallbacks = getattr(h, "range_fallbacks", 0)
        if want_log:
            h.form_log_begin()
        try:
            out = call()
            torch.cuda.synchronize()
        finally:
            entries = h.form_log_end() if want_log else None
        state = (getattr(h, "range_fallbacks", 0) - fallbacks, guard_state(h))
        arena_after(h, cap, fill, f"{what} [{tag}]")
        return flat(out), state, entries

    h.workspace_fill(0x00)
    out0, state0, _ = one(call_b, 0x00, "0x00")
    h.workspace_fill(0xFF)
    outf, statef, entries = one(call_b, 0xFF, "0xFF", log)
    same_bits(out0, outf, f"{what}: arena of 0xFF bytes against an arena of zeros")
    assert state0 == statef, f"{what}: (range_fallbacks, guard) {state0} on zeros, {statef} on 0xFF"
    h.workspace_fill(0x00)
    one(call_a, 0x00, "geometry A")
    outs, states, _ = one(call_b, 0x00, "after A")
    same_bits(out0, outs, f"{what}: after a call of another geometry against an arena of zeros")
    assert state0 == states, f"{what}: (range_fallbacks, guard) {state0} on zeros, {states} after another geometry"
    print(f"{what}: high water {h.workspace_high_water()} of {cap} bytes")
    return entries


def one_chunk(h, nbytes):
    """step 0, on a fresh handle: exactly one chunk of nbytes"""
    assert h.memory()[1] == 0, "the handle has been used: its arena already has a chunk"
    h.workspace_reserve(nbytes)
    assert h.memory()[1] == nbytes
    return h


# ---------------------------------------------------------------------------------------------------
# the hooks themselves

@pytest.fixture(scope="module")
def tiny():
    from megatts2_amd.runtime import NativeModel
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    nat = NativeModel(g, p, a, h, sd_g=sd_g, sd_plm=sd_p, sd_adm=sd_a, sd_hifigan=sd_h)
    batch_a = tiny_synth_inputs(TINY_A)
    Np, Tp, Tm = batch_a["phone"].shape[1], batch_a["mel"].shape[1], batch_a["tm_cap"]
    bound = max(nat.workspace_query(len(TINY_A), Np, Tp, Tm, run_plm=True, vocoder=True, prompt_vqpe=True), TINY_RESERVE)
    print(f"tiny handle: reserve {bound} bytes")
    yield one_chunk(nat, bound)
    nat.close()


def test_hooks_fill_peek_and_wait():
    from megatts2_amd.runtime import NativeError, NativeModel
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    nat = one_chunk(NativeModel(g, p, a, h, sd_g=sd_g, sd_plm=sd_p, sd_adm=sd_a, sd_hifigan=sd_h), TINY_RESERVE)
    try:
        opts = {k: nat.get_option(k) for k in ("x3h", "ar_groups", "splitk", "a_planes")}
        nat.workspace_fill(0xA5)
        cap = nat.memory()[1]
        assert cap == TINY_RESERVE and nat.workspace_high_water() == 0
        assert {k: nat.get_option(k) for k in opts} == opts
        for off in (0, (cap // 2) & ~255, cap - 256):
            got = nat.workspace_peek(off, 256)
            assert got.dtype == np.uint8 and got.shape == (256,) and (got == 0xA5).all(), off
        assert nat.workspace_peek(cap, 0).size == 0
        for off, n in ((cap - 255, 256), (cap + 1, 0), (0, cap + 1)):
            with pytest.raises(NativeError, match="leaves the arena"):
                nat.workspace_peek(off, n)
        with pytest.raises(NativeError, match="0..255"):
            nat.workspace_fill(256)
        b = tiny_synth_inputs(TINY_B)
        kw = dict(forced_dur=b["dur"], vocoder=True, return_aux=True, check_range=False)
        want = flat(nat.synthesize_batch(dev(b["phone"]), b["pl"], dev(b["mel"]), b["ml"], **kw))
        hw = nat.workspace_high_water()
        assert 0 < hw <= cap and nat.memory()[1] == cap
        assert not (nat.workspace_peek(0, hw) == 0xA5).all()            # the call wrote below its high-water mark ...
        assert (nat.workspace_peek(hw, cap - hw) == 0xA5).all()         # ... and nowhere behind it
        # a fill while a call is in flight on another stream waits for that call: the call's result is the unfilled one
        phone, mel = dev(b["phone"]), dev(b["mel"])
        side = torch.cuda.Stream()
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            out = nat.synthesize_batch(phone, b["pl"], mel, b["ml"], **kw)
        nat.workspace_fill(0xFF)
        assert (nat.workspace_peek(0, 4096) == 0xFF).all() and nat.workspace_high_water() == hw
        torch.cuda.synchronize()
        same_bits(want, flat(out), "a fill behind a call in flight on another stream")
    finally:
        nat.close()


# ---------------------------------------------------------------------------------------------------
# AR stages: production-size synthetic models, the cases of tests/ar_step_ref.py

AR_CASES = ("first", "around-64", "tiled", "long-q")
AR_PARTNER = {"first": "tiled", "tiled": "first", "around-64": "long-q", "long-q": "around-64"}
AR_SETTINGS = {"default": {}, "x3h=0": {"x3h": 0}, "a_planes=7": {"a_planes": 7}, "splitk=0": {"splitk": 0},
               "groups=2": {"adm_groups": 2, "plm_groups": 2}}
AR_PARAMS = [pytest.param(m, c, s, id=f"{m}-{c}-{s}") for m in ("adm", "plm") for s in AR_SETTINGS for c in AR_CASES]
# what the 0xFF runs have to reach, or a pass says nothing about those buffers: (decision point, form) as form_keys names them
AR_FORMS = {("ln_linear", "skinny-ln-pairs"), ("ln_linear", "pair-fed"), ("residual", "split"), ("ln_pending", "reduce"),
            ("ln_linear", "plain+planes"), ("attention", "x3h")}


@pytest.fixture(scope="module")
def ar():
    from megatts2_amd.runtime import NativeModel
    (g, p, a, h), (_, sd_p, sd_a, _) = AR.synth_models("prod")
    nat = NativeModel(g, p, a, h, sd_plm=sd_p, sd_adm=sd_a)
    nat.set_option("adm_groups", 1)          # M is per stream group: the default ar_groups = 2 would halve it
    nat.set_option("plm_groups", 1)
    yield one_chunk(nat, AR_RESERVE)
    nat.close()


def ar_call(nat, model, case):
    lens, P, steps = AR.CASES[case]
    cond, hist = AR.inputs(model, case)
    ln, cond, hist = np.asarray(lens, np.int32), dev(cond), dev(hist) if P else None
    if AR.is_adm(model):
        return lambda: nat.adm_infer(cond, ln, return_float=True, p_prefix=hist, max_steps=steps)
    return lambda: nat.plm_infer(cond, ln - P, return_logits=True, prefix_codes=hist, max_steps=steps)


_AR_LOGS = {}


def ar_run(nat, model, case, setting):
    key = (model, case, setting)
    if key not in _AR_LOGS:
        with options(nat, AR_SETTINGS[setting]):
            _AR_LOGS[key] = protocol(nat, ar_call(nat, model, case), ar_call(nat, model, AR_PARTNER[case]),
                                     f"{model}_infer {case} [{setting}]", log=True)
    return _AR_LOGS[key]


@pytest.mark.parametrize("model,case,setting", AR_PARAMS)
def test_ar_stages(ar, model, case, setting):
    assert ar_run(ar, model, case, setting), "the form log of the 0xFF run is empty"


def test_ar_poisoned_runs_reach_the_forms_with_buffers_of_their_own(ar):
    seen = set()
    for p in AR_PARAMS:
        for kind, point, form, attrs in ar_run(ar, *p.values):
            seen.add((point, form))
            if point == "attention" and attrs.get("o_planes"):
                seen.add(("attention", "o_planes"))
    print("forms of the 0xFF runs:", sorted(seen))
    assert not (AR_FORMS | {("attention", "o_planes")}) - seen, sorted((AR_FORMS | {("attention", "o_planes")}) - seen)


# ---------------------------------------------------------------------------------------------------
# vocoder: the generators and cases of tests/voc_ref.py

VOC_CASE = {"prod": ("edges", "equal"), "prod-reflect": ("reflect", "equal"), "prod-pad5": ("pad5", "edges"), "wide-tail": ("edges", "equal")}
VOC_SETTINGS = {"default": {}, "pair_fuse=0,up_fuse=0": {"pair_fuse": 0, "up_fuse": 0}, "voc_streams=1": {"voc_streams": 1}}
VOC_PARAMS = [pytest.param(g, s, id=f"{g}-{VOC_CASE[g][0]}-{s}") for g in VR.GENERATORS for s in VOC_SETTINGS]


@pytest.fixture(scope="module")
def voc():
    from megatts2_amd import megatts2 as M
    handles = {g: M.HIFIGAN(*VR.generator(g)) for g in VR.GENERATORS}
    yield {g: one_chunk(h.native, VOC_RESERVE) for g, h in handles.items()}
    for h in handles.values():
        h.native.close()


def voc_call(nat, case):
    mels, lens = VR.mels(case), np.asarray(VR.CASES[case], np.int32)
    mel = np.zeros((len(mels), 80, int(lens.max())), np.float32)
    for b, m in enumerate(mels):
        mel[b, :, :m.shape[0]] = m.T
    mel = dev(mel)
    return lambda: nat.hifigan(mel, lens)


@pytest.mark.parametrize("gen,setting", VOC_PARAMS)
def test_vocoder(voc, gen, setting):
    nat, (case, partner) = voc[gen], VOC_CASE[gen]
    with options(nat, VOC_SETTINGS[setting]):
        log = protocol(nat, voc_call(nat, case), voc_call(nat, partner), f"hifigan {gen} {case} [{setting}]", log=True)
    forms = {(k, p, f) for k, p, f, _ in log}
    assert forms, "the form log of the 0xFF run is empty"
    last = f"voc-stage{len(VR.generator(gen)[0].upsample_rates) - 1}"
    if setting == "pair_fuse=0,up_fuse=0":      # the multi-launch forms, with their intermediate buffers
        assert (last, "pair", "two") in forms and not any(f == "fused" for _, p, f in forms if p in ("pair", "upsample")), sorted(forms)
    assert (last, "streams", "1" if setting == "voc_streams=1" else "3") in forms, sorted(forms)


# ---------------------------------------------------------------------------------------------------
# the tiny model: a ragged batch of three (B), and five utterances in another order (A)

TINY_B, TINY_A = (0, 1, 2), (3, 0, 2, 1, 3)


def tiny_utts(which):
    return [load_golden(f"tiny_utt{i}.npz") for i in which]


def tiny_synth_inputs(which):
    zs = tiny_utts(which)
    phone, pl = pad_stack([z["phone"] for z in zs])
    mel, ml = pad_stack([z["prompt_mel"] for z in zs])
    dur, _ = pad_stack([z["forced_dur"] for z in zs])
    tm_cap = max(int(z["adm_dur"].sum()) for z in zs) + 3
    return {"phone": phone, "pl": pl, "mel": mel, "ml": ml, "dur": dur, "tm_cap": tm_cap}


def tiny_prompted_inputs(n):
    """the fixture's utterance beside n - 1 others with fewer target phones and another split of the prompt alignment (the ragged pair
    of test_gpu_stages.py::test_prompt_conditioned_synthesis_as_one_call, continued)"""
    z = load_golden("tiny_prompted.npz")
    phones, pphones, pdurs, fdurs = [z["phone"]], [z["prompt_phone"]], [z["prompt_dur"]], [z["forced_dur"]]
    for k in range(1, n):
        ph = z["phone"][:max(1, z["phone"].size - 2 * k - 1)]
        pph = z["prompt_phone"][:max(1, z["prompt_phone"].size - k)]
        pd = z["prompt_dur"][:pph.size].copy()
        pd[-1] += int(z["prompt_dur"].sum()) - int(pd.sum())                      # the same prompt frames, fewer phones
        phones.append(ph), pphones.append(pph), pdurs.append(pd), fdurs.append(z["forced_dur"][:ph.size])
    (phone, pl), (pph, ppl) = pad_stack(phones), pad_stack(pphones)
    return {"phone": phone, "pl": pl, "pph": pph, "ppl": ppl, "pd": pad_stack(pdurs)[0], "fd": pad_stack(fdurs)[0],
            "mel": np.stack([z["prompt_mel"]] * n)}


def tiny_call(nat, name, which):
    """the call `name` on the utterances `which` -> a closure that makes it (inputs go to the device once, here)"""
    from megatts2_amd.sampling import PLMSampling
    zs = tiny_utts(which)
    B = len(zs)
    if name in ("tc_latent", "mel_context", "synthesize_batch"):
        s = tiny_synth_inputs(which)
        phone, mel = dev(s["phone"]), dev(s["mel"])
        if name == "tc_latent":
            return lambda: nat.tc_latent(phone, mel, s["pl"], s["ml"])
        if name == "mel_context":
            return lambda: nat.mel_context(mel, s["ml"])
        return lambda: nat.synthesize_batch(phone, s["pl"], mel, s["ml"], run_plm=True, vocoder=True, tm_cap=s["tm_cap"], return_aux=True)
    if name == "synthesize_prompt_conditioned":
        s = tiny_prompted_inputs(B)
        phone, mel, pph = dev(s["phone"]), dev(s["mel"]), dev(s["pph"])
        return lambda: nat.synthesize_prompt_conditioned(phone, s["pl"], mel, None, pph, s["ppl"], s["pd"], forced_dur=s["fd"], vocoder=True)
    if name == "length_regulate":
        tc, ln = pad_stack([z["tc_latent"] for z in zs])
        dur, tc = pad_stack([z["forced_dur"] for z in zs])[0], dev(tc)
        return lambda: nat.length_regulate(tc, dur, ln)
    if name == "max_pool_ceil":
        x, ln = pad_stack([O.length_regulate(z["tc_latent"], z["forced_dur"]) for z in zs])
        x = dev(x)
        return lambda: nat.max_pool_ceil(x, 8, ln)
    if name in ("plm_infer", "plm_infer_interpolated"):
        cond, ln = pad_stack([z["plm_cond"] for z in zs])
        rev, cond = dev(pad_stack([z["plm_cond"][::-1] for z in zs])[0]), dev(cond)
        kw = dict(return_logits=True, sampling=PLMSampling(0.8, 40, 0.95), seeds=np.arange(B, dtype=np.int64) * 77 + 3)
        if name == "plm_infer":
            return lambda: nat.plm_infer(cond, ln, **kw)
        return lambda: nat.plm_infer_interpolated(cond, rev, ln, 0.5, **kw)
    if name == "vq_decode":
        codes = dev(pad_stack([z["p_codes"] for z in zs])[0][None])
        return lambda: nat.vq_decode(codes)
    if name == "vq_quantize":
        x = dev(np.concatenate([z["vqpe_ze"] for z in zs]))
        return lambda: nat.vq_quantize(x)
    if name == "vqpe_forward":
        mel, ln = pad_stack([z["target_mel"] for z in zs])
        mel = dev(mel)
        return lambda: nat.vqpe_forward(mel, ln, return_ze=True)
    if name == "mel_decoder":
        x, ln = pad_stack([z["decoder_in"] for z in zs])
        x = dev(x).transpose(1, 2).contiguous()
        return lambda: nat.mel_decoder(x, ln)
    if name in ("dtw", "align_durations"):      # the synthetic mel (sum of the forced durations) warped onto the prompt's
        (X, xl), (Y, yl) = pad_stack([z["mel"] for z in zs]), pad_stack([z["prompt_mel"] for z in zs])
        X, Y = dev(X), dev(Y)
        if name == "dtw":
            return lambda: nat.dtw(X, Y, xl, yl, return_cost=True, return_acc=True)
        hi, (dur, pl) = nat.dtw(X, Y, xl, yl)["hi"], pad_stack([z["forced_dur"] for z in zs])
        return lambda: nat.align_durations(hi, yl, dur, pl)
    raise KeyError(name)


TINY_CALLS = ("tc_latent", "mel_context", "length_regulate", "max_pool_ceil", "plm_infer", "plm_infer_interpolated", "vq_decode",
              "vq_quantize", "vqpe_forward", "mel_decoder", "synthesize_batch", "synthesize_prompt_conditioned", "dtw", "align_durations")


@pytest.mark.parametrize("name", TINY_CALLS)
def test_tiny_model(tiny, name):
    protocol(tiny, tiny_call(tiny, name, TINY_B), tiny_call(tiny, name, TINY_A), f"tiny {name}")


# ---------------------------------------------------------------------------------------------------
# MelFrontEnd: the production audio config, and the "small" one of test_gpu_griffinlim.py for the STFT family

def small_audio():
    from megatts2_amd.config import AudioConfig
    return AudioConfig(sample_rate=16000, n_fft=64, hop_length=16, win_length=64, n_mels=8, f_min=0.0, f_max=8000.0)


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    handles = {"prod": one_chunk(MelFrontEnd(), FE_RESERVE), "small": one_chunk(MelFrontEnd(small_audio()), SMALL_RESERVE)}
    yield handles
    for h in handles.values():
        h.close()


def rows_16k(which):
    """ragged utterances at 16 kHz: the signals of test_gpu_f0.py / test_gpu_prosody.py (harmonic tones, noise, silence)"""
    if which == "B":
        return [F0.tone(220.5, 3000, F0.HARMONICS[1], seed=3000), F0.white(2000, 0.1, seed=5), F0.tone(110.0, 1025, F0.HARMONICS[2], seed=9)]
    return [F0.white(4000, 0.1, seed=5), np.zeros(1500, np.float32), F0.tone(146.83, 5000, F0.HARMONICS[1], seed=1), F0.tone(70.0, 2500, F0.HARMONICS[0], seed=2),
            F0.tone(440.0, 700, F0.HARMONICS[2], seed=4)]


def rows_44k(which):
    """the resampler's test signal (test_gpu_resample.py): 0.2 N(0, 1) noise + the three tones, at 44.1 kHz"""
    out = []
    for L in ((9000, 5000, 12001) if which == "B" else (3000, 15000, 7000, 11000)):
        rng = np.random.default_rng(44100 % 997 + L)
        out.append((0.2 * rng.standard_normal(L) + RS.tones(44100, L, 44100)).astype(np.float32))
    return out


def rows_trim(which):
    """test_gpu_trim.py::test_ragged_batch_is_its_utterances_alone"""
    if which == "B":
        return [TR.burst_signal(16000, "interior", seed=1), np.array([0.25], np.float32), TR.burst_signal(5000, "end", seed=2), np.zeros(3000, np.float32)]
    return [TR.burst_signal(5000, "start", seed=3), TR.burst_signal(20000, "interior", seed=4), TR.burst_signal(2049, "end", seed=5)]


def rows_loud(which):
    """noise under a slow envelope (the signal of test_gpu_loudness.py): one utterance over a second, one just over 0.4 s, one under"""
    out = []
    for seed, L in enumerate((20000, 6500, 3000) if which == "B" else (8000, 30000, 1, 12000)):
        rng = np.random.default_rng(1000 * seed + L % 997)
        env = 10.0 ** (-1.0 - 1.0 * np.sin(2 * np.pi * 0.45 * np.arange(L) / 16000 + seed))
        out.append((0.5 * env * rng.standard_normal(L)).astype(np.float32))
    return out


def mel_like(T, D, seed):
    """test_gpu_dtw.py: a smooth random walk with a little noise, in the range of a log-mel"""
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.standard_normal((T, D)), axis=0) * 0.3 + rng.standard_normal((T, D)) * 0.05 - 4.0).astype(np.float32)


def nan_stack(rows, extra=7):
    wav, lens = pad_stack([np.asarray(r, np.float32) for r in rows], fill=np.nan)
    return dev(np.concatenate([wav, np.full((len(rows), extra), np.nan, np.float32)], axis=1)), lens


def fe_call(handles, name, which):
    small = name in ("stft", "istft", "mel_to_linear", "griffin_lim")
    h = handles["small" if small else "prod"]
    hop = h.audio.hop_length
    if small:
        a = h.audio
        Ts = (5, 37) if which == "B" else (21, 4, 37, 9)
        xs = [GL.two_tone_noise((T - 1) * hop, a.sample_rate, seed=T) if T in (4, 37) else GL.vibrato_stack((T - 1) * hop, a.sample_rate) for T in Ts]
        Tn = np.asarray(Ts, np.int32)
        if name == "stft":
            wav, lens = nan_stack(xs, 5)
            return lambda: h.stft(wav, lens)
        if name == "istft":
            spec = dev(pad_stack([GL.stft(x, a).astype(np.complex64) for x in xs], fill=np.nan + 1j * np.nan)[0])
            def call():
                buf, out = sentinel(len(Ts), (max(Ts) - 1) * hop + 7)
                h.istft(spec, Tn, out=out)
                return buf
            return call
        mel = dev(pad_stack([GL.log_mel(x, a) for x in xs], fill=np.nan)[0])
        if name == "mel_to_linear":
            return lambda: h.mel_to_linear(mel, Tn)
        seeds = np.asarray([11, 2 ** 40 + 5, 7, 8][:len(Ts)], np.uint64)
        def call():
            wbuf, out = sentinel(len(Ts), (max(Ts) - 1) * hop + 9)
            rbuf, resid = sentinel(len(Ts), 3, mel.shape[1])
            h.griffin_lim(mel, Tn, n_iter=2, momentum=0.99, seeds=seeds, return_resid=True, out=out, resid_out=resid)
            return wbuf, rbuf
        return call
    if name in ("resample", "from_audio"):
        wav, lens = nan_stack(rows_44k(which))
        if name == "from_audio":
            return lambda: h.from_audio(wav, 44100, lens, trim_db=40.0, return_bounds=True)
        def call():
            buf, out = sentinel(len(lens), max(RS.out_len(44100, 16000, int(n)) for n in lens) + 5)
            return buf, h.resample(wav, 44100, lens, normalize=True, out=out)[1]
        return call
    if name == "trim":
        wav, lens = nan_stack(rows_trim(which))
        def call():
            buf, out = sentinel(len(lens), int(lens.max()) + 5)
            _, out_lens, bounds, energy = h.trim(wav, lens, 40.0, out=out, return_energy=True)
            return buf, out_lens, bounds, energy
        return call
    if name in ("loudness", "loudness_normalize"):
        wav, lens = nan_stack(rows_loud(which))
        if name == "loudness":
            return lambda: h.loudness(wav, lens, return_momentary=True)
        def call():
            buf, out = sentinel(*wav.shape)
            return buf, h.loudness_normalize(wav, lens, -23.0, 0.9, out=out, return_stats=True)[1]
        return call
    if name == "dtw":
        shapes = ((40, 50), (17, 9), (64, 65)) if which == "B" else ((9, 30), (70, 20), (1, 5), (33, 33))
        (X, xl), (Y, yl) = (pad_stack([mel_like(s[k], 8, 10 * i + k) for i, s in enumerate(shapes)], fill=np.nan) for k in (0, 1))
        X, Y = dev(X), dev(Y)
        return lambda: h.dtw(X, Y, xl, yl, return_cost=True, return_acc=True)
    wav, lens = nan_stack(rows_16k(which))
    T = 1 + int(lens.max()) // hop + 3
    if name == "mel":
        return lambda: h(wav, lens)
    if name in ("f0", "f0_track"):
        def call():
            buf, out = sentinel(len(lens), T)
            return (buf,) + tuple(getattr(h, name)(wav, lens, return_cmnd=True, return_lag=True, return_diff=True, out=out)[1:])
        return call
    if name == "energy":
        def call():
            buf, out = sentinel(len(lens), T)
            h.energy(wav, lens, out=out)
            return buf
        return call
    f0 = h.f0(wav, lens)                    # an input of the two calls below, made once
    fl = (1 + lens // hop).astype(np.int32)
    if name == "pitch_contour":
        return lambda: h.pitch_contour(f0, fl, return_index=True)
    assert name == "phone_prosody"
    energy = h.energy(wav, lens)
    dur = np.zeros((len(lens), 5), np.int32)
    for b, n in enumerate(fl):              # four phones that share the frames, the last one running past them; the fifth is padding
        dur[b, :4] = (n // 4, n // 4 + 1, 0, n - 2 * (n // 4) + 2)
    return lambda: h.phone_prosody(f0, dur, energy, phone_lens=np.full(len(lens), 4, np.int32), frame_lens=fl, return_sum=True)


FE_CALLS = ("mel", "from_audio", "resample", "trim", "loudness", "loudness_normalize", "f0", "f0_track", "energy", "phone_prosody",
            "pitch_contour", "dtw", "stft", "istft", "mel_to_linear", "griffin_lim")


@pytest.mark.parametrize("name", FE_CALLS)
def test_front_end(fe, name):
    h = fe["small" if name in ("stft", "istft", "mel_to_linear", "griffin_lim") else "prod"]
    protocol(h, fe_call(fe, name, "B"), fe_call(fe, name, "A"), f"front end {name}")
