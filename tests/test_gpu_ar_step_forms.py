"""Every form of the autoregressive step wiring against a float64 step (GPU).

csrc/model_stages.hip chains 50 - 70 kernel launches into one AR step of the ADM / PLM and decides, from the row count M = A n, from
K and from ~25 run-time options, WHICH kernels: LayerNorm -> Linear as the weight-streaming kernel normalising its own rows, the
same fed by 16-column pairs, the pair-fed algebraic LayerNorm, or launch_layernorm + GEMM with or without fp16 planes; the residual
GEMMs K-split through launch_ln_reduce or un-split with / without a statistics epilogue; the first layer filling or extending its
QKV cache; three forms of the last layer; six attention kernels; three arithmetic pipes.  Every form claims to be an exact identity
of TransformerEncoderLayer.forward.  This file runs the cases of tests/ar_step_ref.py (production-size models, a different sequence
in every slot, lengths not in sorted order) under every option setting of SETTINGS and asserts per (case, setting, step):

  parity    PLM: relative L2 of each sequence's logits to the float64 step <= BAR = 8 x E32(plm); ADM: |p - p64| / max(1, |p64|) <=
            8 x E32(adm).  E32 is the float32 numpy oracle's own worst error against the float64 step over the cases
            (tests/test_ar_step_ref_host.py).  Steps after the first of a call are judged on the history the device used: its own
            float (ADM), its own code (PLM, which must be the float64 arg-max - the margins of the host test make that safe).
  discrete  the PLM code is the float64 arg-max, the forced history comes back untouched, positions at or beyond a length are zero.
  witness   a setting names the form it is there to reach (layer kind, decision point, form, fields); the form log
            (mt2_form_log_begin / _end) of its run shows that entry and the log of the default run of the same case does not.
  identity  the a_planes settings give bit-identical results among themselves (test_planes_hand_offs_are_bit_identical).
  coverage  over the whole file every (layer kind, form) the log can emit at these shapes is reached (test_every_form_is_reached).

The generic attention kernel serves heads wider than 128 columns and the production heads are 96 (ADM) and 64 (PLM) wide, so a
small PLM with two heads of 256 (model "wide" of ar_step_ref) runs the cases "first" and "around-64" under the default options;
case "long-incr" exists because only a second step at more than 128 positions runs the register kernel on the incremental cache,
and case "long-q" (192 queries: the default attn_x6_min) because below it switching the bf16 / fp16-pipe attention off changes nothing.

Measured on an MI355X (test_every_form_is_reached prints both tables, pytest -s).  E32 = 1.98e-6 (adm), 1.03e-6 (plm), 4.9e-7
(wide); the bar is error / E32 <= 8.  Worst error / E32 over all cases and steps, per setting:
    setting                        adm    plm   wide        setting                        adm    plm
    default                        0.63   0.41   0.70       ln_pairs_maxm=64               0.63   0.41
    x3h=0                          0.63   0.65              a_planes=0 / 1 / 2 / 4 / 7     0.63   0.41
    x3h=0,x6_gemm=0                0.63   0.55              attn_lds_min=32                0.63   0.41
    x6_ks=0 / 1 / 5                0.63   0.41              attn_x6_min=32,x3h=15 / 7      0.63   0.41
    splitk=0                       0.63   0.45              attn_lds_min=0,attn_x6_min=0   0.63   0.41
    skinny_tm=0                    0.69   0.46              t_x3h_128=1                    1.24   0.41
    skinny_pairs=0                 0.49   0.41              t_x3h_128=100000               0.63   0.41
    skinny_rows=16                 0.63   0.41              force_gemm_config=12           1.36   1.09
    skinny_nw=8                    0.45   0.52              groups=2 / 3                   0.63   0.41
    ln_pairs_adm=0 / 1 / 2         0.63
and per form.  A call's worst step is booked on the forms of a default run, and for any other setting only on the forms that the
default run of the same case does not show - the forms the setting brings to the case, not every form that took part:
    ln_linear   skinny-ln 0.70  skinny-ln-pairs 0.70  pair-fed 0.34  plain 1.36  plain+planes 0.50
    residual    split 1.36  stat 0.70  nostat 1.36          ln_pending  reduce 1.36          tail  fpl 0.38  nofpl 0.93
    attention   ds 0.63  reg 0.35  generic 0.70  lds 0.37  x6 0.52  x3h 0.36  ds+o_planes 0.38  reg+o_planes 0.35  x3h+o_planes 0.32
    layer       first-fill 0.68  first-incr 0.70  mid 0.70  last-skinny 0.70  last-split 1.36  last-fused 0.55
(the 1.36 rows are the forced 64x64 f32 tile, which turns the ADM's un-split pair-fed layers into split, LayerNorm + GEMM ones).
No form comes nearer to the bar than a factor of 5.9: the device's steps are as close to float64 as the float32 numpy oracle is.
No wiring error was found.
"""
import contextlib
import fnmatch

import numpy as np
import pytest

import ar_step_ref as R
import megatts2_oracle as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


# ---------------------------------------------------------------------------------------------------
# option settings.  (name, options, models it applies to, witnesses).  A witness is (model, case, kind, point, form, fields): the
# form log of that setting's run of (model, case) has an entry of that layer kind, decision point and form whose fields match
# (ints exactly, strings as fnmatch patterns) - and the default run of the same (model, case) has none.  Each is derived from the
# code it names, not from a run.
BOTH = ("adm", "plm")
SETTINGS = [
    ("default", {}, BOTH + ("wide",), []),
    # ---- pipes and splits
    # choose_cfg: without x3h bits the K-split tiles stay x6ks* and the loader tile x6ldr*; gemm_takes_planes is false, so no planes
    ("x3h=0", {"x3h": 0}, BOTH, [("adm", "tiled", "mid", "residual", "stat", {"tile": "x6*"}),
                                 ("plm", "tiled", "mid", "residual", "split", {"tile": "x6*", "a_planes": 0})]),
    # ... and without x6_gemm every launch is on an f32 tile, none of which has the statistics epilogue (has_lnx): the ADM's
    # un-split residual GEMMs hand nothing on and LN -> Linear is launch_layernorm + GEMM
    ("x3h=0,x6_gemm=0", {"x3h": 0, "x6_gemm": 0}, BOTH, [("adm", "tiled", "mid", "residual", "nostat", {"tile": "dma*"}),
                                                         ("adm", "tiled", "mid", "ln_linear", "plain", {"tile": "dma*"}),
                                                         ("plm", "tiled", "mid", "residual", "split", {"tile": "dma*"})]),
    # choose_cfg: x6_ks = 0 leaves the K-split tiles on f32 (and the x3h pairing, which starts from an x6 K-split tile, never applies)
    ("x6_ks=0", {"x6_ks": 0}, BOTH, [("adm", "around-64", "mid", "residual", "nostat", {"tile": "dma*"}),
                                     ("plm", "tiled", "mid", "residual", "split", {"tile": "dma*"})]),
    # x6_ks = 1 / 5: the 32x32 k8 tile (ADM: N = 768 at M = 66 is 72 such tiles, K = 768 = 3 x 256) stays f32
    ("x6_ks=1", {"x6_ks": 1}, BOTH, [("adm", "around-64", "mid", "residual", "nostat", {"tile": "dma32x32*"})]),
    ("x6_ks=5", {"x6_ks": 5}, BOTH, [("adm", "around-64", "mid", "residual", "nostat", {"tile": "dma32x32*"})]),
    # choose_split returns 1: no slabs, no launch_ln_reduce; the PLM's last layer gets an applied x (in.S = 0): LN1 fused into both
    # consumers at M > 64
    ("splitk=0", {"splitk": 0}, BOTH, [("plm", "tiled", "mid", "residual", "nostat", {"K": 4096}),
                                       ("plm", "tiled", "last-fused", "ln_linear", "plain*", {}),
                                       ("plm", "first", "mid", "residual", "stat", {"K": 4096})]),
    # ---- the weight-streaming kernel
    # skinny_tm = 0: ln_linear's first branch and the Q | K | V launch of the last layer need the tile-major kernel; choose_split
    # leaves its <= 64-row rule for the tile rule, which splits the ADM's residual GEMMs too (12 tiles of 32x64: S1 = 2, S2 = 4)
    ("skinny_tm=0", {"skinny_tm": 0}, BOTH, [("adm", "first", "first-incr", "ln_linear", "plain", {}),
                                             ("adm", "first", "last-split", "ln_pending", "reduce", {}),
                                             ("adm", "first", "last-split", "ln_linear", "plain", {"tile": "skinny32_f32"}),
                                             ("plm", "first", "last-split", "ln_pending", "reduce", {})]),
    # skinny_pairs = 0: residual_params asks for no statistics at M <= 64, the LayerNorm prologue computes its own
    ("skinny_pairs=0", {"skinny_pairs": 0}, BOTH, [("adm", "first", "mid", "ln_linear", "skinny-ln", {}),
                                                   ("adm", "first", "mid", "residual", "nostat", {}),
                                                   ("plm", "first", "mid", "residual", "nostat", {"K": 1024})]),
    # skinny_rows = 16: M = 63 and M = 23 leave the weight-streaming kernel
    ("skinny_rows=16", {"skinny_rows": 16}, BOTH, [("adm", "around-64", "first-fill", "ln_linear", "plain", {"M": 63}),
                                                   ("plm", "around-64", "first-fill", "ln_linear", "plain", {"M": 63})]),
    # skinny_nw = 8: gemm_skinny_tm_waves gives eight waves where the default 16 gives twelve (K = 768: 12 chunks of 64) or
    # sixteen (K = 1024) at M <= 32 - the log's nw field is the count the launch used
    ("skinny_nw=8", {"skinny_nw": 8}, BOTH, [("adm", "first", "mid", "ln_linear", "skinny-ln-pairs", {"nw": 8}),
                                             ("plm", "first", "mid", "residual", "stat", {"nw": 8, "K": 1024})]),
    # ---- LayerNorm pairs (ADM)
    # ln_pairs = 0: nothing un-split, nothing handed on - the ADM takes the PLM's forms (slabs reduced by launch_ln_reduce)
    ("ln_pairs_adm=0", {"ln_pairs_adm": 0}, ("adm",), [("adm", "tiled", "mid", "residual", "split", {}),
                                                        ("adm", "tiled", "mid", "ln_pending", "reduce", {}),
                                                        ("adm", "tiled", "last-split", "ln_pending", "reduce", {})]),
    # ln_pairs = 1: statistics only where choose_split leaves a GEMM un-split anyway
    ("ln_pairs_adm=1", {"ln_pairs_adm": 1}, ("adm",), [("adm", "tiled", "mid", "residual", "split", {})]),
    ("ln_pairs_adm=2", {"ln_pairs_adm": 2}, ("adm",), []),
    # ln_pairs_maxm = 64: no launch with more than 64 rows takes part in the hand-off
    ("ln_pairs_maxm=64", {"ln_pairs_maxm": 64}, BOTH, [("adm", "tiled", "mid", "residual", "split", {})]),
    # ---- planes hand-offs (bit 0 LayerNorm -> GEMM, bit 1 ff.0 -> ff.3, bit 2 attention -> out-projection)
    ("a_planes=0", {"a_planes": 0}, BOTH, [("plm", "tiled", "mid", "ln_pending", "reduce", {"h_planes": 0}),
                                           ("plm", "tiled", "mid", "tail", "nofpl", {"M": 280})]),
    ("a_planes=1", {"a_planes": 1}, BOTH, [("plm", "tiled", "mid", "tail", "nofpl", {"M": 280})]),
    ("a_planes=2", {"a_planes": 2}, BOTH, [("plm", "tiled", "mid", "ln_pending", "reduce", {"h_planes": 0})]),
    ("a_planes=4", {"a_planes": 4}, BOTH, [("plm", "tiled", "mid", "attention", "ds", {"o_planes": 1}),
                                           ("plm", "tiled", "first-fill", "attention", "ds", {"o_planes": 1})]),
    ("a_planes=7", {"a_planes": 7}, BOTH, [("plm", "long-keys", "mid", "attention", "reg", {"o_planes": 1}),
                                           ("plm", "tiled", "mid", "residual", "split", {"a_planes": 1, "K": 1024})]),
    # ---- attention thresholds (attn_route: x6 / x3h from x6_min queries on at D = 64 / 96, then LDS from lds_min on, then ds up
    # to 128 keys, else the register kernel)
    ("attn_lds_min=32", {"attn_lds_min": 32}, BOTH, [("adm", "tiled", "mid", "attention", "lds", {}),
                                                     ("plm", "long-keys", "first-fill", "attention", "lds", {})]),
    ("attn_x6_min=32,x3h=15", {"attn_x6_min": 32, "x3h": 15}, BOTH, [("adm", "tiled", "mid", "attention", "x3h", {}),
                                                                    ("plm", "long-keys", "first-fill", "attention", "x3h", {})]),
    ("attn_x6_min=32,x3h=7", {"attn_x6_min": 32, "x3h": 7}, BOTH, [("adm", "tiled", "mid", "attention", "x6", {}),
                                                                  ("plm", "long-keys", "first-fill", "attention", "x6", {})]),
    # both off: at 192 queries (case long-q: the default attn_x6_min) the fp16-pipe kernel gives way to the register kernel
    # (192 keys: more than the short-key kernel's 128); below that nothing changes
    ("attn_lds_min=0,attn_x6_min=0", {"attn_lds_min": 0, "attn_x6_min": 0}, BOTH, [("adm", "long-q", "mid", "attention", "reg", {"qlen": 192}),
                                                                                  ("plm", "long-q", "first-fill", "attention", "reg", {"qlen": 192})]),
    # ---- tile thresholds and forcing
    # t_x3h_128 = 1: every launch with planes and N > 64 goes to the 128x128 loader tile (choose_cfg: t128 >= 1)
    ("t_x3h_128=1", {"t_x3h_128": 1}, BOTH, [("adm", "tiled", "mid", "residual", "*", {"tile": "x3hldr128x128*", "K": 768}),
                                             ("plm", "tiled", "mid", "residual", "*", {"tile": "x3hldr128x128*", "K": 1024})]),
    # t_x3h_128 = 100000: never the loader tile below t_x6_256.  PLM at M = 280: LN1 -> QKV (N = 3072: 3 x 24 = 72 tiles of 128x128,
    # the default threshold) stays on a K-split tile (240 tiles of 64x64 <= t_ks4), and so does ff.0, whose epilogue then cannot
    # store planes (gemm_writes_planes: the loader tile only)
    ("t_x3h_128=100000", {"t_x3h_128": 100000}, BOTH, [("plm", "tiled", "first-fill", "ln_linear", "plain*", {"tile": "x3hks*", "M": 280}),
                                                       ("plm", "tiled", "mid", "tail", "nofpl", {"M": 280})]),
    # a forced configuration switches off the weight-streaming kernel, the pair forms, the un-splitting and the planes: every
    # LN -> Linear is launch_layernorm (or launch_ln_reduce) + GEMM
    ("force_gemm_config=12", {"force_gemm_config": 12}, BOTH,
     [("adm", "first", "first-incr", "ln_linear", "plain", {"tile": "dma64x64_2x2_s3"}),
      ("adm", "tiled", "first-fill", "ln_linear", "plain", {"tile": "dma64x64_2x2_s3"}),
      ("adm", "tiled", "mid", "residual", "split", {"tile": "dma64x64_2x2_s3"}),
      ("plm", "first", "last-split", "ln_pending", "reduce", {})]),
    # ---- stream groups: M is per group
    ("groups=2", {"adm_groups": 2, "plm_groups": 2}, BOTH, [("adm", "tiled", "mid", "ln_linear", "pair-fed", {"M": 140}),
                                                            ("plm", "tiled", "mid", "tail", "*", {"M": 140})]),
    ("groups=3", {"adm_groups": 3, "plm_groups": 3}, BOTH, [("adm", "tiled", "mid", "ln_linear", "pair-fed", {"M": 70}),
                                                            ("plm", "tiled", "mid", "tail", "*", {"M": 70})]),
]
SETTING = {s[0]: s for s in SETTINGS}
PLANES = ("a_planes=0", "a_planes=1", "a_planes=2", "a_planes=4", "a_planes=7")
PARAMS = [pytest.param(m, c, s[0], id=f"{m}-{c}-{s[0]}") for s in SETTINGS for m in s[2] for c in R.MODEL_CASES[m]]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def nat():
    """This file's own handles, by model: one for the ADM + PLM at production size, one for the small wide-head PLM.  No option
    set here can leak into another file."""
    from megatts2_amd.runtime import NativeModel
    (g, p, a, h), (_, sd_p, sd_a, _) = R.synth_models("prod")
    prod = NativeModel(g, p, a, h, sd_plm=sd_p, sd_adm=sd_a)
    wide = NativeModel(g, R.model_of("wide")[0], a, h, sd_plm=R.model_of("wide")[1])
    for n in (prod, wide):
        n.set_option("adm_groups", 1)          # M is per stream group: the default ar_groups = 2 would halve it
        n.set_option("plm_groups", 1)
    yield {"adm": prod, "plm": prod, "wide": wide}
    prod.close()
    wide.close()


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


_RUNS = {}


def run(handles, model, case, setting):
    """One call of (model, case) under a setting, once per module: {"out": device tensors, "log": the form log}."""
    key = (model, case, setting)
    if key in _RUNS:
        return _RUNS[key]
    nat = handles[model]
    lens, P, steps = R.CASES[case]
    cond, hist = R.inputs(model, case)
    ln = np.asarray(lens, np.int32)
    fallbacks = nat.range_fallbacks
    with options(nat, SETTING[setting][1]):
        nat.form_log_begin()
        try:
            if R.is_adm(model):
                out = nat.adm_infer(dev(cond), ln, return_float=True, p_prefix=dev(hist) if P else None, max_steps=steps)
            else:
                out = nat.plm_infer(dev(cond), ln - P, return_logits=True, prefix_codes=dev(hist) if P else None, max_steps=steps)
            torch.cuda.synchronize()
        finally:
            log = nat.form_log_end()
    assert nat.range_fallbacks == fallbacks, "the fp16 range guard tripped: the call ran twice"
    _RUNS[key] = {"out": out, "log": log}
    return _RUNS[key]


def matches(entry, kind, point, form, fields):
    k, p, f, attrs = entry
    if k != kind or p != point or not fnmatch.fnmatchcase(f, form):
        return False
    for name, want in fields.items():
        got = attrs.get(name)
        if isinstance(want, str):
            if got is None or not fnmatch.fnmatchcase(str(got), want):
                return False
        elif got != want:
            return False
    return True


def judge(handles, model, case, setting):
    """run() + every figure of the call, once per module: r["ratios"] - error / E32 per (slot, step); r["problems"] - what the
    assertions of test_step_forms would say (empty: parity within the bar, discrete outputs right).  Prints each figure."""
    r = run(handles, model, case, setting)
    if "ratios" in r:
        return r
    lens, P, _ = R.CASES[case]
    e32, bar = R.e32(model), R.bar(model)
    ratios, problems = [], []
    if R.is_adm(model):
        _, hist = R.inputs("adm", case)
        dur, flt = (t.cpu().numpy() for t in r["out"])
    else:
        codes, logits = (t.cpu().numpy() for t in r["out"])
        ref = R.plm_reference(model, case)
    for b, n in enumerate(lens):
        steps = R.steps_of(case, b)
        if R.is_adm(model):
            if not np.array_equal(flt[b, :P], hist[b]):
                problems.append(f"slot {b}: the forced history changed")
            if flt[b, n:].any() or dur[b, n:].any():
                problems.append(f"slot {b}: positions beyond the length are not zero")
        elif codes[b, n - P:].any() or logits[b, steps:].any():
            problems.append(f"slot {b}: positions beyond the length / the steps run are not zero")
        for k in range(steps):
            if R.is_adm(model):
                p64 = R.adm_step64(case, b, flt[b, :P + k])            # on the history the device used
                err = R.adm_err(flt[b, P + k], p64)
                print(f"adm {case} [{setting}] slot {b} n {P + k + 1}: p {flt[b, P + k]:+.8f} p64 {p64:+.10f} err {err:.3e} ratio {err / e32:.2f}")
                if dur[b, P + k] != min(max(int(np.float32(flt[b, P + k]) + np.float32(0.5)), 1), 128):
                    problems.append(f"slot {b} step {k}: the duration is not the rounded float")
            else:
                err = O.rel_l2(logits[b, k], ref[b]["logits64"][k])
                print(f"{model} {case} [{setting}] slot {b} n {P + k + 1}: rel-L2 {err:.3e} ratio {err / e32:.2f}")
                if codes[b, k] != ref[b]["codes64"][k]:
                    problems.append(f"slot {b} step {k}: the device's code is not the float64 arg-max")
            ratios.append(err / e32)
            if not err <= bar:
                problems.append(f"slot {b} step {k}: error / E32 = {err / e32:.2f} is above the bar of 8")
    r["ratios"], r["problems"] = ratios, problems
    return r


def form_keys(log):
    """The (decision point, form) pairs and the layer kinds of a log, as the per-form table names them."""
    return {key for kind, point, form, attrs in log
            for key in (("layer", kind), (point, form + ("+o_planes" if attrs.get("o_planes") else "")))}


@pytest.mark.parametrize("model,case,setting", PARAMS)
def test_step_forms(nat, model, case, setting):
    r = judge(nat, model, case, setting)
    assert not r["problems"], r["problems"]
    assert r["log"], "the form log is empty"
    base = run(nat, model, case, "default")["log"]
    for wm, wc, kind, point, form, fields in SETTING[setting][3]:
        if (wm, wc) != (model, case):
            continue
        assert any(matches(e, kind, point, form, fields) for e in r["log"]), \
            (f"{setting} did not reach {kind} {point} {form} {fields}", sorted({(e[0], e[1], e[2], e[3].get('tile', '')) for e in r["log"]}))
        assert not any(matches(e, kind, point, form, fields) for e in base), f"the default run already shows {kind} {point} {form} {fields}"


@pytest.mark.parametrize("model", BOTH)
def test_form_log_only_observes(nat, model):
    """With the log on and with it off the `tiled` case launches the same GEMMs (configuration, M, N, K, groups, count: the
    launch trace) and leaves the same bits."""
    h = nat[model]
    lens, P, steps = R.CASES["tiled"]
    cond, hist = R.inputs(model, "tiled")
    ln = np.asarray(lens, np.int32)
    got = []
    for log in (False, True):
        h.gemm_trace_begin()
        if log:
            h.form_log_begin()
        try:
            if R.is_adm(model):
                out = h.adm_infer(dev(cond), ln, return_float=True, p_prefix=dev(hist), max_steps=steps)
            else:
                out = h.plm_infer(dev(cond), ln - P, return_logits=True, prefix_codes=dev(hist), max_steps=steps)
            torch.cuda.synchronize()
            shapes = sorted((s["config"], s["M"], s["N"], s["K"], s["groups"], s["launches"]) for s in h.gemm_trace_shapes(top=1000))
        finally:
            h.gemm_trace_end()
            entries = h.form_log_end() if log else []
        assert bool(entries) == log and len(shapes) > 3
        got.append((shapes, out))
    assert got[0][0] == got[1][0]
    assert all(torch.equal(a, b) for a, b in zip(got[0][1], got[1][1]))
    h.form_log_begin()
    assert h.form_log_end() == []          # nothing is recorded outside the AR steps, and end() drops what it returned


def test_witnesses_name_cases_that_exist():
    for name, _, models, wit in SETTINGS:
        for wm, wc, kind, *_ in wit:
            assert wm in models and wc in R.MODEL_CASES[wm] and kind in KINDS, (name, wm, wc, kind)


@pytest.mark.parametrize("model", BOTH)
@pytest.mark.parametrize("case", list(R.CASES))      # (both production models run every case)
def test_planes_hand_offs_are_bit_identical(nat, model, case):
    """model_stages.hip and mt2_kernels.h say "same values, bit-identical results" of every planes hand-off (LayerNorm -> GEMM,
    ff.0 -> ff.3, attention -> out-projection): the five a_planes settings leave the same bits."""
    outs = [run(nat, model, case, s)["out"] for s in PLANES]
    for s, o in zip(PLANES[1:], outs[1:]):
        for a, b in zip(outs[0], o):
            assert torch.equal(a, b), f"{model} {case}: {s} differs from {PLANES[0]}"


# ---------------------------------------------------------------------------------------------------
# coverage: what the log can emit at these shapes, per layer kind (from the call sites of model_stages.hip)
KINDS = ("first-fill", "first-incr", "mid", "last-skinny", "last-split", "last-fused")
RESIDUAL = ("split", "stat", "nostat")
ATTN_PROD = ("reg", "ds", "lds", "x6", "x3h")       # at the production head widths (D = 96 / 64); "generic": the wide model below
EXPECTED = set()
# first layer: ln_linear has no statistics to take (st = nullptr) - no pair forms; the incremental form has A <= 4 rows here, and
# planes need more than 64 (gemm_takes_planes).  Attention on the cache: every kernel; then the common tail
for kind in ("first-fill", "first-incr"):
    EXPECTED |= {(kind, "ln_linear", f) for f in (("skinny-ln", "plain", "plain+planes") if kind == "first-fill" else ("skinny-ln", "plain"))}
# the tail (first and middle layers): LN2 -> ff.0 through ln_linear (S1 = 1) or ln_pending (S1 > 1), both residual GEMMs, fpl;
# the incremental first layer runs with M = A n rows like the others
for kind in ("first-fill", "first-incr", "mid"):
    EXPECTED |= {(kind, "residual", f) for f in RESIDUAL} | {(kind, "tail", f) for f in ("fpl", "nofpl")}
    EXPECTED |= {(kind, "ln_pending", "reduce")}
    EXPECTED |= {(kind, "attention", f) for f in ATTN_PROD}
    EXPECTED |= {(kind, "attention+planes", f) for f in ("reg", "ds")}      # (a_planes bit 2 at <= 128 / more keys)
    EXPECTED |= {(kind, "ln_linear", f) for f in ("skinny-ln-pairs", "pair-fed", "plain", "plain+planes")}
# ... and the fp16-pipe kernel storing planes: a_planes bit 2 on case long-q, whose one step fills the cache (no incremental form)
EXPECTED |= {(kind, "attention+planes", "x3h") for kind in ("first-fill", "mid")}
EXPECTED |= {("mid", "ln_linear", "skinny-ln")}      # LN1 -> QKV of a middle layer whose producer handed nothing on (skinny_pairs = 0)
# last layer: K | V and Q.  skinny: one launch (or ln_pending + GEMM behind slabs); split: ln_pending (reduce) + two GEMMs; fused: two
# ln_linear.  Then one query per sequence (never more than 31 queries: ds / reg only), the residual GEMM of A <= 4 rows
# (weight-streaming kernel: stat / nostat) and LN2 -> ff.0 of A rows
EXPECTED |= {("last-skinny", "ln_linear", f) for f in ("skinny-ln", "skinny-ln-pairs")} | {("last-skinny", "ln_pending", "reduce")}
EXPECTED |= {("last-split", "ln_pending", "reduce")}
EXPECTED |= {("last-fused", "ln_linear", f) for f in ("skinny-ln", "pair-fed", "plain", "plain+planes")}
for kind in ("last-skinny", "last-split", "last-fused"):
    EXPECTED |= {(kind, "attention", f) for f in ("ds", "reg")} | {(kind, "residual", f) for f in ("stat", "nostat")}
    EXPECTED |= {(kind, "ln_linear", f) for f in ("skinny-ln", "skinny-ln-pairs", "plain")}
# ... but the skinny form of the last layer exists only while the weight-streaming kernel takes M = A n <= 64 rows: its LN -> Linear
# pairs never fall back to launch_layernorm + GEMM, and its sequences never have more than 64 keys (the register kernel starts at 129)
EXPECTED -= {("last-skinny", "ln_linear", "plain"), ("last-skinny", "attention", "reg")}
# the generic kernel (heads wider than 128: the wide model, default options): cases "first" (M = 1, 2, 3) and "around-64" (M = 63: the
# weight-streaming forms; M = 66: ff.3 with K = 2048 is split eight ways - 24 tiles of 32x64 - so the last layer reduces slabs)
EXPECTED |= {(kind, "attention", "generic") for kind in ("first-fill", "first-incr", "mid", "last-skinny", "last-split")}


def test_every_form_is_reached(nat):
    """The (layer kind, decision point, form) triples seen over every (model, case, setting) of this file are exactly EXPECTED, and
    the split counts, statistics layouts and hand-offs the issue of this test names all occur."""
    seen, S, stat_w, worst, form_worst = set(), set(), set(), {}, {}
    for name, _, models, _ in SETTINGS:
        for model in models:
            for case in R.MODEL_CASES[model]:
                r = judge(nat, model, case, name)
                w = max(r["ratios"])
                worst[(model, name)] = max(worst.get((model, name), 0.0), w)
                # a call's worst step is booked on the forms that the default run of the same case does not show (a default
                # run: on all of its forms) - the forms the setting is there for, not every form that merely took part
                new = form_keys(r["log"]) - (form_keys(run(nat, model, case, "default")["log"]) if name != "default" else set())
                for key in new:
                    form_worst[key] = max(form_worst.get(key, 0.0), w)
                for kind, point, form, attrs in r["log"]:
                    if point == "attention" and attrs.get("o_planes"):
                        point = "attention+planes"
                    seen.add((kind, point, form))
                    if point == "residual":
                        S.add(attrs["S"])
                        stat_w.add(attrs["stat_w"])
    print("worst error / E32 per setting (adm, plm, wide); E32 = " + ", ".join("%.3e" % R.e32(m) for m in R.MODELS))
    for name, *_ in SETTINGS:
        print("    %-30s %s" % (name, "  ".join("%5.2f" % worst[(m, name)] if (m, name) in worst else "    -" for m in R.MODELS)))
    print("worst error / E32 per form: over the default runs, and over the calls of settings that bring the form to a case")
    for (point, form), w in sorted(form_worst.items()):
        print("    %-12s %-22s %5.2f" % (point, form, w))
    assert {k for k, _, _ in seen} == set(KINDS)
    assert not EXPECTED - seen, f"never reached: {sorted(EXPECTED - seen)}"
    assert not seen - EXPECTED, f"reached but not expected: {sorted(seen - EXPECTED)}"
    assert 1 in S and any(s > 1 for s in S) and {0, 16} < stat_w, (S, stat_w)       # un-split and split; no / 16-column / tile-wide pairs
