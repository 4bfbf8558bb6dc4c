"""float64 reference of ONE autoregressive step of the ADM and of the PLM on a forced history (host only, no GPU).

The rule is the oracle's (oracle/megatts2_oracle.py: adm_infer / plm_infer with p_prefix / prefix_codes and steps, which restate
MegaADM.infer / MegaPLM.infer): the oracle's source is loaded a second time under another module name with its F32 set to
numpy.float64, so every product, sum, LayerNorm and soft-max of the step runs in float64.  Its inputs are exactly what the device
holds, each rounded to float32 ONCE: the weights, the conditioning rows, the forced history and the positional table (the float32
table runtime.sine_table uploads - alpha folded in - not a float64 sine).

The cases are the smallest shapes at which every form of the AR step wiring (csrc/model_stages.hip, ar_step_layers) can be reached
at production size - tests/test_gpu_ar_step_forms.py runs them on the device, tests/test_ar_step_ref_host.py pins this reference to
the float32 oracle and checks the arg-max margins.  Everything here is computed once per process and shared.
"""
import functools
import importlib.util
import os
import sys
import zlib

import numpy as np

import megatts2_oracle as O
from conftest import ROOT, synth_models


def _load_f64():
    spec = importlib.util.spec_from_file_location("megatts2_oracle_f64", os.path.join(ROOT, "oracle", "megatts2_oracle.py"))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[spec.name] = mod
    spec.loader.exec_module(mod)
    mod.F32 = np.float64

    def add_pe(x, alpha):      # the device adds its float32 table alpha * pe (runtime.sine_table) to the step's input rows
        from megatts2_amd.runtime import sine_table
        T, d = x.shape
        return x.astype(np.float64) + sine_table(T, d, float(np.asarray(alpha).reshape(-1)[0])).astype(np.float64)

    mod.add_pe = add_pe
    return mod


O64 = _load_f64()

# name -> (lengths per slot, forced positions P, steps).  NOT in sorted order: the length order of ar_order is a real permutation.
#   first      n = 1, 2, 3; no fill_all; the layer-0 cache grows from empty
#   around-64  M = 3 x 21 = 63 (weight-streaming kernel) -> 3 x 22 = 66 (tiles; pairs in the ADM) -> 1 x 23 (A shrunk to 1);
#              fill_all, then the incremental cache
#   tiled      M = 4 x 70 = 280 -> 2 x 71 = 142 (A shrinks by two); at most 128 keys
#   long-keys  M = 2 x 130 = 260; more than 128 keys
#   long-incr  M = 130 -> 131: the only way to more than 128 keys in the INCREMENTAL form of the first layer (a step after the
#              first of its call) - no option reaches that at the four shapes above
#   long-q     M = n = 192 queries per sequence: the default attn_x6_min, from which on the bf16 / fp16-pipe attention kernels run by
#              default - the smallest shape at which switching them off changes anything
CASES = {
    "first": ((3,), 0, 3),
    "around-64": ((22, 23, 22), 20, 3),
    "tiled": ((70, 71, 71, 70), 69, 2),
    "long-keys": ((130, 130), 129, 1),
    "long-incr": ((131,), 129, 2),
    "long-q": ((192,), 191, 1),
}
# "wide": a small PLM with heads of 256 columns (3 layers: first, middle, last).  The production heads are 96 (ADM) and 64 (PLM)
# wide, and the generic attention kernel serves heads wider than 128 only: no option and no shape reaches it with them
MODELS = ("adm", "plm", "wide")
MODEL_CASES = {"adm": tuple(CASES), "plm": tuple(CASES), "wide": ("first", "around-64")}
SEEDS = {"adm": 11, "plm": 23, "wide": 37}


def is_adm(model):
    return model == "adm"


@functools.lru_cache(maxsize=None)
def model_of(model):
    """(config, state dict) of the synthetic-weight model: production size, or the small wide-head PLM."""
    if model == "wide":
        from megatts2_amd import config as C
        from megatts2_amd import weights
        cfg = C.PLMConfig(n_layers=3, n_heads=2, vq_dim=256, tc_latent_dim=256, vq_bins=1024)
        return cfg, weights.synth_state_dict(weights.inventory_plm(cfg), 0, "plm.")
    (_, p, a, _), (_, sd_p, sd_a, _) = synth_models("prod")
    return (a, sd_a) if model == "adm" else (p, sd_p)


def steps_of(case, b):
    lens, P, steps = CASES[case]
    return min(steps, lens[b] - P)


@functools.lru_cache(maxsize=None)
def inputs(model, case):
    """cond f32 [B, Lmax, tc] post-ReLU standard normal (a different sequence in every slot; rows beyond a length are never read),
    hist: the forced history [B, P] - uniform [1, 7) floats (ADM) or random codes (PLM)."""
    lens, P, _ = CASES[case]
    cfg, _ = model_of(model)
    rng = np.random.Generator(np.random.PCG64([SEEDS[model], zlib.crc32(case.encode())]))       # (adding a case moves no other's inputs)
    cond = np.maximum(rng.standard_normal((len(lens), max(lens), cfg.tc_latent_dim)), 0).astype(np.float32)
    if is_adm(model):
        hist = rng.uniform(1.0, 7.0, (len(lens), P)).astype(np.float32)
    else:
        hist = rng.integers(0, cfg.vq_bins, (len(lens), P)).astype(np.int64)
    return cond, hist


def adm_step(oracle, case, b, hist):
    """The prediction of position len(hist) of slot b given the float32 history `hist` (forced positions first)."""
    cfg, sd = model_of("adm")
    cond, _ = inputs("adm", case)
    hist = np.asarray(hist, np.float32)
    _, flt = oracle.adm_infer(sd, cfg, cond[b, :CASES[case][0][b]], return_float=True, p_prefix=hist if hist.size else None, steps=1)
    return float(flt[hist.size])


_ADM64 = {}


def adm_step64(case, b, hist):
    """adm_step in float64, remembered per history (option settings that leave the same bits share one evaluation)."""
    key = (case, b, np.asarray(hist, np.float32).tobytes())
    if key not in _ADM64:
        _ADM64[key] = adm_step(O64, case, b, hist)
    return _ADM64[key]


@functools.lru_cache(maxsize=None)
def adm_reference(case):
    """Per slot: p64 - the float64 prediction of every step, each on the forced history followed by the EARLIER float64
    predictions rounded to float32; p32 - the float32 oracle's prediction on the same history."""
    _, hist0 = inputs("adm", case)
    out = []
    for b in range(len(CASES[case][0])):
        hist, p64, p32 = hist0[b].copy(), [], []
        for _ in range(steps_of(case, b)):
            p64.append(adm_step64(case, b, hist))
            p32.append(adm_step(O, case, b, hist))
            hist = np.append(hist, np.float32(p64[-1]))
        out.append({"p64": np.asarray(p64), "p32": np.asarray(p32)})
    return out


@functools.lru_cache(maxsize=None)
def plm_reference(model, case):
    """Per slot: logits64 [steps, bins] and codes64 of the greedy float64 run from the forced history (every later step on the
    float64 arg-max of the earlier ones), logits32 / codes32 of the float32 oracle's own run.  model: "plm" or "wide"."""
    cfg, sd = model_of(model)
    cond, hist = inputs(model, case)
    lens, P, _ = CASES[case]
    out = []
    for b in range(len(lens)):
        kw = dict(return_logits=True, prefix_codes=hist[b] if P else None, steps=steps_of(case, b))
        c64, l64 = O64.plm_infer(sd, cfg, cond[b, :lens[b]], **kw)
        c32, l32 = O.plm_infer(sd, cfg, cond[b, :lens[b]], **kw)
        out.append({"logits64": l64, "codes64": c64, "logits32": l32, "codes32": c32})
    return out


def adm_err(p, p64):
    return abs(float(p) - float(p64)) / max(1.0, abs(float(p64)))


@functools.lru_cache(maxsize=None)
def e32(model):
    """E32(model): the largest error of the float32 oracle against the float64 step over all cases of the model - relative L2 of a step's
    logits (PLM), |p - p64| / max(1, |p64|) (ADM)."""
    worst = 0.0
    for case in MODEL_CASES[model]:
        if is_adm(model):
            for r in adm_reference(case):
                worst = max([worst] + [adm_err(a, b) for a, b in zip(r["p32"], r["p64"])])
        else:
            for r in plm_reference(model, case):
                worst = max([worst] + [O.rel_l2(a, b) for a, b in zip(r["logits32"], r["logits64"])])
    return worst


def bar(model):
    """The parity bar of a device step: 8 x E32(model)."""
    return 8.0 * e32(model)


def top2_gap(logits):
    """(largest - second largest) / max |logit| of one step's logits."""
    s = np.sort(np.asarray(logits, np.float64))
    return float((s[-1] - s[-2]) / np.abs(s).max())
