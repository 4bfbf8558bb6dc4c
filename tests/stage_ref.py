"""float64 forward of the parallel (non-AR) stages and the cases of their wiring tests (host only, no GPU).

The stages are the ones in front of and behind the AR steps: the MRTE mel encoder (mel_context), the phone encoder with the cross
attention (tc_latent), the VQ prosody encoder (ze, codes) and the mel decoder.  The rule is the oracle's
(oracle/megatts2_oracle.py: mrte_mel_context, mrte_tc_latent, vqpe_encode / vqpe_forward, mel_decoder): ar_step_ref.O64 is the
oracle's source loaded a second time with F32 = numpy.float64 and the float32 positional table runtime.sine_table, so every product,
sum, LayerNorm and soft-max runs in float64 - on exactly what the device holds, each rounded to float32 ONCE: the synthetic weights,
phone ids, prompt mel, target mel, decoder input.  One utterance at a time: the reference has no batch.

Two generators: `prod` (conftest.synth_models("prod")) and `k7`, a small G on the same synthetic-weight generator whose kernels are
7 wide (halo 3: wider than the gap of 2 rows that every tested configuration could live with), whose heads are 64 (phone encoder)
and 128 (cross attention) wide - ragged launches from real wiring on attention kernels other than the generic one - and whose
decoder stack is a square 128-channel convolution with one group (the window tiles).

The judge, per stage output (mel_context, tc_latent, ze, mel), per utterance and per row r:
    e[r] = ||y[r] - y64[r]|| / max_r' ||y64[r']||
per row because a row read across an utterance's edge damages a few edge rows, which a whole-utterance L2 dilutes.  E32[generator][stage]
is the float32 oracle's worst e[r] over all cases (ATen's float32 kernels on one thread; measured against this reference and never
against the device; tests/test_stage_ref_host.py recomputes it); the bar of a device row is 8 x E32.  Everything here is computed once per
process and shared; the arrays handed out are read-only.
"""
import functools
import zlib

import numpy as np

import megatts2_oracle as O
from ar_step_ref import O64
from conftest import synth_models

STAGES = ("mel_context", "tc_latent", "ze", "mel")

# E32 as test_stage_ref_host.py recomputes it (test_pinned_e32: recomputed <= E32 <= 1.5 x recomputed), pinned so that the GPU test
# spends no CPU time on the float32 oracle.  Recomputed on ONE thread (ATen's float32 sums follow the thread count):
#   prod  mel_context 5.33e-7  tc_latent 6.64e-6  ze 4.22e-7  mel 4.98e-7
#   k7    mel_context 5.86e-7  tc_latent 4.76e-6  ze 4.37e-7  mel 5.95e-7
# (tc_latent: the soft-max of the cross attention - ONE head as wide as the model - amplifies the float32 error of its scores)
E32 = {"prod": {"mel_context": 6.4e-7, "tc_latent": 8.0e-6, "ze": 5.1e-7, "mel": 6.0e-7},
       "k7": {"mel_context": 7.0e-7, "tc_latent": 5.7e-6, "ze": 5.2e-7, "mel": 7.1e-7}}


def e32(gen, stage):
    return E32[gen][stage]


def bar(gen, stage):
    """The parity bar of a device row: 8 x E32."""
    return 8.0 * E32[gen][stage]


# ---------------------------------------------------------------------------------------------------
# generators and cases

GENERATORS = ("prod", "k7")

# name -> (phones, prompt frames, target-mel frames) per slot, NOT in sorted order; every slot holds a different utterance.
#   one     every linear of the phone branch has at most 64 rows; the minimum prompt used (two context rows at stride 16); one VQ row
#   pair    two utterances: the smallest batch with a neighbour
#   ragged  a 1-phone utterance, the minimum prompt, lengths at 32 / 64 / 128 edges, a partial last pool window (9, 130, 1 frames)
#   rows    200 + 17 + 180 prompt rows and four gaps of 8: 429 rows = 4 row tiles x 4 column tiles x 5 groups = 80 tiles of 128x128 in the
#           mel stacks, over the default t_x3h_128 = 72: the stack runs on the x3h loader tile with the planes hand-off by default
#   <case>-k  utterance k of `pair` / `ragged` as a batch of one (the same inputs: the same reference)
CASES = {
    "one": ((1,), (17,), (1,)),
    "pair": ((5, 9), (17, 30), (9, 17)),
    "ragged": ((33, 1, 64, 7), (40, 17, 130, 64), (9, 1, 130, 40)),
    "rows": ((70, 1, 64), (200, 17, 180), (300, 8, 17)),
}
ALONE = {c: tuple(f"{c}-{k}" for k in range(len(CASES[c][0]))) for c in ("pair", "ragged")}
for _c, _names in ALONE.items():
    for _k, _n in enumerate(_names):
        CASES[_n] = tuple((v[_k],) for v in CASES[_c])
BATCH_CASES = {"prod": ("one", "ragged", "rows"), "k7": ("one", "pair", "ragged")}
GEN_CASES = {"prod": BATCH_CASES["prod"] + ALONE["ragged"], "k7": BATCH_CASES["k7"] + ALONE["pair"] + ALONE["ragged"]}
SEED = 54


@functools.lru_cache(maxsize=None)
def generator(name):
    """(GConfig, f32 state dict) of a generator: synthetic weights as everywhere in the suite."""
    if name == "prod":
        cfgs, sds = synth_models("prod")
        return cfgs[0], sds[0]
    assert name == "k7"
    from megatts2_amd import config as C
    from megatts2_amd import weights
    cfg = C.GConfig(
        mrte=C.MRTEConfig(mel_kernel_size=7, mel_stride=4, mel_n_layer=2, mel_n_stack=2, mel_n_block=2, hidden_size=128,
                          content_n_heads=2, content_n_layers=2, content_ff_dim=256),
        vqpe=C.VQPEConfig(hidden_size=128, kernel_size=7, n_layers=2, n_stacks=2, n_blocks=2, mel_bins=20, vq_dim=32),
        kernel_size=7, hidden_size=128, decoder_n_stack=2, decoder_n_block=2)
    return cfg, weights.synth_state_dict(weights.inventory_g(cfg), 0, "G.")


@functools.lru_cache(maxsize=None)
def _sd64(gen):
    return {k: np.asarray(v, np.float32).astype(np.float64) for k, v in generator(gen)[1].items()}


def codebook(gen):
    return generator(gen)[1][O.CODEBOOK]


@functools.lru_cache(maxsize=None)
def inputs(gen, case):
    """Per slot a dict of what the device is handed, all float32 / int64: phone [Np], prompt [Tp, 80], target [T, 80] (the VQ
    prosody encoder's mel), xdec [T, hidden + vq_dim] (the decoder's input: post-ReLU standard normal rows followed by codebook rows
    repeated x stride, as models/megatts2.py:361-366 builds it)."""
    for base, names in ALONE.items():
        if case in names:
            return (inputs(gen, base)[names.index(case)],)
    from megatts2_amd import synth
    cfg, sd = generator(gen)
    phones, prompts, frames = CASES[case]
    rng = np.random.Generator(np.random.PCG64([SEED, zlib.crc32(gen.encode()), zlib.crc32(case.encode())]))      # (a new case moves no other's inputs)
    out = []
    for n, tp, t in zip(phones, prompts, frames):
        u = synth.make_utterance(rng, n, tp, max(t, n), cfg.mrte.phone_vocab_size)
        target = synth.make_utterance(rng, 1, t, t).prompt_mel
        tc = np.maximum(rng.standard_normal((t, cfg.mrte.hidden_size)), 0).astype(np.float32)
        codes = rng.integers(0, cfg.vqpe.vq_bins, -(-t // cfg.vqpe.stride))
        slot = {"phone": u.phone, "prompt": u.prompt_mel, "target": target, "xdec": O.decoder_input(sd, cfg, tc, codes)}
        for a in slot.values():
            a.setflags(write=False)
        out.append(slot)
    return tuple(out)


# ---------------------------------------------------------------------------------------------------
# the forward of one utterance -> {"mel_context", "tc_latent", "ze", "codes", "mel"}

def forward(oracle, sd, cfg, slot):
    """All four stages of one utterance with the primitives of `oracle` (O: float32, O64: float64).  tc_latent restates
    oracle.mrte_tc_latent on the mel context already computed."""
    ctx = oracle.mrte_mel_context(sd, cfg, slot["prompt"])
    px = oracle.mrte_phone_encoder(sd, cfg, slot["phone"])
    y = oracle.mha(sd, "mrte.mha", px, ctx, 1)
    tc = oracle.relu(oracle.layer_norm(y, sd["mrte.norm.weight"], sd["mrte.norm.bias"]))
    ze = oracle.vqpe_encode(sd, cfg, slot["target"])
    return {"mel_context": ctx, "tc_latent": tc, "ze": ze, "codes": oracle.vq_quantize(sd[O.CODEBOOK], ze),
            "mel": oracle.mel_decoder(sd, cfg, slot["xdec"])}


_TAPS = {}


def _conv1d64(x, w, b, stride=1, padding=0, dilation=1):
    """O64.conv1d with one CONTIGUOUS [Cin, Cout] float64 matrix per tap, made once per weight: the same products summed over the
    taps in the same order - numpy's matmul leaves BLAS for the strided w[:, :, tap].T of the oracle's (20 x slower at 512 channels)."""
    key = (w.ctypes.data, w.shape, w.dtype.str)
    if key not in _TAPS:
        _TAPS[key] = (w, np.ascontiguousarray(np.asarray(w, np.float64).transpose(2, 1, 0)))      # (w kept: its address stays its own)
    wt = _TAPS[key][1]
    T, cin = x.shape
    cout, cin_w, k = w.shape
    assert cin == cin_w
    t_out = (T + 2 * padding - dilation * (k - 1) - 1) // stride + 1
    if t_out <= 0:
        return np.zeros((0, cout), np.float64)
    xp = np.zeros((T + 2 * padding, cin), np.float64)
    xp[padding:padding + T] = x
    y = np.zeros((t_out, cout), np.float64)
    for tap in range(k):
        y += np.ascontiguousarray(xp[tap * dilation: tap * dilation + (t_out - 1) * stride + 1: stride]) @ wt[tap]
    return y if b is None else y + b


O64.conv1d = _conv1d64          # (the AR steps of ar_step_ref have no convolution)

_R64, _R32 = {}, {}


def _key(gen, slot):
    return (gen,) + tuple(slot[k].tobytes() for k in ("phone", "prompt", "target", "xdec"))


def reference(gen, case):
    """Per slot: the float64 outputs (read-only; the <case>-k cases share their utterance's of the batch case)."""
    out = []
    for slot in inputs(gen, case):
        key = _key(gen, slot)
        if key not in _R64:
            _R64[key] = forward(O64, _sd64(gen), generator(gen)[0], slot)
            for a in _R64[key].values():
                assert a.dtype in (np.float64, np.int64)
                a.setflags(write=False)
        out.append(_R64[key])
    return out


def restatement32(gen, case):
    """Per slot: the float32 oracle's outputs on ATen's float32 kernels, on one thread: the summation order, and with it E32,
    follows the thread count."""
    import torch
    cfg, sd = generator(gen)
    out = []
    for slot in inputs(gen, case):
        key = _key(gen, slot)
        if key not in _R32:
            swapped = bool(O._NUMPY_PRIMS) and O.linear is not O._NUMPY_PRIMS["linear"]
            threads = torch.get_num_threads()
            O.enable_torch_kernels()
            try:
                torch.set_num_threads(1)
                _R32[key] = forward(O, sd, cfg, {k: v.copy() for k, v in slot.items()})      # (torch.from_numpy wants writable arrays)
            finally:
                torch.set_num_threads(threads)
                if not swapped:
                    O.disable_torch_kernels()
        out.append(_R32[key])
    return out


def row_err(y, y64):
    """e[r] = ||y[r] - y64[r]|| / max_r' ||y64[r']|| over the rows of one utterance's stage output [rows, C]."""
    y, y64 = np.asarray(y, np.float64), np.asarray(y64, np.float64)
    assert y.shape == y64.shape and y.ndim == 2, (y.shape, y64.shape)
    return np.sqrt(((y - y64) ** 2).sum(axis=1)) / np.sqrt((y64 ** 2).sum(axis=1)).max()


@functools.lru_cache(maxsize=None)
def e32_measured(gen):
    """{stage: the float32 restatement's largest row error over the batch cases of the generator}."""
    worst = dict.fromkeys(STAGES, 0.0)
    for case in BATCH_CASES[gen]:
        for a, b in zip(restatement32(gen, case), reference(gen, case)):
            for s in STAGES:
                worst[s] = max(worst[s], float(row_err(a[s], b[s]).max()))
    return worst


def vq_margin(gen, ze64, eps):
    """Per row of ze64: min over the codes j other than the float64 arg-min a of (score_a - score_j) / (2 eps ||e_a - e_j||).  An
    error d in a row of ze moves the difference of two scores by 2 d.(e_a - e_j), at most 2 ||d|| ||e_a - e_j||: a margin above 1 means
    that no error of norm eps can change the decision."""
    e = codebook(gen).astype(np.float64)
    d = O.vq_distances(codebook(gen), ze64)
    best = d.argmax(axis=1)
    r = np.arange(d.shape[0])
    dist = np.sqrt(((e[best][:, None, :] - e[None, :, :]) ** 2).sum(axis=2))
    with np.errstate(divide="ignore", invalid="ignore"):
        m = (d[r, best][:, None] - d) / (2.0 * eps * dist)
    m[r, best] = np.inf
    return m.min(axis=1)


# ---------------------------------------------------------------------------------------------------
# the mutant of the host test: the decoder / the mel encoder of a batch in ONE buffer, `gap` zero rows between the utterances, the
# convolutions run across the buffer and every row outside an utterance set to zero behind each launch - the device's row layout

def _buffer(xs, gap):
    R = gap + sum(x.shape[0] + gap for x in xs)
    buf, valid, off = np.zeros((R, xs[0].shape[1])), np.zeros((R, 1)), []
    r = gap
    for x in xs:
        off.append(r)
        buf[r:r + x.shape[0]] = x
        valid[r:r + x.shape[0]] = 1.0
        r += x.shape[0] + gap
    return buf, valid, off


def _stack_rows(sd, p, x, valid, k, n_stacks, n_blocks):
    for s in range(n_stacks):
        y = x
        for b in range(n_blocks):
            q = f"{p}.conv_stacks.{s}.blocks.{b}"
            y = O64.conv1d(O64.relu(y), sd[f"{q}.conv.weight"], sd[f"{q}.conv.bias"], padding=(k - 1) // 2) * valid
            y = O64.layer_norm(y, sd[f"{q}.norm.weight"], sd[f"{q}.norm.bias"]) * valid
        x = x + y
    return x


def decoder_rows64(gen, case, gap):
    """The mel decoder of all utterances of a case laid out in one buffer with `gap` zero rows between them -> per slot [T, 80]."""
    cfg, sd = generator(gen)[0], _sd64(gen)
    xs = [s["xdec"].astype(np.float64) for s in inputs(gen, case)]
    buf, valid, off = _buffer(xs, gap)
    k, pad = cfg.kernel_size, (cfg.kernel_size - 1) // 2
    x = O64.conv1d(buf, sd["decoder.first_layer.weight"], sd["decoder.first_layer.bias"], padding=pad) * valid
    x = _stack_rows(sd, "decoder.conv_stack", x, valid, k, cfg.decoder_n_stack, cfg.decoder_n_block)
    y = O64.conv1d(x, sd["decoder.last_layer.weight"], sd["decoder.last_layer.bias"], padding=pad) * valid
    return [y[o:o + x_.shape[0]] for o, x_ in zip(off, xs)]
