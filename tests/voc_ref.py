"""float64 reference of the HiFi-GAN V1 generator and the cases of the vocoder wiring tests (host only, no GPU).

hifigan64 restates oracle/megatts2_oracle.py: hifigan in plain numpy float64 on exactly what the device holds: the float32 weights
and mel frames, and both leaky-ReLU slopes rounded to float32 ONCE (cfg.leaky_relu_slope and F.leaky_relu's default 0.01 are
float arguments of the device's kernels).  Zero and reflect edge modes (cfg.pad_mode); cfg.inference_padding as edge frames
replicated in front of the generator; the MRF mean a plain / 3.

The generators and cases are the smallest at which every form of the vocoder wiring (csrc/model_stages.hip, hifigan_rows) can be
reached at the production widths - tests/test_gpu_voc_forms.py runs them on the device, tests/test_voc_ref_host.py pins this
reference to torch in float64 and to transformers.SpeechT5HifiGan, recomputes E32 and shows that the judge catches one row read
behind an utterance's end.  Everything here is computed once per process and shared.

The judge: per utterance and per mel frame f, err[f] = max |w - w64| over that frame's hop samples - absolute, the output being a
tanh (rms about 0.2 on these weights).  E32 is the float32 restatement's largest err[f] over all cases and frames of a generator
family (the oracle on ATen's float32 kernels, measured against hifigan64 and never against the device); the bar of a device frame is
8 x E32.
"""
import dataclasses
import functools
import zlib

import numpy as np

import megatts2_oracle as O

# E32 per generator family as test_voc_ref_host.py recomputes it (test_pinned_e32: recomputed <= E32 <= 1.5 x recomputed), pinned so
# that the GPU test does not spend CPU time on the float32 oracle.  Recomputed: 5.49e-7 over prod / prod-reflect / prod-pad5, 9.56e-7
# on wide-tail, whose waveform is four times as large (rms 0.8) - on ONE thread: ATen's float32 convolutions sum in another order
# with every thread count (5.5e-7 .. 6.5e-7 and 9.6e-7 .. 1.56e-6 with 1 to 8 threads here), so restatement32 pins the count.
# A family's own E32 is never above the largest over all generators, so neither is its bar
E32 = {"prod": 6.0e-7, "prod-reflect": 6.0e-7, "prod-pad5": 6.0e-7, "wide-tail": 1.05e-6}
FAMILIES = (("prod", "prod-reflect", "prod-pad5"), ("wide-tail",))


def e32(gen):
    return E32[gen]


def bar(gen):
    """The parity bar of a device frame: 8 x E32."""
    return 8.0 * E32[gen]


# ---------------------------------------------------------------------------------------------------
# the float64 generator, on [T, C] arrays

def conv1d64(x, w, b, padding=0, dilation=1):
    """nn.Conv1d (cross-correlation, zero padding, stride 1) on x[T, Cin] float64; w[Cout, Cin, k] -> [T_out, Cout]."""
    T, cin = x.shape
    cout, cin_w, k = w.shape
    assert cin == cin_w and x.dtype == np.float64 and w.dtype == np.float64
    t_out = T + 2 * padding - dilation * (k - 1)
    assert t_out > 0
    xp = np.zeros((T + 2 * padding, cin), np.float64)
    xp[padding:padding + T] = x
    wt = np.ascontiguousarray(w.transpose(2, 1, 0))      # [k, Cin, Cout]: one contiguous matrix per tap
    y = np.zeros((t_out, cout), np.float64)
    for tap in range(k):
        y += xp[tap * dilation: tap * dilation + t_out] @ wt[tap]
    return y if b is None else y + b


def conv_transpose1d64(x, w, b, stride, padding):
    """nn.ConvTranspose1d on x[T, Cin] float64; w[Cin, Cout, k] -> [(T - 1) stride - 2 padding + k, Cout]."""
    T, cin = x.shape
    cin_w, cout, k = w.shape
    assert cin == cin_w and x.dtype == np.float64 and w.dtype == np.float64
    wt = np.ascontiguousarray(w.transpose(2, 0, 1))      # [k, Cin, Cout]
    full = np.zeros(((T - 1) * stride + k, cout), np.float64)
    for tap in range(k):
        full[tap: tap + (T - 1) * stride + 1: stride] += x @ wt[tap]
    y = full[padding: full.shape[0] - padding]
    return y if b is None else y + b


def same64(x, w, b, dilation=1, reflect=False, extra_tail=False):
    """'same' Conv1d (odd kernel): zero padding, or - reflect - the input mirrored at both ends first (F.pad(mode="reflect"): raises
    like it when the padding is not smaller than the input).  extra_tail (the mutant of the host test, zero mode): the first row
    behind the end is a copy of the last row instead of zero."""
    g = (w.shape[2] - 1) // 2 * dilation
    if reflect and g:
        assert g < x.shape[0], "reflect padding must be smaller than the input"
        return conv1d64(np.concatenate([x[g:0:-1], x, x[-2:-g - 2:-1]], axis=0), w, b, 0, dilation)
    if extra_tail:
        assert g >= 1
        xp = np.concatenate([np.zeros((g, x.shape[1])), x, x[-1:], np.zeros((g - 1, x.shape[1]))], axis=0)
        return conv1d64(xp, w, b, 0, dilation)
    return conv1d64(x, w, b, g, dilation)


def lrelu64(x, slope):
    return np.where(x >= 0, x, x * slope)


def hifigan64(sd, cfg, mel, mutant=None):
    """mel f32 [T, in_dim] -> waveform float64 [(T + 2 cfg.inference_padding) hop].  mutant = (stage, resblock, pair): that convs2
    reads one extra copy of its last input row behind the utterance's end (a simulated wiring defect; zero mode only)."""
    w = {k: np.asarray(v, np.float32).astype(np.float64) for k, v in sd.items()}
    slope = np.float64(np.float32(cfg.leaky_relu_slope))
    slope_post = np.float64(np.float32(0.01))           # F.leaky_relu's default in front of conv_post
    reflect = getattr(cfg, "pad_mode", "zeros") == "reflect"
    assert mutant is None or not reflect
    pad = int(getattr(cfg, "inference_padding", 0))
    x = np.asarray(mel, np.float32).astype(np.float64)
    if pad:
        x = np.pad(x, ((pad, pad), (0, 0)), mode="edge")
    x = same64(x, w["conv_pre.weight"], w["conv_pre.bias"], 1, reflect)
    nk = len(cfg.resblock_kernel_sizes)
    for i, (r, k) in enumerate(zip(cfg.upsample_rates, cfg.upsample_kernel_sizes)):
        x = conv_transpose1d64(lrelu64(x, slope), w[f"upsampler.{i}.weight"], w[f"upsampler.{i}.bias"], r, (k - r) // 2)
        acc = 0.0
        for j, dils in enumerate(cfg.resblock_dilation_sizes):
            p = f"resblocks.{i * nk + j}"
            h = x
            for n, d in enumerate(dils):
                y = same64(lrelu64(h, slope), w[f"{p}.convs1.{n}.weight"], w[f"{p}.convs1.{n}.bias"], d, reflect)
                y = same64(lrelu64(y, slope), w[f"{p}.convs2.{n}.weight"], w[f"{p}.convs2.{n}.bias"], 1, reflect,
                           extra_tail=mutant == (i, j, n))
                h = y + h
            acc = acc + h
        x = acc / nk
    x = same64(lrelu64(x, slope_post), w["conv_post.weight"], w["conv_post.bias"], 1, reflect)
    return np.tanh(x[:, 0])


# ---------------------------------------------------------------------------------------------------
# generators and cases

# wide-tail: one stage of 256 channels - hifigan_rows cannot take the fused output layer at zero padding (ch <= 128 fails) and runs
# avg3 + the Cout = 1 GEMM with the tanh epilogue
GENERATORS = ("prod", "prod-reflect", "prod-pad5", "wide-tail")

# name -> mel lengths per slot, NOT in sorted order; every utterance differs from every other.
#   edges    1 frame = 8 rows at stage 0, shorter than every dilated span ((11 - 1) 5 = 50 rows); 24 frames = 192 rows at stage 0
#            (crosses a 128-row tile) and 6144 at stage 3; with 8 / 64 / 128 / 256 rows per frame and a gap of 4 frames the
#            utterance ends fall inside window tiles of 254 / 250 / 246 output rows
#   alone-k  utterance k of `edges` as a batch of one (the same mel: the same reference)
#   equal    three utterances of one length
#   pad5     inference_padding = 5: 11 and 17 frames after the replication
#   reflect  reflect needs len x scale > halo: conv_pre (halo 3) and stage 0's widest halo of 25 rows at 8 rows per frame need 4 frames
EDGES = (5, 1, 24, 2, 9)
CASES = {"edges": EDGES, "equal": (8, 8, 8), "pad5": (1, 7), "reflect": (7, 23, 9, 40)}
CASES.update({f"alone-{k}": (n,) for k, n in enumerate(EDGES)})
ALONE = tuple(f"alone-{k}" for k in range(len(EDGES)))
GEN_CASES = {"prod": ("edges",) + ALONE + ("equal",), "wide-tail": ("edges",) + ALONE, "prod-pad5": ("pad5",),
             "prod-reflect": ("reflect",)}


@functools.lru_cache(maxsize=None)
def generator(name):
    """(config, f32 state dict) of a generator: synthetic weights as everywhere in the suite."""
    from megatts2_amd import config as C
    from megatts2_amd import weights
    if name == "wide-tail":
        cfg = C.HifiGanConfig(in_dim=80, upsample_initial_channel=512, upsample_rates=[2], upsample_kernel_sizes=[4])
    else:
        cfg = C.production_hifigan()
        if name == "prod-reflect":
            cfg = dataclasses.replace(cfg, pad_mode="reflect")
        elif name == "prod-pad5":
            cfg = dataclasses.replace(cfg, inference_padding=5)
        else:
            assert name == "prod"
    return cfg, weights.synth_state_dict(weights.inventory_hifigan(cfg), 0, "hifigan.")


@functools.lru_cache(maxsize=None)
def mels(case):
    """The mel frames [T, 80] f32 of every slot of a case (synth.make_utterance(...).prompt_mel)."""
    from megatts2_amd import synth
    if case.startswith("alone-"):
        return (mels("edges")[int(case[6:])],)
    rng = np.random.Generator(np.random.PCG64([41, zlib.crc32(case.encode())]))       # (adding a case moves no other's inputs)
    return tuple(synth.make_utterance(rng, 1, T, T).prompt_mel for T in CASES[case])


def out_frames(gen, case, b):
    """Frames of slot b's waveform: its length plus the replicated frames of both sides."""
    return CASES[case][b] + 2 * int(generator(gen)[0].inference_padding)


_W64, _W32 = {}, {}


def reference(gen, case):
    """Per slot: the float64 waveform [out_frames x hop] (read-only; the alone-k cases share their utterance's of `edges`)."""
    out = []
    for m in mels(case):
        key = (gen, m.tobytes())
        if key not in _W64:
            cfg, sd = generator(gen)
            _W64[key] = hifigan64(sd, cfg, m)
            _W64[key].setflags(write=False)
        out.append(_W64[key])
    return out


def restatement32(gen, case):
    """Per slot: the float32 oracle's waveform (megatts2_oracle.hifigan on ATen's float32 kernels: plain numpy float32 takes 4 to
    15 s per utterance at production widths), on one thread: the summation order, and with it E32, follows the thread count."""
    import torch
    cfg, sd = generator(gen)
    pad = int(cfg.inference_padding)
    out = []
    for m in mels(case):
        key = (gen, m.tobytes())
        if key not in _W32:
            swapped = bool(O._NUMPY_PRIMS) and O.hifigan is not O._NUMPY_PRIMS["hifigan"]
            threads = torch.get_num_threads()
            O.enable_torch_kernels()
            try:
                torch.set_num_threads(1)
                _W32[key] = O.hifigan(sd, cfg, np.pad(m, ((pad, pad), (0, 0)), mode="edge") if pad else m)
            finally:
                torch.set_num_threads(threads)
                if not swapped:
                    O.disable_torch_kernels()
        out.append(_W32[key])
    return out


def frame_err(w, w64, hop):
    """err[f] = max |w - w64| over the hop samples of frame f."""
    w, w64 = np.asarray(w, np.float64), np.asarray(w64, np.float64)
    assert w.shape == w64.shape and w.size % hop == 0
    return np.abs(w - w64).reshape(-1, hop).max(axis=1)


@functools.lru_cache(maxsize=None)
def e32_measured(gens):
    """The float32 restatement's largest frame error over all cases of the generators `gens` (a tuple)."""
    worst = 0.0
    for g in gens:
        hop = generator(g)[0].hop
        for case in GEN_CASES[g]:
            for a, b in zip(restatement32(g, case), reference(g, case)):
                worst = max(worst, float(frame_err(a, b, hop).max()))
    return worst
