"""Every form of the parallel (non-AR) stage wiring against a float64 forward (GPU).

csrc/model_stages.hip: the stages in front of and behind the AR steps - the MRTE mel encoder (mel_context_rows), the phone encoder and
the cross attention (tc_latent_rows, encoder_layer), the VQ prosody encoder (vqpe_rows) and the mel decoder (decoder_rows), the conv
stacks of all of them in run_stack - decide from the row counts and from run-time options WHICH kernels run: the weight-streaming
kernel for linears of at most 64 rows, the f32 K-split / 64x64 tiles for convolutions with few tiles, the x6 / x3h K-split tiles for
linears, the loader tiles from t_x6_256 / t_x6_128 / t_x3h_128 tiles on, the window tiles for square one-group convolutions; whether a
LayerNorm of run_stack stores ReLU'd fp16 planes for the next block's convolution; which attention kernel serves a ragged launch.  This
file runs the cases of tests/stage_ref.py (production widths, and the small 7-tap generator k7; a different utterance in every slot,
lengths not in sorted order) under every option setting of SETTINGS and asserts per (generator, case, setting):

  parity    every row r of every utterance of the four outputs (mel_context, tc_latent, ze, decoder mel):
            e[r] = ||y[r] - y64[r]|| / max_r' ||y64[r']|| <= 8 x E32 against the float64 forward of stage_ref.  E32 is the float32
            oracle's own worst row against that forward (tests/test_stage_ref_host.py; pinned in stage_ref).
  discrete  the VQ codes are the float64 arg-min on EVERY row (the host test shows the margins are 77 bars wide at the least); zq is
            the codebook rows of those codes; every padded position behind an utterance's length is exactly zero; range_fallbacks
            unchanged (no call ran twice).
  witness   a setting names the log entries it is there to reach (generator, case, kind, decision point, form, fields); the form log
            (mt2_form_log_begin / _end) of its run shows them and the default run of the same case does not.
  identity  a_planes = 0 leaves the bits of the default in all outputs (the planes are the split of the same f32 values); settings
            that cannot change a launch of these stages (skinny_tm = 0; attn_lds_min = 0, attn_x6_min = 0; t_x3h_128 = 100000
            wherever no launch has 72 tiles) leave the bits of the default; the default call made twice leaves the same bits.
  alone     every utterance of `pair` and `ragged` as a batch of one passes the same parity: a batch is B independent runs, held
            against float64 on both sides.
  coverage  over the whole file the (kind, decision point, form / tile) triples seen are exactly EXPECTED (test_every_form_is_reached).

Measured on an MI355X (test_every_form_is_reached prints both tables, pytest -s).  E32 (mel_context, tc_latent, ze, mel) = 6.4e-7, 8.0e-6,
5.1e-7, 6.0e-7 on prod (recomputed 5.33e-7, 6.64e-6, 4.22e-7, 4.98e-7) and 7.0e-7, 5.7e-6, 5.2e-7, 7.1e-7 on k7 (5.86e-7, 4.76e-6,
4.37e-7, 5.95e-7); the bar is e / E32 <= 8.  Worst e / E32 over all cases and rows, per setting and stage (mel_context tc_latent ze mel):
    default                            prod 0.83 0.92 0.73 1.10    k7 0.52 0.53 1.25 0.62
    x3h=0                              prod 0.96 1.78 0.73 1.10    k7 0.81 0.55 1.25 1.06
    x3h=0,x6_gemm=0                    prod 0.87 0.82 0.73 1.10    k7 0.81 0.59 1.25 1.06
    a_planes=0                         prod 0.83 0.92 0.73 1.10    k7 0.52 0.52 1.25 0.62
    t_x3h_128=1                        prod 0.86 1.18 0.80 1.05    k7 0.55 0.63 1.22 0.70
    t_x3h_128=100000                   prod 0.87 0.74 0.73 1.10    k7 0.52 0.52 1.25 0.62
    x3h=0,t_x6_256=1                   prod 2.09 1.98 1.82 2.48    k7 1.16 1.25 1.43 1.49
    x3h=0,t_x6_128=1                   prod 2.09 1.98 1.82 2.48    k7 1.16 1.25 1.43 1.49
    t32x32=0                           prod 1.08 1.13 0.98 1.28    k7 0.60 0.81 1.13 0.75
    t32x32=0,t32=0                     prod 1.08 1.28 0.98 1.28    k7 0.60 0.56 1.13 0.75
    t32x32=0,t32=0,t_ks4=0             prod 1.55 1.58 1.34 1.91    k7 0.77 0.57 1.25 0.94
    t32x32=0,t32=0,t_ks4=0,t_ks2=0     prod 2.16 4.47 1.95 2.62    k7 1.10 0.87 1.39 1.20
    x6_ks=0                            prod 0.83 1.44 0.73 1.10    k7 0.52 0.81 1.25 0.62
    skinny_tm=0                        prod 0.83 0.92 0.73 1.10    k7 0.52 0.52 1.25 0.62
    skinny_rows=16                     prod 0.83 0.95 0.73 1.10    k7 0.52 0.52 1.25 0.62
    force_gemm_config=12               prod 2.12 3.52 1.95 2.62    k7 1.43 1.20 1.39 1.39
    attn_lds_min=32                                                k7 0.52 0.58 1.25 0.62
    attn_x6_min=32,x3h=15 / x3h=7                                  k7 0.52 0.49 1.25 0.62
    attn_lds_min=0,attn_x6_min=0                                   k7 0.52 0.52 1.25 0.62
    win_conv=0 / x6_conv=0                                         k7 0.49 0.56 1.25 0.54 / 0.97 0.76 1.25 0.96
and per form and tile.  A call's worst rows are booked on the forms of a default run, and for any other setting only on the forms and
tiles that the default run of the same case does not show, by the stages the kind feeds:
    conv       dma128x32 1.25  dma32x32k8 1.25  dma32x64k4 1.28  dma64x64k4 1.28  dma64x64k2 1.91  dma64x64 (s3) 4.47  win128x128 0.97
               x6winl128x128 1.49  x3hwin128x128 0.62  x6ldr128x128 2.48  x6ldr256x128 2.48  x3hldr128x128 1.22
    linear     skinny32 1.25  skinny64 1.25  dma32x32k8 1.44  dma32x64k4 1.25  dma64x64k4 1.44  dma64x64 (s3) 4.47  x6ks32x32k8 1.78
               x6ks32x64k4 0.55  x6ks64x64k2 1.78  x3hks32x32k8 0.92  x3hks32x64k4 1.13  x3hks64x64k2 1.58  x6ldr128x128 1.98  x6ldr256x128 1.98
               x3hldr128x128 1.18
    ln         block 1.25  block+planes 1.22  residual 1.25  plain 0.92        attention  generic 0.92  ds 0.53  reg 0.53  lds 0.58  x6 0.49  x3h 0.49
Every triple of EXPECTED is reached and no other.  No form comes nearer to the bar than a factor of 1.8 (4.47: tc_latent of `rows` with
everything on the plain 64x64 f32 tile, whose one serial K chain rounds most; the default stays below 1.3): the device's rows are as
close to float64 as the float32 oracle's.  All identities hold; the alone runs pass with the figures of their batch (0.05 .. 1.25).

ONE WIRING ERROR WAS FOUND, in the row layouts that the four drivers are handed (make_rows(.., 2) in tc_latent_rows, plan_mel,
plan_frames, vqpe_rows and the mt2_mel_decoder entry; max(stride / 2, 2) for the prompt rows; the same numbers in mt2_workspace_query).
The gap between the utterances of a batch was 2 rows whatever the model: zero padding IS that gap, and 2 rows cover kernels of at most
5 taps - every configuration that was ever tested.  k7 (7 taps: halo 3) read its neighbours' rows: with the constants put back, all four
outputs of every utterance of k7 / pair and k7 / ragged miss the bar, from the shared edges far into the utterances - mel_context by up to
6.3e5 x E32, tc_latent 1.0e5, ze 6.2e6 (and 3 of the 5 VQ codes of `pair` wrong), decoder mel 2.7e6 - while k7 / one, every utterance alone and all of prod pass with the figures above
(tests/test_stage_ref_host.py shows the same on the CPU: 7e4 .. 9e4 bars at the shared edge).  The gaps now follow from the model
(prompt_mel_gap, mel_context_gap, phone_gap, decoder_gap, vqpe_gap in model_stages.hip: the widest halo of the convolutions over the row
set, never less than the 2 / stride / 2 rows of before - the production and tiny layouts, their outputs (bit for bit against the parent
commit on prod_utt0, alone and in a batch of two) and the workspace bound are unchanged), the drivers refuse a row set narrower than their
halo, and even kernel sizes - which the reference itself cannot run: its residual adds fail - are refused at load.
"""
import contextlib
import fnmatch

import numpy as np
import pytest

import stage_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KINDS = ("mel-encoder", "phone-encoder", "cross", "vqpe", "decoder")
OUTPUTS = ("mel_context", "tc_latent", "zq", "codes", "ze", "mel")

# ---------------------------------------------------------------------------------------------------
# option settings: (name, options, generators, witnesses).  A witness is (generator, case, kind, point, form, fields): the form log of
# that setting's run of that case has such an entry (ints exactly, strings as fnmatch patterns) and the default run of the same case
# has none.  Each is derived from the code it names (gemm_dispatch.hip: choose_cfg, gemm_route; attention.hip: attn_route).
# Rows of the launches (every row set with its gaps: make_rows): prod gaps 8 (prompt mel: stride / 2) and 2; k7 gaps 3 (halo of 7 taps)
#   gen  case    phone P  prompt F  context X  target F  pooled Q  decoder D
#   prod one     5        33        6          5         5         5
#   prod ragged  115      291       28         190       35        190
#   prod rows    143      429       35         333       50        333
#   k7   one     5        23        11         7         7         7
#   k7   pair    20       56        22         35        14        35
#   k7   ragged  115      266       79         195       40        195
# and what choose_cfg makes of them by default (widths: prod 512 / 384 (vqpe) with 5 / 3 groups, k7 128 with 2 groups):
#   * a linear layer of at most 64 rows runs on the weight-streaming kernel (skinny32 / skinny64; NOT its tile-major form: only the
#     Linear-FF encoders of the AR models have tile-major copies, model_load.hip) - every linear of `one`, of k7 / pair, the K / V
#     projection (X rows) and the VQ distance GEMM (Q rows) of every case;
#   * longer linears (taps = 1, planes) run on the x3h K-split tiles: 32x32 k8 (K >= 512, <= 160 tiles of 32x32), 32x64 k4 (<= 64 tiles), 64x64 k2;
#   * convolutions (taps > 1: no x6 / x3h K-split form) stay on the f32 ladder 32x32 k8 -> 32x64 k4 -> 64x64 k4 -> k2 -> s3 by tile count
#     until 72 tiles of 128x128 put them on the x3h loader tile: the prompt stack of `rows` only (4 x 4 x 5 = 80);
#   * k7's decoder stack and mel-encoder last layer - square, 128 channels, one group, no row map - are win_eligible: x3hwin128x128.
K7 = ("k7",)
QKV_RAGGED = ("prod", "ragged", "phone-encoder", "linear", "qkv")       # M = 115, N = 1536, K = 512: 48 tiles of 64x64 -> 64x64 k4 -> its x6 / x3h form (k2)
KV_K7 = ("k7", "ragged", "cross", "linear", "kv")                        # M = 79, N = 256, K = 128 (< 512: no 32x32 k8): 12 tiles of 32x64 -> 32x64 k4
STACK_ROWS = ("prod", "rows", "mel-encoder", "conv", "block")            # M = 429, N = 512, 5 groups: 80 tiles of 128x128, 280 of 64x64
MID_ONE = ("prod", "one", "mel-encoder", "conv", "mid")                  # M = 6, 5 groups, ONE weight (strideW = 0), 17 taps through the row map
DEC_ONE = ("prod", "one", "decoder", "conv", "block")                    # M = 5, N = 512, 5 taps
DEC_RAGGED = ("prod", "ragged", "decoder", "conv", "block")              # M = 190: 96 tiles of 32x32 by default; 24 of 64x64
DEC_K7 = ("k7", "pair", "decoder", "conv", "block")                      # M = 35, 128 -> 128, 7 taps: the window tile
S3 = "dma64x64_2x2_s3"
SETTINGS = [
    ("default", {}, R.GENERATORS, []),
    # ---- the fp16 pipe off: every x3h tile in its x6 form (kX3hForm backwards): K-split, loader (t_x6_128 = 72 <= 80) and window
    ("x3h=0", {"x3h": 0}, R.GENERATORS, [QKV_RAGGED + ({"tile": "x6ks64x64*k2*", "M": 115},), STACK_ROWS + ({"tile": "x6ldr128x128*", "groups": 5},),
                                         KV_K7 + ({"tile": "x6ks32x64*k4*"},), DEC_K7 + ({"tile": "x6winl128x128*"},)]),
    # ---- ... and no bf16 pipe for the GEMMs either: the f32 K-split tiles themselves (`rows`: 280 tiles of 64x64 > t_ks4 = 256: k2); the
    # window convolutions follow x6_conv, not x6_gemm
    ("x3h=0,x6_gemm=0", {"x3h": 0, "x6_gemm": 0}, R.GENERATORS, [QKV_RAGGED + ({"tile": "dma64x64*k4*"},), STACK_ROWS + ({"tile": "dma64x64*k2*"},),
                                                                 KV_K7 + ({"tile": "dma32x64*k4*"},), DEC_K7 + ({"tile": "x6winl128x128*"},)]),
    # ---- run_stack's hand-off off: the LayerNorm in front of a block convolution on the loader tile stores f32 and the convolution
    # (no prologue: relued) splits it itself; the same bits (test_planes_handoff_is_bit_identical)
    ("a_planes=0", {"a_planes": 0}, R.GENERATORS, [STACK_ROWS + ({"tile": "x3hldr128x128*", "relued": 1, "a_planes": 0},),
                                                   ("prod", "rows", "mel-encoder", "ln", "block", {"out_planes": 0, "M": 429})]),
    # ---- the x3h loader tile from one tile on: every launch with planes, more than 64 columns and K % 8 = 0 - all stacks, the strided
    # middle convolution (row map, one weight for 5 groups), the conv-FF, the linears above 64 rows; planes wherever a stack has more
    # than 64 rows (gemm_takes_planes)
    ("t_x3h_128=1", {"t_x3h_128": 1}, R.GENERATORS,
     [DEC_ONE + ({"tile": "x3hldr128x128*", "a_planes": 0},), MID_ONE + ({"tile": "x3hldr128x128*", "groups": 5, "wshared": 1},),
      ("prod", "one", "phone-encoder", "conv", "ff", {"tile": "x3hldr128x128*"}), QKV_RAGGED + ({"tile": "x3hldr128x128*"},),
      DEC_RAGGED + ({"tile": "x3hldr128x128*", "relued": 1, "a_planes": 1},), ("prod", "ragged", "decoder", "ln", "block", {"out_planes": 1, "M": 190}),
      ("prod", "ragged", "vqpe", "ln", "block", {"out_planes": 1, "groups": 3}), ("k7", "ragged", "mel-encoder", "ln", "block", {"out_planes": 1, "M": 266, "groups": 2}),
      KV_K7 + ({"tile": "x3hldr128x128*"},)]),
    # ---- never the loader tile: the prompt stack of `rows` falls back to the f32 ladder (k2); no other launch has 72 tiles - the other
    # cases leave the same bits (test_unreached_thresholds_and_repeated_calls_leave_the_same_bits)
    ("t_x3h_128=100000", {"t_x3h_128": 100000}, R.GENERATORS, [STACK_ROWS + ({"tile": "dma64x64*k2*", "a_planes": 0},)]),
    # ---- both bf16 loader tiles
    ("x3h=0,t_x6_256=1", {"x3h": 0, "t_x6_256": 1}, R.GENERATORS, [DEC_ONE + ({"tile": "x6ldr256x128*"},), MID_ONE + ({"tile": "x6ldr256x128*", "wshared": 1},),
                                                                   QKV_RAGGED + ({"tile": "x6ldr256x128*"},), KV_K7 + ({"tile": "x6ldr256x128*"},)]),
    ("x3h=0,t_x6_128=1", {"x3h": 0, "t_x6_128": 1}, R.GENERATORS, [DEC_ONE + ({"tile": "x6ldr128x128*"},), MID_ONE + ({"tile": "x6ldr128x128*", "wshared": 1},),
                                                                   QKV_RAGGED + ({"tile": "x6ldr128x128*"},), KV_K7 + ({"tile": "x6ldr128x128*"},)]),
    # ---- the f32 ladder for convolutions with few tiles, one rung at a time (prod / one: 40 tiles of 32x64 in the context stack and the
    # middle convolution, 8 in the decoder; 24 tiles of 64x64 in the decoder of `ragged`) - with taps > 1, groups and the row map
    ("t32x32=0", {"t32x32": 0}, R.GENERATORS, [MID_ONE + ({"tile": "dma32x64*k4*", "groups": 5, "wshared": 1, "taps": 17},), DEC_ONE + ({"tile": "dma32x64*k4*", "taps": 5},),
                                               ("k7", "pair", "vqpe", "conv", "block", {"tile": "dma32x64*k4*", "groups": 2, "taps": 7})]),
    ("t32x32=0,t32=0", {"t32x32": 0, "t32": 0}, R.GENERATORS, [MID_ONE + ({"tile": "dma64x64*k4*", "groups": 5},), DEC_ONE + ({"tile": "dma64x64*k4*"},),
                                                               ("k7", "pair", "vqpe", "conv", "block", {"tile": "dma64x64*k4*", "groups": 2})]),
    ("t32x32=0,t32=0,t_ks4=0", {"t32x32": 0, "t32": 0, "t_ks4": 0}, R.GENERATORS, [MID_ONE + ({"tile": "dma64x64*k2*", "groups": 5},), DEC_RAGGED + ({"tile": "dma64x64*k2*"},),
                                                                                   ("k7", "pair", "vqpe", "conv", "block", {"tile": "dma64x64*k2*"})]),
    ("t32x32=0,t32=0,t_ks4=0,t_ks2=0", {"t32x32": 0, "t32": 0, "t_ks4": 0, "t_ks2": 0}, R.GENERATORS,
     [MID_ONE + ({"tile": S3, "groups": 5},), DEC_RAGGED + ({"tile": S3},), ("k7", "pair", "vqpe", "conv", "block", {"tile": S3}), QKV_RAGGED + ({"tile": S3},)]),
    # ---- the K-split linears on the f32 tiles (the loader tile and the window tiles stay)
    ("x6_ks=0", {"x6_ks": 0}, R.GENERATORS, [QKV_RAGGED + ({"tile": "dma64x64*k4*"},), ("prod", "ragged", "cross", "linear", "q", {"tile": "dma32x32*k8*", "M": 115}),
                                             KV_K7 + ({"tile": "dma32x64*k4*"},)]),
    # ---- skinny_tm = 0: attach_tm finds no tile-major copy for any weight of these stages (model_load.hip uploads them for the
    # Linear-FF encoders of the AR models only), so the <= 64-row linears run on gemm_skinny either way: no launch changes, no
    # witness; the same bits
    ("skinny_tm=0", {"skinny_tm": 0}, R.GENERATORS, []),
    # ---- skinny_rows = 16: launches of 17 .. 64 rows leave the weight-streaming kernel for the K-split tiles: k7 / pair's 20 phone
    # rows, the 28 context rows and 35 pooled rows of prod / ragged (the codebook has no planes: f32)
    ("skinny_rows=16", {"skinny_rows": 16}, R.GENERATORS, [("k7", "pair", "phone-encoder", "linear", "qkv", {"tile": "x3hks32x64*", "M": 20}),
                                                           ("prod", "ragged", "cross", "linear", "kv", {"tile": "x3hks32x32*", "M": 28}),
                                                           ("prod", "ragged", "vqpe", "linear", "vq", {"tile": "dma32x64*k4*", "M": 35})]),
    # ---- a forced configuration: no weight-streaming kernel, no window tile, no planes: everything on the 64x64 f32 tile
    ("force_gemm_config=12", {"force_gemm_config": 12}, R.GENERATORS,
     [("prod", "one", "cross", "linear", "kv", {"tile": S3, "M": 6}), STACK_ROWS + ({"tile": S3, "a_planes": 0},), DEC_K7 + ({"tile": S3},),
      ("k7", "ragged", "vqpe", "linear", "vq", {"tile": S3})]),
    # ---- attention (attn_route): prod's heads are 256 and 512 wide: the generic kernel whatever the options.  k7: 64 wide in the phone
    # encoder (ds by default: at most 128 keys), 128 wide in the cross attention (reg).  `ragged` has 64 queries, `one` and `pair` at most 9
    ("attn_lds_min=32", {"attn_lds_min": 32}, K7, [("k7", "ragged", "phone-encoder", "attention", "lds", {"qlen": 64, "D": 64}),
                                                   ("k7", "ragged", "cross", "attention", "lds", {"qlen": 64, "kvlen": 33, "D": 128})]),
    ("attn_x6_min=32,x3h=15", {"attn_x6_min": 32, "x3h": 15}, K7, [("k7", "ragged", "phone-encoder", "attention", "x3h", {"qlen": 64, "kvlen": 64})]),
    ("attn_x6_min=32,x3h=7", {"attn_x6_min": 32, "x3h": 7}, K7, [("k7", "ragged", "phone-encoder", "attention", "x6", {"qlen": 64})]),
    # never the LDS / bf16 kernels: at 64 queries the defaults (640, 192) never reach them either - no launch changes; the same bits
    ("attn_lds_min=0,attn_x6_min=0", {"attn_lds_min": 0, "attn_x6_min": 0}, K7, []),
    # ---- k7's window convolutions off the x3h window tile: the f32 ladder (8 tiles of 32x32, K = 896) / the f32 window tile
    ("win_conv=0", {"win_conv": 0}, K7, [DEC_K7 + ({"tile": "dma32x32*k8*", "taps": 7},), ("k7", "pair", "mel-encoder", "conv", "last", {"tile": "dma32x32*k8*"})]),
    ("x6_conv=0", {"x6_conv": 0}, K7, [DEC_K7 + ({"tile": "win128x128*"},), ("k7", "pair", "mel-encoder", "conv", "last", {"tile": "win128x128*"})]),
]
SETTING = {s[0]: s for s in SETTINGS}
PARAMS = [pytest.param(g, c, s[0], id=f"{g}-{c}-{s[0]}") for s in SETTINGS for g in s[2] for c in R.BATCH_CASES[g]]
ALONE_PARAMS = [pytest.param(g, c, id=f"{g}-{c}") for g in R.GENERATORS for c in R.GEN_CASES[g] if c not in R.BATCH_CASES[g]]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def nat():
    """This file's own handles, one per generator, G only: no option set here can leak into another file."""
    from megatts2_amd.runtime import NativeModel
    handles = {}
    for g in R.GENERATORS:
        cfg, sd = R.generator(g)
        handles[g] = NativeModel(g_cfg=cfg, sd_g=sd)
    yield handles
    for h in handles.values():
        h.close()


@contextlib.contextmanager
def options(h, opts):
    prev = {k: h.get_option(k) for k in opts}
    try:
        for k, v in opts.items():
            h.set_option(k, v)
        yield
    finally:
        for k, v in prev.items():
            h.set_option(k, v)


def padded(arrs, dtype):
    out = np.zeros((len(arrs), max(a.shape[0] for a in arrs)) + arrs[0].shape[1:], dtype)
    for b, a in enumerate(arrs):
        out[b, :a.shape[0]] = a
    return out


_RUNS = {}


def run(handles, gen, case, setting, again=False):
    """The four stage calls of (generator, case) under a setting, once per module: {"out": device tensors by name, "log"}."""
    key = (gen, case, setting, again)
    if key in _RUNS:
        return _RUNS[key]
    h = handles[gen]
    slots = R.inputs(gen, case)
    pl, ml, tl = (np.asarray(v, np.int32) for v in R.CASES[case])
    phone, prompt = dev(padded([s["phone"] for s in slots], np.int64)), dev(padded([s["prompt"] for s in slots], np.float32))
    target = dev(padded([s["target"] for s in slots], np.float32))
    xdec = dev(padded([s["xdec"] for s in slots], np.float32).transpose(0, 2, 1))        # "B D T"
    fallbacks = h.range_fallbacks
    with options(h, SETTING[setting][1]):
        h.form_log_begin()
        try:
            out = {"mel_context": h.mel_context(prompt, ml), "tc_latent": h.tc_latent(phone, prompt, pl, ml)}
            out["zq"], out["codes"], out["ze"] = h.vqpe_forward(target, tl, return_ze=True)
            out["mel"] = h.mel_decoder(xdec, tl)
            torch.cuda.synchronize()
        finally:
            log = h.form_log_end()
    assert h.range_fallbacks == fallbacks, "the fp16 range guard tripped: a call ran twice"
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


def judge(handles, gen, case, setting):
    """run() + every figure of the calls, once per module: r["ratios"] - {stage: worst e / E32 over the rows of all utterances};
    r["problems"] - what the assertions of test_stage_forms would say (empty: parity within the bar, discrete outputs right).
    Prints each utterance's figures."""
    r = run(handles, gen, case, setting)
    if "ratios" in r:
        return r
    cfg, _ = R.generator(gen)
    st, E = cfg.vqpe.stride, R.codebook(gen)
    o = {k: v.cpu().numpy() for k, v in r["out"].items()}
    o["mel"] = o["mel"].transpose(0, 2, 1)           # [B, T, 80]
    ratios, problems = dict.fromkeys(R.STAGES, 0.0), []
    for b, ref in enumerate(R.reference(gen, case)):
        n, tp, t = (v[b] for v in R.CASES[case])
        rows = {"mel_context": (tp - 1) // cfg.mrte.mel_stride + 1, "tc_latent": n, "ze": -(-t // st), "mel": t}
        for s in R.STAGES:
            y = o[s][b]
            if y[rows[s]:].any():
                problems.append(f"slot {b} {s}: rows behind the utterance's {rows[s]} are not zero")
            q = R.row_err(y[:rows[s]], ref[s]) / R.e32(gen, s)
            w = int(q.argmax())
            print(f"{gen} {case} [{setting}] slot {b} {s} ({q.size} rows): worst e / E32 {q.max():.2f} at row {w}, first {q[0]:.2f} last {q[-1]:.2f} "
                  f"median {np.median(q):.2f}")
            ratios[s] = max(ratios[s], float(q.max()))
            if not (q <= 8.0).all():
                bad = np.flatnonzero(~(q <= 8.0))
                problems.append(f"slot {b} {s}: e / E32 above the bar of 8 at rows {bad.tolist()[:8]} of {q.size}: {q[bad][:8].round(1).tolist()}")
        tq = rows["ze"]
        codes = o["codes"][0, b]
        if not np.array_equal(codes[:tq], ref["codes"]):
            problems.append(f"slot {b}: the device's codes are not the float64 arg-min at rows {np.flatnonzero(codes[:tq] != ref['codes']).tolist()[:8]}")
        if codes[tq:].any() or o["zq"][b, t:].any():
            problems.append(f"slot {b}: codes / zq behind the utterance's length are not zero")
        if not np.array_equal(o["zq"][b, :t], np.repeat(E[ref["codes"]], st, axis=0)[:t]):
            problems.append(f"slot {b}: zq is not the codebook rows of the codes")
    r["ratios"], r["problems"] = ratios, problems
    return r


def tile_of(attrs):
    """dma64x64_2x2_k4_s2 -> dma64x64k4, x3hks32x32_1x1_k8+8_s2 -> x3hks32x32k8, dma64x64_2x2_s3 -> dma64x64: the tile and how it splits K"""
    parts = str(attrs.get("tile", "")).split("_")
    ks = [p.split("+")[0] for p in parts[1:] if p[:1] == "k" and p[1:2].isdigit()]
    return parts[0] + (ks[0] if ks else "")


def form_keys(log):
    """(kind, point, form / tile) of every entry: a convolution or linear layer by the tile it ran on and - as its own triple, point
    conv-layer / linear-layer - by which layer it is; a LayerNorm by its form and whether it stored planes; an attention launch by its kernel."""
    out = set()
    for kind, point, form, a in log:
        if point in ("conv", "linear"):
            out |= {(kind, point, tile_of(a)), (kind, point + "-layer", form)}
        elif point == "ln":
            out.add((kind, point, form + ("+planes" if a.get("out_planes") else "")))
        else:
            out.add((kind, point, form))
    return out


@pytest.mark.parametrize("gen,case,setting", PARAMS)
def test_stage_forms(nat, gen, case, setting):
    r = judge(nat, gen, case, setting)
    assert not r["problems"], r["problems"]
    assert r["log"] and {e[0] for e in r["log"]} == set(KINDS), sorted({e[0] for e in r["log"]})
    base = run(nat, gen, case, "default")["log"]
    for wg, wc, kind, point, form, fields in SETTING[setting][3]:
        if (wg, wc) != (gen, case):
            continue
        assert any(matches(e, kind, point, form, fields) for e in r["log"]), \
            (f"{setting} did not reach {kind} {point} {form} {fields}", sorted(form_keys(r["log"])))
        assert not any(matches(e, kind, point, form, fields) for e in base), f"the default run already shows {kind} {point} {form} {fields}"


@pytest.mark.parametrize("gen,case", ALONE_PARAMS)
def test_each_utterance_alone(nat, gen, case):
    """Every utterance of `pair` and `ragged` as a batch of one passes the same parity against the same float64 forward: the N1
    property (a batch is B independent runs) held against float64 on both sides."""
    r = judge(nat, gen, case, "default")
    assert not r["problems"], r["problems"]


def test_default_forms(nat):
    """What the comment above SETTINGS derives for the default run: the weight-streaming kernel for every linear of `one`, the x3h
    K-split tiles above 64 rows, the f32 ladder for the convolutions, the loader tile with the planes hand-off for the prompt stack of
    `rows` (shared input in the first block of the first stack, per-group input behind it), the window tile for k7's decoder stack;
    pool, sum over groups and VQ leave one entry per launch that the log knows of."""
    log = run(nat, "prod", "one", "default")["log"]
    assert {tile_of(e[3]) for e in log if e[1] == "linear"} == {"skinny32"}
    assert {tile_of(e[3]) for e in log if e[1] == "conv"} == {"dma32x32k8", "dma32x64k4"}          # (first layers: K = 3 x 80, 5 x 20 < 512)
    log = run(nat, "prod", "rows", "default")["log"]
    for want in (STACK_ROWS + ({"tile": "x3hldr128x128*", "shared": 1, "relued": 0, "a_planes": 0, "groups": 5},),
                 STACK_ROWS + ({"tile": "x3hldr128x128*", "shared": 0, "relued": 0, "a_planes": 0},),
                 STACK_ROWS + ({"tile": "x3hldr128x128*", "shared": 0, "relued": 1, "a_planes": 1},),
                 ("prod", "rows", "mel-encoder", "ln", "block", {"out_planes": 1, "act": 1, "M": 429, "groups": 5}),
                 ("prod", "rows", "mel-encoder", "ln", "residual", {"out_planes": 0, "act": 0, "M": 429}),
                 ("prod", "rows", "mel-encoder", "conv", "mid", {"M": 35, "taps": 17, "groups": 5, "shared": 0, "wshared": 1, "tile": "dma32x32*k8*"}),
                 ("prod", "rows", "mel-encoder", "conv", "block", {"M": 35, "tile": "dma32x32*k8*", "a_planes": 0}),
                 ("prod", "rows", "phone-encoder", "linear", "qkv", {"M": 143, "tile": "x3hks64x64*k2*"}),
                 ("prod", "rows", "cross", "linear", "kv", {"M": 35, "tile": "skinny64*"}),
                 ("prod", "rows", "cross", "attention", "generic", {"B": 3, "qlen": 70, "kvlen": 13, "D": 512}),
                 ("prod", "rows", "vqpe", "linear", "vq", {"M": 50, "N": 1024, "K": 256, "tile": "skinny64*"})):
        assert any(matches(e, *want[2:]) for e in log), (want, sorted(form_keys(log)))
    # the mel encoder runs twice (mel_context, tc_latent): 2 x (2 stacks x 5 x 2 blocks) block convolutions, half of them on the prompt rows
    assert sum(e[0] == "mel-encoder" and e[1] == "conv" and e[2] == "block" for e in log) == 2 * 2 * 5 * 2
    assert sum(e[0] == "mel-encoder" and e[1] == "ln" and e[3].get("out_planes") == 1 for e in log) == 2 * 5
    log = run(nat, "k7", "ragged", "default")["log"]
    for want in (("decoder", "conv", "block", {"tile": "x3hwin128x128*", "taps": 7, "groups": 1, "M": 195}),
                 ("mel-encoder", "conv", "last", {"tile": "x3hwin128x128*", "M": 79}),
                 ("phone-encoder", "attention", "ds", {"B": 4, "qlen": 64, "kvlen": 64, "D": 64}),
                 ("cross", "attention", "reg", {"B": 4, "qlen": 64, "kvlen": 33, "D": 128}),
                 ("vqpe", "conv", "last", {"N": 32, "tile": "dma128x32*"})):
        assert any(matches(e, *want) for e in log), (want, sorted(form_keys(log)))


def test_witnesses_name_cases_and_forms_that_exist():
    for name, _, gens, wit in SETTINGS:
        assert all(g in R.GENERATORS for g in gens)
        for wg, wc, kind, point, form, fields in wit:
            assert wg in gens and wc in R.BATCH_CASES[wg] and kind in KINDS and point in ("conv", "linear", "ln", "attention"), (name, wg, wc, kind, point)
            if point == "attention" or point == "ln":
                assert (kind, point, form + ("+planes" if fields.get("out_planes") else "")) in EXPECTED, (name, kind, point, form)
            else:
                assert (kind, point + "-layer", form) in EXPECTED, (name, kind, point, form)
    assert all(s[3] for s in SETTINGS if s[0] not in ("default",) + SAME_BITS)


def same_bits(nat, gen, case, a, b):
    x, y = run(nat, gen, case, a)["out"], run(nat, gen, case, b)["out"]
    for k in OUTPUTS:
        assert torch.equal(x[k], y[k]), f"{gen} {case} {k}: {a} differs from {b}"


# settings that cannot change a launch of these stages (see SETTINGS): no witness, the bits of the default
SAME_BITS = ("skinny_tm=0", "attn_lds_min=0,attn_x6_min=0")


def test_planes_handoff_is_bit_identical(nat):
    """a_planes = 0 leaves the same bits as the default in all outputs: the planes a LayerNorm stores are the split of the same f32
    values that the convolution would split itself (test_layernorm_relu_planes_feed_a_convolution_bit_for_bit) - on `rows`, where the
    default hands planes over, and everywhere else, where it does not."""
    assert any(e[1] == "ln" and e[3].get("out_planes") == 1 for e in run(nat, "prod", "rows", "default")["log"])
    for gen in R.GENERATORS:
        for case in R.BATCH_CASES[gen]:
            same_bits(nat, gen, case, "default", "a_planes=0")


def test_unreached_thresholds_and_repeated_calls_leave_the_same_bits(nat):
    for gen in R.GENERATORS:
        for case in R.BATCH_CASES[gen]:
            for s in SAME_BITS:
                if gen in SETTING[s][2]:
                    same_bits(nat, gen, case, "default", s)
            if (gen, case) != ("prod", "rows"):          # (the only case with 72 tiles of 128x128)
                same_bits(nat, gen, case, "default", "t_x3h_128=100000")
        for case in R.GEN_CASES[gen]:
            x, y = run(nat, gen, case, "default")["out"], run(nat, gen, case, "default", again=True)["out"]
            assert all(torch.equal(x[k], y[k]) for k in OUTPUTS), (gen, case)


def test_form_log_only_observes_and_no_option_leaks(nat):
    """With the log off the default call leaves the bits it leaves with the log on; nothing is recorded without a call; every option is
    back at the value of a fresh handle."""
    from megatts2_amd.runtime import NativeModel
    h = nat["k7"]
    slots = R.inputs("k7", "pair")
    tl = np.asarray(R.CASES["pair"][2], np.int32)
    mel = h.mel_decoder(dev(padded([s["xdec"] for s in slots], np.float32).transpose(0, 2, 1)), tl)
    assert torch.equal(mel, run(nat, "k7", "pair", "default")["out"]["mel"])
    cfg, sd = R.generator("k7")
    fresh = NativeModel(g_cfg=cfg, sd_g=sd)
    try:
        names = sorted({k for s in SETTINGS for k in s[1]})
        for g in R.GENERATORS:
            assert [nat[g].get_option(k) for k in names] == [fresh.get_option(k) for k in names]
            nat[g].form_log_begin()
            assert nat[g].form_log_end() == []
    finally:
        fresh.close()


@pytest.mark.parametrize("where", ["mrte", "vqpe", "decoder"])
def test_even_kernel_sizes_are_refused_at_load(where):
    """With (k - 1) // 2 padding an even kernel leaves the reference's own convolution a row short and its residual adds fail: the
    handle refuses such a model when it is loaded, not at the first launch."""
    import dataclasses

    from megatts2_amd import weights
    from megatts2_amd.runtime import NativeError, NativeModel
    cfg, _ = R.generator("k7")
    if where == "mrte":
        cfg = dataclasses.replace(cfg, mrte=dataclasses.replace(cfg.mrte, mel_kernel_size=4))
    elif where == "vqpe":
        cfg = dataclasses.replace(cfg, vqpe=dataclasses.replace(cfg.vqpe, kernel_size=6))
    else:
        cfg = dataclasses.replace(cfg, kernel_size=4)
    sd = weights.synth_state_dict(weights.inventory_g(cfg), 0, "G.")
    with pytest.raises(NativeError, match="must be odd"):
        NativeModel(g_cfg=cfg, sd_g=sd)


# ---------------------------------------------------------------------------------------------------
# coverage: what the log can emit at these shapes, from the call sites of the four drivers and choose_cfg / attn_route
LADDER = {"dma32x32k8", "dma32x64k4", "dma64x64k4", "dma64x64k2", "dma64x64"}       # the f32 tiles for launches with few tiles (t32x32, t32, t_ks4, t_ks2; s3)
LOADERS = {"x3hldr128x128", "x6ldr128x128", "x6ldr256x128"}                         # t_x3h_128 / t_x6_128 / t_x6_256
WINDOW = {"x3hwin128x128", "x6winl128x128", "win128x128"}                           # win_eligible (k7: 128 -> 128, one group): x3h & 4, x6_conv
KSPLIT = {"x3hks32x32k8", "x3hks32x64k4", "x3hks64x64k2", "x6ks32x32k8", "x6ks32x64k4", "x6ks64x64k2"}      # linears only (taps = 1)
SKINNY = {"skinny32", "skinny64"}
EXPECTED = set()
# convolutions: every stage's on the ladder and the loader tiles; the window tiles where k7 has a square one-group layer; k7's VQ
# output layer (N = 32 columns) on dma128x32
for _kind, _tiles, _layers in (("mel-encoder", LADDER | LOADERS | WINDOW, ("first", "block", "mid", "last")), ("phone-encoder", LADDER | LOADERS, ("ff",)),
                               ("vqpe", LADDER | LOADERS | {"dma128x32"}, ("first", "block", "last")), ("decoder", LADDER | LOADERS | WINDOW, ("first", "block", "last"))):
    EXPECTED |= {(_kind, "conv", t) for t in _tiles} | {(_kind, "conv-layer", w) for w in _layers}
# linears: the weight-streaming kernel, the K-split tiles on both 16-bit pipes and on f32 (x6_ks = 0, x6_gemm = 0: k8 / k4 / k4; the f32
# 64x64 k2 tile takes t_ks4 = 0 WITH x6_ks = 0, which no setting combines), the loader tiles, s3.  The cross attention's projections (512 /
# 128 columns: at most 64 tiles of 32x32) reach a 64x64 K-split tile only under t32 = 0, which leaves x3h on: x3hks64x64k2, but neither
# x6ks64x64k2 nor dma64x64k4 (x3h = 0, x6_ks = 0 find them on 32x32 k8 / 32x64 k4).  The codebook has no planes: f32 tiles only
EXPECTED |= {("phone-encoder", "linear", t) for t in SKINNY | KSPLIT | LOADERS | (LADDER - {"dma64x64k2"})}
EXPECTED |= {("cross", "linear", t) for t in SKINNY | (KSPLIT - {"x6ks64x64k2"}) | LOADERS | {"dma32x32k8", "dma32x64k4", "dma64x64"}}
EXPECTED |= {("vqpe", "linear", t) for t in SKINNY | {"dma32x64k4", "dma64x64"}}
EXPECTED |= {("phone-encoder", "linear-layer", w) for w in ("qkv", "out")} | {("cross", "linear-layer", w) for w in ("q", "kv", "out")} | {("vqpe", "linear-layer", "vq")}
# LayerNorm: run_stack's two (the block's, with or without planes; the stack's last, with the residual), the encoder's and the cross attention's
EXPECTED |= {(k, "ln", f) for k in ("mel-encoder", "vqpe", "decoder") for f in ("block", "block+planes", "residual")}
EXPECTED |= {("phone-encoder", "ln", "plain"), ("cross", "ln", "plain")}
# attention: generic for prod's heads (256, 512); k7's 64-wide heads on ds / lds / x6 / x3h, its 128-wide cross attention on reg / lds
EXPECTED |= {("phone-encoder", "attention", k) for k in ("generic", "ds", "lds", "x6", "x3h")} | {("cross", "attention", k) for k in ("generic", "reg", "lds")}


def test_every_form_is_reached(nat):
    """The (kind, point, form / tile) triples seen over every (generator, case, setting) of this file are exactly EXPECTED.  Prints
    the tables of the docstring."""
    seen, worst, form_worst = set(), {}, {}
    for name, _, gens, _ in SETTINGS:
        for gen in gens:
            for case in (R.GEN_CASES[gen] if name == "default" else R.BATCH_CASES[gen]):
                r = judge(nat, gen, case, name)
                for s in R.STAGES:
                    worst[(name, gen, s)] = max(worst.get((name, gen, s), 0.0), r["ratios"][s])
                # a call's worst rows are booked on the forms that the default run of the same case does not show (a default run: on all
                # of its forms) - the forms the setting brings, not every form that merely took part - by the stage the kind feeds
                keys = form_keys(r["log"])
                if name != "default":
                    keys -= form_keys(run(nat, gen, case, "default")["log"])
                for kind, point, form in keys:
                    if point.endswith("-layer"):
                        continue
                    for s in {"mel-encoder": ("mel_context", "tc_latent"), "phone-encoder": ("tc_latent",), "cross": ("tc_latent",), "vqpe": ("ze",),
                              "decoder": ("mel",)}[kind]:
                        form_worst[(point, form)] = max(form_worst.get((point, form), 0.0), r["ratios"][s])
                seen |= form_keys(r["log"])
    print("worst e / E32 per setting and stage (mel_context tc_latent ze mel); E32 = " +
          "; ".join(f"{g} " + " ".join(f"{R.e32(g, s):.2e}" for s in R.STAGES) for g in R.GENERATORS))
    for name, _, gens, _ in SETTINGS:
        print("    %-34s %s" % (name, "    ".join(g + " " + " ".join("%4.2f" % worst[(name, g, s)] for s in R.STAGES) for g in gens)))
    print("worst e / E32 per form and tile: over the default runs, and over the calls of settings that bring it to a case")
    for point in ("conv", "linear", "ln", "attention"):
        print("    " + point + ":  " + "  ".join("%s %.2f" % (f, w) for (p, f), w in sorted(form_worst.items()) if p == point))
    print("nearest to the bar of 8: %.2f" % max(worst.values()))
    assert not EXPECTED - seen, f"never reached: {sorted(EXPECTED - seen)}"
    assert not seen - EXPECTED, f"reached but not expected: {sorted(seen - EXPECTED)}"
