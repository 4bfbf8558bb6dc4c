"""Every form of the HiFi-GAN wiring against a float64 generator (GPU).

csrc/model_stages.hip: hifigan_rows chains ~90 launches into one call of the vocoder and decides, from the channel widths and from
run-time options, WHICH: the transposed convolution as two GEMM halves or - behind an MRF mean with a stride-2 upsampler - one
up_mrf launch that forms the mean itself; the mean by launch_avg3, inside the next upsampler or inside the output layer; every
resblock pair as one conv_pair launch or as two convolutions on x3h / x6 / f32 window tiles, K-split tiles or the loader tile; the
three resblock chains of a stage on one stream or three; the output layer fused or as avg3 + a GEMM with the tanh epilogue; six halo
fills per resblock in reflect mode.  This file runs the cases of tests/voc_ref.py (production widths, a different utterance in
every slot, lengths not in sorted order, 1 to 40 frames) under every option setting of SETTINGS and asserts per (generator, case,
setting):

  parity    every mel frame of every utterance: max |w - w64| over its hop samples <= 8 x E32 against voc_ref.hifigan64.  E32 is the
            float32 oracle's own worst frame against the float64 generator (tests/test_voc_ref_host.py; pinned in voc_ref).
  discrete  samples at or beyond an utterance's (len + 2 x inference_padding) x hop are exactly zero; range_fallbacks unchanged
            (the call did not run twice).
  witness   a setting names the log entries it is there to reach (kind, decision point, form, fields); the form log
            (mt2_form_log_begin / _end) of its run shows them and the default run of the same (generator, case) does not.  The
            default run of each generator shows exactly DEFAULT_FORMS.
  identity  the six pair_fuse values leave the same bits (hifigan_rows: "Bit-identical; NotSupported keeps the two launches
            below" - at 32, 64 and 128 channels); voc_streams = 1 equals the default (which stream a chain runs on cannot
            change a value); ldr64 = 1 equals pair_fuse = 0, up_fuse = 0 (the kernel tests' "loader address forms agree bit for
            bit"); t_x3h_128 = 100000 equals the default (see SETTINGS); the default call made twice leaves the same bits.
  coverage  over the whole file the (kind, decision point, form) triples seen are exactly EXPECTED (test_every_form_is_reached).

Measured on an MI355X (test_every_form_is_reached prints both tables, pytest -s).  E32 = 6.0e-7 (prod, prod-reflect, prod-pad5;
recomputed 5.49e-7) and 1.05e-6 (wide-tail; 9.56e-7); the bar is err / E32 <= 8.  Worst err / E32 over all cases and frames, per setting:
    setting                        prod   reflect  pad5  wide-tail      setting                        prod
    default                        0.75   0.80     0.67  2.13           x6_conv=0                      1.01
    pair_fuse=0 / 1 / 2 / 4 / 7    0.75                                 x3h=11, x3h=0                  1.03
    up_fuse=0 / 1 / 2              0.82 / 0.67 / 0.71                   x3h=0,x6_gemm=0,x6_conv=0      1.01
    up_fuse=0 (reflect)                   0.70                          ldr64=1                        0.82
    voc_streams=1                  0.75   0.80                          pair_fuse=0,up_fuse=0          0.82
    win_conv=0                     0.88                                 t_x3h_128=1 / 100000           0.66 / 0.75
                                                                        force_gemm_config=12           1.39
and per form and tile.  A call's worst frame is booked on the forms of a default run, and for any other setting only on the forms and
tiles that the default run of the same case does not show.  The prod generators:
    upsample  halves 0.80  fused 0.80      mean  avg3 0.80  in-upsample 0.80  in-post 0.75      pair  two 0.80  fused 0.75
    streams   3 0.80  1 0.80               halo  fill 0.80                                      post  fused 0.75  gemm 0.80
    tile      dma32x32 0.80  dma32x64 1.01  dma64x64 1.39  dma128x32 1.03  win128x128 / 256x64 / 256x32 1.01  x6winl128x128 / x6winl256x64 /
              x6win256x32 1.03  x3hwin128x128 0.80  x3hwin256x64 / 256x32 0.82  x3hpair 0.75  x3hupmrf 0.80  x3hldr128x128 0.66
and wide-tail (default run only): every form 2.13 - interior frames 13 and 6 of the 24- and 9-frame utterances, the edge frames 0.03 .. 0.36.
Every triple of EXPECTED is reached and no other.  No form comes nearer to the bar than a factor of 3.7; the worst frames are
interior ones as often as edge ones: the device's waveform is as close to float64 as the float32 oracle's.  All identities hold.

ONE WIRING ERROR WAS FOUND, in the row layout that hifigan_rows is handed (capi.inc, vocoder_rows).  The gap between the utterances
of a batch was 4 mel rows (8 in reflect mode) whatever the generator: zero padding IS that gap, and "4 cover the zero-padded dilated
convs" holds only where the first upsampling rate is 7 or more (the widest halo, k 11 x dilation 5, is 25 rows; production: 4 x 8 =
32).  wide-tail (x2 first: 8 rows) read its neighbours' rows: every frame of `edges` was off by 6e-4 to 0.26 absolute, 560 to 245000
x E32 (an utterance alone has no neighbour).  The gap now follows from the generator (vocoder_gap: every stage's widest halo, two
of them in reflect mode, never less than 4 / 8 - the production layout is unchanged) and hifigan_rows refuses a narrower one.
By hand, not committed: `valid` -> nullptr in the second conv_same of a pair fails parity in the first and last frames of every
utterance by 0.02 .. 0.045 absolute, 3e4 .. 7e4 x E32 (interior median 470 x; test_hifigan_stand_in catches that one too, rel-L2
6e-3 .. 9e-3); one halo() call skipped in reflect mode (stage 2, resblock 1, pair 1, the second convolution) fails the first and
last frame only, by 0.008 .. 0.02 absolute, 1.3e4 .. 3.5e4 x E32, the interior median staying at 0.5 - test_hifigan_stand_in (zero
mode) passes; test_hifigan_reflect_edge_mode sees rel-L2 2.1e-3 on its 9-frame tiny utterance.
"""
import contextlib
import fnmatch

import numpy as np
import pytest

import voc_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

STAGES = ("voc-stage0", "voc-stage1", "voc-stage2", "voc-stage3")      # prod: 256, 128, 64, 32 channels; x8, x8, x2, x2

# ---------------------------------------------------------------------------------------------------
# option settings: (name, options, generators, witnesses).  A witness is (kind, point, form, fields): the form log of that setting's
# run of every case of the generator has such an entry (ints exactly, strings as fnmatch patterns) and the default run of the same
# case has none.  Each is derived from the code it names, not from a run.  A batch of these cases has at most 111 mel rows (reflect:
# 79 frames + four gaps of 8), 888 rows at stage 0: choose_cfg (gemm_dispatch.hip) never reaches the 72 tiles of 128x128 from which
# the loader tile starts (the halves of stage 1: 7 x 4), the K-split x6 / x3h forms take linear layers only (taps == 1) and so does
# the weight-streaming kernel of launches with at most 64 rows - by default conv_pre, the upsampler halves and the 256-channel pairs
# run on f32 tiles (dma*), the 128-channel pairs on the x3h window tile.
PROD = ("prod",)
NOTHING_FUSED = [(s, "pair", "two", {}) for s in STAGES[2:]] + [(s, "upsample", "halves", {}) for s in STAGES[2:]] + \
                [(s, "mean", "avg3", {}) for s in STAGES[1:3]]
SETTINGS = [
    ("default", {}, R.GENERATORS, []),
    # ---- conv_pair_route: bit 0 the 32-channel stage (3), bit 1 the 64-channel stage (2), bit 2 the 128-channel stage (1); the
    # default 3 leaves stage 1 on two launches of the x3h window tile; 256 channels (stage 0) have no pair kernel
    ("pair_fuse=0", {"pair_fuse": 0}, PROD, [("voc-stage2", "pair", "two", {"ch": 64, "tile": "x3hwin256x64*", "tile2": "x3hwin256x64*"}),
                                             ("voc-stage3", "pair", "two", {"ch": 32, "tile": "x3hwin256x32*"})]),
    ("pair_fuse=1", {"pair_fuse": 1}, PROD, [("voc-stage2", "pair", "two", {"ch": 64, "tile": "x3hwin*"})]),
    ("pair_fuse=2", {"pair_fuse": 2}, PROD, [("voc-stage3", "pair", "two", {"ch": 32, "tile": "x3hwin*"})]),
    ("pair_fuse=4", {"pair_fuse": 4}, PROD, [("voc-stage1", "pair", "fused", {"ch": 128, "k": 11, "dil": 5, "tile": "x3hpair"}),
                                             ("voc-stage2", "pair", "two", {}), ("voc-stage3", "pair", "two", {})]),
    ("pair_fuse=7", {"pair_fuse": 7}, PROD, [("voc-stage1", "pair", "fused", {"ch": 128, "k": 3, "dil": 1, "tile": "x3hpair"}),
                                             ("voc-stage1", "pair", "fused", {"ch": 128, "k": 11, "dil": 5})]),
    # ---- up_mrf_route: bit 0 the 64-channel boundary (stage 2 -> 3), bit 1 the 128-channel one (stage 1 -> 2); a clear bit leaves
    # launch_avg3 (booked on the stage whose resblocks it averages) + the two GEMM halves (N = 32 / 64 columns: f32 tiles)
    ("up_fuse=0", {"up_fuse": 0}, PROD, [("voc-stage1", "mean", "avg3", {"ch": 128}), ("voc-stage2", "upsample", "halves", {"ch": 128, "tile": "dma*"}),
                                         ("voc-stage2", "mean", "avg3", {"ch": 64}), ("voc-stage3", "upsample", "halves", {"ch": 64, "half": 1})]),
    ("up_fuse=1", {"up_fuse": 1}, PROD, [("voc-stage1", "mean", "avg3", {}), ("voc-stage2", "upsample", "halves", {"half": 0})]),
    ("up_fuse=2", {"up_fuse": 2}, PROD, [("voc-stage2", "mean", "avg3", {}), ("voc-stage3", "upsample", "halves", {"half": 0})]),
    ("voc_streams=1", {"voc_streams": 1}, PROD, [(s, "streams", "1", {}) for s in STAGES]),
    # ---- x3h_window_engine (x3h_window.h): win_conv && x6_conv && (x3h & 4) && no forced configuration && !ldr64 - without it
    # nothing is fused (the output layer, launch_conv_post, is no window kernel and stays).  choose_cfg names the tile of the pairs:
    # win_conv = 0: no window tile - 128 columns: an f32 tile by the tile count (taps > 1: no x6 K-split form), 32 columns: dma128x32
    ("win_conv=0", {"win_conv": 0}, PROD, NOTHING_FUSED + [("voc-stage1", "pair", "two", {"tile": "dma*", "tile2": "dma*"}),
                                                           ("voc-stage3", "pair", "two", {"tile": "dma128x32*"})]),
    # x6_conv = 0: the f32 window tiles
    ("x6_conv=0", {"x6_conv": 0}, PROD, NOTHING_FUSED + [("voc-stage1", "pair", "two", {"tile": "win128x128*", "tile2": "win128x128*"}),
                                                         ("voc-stage2", "pair", "two", {"tile": "win256x64*"}),
                                                         ("voc-stage3", "pair", "two", {"tile": "win256x32*"})]),
    # x3h without bit 4 / x3h = 0: the bf16-pipe window tiles (loader-wave forms at 64 / 128 channels)
    ("x3h=11", {"x3h": 11}, PROD, NOTHING_FUSED + [("voc-stage1", "pair", "two", {"tile": "x6winl128x128*", "tile2": "x6winl128x128*"}),
                                                   ("voc-stage2", "pair", "two", {"tile": "x6winl256x64*"}),
                                                   ("voc-stage3", "pair", "two", {"tile": "x6win256x32*"})]),
    ("x3h=0", {"x3h": 0}, PROD, NOTHING_FUSED + [("voc-stage1", "pair", "two", {"tile": "x6winl128x128*"}),
                                                 ("voc-stage3", "pair", "two", {"tile": "x6win256x32*"})]),
    ("x3h=0,x6_gemm=0,x6_conv=0", {"x3h": 0, "x6_gemm": 0, "x6_conv": 0}, PROD,
     NOTHING_FUSED + [("voc-stage1", "pair", "two", {"tile": "win128x128*"}), ("voc-stage2", "pair", "two", {"tile": "win256x64*"})]),
    # ldr64: the x3h window tiles in their 64-bit loader form, which the fused kernels do not have
    ("ldr64=1", {"ldr64": 1}, PROD, NOTHING_FUSED + [("voc-stage2", "pair", "two", {"tile": "x3hwin256x64*"}),
                                                     ("voc-stage3", "pair", "two", {"tile": "x3hwin256x32*"})]),
    ("pair_fuse=0,up_fuse=0", {"pair_fuse": 0, "up_fuse": 0}, PROD, NOTHING_FUSED),
    # t_x3h_128 = 1: every launch with planes and more than 64 columns goes to the 128x128 loader tile that long batches use:
    # conv_pre (N = 512), the upsampler halves of stages 0 and 1 (N = 4 x 256, 4 x 128) and the 256-channel pairs
    ("t_x3h_128=1", {"t_x3h_128": 1}, PROD, [("voc-pre", "pre", "gemm", {"tile": "x3hldr128x128*"}),
                                             ("voc-stage0", "upsample", "halves", {"tile": "x3hldr128x128*", "half": 0}),
                                             ("voc-stage1", "upsample", "halves", {"tile": "x3hldr128x128*", "half": 1}),
                                             ("voc-stage0", "pair", "two", {"ch": 256, "tile": "x3hldr128x128*", "tile2": "x3hldr128x128*"})]),
    # t_x3h_128 = 100000: never the loader tile below t_x6_256 - but no launch of these cases has 72 tiles of 128x128 (that takes 288
    # frames in a batch): the same launches as the default, asserted bit for bit below; no witness
    ("t_x3h_128=100000", {"t_x3h_128": 100000}, PROD, []),
    # a forced configuration: no window tile, nothing fused, every GEMM on the 64x64 f32 tile
    ("force_gemm_config=12", {"force_gemm_config": 12}, PROD,
     NOTHING_FUSED + [("voc-pre", "pre", "gemm", {"tile": "dma64x64_2x2_s3"}),
                      ("voc-stage1", "pair", "two", {"tile": "dma64x64_2x2_s3", "tile2": "dma64x64_2x2_s3"}),
                      ("voc-stage3", "pair", "two", {"tile": "dma64x64_2x2_s3"})]),
    # ---- reflect mode (its default run: DEFAULT_FORMS)
    ("reflect:up_fuse=0", {"up_fuse": 0}, ("prod-reflect",), [("voc-stage1", "mean", "avg3", {}), ("voc-stage2", "upsample", "halves", {}),
                                                              ("voc-stage2", "mean", "avg3", {}), ("voc-stage3", "upsample", "halves", {})]),
    ("reflect:voc_streams=1", {"voc_streams": 1}, ("prod-reflect",), [(s, "streams", "1", {}) for s in STAGES]),
]
SETTING = {s[0]: s for s in SETTINGS}
PAIR_FUSE = ("default", "pair_fuse=0", "pair_fuse=1", "pair_fuse=2", "pair_fuse=4", "pair_fuse=7")       # (the default is 3)
PARAMS = [pytest.param(g, c, s[0], id=f"{g}-{c}-{s[0]}") for s in SETTINGS for g in s[2] for c in R.GEN_CASES[g]]


def _forms(up, mean, pair, halo, post):
    out = {("voc-pre", "pre", "gemm"), ("voc-post", "post", post)}
    for i, s in enumerate(STAGES[:len(up)]):
        out |= {(s, "upsample", up[i]), (s, "mean", mean[i]), (s, "pair", pair[i]), (s, "streams", "3")}
        if halo:
            out |= {(s, "halo", "fill")}
    return out | ({("voc-pre", "halo", "fill"), ("voc-post", "halo", "fill")} if halo else set())


# what the default run of each generator shows - exactly.  prod: stage 0 (256 channels) has neither fused form and its x8 successor
# no up_mrf: halves, two, avg3; stage 1 (128): pair_fuse bit 2 is off, its mean is formed in stage 2's x2 upsampler; stages 2, 3:
# everything fused, the last mean in the output layer.  Reflect: conv_pair_route and the fused output layer refuse, up_mrf (a
# transposed convolution has no halo) stays.  wide-tail: one stage of 256 channels, conv_post's ch <= 128 fails
DEFAULT_FORMS = {
    "prod": _forms(("halves", "halves", "fused", "fused"), ("avg3", "in-upsample", "in-upsample", "in-post"), ("two", "two", "fused", "fused"), False, "fused"),
    "prod-reflect": _forms(("halves", "halves", "fused", "fused"), ("avg3", "in-upsample", "in-upsample", "avg3"), ("two",) * 4, True, "gemm"),
    "wide-tail": _forms(("halves",), ("avg3",), ("two",), False, "gemm"),
}
DEFAULT_FORMS["prod-pad5"] = DEFAULT_FORMS["prod"]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.fixture(scope="module")
def voc():
    """This file's own vocoder handles, one per generator: no option set here can leak into another file."""
    from megatts2_amd import megatts2 as M
    handles = {g: M.HIFIGAN(*R.generator(g)) for g in R.GENERATORS}
    yield {g: h.native for g, h in handles.items()}
    for h in handles.values():
        h.native.close()


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


def run(handles, gen, case, setting, again=False):
    """One call of (generator, case) under a setting, once per module: {"wav": device tensor [B, 1, hop x frames], "log"}."""
    key = (gen, case, setting, again)
    if key in _RUNS:
        return _RUNS[key]
    nat = handles[gen]
    mels, lens = R.mels(case), np.asarray(R.CASES[case], np.int32)
    mel = np.zeros((len(mels), 80, int(lens.max())), np.float32)
    for b, m in enumerate(mels):
        mel[b, :, :m.shape[0]] = m.T
    fallbacks = nat.range_fallbacks
    with options(nat, SETTING[setting][1]):
        nat.form_log_begin()
        try:
            wav = nat.hifigan(dev(mel), lens)
            torch.cuda.synchronize()
        finally:
            log = nat.form_log_end()
    assert nat.range_fallbacks == fallbacks, "the fp16 range guard tripped: the call ran twice"
    _RUNS[key] = {"wav": wav, "log": log}
    return _RUNS[key]


def matches(entry, kind, point, form, fields):
    k, p, f, attrs = entry
    if k != kind or p != point or f != form:
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
    """run() + every figure of the call, once per module: r["ratios"] - error / E32 per (slot, frame); r["problems"] - what the
    assertions of test_voc_forms would say (empty: parity within the bar, padding zero).  Prints each utterance's figures."""
    r = run(handles, gen, case, setting)
    if "ratios" in r:
        return r
    hop, e32 = R.generator(gen)[0].hop, R.e32(gen)
    wav = r["wav"].cpu().numpy()
    ratios, problems = [], []
    for b, w64 in enumerate(R.reference(gen, case)):
        n = R.out_frames(gen, case, b) * hop
        assert n == w64.size and wav.shape[1] == 1 and wav.shape[2] >= n
        if wav[b, 0, n:].any():
            problems.append(f"slot {b}: samples beyond the utterance's {n} are not zero")
        q = R.frame_err(wav[b, 0, :n], w64, hop) / e32
        f = int(q.argmax())
        print(f"{gen} {case} [{setting}] slot {b} ({q.size} frames): worst err / E32 {q.max():.2f} at frame {f} "
              f"({'edge' if f in (0, q.size - 1) else 'interior'}), first {q[0]:.2f} last {q[-1]:.2f} median {np.median(q):.2f}")
        ratios.extend(q.tolist())
        if not (q <= 8.0).all():
            bad = np.flatnonzero(~(q <= 8.0))
            problems.append(f"slot {b}: err / E32 above the bar of 8 at frames {bad.tolist()[:8]} of {q.size}: {q[bad][:8].round(1).tolist()}")
    r["ratios"], r["problems"] = ratios, problems
    return r


def form_keys(log):
    return {(k, p, f) for k, p, f, _ in log}


@pytest.mark.parametrize("gen,case,setting", PARAMS)
def test_voc_forms(voc, gen, case, setting):
    r = judge(voc, gen, case, setting)
    assert not r["problems"], r["problems"]
    assert r["log"], "the form log is empty"
    base = run(voc, gen, case, "default")["log"]
    if setting == "default":
        assert form_keys(r["log"]) == DEFAULT_FORMS[gen], sorted(form_keys(r["log"]) ^ DEFAULT_FORMS[gen])
    for kind, point, form, fields in SETTING[setting][3]:
        assert any(matches(e, kind, point, form, fields) for e in r["log"]), \
            (f"{setting} did not reach {kind} {point} {form} {fields}", sorted({(e[0], e[1], e[2], e[3].get('tile', ''), e[3].get('tile2', '')) for e in r["log"]}))
        assert not any(matches(e, kind, point, form, fields) for e in base), f"the default run already shows {kind} {point} {form} {fields}"


def test_default_tiles_on_prod(voc):
    """The tiles of the default run, derived in the comment above SETTINGS: the 128-channel pairs on the x3h window tile, conv_pre,
    the halves and the 256-channel pairs on f32 tiles; six halo fills per resblock - and three more per stage and end - in reflect mode."""
    log = run(voc, "prod", "edges", "default")["log"]
    for want in (("voc-stage1", "pair", "two", {"ch": 128, "tile": "x3hwin128x128*", "tile2": "x3hwin128x128*"}),
                 ("voc-stage0", "pair", "two", {"ch": 256, "tile": "dma*", "tile2": "dma*"}), ("voc-pre", "pre", "gemm", {"ch": 512, "tile": "dma*"}),
                 ("voc-stage0", "upsample", "halves", {"ch": 512, "tile": "dma*"}), ("voc-stage2", "upsample", "fused", {"ch": 128, "tile": "x3hupmrf"}),
                 ("voc-stage3", "pair", "fused", {"ch": 32, "tile": "x3hpair"})):
        assert any(matches(e, *want) for e in log), (want, log)
    assert sum(e[1] == "pair" for e in log) == 4 * 9
    log = run(voc, "prod-reflect", "reflect", "default")["log"]
    for s in STAGES:      # per stage: one fill in front of the fork, then per resblock 3 x conv2's and 2 x the later conv1's
        assert sum(e[0] == s and e[1] == "halo" for e in log) == 1 + 3 * 5
    assert sum(e[1] == "halo" for e in log) == 2 + 4 * 16


def test_witnesses_name_forms_that_exist():
    for name, _, gens, wit in SETTINGS:
        assert all(g in R.GENERATORS for g in gens)
        for kind, point, form, _ in wit:
            assert (kind, point, form) in EXPECTED, (name, kind, point, form)


def same_bits(voc, gen, a, b):
    for case in R.GEN_CASES[gen]:
        assert torch.equal(run(voc, gen, case, a)["wav"], run(voc, gen, case, b)["wav"]), f"{gen} {case}: {a} differs from {b}"


def test_fused_pairs_are_bit_identical(voc):
    """hifigan_rows says of the fused pair "Bit-identical; NotSupported keeps the two launches below": the six pair_fuse values
    (the 32-, 64- and 128-channel stages fused or not) leave the same bits."""
    for s in PAIR_FUSE[1:]:
        same_bits(voc, "prod", PAIR_FUSE[0], s)


@pytest.mark.parametrize("gen,setting", [("prod", "voc_streams=1"), ("prod-reflect", "reflect:voc_streams=1")])
def test_streams_do_not_change_a_value(voc, gen, setting):
    same_bits(voc, gen, "default", setting)


def test_loader_address_forms_are_bit_identical(voc):
    """ldr64 = 1 runs the two-launch forms on the x3h window tiles with 64-bit loader addresses: the bits of pair_fuse = 0,
    up_fuse = 0 (tests/test_gpu_kernels.py: the loader address forms agree bit for bit)."""
    same_bits(voc, "prod", "pair_fuse=0,up_fuse=0", "ldr64=1")


def test_unreached_threshold_and_repeated_call_leave_the_same_bits(voc):
    same_bits(voc, "prod", "default", "t_x3h_128=100000")
    for gen in R.GENERATORS:
        for case in R.GEN_CASES[gen]:
            assert torch.equal(run(voc, gen, case, "default")["wav"], run(voc, gen, case, "default", again=True)["wav"]), (gen, case)


def test_no_option_leaks(voc):
    from megatts2_amd import megatts2 as M
    fresh = M.HIFIGAN(*R.generator("wide-tail")).native
    try:
        names = sorted({k for s in SETTINGS for k in s[1]})
        for nat in voc.values():
            assert [nat.get_option(k) for k in names] == [fresh.get_option(k) for k in names]
            nat.form_log_begin()
            assert nat.form_log_end() == []          # nothing is recorded without a call, and end() drops what it returned
    finally:
        fresh.close()


# ---------------------------------------------------------------------------------------------------
# coverage: what the log can emit on these generators, from the call sites of hifigan_rows
EXPECTED = {("voc-pre", "pre", "gemm")}
# the upsampler: two halves anywhere; fused only behind an MRF mean with a stride-2 successor of half the width (stages 2, 3)
EXPECTED |= {(s, "upsample", "halves") for s in STAGES} | {(s, "upsample", "fused") for s in STAGES[2:]}
# the mean of a stage: launch_avg3 anywhere (stage 0: always; 1, 2: up_fuse bit clear; 3: reflect mode, whose output layer is not
# fused), inside the next upsampler (1, 2), inside the output layer (the last stage)
EXPECTED |= {(s, "mean", "avg3") for s in STAGES} | {(s, "mean", "in-upsample") for s in STAGES[1:3]} | {("voc-stage3", "mean", "in-post")}
# pairs: two launches anywhere; fused at 128, 64 and 32 channels (256 has no pair kernel)
EXPECTED |= {(s, "pair", "two") for s in STAGES} | {(s, "pair", "fused") for s in STAGES[1:]}
# the chains of every stage on three streams or one; halo fills at every stage and at both ends (reflect mode)
EXPECTED |= {(s, "streams", n) for s in STAGES for n in ("1", "3")}
EXPECTED |= {(s, "halo", "fill") for s in STAGES + ("voc-pre", "voc-post")}
# the output layer: fused (prod), avg3 + the Cout = 1 GEMM with the tanh epilogue (reflect mode; wide-tail at zero padding)
EXPECTED |= {("voc-post", "post", "fused"), ("voc-post", "post", "gemm")}


def test_every_form_is_reached(voc):
    """The (kind, decision point, form) triples seen over every (generator, case, setting) of this file are exactly EXPECTED; the
    two-launch output layer is reached at zero padding (wide-tail) as well as in reflect mode.  Prints the tables of the docstring."""
    seen, worst, form_worst = set(), {}, {}
    for name, _, gens, _ in SETTINGS:
        for gen in gens:
            for case in R.GEN_CASES[gen]:
                r = judge(voc, gen, case, name)
                w = max(r["ratios"])
                worst[(gen, name)] = max(worst.get((gen, name), 0.0), w)
                # a call's worst frame is booked on the forms that the default run of the same case does not show (a default run: on
                # all of its forms) - the forms the setting brings, not every form that merely took part; tiles likewise
                keys = {(p, f) for _, p, f, _ in r["log"]} | {("tile", a[t].split("_")[0]) for _, _, _, a in r["log"] for t in ("tile", "tile2") if t in a}
                if name != "default":
                    b = run(voc, gen, case, "default")["log"]
                    keys -= {(p, f) for _, p, f, _ in b} | {("tile", a[t].split("_")[0]) for _, _, _, a in b for t in ("tile", "tile2") if t in a}
                for key in keys:
                    key += ("wide-tail" if gen == "wide-tail" else "prod*",)
                    form_worst[key] = max(form_worst.get(key, 0.0), w)
                seen |= form_keys(r["log"])
    print("worst err / E32 per setting; E32 = " + ", ".join(f"{g} {R.e32(g):.2e}" for g in R.GENERATORS))
    for name, *_ in SETTINGS:
        print("    %-30s %s" % (name, "  ".join("%s %5.2f" % (g, worst[(g, name)]) for g in R.GENERATORS if (g, name) in worst)))
    print("worst err / E32 per form and tile: over the default runs, and over the calls of settings that bring it to a case")
    for fam in ("prod*", "wide-tail"):
        print("  " + fam + ":  " + "  ".join("%s %s %.2f" % (p, f, w) for (p, f, g), w in sorted(form_worst.items()) if g == fam))
    assert not EXPECTED - seen, f"never reached: {sorted(EXPECTED - seen)}"
    assert not seen - EXPECTED, f"reached but not expected: {sorted(seen - EXPECTED)}"
    assert ("voc-post", "post", "gemm") in form_keys(run(voc, "wide-tail", "edges", "default")["log"])
