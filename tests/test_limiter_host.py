"""Host side of the true-peak look-ahead limiter (no GPU): the float64 restatement of the rule (tests/limiter_ref.py) against the
properties that define a limiter - s <= need <= 1, s never under the smallest need, s = 1 exactly away from every crest, the sample
peak at or under the ceiling - against ground truth (audio under the ceiling comes back as x G bit for bit) and against the figures
the feature rests on: what one gain under a ceiling reaches on a signal with crests, and what the passes of the limiter reach.  Then
the library's host-only entry points mt2_limiter_query and mt2_limiter_window, the refusals and the exports."""
import ctypes as C
import os

import numpy as np
import pytest

import ebu_ref as E
import limiter_ref as LM
import loudness_ref as R


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


@pytest.mark.parametrize("sr, ms, H", [(16000, 0.0625, 1), (16000, 5.0, 80), (16000, 64.0, 1024), (22050, 5.0, 110), (48000, 5.0, 240)])
def test_window_is_the_restatements_after_one_rounding(rt, sr, ms, H):
    assert LM.half_window(sr, ms) == H and rt.limiter_query(sr, 1, ms)[:2] == (H, LM.TILE)
    got = rt.limiter_window(sr, ms)
    W = 2 * H + 1
    assert got.shape == (W,) and got.dtype == np.float32 and np.array_equal(got, LM.window(H))
    assert (got > 0).all() and np.array_equal(got, got[::-1]) and got.argmax() == H
    total = float(got.astype(np.float64).sum())
    print(f"H {H}: the f32 weights add up to 1 {total - 1.0:+.3g} (bar {W * 2.0 ** -24:.3g})")
    assert abs(total - 1.0) <= W * 2.0 ** -24


def r256(x):
    return max(256, -(-x // 256) * 256)


@pytest.mark.parametrize("sr, L, ms", [(16000, 1, 5.0), (16000, 3000, 5.0), (16000, 80001, 0.0625), (48000, 480000, 5.0), (16000, 48000, 64.0)])
def test_query_is_the_byte_formula(rt, sr, L, ms):
    H, tile, ws = rt.limiter_query(sr, L, ms)
    Wp, Lp = (2 * H + 1 + 3) // 4 * 4, (L + 3) // 4 * 4
    extra = r256(4 * Wp) + 2 * r256(4 * Lp) + r256(64) + r256(12) + r256(144) + r256(64)
    assert (H, tile) == (LM.half_window(sr, ms), 1024) and ws == rt.ebu_query(sr, L)[4] + extra


@pytest.mark.parametrize("sr, L, ms", [(16005, 1000, 5.0), (16000, 0, 5.0), (16000, 2 ** 31, 5.0), (16000, 1000, 0.0), (16000, 1000, 0.03), (16000, 1000, 64.1),
                                       (16000, 1000, float("nan")), (16000, 1000, float("inf")), (16000, 1000, -5.0)])
def test_query_and_window_reject(rt, sr, L, ms):
    with pytest.raises(rt.NativeError):
        rt.limiter_query(sr, L, ms)
    buf = np.zeros(4096, np.float32)
    if L == 1000:
        assert rt.load_library().mt2_limiter_window(sr, ms, buf.ctypes.data_as(C.c_void_p)) != 0 and not buf.any()
    assert rt.load_library().mt2_limiter_window(16000, 5.0, None) != 0 and b"null w" in rt.load_library().mt2_last_error()


def test_calls_refuse_on_the_host_with_a_null_handle(rt):
    """every refusal is decided before the handle is looked at: with a NULL handle and pointers that are never followed, each bad
    argument is named in the error - and the valid call gets as far as the handle"""
    lib = rt.load_library()
    lens = np.array([3000, 3000], np.int32)
    wav, out, gain, need, stats = (C.c_void_p(a) for a in (0x10000, 0x100000, 0x200000, 0x300000, 0x400000))

    def limit(lens=lens, L_max=3000, B=2, sr=16000, pre=6.0, ceiling=-1.0, ms=5.0, wav=wav, out=out, gain=gain, need=need, stats=stats):
        return lib.mt2_limit_true_peak(None, None, wav, rt._iptr(lens), L_max, B, sr, pre, ceiling, ms, out, gain, need, stats)

    def normalize(lens=lens, L_max=3000, B=2, sr=16000, target=-23.0, ceiling=-1.0, ms=5.0, passes=2, wav=wav, out=out, gain=gain, need=need,
                  stats=stats):
        return lib.mt2_loudness_normalize_limited(None, None, wav, rt._iptr(lens), L_max, B, sr, target, ceiling, ms, passes, out, gain, need,
                                                  stats)

    def refused(rc, word):
        assert rc != 0
        msg = lib.mt2_last_error().decode()
        assert word in msg, msg

    for call in (limit, normalize):
        refused(call(), "null model handle")
        refused(call(out=wav, gain=None, need=None, stats=None), "null model handle")          # in place is allowed
        refused(call(B=0), "B outside")
        refused(call(B=65536), "B outside")
        refused(call(lens=np.array([3000, 0], np.int32)), "length outside")
        refused(call(lens=np.array([3001, 3000], np.int32)), "length outside")
        for sr in (7990, 16005, 192010, 0):
            refused(call(sr=sr), "sample_rate")
        refused(call(wav=None), "bad buffers")
        refused(call(out=None), "null out")
        for bad in (float("nan"), float("inf"), -float("inf")):
            refused(call(ceiling=bad), "finite")
            refused(call(ms=bad), "window_ms")
        for ms in (0.0, 0.03, 64.1, -1.0):
            refused(call(ms=ms), "window_ms")
        refused(call(out=C.c_void_p(0x10000 + 4 * 3000)), "out overlaps wav")                   # out's first row is wav's second
        refused(call(out=C.c_void_p(0x10000 + 4)), "out overlaps wav")
        refused(call(gain=wav), "overlapping")                                                  # only out may be wav
        refused(call(need=C.c_void_p(0x100000 + 4 * 5999)), "overlapping")                      # need starts on out's last word
        refused(call(gain=C.c_void_p(0x300000 - 4)), "overlapping")                             # gain's last word is need's first
        refused(call(stats=C.c_void_p(0x200000 + 64)), "overlapping")
        refused(call(stats=C.c_void_p(0x10000 + 4 * 6000 - 8)), "overlapping")
        refused(call(stats=C.c_void_p(0x400000 + 4)), "misaligned")
        refused(call(gain=C.c_void_p(0x200000 + 2)), "misaligned")
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(limit(pre=bad), "pre_gain_db")
        refused(normalize(target=bad), "finite")
    refused(limit(pre=800.0), "pre-gain")
    refused(limit(pre=-2000.0), "pre-gain")
    for passes in (0, 5, -1):
        refused(normalize(passes=passes), "passes")
    for passes in (1, 4):
        refused(normalize(passes=passes), "null model handle")


def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_limiter_query", "mt2_limiter_window", "mt2_limit_true_peak", "mt2_loudness_normalize_limited"):
        assert hasattr(lib, name) and name in header
    assert f"MT2_LIMITER_FIELDS {rt.LIMITER_FIELDS}" in header and rt.LIMITER_FIELDS == LM.FIELDS == 24
    assert f"MT2_LIMITER_TILE {rt.LIMITER_TILE}" in header and f"MT2_LIMITER_MAX_HALF_WINDOW {rt.LIMITER_MAX_HALF_WINDOW}" in header
    assert f"MT2_LIMITER_MAX_PASSES {rt.LIMITER_MAX_PASSES}" in header and (rt.LIMITER_TILE, rt.LIMITER_MAX_HALF_WINDOW, rt.LIMITER_MAX_PASSES) == (LM.TILE, LM.MAX_H, LM.MAX_PASSES)
    for word in ("look-ahead", "0.5 - 0.5 cos", "rounded toward zero", "unpinned"):
        assert word in header
    import inspect
    from megatts2_amd import megatts2
    assert inspect.signature(rt.MelFrontEnd.loudness_normalize).parameters["limiter"].default is None
    assert inspect.signature(megatts2.Megatts.synthesize).parameters["limiter"].default is None
    assert inspect.signature(megatts2.Megatts.forward).parameters["limiter"].default is None
    assert callable(rt.MelFrontEnd.limit) and callable(megatts2.limit_true_peak)
    lim = rt.Limiter()
    assert (lim.window_ms, lim.passes) == (5.0, 2)


# ---- the restatement: properties, ground truth and the figures ---------------------------------------------------------------------------

@pytest.mark.parametrize("H", [1, 16, 80])
@pytest.mark.parametrize("G", [1.3, 1.9, 4.5])
def test_properties_on_the_pulse_signal(H, G):
    x = LM.pulse_signal()
    r = LM.limit(x, 16000, np.float32(G), -1.0, H)
    s, need, c = r["s"], r["need"], float(LM.ceiling(-1.0))
    limited = np.flatnonzero(need < 1.0)
    assert limited.size >= 19 and (s <= need).all() and (need <= 1.0).all()
    assert s.min() >= need.min() - (2 * H + 1) * 2.0 ** -24                                   # d <= (1 - min need) sum w, and the f32 weights add up to 1 within W 2^-24
    far = np.ones(x.size, bool)
    for i in limited:
        far[max(0, i - 2 * H):i + 2 * H + 1] = False
    assert far.any() and (s[far] == 1.0).all()                                                # exactly 1 outside 2 H of any need < 1
    near = ~far
    print(f"H {H} G {G}: {limited.size} samples need a gain, {int((s < 1).sum())} get one ({(s < 1).mean():.4f} of all), min s {s.min():.4f}, "
          f"min need {need.min():.4f}; sample peak of step 5 {E.db(np.abs(r['out']).max()):.4f} dBFS")
    assert (s < 1).sum() <= near.sum() and (s < 1).mean() < 0.08
    assert np.abs(r["out"]).max() <= c * (1.0 + 2.0 ** -50)                                                    # s <= need: no sample over the ceiling
    assert np.abs(r["out"].astype(np.float32)).max() <= c


def test_audio_under_the_ceiling_comes_back_as_x_g_bit_for_bit():
    x = LM.pulse_signal()[:20000]
    tp = E.true_peak(x, 16000)
    G = np.float32(0.98 * float(LM.ceiling(-1.0)) / tp)                                       # G TP <= c under a margin of 2 %
    p = LM.one_pass(x, 16000, G, -1.0, 80)
    assert p["limited"] == 0 and p["min_s"] == 1.0 and p["t"] == 1.0 and (p["need"] == 1.0).all()
    assert np.array_equal(p["out"].view(np.uint32), (x * G).view(np.uint32))
    over = LM.one_pass(x, 16000, np.float32(1.02 * float(LM.ceiling(-1.0)) / tp), -1.0, 80)  # 2 % over: the largest crest alone
    assert 0 < over["limited"] <= 4 * (4 * 80 + 3) and over["min_s"] >= 1 / 1.0201


@pytest.mark.parametrize("target", [-23.0, -16.0])
def test_figures_of_the_pulse_signal(target):
    """one gain under -1 dBTP stops 3.7 LU under a -23 LUFS target; three passes of the limiter at H = 80 reach it"""
    c = float(LM.ceiling(-1.0))
    g, reached = LM.pulse_one_gain(target)
    print(f"target {target}: one gain {float(g):.5f} under -1 dBTP reaches {reached:.4f} LUFS")
    assert abs(reached - (-26.70)) <= 0.005                                                   # the cap binds at either target
    res = LM.pulse_case(target)
    errs = [abs(p["I"] - target) for p in res]
    for k, p in enumerate(res):
        print(f"  pass {k + 1}: G {float(p['G']):.5f}, {p['I']:.4f} LUFS ({errs[k]:.4f} LU off), true peak before the trim {E.db(p['tp']):+.6f} dBTP, "
              f"t {float(p['t']):.8f}, min s {p['min_s']:.4f}, {p['limited'] / p['s'].size:.4f} of the samples limited")
        assert abs(E.db(p["tp"] / c)) <= 1e-3 and 0.9999 <= float(p["t"]) <= 1.0
        assert p["limited"] < 0.08 * p["s"].size
    assert errs[0] > errs[1] > errs[2] and errs[2] <= LM.REACHED_BAR
    if target == -23.0:
        assert [round(e, 2) for e in errs] == [0.85, 0.13, 0.02] and abs(errs[2] - LM.REACHED_READING) <= 1e-3
        assert 2 * LM.REACHED_READING == LM.REACHED_BAR
    tp = E.true_peak(res[-1]["out"], 16000)
    print(f"  final true peak {E.db(tp):+.7f} dBTP")
    assert tp <= c * (1.0 + 4.0 * float(np.abs(E.table(16000).astype(np.float64)).sum(axis=1).max()) * 2.0 ** -24)


def test_short_and_silent_utterances_are_copied():
    for x in (LM.pulse_signal()[:6000], np.zeros(16000, np.float32)):
        res = LM.normalize(x, 16000, -23.0, -1.0, 80, 3)
        assert len(res) == 1 and np.array_equal(res[0]["out"], x) and res[0]["G"] == 1.0
