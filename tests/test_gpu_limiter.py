"""True-peak look-ahead limiter on the GPU (csrc/limiter.hip: mt2_limit_true_peak, mt2_loudness_normalize_limited) against the float64
restatement of the rule (tests/limiter_ref.py) applied to the same f32 input, against the properties that hold exactly whatever the
rounding (s <= need, s = 1 away from every crest), against ground truth (audio under the ceiling comes back as x G) and on the tiny
synthetic model.

Bars.  need: limiter_ref.need_bound - E carries the error of one f32 fma chain of 24 terms (ebu_ref.chain_bound), the product G E and
the division c / a one rounding each, and need falls from 1 with a slope of at most 1 / c, continuously.  s: within (W + 4) 2^-24
(limiter_ref.smooth_bound) of the float64 smoothing of the DEVICE's own need - the hold is a minimum, hence exact, and the chain has
W terms in [0, 1] under weights that add up to 1.  The ceiling: the true peak re-measured by loudness_ebu is at or under c times
1 + 4 max_p sum_k |h| 2^-24, the margin of the one-gain call.  The loudness reached by three passes: limiter_ref.REACHED_BAR, twice what
the restatement itself reads.

Both kernels take T = 1024 samples a workgroup, tile t holding i in [T t, T (t + 1)); the gain kernel reads need over a halo of 2 H on
each side.  Input padding beyond lens[b] is NaN, outputs are pre-filled with a sentinel, wider than needed, with guard words behind."""
import functools

import numpy as np
import pytest

import ebu_ref as E
import limiter_ref as LM
import loudness_ref as R
from conftest import synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = -77.25
T, NF = LM.TILE, LM.FIELDS
MS = {1: 0.0625, 80: 5.0, 1024: 64.0}              # window_ms of a half window at 16 kHz


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def tp_margin(sr):
    return 1.0 + 4.0 * float(np.abs(E.table(sr).astype(np.float64)).sum(axis=1).max()) * 2.0 ** -24


@functools.lru_cache(maxsize=None)
def noise(L, seed=0):
    x = (0.3 * np.random.default_rng(91 * seed + L).standard_normal(L)).astype(np.float32)
    x.flags.writeable = False
    return x


def run(rows, pre_gain_db=0.0, ceiling=-1.0, ms=5.0, sr=16000, target=None, passes=2, extra_L=7, slots=None, in_place=False, fe=None,
        want_gain=True, want_need=True, want_stats=True):
    """the C entry point (mt2_limit_true_peak, or mt2_loudness_normalize_limited with a target) on the utterances `rows` as one batch
    (slots: the batch row of each; rows without one hold a 1-sample utterance) -> dict of out, gain, need [B, Lw] and stats [B, 24] for
    the rows, the guard words behind each checked"""
    from megatts2_amd import runtime as rt
    fe = fe or frontend()
    slots = list(range(len(rows))) if slots is None else slots
    B = max(slots) + 1
    lens = np.ones(B, np.int32)
    for s, r in zip(slots, rows):
        lens[s] = r.size
    Lw = int(lens.max()) + extra_L
    wav = np.full((B, Lw), np.nan, np.float32)
    wav[:, 0] = 0.25
    for s, r in zip(slots, rows):
        wav[s, :r.size] = r
    bufs = {k: torch.full((B * Lw + 11,), SENT, device="cuda", dtype=torch.float32) for k in ("out", "gain", "need")}
    st = torch.full((B * NF + 5,), SENT, device="cuda", dtype=torch.float64)
    out = bufs["out"][:B * Lw].view(B, Lw)
    if in_place:
        out.copy_(dev(wav))
    x = out if in_place else dev(wav)
    tail = (rt._ptr(out), rt._ptr(bufs["gain"] if want_gain else None), rt._ptr(bufs["need"] if want_need else None),
            rt._ptr(st if want_stats else None))
    if target is None:
        rt._check(fe.lib.mt2_limit_true_peak(fe.h, rt._stream(), rt._ptr(x), rt._iptr(lens), Lw, B, sr, float(pre_gain_db), float(ceiling),
                                             float(ms), *tail))
    else:
        rt._check(fe.lib.mt2_loudness_normalize_limited(fe.h, rt._stream(), rt._ptr(x), rt._iptr(lens), Lw, B, sr, float(target), float(ceiling),
                                                        float(ms), int(passes), *tail))
    res = {}
    for k, b in bufs.items():
        a = b.cpu().numpy()
        assert (a[B * Lw:] == np.float32(SENT)).all()
        res[k] = a[:B * Lw].reshape(B, Lw)[slots]
    s = st.cpu().numpy()
    assert (s[B * NF:] == SENT).all()
    res["stats"] = s[:B * NF].reshape(B, NF)[slots]
    assert want_gain or (res["gain"] == np.float32(SENT)).all()
    assert want_need or (res["need"] == np.float32(SENT)).all()
    assert want_stats or (res["stats"] == SENT).all()
    for b, r in enumerate(rows):                                                              # behind every utterance: zeros, and ones
        assert not res["out"][b, r.size:].any()
        assert not want_gain or (res["gain"][b, r.size:] == 1.0).all()
        assert not want_need or (res["need"][b, r.size:] == 1.0).all()
    return res


def meter(rows, sr=16000):
    """loudness_ebu's rows [B, 18] of the utterances"""
    B, lens = len(rows), np.asarray([r.size for r in rows], np.int32)
    wav = np.zeros((B, int(lens.max())), np.float32)
    for b, r in enumerate(rows):
        wav[b, :r.size] = r
    return frontend().loudness_ebu(dev(wav), lens, sample_rate=sr).cpu().numpy()


def test_constants_are_the_librarys():
    from megatts2_amd import runtime as rt
    assert rt.limiter_query(16000, 48000)[:2] == (80, T) and rt.LIMITER_FIELDS == NF and rt.LIMITER_TILE == T


def check_need(x, sr, G, ceiling, need, note=""):
    want = LM.need_of(LM.envelope(x, sr), G, LM.ceiling(ceiling))
    bar = LM.need_bound(sr, np.abs(x).max(), G, ceiling)
    err = float(np.abs(need[:x.size] - want).max())
    print(f"{note}sr {sr} L {x.size}: {int((want < 1).sum())} samples need a gain, min {want.min():.4f}; worst need error / bar {err / bar:.3g}")
    assert err <= bar
    return err / bar


def check_hold(need, gain, H, L, note=""):
    """what holds exactly, and the smoothing of the device's own need"""
    need, gain = need[:L], gain[:L]
    assert (gain <= need).all() and (need <= 1.0).all()                                      # bit-wise: f32 against f32
    far = np.convolve((need < 1.0).astype(np.float64), np.ones(4 * H + 1), mode="same") < 0.5 if L > 4 * H else \
        np.full(L, not (need < 1.0).any())
    assert (gain[far] == 1.0).all()                                                           # exactly 1 where need is 1 over +- 2 H
    want = LM.smooth(need.astype(np.float64), H)
    err = float(np.abs(gain - want).max())
    print(f"{note}H {H} L {L}: {int((gain < 1).sum())} samples with s < 1, {int(far.sum())} held to exactly 1; worst s error / bar {err / LM.smooth_bound(H):.3g}")
    assert err <= LM.smooth_bound(H)


def check_out(x, G, res, b, t=None):
    """out = ((x G) s) t, f32 products"""
    L = x.size
    t = np.float32(res["stats"][b, 22]) if t is None else t
    want = (x * np.float32(G)) * res["gain"][b, :L]
    if t != 1.0:
        want = want * t
    assert np.array_equal(bits(res["out"][b, :L]), bits(want))


def gain_of(db):
    return np.float32(10.0 ** (db / 20.0))


# ---- envelope and need ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("sr", [16000, 22050, 48000])
def test_need_against_restatement(sr):
    """noise with a fifth of its samples over the ceiling, at lengths around the tile, as one ragged batch"""
    H = LM.half_window(sr)
    rows = [noise(L, 1) for L in (1, 2, 24, T - 1, T, T + 1, 2 * T + 3, 5000)]
    res = run(rows, 10.0, -1.0, 5.0, sr)
    G = gain_of(10.0)
    worst = max(check_need(x, sr, G, -1.0, res["need"][b]) for b, x in enumerate(rows))
    print(f"sr {sr}: worst need error / bar {worst:.3g}")
    for b, x in enumerate(rows):
        check_hold(res["need"][b], res["gain"][b], H, x.size)
        check_out(x, G, res, b)
        assert res["stats"][b, 18] == H and res["stats"][b, 7] == float(G)
        s = res["gain"][b, :x.size]
        assert res["stats"][b, 19] == float(s.min()) and res["stats"][b, 20] == int((s < 1).sum())


# ---- the edges of the tile and of the halo ------------------------------------------------------------------------------------------------

def pulse_row(L, p, seed):
    x = 0.01 * noise(L, seed).copy()
    x[p] = 0.9
    return x.astype(np.float32)


@pytest.mark.parametrize("H", [1, 80, 1024])
def test_edges_of_the_tile_and_of_the_halo(H):
    """lengths around the window and the tile, and a lone crest where the tile and its halo end: with Bd the first tile boundary
    beyond 2 H, the crest's last sample on Bd - 2 H (the first word of the halo of the tile that starts at Bd) and its first on
    Bd - 1 + 2 H (the last word of the halo of the tile that ends there), on the last sample of a tile and the first of the next, and
    on samples 0 and L - 1"""
    ms, G, c = MS[H], gain_of(6.0), float(LM.ceiling(-1.0))
    Bd = T * (2 * H // T + 1)
    L = Bd + 2 * H + 40
    ref = LM.need_of(LM.envelope(pulse_row(4096, 2048, 5), 16000), G, c)
    at = np.flatnonzero(ref < 1.0)
    lo, hi = int(at.min()) - 2048, int(at.max()) - 2048                                        # the samples a crest at p asks a gain for: p + lo .. p + hi
    assert -2 <= lo <= 0 <= hi <= 2
    cases = [(Bd - 2 * H - hi, "last", Bd - 2 * H), (Bd - 1 + 2 * H - lo, "first", Bd - 1 + 2 * H), (Bd - 1, "at", Bd - 1), (Bd, "at", Bd),
             (0, "at", 0), (L - 1, "at", L - 1)]
    rows = []
    for k, (p, how, where) in enumerate(cases):
        x = pulse_row(L, p, 7 + k)
        env = LM.envelope(x, 16000)
        need = LM.need_of(env, G, c)
        at = np.flatnonzero(need < 1.0)
        assert need.min() < 0.6 and (float(G) * env[need == 1.0] < 0.5 * c).all()          # the test's own aim: a clear crest, nothing else near the ceiling
        assert {"last": at.max(), "first": at.min(), "at": p}[how] == where and at.min() <= p <= at.max(), (at, where)
        rows.append(x)
    rows += [noise(n, 2) for n in (1, H, H + 1, 2 * H + 1, T - 1, T, T + 1, 2 * T + 3)]
    res = run(rows, 6.0, -1.0, ms)
    for b, x in enumerate(rows):
        check_need(x, 16000, G, -1.0, res["need"][b], f"row {b}: ")
        check_hold(res["need"][b], res["gain"][b], H, x.size, f"row {b}: ")
        check_out(x, G, res, b)
    for b, (p, how, where) in enumerate(cases[:2]):                                           # the crest reaches across the boundary, as far as the rule says and no further
        s = res["gain"][b]
        reach = np.flatnonzero(LM.smooth(res["need"][b, :L].astype(np.float64), H) < 1.0 - 4 * LM.smooth_bound(H))
        assert reach.size and (s[reach] < 1.0).all()
        if H == 1:
            assert (s[Bd] < 1.0) if how == "last" else (s[Bd - 1] < 1.0)                      # through the one outermost word of the halo
    alone = run(rows[:2], 6.0, -1.0, ms)
    for k in ("out", "gain", "need"):
        assert np.array_equal(bits(alone[k][:, :L]), bits(res[k][:2, :L]))


# ---- the ceiling and the loudness reached -------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def parent_reaches():
    """the one-gain call under -1 dBTP on the pulse signal, to -23 LUFS: (gain, loudness reached)"""
    x = LM.pulse_signal()
    out, st = frontend().loudness_normalize(dev(x[None]), None, -23.0, return_stats=True, true_peak_ceiling_dbtp=-1.0)
    return float(st[0, 7]), float(meter([out[0].cpu().numpy()])[0, 0])


@pytest.mark.parametrize("target", [-23.0, -16.0])
def test_pulse_signal_reaches_the_target_under_the_ceiling(target):
    x = LM.pulse_signal()
    c = float(LM.ceiling(-1.0))
    res = run([x], ceiling=-1.0, target=target, passes=3)
    st, out = res["stats"][0], res["out"][0, :x.size]
    back = meter([out])[0]
    ref = LM.pulse_case(target)[-1]
    print(f"target {target}: field 23 {st[23]:.6f} LUFS (restatement {ref['I']:.6f}), re-measured {back[0]:.6f} LUFS, true peak {E.db(back[8]):+.6f} dBTP "
          f"({back[8] / c - 1:+.3g} of the ceiling, room {tp_margin(16000) - 1:.3g}); G {st[7]:.5f} (restatement {float(ref['G']):.5f}), min s {st[19]:.4f}, "
          f"{st[20] / x.size:.4f} of the samples limited, TP' {E.db(st[21]):+.6f} dBTP, t {st[22]:.8f}")
    assert back[8] <= c * tp_margin(16000)                                                    # the ceiling holds, by the parent's margin
    assert abs(st[23] - back[0]) <= 1e-8
    assert abs(st[23] - target) <= LM.REACHED_BAR
    assert abs(E.db(st[21] / c)) <= 1e-3 and 0.9999 <= st[22] <= 1.0 and st[20] < 0.08 * x.size and st[18] == 80
    want = meter([x])[0]
    assert np.array_equal(bits64(np.delete(st[:18], 7)), bits64(np.delete(want, 7)))          # the meter's row of the INPUT
    check_hold(res["need"][0], res["gain"][0], 80, x.size)
    check_out(x, np.float32(st[7]), res, 0)
    g, reached = parent_reaches()
    ref_g, ref_reached = LM.pulse_one_gain(-23.0)
    print(f"one gain under -1 dBTP: {g:.6f}, reaches {reached:.4f} LUFS (restatement {float(ref_g):.6f}, {ref_reached:.4f})")
    assert abs(reached - (-26.70)) <= 0.005                                                   # what the limiter is for
    assert st[23] > reached + 3.0


def test_passes_close_in_on_the_target():
    x = LM.pulse_signal()
    errs = [abs(run([x], target=-23.0, passes=P, want_gain=False, want_need=False)["stats"][0, 23] + 23.0) for P in (1, 2, 3, 4)]
    print("error after 1 .. 4 passes:", errs)
    assert errs[0] > errs[1] > errs[2] and errs[3] <= errs[2] + 1e-3
    assert [round(e, 2) for e in errs[:3]] == [0.85, 0.13, 0.02]                              # the figures of the host test


# ---- nothing to do --------------------------------------------------------------------------------------------------------------------------

def test_audio_under_the_ceiling_comes_back_as_x_g():
    rows = [LM.pulse_signal()[:20000], noise(T + 5, 3), noise(1, 4)]
    tp = max(E.true_peak(x, 16000) for x in rows)
    db = 20.0 * np.log10(0.98 * float(LM.ceiling(-1.0)) / tp)
    G = gain_of(db)
    res = run(rows, db, -1.0)
    for b, x in enumerate(rows):
        st = res["stats"][b]
        assert np.array_equal(bits(res["out"][b, :x.size]), bits(x * G))
        assert st[20] == 0 and st[19] == 1.0 and st[22] == 1.0 and st[7] == float(G)
        assert (res["gain"][b] == 1.0).all() and (res["need"][b] == 1.0).all()
        assert st[21] <= float(LM.ceiling(-1.0)) and abs(st[21] - float(G) * E.true_peak(x, 16000)) <= 2 * float(G) * E.chain_bound(16000, np.abs(x).max())
    norm = run(rows, target=-30.0, passes=2)                                                  # the pulse signal at -30 LUFS is far under the ceiling
    st = norm["stats"]
    assert st[0, 20] == 0 and st[0, 22] == 1.0 and abs(st[0, 23] + 30.0) <= 1e-4
    assert np.array_equal(bits(norm["out"][0, :20000]), bits(rows[0] * np.float32(st[0, 7])))
    for b in (1, 2):                                                                          # under 0.4 s: copied unchanged
        assert st[b, 7] == 1.0 and st[b, 20] == 0 and np.array_equal(bits(norm["out"][b, :rows[b].size]), bits(rows[b]))
        assert not np.isfinite(st[b, 23])


# ---- the batch, the refusals, the arena --------------------------------------------------------------------------------------------------

def ragged_rows():
    return [noise(1, 6), noise(7000, 6), LM.pulse_signal()[:30000], noise(2 * T + 3, 6)]


def same(a, b, rows):
    for k in ("out", "gain", "need"):
        for r, x in enumerate(rows):
            assert np.array_equal(bits(a[k][r, :x.size]), bits(b[k][r, :x.size])), (k, r)
    assert np.array_equal(bits64(a["stats"]), bits64(b["stats"]))


@pytest.mark.parametrize("target", [None, -8.0])
def test_ragged_batch_is_its_utterances_alone(target):
    rows = ragged_rows()
    kw = dict(pre_gain_db=9.0, target=target, passes=2)
    first = run(rows, **kw)
    for other in (run(rows, **kw), run(rows, extra_L=7 + 13, **kw), run(rows, slots=[4, 2, 0, 1], **kw)):      # again; another L_max; other slots, a stranger
        same(first, other, rows)
    for b, r in enumerate(rows):
        alone = run([r], **kw)
        same({k: v[b:b + 1] for k, v in first.items()}, alone, [r])
    inp = run(rows, in_place=True, **kw)                                                      # out is wav: the same bits
    same(first, inp, rows)
    quiet = run(rows, want_gain=False, want_need=False, want_stats=False, **kw)              # the optional outputs change nothing
    for r, x in enumerate(rows):
        assert np.array_equal(bits(quiet["out"][r, :x.size]), bits(first["out"][r, :x.size]))
    assert (first["stats"][1:3, 20] > 0).all()                                                # the two utterances over 0.4 s are limited in either form


def test_non_finite_sample_changes_its_own_utterance_only():
    clean = LM.pulse_signal()[:30000]
    bad, worse = clean.copy(), clean.copy()
    bad[9000], worse[20000] = np.nan, np.inf
    for kw in (dict(pre_gain_db=6.0), dict(target=-16.0, passes=2)):
        res = run([clean, bad, worse, clean[:12000]], **kw)
        same({k: v[0:1] for k, v in res.items()}, run([clean], **kw), [clean])
        same({k: v[3:4] for k, v in res.items()}, run([clean[:12000]], **kw), [clean[:12000]])
    res = run([clean, bad, worse], pre_gain_db=6.0)
    far = np.ones(30000, bool)
    far[9000 - 12 - 2 * 80 - 1:9000 + 12 + 2 * 80 + 2] = False                                # the interpolator's window and the limiter's reach
    assert np.array_equal(bits(res["gain"][1, :30000][far]), bits(res["gain"][0, :30000][far])) and np.isnan(res["out"][1, 9000])
    assert res["need"][2, 20000] == 0.0 and res["stats"][2, 19] <= 0.0                        # an Inf wins the envelope: the gain goes to 0


def test_calls_refuse_before_launch():
    """each case is refused on the host: nothing is launched and every output keeps its sentinel"""
    from megatts2_amd import runtime as rt
    fe = frontend()
    base = torch.full((9000,), SENT, device="cuda", dtype=torch.float32)
    x = base[:6000].view(2, 3000)
    x.copy_(dev(np.stack([noise(3000, 7), noise(3000, 8)])))
    keep = x.clone()
    st = torch.full((2 * NF,), SENT, device="cuda", dtype=torch.float64)
    out, gain, need = (torch.full((2, 3000), SENT, device="cuda", dtype=torch.float32) for _ in range(3))

    def untouched():
        torch.cuda.synchronize()
        assert (st == SENT).all() and (out == SENT).all() and (gain == SENT).all() and (need == SENT).all() and torch.equal(x, keep)
        assert (base[6000:] == SENT).all()

    def refuse(lens=(3000, 3000), B=2, sr=16000, pre=6.0, target=-23.0, ceiling=-1.0, ms=5.0, passes=2, o=out, g=gain, n=need, s=st, both=True):
        ln = np.asarray(lens, np.int32)
        with pytest.raises(rt.NativeError):
            rt._check(fe.lib.mt2_loudness_normalize_limited(fe.h, rt._stream(), rt._ptr(x), rt._iptr(ln), 3000, B, sr, target, ceiling, ms, passes,
                                                            rt._ptr(o), rt._ptr(g), rt._ptr(n), rt._ptr(s)))
        untouched()
        if both:
            with pytest.raises(rt.NativeError):
                rt._check(fe.lib.mt2_limit_true_peak(fe.h, rt._stream(), rt._ptr(x), rt._iptr(ln), 3000, B, sr, pre, ceiling, ms, rt._ptr(o),
                                                     rt._ptr(g), rt._ptr(n), rt._ptr(s)))
            untouched()

    refuse(lens=(3000, 0))
    refuse(lens=(3001, 3000))
    refuse(B=0)
    for sr in (7990, 16005, 192010):
        refuse(sr=sr)
    for bad in (float("nan"), float("inf")):
        refuse(ceiling=bad)
        refuse(ms=bad)
        refuse(target=bad, pre=bad)
    for ms in (0.0, 0.03, 64.1):
        refuse(ms=ms)
    for passes in (0, 5):
        refuse(passes=passes, both=False)
    refuse(o=None)
    refuse(o=base[3000:9000].view(2, 3000))                                                   # out's first row is wav's second
    refuse(o=base[1:6001].view(2, 3000))
    refuse(g=x)
    refuse(n=out)
    refuse(g=need)
    with pytest.raises(ValueError):
        fe.loudness_normalize(x, None, -23.0, limiter=rt.Limiter())                           # a limiter without a ceiling to hold
    with pytest.raises(ValueError):
        fe.loudness_normalize(x, None, -23.0, 0.9, true_peak_ceiling_dbtp=-1.0, limiter=rt.Limiter())
    untouched()
    rt._check(fe.lib.mt2_loudness_normalize_limited(fe.h, rt._stream(), rt._ptr(x), rt._iptr(np.asarray([3000, 3000], np.int32)), 3000, 2, 16000,
                                                    -23.0, -1.0, 5.0, 2, rt._ptr(out), rt._ptr(gain), rt._ptr(need), rt._ptr(st)))      # and the valid call goes through
    torch.cuda.synchronize()
    assert (st != SENT).all() and (out != SENT).all() and (gain == 1.0).all() and torch.equal(out, keep)      # under 0.4 s: copied


def test_arena_high_water_is_the_querys_figure():
    from megatts2_amd import runtime as rt
    fe = rt.MelFrontEnd()
    try:
        for L, ms in ((3000, 5.0), (30003, 0.0625), (30003, 64.0), (48000, 5.0)):      # ascending: the high water never falls
            x = LM.pulse_signal()[:L]
            run([x], 6.0, ms=ms, fe=fe)
            assert fe.workspace_high_water() == rt.limiter_query(16000, L, ms)[2]
        for P in (1, 4):
            run([LM.pulse_signal()[:48000]], target=-20.0, passes=P, fe=fe)
            assert fe.workspace_high_water() == rt.limiter_query(16000, 48000, 5.0)[2] > rt.ebu_query(16000, 48000)[4]
    finally:
        fe.close()


def test_stage_events_name_the_kernels():
    fe = frontend()
    fe.set_profiling(True)
    try:
        meter_marks = ["loud_zero_state", "loud_carry", "loud_sums", "loud_gate", "ebu_true_peak", "ebu_range", "lim_envelope"]
        run([LM.pulse_signal()[:48000]], target=-20.0, passes=2)
        assert list(fe.last_stage_ms()) == meter_marks + ["lim_gain1", "lim_trim1", "lim_measure1", "lim_gain2", "lim_trim2", "lim_measure2"]
        run([LM.pulse_signal()[:48000]], target=-20.0, passes=2, want_stats=False)
        assert list(fe.last_stage_ms()) == meter_marks + ["lim_gain1", "lim_trim1", "lim_measure1", "lim_gain2", "lim_trim2"]
        run([LM.pulse_signal()[:48000]], 6.0, want_stats=False)
        assert list(fe.last_stage_ms()) == meter_marks + ["lim_gain1", "lim_trim1"]
    finally:
        fe.set_profiling(False)


def test_frontend_methods_are_the_entry_points():
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime as rt
    fe = frontend()
    rows = [LM.pulse_signal()[:40000], noise(9000, 9)]
    wav = np.zeros((2, 40000), np.float32)
    wav[0], wav[1, :9000] = rows[0], rows[1]
    lens = [40000, 9000]
    want = run(rows, 8.0, -2.0, 2.5)
    out, st, gain, need = fe.limit(dev(wav), lens, 8.0, -2.0, 2.5, return_stats=True, return_gain=True, return_need=True)
    assert st.shape == (2, NF) and st.dtype == torch.float64 and np.array_equal(bits64(st.cpu().numpy()), bits64(want["stats"]))
    for got, k in ((out, "out"), (gain, "gain"), (need, "need")):
        assert np.array_equal(bits(got.cpu().numpy()), bits(want[k][:, :40000]))
    assert torch.equal(fe.limit(dev(wav), lens, 8.0, -2.0, 2.5), out)
    y, d = M.limit_true_peak(wav[0], pre_gain_db=8.0, ceiling_dbtp=-2.0, window_ms=2.5)
    assert np.array_equal(bits(y), bits(want["out"][0, :40000])) and d["samples_limited"][0] == want["stats"][0, 20] and d["half_window"][0] == 40
    assert d["min_gain"][0] == want["stats"][0, 19] and d["gain"][0] == want["stats"][0, 7] and d["output_lufs"][0] == want["stats"][0, 23]
    norm = run(rows, ceiling=-1.0, target=-16.0, passes=3)
    out, st = fe.loudness_normalize(dev(wav), lens, -16.0, return_stats=True, true_peak_ceiling_dbtp=-1.0, limiter=rt.Limiter(5.0, 3))
    assert np.array_equal(bits(out.cpu().numpy()), bits(norm["out"][:, :40000])) and np.array_equal(bits64(st.cpu().numpy()), bits64(norm["stats"]))
    today = fe.loudness_normalize(dev(wav), lens, -16.0, true_peak_ceiling_dbtp=-1.0)
    none = fe.loudness_normalize(dev(wav), lens, -16.0, true_peak_ceiling_dbtp=-1.0, limiter=None)      # None: today's call, today's bits
    assert torch.equal(today.view(torch.int32), none.view(torch.int32)) and not torch.equal(today, out)


# ---- the model: tiny synthetic weights ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny_tts(with_hifigan):
    from megatts2_amd import megatts2 as M
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    return M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)), hifi_gan=M.HIFIGAN(h, sd_h) if with_hifigan else None), g


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifigan"])
def test_synthesize_with_a_limiter(vocoder):
    from megatts2_amd import megatts2 as M
    tts, g = tiny_tts(vocoder == "hifigan")
    rng = np.random.default_rng(21)
    B, Np, Tp = 3, 8, 24
    phone = dev(rng.integers(0, g.mrte.phone_vocab_size, (B, Np)).astype(np.int64))
    mels = dev((0.5 * rng.standard_normal((B, Tp, 80)) - 4.0).astype(np.float32))
    dur = np.asarray([[6] * 8, [4, 5, 4, 5, 4, 5, 4, 5], [2] * 8], np.int32)                # 48, 36 and 16 frames: the last is under 0.4 s
    kw = dict(forced_durations=dur, return_aux=True)
    kw.update({"griffin_lim": {"n_iter": 3, "seeds": 5}} if vocoder == "griffin_lim" else {"vocoder": True})
    raw = tts.synthesize(phone, mels, **kw)
    one = tts.synthesize(phone, mels, loudness_lufs=0.0, true_peak_ceiling_dbtp=-1.0, **kw)
    none = tts.synthesize(phone, mels, loudness_lufs=0.0, true_peak_ceiling_dbtp=-1.0, limiter=None, **kw)      # None: today's path, today's bits
    assert torch.equal(one[2]["wav"].view(torch.int32), none[2]["wav"].view(torch.int32)) and "limiter_stats" not in none[2]
    mel, lens, aux = tts.synthesize(phone, mels, loudness_lufs=0.0, true_peak_ceiling_dbtp=-1.0, limiter=M.Limiter(), **kw)
    assert torch.equal(mel, raw[0]) and np.array_equal(lens, raw[1]) and aux["limiter_stats"].shape == (B, NF)
    n = (np.asarray(lens) - 1) * 256 if vocoder == "griffin_lim" else np.asarray(lens) * 256
    before = M.measure_loudness(one[2]["wav"], 16000, lens=n, ebu=True)
    after = M.measure_loudness(aux["wav"], 16000, lens=n, ebu=True)
    print(f"{vocoder} to 0 LUFS under -1 dBTP: one gain {before['integrated_lufs']} LUFS, with the limiter {after['integrated_lufs']} LUFS, "
          f"true peaks {after['true_peak_dbtp']} dBTP; limited {aux['limiter_stats'][:, 20].cpu().numpy()} samples")
    ceiling = 10.0 ** (-1.0 / 20.0)
    for b in range(2):
        assert after["true_peak"][b] <= ceiling * tp_margin(16000)
        assert after["integrated_lufs"][b] > before["integrated_lufs"][b]                     # strictly above what one gain reaches
    assert not np.isfinite(after["integrated_lufs"][2])                                       # under 0.4 s: left as it was
    k = int(n[2])
    assert torch.equal(aux["wav"][2, :k].view(torch.int32), raw[2]["wav"][2, :k].view(torch.int32))
    with pytest.raises(ValueError):
        tts.synthesize(phone, mels, loudness_lufs=0.0, limiter=M.Limiter(), **kw)             # a limiter without a ceiling to hold


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifigan"])
def test_forward_with_a_limiter_keeps_both_parts_of_the_file_under_the_ceiling(tmp_path, vocoder):
    from megatts2_amd import audio_io
    from megatts2_amd import megatts2 as M
    tts, g = tiny_tts(vocoder == "hifigan")
    wavs = tmp_path / "prompts"
    wavs.mkdir()
    x = 0.05 * noise(16000, 11) / np.abs(noise(16000, 11)).max()
    audio_io.write_wav(str(wavs / "p.wav"), x, 16000)
    phone = np.random.default_rng(22).integers(0, g.mrte.phone_vocab_size, 40)             # 40 phones of at least one frame: over 0.4 s
    kw = {"vocoder": {"n_iter": 2}} if vocoder == "griffin_lim" else {}
    Tp = 1 + x.size // 256
    split = (Tp - 1) * 256 if vocoder == "griffin_lim" else Tp * 256
    ceiling = 10.0 ** (-1.0 / 20.0)
    got = {}
    for name, lim in (("one gain", None), ("limiter", M.Limiter())):
        out = tmp_path / f"{name[:3]}.wav"
        tts.forward(str(wavs), phone_tokens=phone, out_path=str(out), loudness_lufs=0.0, true_peak_ceiling_dbtp=-1.0, limiter=lim, **kw)
        y, sr = audio_io.read_wav(str(out))
        assert sr == 16000 and np.isfinite(y).all() and y.size > split + 6400
        got[name] = [M.measure_loudness(part, ebu=True) for part in (y[:split], y[split:])]
        print(f"{vocoder}, {name}: parts read {[float(p['integrated_lufs'][0]) for p in got[name]]} LUFS, {[float(p['true_peak_dbtp'][0]) for p in got[name]]} dBTP")
    for p, q in zip(got["limiter"], got["one gain"]):
        # the file holds 16-bit samples: each moves by at most half a step of 2^-15, through the filter sum |h| times that
        assert p["true_peak"][0] <= ceiling * tp_margin(16000) + 2.0 ** -16 * 2.21
        assert p["integrated_lufs"][0] > q["integrated_lufs"][0]
    with pytest.raises(ValueError):
        tts.forward(str(wavs), phone_tokens=phone, out_path=None, loudness_lufs=0.0, limiter=M.Limiter(), **kw)
