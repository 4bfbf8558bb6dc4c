"""Speech segments by frame energy and the cut of the pauses on the GPU (csrc/segments.hip: mt2_segment_frames, mt2_speech_segments,
mt2_cut_pauses) against the numpy restatement of the rule (tests/segments_ref.py).

The staged call is given energies in {0, 1} with top_db 10, so the raw flags ARE the pattern, and flags, segments and counts must EQUAL
the restatement's.  The frame counts sit around every constant of the kernel: the wave (64), the workgroup = the chunk of the passes
(256 = MT2_SEGMENTS_CHUNK) and its multiples.  The audio calls are asserted only after the restatement itself shows that no frame of
the input lies within relative 1e-3 of the threshold (an f32 sum of 2052 non-negative terms errs by at most 2052 * 2^-24 = 1.2e-4
relative, the trim's bound); then the segments equal the restatement's, and the restatement's on the device's own energies, the cut is
a bit-exact concatenation of slices in both `keep` modes, and the two means are within F * 2^-52 relative of the restatement's sums over
the device's energies (F terms in double, any order).  Input padding beyond lens[b] is NaN, every output buffer is pre-filled with a
sentinel and has guard words behind it."""
import ctypes as C
import functools

import numpy as np
import pytest

import segments_ref as S
import trim_ref as T

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = -77.25
GUARD = 11
MARGIN = 1e-3
INT_MAX = 2 ** 31 - 1
CHUNK = 256
FRAMES = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 513, 767, 768, 769, 1023, 1024, 1025, 2049, 4100)
CONFIGS = ((10, 3, 2), (3, 2, 1), (1, 2, 0), (7, 5, 3), (12, 7, 0))          # (min_pause, min_speech, pad)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def rt():
    from megatts2_amd import runtime
    return runtime


@functools.lru_cache(maxsize=None)
def frontend():
    return rt().MelFrontEnd()


# ---- the staged call on flag patterns ---------------------------------------------------------------------------------------------

def random_pattern(F, seed):
    rng = np.random.default_rng(1000003 * seed + F)
    a, f, on = np.zeros(F, bool), 0, bool(rng.integers(2))
    mean = float(rng.choice([1.5, 4.0, 12.0]))
    while f < F:
        n = int(rng.geometric(1.0 / mean))
        a[f:f + n] = on
        f, on = f + n, not on
    return a


def check_patterns(pats, mp, ms, pad, keep="speech"):
    """one ragged batch of flag patterns through mt2_segment_frames, every output against the restatement"""
    B, lens = len(pats), np.asarray([p.size for p in pats], np.int32)
    e = np.full((B, int(lens.max()) + 3), np.nan, np.float32)           # NaN beyond frame_lens[b]: never read
    for b, p in enumerate(pats):
        e[b, :p.size] = p
    cfg = rt().segments_config(10.0, mp, ms, pad, keep)
    out = frontend().segment_frames(dev(e), lens, cfg)
    flags, seg, cnt, fig = (out[k].cpu().numpy() for k in ("flags", "segments", "counts", "figures"))
    assert seg.shape[1] == S.bound(int(lens.max()), mp, ms)
    for b, p in enumerate(pats):
        F = p.size
        a = S.raw(e[b, :F], 10.0)
        assert np.array_equal(a, p if p.any() else np.ones(F, bool))       # an all-zero contour is silence: every frame active
        s = S.smooth(a, mp, ms, pad)
        want = S.frame_segments(s["d"])
        what = (F, mp, ms, pad, b)
        assert np.array_equal(flags[b, :F].astype(bool), s["d"]) and flags[b, :F].max() <= 1 and not flags[b, F:].any(), what
        assert cnt[b] == len(want) and seg[b, :len(want)].tolist() == [list(w) for w in want] and (seg[b, len(want):] == -1).all(), what
        ref = S.figures(e[b, :F], a, s, keep)
        assert np.array_equal(fig[b, :6], ref[:6]), (what, fig[b], ref)
        assert (np.abs(fig[b, 6:] - ref[6:]) <= F * 2.0 ** -52 * np.abs(ref[6:])).all(), what


@pytest.mark.parametrize("mp, ms, pad", CONFIGS)
def test_random_patterns_at_every_frame_count(mp, ms, pad):
    for seed in range(3):
        check_patterns([random_pattern(F, seed) for F in FRAMES], mp, ms, pad)
    check_patterns([random_pattern(F, 7) for F in FRAMES], mp, ms, pad, keep="pauses")


def built_patterns(F, mp, ms, pad):
    """the edges of the rule, once near frame 0 and once across every multiple of the chunk that fits"""
    pats = []

    def put(*spans):
        a = np.zeros(F, bool)
        for lo, hi in spans:
            if 0 <= lo < hi <= F:
                a[lo:hi] = True
        pats.append(a)

    for at in [20] + list(range(CHUNK, F - 3 * (mp + ms) - 8, CHUNK)):
        gap = min(mp, 64)
        lo = at - gap // 2 - 1                                             # the pause [lo, lo + gap) straddles `at`
        put((lo - ms - 2, lo), (lo + gap - 1, lo + gap + ms + 2))          # a pause of min_pause - 1: closed
        put((lo - ms - 2, lo), (lo + gap, lo + gap + ms + 2))              # a pause of min_pause: stays
        put((at - 1, at - 1 + ms - 1), (at + 2 * mp + ms, at + 2 * mp + 2 * ms))      # a run of min_speech - 1 across `at`: goes
        put((at - 1, at - 1 + ms))                                         # a run of min_speech across `at`: stays
        put((at - 1, at), (at + 1, at + ms - 1 + (mp > 1)))                # blips a frame apart: closed first, then long enough or not
    put((0, ms))                                                           # the pad clamped at frame 0 ...
    put((F - ms, F))                                                       # ... and at F - 1
    put((1, 1 + ms), (F - 1 - ms, F - 1))
    put((0, F))                                                            # all active
    put()                                                                  # all inactive: silence, every frame active
    put((F // 2, F // 2 + 1))                                              # a single blip: nothing found, the utterance stays whole
    return [p for p in pats if p.size]


@pytest.mark.parametrize("mp, ms, pad", CONFIGS)
def test_built_patterns(mp, ms, pad):
    for F in (40, 300, 600, 1100):
        if F > 3 * (mp + ms) + 30:
            check_patterns(built_patterns(F, mp, ms, pad), mp, ms, pad)


def test_single_blip_and_min_pause_int_max():
    a = np.zeros(300, bool)
    a[150] = True
    e = dev(a.astype(np.float32)[None])
    out = frontend().segment_frames(e, None, rt().segments_config(10.0, 10, 3, 2))
    assert out["segments"].cpu().numpy()[0, 0].tolist() == [0, 300] and out["counts"].cpu().numpy()[0] == 1
    assert out["figures"].cpu().numpy()[0].tolist()[:6] == [300, 1, 300, -1, 300 * 512, 0]           # -1: nothing found
    # min_pause = INT_MAX closes every pause between two active frames; the bound is 1 whatever F
    for F in (2, 257, 1025):
        pats = [random_pattern(F, s) for s in range(4)] + [np.r_[True, np.zeros(F - 2, bool), True]]
        check_patterns(pats, INT_MAX, 2, 0)
    check_patterns([random_pattern(700, 3)], INT_MAX, INT_MAX, 0)                                    # nothing can be long enough


# ---- the audio calls --------------------------------------------------------------------------------------------------------------

def cut_raw(rows, cfg, extra_L=7, extra_out=5, fe=None, energy=True):
    """mt2_cut_pauses (and mt2_speech_segments for the energies) on the utterances `rows` as one batch, through buffers of this file's
    own: every output pre-filled with a sentinel, GUARD words behind it -> dict of host arrays"""
    r, fe = rt(), fe or frontend()
    B, lens = len(rows), np.asarray([x.size for x in rows], np.int32)
    wav = np.full((B, int(lens.max()) + extra_L), np.nan, np.float32)
    for b, x in enumerate(rows):
        wav[b, :x.size] = x
    wav = dev(wav)
    Lw, F = int(lens.max()) + extra_out, 1 + int(lens.max()) // 512
    Sm = r.segments_bound(F, cfg.min_pause, cfg.min_speech)
    obuf = torch.full((B * Lw + GUARD,), SENT, device="cuda", dtype=torch.float32)
    sbuf = torch.full((B * Sm * 2 + GUARD,), -7, device="cuda", dtype=torch.int32)
    cbuf = torch.full((B + GUARD,), -7, device="cuda", dtype=torch.int32)
    fbuf = torch.full((B * 8 + GUARD,), SENT, device="cuda", dtype=torch.float64)
    olens = np.full(B, -7, np.int32)
    r._check(fe.lib.mt2_cut_pauses(fe.h, r._stream(), C.byref(cfg), r._ptr(wav), r._iptr(lens), wav.shape[1], B, r._ptr(obuf), Lw, r._iptr(olens),
                                   r._ptr(sbuf), Sm, r._ptr(cbuf), r._ptr(fbuf)))
    res = {"out": obuf.cpu().numpy()[:B * Lw].reshape(B, Lw), "out_lens": olens, "segments": sbuf.cpu().numpy()[:B * Sm * 2].reshape(B, Sm, 2),
           "counts": cbuf.cpu().numpy()[:B], "figures": fbuf.cpu().numpy()[:B * 8].reshape(B, 8)}
    assert (obuf.cpu().numpy()[B * Lw:] == SENT).all() and (sbuf.cpu().numpy()[B * Sm * 2:] == -7).all()
    assert (cbuf.cpu().numpy()[B:] == -7).all() and (fbuf.cpu().numpy()[B * 8:] == SENT).all()
    if energy:
        ebuf = torch.full((B * (F + 2) + GUARD,), SENT, device="cuda", dtype=torch.float32)
        s2 = torch.full((B * Sm * 2,), -7, device="cuda", dtype=torch.int32)
        r._check(fe.lib.mt2_speech_segments(fe.h, r._stream(), C.byref(cfg), r._ptr(wav), r._iptr(lens), wav.shape[1], B, r._ptr(s2), Sm, None, None,
                                            r._ptr(ebuf), F + 2))
        assert (ebuf.cpu().numpy()[B * (F + 2):] == SENT).all()
        res["energy"] = ebuf.cpu().numpy()[:B * (F + 2)].reshape(B, F + 2)
        assert np.array_equal(s2.cpu().numpy().reshape(B, Sm, 2), res["segments"])                 # the two calls agree
    return res


def check_utterance(x, g, b, top_db, mp, ms, pad, keep):
    """row b of cut_raw's result against the restatement of the rule on x"""
    L, F = x.size, 1 + x.size // 512
    m = T.margin(x, top_db)
    assert m >= MARGIN, f"the test input has a frame within {m:.3g} of the threshold: choose another input, not another bar"
    ref = S.analyse(x, top_db, mp, ms, pad, keep)
    own = S.analyse(x, top_db, mp, ms, pad, keep, e=g["energy"][b, :F])                              # on the device's own energies
    assert not g["energy"][b, F:].any()
    n = int(g["counts"][b])
    segs = [tuple(v) for v in g["segments"][b, :n].tolist()]
    assert segs == ref["segments"] == own["segments"] and (g["segments"][b, n:] == -1).all(), (L, segs, ref["segments"])
    assert all(s % 512 == 0 and 0 <= s < e <= L for s, e in segs)
    out, n_out = g["out"][b], int(g["out_lens"][b])
    assert n_out == ref["out"].size and np.array_equal(out[:n_out], ref["out"]) and not out[n_out:].any()      # bit-exact, zeros behind
    if keep == "speech":
        assert np.array_equal(out[:n_out], np.concatenate([x[s:e] for s, e in segs]))
    fig, want = g["figures"][b], own["figures"]
    assert np.array_equal(fig[:6], want[:6]) and fig[4] == n_out, (fig, want)
    assert (np.abs(fig[6:] - want[6:]) <= F * 2.0 ** -52 * np.abs(want[6:])).all(), (fig, want)
    return ref


def both_modes(x, top_db, mp, ms, pad):
    cfgs = {k: rt().segments_config(top_db, mp, ms, pad, k) for k in ("speech", "pauses")}
    got = {k: cut_raw([x], c) for k, c in cfgs.items()}
    ref = {k: check_utterance(x, got[k], 0, top_db, mp, ms, pad, k) for k in got}
    # the two modes partition the input: frame by frame, each kept in exactly one of them
    assert got["speech"]["out_lens"][0] + got["pauses"]["out_lens"][0] == x.size
    assert np.array_equal(got["speech"]["segments"], got["pauses"]["segments"])
    d = ref["speech"]["d"]
    at = {"speech": 0, "pauses": 0}
    for f in range(d.size):
        k = "speech" if d[f] else "pauses"
        blk = x[512 * f:512 * (f + 1)]
        assert np.array_equal(got[k]["out"][0, at[k]:at[k] + blk.size], blk)
        at[k] += blk.size
    return ref["speech"]


def test_the_burst_plan():
    x = S.plan_signal()
    assert x.size == 62601
    a = both_modes(x, 40.0, 10, 3, 2)
    b = both_modes(x, 40.0, 3, 2, 1)
    assert len(a["segments"]) == 3 and len(b["segments"]) == 4
    for shift in (137, 300):
        both_modes(S.plan_signal(shift=shift, seed=shift), 40.0, 10, 3, 2)


@pytest.mark.parametrize("L", [1, 511, 512, 513, 1024, 2047, 32768, 131072 + 700])
def test_lengths(L):
    """32768: the last frame owns no sample; 131072 + 700: 258 frames, two chunks of the passes"""
    for where in ("start", "interior", "end"):
        both_modes(T.burst_signal(L, where), 40.0, 3, 2, 1)


def test_several_chunks_of_bursts():
    x = S.plan_signal(plan=S.PLAN * 5, seed=4)                     # 611 frames: three chunks, segments and pauses across both boundaries
    r = both_modes(x, 40.0, 10, 3, 2)
    assert x.size == 312457 and len(r["segments"]) == 9
    assert len(both_modes(x, 40.0, 3, 2, 1)["segments"]) == 22


def test_one_segment_is_the_trim():
    fe = frontend()
    for L, where in ((16000, "interior"), (5000, "end"), (48000, "start")):
        x = T.burst_signal(L, where, seed=5)
        F = 1 + L // 512
        g = cut_raw([x], rt().segments_config(40.0, F, 2, 0), extra_out=0, energy=False)
        out, out_lens, bounds = fe.trim(dev(x[None]), None, 40.0)
        assert bounds[0, 1] - bounds[0, 0] >= 1024 and g["counts"][0] == 1
        assert g["segments"][0, 0].tolist() == bounds[0].tolist() == list(T.bounds(x, 40.0))
        assert g["out_lens"][0] == out_lens[0] and np.array_equal(g["out"], out.cpu().numpy())


def ragged_rows():
    return [S.plan_signal(seed=1), np.zeros(3000, np.float32), np.array([0.25], np.float32), T.burst_signal(20000, "interior", seed=2)]


def test_ragged_batch_is_its_utterances_alone_and_two_runs_agree():
    rows = ragged_rows()
    cfg = rt().segments_config(40.0, 10, 3, 2)
    g = cut_raw(rows, cfg)
    again, wider = cut_raw(rows, cfg), cut_raw(rows, cfg, extra_L=7 + 13)
    for k in g:
        assert np.array_equal(g[k].view(np.uint8), again[k].view(np.uint8)), k
        assert np.array_equal(g[k].view(np.uint8), wider[k].view(np.uint8)), k                  # L_max does not enter
    assert g["segments"][1, 0].tolist() == [0, 3000] and g["figures"][1, 3] == 1 and not g["out"][1].any()      # silence: every frame active
    assert g["segments"][2, 0].tolist() == [0, 1] and g["out_lens"][2] == 1 and g["out"][2, 0] == 0.25
    for b, x in enumerate(rows):
        one = cut_raw([x], cfg)
        n, F, k = int(g["out_lens"][b]), 1 + x.size // 512, int(g["counts"][b])
        assert one["out_lens"][0] == n and one["counts"][0] == k
        assert np.array_equal(one["out"][0, :n], g["out"][b, :n]) and not g["out"][b, n:].any()
        assert np.array_equal(one["segments"][0, :k], g["segments"][b, :k]) and (g["segments"][b, k:] == -1).all()
        assert np.array_equal(one["figures"][0].view(np.uint8), g["figures"][b].view(np.uint8))                # figures included
        assert np.array_equal(one["energy"][0, :F], g["energy"][b, :F])
        if x.size > 3000:
            check_utterance(x, g, b, 40.0, 10, 3, 2, "speech")


def test_non_finite_samples_give_segments_inside_the_utterance():
    x = S.plan_signal(seed=3).copy()
    x[1234], x[40000] = np.nan, np.inf
    y = x.copy()
    y[:] = np.nan
    for row in (x, y):
        for keep in ("speech", "pauses"):
            g = cut_raw([row], rt().segments_config(40.0, 10, 3, 2, keep), energy=False)
            n = int(g["counts"][0])
            assert n >= 1 and 0 <= g["out_lens"][0] <= row.size
            assert all(0 <= s < e <= row.size for s, e in g["segments"][0, :n].tolist()) and (g["segments"][0, n:] == -1).all()


def test_refusals_leave_outputs_and_arena_untouched():
    r = rt()
    fe = r.MelFrontEnd()
    try:
        fe.workspace_reserve(1 << 20)
        fe.workspace_fill(0xA5)
        x = dev(S.plan_signal()[None])
        lens = np.asarray([x.shape[1]], np.int32)
        out = torch.full((1, x.shape[1]), SENT, device="cuda")
        seg = torch.full((1, 10, 2), -7, device="cuda", dtype=torch.int32)
        fig = torch.full((1, 8), SENT, device="cuda", dtype=torch.float64)
        olens = np.full(1, -7, np.int32)

        def call(cfg, Lout=None, Sm=10, o=out):
            return fe.lib.mt2_cut_pauses(fe.h, r._stream(), C.byref(cfg), r._ptr(x), r._iptr(lens), x.shape[1], 1, r._ptr(o),
                                         x.shape[1] if Lout is None else Lout, r._iptr(olens), r._ptr(seg), Sm, None, r._ptr(fig))

        ok = r.MT2SegmentsConfig(40.0, 10, 3, 2, 0)
        cases = (("top_db", lambda: call(r.MT2SegmentsConfig(0.0, 10, 3, 2, 0))), ("min_speech", lambda: call(r.MT2SegmentsConfig(40.0, 10, 1, 2, 0))),
                 ("2 pad", lambda: call(r.MT2SegmentsConfig(40.0, 4, 3, 2, 0))), ("S_max", lambda: call(ok, Sm=9)),
                 ("Lout_max", lambda: call(ok, Lout=62600)), ("overlapping", lambda: call(ok, o=x)))
        for why, refused in cases:
            rc = refused()
            assert rc != 0 and why in fe.lib.mt2_last_error().decode(), why
        torch.cuda.synchronize()
        assert (out == SENT).all() and (seg == -7).all() and (fig == SENT).all() and (olens == -7).all()
        assert fe.workspace_high_water() == 0 and (fe.workspace_peek(0, 1 << 20) == 0xA5).all()
        assert call(ok) == 0 and olens[0] > 0
    finally:
        fe.close()


def test_high_water_is_the_query():
    """on handles nothing else has used: the high-water mark is the most any call took since the handle was made"""
    r = rt()
    rows = ragged_rows()
    lens = np.asarray([x.size for x in rows], np.int32)
    want = r.segments_query(lens=lens)[3]
    cfg = r.segments_config(40.0, 10, 3, 2)
    wav = dev(np.stack([np.resize(x, int(lens.max())) for x in rows]))
    calls = {"cut, every output": lambda fe: cut_raw(rows, cfg, fe=fe, energy=False),
             "cut, no optional output": lambda fe: fe.cut_pauses(wav, lens),
             "segments": lambda fe: fe.speech_segments(wav, lens, return_energy=True)}
    for what, call in calls.items():
        fe = r.MelFrontEnd()
        try:
            call(fe)
            torch.cuda.synchronize()
            assert fe.workspace_high_water() == want, what
        finally:
            fe.close()
    fe = r.MelFrontEnd()
    try:
        fl = np.asarray([300, 17, 1025], np.int32)
        fe.segment_frames(torch.ones(3, 1025, device="cuda"), fl)
        torch.cuda.synchronize()
        rr = lambda n: max(256, (n + 255) // 256 * 256)
        assert fe.workspace_high_water() == rr(4 * 3) + 2 * rr(4 * 1025 * 3) + 3 * rr(1025 * 3) + rr(32 * 3)
    finally:
        fe.close()


# ---- the front end ----------------------------------------------------------------------------------------------------------------

def bits(t):
    return t.detach().cpu().numpy().view(np.uint8)


def test_from_audio_without_the_argument_keeps_its_bits():
    r, fe = rt(), frontend()
    x = dev(S.plan_signal()[None] * np.float32(0.5))
    for kw in ({}, {"denoise": r.Denoise()}, {"dereverb": r.Dereverb(), "declip": r.Declip(frame=256)}):
        for sr in (16000, 24000):
            a, b = fe.from_audio(x, sr, **kw), fe.from_audio(x, sr, cut_pauses=None, return_segments=False, return_pauses=False, **kw)
            assert len(a) == len(b) == 2 and np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(a[1], b[1])
    y = torch.empty_like(x)
    ln = np.asarray([x.shape[1]], np.int32)
    r._check(fe.lib.mt2_peak_normalize(fe.h, r._stream(), r._ptr(x), r._iptr(ln), x.shape[1], 1, r._ptr(y)))
    assert np.array_equal(bits(fe.from_audio(x, 16000)[0]), bits(fe(y, ln)))                       # the path of before: normalise, mel
    with pytest.raises(ValueError):
        fe.from_audio(x, 16000, cut_pauses=r.Pauses(), trim_db=40.0)
    with pytest.raises(ValueError):
        fe.from_audio(x, 16000, cut_pauses=r.Pauses(), return_bounds=True)
    with pytest.raises(ValueError):
        fe.from_audio(x, 16000, return_pauses=True)


def test_from_audio_with_cut_pauses():
    r, fe = rt(), frontend()
    x = S.plan_signal()
    wav = dev(np.stack([x, np.r_[x[:30000], np.zeros(x.size - 30000, np.float32)]]) * np.float32(0.5))
    lens = np.asarray([x.size, 30000], np.int32)
    mel0, T0 = fe.from_audio(wav, 16000, lens)
    mel, Tm, seg, cnt, fig = fe.from_audio(wav, 16000, lens, cut_pauses=r.Pauses(), return_segments=True, return_pauses=True)
    fig, cnt = fig.cpu().numpy(), cnt.cpu().numpy()
    assert fig.shape == (2, 8) and cnt.tolist() == [3, 2] and seg.shape[0] == 2
    for b in range(2):
        out_len = int(fig[b, 4])
        assert Tm[b] == 1 + out_len // 256 and Tm[b] < T0[b]
        want = sum(e - s for s, e in seg[b, :cnt[b]].tolist())
        assert out_len == want
        cut_mean, whole_mean = float(mel[b, :Tm[b]].mean()), float(mel0[b, :T0[b]].mean())
        print(f"utterance {b}: {T0[b]} -> {Tm[b]} frames, mean log-mel {whole_mean:.3f} -> {cut_mean:.3f}")
        assert cut_mean > whole_mean                                                               # the pauses are gone
    # the same through the staged calls: normalise, cut, mel
    y = torch.empty_like(wav)
    r._check(fe.lib.mt2_peak_normalize(fe.h, r._stream(), r._ptr(wav), r._iptr(lens), wav.shape[1], 2, r._ptr(y)))
    out, out_lens = fe.cut_pauses(y, lens, r.Pauses())
    assert np.array_equal(1 + out_lens // 256, Tm) and np.array_equal(bits(fe(out, out_lens)), bits(mel))


# ---- megatts2 ----------------------------------------------------------------------------------------------------------------------

def test_megatts2_functions():
    from megatts2_amd import megatts2 as M
    x = S.plan_signal()
    ref = S.analyse(x, 40.0, 10, 3, 2)
    st = M.speech_segments(x)
    assert st["segments"] == [ref["segments"]] and st["n_segments"][0] == 3 and st["kept_samples"][0] == ref["out"].size
    out, out_lens, st2 = M.cut_pauses(x)
    assert out.ndim == 1 and out_lens[0] == ref["out"].size and np.array_equal(out, ref["out"]) and st2["segments"] == st["segments"]
    noise, noise_lens, _ = M.cut_pauses(x, keep="pauses")
    assert noise_lens[0] + out_lens[0] == x.size and np.array_equal(noise, S.cut(x, ref["d"], "pauses"))
    parts = M.split_on_pauses(x)
    assert len(parts) == 3 and all(np.array_equal(p, x[s:e]) for p, (s, e) in zip(parts, ref["segments"]))
    batch = M.split_on_pauses(np.stack([x, x[::-1]]))
    assert len(batch) == 2 and all(np.array_equal(p, q) for p, q in zip(batch[0], parts))
    # the durations become frames at the rate of the audio: three times as many at 48 kHz
    assert M.speech_segments(x, 48000)["segments"] == [S.analyse(x, 40.0, 30, 9, 6)["segments"]]
    mel = M.extract_mel_spec(x, cut_pauses=M.Pauses())
    assert tuple(mel.shape) == (80, 1 + int(out_lens[0]) // 256)
    with pytest.raises(ValueError):
        M.extract_mel_spec(x, trim_db=40.0, cut_pauses=M.Pauses())


def test_forward_cuts_the_pauses_of_every_prompt(tmp_path):
    """Megatts.forward(cut_pauses=Pauses()) on one 16 kHz and one 48 kHz prompt is `synthesize` on the concatenated
    from_audio(cut_pauses=Pauses()) mels, and aux["prompt_pauses"] holds the figures of each file"""
    from conftest import synth_models
    from megatts2_amd import audio_io
    from megatts2_amd import megatts2 as M
    (g, p, a, _), (sd_g, sd_p, sd_a, _) = synth_models("tiny")
    tts = M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)))
    files = []
    for name, sr, plan in (("a16k.wav", 16000, (7, 9, 13, 6, 9)), ("b48k.wav", 48000, (20, 30, 45, 24, 12))):
        x = np.array(S.plan_signal(plan=plan, tail=137, seed=sr))
        audio_io.write_wav(str(tmp_path / name), x, sr)
        files.append((x, sr))
    fe = M._frontend()
    parts = [fe.from_audio(dev(x[None]), sr, cut_pauses=M.Pauses(), return_pauses=True) for x, sr in files]
    for mel, mel_lens, fig in parts:
        f = fig.cpu().numpy()[0]
        assert f[3] == 2 and mel.shape[1] == mel_lens[0] == 1 + int(f[4]) // 256
    mels = torch.cat([mel[0] for mel, _, _ in parts], dim=0).unsqueeze(0)
    phone = np.random.default_rng(9).integers(0, g.mrte.phone_vocab_size, 6)
    want_mel, want_lens, want_aux = tts.synthesize(dev(phone.reshape(1, -1).astype(np.int64)), mels, return_aux=True)
    mel, mel_lens, aux = tts.forward(str(tmp_path), phone_tokens=phone, out_path=None, cut_pauses=M.Pauses())
    assert np.array_equal(np.asarray(mel_lens), np.asarray(want_lens))
    assert torch.equal(mel, want_mel) and torch.equal(aux["dur"], want_aux["dur"]) and torch.equal(aux["codes"], want_aux["codes"])
    assert [int(d["segments"]) for d in aux["prompt_pauses"]] == [2, 2] and set(aux["prompt_pauses"][0]) == set(M.PAUSES_NAMES)
    whole = torch.cat([fe.from_audio(dev(x[None]), sr)[0][0] for x, sr in files], dim=0)
    assert whole.shape[0] > mels.shape[1] and "prompt_pauses" not in tts.forward(str(tmp_path), phone_tokens=phone, out_path=None)[2]
    with pytest.raises(ValueError):
        tts.forward(str(tmp_path), phone_tokens=phone, out_path=None, cut_pauses=M.Pauses(), trim_db=40.0)
