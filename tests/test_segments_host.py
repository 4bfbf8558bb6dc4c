"""The speech-segment rule without a GPU: the consequences the header of include/megatts2_hip.h states for it, checked on its numpy
restatement (tests/segments_ref.py) over random flag patterns; the equality with the trim; the burst plan the GPU tests cut; two
deliberately wrong variants of the restatement, which the same checks must tell apart; `cut_alignment` against a frame-by-frame
restatement and against `trim_alignment`; the `Pauses` settings; and the library's host-only entry point mt2_segments_query with the
refusals of the three device calls, which are decided on the host before the handle is looked at."""
import ctypes as C
import inspect
import math
import os

import numpy as np
import pytest

import segments_ref as S
import trim_ref as T

INT_MAX = 2 ** 31 - 1


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


def patterns(n, seed):
    """random flag patterns of 1 .. 80 frames, and every tenth of up to 400: runs and gaps of geometric lengths, so that runs shorter and
    longer than every parameter occur"""
    rng = np.random.default_rng(seed)
    for i in range(n):
        F = int(rng.integers(1, 81)) if i % 10 else int(rng.integers(81, 401))
        a, f, on = np.zeros(F, bool), 0, bool(rng.integers(2))
        mean = float(rng.choice([1.5, 3.0, 8.0]))
        while f < F:
            n_run = int(rng.geometric(1.0 / mean))
            a[f:f + n_run] = on
            f, on = f + n_run, not on
        pad = int(rng.integers(0, 4))
        yield a, int(rng.integers(2 * pad + 1, 2 * pad + 12)), int(rng.integers(2, 8)), pad


def check_consequences(a, min_pause, min_speech, pad, mutate=None):
    """the four consequences; -> None, or the name of the first that fails"""
    F = len(a)
    s = S.smooth(a, min_pause, min_speech, pad, mutate)
    rc, rd = S.runs(s["c"]), S.runs(s["d"])
    if not s["found"]:
        return None if rd == [(0, F - 1)] else "whole"
    if len(rc) != len(rd):
        return "one for one"
    if any((max(0, c0 - pad), min(F - 1, c1 + pad)) != d for (c0, c1), d in zip(rc, rd)):
        return "widened and clamped"
    if any(n[0] - p[1] - 1 < min_pause - 2 * pad for p, n in zip(rd[:-1], rd[1:])):
        return "gap"
    if len(rd) > S.bound(F, min_pause, min_speech):
        return "bound"
    return None


def test_the_consequences_on_random_patterns():
    n = 0
    for a, mp, ms, pad in patterns(4000, 1):
        assert check_consequences(a, mp, ms, pad) is None, (a.astype(int), mp, ms, pad)
        n += 1
    assert n == 4000


def test_the_count_bound_is_met_and_64_bit():
    # speech runs of exactly min_speech with pauses of exactly min_pause between them reach the bound
    for mp, ms, k in ((5, 2, 7), (10, 3, 4), (1, 2, 30)):
        a = np.tile(np.r_[np.ones(ms, bool), np.zeros(mp, bool)], k)[:k * (ms + mp) - mp]
        s = S.smooth(a, mp, ms, 0)
        assert len(S.runs(s["d"])) == k == S.bound(len(a), mp, ms)
    assert S.bound(80, INT_MAX, 2) == 1 and S.bound(INT_MAX // 512, INT_MAX, INT_MAX) == 1


def test_built_cases():
    def d(a, mp, ms, pad):
        return S.runs(S.smooth(np.array(a, bool), mp, ms, pad)["d"])
    on, off = [1], [0]
    # a pause of min_pause - 1 is closed, one of min_pause is not
    assert d(on * 3 + off * 4 + on * 3, 5, 2, 0) == [(0, 9)]
    assert d(on * 3 + off * 5 + on * 3, 5, 2, 0) == [(0, 2), (8, 10)]
    # a run of min_speech - 1 goes, one of min_speech stays
    assert d(off * 6 + on * 2 + off * 6 + on * 3 + off * 6, 5, 3, 0) == [(14, 16)]
    # leading and trailing pauses are never closed, however short
    assert d(off * 1 + on * 4 + off * 2, 5, 2, 0) == [(1, 4)]
    # the pad is clamped at both ends
    assert d(off * 1 + on * 4 + off * 9 + on * 3 + off * 1, 5, 2, 2) == [(0, 6), (12, 17)]
    # all active; a single blip -> nothing found -> whole
    assert d(on * 9, 5, 2, 1) == [(0, 8)]
    s = S.smooth(np.array(off * 4 + on + off * 4, bool), 5, 2, 1)
    assert not s["found"] and S.runs(s["d"]) == [(0, 8)]
    # closing happens before opening: two blips a short pause apart make one run that stays
    assert d(off * 3 + on + off * 2 + on + off * 3, 5, 3, 0) == [(3, 6)]
    assert d(on + off * 70 + on, INT_MAX, 2, 0) == [(0, 71)]


@pytest.mark.parametrize("mutate", ["close_le", "pad_unclamped"])
def test_the_checks_tell_a_wrong_rule(mutate):
    bad = [check_consequences(a, mp, ms, pad, mutate) for a, mp, ms, pad in patterns(2000, 2)]
    names = {b for b in bad if b}
    print(mutate, sorted(names), sum(b is not None for b in bad))
    # "close_le" still satisfies the consequences (they do not pin the comparison): the built cases above are what tells it
    if mutate == "close_le":
        a = np.array([1] * 3 + [0] * 5 + [1] * 3, bool)
        assert S.runs(S.smooth(a, 5, 2, 0, mutate)["d"]) == [(0, 10)] != S.runs(S.smooth(a, 5, 2, 0)["d"])
    else:
        assert "widened and clamped" in names


def test_one_segment_is_the_trim():
    n = 0
    for seed in range(6):
        for L in (1500, 5000, 20000, 32768):
            for where in ("start", "interior", "end"):
                x = T.burst_signal(L, where, seed)
                for top_db in (20.0, 40.0):
                    e = T.energies(x)
                    if (e > e.max() * float(T.factor(top_db))).sum() < 2:
                        continue
                    r = S.analyse(x, top_db, min_pause=len(e), min_speech=2, pad=0)
                    assert r["segments"] == [T.bounds(x, top_db)]
                    n += 1
    assert n > 100


def test_the_burst_plan():
    x = S.plan_signal()
    assert len(x) == 62601 and 1 + len(x) // 512 == 123
    m = T.margin(x, 40.0)
    print("margin", m)
    assert m >= 0.5                                   # every frame a factor two or more from the threshold
    a = S.analyse(x, 40.0, 10, 3, 2)
    b = S.analyse(x, 40.0, 3, 2, 1)
    print(a["segments"], b["segments"])
    assert len(a["segments"]) == 3 and len(b["segments"]) == 4
    for r, keep in ((a, "speech"), (b, "speech")):
        sp, pa = S.cut(x, r["d"], "speech"), S.cut(x, r["d"], "pauses")
        assert len(sp) + len(pa) == len(x)
        assert len(sp) == sum(e - s for s, e in r["segments"]) == r["figures"][4]
        assert np.array_equal(sp, np.concatenate([x[s:e] for s, e in r["segments"]]))
    # the tail: the last frame owns 137 samples and is a pause
    assert len(S.cut(x, a["d"], "pauses")) % 512 == 137
    f = a["figures"]
    assert f[0] == 123 and f[3] == 3 and f[6] > 1e3 * f[7] > 0


# ---- the alignment ---------------------------------------------------------------------------------------------------------------

def test_cut_alignment():
    from megatts2_amd import audio_io
    rng = np.random.default_rng(5)
    n = 0
    for _ in range(300):
        F = int(rng.integers(3, 60))
        L = 512 * (F - 1) + int(rng.integers(0, 512))
        a = rng.random(F) < 0.5
        d = S.smooth(a, 3, 2, 1)["d"]
        segs = S.sample_segments(d, L)
        frames = 1 + L // 256
        dur = rng.multinomial(frames, np.ones(7) / 7)
        tok = np.arange(100, 107)
        want = S.cut_alignment(list(tok), list(dur), segs)
        got = audio_io.cut_alignment(tok, dur, segs)
        assert list(got[0]) == want[0] and list(got[1]) == want[1]
        Lc = sum(e - s for s, e in segs)
        assert int(got[1].sum()) == 1 + Lc // 256
        if len(segs) == 1:
            one = audio_io.trim_alignment(tok, dur, *segs[0])
            assert np.array_equal(one[0], got[0]) and np.array_equal(one[1], got[1]) and one[1].dtype == got[1].dtype
            n += 1
    assert n > 20
    with pytest.raises(ValueError):
        audio_io.cut_alignment([1, 2], [4, 4], [(100, 512)])
    with pytest.raises(ValueError):
        audio_io.cut_alignment([1, 2], [4, 4], [(512, 1024), (0, 512)])
    with pytest.raises(ValueError):
        audio_io.cut_alignment([1, 2], [4, 4], [(0, 4096)])
    with pytest.raises(ValueError):
        audio_io.cut_alignment([1, 2], [4, 4], [])


# ---- the settings ----------------------------------------------------------------------------------------------------------------

def test_pauses_settings(rt):
    p = rt.Pauses()
    assert (p.top_db, p.min_pause_ms, p.min_speech_ms, p.pad_ms) == (40.0, 320.0, 96.0, 64.0)
    assert p.frames(16000) == (10, 3, 2)
    assert p.frames(48000) == (30, 9, 6) and p.frames(8000) == (5, 2, 1)
    assert p.frames(22050) == tuple(round(ms * 22050 / 512000) for ms in (320, 96, 64))
    s = p.c_struct(16000, "pauses")
    assert (s.top_db, s.min_pause, s.min_speech, s.pad, s.keep) == (40.0, 10, 3, 2, 1)
    assert p.c_struct(16000).keep == 0
    for bad in (rt.Pauses(top_db=0.0), rt.Pauses(top_db=math.nan), rt.Pauses(top_db=math.inf), rt.Pauses(min_speech_ms=40.0),
                rt.Pauses(pad_ms=-40.0), rt.Pauses(min_pause_ms=128.0), rt.Pauses(min_pause_ms=math.nan)):
        with pytest.raises(ValueError):
            bad.c_struct(16000)
    with pytest.raises(ValueError):
        p.c_struct(16000, "both")
    with pytest.raises(ValueError):
        p.c_struct(4000)                              # 96 ms are under two frames at 4 kHz
    with pytest.raises(ValueError):
        p.c_struct(0)
    assert rt.segments_config(10.0, INT_MAX, 2, 0).min_pause == INT_MAX
    assert rt.segments_bound(80, INT_MAX, 2) == 1 and rt.segments_bound(123, 10, 3) == 10


def test_exports_and_the_struct(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_segments_query", "mt2_segment_frames", "mt2_speech_segments", "mt2_cut_pauses", "mt2_segments_config"):
        assert name in header and (name == "mt2_segments_config" or hasattr(lib, name))
    assert "MT2_SEGMENTS_FIELDS 8" in header and "MT2_SEGMENTS_CHUNK 256" in header
    assert rt.PAUSES_NAMES == S.NAMES and len(rt.PAUSES_NAMES) == 8
    assert C.sizeof(rt.MT2SegmentsConfig) == 20
    offs = {n: getattr(rt.MT2SegmentsConfig, n).offset for n, _ in rt.MT2SegmentsConfig._fields_}
    assert offs == {"top_db": 0, "min_pause": 4, "min_speech": 8, "pad": 12, "keep": 16}
    for cls in (rt.NativeModel, rt.MelFrontEnd):
        assert all(hasattr(cls, n) for n in ("segment_frames", "speech_segments", "cut_pauses"))
    sig = inspect.signature(rt.MelFrontEnd.from_audio)
    assert all(sig.parameters[n].default in (None, False) for n in ("cut_pauses", "return_segments", "return_pauses"))
    from megatts2_amd import audio_io
    assert hasattr(audio_io, "cut_alignment")


# ---- the library without a device ------------------------------------------------------------------------------------------------

def carve(lens):
    """segments_carve by hand: every piece rounded up to 256 bytes, never none -> (an audio call, the staged call on the same frames)"""
    r = lambda n: max(256, (n + 255) // 256 * 256)
    B, W, NB = len(lens), 1 + max(lens) // 512, -(-max(lens) // 512)
    smooth = 2 * r(4 * W * B) + 3 * r(W * B) + r(32 * B)
    return r(4 * 2 * B) + r(4 * NB * B) + r(4 * B) + r(4 * W * B) + smooth, r(4 * B) + smooth


@pytest.mark.parametrize("lens", [(1,), (62601,), (480000,), (1024, 99999, 5000), (480000,) * 32, (511, 512, 513), (28800000,)])
def test_query_is_the_carve(rt, lens):
    F, c, S_max, nbytes = rt.segments_query(lens=np.asarray(lens))
    assert F == 1 + max(lens) // 512 and c == float(T.factor(40.0)) and nbytes == carve(lens)[0]
    assert S_max == max(1, (F + 10) // 13)
    assert rt.segments_query(lens=np.asarray(lens), pauses=rt.segments_config(40.0, INT_MAX, 2, 0))[2] == 1
    assert rt.segments_query(L_max=max(lens), B=len(lens))[3] == nbytes


def test_query_refuses(rt):
    def why(L_max=8000, B=1, lens=None, **kw):
        cfg = rt.MT2SegmentsConfig(kw.get("top_db", 40.0), kw.get("min_pause", 10), kw.get("min_speech", 3), kw.get("pad", 2), kw.get("keep", 0))
        with pytest.raises(rt.NativeError) as e:
            rt.segments_query(lens=lens, L_max=L_max, B=B, pauses=cfg)
        return str(e.value)

    for bad in (0.0, -3.0, math.nan, math.inf):
        assert "top_db" in why(top_db=bad)
    assert "min_speech" in why(min_speech=1)
    assert "pad < 0" in why(pad=-1)
    assert "min_pause <= 2 pad" in why(min_pause=4) and "min_pause <= 2 pad" in why(min_pause=0, pad=0)
    assert "keep" in why(keep=2)
    assert "B outside" in why(B=0) and "B outside" in why(B=65536)
    assert "L_max" in why(L_max=0)
    assert "outside [1, L_max]" in why(lens=np.asarray([8000, 9000]), L_max=8000)
    assert "outside [1, L_max]" in why(lens=np.asarray([8000, 0]), L_max=8000)
    assert "INT_MAX - 4 * 512" in why(L_max=INT_MAX - 2047)
    assert rt.segments_query(L_max=INT_MAX - 2048, B=1)[0] == 1 + (INT_MAX - 2048) // 512


SENT = -77.25


def test_device_calls_refuse_on_the_host(rt):
    """host arrays stand in for device buffers: a refused call never reads or writes them, and the handle is looked at last"""
    lib = rt.load_library()

    def run(name, lens, L, B=None, overlap=None, null=(), Lout=None, S=None, F_max=None, **kw):
        lens = np.asarray(lens, np.int32)
        n = lens.size if B is None else B
        cfg = rt.MT2SegmentsConfig(kw.get("top_db", 40.0), kw.get("min_pause", 10), kw.get("min_speech", 3), kw.get("pad", 2), kw.get("keep", 0))
        rows = max(min(n, 2), 1)
        frames = name == "segment_frames"
        F = max(L, 1) if frames else 1 + max(L, 1) // 512
        S_need = max(1, (F + cfg.min_pause) // (cfg.min_speech + cfg.min_pause))
        cols, fcols = min(max(L, 1), 8000), min(F, 8000)      # a refused call touches no buffer, so the huge lengths need no huge arrays
        bufs = {"fig": np.full((rows, 8), SENT, np.float64), "in": np.full((rows, cols), SENT, np.float32),
                "out": np.full((rows, cols), SENT, np.float32), "seg": np.full((rows, S_need, 2), -7, np.int32),
                "cnt": np.full(rows, -7, np.int32), "flags": np.full((rows, fcols), 7, np.uint8), "energy": np.full((rows, fcols), SENT, np.float32),
                "olens": np.full(rows, -7, np.int32)}
        p = lambda k: None if k in null else rt._iptr(bufs["in"] if overlap == k else bufs[k])
        S_arg = S_need if S is None else S
        if frames:
            rc = lib.mt2_segment_frames(None, None, C.byref(cfg), p("in"), rt._iptr(lens), L if F_max is None else F_max, n, p("flags"), p("seg"), S_arg,
                                        p("cnt"), p("fig"))
        elif name == "speech_segments":
            rc = lib.mt2_speech_segments(None, None, C.byref(cfg), p("in"), rt._iptr(lens), L, n, p("seg"), S_arg, p("cnt"), p("fig"), p("energy"),
                                         F if F_max is None else F_max)
        else:
            rc = lib.mt2_cut_pauses(None, None, C.byref(cfg), p("in"), rt._iptr(lens), L, n, p("out"), L if Lout is None else Lout, p("olens"),
                                    p("seg"), S_arg, p("cnt"), p("fig"))
        assert rc != 0
        for k, v in bufs.items():
            assert (v == (7 if v.dtype == np.uint8 else -7 if v.dtype == np.int32 else SENT)).all(), k
        return lib.mt2_last_error().decode()

    for name in ("segment_frames", "speech_segments", "cut_pauses"):
        lens, L = ([40, 20], 40) if name == "segment_frames" else ([8000, 4000], 8000)
        assert "null model handle" in run(name, lens, L)
        for bad in (0.0, math.nan, -math.inf):
            assert "top_db" in run(name, lens, L, top_db=bad)
        assert "min_speech" in run(name, lens, L, min_speech=1)
        assert "pad < 0" in run(name, lens, L, pad=-1)
        assert "min_pause <= 2 pad" in run(name, lens, L, min_pause=4)
        assert "keep" in run(name, lens, L, keep=-1)
        assert "B outside" in run(name, lens, L, B=0)
        assert "B outside" in run(name, lens, L, B=65536)
        assert "outside [1, " in run(name, [L, L + 1], L)
        assert "outside [1, " in run(name, [0, L], L)
        assert "bad buffers" in run(name, lens, L, null=("in",))
        assert "S_max" in run(name, lens, L, S=0, min_pause=5, pad=0, min_speech=2)
        for k in ("seg", "cnt", "fig"):
            assert "overlapping" in run(name, lens, L, overlap=k)
        assert "null model handle" in run(name, lens, L, null=("seg", "cnt", "fig"))       # every optional output may be NULL
        assert "null model handle" in run(name, lens, L, null=("seg",), S=0)
    assert "F_max" in run("segment_frames", [40], 40, F_max=0)
    assert "F_max" in run("segment_frames", [40], 40, F_max=INT_MAX // 512 + 1)
    assert "overlapping" in run("segment_frames", [40, 20], 40, overlap="flags")
    assert "null model handle" in run("segment_frames", [40, 20], 40, null=("flags",))
    assert "F_max" in run("speech_segments", [8000, 4000], 8000, F_max=15)
    assert "overlapping" in run("speech_segments", [8000, 4000], 8000, overlap="energy")
    assert "null model handle" in run("speech_segments", [8000, 4000], 8000, null=("energy",), F_max=0)
    assert "INT_MAX - 4 * 512" in run("speech_segments", [INT_MAX - 2047], INT_MAX - 2047, null=("seg", "cnt", "fig", "energy"))
    assert "null out" in run("cut_pauses", [8000], 8000, null=("out",))
    assert "overlapping" in run("cut_pauses", [8000, 4000], 8000, overlap="out")           # in place is not offered
    assert "Lout_max" in run("cut_pauses", [8000, 4000], 8000, Lout=7999)
    assert "null model handle" in run("cut_pauses", [8000, 4000], 8000, null=("olens",))
