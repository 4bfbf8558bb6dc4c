"""The weighted-prediction-error rule without a GPU: its float64 restatement (tests/wpe_ref.py) against ground truth that is neither an
oracle nor a restatement - a column built by a known prediction filter must come back with that filter removed, a hop-aligned echo
must go - then the library's host-only entry point mt2_dereverb_query and the refusals of the two device calls, which are decided on
the host before the handle is looked at.

Ground truth, measured with the committed restatement over seeds 0 .. 7 (this file prints each figure before it asserts); a bar is the
worst seed's figure plus 3 dB (the spread seen from seed to seed is about +-2 dB):

  known filter (|g_k| = 0.2 0.8^k, S gated 1 / 0.01 every 12 frames, 8 bins pooled), ||D - S||^2 / ||S||^2, before: -9.9 .. -6.0 dB
    K 10, delay 3   T 256: -28.0 .. -25.8 dB    T 1024: -33.0 .. -32.1 dB    T 4100: -40.7 .. -37.8 dB, max |g^ - g| <= 0.015
    K 16, delay 1   T 4100: -33.9 .. -31.1 dB
    the residual falls roughly as K / T, the statistical error of the estimate
  one echo of gain 0.5 on gated white-noise bursts with exactly silent gaps, error against the clean signal, before: -6.2 .. -6.0 dB
    n_fft 1024, hop 256, 4 s   4 hops: -20.9 .. -19.7 dB    6 hops: -17.8 .. -16.9 dB      (no 10-tap filter beats 0.5^4 = -24.1 dB)
    n_fft 128, hop 32, 4 hops  T 64: -11.9 .. -7.1 dB       T 257: -16.7 .. -14.6 dB       T 1025: -21.1 .. -19.4 dB
    variance_floor 1e-4 and 1e-10 on the first signal: -23.8 dB both - on THESE bursts the smaller floors do better than the default
    1e-2 (-20.0 dB); the default follows the rule's statement and is not tuned to this builder
  clean bursts come out -23.1 dB from themselves; a steady 440 Hz tone is removed (-61 dB away from the clip's edges)
  mutations: delay + 1 leaves the known-filter residual at -14 dB at every T; the variance taken from Y in every iteration leaves it
    at -27.6 dB at K 10, T 4100 - both over the bars.  The echo figures do not tell the first mutation from the rule (a
    reflection at 4 hops is still inside delay 4 .. 13)."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import wpe_ref as W

SR = 16000
SEEDS = range(8)
BINS = 8
# (K, delay, T) -> (the worst seed's pooled residual in dB, the bar = that + 3 dB)
KNOWN = {(10, 3, 256): (-25.8, -22.8), (10, 3, 1024): (-32.1, -29.1), (10, 3, 4100): (-37.8, -34.8), (16, 1, 4100): (-31.1, -28.1)}
G_BAR = 0.02                                    # max |g^ - g| at K 10, T 4100: 0.015 seen
# (configuration, hops, samples) -> (the worst seed's error in dB, the bar = that + 3 dB)
ECHO = {("prod", 4, 64000): (-19.7, -16.7), ("prod", 6, 64000): (-16.9, -13.9), ("small", 4, 63 * 32): (-7.1, -4.1),
        ("small", 4, 256 * 32): (-14.6, -11.6), ("small", 4, 1024 * 32): (-19.4, -16.4)}


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


def audio(name="prod"):
    from megatts2_amd.config import AudioConfig
    if name == "prod":
        return AudioConfig()
    return AudioConfig(sample_rate=SR, n_fft=128, hop_length=32, win_length=128, n_mels=8, f_min=0.0, f_max=8000.0)


def pooled_db(D, S):
    return 10 * math.log10((np.abs(D - S) ** 2).sum() / (np.abs(S) ** 2).sum())


def known_case(K, delay, T, seed, **kw):
    g = W.known_filter(K, seed)
    Y, S = W.ar_columns(T, BINS, g, delay, seed)
    r = W.wpe(Y, W.Config(delay=delay, taps=K), **kw)
    return pooled_db(Y, S), pooled_db(r["D"], S), float(np.abs(r["g"] - g[None]).max()), r


# ---- ground truth ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K, delay, T", sorted(KNOWN))
def test_a_known_prediction_filter_is_removed(K, delay, T):
    seen, bar = KNOWN[(K, delay, T)]
    rows = [known_case(K, delay, T, s)[:3] for s in SEEDS]
    before, after, gerr = (np.array(c) for c in zip(*rows))
    print(f"K {K} delay {delay} T {T}: before {before.min():.1f} .. {before.max():.1f} dB, after {after.min():.1f} .. {after.max():.1f} dB "
          f"(bar {bar}), max |g^ - g| {gerr.max():.4f}")
    assert before.min() > -12.0 and before.max() < -5.5
    assert after.max() <= bar
    if (K, T) == (10, 4100):
        assert gerr.max() <= G_BAR


@pytest.mark.parametrize("name, hops, L", sorted(ECHO))
def test_a_hop_aligned_echo_is_removed(name, hops, L):
    a = audio(name)
    seen, bar = ECHO[(name, hops, L)]
    before, after = [], []
    for s in SEEDS:
        x = W.gated_bursts(L, s)
        y = W.echo(x, hops, a.hop_length)
        r = W.dereverb(y, a)
        assert r["filtered"].all() and len(r["y"]) == a.hop_length * (L // a.hop_length)
        before.append(W.error_db(y, x))
        after.append(W.error_db(r["y"], x))
    print(f"{name} echo at {hops} hops, T {1 + L // a.hop_length}: before {min(before):.2f} .. {max(before):.2f} dB, after {min(after):.2f} .. "
          f"{max(after):.2f} dB (bar {bar})")
    assert -6.6 < min(before) and max(before) < -5.9
    assert max(after) <= bar


def test_both_mutations_fail_the_known_filter_bars():
    for mutate in ("delay", "lambda_from_Y"):
        worst = max(known_case(10, 3, 4100, s, mutate=mutate)[1] for s in (0, 1))
        print(f"mutation {mutate}: {worst:.1f} dB against the bar {KNOWN[(10, 3, 4100)][1]}")
        assert worst > KNOWN[(10, 3, 4100)][1]
    assert max(known_case(10, 3, 256, s, mutate="delay")[1] for s in (0, 1)) > KNOWN[(10, 3, 256)][1]


def test_the_two_consequences_said_plainly():
    """a steady tone is predictable from its own past and goes like a reflection; clean gated noise comes out slightly distorted"""
    a = audio()
    t = np.arange(4 * SR) / SR
    tone = (0.2 * np.sin(2 * np.pi * 440.0 * t)).astype(np.float32)
    y = W.dereverb(tone, a)["y"]
    edge = 4 * a.n_fft
    level = 10 * math.log10((y[edge:-edge] ** 2).sum() / (tone[edge:len(y) - edge].astype(np.float64) ** 2).sum())
    x = W.gated_bursts(4 * SR, 0)
    own = W.error_db(W.dereverb(x, a)["y"], x)
    print(f"steady 440 Hz tone: {level:.1f} dB of its level left away from the edges; clean bursts: {own:.1f} dB from themselves")
    assert level <= -15.0              # -61 dB seen: removed
    assert -30.0 < own <= -20.1        # -23.1 dB seen, + 3 dB: distorted, slightly


# ---- the restatement's edges ---------------------------------------------------------------------------------------------------------

def test_silence_gives_silence_and_a_zero_bin_passes_through():
    r = W.wpe(np.zeros((40, 5), np.complex128))
    assert (r["D"] == 0).all() and not r["filtered"].any() and (r["g"] == 0).all() and r["figures"][5] == 5 and r["figures"][7] == 0
    Y, _ = W.ar_columns(120, 6, W.known_filter(10, 0), 3, 0)
    Y[:, 2] = 0
    r = W.wpe(Y)
    assert r["filtered"].tolist() == [True, True, False, True, True, True] and (r["D"][:, 2] == 0).all()
    assert r["figures"][4] == 5 and r["figures"][5] == 1 and r["figures"][7] == 3 and (r["g"][2] == 0).all()
    alone = W.wpe(Y[:, :2])
    assert np.array_equal(alone["D"], r["D"][:, :2])                           # a bin depends on itself alone


@pytest.mark.parametrize("T", [1, 2, 3])
def test_no_frame_behind_the_delay_passes_through(T):
    Y, _ = W.ar_columns(T, 4, W.known_filter(10, 0), 3, 1)
    r = W.wpe(Y)
    assert not r["filtered"].any() and np.array_equal(r["D"], Y)
    r4 = W.wpe(W.ar_columns(4, 4, W.known_filter(10, 0), 3, 1)[0])            # T = delay + 1: one non-zero regressor, and it is used
    assert r4["filtered"].all()


def test_a_short_clip_passes_through_the_whole_call():
    a = audio("small")
    x = W.echo(W.gated_bursts(42 * 32, 3), 4, 32)                              # T = 43 = delay + 4 taps: filtered
    assert W.dereverb(x, a)["filtered"].all()
    x = x[:41 * 32 + 5]                                                        # T = 42: not
    r = W.dereverb(x, a)
    assert not r["filtered"].any() and np.array_equal(r["D"], r["S"])


def test_the_two_summing_orders_agree_to_rounding():
    Y, _ = W.ar_columns(300, 4, W.known_filter(10, 2), 3, 2)
    a, b = W.wpe(Y, order="lanes"), W.wpe(Y, order="ascending")
    err = np.linalg.norm(a["D"] - b["D"]) / np.linalg.norm(b["D"])
    assert err < 1e-6 and np.allclose(a["g"], b["g"], rtol=0, atol=1e-9)


def test_tsum_is_the_lane_order():
    rng = np.random.default_rng(0)
    for T in (1, 63, 64, 65, 300):
        A = rng.standard_normal((T, 3)) * 10.0 ** rng.integers(-8, 8, (T, 3))
        want = []
        for f in range(3):
            lanes = [0.0] * 64
            for t in range(T):
                lanes[t % 64] += A[t, f]
            for d in (32, 16, 8, 4, 2, 1):
                lanes = [lanes[i] + lanes[i ^ d] for i in range(64)]
            want.append(lanes[0])
        assert np.array_equal(W.tsum(A, "lanes"), np.array(want))
        asc = np.zeros(3)
        for t in range(T):
            asc += A[t]
        assert np.array_equal(W.tsum(A, "ascending"), asc)


# ---- the library without a device ------------------------------------------------------------------------------------------------

def dataclass_fields(d):
    import dataclasses
    return {f.name: getattr(d, f.name) for f in dataclasses.fields(d)}


def test_exports_and_the_struct(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_dereverb_query", "mt2_wpe_spectrum", "mt2_dereverb", "mt2_wpe_config"):
        assert name in header and (name == "mt2_wpe_config" or hasattr(lib, name))
    assert "MT2_WPE_FIELDS 8" in header and "MT2_WPE_MAX_FRAMES MT2_DENOISE_MAX_FRAMES" in header
    assert rt.WPE_NAMES == W.FIELDS and len(rt.WPE_NAMES) == 8
    assert dataclass_fields(rt.Dereverb()) == dataclass_fields(W.Config())
    d = rt.Dereverb(delay=2, taps=7, iterations=5, context=4, variance_floor=0.25, loading=1e-3)
    s = d.c_struct()
    assert (s.delay, s.taps, s.iterations, s.context, s.variance_floor, s.loading, s.reserved) == (2, 7, 5, 4, 0.25, 1e-3, 0)
    assert C.sizeof(s) == 40
    from megatts2_amd import megatts2 as M
    assert hasattr(M, "dereverb_audio") and M.Dereverb is rt.Dereverb
    for cls in (rt.NativeModel, rt.MelFrontEnd):
        assert all(hasattr(cls, n) for n in ("dereverb", "wpe_spectrum"))


def carve(a, lens):
    """dereverb_layout by hand: every piece rounded up to 256 bytes, never none"""
    r = lambda n: max(256, (n + 255) // 256 * 256)
    q = lambda n: (n + 3) // 4 * 4
    N, h = a.n_fft, a.hop_length
    F = N // 2 + 1
    S, B = q(2 * F), len(lens)
    T = [1 + L // h for L in lens]
    Fr, Rb = sum(T), sum(t - 1 + N // h for t in T)
    cells = sum(F * q(t) for t in T)
    return (r(4 * (2 * q(Rb) + q(B) + 2 * q(Fr) + 3 * q(B) + B)) + r(4 * Rb * h) + r(4 * Fr * S) + 2 * r(8 * cells) + r(40 * B * F)
            + r(4 * Fr * N))


@pytest.mark.parametrize("lens", [(1024,), (480000,), (1024, 99999, 5000), (8000,) * 32, (770, 1279)])
def test_query_is_the_carve(rt, lens):
    nbytes, lout = rt.dereverb_query(audio(), lens=np.asarray(lens))
    assert nbytes == carve(audio(), lens) and lout == 256 * (max(lens) // 256)
    small = [max(64, L // 8) for L in lens]
    assert rt.dereverb_query(audio("small"), lens=np.asarray(small))[0] == carve(audio("small"), small)


def test_query_refuses(rt):
    def why(L_max=8000, B=1, lens=None, **kw):
        with pytest.raises(rt.NativeError) as e:
            rt.dereverb_query(audio(), lens=lens, L_max=L_max, B=B, dereverb=rt.Dereverb(**kw))
        return str(e.value)

    assert rt.dereverb_query(audio(), L_max=8000, B=1)[1] == 7936
    assert "delay" in why(delay=0) and "delay" in why(delay=9)
    assert "taps" in why(taps=0) and "taps" in why(taps=17)
    assert "iterations" in why(iterations=0) and "iterations" in why(iterations=9)
    assert "context" in why(context=-1) and "context" in why(context=5)
    for bad in (0.0, -1.0, 1.0001, math.nan, math.inf):
        assert "variance_floor" in why(variance_floor=bad)
    for bad in (-1e-9, 0.011, math.nan, math.inf):
        assert "loading" in why(loading=bad)
    assert rt.dereverb_query(audio(), L_max=8000, B=1, dereverb=rt.Dereverb(delay=8, taps=16, iterations=8, context=4, variance_floor=1.0,
                                                                           loading=0.0))[1] == 7936
    assert "B outside" in why(B=0) and "B outside" in why(B=65536)
    assert "fewer frames" in why(L_max=767)
    assert "fewer frames" in why(lens=np.asarray([8000, 700]))
    assert "MAX_FRAMES" in why(L_max=16384 * 256)
    assert rt.dereverb_query(audio(), L_max=16384 * 256 - 1, B=1)[1] == 16383 * 256
    assert "outside [1, L_max]" in why(lens=np.asarray([8000, 9000]), L_max=8000)


SENT = -77.25


def test_device_calls_refuse_on_the_host(rt):
    """host arrays stand in for device buffers: a refused call never reads or writes them, and the handle is looked at last"""
    lib = rt.load_library()
    a = audio()
    ac = rt._audio_struct(a)
    F = a.n_fft // 2 + 1
    Fp, S = (F + 3) & ~3, (2 * F + 3) & ~3

    def run(name, lens, T_or_L, B=None, cfg=None, overlap=None, null=None, Lout=None, in_place=False, reserved=0):
        lens = np.asarray(lens, np.int32)
        n = lens.size if B is None else B
        wc = (cfg or rt.Dereverb()).c_struct()
        wc.reserved = reserved
        rows = max(min(n, 2), 1)
        bufs = {"fig": np.full((rows, 8), SENT, np.float64)}
        p = lambda k: None if null == k else rt._iptr(bufs[k])
        if name == "dereverb":
            bufs["wav"] = np.full((rows, max(T_or_L, 1)), SENT, np.float32)
            bufs["out"] = np.full((rows, max(T_or_L, 1)), SENT, np.float32)
            rc = lib.mt2_dereverb(None, None, C.byref(ac), C.byref(wc), p("wav"), rt._iptr(lens), T_or_L, n, p("fig"),
                                  p("wav") if overlap == "out" else p("out"), T_or_L if Lout is None else Lout)
        else:
            bufs["spec"] = np.full((rows, 4, S), SENT, np.float32)
            bufs["out"] = np.full((rows, 4, S), SENT, np.float32)
            bufs["filt"] = np.full((rows, Fp, 16, 2), SENT, np.float64)
            out = p("spec") if in_place else p("out")
            rc = lib.mt2_wpe_spectrum(None, None, C.byref(ac), C.byref(wc), p("spec"), rt._iptr(lens), T_or_L, n, out,
                                      p("spec") if overlap == "filt" else p("filt"), p("filt") if overlap == "fig" else p("fig"))
        assert rc != 0 and all((v == SENT).all() for v in bufs.values())
        return lib.mt2_last_error().decode()

    for name, lens, size in (("dereverb", [8000, 4000], 8000), ("wpe_spectrum", [4, 2], 4)):
        assert "null model handle" in run(name, lens, size)
        assert "delay" in run(name, lens, size, cfg=rt.Dereverb(delay=0))
        assert "taps" in run(name, lens, size, cfg=rt.Dereverb(taps=17))
        assert "iterations" in run(name, lens, size, cfg=rt.Dereverb(iterations=9))
        assert "context" in run(name, lens, size, cfg=rt.Dereverb(context=5))
        assert "variance_floor" in run(name, lens, size, cfg=rt.Dereverb(variance_floor=math.nan))
        assert "loading" in run(name, lens, size, cfg=rt.Dereverb(loading=0.5))
        assert "reserved" in run(name, lens, size, reserved=1)
        assert "B outside" in run(name, lens, size, B=0)
    assert "overlapping" in run("dereverb", [8000, 4000], 8000, overlap="out")
    assert "fewer frames" in run("dereverb", [8000, 767], 8000)
    assert "outside [1, L_max]" in run("dereverb", [8000, 8001], 8000)
    assert "MAX_FRAMES" in run("dereverb", [16384 * 256], 16384 * 256, Lout=1)
    assert "Lout_max" in run("dereverb", [8000, 4000], 8000, Lout=7935)
    assert "bad buffers" in run("dereverb", [8000], 8000, null="wav")
    assert "bad buffers" in run("dereverb", [8000], 8000, null="out")
    assert "overlapping" in run("wpe_spectrum", [4, 2], 4, overlap="filt")
    assert "overlapping" in run("wpe_spectrum", [4, 2], 4, overlap="fig")
    assert "null model handle" in run("wpe_spectrum", [4, 2], 4, in_place=True)      # spec_out may BE spec: the checks pass
    assert "frame count" in run("wpe_spectrum", [4, 5], 4)
    assert "frame count" in run("wpe_spectrum", [0, 4], 4)
    assert "T_max" in run("wpe_spectrum", [4], 0)
    assert "T_max" in run("wpe_spectrum", [4], 16385)
    assert "bad buffers" in run("wpe_spectrum", [4], 4, null="spec")
    assert "spec_out" in run("wpe_spectrum", [4], 4, null="out")
