"""The second F0 tracker on the GPU (csrc/f0.hip: mt2_f0_track, a Viterbi pass over YIN's lag costs) against the restatement of its
rule (tests/f0_track_ref.py) and against ground truth.

Bars.  lag, cmnd and f0 BIT-EQUAL to the float32 restatement (one numpy float32 operation at a time) run on the kernel's own d, at
every length, hop, lag range (2, 63, 64, 65, 225 and 255 states) and both jump costs.  Tones and the H signals (even harmonics
dominant: plain YIN an octave high): interior frames voiced and within 1 cent of the truth, lag paths equal to the float64
restatement's on float64 d.  A ragged batch bit-identical to its utterances alone.

In every case the input padding beyond lens[b] is NaN, the outputs are wider than needed (frames in [T_b, T_max) must come back as
mt2_f0_yin writes them: f0 0, cmnd 1, lag 0, d 0), pre-filled with a sentinel, and followed by guard words.

The NaN case: f0 is finite everywhere and every lag lies in [tau_min, tau_max]; cmnd is d'[t, tau*] by the rule, which IS a NaN in a
frame whose window holds the NaN sample, so cmnd is held finite on the other frames only."""
import ctypes as C
import functools

import numpy as np
import pytest

import f0_ref as R
import f0_track_ref as V

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT, ISENT, GUARD = np.float32(-77.25), -7777, 11
SHORT = (1, 255, 256, 257, 1500, 4000, 8000)
HOPS = (256, 80)
# (fmin, fmax) -> states; each asserted through mt2_f0_query below
RANGES = {2: (5333.0, 8000.0), 63: (240.6, 4000.0), 64: (237.0, 4000.0), 65: (233.6, 4000.0), 225: (62.5, 500.0), 255: (62.5, 8000.0)}


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()          # a copy: the cached signals are read-only


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


@functools.lru_cache(maxsize=None)
def signal(key):
    kind = key[0]
    if kind == "tone":
        _, f, harm, L = key
        return R.tone(f, L, R.HARMONICS[harm], seed=int(f) + harm)
    if kind == "H":
        return V.H(key[1], key[2])
    if kind == "noise":
        return R.white(key[2], key[1], seed=3)
    if kind == "zeros":
        x = np.zeros(key[1], np.float32)
        x.setflags(write=False)
        return x
    if kind == "mixed":
        return R.mixed()
    raise KeyError(key)


@functools.lru_cache(maxsize=None)
def path64(key):
    """the float64 restatement's lag path on float64 d, computed once"""
    return V.viterbi_track(signal(key))[2]


SHORT_KEYS = tuple(("tone", 220.5, 1, L) for L in SHORT)
TONE_KEYS = tuple(("tone", f, h, 8000) for f in R.FREQS for h in range(len(R.HARMONICS)))
H_KEYS = tuple(("H", f, a) for a in V.H_WEAK for f in V.H_FREQS)
REPLAY_KEYS = SHORT_KEYS + (("tone", 493.9, 2, 8000), ("tone", 110.0, 2, 8000), ("noise", 0.1, 8000), ("zeros", 4000), ("mixed",),
                            ("H", 146.83, 0.3))


class Out:
    pass


def run(rows, hop=256, fmin=62.5, fmax=500.0, thr=0.15, oc=V.OCTAVE_COST, jc=V.JUMP_COST, extra_L=7, extra_T=3, extras=True,
        expect_error=False, wav=None, lens=None, T_w=None):
    """mt2_f0_track on the utterances `rows` as one batch, into sentinel-filled buffers with guard words behind them -> Out with
    f0, cmnd [B, T_w], lag [B, T_w], diff [B, T_w, 257] (numpy; None without `extras`), T [B]"""
    from megatts2_amd import runtime
    fe = frontend()
    if wav is None:
        B, lens = len(rows), np.asarray([r.size for r in rows], np.int32)
        host = np.full((B, int(lens.max()) + extra_L), np.nan, np.float32)
        for b, r in enumerate(rows):
            host[b, :r.size] = r
        wav = dev(host)
    B, L_max = wav.shape
    lens = np.asarray(lens, np.int32)
    if T_w is None:
        T_w = 1 + int(lens.max()) // hop + extra_T
    n = B * T_w
    f0 = torch.full((n + GUARD,), float(SENT), device="cuda", dtype=torch.float32)
    cmnd = torch.full((n + GUARD,), float(SENT), device="cuda", dtype=torch.float32) if extras else None
    lag = torch.full((n + GUARD,), ISENT, device="cuda", dtype=torch.int32) if extras else None
    diff = torch.full((n * 257 + GUARD,), float(SENT), device="cuda", dtype=torch.float32) if extras else None
    rc = fe.lib.mt2_f0_track(fe.h, runtime._stream(), runtime._ptr(wav), runtime._iptr(lens), L_max, B, 16000, hop, C.c_float(fmin),
                             C.c_float(fmax), C.c_float(thr), C.c_float(oc), C.c_float(jc), runtime._ptr(f0), runtime._ptr(cmnd),
                             runtime._ptr(lag), T_w, runtime._ptr(diff))
    torch.cuda.synchronize()
    bufs = [t.cpu().numpy() for t in (f0, cmnd, lag, diff) if t is not None]
    if expect_error:
        assert rc != 0 and fe.lib.mt2_last_error()
        for a in bufs:                                        # a refused call leaves every output as it was
            assert (a == (ISENT if a.dtype == np.int32 else SENT)).all()
        return None
    assert rc == 0, fe.lib.mt2_last_error().decode()
    o = Out()
    o.T = 1 + lens // hop
    o.f0 = bufs[0][:n].reshape(B, T_w)
    assert (bufs[0][n:] == SENT).all()
    o.cmnd = o.lag = o.diff = None
    if extras:
        o.cmnd, o.lag, o.diff = bufs[1][:n].reshape(B, T_w), bufs[2][:n].reshape(B, T_w), bufs[3][:n * 257].reshape(B, T_w, 257)
        assert (bufs[1][n:] == SENT).all() and (bufs[2][n:] == ISENT).all() and (bufs[3][n * 257:] == SENT).all()
    for b in range(B):                                        # frames behind the utterance's own: as mt2_f0_yin writes them
        t = int(o.T[b])
        assert not o.f0[b, t:].any()
        if extras:
            assert (o.cmnd[b, t:] == 1).all() and not o.lag[b, t:].any() and not o.diff[b, t:].any()
    return o


def assert_is_the_restatement(o, B, fmin, fmax, thr, oc, jc):
    """every utterance of o against the float32 restatement on the kernel's own d"""
    for b in range(B):
        T = int(o.T[b])
        f0, cmnd, lag = V.track(o.diff[b, :T], R.SR, fmin, fmax, thr, oc, jc, dtype=np.float32)
        assert o.f0.dtype == o.cmnd.dtype == np.float32
        assert np.array_equal(o.lag[b, :T], lag), (b, np.nonzero(o.lag[b, :T] != lag)[0][:8])
        assert np.array_equal(o.cmnd[b, :T].view(np.uint32), cmnd.view(np.uint32)), b
        assert np.array_equal(o.f0[b, :T].view(np.uint32), f0.view(np.uint32)), b


# ---- 1. bit equality with the float32 restatement on the kernel's own d -------------------------------------------------------------

@pytest.mark.parametrize("jc", (0.0, 0.5))
@pytest.mark.parametrize("states", sorted(RANGES))
@pytest.mark.parametrize("hop", HOPS)
def test_track_is_the_float32_restatement_on_the_kernels_d(hop, states, jc):
    from megatts2_amd import runtime
    fmin, fmax = RANGES[states]
    _, lo, hi, _ = runtime.f0_query(8000, hop=hop, fmin=fmin, fmax=fmax)
    assert hi - lo + 1 == states and (lo, hi) == R.lags(R.SR, fmin, fmax)
    assert runtime.f0_track_query(8000, hop=hop, fmin=fmin, fmax=fmax)[1:4] == (lo, hi, states)
    if states == 255:
        assert (lo, hi) == (2, 256)
    rows = [signal(k) for k in REPLAY_KEYS]
    o = run(rows, hop, fmin, fmax, jc=jc)
    assert_is_the_restatement(o, len(rows), fmin, fmax, 0.15, V.OCTAVE_COST, jc)
    assert ((o.lag[0, :1] >= lo) & (o.lag[0, :1] <= hi)).all()
    if states == 225:
        assert (o.f0 > 0).any() and (o.f0[:, 0] == 0).any()


@pytest.mark.parametrize("jc", (0.0, 0.5))
def test_ties_take_the_smallest_state(jc):
    """silence with octave_cost 0: every o is 1, every predecessor ties - the smallest state wins throughout"""
    o = run([signal(("zeros", 4000)), signal(("zeros", 1500))], oc=0.0, jc=jc)
    for b in range(2):
        T = int(o.T[b])
        assert (o.lag[b, :T] == 32).all() and (o.cmnd[b, :T] == 1).all() and not o.f0[b].any()
    assert_is_the_restatement(o, 2, 62.5, 500.0, 0.15, 0.0, jc)


# ---- 2. ground truth and the float64 paths ------------------------------------------------------------------------------------------

def test_tones_are_within_a_cent_of_the_truth():
    o = run([signal(k) for k in TONE_KEYS])
    inner = R.interior(8000)
    worst = 0.0
    for b, k in enumerate(TONE_KEYS):
        got = o.f0[b, inner]
        assert (got > 0).all() and (o.cmnd[b, inner] < 0.15).all(), k
        worst = max(worst, float(np.abs(R.cents(got, k[1])).max()))
        assert np.array_equal(o.lag[b, :32], path64(k)), k
    print(f"tones: worst {worst:.3g} cents from the truth")
    assert worst <= 1.0


def test_dominant_even_harmonics_are_within_a_cent_of_the_truth():
    o = run([signal(k) for k in H_KEYS])
    inner = R.interior(16000)
    worst = 0.0
    for b, k in enumerate(H_KEYS):
        got = o.f0[b, inner]
        assert (got > 0).all() and (o.cmnd[b, inner] < 0.15).all(), k
        worst = max(worst, float(np.abs(R.cents(got, k[1])).max()))
        assert np.array_equal(o.lag[b, :63], path64(k)), k
    print(f"H signals: worst {worst:.3g} cents from the truth")
    assert worst <= 1.0


# ---- 3. batch identity and the optional outputs -------------------------------------------------------------------------------------

def test_ragged_batch_is_its_utterances_alone():
    keys = (("tone", 220.5, 1, 1), ("tone", 220.5, 1, 1500), ("tone", 220.5, 1, 4000), ("mixed",))
    rows = [signal(k) for k in keys]
    assert [r.size for r in rows] == [1, 1500, 4000, 16000]
    o = run(rows)
    fields = ("f0", "cmnd", "lag", "diff")
    again = run(rows)                                         # repetition
    wider = run(rows, extra_L=20, extra_T=9)                  # L_max and T_max
    turned = run(rows[::-1])                                  # the slot
    for b, r in enumerate(rows):
        T = int(o.T[b])
        alone = run([r])
        for name in fields:
            want = getattr(o, name)[b, :T]
            for other, slot in ((again, b), (wider, b), (turned, len(rows) - 1 - b), (alone, 0)):
                assert np.array_equal(want, getattr(other, name)[slot, :T], equal_nan=False), (name, b)


def test_optional_outputs_do_not_change_f0():
    rows = [signal(k) for k in REPLAY_KEYS]
    o = run(rows)
    bare = run(rows, extras=False)
    assert np.array_equal(bare.f0.view(np.uint32), o.f0.view(np.uint32))


# ---- 4. a NaN sample -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hop", HOPS)
def test_a_nan_sample_cannot_move_a_lag_out_of_range(hop):
    x = signal(("tone", 146.83, 1, 8000))
    y = x.copy()
    y[4000] = np.nan
    o = run([x, y], hop)                                      # the guard words behind every output are checked in run()
    T = int(o.T[0])
    clean = np.array([not (hop * t - 512 <= 4000 < hop * t + 512) for t in range(T)])
    assert 0 < clean.sum() < T and np.isnan(o.diff[1, :T][~clean]).any()
    assert np.isfinite(o.f0).all() and np.isfinite(o.cmnd[0]).all() and np.isfinite(o.cmnd[1, :T][clean]).all()
    assert ((o.lag[:, :T] >= 32) & (o.lag[:, :T] <= 256)).all()
    assert_is_the_restatement(o, 2, 62.5, 500.0, 0.15, V.OCTAVE_COST, V.JUMP_COST)


def test_arena_high_water_is_the_querys_figure():
    """B = 2 with lengths (4000, 2500) at hop 256: T = 16; the first call of a fresh handle takes what mt2_f0_track_query says"""
    from megatts2_amd import runtime as rt
    fe = rt.MelFrontEnd()
    try:
        assert fe.workspace_high_water() == 0
        wav = torch.zeros(2, 4000, device="cuda", dtype=torch.float32)
        wav[0].copy_(dev(signal(("tone", 220.5, 1, 4000))))
        wav[1, :2500].copy_(dev(signal(("tone", 220.5, 1, 4000))[:2500]))
        f0 = fe.f0_track(wav, lens=[4000, 2500], hop=256)
        torch.cuda.synchronize()
        assert f0.shape == (2, 16)
        assert fe.workspace_high_water() == rt.f0_track_query(4000, 2)[4]
    finally:
        fe.close()


# ---- 5. refusals ---------------------------------------------------------------------------------------------------------------------

def test_device_call_rejects_before_launch():
    base = torch.full((2 * 3000 + 4000,), 0.0, device="cuda", dtype=torch.float32)
    wav = base[:6000].view(2, 3000)
    wav.copy_(dev(np.stack([signal(("tone", 220.5, 1, 4000))[:3000], signal(("tone", 110.0, 2, 8000))[:3000]])))
    ok = dict(wav=wav, lens=[3000, 2000])

    def refused(**kw):
        assert run(None, expect_error=True, **{**ok, **kw}) is None

    refused(lens=[3000, 0])
    refused(lens=[3001, 3000])
    refused(lens=[3000, -1])
    for hop in (0, -1, 1025):
        refused(hop=hop, T_w=40)
    for f in (0.0, -1.0, float("nan"), float("inf")):
        refused(fmin=f)
        refused(fmax=f)
    refused(fmin=62.0)                                        # tau_max = 258
    refused(fmax=16000.0)                                     # tau_min = 1
    refused(fmin=400.0, fmax=80.0)                            # tau_min > tau_max
    refused(fmin=500.0, fmax=500.0)                           # tau_min == tau_max
    for thr in (0.0, -0.1, 1.0001, float("nan")):
        refused(thr=thr)
    for cost in (-0.01, float("nan"), float("inf"), float("-inf")):
        refused(oc=cost)
        refused(jc=cost)
    refused(T_w=1 + 3000 // 256 - 1)
    refused(hop=80, T_w=1 + 3000 // 80 - 1)
    # B outside [1, 65535] and outputs overlapping the input: the C entry point itself
    from megatts2_amd import runtime
    fe = frontend()
    lens = np.asarray([3000, 2000], np.int32)

    def call(B, f0, cmnd=None, lag=None, diff=None, T_max=12):
        return fe.lib.mt2_f0_track(fe.h, runtime._stream(), runtime._ptr(wav), runtime._iptr(lens), 3000, B, 16000, 256, C.c_float(62.5),
                                   C.c_float(500.0), C.c_float(0.15), C.c_float(0.02), C.c_float(0.5), runtime._ptr(f0),
                                   runtime._ptr(cmnd), runtime._ptr(lag), T_max, runtime._ptr(diff))

    before = base.clone()
    out = torch.full((2, 12), float(SENT), device="cuda", dtype=torch.float32)
    spare = torch.full((2, 12, 257), float(SENT), device="cuda", dtype=torch.float32)
    assert call(0, out) != 0 and call(-1, out) != 0 and call(65536, out) != 0
    inside = base[2990:2990 + 24].view(2, 12)                 # lies in wav
    tail = base[5990:5990 + 24].view(2, 12)                   # starts in wav's last row
    for over in (inside, tail):
        assert call(2, over) != 0
        assert call(2, out, cmnd=over) != 0
        assert call(2, out, lag=over.view(torch.int32)) != 0
    assert call(2, out, diff=base[3000:3000 + 2 * 12 * 257].view(2, 12, 257)) != 0
    torch.cuda.synchronize()
    assert torch.equal(base, before) and (out == float(SENT)).all() and (spare == float(SENT)).all()
    assert call(2, out, diff=spare) == 0                      # and the same call with valid arguments goes through
    torch.cuda.synchronize()
    assert torch.equal(base, before) and not (out == float(SENT)).any() and not (spare == float(SENT)).any()


# ---- 6. the surface --------------------------------------------------------------------------------------------------------------------

def test_surface():
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime
    fe = M._frontend()
    x = signal(("H", 146.83, 0.3))
    o = run([x])
    f0, cmnd, lag, diff = fe.f0_track(dev(x[None]), return_cmnd=True, return_lag=True, return_diff=True)
    assert f0.shape == (1, 63) and diff.shape == (1, 63, 257) and lag.dtype == torch.int32
    for a, b in ((f0, o.f0), (cmnd, o.cmnd), (lag, o.lag), (diff, o.diff)):
        assert np.array_equal(a.cpu().numpy()[0], b[0, :63])
    assert torch.equal(fe.f0_track(dev(x[None])), f0)
    assert torch.equal(fe.f0_track(dev(x[None]), return_lag=True)[1], lag)
    assert torch.equal(fe.f0(dev(x[None]), return_diff=True)[1], diff)          # both trackers see the same d bits
    jumpy = fe.f0_track(dev(x[None]), jump_cost=0.0, octave_cost=0.0)
    assert np.array_equal(jumpy.cpu().numpy()[0], run([x], oc=0.0, jc=0.0).f0[0, :63])
    with pytest.raises(runtime.NativeError):
        fe.f0_track(dev(x[None]), jump_cost=-1.0)
    # plain YIN is an octave high on this signal, the tracker is not
    inner = R.interior(16000)
    plain = fe.f0(dev(x[None])).cpu().numpy()[0]
    assert (np.abs(R.cents(np.where(plain > 0, plain, 1e-9)[inner], 146.83)) > 50).sum() >= 25
    assert np.abs(R.cents(f0.cpu().numpy()[0][inner], 146.83)).max() <= 1.0
    # 44.1 kHz audio: silence, a tone, silence
    n = np.arange(22050)
    burst = (0.5 * np.sin(2 * np.pi * 196.0 * n / 44100) + 1e-3 * np.random.default_rng(4).standard_normal(n.size)).astype(np.float32)
    x44 = np.concatenate([np.zeros(9000, np.float32), burst, np.zeros(7000, np.float32)])
    y, y_lens = fe.resample(dev(x44[None]), 44100)
    got = M.extract_f0(x44, 44100, method="viterbi")
    assert got.dim() == 1 and torch.equal(got, fe.f0_track(y, y_lens)[0])
    assert got.shape[0] == M.extract_mel_spec(x44, 44100).shape[1]
    assert torch.equal(M.extract_f0(x44, 44100, method="viterbi", jump_cost=0.25, octave_cost=0.01),
                       fe.f0_track(y, y_lens, jump_cost=0.25, octave_cost=0.01)[0])
    assert torch.equal(M.extract_f0(x44, 44100), fe.f0(y, y_lens)[0])          # the default: plain YIN, as before
    assert torch.equal(M.extract_f0(x44, 44100, method="yin"), fe.f0(y, y_lens)[0])
    with pytest.raises(ValueError):
        M.extract_f0(x44, 44100, method="pyin")
    voiced = got.cpu().numpy() > 0
    assert voiced.any() and not voiced.all()
    st = M.pitch_stats(got)
    want = R.moments(got.cpu().numpy())
    assert np.allclose([st[k][0] for k in M.PITCH_STATS], want, rtol=1e-12, atol=0)
    assert np.allclose(fe.f0_stats(got[None]).cpu().numpy()[0], want, rtol=1e-12, atol=0)
    assert st["voiced_frames"][0] == voiced.sum() and abs(st["mean_hz"][0] - 196.0) < 1.0
