"""The formant kernels on the GPU (csrc/formants.hip: mt2_lpc_formants, mt2_formant_stats) against the restatement of their rule
(tests/formant_ref.py) and against ground truth: the impulse response of a known all-pole filter comes back with its own poles.

Bars.  autocorr: every r[t, k] within W * 2^-52 * sum |terms| of the restatement - twice the bound (W - 1) 2^-53 sum |terms| of a W-term
double sum in ANY order, one for each side.  lpc and err: BIT-EQUAL to the restatement's Levinson recursion run on the device's own
autocorr.  roots: within 1e-11 of the restatement's roots of the device's own lpc, matched one for one; iters equal or one apart.  count:
equal wherever the restatement finds no candidate within 1e-6 (relative) of a keep / drop threshold or of another candidate.  freq and
bw: within one f32 ulp (2^-23 relative) of the restatement's doubles plus what 1e-11 on a root is in Hz (4e-12 sample_rate, for the |z|
> 0.8 that a bandwidth under 1 kHz means).  Ground truth: the bars of tests/test_formants_host.py.  Figures: n exact, the rest within
T * 2^-52 relative.
Observed on an MI355X over the 30 cases of test_against_the_restatement (1337 frames): autocorr at 0.0053 of its bound at worst; iters
equal in all 1313 frames that converge, one apart in none; roots 5.7e-14 apart at worst; count, freq and bw compared on 932 frames.  The
recovery sets: 2.2e-6 (frequency) and 6.2e-5 (bandwidth) at worst.  The voiced case: F1 763.7 Hz, 0.82 % from the 7th harmonic; F2 - F4
1.94 / 0.25 / 0.55 % from the truth.

In every case the input padding beyond lens[b] is NaN (a read of it empties a frame that must not be empty), the outputs are wider than
needed (frames in [T_b, T_max) must come back as zeros), pre-filled with a sentinel, and followed by guard words."""
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import formant_ref as F

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT, ISENT, GUARD = -77.25, -7777, 11
WINDOWS = (64, 66, 256, 550, 1022, 1024)
ORDERS = (2, 8, 10, 12, 32)
OUTS = ("freq", "bw", "count", "lpc", "err", "autocorr", "roots", "iters")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


def lengths(hop, W):
    return (1, hop - 1, hop, W // 2 - 1, W // 2, W // 2 + 1, W, 3 * W + 7, 5000)


@functools.lru_cache(maxsize=None)
def rows_for(hop, W):
    """one utterance of every length: noise at several levels, the longest a voiced signal"""
    rows = []
    for n, L in enumerate(lengths(hop, W)):
        x = F.voiced_signal(5000) if L == 5000 else F.noise_signal(L, 100 + n, scale=0.3 * 0.1 ** (n % 3))
        x.setflags(write=False)
        rows.append(x)
    return tuple(rows)


class Out:
    pass


def run(rows, sr=11000, hop=176, W=550, P=10, kind=F.HANN, pre=50.0, fmin=50.0, max_bw=500.0, extra_L=7, extra_T=3, extras=True,
        expect_error=False, lens=None, B=None, T_w=None, L_max=None, reserved=0, fe=None, overlap=None, null=(), shift=None):
    """mt2_lpc_formants on the utterances `rows` as one batch, into sentinel-filled buffers with guard words behind them -> Out with
    freq, bw [B, T_w, 5], count, iters [B, T_w], lpc, autocorr [B, T_w, P + 1], err [B, T_w], roots complex [B, T_w, P] (numpy; the
    last five None without `extras`), T [B]"""
    from megatts2_amd import runtime as rt
    fe = fe or frontend()
    nb = len(rows)
    ln = np.asarray([r.size for r in rows] if lens is None else lens, np.int32)
    host = np.full((nb, max(r.size for r in rows) + extra_L), np.nan, np.float32)
    for b, r in enumerate(rows):
        host[b, :r.size] = r
    wav = dev(host)
    if T_w is None:
        T_w = 1 + max(r.size for r in rows) // max(hop, 1) + extra_T
    n, Pn = nb * T_w, min(max(P, 0), 32)
    size = {"freq": 5 * n, "bw": 5 * n, "count": n, "lpc": n * (Pn + 1), "err": n, "autocorr": n * (Pn + 1), "roots": 2 * n * Pn, "iters": n}
    kinds = {"freq": torch.float32, "bw": torch.float32, "count": torch.int32, "iters": torch.int32}
    buf = {}
    for k in OUTS:
        if extras or k in ("freq", "bw", "count"):
            dt = kinds.get(k, torch.float64)
            buf[k] = torch.full((size[k] + GUARD,), ISENT if dt == torch.int32 else SENT, device="cuda", dtype=dt)
    cfg = rt.MT2FormantConfig(W, P, kind, reserved, pre, fmin, max_bw)
    p = {k: rt._ptr(buf.get(k)) for k in OUTS}
    p["wav"] = rt._ptr(wav)
    if overlap:
        p[overlap] = rt._ptr(wav)
    for k in null:                                             # a NULL where a buffer is required
        p[k] = None
    if shift:                                                  # (name, bytes): a buffer off its alignment
        p[shift[0]] = C.c_void_p((wav if shift[0] == "wav" else buf[shift[0]]).data_ptr() + shift[1])
    rc = fe.lib.mt2_lpc_formants(fe.h, rt._stream(), p["wav"], rt._iptr(ln), host.shape[1] if L_max is None else L_max,
                                 nb if B is None else B, sr, hop, C.byref(cfg), p["freq"], p["bw"], p["count"], T_w, p["lpc"], p["err"],
                                 p["autocorr"], p["roots"], p["iters"])
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in buf.items()}
    if expect_error:
        assert rc != 0
        msg = fe.lib.mt2_last_error().decode()
        for k, a in got.items():                               # a refused call leaves every output as it was
            assert (a == (ISENT if a.dtype == np.int32 else SENT)).all(), k
        assert np.array_equal(wav.cpu().numpy(), host, equal_nan=True)
        return msg
    assert rc == 0, fe.lib.mt2_last_error().decode()
    o = Out()
    o.T = 1 + ln // hop
    shape = {"freq": (nb, T_w, 5), "bw": (nb, T_w, 5), "count": (nb, T_w), "lpc": (nb, T_w, P + 1), "err": (nb, T_w),
             "autocorr": (nb, T_w, P + 1), "roots": (nb, T_w, P, 2), "iters": (nb, T_w)}
    for k in OUTS:
        a = got.get(k)
        if a is None:
            setattr(o, k, None)
            continue
        assert (a[size[k]:] == (ISENT if a.dtype == np.int32 else SENT)).all(), k
        setattr(o, k, a[:size[k]].reshape(shape[k]))
    for b in range(nb):                                        # frames behind the utterance's own: zeros everywhere
        for k in OUTS:
            a = getattr(o, k)
            assert a is None or not a[b, int(o.T[b]):].any(), k
    if o.roots is not None:
        o.roots = o.roots[..., 0] + 1j * o.roots[..., 1]
    return o


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.complex128).view(np.int64) if np.iscomplexobj(a) else a.view({4: np.int32, 8: np.int64}[a.dtype.itemsize])


SEEN = {"equal": 0, "one apart": 0, "frames": 0, "roots": 0.0, "autocorr": 0.0, "count checked": 0}


def check_against_restatement(o, rows, sr, hop, W, P, kind, pre, fmin, max_bw):
    for b, x in enumerate(rows):
        T = int(o.T[b])
        ref = F.analyse(x, sr, hop, W, P, pre, fmin, max_bw, kind)
        assert ref["autocorr"].shape == (T, P + 1)
        # step 4 within the bound of a W-term sum in any order
        r = o.autocorr[b, :T]
        assert np.isfinite(r).all()
        bound = W * 2.0 ** -52 * ref["mag"] * (1 + 1e-9)
        err = np.abs(r - ref["autocorr"])
        assert (err <= bound).all(), (b, x.size)
        SEEN["autocorr"] = max(SEEN["autocorr"], float(np.max(err / np.maximum(bound, 1e-300))))
        # steps 5-7 from the device's own r: Levinson to the bit
        fin = F.finish(r, sr, fmin, max_bw)
        assert np.array_equal(bits(o.lpc[b, :T]), bits(fin["lpc"])), (b, x.size)
        assert np.array_equal(bits(o.err[b, :T]), bits(fin["err"])), (b, x.size)
        for t in range(T):
            it, dit = int(fin["iters"][t]), int(o.iters[b, t])
            SEEN["frames"] += 1
            if it < 0:
                assert dit == -1 and o.count[b, t] == 0 and not o.freq[b, t].any() and not o.bw[b, t].any() and not o.roots[b, t].any()
                continue
            assert abs(dit - it) <= 1 and dit > 0, (b, t, it, dit)
            SEEN["equal" if dit == it else "one apart"] += 1
            d = np.abs(o.roots[b, t][:, None] - fin["roots"][t][None, :])
            assert sorted(d.argmin(axis=1)) == list(range(P)) and d.min(axis=1).max() < 1e-11, (b, t, d.min(axis=1).max())
            SEEN["roots"] = max(SEEN["roots"], float(d.min(axis=1).max()))
            if fin["near"][t]:
                continue
            SEEN["count checked"] += 1
            c = int(fin["count"][t])
            assert o.count[b, t] == c, (b, t)
            for got, want in ((o.freq[b, t], fin["freq"][t]), (o.bw[b, t], fin["bw"][t])):
                assert not got[c:].any()
                assert (np.abs(got[:c].astype(np.float64) - want[:c]) <= 2.0 ** -23 * np.abs(want[:c]) + 4e-12 * sr).all(), (b, t, got, want)


CASES = [(W, P, i) for i, (W, P) in enumerate(itertools.product(WINDOWS, ORDERS)) if P < W]


@pytest.mark.parametrize("W, P, i", CASES)
def test_against_the_restatement(W, P, i):
    """every window with every order; hop, window kind and pre-emphasis cycle so that each of their eight combinations meets several"""
    hop, kind, pre = (176, 256)[i % 2], (F.HANN, F.RECT)[(i // 2) % 2], (50.0, 0.0)[(i // 4) % 2]
    sr = 11000 if hop == 176 else 16000
    rows = rows_for(hop, W)
    o = run(rows, sr, hop, W, P, kind, pre)
    check_against_restatement(o, rows, sr, hop, W, P, kind, pre, 50.0, 500.0)
    print(f"W {W} P {P} hop {hop} kind {kind} pre {pre}: {SEEN}")


def test_hop_one():
    rows = (F.noise_signal(40, 7), F.noise_signal(1, 8))
    o = run(rows, 8000, 1, 64, 8, F.HANN, 50.0)
    assert list(o.T) == [41, 2]
    check_against_restatement(o, rows, 8000, 1, 64, 8, F.HANN, 50.0, 50.0, 500.0)


def test_a_batch_is_its_rows_alone():
    rows = rows_for(176, 550)
    whole = run(rows)
    for b, x in enumerate(rows):
        alone = run((x,), extra_L=b, extra_T=b % 3)
        T = int(whole.T[b])
        assert alone.T[0] == T
        for k in OUTS:
            assert np.array_equal(bits(getattr(whole, k)[b, :T]), bits(getattr(alone, k)[0, :T])), (k, x.size)


@pytest.mark.parametrize("pre", [50.0, 0.0])
def test_non_finite_samples_empty_their_frames_alone(pre):
    hop, W = 176, 550
    clean = F.noise_signal(3000, 21)
    rows, at = [clean], [None]
    for pos, bad in ((1500, np.nan), (700, np.inf), (0, -np.inf), (2999, np.nan)):
        x = clean.copy()
        x[pos] = bad
        rows.append(x)
        at.append(pos)
    rows.append(np.zeros(3000, np.float32))
    o = run(rows, pre=pre)
    T = int(o.T[0])
    assert (o.iters[0, :T] > 0).all()
    s = hop * np.arange(T) - W // 2
    for b in range(1, len(at)):
        reads = (s - (1 if pre else 0) <= at[b]) & (at[b] < s + W)          # step 2: with pre-emphasis a frame reads x[s - 1] as well
        assert reads.any() and not reads.all()
        assert (o.count[b, :T][reads] == 0).all() and (o.iters[b, :T][reads] == -1).all()
        assert not o.freq[b, :T][reads].any() and not o.bw[b, :T][reads].any() and not o.roots[b, :T][reads].any()
        for k in OUTS:
            assert np.array_equal(bits(getattr(o, k)[b, :T][~reads]), bits(getattr(o, k)[0, :T][~reads])), (k, at[b])
    z = len(rows) - 1
    assert (o.count[z, :T] == 0).all() and (o.iters[z, :T] == -1).all()
    for k in OUTS:
        if k != "iters":
            assert not getattr(o, k)[z].any(), k


@pytest.mark.parametrize("case", range(len(F.RECOVERY_SETS)))
def test_exact_recovery_on_the_device(case):
    sr, poles, max_bw = F.RECOVERY_SETS[case]
    y = F.recovery_signal(sr, poles).astype(np.float32)
    o = run((y,), sr, F.RECOVERY_HOP, F.RECOVERY_W, 2 * len(poles), F.RECT, 0.0, 50.0, max_bw)
    t, n = F.RECOVERY_FRAME, len(poles)
    assert o.iters[0, t] > 0 and o.count[0, t] == min(n, F.MAX)
    z = o.roots[0, t]
    z = z[z.imag > 0]
    z = z[np.argsort(np.angle(z))]
    assert z.size == n
    f, bw = np.angle(z) * sr / (2 * np.pi), -np.log(np.abs(z)) * sr / np.pi
    tf, tb = np.array([p[0] for p in poles], float), np.array([p[1] for p in poles], float)
    ef, eb = np.max(np.abs(f - tf) / tf), np.max(np.abs(bw - tb) / tb)
    print(f"set {case}: frequency {ef:.3g}, bandwidth {eb:.3g}")
    assert ef < 1e-5 and eb < 2e-4
    # and what the call writes out: the first five, rounded to f32
    k = min(n, F.MAX)
    assert np.allclose(o.freq[0, t, :k], f[:k], rtol=2.0 ** -23, atol=0) and np.allclose(o.bw[0, t, :k], bw[:k], rtol=2.0 ** -23, atol=0)


def test_default_settings_on_a_voiced_signal_on_the_device():
    x = F.voiced_signal()
    v = F.VOICED
    o = run((x,), F.VOICED_SR, v["hop"], v["W"], v["P"], v["kind"], v["pre_hz"], v["fmin"], v["max_bw"])
    T = int(o.T[0])
    inner = F.interior(v["hop"] * np.arange(T) - v["W"] // 2, v["W"], x.size)
    assert inner.sum() > 20 and (o.count[0, :T][inner] >= 4).all()
    f = o.freq[0, :T][inner][:, :4].astype(np.float64)
    truth = np.array([p[0] for p in F.VOICED_POLES], float)
    lock = np.max(np.abs(f[:, 0] - 770.0) / 770.0)
    err = np.max(np.abs(f[:, 1:] - truth[None, 1:]) / truth[None, 1:], axis=0)
    print(f"F1 {f[:, 0].mean():.1f} Hz, within {100 * lock:.2f} % of 770; F2-F4 off by {100 * err} %")
    assert lock < 0.02 and err[0] < 0.03 and err[1] < 0.01 and err[2] < 0.01


# ---- mt2_formant_stats -----------------------------------------------------------------------------------------------------------------
def stats_call(freq, count, f0, lens, expect_error=False, T=None, B=None, overlap=None, null=(), shift=None):
    from megatts2_amd import runtime as rt
    fe = frontend()
    nb, Tn = count.shape
    ln = np.asarray(lens, np.int32)
    d = {"freq": dev(freq), "count": dev(count), "f0": None if f0 is None else dev(f0)}
    st = torch.full((nb * F.STAT_FIELDS + GUARD,), SENT, device="cuda", dtype=torch.float64)
    p = {"freq": rt._ptr(d["freq"]), "count": rt._ptr(d["count"]), "f0": rt._ptr(d["f0"]), "stats": rt._ptr(d[overlap]) if overlap else rt._ptr(st)}
    for k in null:
        p[k] = None
    if shift:
        p[shift[0]] = C.c_void_p((st if shift[0] == "stats" else d[shift[0]]).data_ptr() + shift[1])
    rc = fe.lib.mt2_formant_stats(fe.h, rt._stream(), p["freq"], p["count"], p["f0"], rt._iptr(ln), Tn if T is None else T,
                                  nb if B is None else B, p["stats"])
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    if expect_error:
        assert rc != 0 and (got == SENT).all()
        for k, a in (("freq", freq), ("count", count), ("f0", f0)):
            assert a is None or np.array_equal(d[k].cpu().numpy(), a, equal_nan=True), k
        return fe.lib.mt2_last_error().decode()
    assert rc == 0, fe.lib.mt2_last_error().decode()
    assert (got[nb * F.STAT_FIELDS:] == SENT).all()
    return got[:nb * F.STAT_FIELDS].reshape(nb, F.STAT_FIELDS)


def stats_rows(seed=5):
    rng = np.random.default_rng(seed)
    lens = np.array([1, 63, 64, 65, 257, 1030, 40, 30], np.int32)
    nb, T = lens.size, int(lens.max()) + 2
    freq = np.full((nb, T, 5), np.nan, np.float32)
    count = np.full((nb, T), 5, np.int32)
    f0 = np.full((nb, T), np.nan, np.float32)
    for b, n in enumerate(lens):
        freq[b, :n] = np.sort(rng.uniform(200.0, 5000.0, (n, 5)), axis=1)
        count[b, :n] = rng.integers(0, 6, n)
        f0[b, :n] = np.where(rng.random(n) < 0.6, rng.uniform(80.0, 300.0, n), 0.0)
    count[6, :40] = 3                                          # n = 0 by the counts
    f0[7, :30] = 0.0                                           # n = 0 by the voicing (with f0)
    return freq, count, f0, lens


@pytest.mark.parametrize("voiced", [False, True])
def test_stats_against_float64(voiced):
    freq, count, f0, lens = stats_rows()
    got = stats_call(freq, count, f0 if voiced else None, lens)
    for b, n in enumerate(lens):
        ref = F.stats(freq[b], count[b], f0[b] if voiced else None, n)
        assert got[b, 0] == ref[0], b
        if ref[0] == 0:
            assert not got[b].any()
            continue
        assert (np.abs(got[b] - ref) <= int(n) * 2.0 ** -52 * np.abs(ref)).all(), (b, got[b], ref)
    assert not got[6].any() and (not voiced or not got[7].any())


def test_stats_of_the_neutral_tube():
    freq = np.tile(np.array([500, 1500, 2500, 3500, 4500], np.float32), (2, 9, 1))
    got = stats_call(freq, np.full((2, 9), 4, np.int32), None, [9, 4])
    for b, n in enumerate((9, 4)):
        assert got[b, 0] == n and got[b, 1] == 1.0 and got[b, 11] == 17.5 and got[b, 10] == 1000.0
        assert (got[b, 2:6] == [500, 1500, 2500, 3500]).all() and not got[b, 6:10].any()


# ---- refusals, and the arena -----------------------------------------------------------------------------------------------------------
def test_refusals_leave_the_outputs_alone():
    rows = (F.noise_signal(4000, 1), F.noise_signal(2000, 2))
    nan, inf = float("nan"), float("inf")
    for kw, word in ((dict(B=0), "B outside"), (dict(B=65536), "B outside"), (dict(lens=(4000, 0)), "length outside"),
                     (dict(lens=(4000, 4008)), "length outside"), (dict(sr=0), "sample_rate"), (dict(hop=0), "hop outside"),
                     (dict(hop=1025), "hop outside"), (dict(W=62), "window outside"), (dict(W=1026), "window outside"),
                     (dict(W=551), "window outside"), (dict(P=0), "order outside"), (dict(P=34), "order outside"), (dict(P=11), "order outside"),
                     (dict(kind=2), "kind"), (dict(reserved=1), "reserved"), (dict(pre=-1.0), "preemphasis_hz"), (dict(pre=nan), "preemphasis_hz"),
                     (dict(pre=inf), "preemphasis_hz"), (dict(fmin=-1.0), "fmin_hz"), (dict(fmin=nan), "fmin_hz"), (dict(fmin=inf), "fmin_hz"),
                     (dict(max_bw=-1.0), "max_bandwidth_hz"), (dict(max_bw=nan), "max_bandwidth_hz"), (dict(max_bw=inf), "max_bandwidth_hz"),
                     (dict(fmin=2750.0), "fmin_hz >= sample_rate / 4"), (dict(T_w=1 + 4000 // 176 - 1), "T_max smaller"),
                     (dict(overlap="freq"), "overlapping"), (dict(overlap="roots"), "overlapping"), (dict(overlap="iters"), "overlapping"),
                     (dict(null=("wav",)), "bad buffers"), (dict(null=("freq",)), "bad buffers"), (dict(null=("bw",)), "bad buffers"),
                     (dict(null=("count",)), "bad buffers"), (dict(shift=("wav", 2)), "misaligned"), (dict(shift=("freq", 2)), "misaligned"),
                     (dict(shift=("count", 1)), "misaligned"), (dict(shift=("lpc", 4)), "misaligned"), (dict(shift=("roots", 4)), "misaligned")):
        assert word in run(rows, expect_error=True, **kw), kw
    freq, count, f0, lens = stats_rows()
    for kw, word in ((dict(B=0), "B outside"), (dict(B=65536), "B outside"), (dict(T=0), "bad buffers"), (dict(T=1029), "frame count outside"),
                     (dict(overlap="freq"), "overlaps"), (dict(overlap="count"), "overlaps"), (dict(overlap="f0"), "overlaps"),
                     (dict(null=("freq",)), "bad buffers"), (dict(null=("count",)), "bad buffers"), (dict(null=("stats",)), "bad buffers"),
                     (dict(shift=("freq", 2)), "misaligned"), (dict(shift=("f0", 1)), "misaligned"), (dict(shift=("stats", 4)), "misaligned")):
        assert word in stats_call(freq, count, f0, lens, expect_error=True, **kw), kw
    bad = lens.copy()
    bad[0] = 0
    assert "frame count outside" in stats_call(freq, count, f0, bad, expect_error=True)


def test_the_arena_is_the_querys():
    from megatts2_amd import runtime as rt
    fe = rt.MelFrontEnd()
    try:
        assert fe.workspace_high_water() == 0
        for rows, kw in (((F.noise_signal(900, 1),), dict(extras=False)), (rows_for(176, 550), dict(extras=True))):
            run(rows, fe=fe, **kw)
            assert fe.workspace_high_water() == rt.formant_query(5000)[1] == (4 * 65535 + 255) // 256 * 256
    finally:
        fe.close()
