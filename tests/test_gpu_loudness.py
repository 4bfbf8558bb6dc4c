"""Integrated loudness and loudness normalisation on the GPU (csrc/loudness.hip: mt2_loudness, mt2_loudness_normalize) against the
float64 restatement of the rule (tests/loudness_ref.py) applied to the same f32 input, against the standard's own figure and the
analytic readings of sines, and on the tiny synthetic model.

Bars.  Momentary loudness: |l - l_ref| <= 10 log10(1 + 1e-10) = 4.34e-10 LU, which is relative 1e-10 in z - the CPU's chunked and
serial forms differ by 1.4e-14, the rest is room for the device's fma contraction and log10.  I and Gamma: 1e-8 LU.  The three counts
are EXACT, asserted only after the restatement shows no block within 1e-3 LU of either gate.  The peak is exact.  Normalised output
is bit-equal to x * g with g the f32 of the stats row; re-measured it reads the target within 1e-5 LU (g and each product are
rounded to f32, 2^-24 relative = 5e-7 LU each).

The kernels run the recurrence in chunks of one sub-block (h = 1600 samples at 16 kHz), 64 chunks to a workgroup of the two filter
kernels and 64 to a step of the carry kernel: 102400 samples.  Input padding beyond lens[b] is NaN (a read of it poisons the
loudness), outputs are pre-filled with a sentinel, wider than needed, with guard words behind them."""
import functools

import numpy as np
import pytest

import loudness_ref as R
from conftest import synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = -77.25
L_BAR = 10.0 * np.log10(1.0 + 1e-10)
MARGIN = 1e-3
H = 1600
LENGTHS = (1, H - 1, H, H + 1, 4 * H - 1, 4 * H, 4 * H + 1, 5 * H, 48000, 64 * H - 1, 64 * H, 64 * H + 1, 65 * H, 68 * H + 3)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


@functools.lru_cache(maxsize=None)
def signal(L, seed=0, sr=16000):
    """noise under a slow envelope that spans 40 dB, with a stretch under the absolute gate: every gate has blocks on both sides"""
    rng = np.random.default_rng(1000 * seed + L % 997)
    t = np.arange(L) / sr
    env = 10.0 ** (-1.0 - 1.0 * np.sin(2 * np.pi * 0.45 * t + seed))
    x = 0.5 * env * rng.standard_normal(L)
    if L >= 3 * sr // 2:
        x[sr // 2:sr] *= 1e-4
    x.flags.writeable = False
    return x.astype(np.float32)


@functools.lru_cache(maxsize=None)
def reference(L, seed=0, sr=16000):
    return R.measure(signal(L, seed, sr), sr)


def measure(rows, sr=16000, extra_L=7, extra_nb=3, fe=None, slots=None):
    """the C entry point on the utterances `rows` as one batch (slots: the batch row of each; rows without one hold a 1-sample
    utterance) -> (stats [B, 8], momentary [B, NB], the words behind each)"""
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
    NB = max(1, int(lens.max()) // (sr // 10) - 3) + extra_nb
    st = torch.full((B * 8 + 5,), SENT, device="cuda", dtype=torch.float64)
    mom = torch.full((B * NB + 5,), SENT, device="cuda", dtype=torch.float64)
    rt._check(fe.lib.mt2_loudness(fe.h, rt._stream(), rt._ptr(dev(wav)), rt._iptr(lens), Lw, B, sr, rt._ptr(st), rt._ptr(mom), NB))
    st, mom = st.cpu().numpy(), mom.cpu().numpy()
    assert (st[B * 8:] == SENT).all() and (mom[B * NB:] == SENT).all()
    return st[:B * 8].reshape(B, 8)[slots], mom[:B * NB].reshape(B, NB)[slots]


def check_against_reference(x, sr, st, mom, m=None, note=""):
    m = R.measure(x, sr) if m is None else m
    margin = R.gate_margin(m)
    assert margin >= MARGIN, f"the test input has a block within {margin:.3g} LU of a gate: choose another input, not another bar"
    nb = m["nb"]
    assert np.isneginf(mom[nb:]).all()
    l = mom[:nb]
    fin = np.isfinite(m["l"])
    assert np.array_equal(np.isneginf(l), np.isneginf(m["l"]))
    err = np.abs(l[fin] - m["l"][fin]).max() if fin.any() else 0.0
    print(f"{note}L {x.size} sr {sr}: {nb} blocks, {m['n_abs']} over -70, {m['n_rel']} over both, gate margin {margin:.3g} LU, I {st[0]:.6f}; "
          f"worst momentary error / bar {err / L_BAR:.3g}, I error {abs(st[0] - m['I']) if np.isfinite(m['I']) else 0.0:.3g}")
    assert err <= L_BAR
    assert (int(st[1]), int(st[2]), int(st[3])) == (nb, m["n_abs"], m["n_rel"])
    for got, want in ((st[0], m["I"]), (st[4], m["gamma"])):
        assert got == want if not np.isfinite(want) else abs(got - want) <= 1e-8
    assert st[5] == m["peak"] == float(np.abs(x).max())
    assert st[6] == m["lmax"] if not np.isfinite(m["lmax"]) else abs(st[6] - m["lmax"]) <= L_BAR
    assert st[7] == 1.0


@pytest.mark.parametrize("L", LENGTHS)
def test_lengths_against_restatement(L):
    """one utterance per launch, at 16 kHz"""
    x = signal(L)
    st, mom = measure([x])
    check_against_reference(x, 16000, st[0], mom[0], reference(L))


@pytest.mark.parametrize("sr, L", [(22050, 30001), (48000, 60000)])
def test_other_rates_against_restatement(sr, L):
    """h = 2205 is odd: no chunk starts on a 16-byte boundary"""
    x = signal(L, 1, sr)
    st, mom = measure([x], sr)
    check_against_reference(x, sr, st[0], mom[0], reference(L, 1, sr))


def test_frontend_method_is_the_entry_point():
    fe = frontend()
    rows = [signal(48000), signal(5 * H)]
    wav = np.zeros((2, 48000), np.float32)
    wav[0], wav[1, :5 * H] = rows[0], rows[1]
    st, mom = fe.loudness(dev(wav), [48000, 5 * H], return_momentary=True)
    want_st, want_mom = measure(rows)
    assert st.dtype == torch.float64 and st.shape == (2, 8) and mom.shape == (2, 27)
    assert np.array_equal(st.cpu().numpy(), want_st) and np.array_equal(mom.cpu().numpy(), want_mom[:, :27])
    assert torch.equal(fe.loudness(dev(wav), [48000, 5 * H]), st)
    from megatts2_amd import megatts2 as M
    d = M.measure_loudness(wav[0])
    assert d["integrated_lufs"][0] == want_st[0, 0] and d["blocks"][0] == 27 and d["sample_peak"][0] == want_st[0, 5] and d["gain"][0] == 1.0


def test_standard_ground_truth_997_hz_at_48k():
    st, _ = measure([R.sine(997.0, 48000, 3.0)], 48000)
    print(f"997 Hz, amplitude 1.0, 48 kHz: {st[0, 0]:.6f} LKFS")
    assert abs(st[0, 0] - (-3.01)) <= 0.01 and st[0, 1] == st[0, 2] == st[0, 3] == 27 and st[0, 5] == 1.0


@pytest.mark.parametrize("sr, printed", [(16000, -2.9701), (22050, -2.9810), (24000, -2.9843), (44100, -3.0075)])
def test_analytic_ground_truth_of_sines(sr, printed):
    """the same figures and the same clips as tests/test_loudness_host.py, the three tones as one ragged batch"""
    rows = [R.sine(f, sr, seconds) for f, seconds in R.SINE_CASES]
    st, _ = measure(rows, sr)
    assert abs(st[0, 0] - printed) <= 1e-3
    for (f, _), row in zip(R.SINE_CASES, st):
        print(f"sr {sr} f {f}: {row[0]:.6f} against {R.sine_reading(f, sr):.6f}")
        assert abs(row[0] - R.sine_reading(f, sr)) <= 1e-3


def test_scaling_by_20_db_lowers_the_reading_by_20_lu():
    x = signal(23000, 2)
    y = (x.astype(np.float64) * 2.0 ** -3).astype(np.float32)          # exact in f32: the readings differ by 20 log10(8) up to rounding
    a, b = reference(23000, 2), R.measure(y, 16000)
    assert R.gate_margin(a) >= MARGIN and R.gate_margin(b) >= MARGIN and (a["n_abs"], a["n_rel"]) == (b["n_abs"], b["n_rel"])
    st, _ = measure([x, y])
    assert (st[0, 2], st[0, 3]) == (st[1, 2], st[1, 3]) == (a["n_abs"], a["n_rel"])
    assert abs((st[0, 0] - st[1, 0]) - 20.0 * np.log10(8.0)) <= 1e-9


def test_both_gates():
    """the relative-gate case and the same with 2 s at -72 LUFS around it, as one ragged batch, against the figures of the host test"""
    x, p = R.gating_case(), R.gating_case(pad=True)
    mx, mp = R.measure(x, 16000), R.measure(p, 16000)
    st, mom = measure([x, p])
    check_against_reference(x, 16000, st[0], mom[0], mx, "relative gate: ")
    check_against_reference(p, 16000, st[1], mom[1], mp, "absolute gate: ")
    assert (st[0, 1], st[0, 2], st[0, 3]) == (97, 97, 63) and (st[1, 1], st[1, 3]) == (137, 63) and st[1, 2] < 137
    assert abs(st[0, 0] - (-23.201)) <= 1e-3 and abs(st[0, 0] - (-23.0)) <= 0.25 and abs(st[0, 0] - mx["ungated"]) > 1.5
    assert abs(st[1, 0] - st[0, 0]) < 1e-9


def test_shortest_utterances():
    x = R.sine(997.0, 16000, 0.5)
    st, mom = measure([x[:4 * H - 1], x[:4 * H], np.zeros(16000, np.float32)])
    assert st[0, 0] == -np.inf and st[0, 1:5].tolist() == [0, 0, 0, -np.inf] and st[0, 6] == -np.inf and np.isneginf(mom[0]).all()
    assert st[1, 1:4].tolist() == [1, 1, 1] and np.isfinite(st[1, 0]) and st[1, 0] == st[1, 6] == mom[1, 0]
    assert st[2, 0] == -np.inf and st[2, 1:4].tolist() == [7, 0, 0] and st[2, 5] == 0.0 and np.isneginf(mom[2]).all()


def test_ragged_batch_is_its_utterances_alone():
    rows = [signal(L, 3) for L in (1, 4 * H - 1, 4 * H, 48000)]
    st, mom = measure(rows)
    again = measure(rows)
    assert np.array_equal(st, again[0]) and np.array_equal(mom, again[1])                        # on repetition
    wider = measure(rows, extra_L=7 + 13)                                                        # with another L_max
    moved = measure(rows, slots=[4, 2, 0, 1])                                                    # in other slots, beside a stranger
    for other in (wider, moved):
        assert np.array_equal(st, other[0]) and np.array_equal(mom, other[1])
    for b, r in enumerate(rows):
        alone_st, alone_mom = measure([r])
        nb = max(1, r.size // H - 3)
        assert np.array_equal(alone_st[0], st[b]) and np.array_equal(alone_mom[0, :nb], mom[b, :nb])
    check_against_reference(rows[3], 16000, st[3], mom[3])


def test_non_finite_sample_poisons_its_own_utterance_only():
    clean = signal(48000, 4)
    bad, worse = clean.copy(), clean.copy()
    bad[9000], worse[20000] = np.nan, np.inf
    st, mom = measure([clean, bad, worse, clean[:20000]])
    alone, alone_mom = measure([clean])
    assert np.array_equal(st[0], alone[0]) and np.array_equal(mom[0], alone_mom[0])              # no bit of a neighbour changes
    check_against_reference(clean[:20000], 16000, st[3], mom[3])
    assert np.isnan(st[1, 0]) and not np.isfinite(st[2, 0])
    assert np.array_equal(mom[1, :2], mom[0, :2]) and np.isnan(mom[1, 2:27]).all()               # from the sub-block that holds it on
    assert st[1, 5] == float(np.nanmax(np.abs(bad))) and st[2, 5] == np.inf and st[1, 1] == 27


# ---- normalisation ------------------------------------------------------------------------------------------------------------

def normalize(rows, target, ceiling=0.0, in_place=False, extra_L=7, fe=None):
    """-> (out [B, Lw], stats [B, 8], wav as it was passed [B, Lw])"""
    fe = fe or frontend()
    B, lens = len(rows), np.asarray([r.size for r in rows], np.int32)
    Lw = int(lens.max()) + extra_L
    wav = np.full((B, Lw), np.nan, np.float32)
    for b, r in enumerate(rows):
        wav[b, :r.size] = r
    buf = torch.full((B * Lw + 11,), SENT, device="cuda", dtype=torch.float32)
    out = buf[:B * Lw].view(B, Lw)
    if in_place:
        out.copy_(dev(wav))
    got, st = fe.loudness_normalize(out if in_place else dev(wav), lens, target, ceiling, out=out, return_stats=True)
    assert got.data_ptr() == out.data_ptr()
    res = buf.cpu().numpy()
    assert (res[B * Lw:] == np.float32(SENT)).all()
    return res[:B * Lw].reshape(B, Lw), st.cpu().numpy(), wav


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def test_normalize_to_target():
    nan_row = signal(5 * H + 200, 6).copy()
    nan_row[3000] = np.nan
    rows = [signal(48000, 5), signal(4 * H - 1, 5), np.zeros(8000, np.float32), signal(68 * H + 3), nan_row, signal(5 * H, 5)]
    refs = [R.measure(r, 16000) for r in (rows[0], rows[3], rows[5])]
    out, st, wav = normalize(rows, -23.0)
    for b, r in enumerate(rows):
        g = np.float32(st[b, 7])
        assert float(g) == st[b, 7]
        assert np.array_equal(bits(out[b, :r.size]), bits(r * g)) and not out[b, r.size:].any()      # one f32 product; zeros in [L, L_max)
    for b in (1, 2, 4):                                                                               # too short, silent, one NaN: unchanged
        assert st[b, 7] == 1.0 and np.array_equal(bits(out[b, :rows[b].size]), bits(rows[b]))
    assert st[1, 0] == -np.inf and st[2, 0] == -np.inf and np.isnan(st[4, 0])
    for b, m in zip((0, 3, 5), refs):
        assert abs(st[b, 0] - m["I"]) <= 1e-8 and st[b, 7] == float(R.gain(st[b, 0], -23.0)) and st[b, 7] != 1.0
    again, _ = measure([out[b, :rows[b].size] for b in (0, 3, 5)])
    print("re-measured:", again[:, 0])
    assert (np.abs(again[:, 0] - (-23.0)) <= 1e-5).all()
    inp, st_inp, _ = normalize(rows, -23.0, in_place=True)                                            # out == wav: the same bits
    assert np.array_equal(bits(inp), bits(out)) and np.array_equal(st_inp, st, equal_nan=True)
    for b in (0, 5):                                                                                  # neighbours of the odd rows are unaffected
        alone, alone_st, _ = normalize([rows[b]], -23.0)
        assert np.array_equal(alone[0, :rows[b].size], out[b, :rows[b].size]) and np.array_equal(alone_st[0], st[b])
    for b, r in enumerate(rows):
        wav[b, r.size:] = 0.0
    plain = frontend().loudness_normalize(dev(wav), [r.size for r in rows], -23.0)                    # the defaults: no out, no stats
    assert np.array_equal(bits(plain.cpu().numpy()), bits(out))


def test_normalize_with_a_ceiling_that_binds():
    rows = [signal(48000, 5), signal(5 * H, 5)]
    free, st_free, _ = normalize(rows, -6.0)
    ceiling = 0.5
    assert all(np.abs(free[b]).max() > 2 * ceiling for b in range(2))                                 # it binds for both
    out, st, _ = normalize(rows, -6.0, ceiling)
    for b, r in enumerate(rows):
        g, peak = np.float32(st[b, 7]), float(np.abs(out[b]).max())
        assert g < np.float32(st_free[b, 7]) and g == R.gain(st[b, 0], -6.0, st[b, 5], ceiling)
        assert np.array_equal(bits(out[b, :r.size]), bits(r * g))
        ulp = float(np.spacing(np.float32(ceiling)))
        print(f"ceiling {ceiling}: peak {peak!r}, {(np.float32(ceiling) - np.float32(peak)) / ulp:.1f} ulp under")
        assert peak <= ceiling and float(np.float32(ceiling)) - peak <= 2 * ulp
    loose, st_loose, _ = normalize(rows, -6.0, 100.0)                                                 # a ceiling that does not bind changes nothing
    assert np.array_equal(loose, free) and np.array_equal(st_loose, st_free)


def test_calls_refuse_before_launch():
    """each case is refused on the host: nothing is launched and every output keeps its sentinel"""
    from megatts2_amd import runtime as rt
    fe = frontend()
    base = torch.full((9000,), SENT, device="cuda", dtype=torch.float32)
    x = base[:6000].view(2, 3000)
    x.copy_(dev(np.stack([signal(3000, 7), signal(3000, 8)])))
    keep = x.clone()
    st = torch.full((16,), SENT, device="cuda", dtype=torch.float64)
    mom = torch.full((8,), SENT, device="cuda", dtype=torch.float64)
    out = torch.full((2, 3000), SENT, device="cuda", dtype=torch.float32)

    def untouched():
        torch.cuda.synchronize()
        assert (st == SENT).all() and (mom == SENT).all() and (out == SENT).all() and torch.equal(x, keep) and (base[6000:] == SENT).all()

    def refuse_measure(lens=(3000, 3000), B=2, sr=16000, NB=4):
        ln = np.asarray(lens, np.int32)
        with pytest.raises(rt.NativeError):
            rt._check(fe.lib.mt2_loudness(fe.h, rt._stream(), rt._ptr(x), rt._iptr(ln), 3000, B, sr, rt._ptr(st), rt._ptr(mom), NB))
        untouched()

    def refuse_normalize(lens=(3000, 3000), sr=16000, target=-23.0, ceiling=0.0, o=out):
        ln = np.asarray(lens, np.int32)
        with pytest.raises(rt.NativeError):
            rt._check(fe.lib.mt2_loudness_normalize(fe.h, rt._stream(), rt._ptr(x), rt._iptr(ln), 3000, 2, sr, target, ceiling, rt._ptr(o),
                                                    rt._ptr(st)))
        untouched()

    for call in (refuse_measure, refuse_normalize):
        call(lens=(3000, 0))
        call(lens=(3001, 3000))
        for sr in (7990, 16005, 192010):
            call(sr=sr)
    refuse_measure(B=0)
    refuse_measure(NB=0)
    refuse_measure(sr=8000, NB=0)                                                                     # 3000 samples at 8 kHz: 0 blocks, and still NB_max >= 1
    for bad in (float("nan"), float("inf")):
        refuse_normalize(target=bad)
        refuse_normalize(ceiling=bad)
    refuse_normalize(o=base[3000:9000].view(2, 3000))                                                 # out's first row is wav's second
    refuse_normalize(o=base[1:6001].view(2, 3000))
    rt._check(fe.lib.mt2_loudness(fe.h, rt._stream(), rt._ptr(x), rt._iptr(np.asarray([3000, 3000], np.int32)), 3000, 2, 16000, rt._ptr(st),
                                  rt._ptr(mom), 4))                                                   # and the valid call goes through
    torch.cuda.synchronize()
    assert (st != SENT).all() and np.isneginf(mom.cpu().numpy()).all()


def test_arena_high_water_is_the_querys_figure():
    from megatts2_amd import runtime as rt
    fe = rt.MelFrontEnd()
    try:
        for L in (3000, 48000, 68 * H + 3):
            x = signal(L, 9)
            measure([x], fe=fe)
            assert fe.workspace_high_water() == rt.loudness_query(16000, L)[3]
            normalize([x], -23.0, fe=fe)
            assert fe.workspace_high_water() == rt.loudness_query(16000, L + 7)[3] == rt.loudness_query(16000, L)[3]
    finally:
        fe.close()


def test_stage_events_name_the_kernels():
    fe = frontend()
    fe.set_profiling(True)
    try:
        normalize([signal(48000)], -23.0)
        assert list(fe.last_stage_ms()) == ["loud_zero_state", "loud_carry", "loud_sums", "loud_gate", "loud_scale"]
        measure([signal(48000)])
        assert list(fe.last_stage_ms()) == ["loud_zero_state", "loud_carry", "loud_sums", "loud_gate"]
    finally:
        fe.set_profiling(False)


# ---- the model: tiny synthetic weights ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny_tts(with_hifigan):
    from megatts2_amd import megatts2 as M
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    return M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)), hifi_gan=M.HIFIGAN(h, sd_h) if with_hifigan else None), g


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifigan"])
def test_synthesize_to_a_target_loudness(vocoder):
    from megatts2_amd import megatts2 as M
    tts, g = tiny_tts(vocoder == "hifigan")
    rng = np.random.default_rng(21)
    B, Np, Tp = 3, 8, 24
    phone = dev(rng.integers(0, g.mrte.phone_vocab_size, (B, Np)).astype(np.int64))
    mels = dev((0.5 * rng.standard_normal((B, Tp, 80)) - 4.0).astype(np.float32))
    dur = np.asarray([[6] * 8, [4, 5, 4, 5, 4, 5, 4, 5], [2] * 8], np.int32)                # 48, 36 and 16 frames: the last is under 0.4 s
    kw = dict(forced_durations=dur, return_aux=True)
    kw.update({"griffin_lim": {"n_iter": 3, "seeds": 5}} if vocoder == "griffin_lim" else {"vocoder": True})
    mel0, lens0, aux0 = tts.synthesize(phone, mels, **kw)
    mel1, lens1, aux1 = tts.synthesize(phone, mels, loudness_lufs=None, **kw)                # None: today's path, today's bits
    assert torch.equal(mel0, mel1) and torch.equal(aux0["wav"], aux1["wav"]) and np.array_equal(lens0, lens1)
    mel, lens, aux = tts.synthesize(phone, mels, loudness_lufs=-23.0, **kw)
    assert torch.equal(mel, mel0) and aux["wav"].shape == aux0["wav"].shape
    n = (np.asarray(lens) - 1) * 256 if vocoder == "griffin_lim" else np.asarray(lens) * 256
    assert (n[:2] >= 4 * H).all() and n[2] < 4 * H, "the phones must be long enough for a block"
    before = M.measure_loudness(aux0["wav"], 16000, lens=n)
    after = M.measure_loudness(aux["wav"], 16000, lens=n)
    print(f"{vocoder}: {before['integrated_lufs']} -> {after['integrated_lufs']}, gated blocks {after['blocks_over_both_gates']}")
    for b in range(B):
        if before["blocks_over_both_gates"][b] >= 1:
            assert abs(after["integrated_lufs"][b] - (-23.0)) <= 1e-4
        else:
            assert torch.equal(aux["wav"][b, :n[b]], aux0["wav"][b, :n[b]])
        assert not aux["wav"][b, n[b]:].any()
    assert before["blocks_over_both_gates"][:2].min() >= 1 and before["blocks"][2] == 0
    with pytest.raises(ValueError):
        tts.synthesize(phone, mels, forced_durations=dur, loudness_lufs=-23.0)               # no audio to normalise


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifigan"])
def test_forward_levels_both_parts_of_the_file(tmp_path, vocoder):
    from megatts2_amd import audio_io
    from megatts2_amd import megatts2 as M
    tts, g = tiny_tts(vocoder == "hifigan")
    wavs = tmp_path / "prompts"
    wavs.mkdir()
    x = 0.05 * signal(16000, 11) / np.abs(signal(16000, 11)).max()
    audio_io.write_wav(str(wavs / "p.wav"), x, 16000)
    phone = np.random.default_rng(22).integers(0, g.mrte.phone_vocab_size, 40)             # 40 phones of at least one frame: over 0.4 s
    out = tmp_path / "out.wav"
    kw = {"vocoder": {"n_iter": 2}} if vocoder == "griffin_lim" else {}
    mel, lens, aux = tts.forward(str(wavs), phone_tokens=phone, out_path=str(out), loudness_lufs=-23.0, **kw)
    y, sr = audio_io.read_wav(str(out))
    Tp = 1 + x.size // 256
    split = (Tp - 1) * 256 if vocoder == "griffin_lim" else Tp * 256
    n_gen = (int(lens[0]) - 1) * 256 if vocoder == "griffin_lim" else int(lens[0]) * 256
    assert sr == 16000 and y.size == split + n_gen and np.isfinite(y).all()
    assert n_gen >= 4 * H, "the generated audio must hold a block"
    parts = [M.measure_loudness(y[:split])["integrated_lufs"][0], M.measure_loudness(y[split:])["integrated_lufs"][0]]
    print(f"{vocoder}: the file's parts read {parts}")
    assert abs(parts[0] - (-23.0)) <= 0.05 and abs(parts[1] - (-23.0)) <= 0.05
    plain = tmp_path / "plain.wav"
    mel0, lens0, aux0 = tts.forward(str(wavs), phone_tokens=phone, out_path=str(plain), **kw)
    assert torch.equal(mel, mel0) and np.array_equal(lens, lens0)
    y0, _ = audio_io.read_wav(str(plain))
    assert y0.size == y.size and not np.array_equal(y0, y)
