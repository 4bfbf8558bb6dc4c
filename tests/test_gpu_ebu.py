"""EBU-mode metering on the GPU (csrc/ebu.hip: mt2_loudness_ebu, mt2_loudness_normalize_tp) against the float64 restatement of the
rules (tests/ebu_ref.py) applied to the same f32 input, against ground truth that needs no outside meter (a tone's true peak is its
amplitude; the range of a two-level tone is the difference of the levels) and on the tiny synthetic model.

Bars.  True peak: |TP - TP_ref| <= 24 2^-24 max_p sum_k |h[p][k]| max |x|, what one f32 fma chain of 24 terms can lose against the
exact sum (ebu_ref.chain_bound, from the table) - the max of two lists differs by no more than their elements do.  Short-term
loudness: |s - s_ref| <= 10 log10(1 + 1e-10) LU, relative 1e-10 in z, as for momentary loudness.  The three counts are EXACT,
asserted only after the restatement shows no block within 1e-3 LU of either gate.  Gamma_r: 1e-8 LU.  P10, P95 and LRA: 2e-10 LU
(each is an element of the set of s).  Fields 0-7 and `momentary` are bit-equal to mt2_loudness's.  Normalised output is bit-equal
to x * g with g the f32 of field 7;  where the ceiling binds, the re-measured true peak is at or under the ceiling times
1 + 4 max_p sum_k |h| 2^-24: the products x g are rounded to f32 (2^-24 relative each) and pass through the filter (sum |h|), the
re-measurement runs its own chain; 4 is room for both and the rounding of g itself, which goes toward zero.

The true-peak kernel takes T = 1024 positions i a workgroup, tile t holding i in [T t - Z, T (t + 1) - Z), Z = 12, with the samples
[T t - 2 Z, T (t + 1)) in LDS.  The range kernel sums 256 blocks abreast.  Input padding beyond lens[b] is NaN (a read of it
poisons peak and loudness), outputs are pre-filled with a sentinel, wider than needed, with guard words behind them.

The issue's binding case for the ceiling, "the fs/4 45 degree tone, target -10 LUFS, ceiling -1 dBTP", cannot bind as a steady tone:
at -10 LUFS a 4 kHz sine has an amplitude of 0.33, whatever it had before.  The steady tone is kept as a case whose ceiling is
free, and the tone keyed in 20 ms raised-cosine bursts every 100 ms (the same carrier, 11 dB less loudness under the same peak) is
the case in which it binds."""
import functools

import numpy as np
import pytest

import ebu_ref as E
import loudness_ref as R
from conftest import synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SENT = -77.25
L_BAR = 10.0 * np.log10(1.0 + 1e-10)
MARGIN = 1e-3
H, Z, T = 1600, E.Z, 1024
NF = 18


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


def test_constants_are_the_librarys():
    from megatts2_amd import runtime as rt
    assert rt.ebu_query(16000, 48000) == (12, 2 * Z, T, 1, rt.ebu_query(16000, 48000)[4]) and rt.EBU_FIELDS == NF


def measure(rows, sr=16000, extra_L=7, extra_n=3, fe=None, slots=None, momentary=True, short_term=True):
    """the C entry point on the utterances `rows` as one batch (slots: the batch row of each; rows without one hold a 1-sample
    utterance) -> (stats [B, 18], momentary [B, NB], short_term [B, NST]), the guard words behind each checked"""
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
    ns = int(lens.max()) // (sr // 10)
    NB, NST = max(1, ns - 3) + extra_n, max(1, ns - 29) + extra_n
    st = torch.full((B * NF + 5,), SENT, device="cuda", dtype=torch.float64)
    mom = torch.full((B * NB + 5,), SENT, device="cuda", dtype=torch.float64)
    sht = torch.full((B * NST + 5,), SENT, device="cuda", dtype=torch.float64)
    rt._check(fe.lib.mt2_loudness_ebu(fe.h, rt._stream(), rt._ptr(dev(wav)), rt._iptr(lens), Lw, B, sr, rt._ptr(st),
                                      rt._ptr(mom if momentary else None), NB if momentary else 0, rt._ptr(sht if short_term else None),
                                      NST if short_term else 0))
    st, mom, sht = st.cpu().numpy(), mom.cpu().numpy(), sht.cpu().numpy()
    assert (st[B * NF:] == SENT).all() and (mom[B * NB:] == SENT).all() and (sht[B * NST:] == SENT).all()
    assert momentary or (mom == SENT).all()
    assert short_term or (sht == SENT).all()
    return st[:B * NF].reshape(B, NF)[slots], mom[:B * NB].reshape(B, NB)[slots], sht[:B * NST].reshape(B, NST)[slots]


def loudness_rows(rows, sr=16000, extra_L=7, extra_n=3):
    """mt2_loudness on the same batch -> (stats [B, 8], momentary [B, NB])"""
    from megatts2_amd import runtime as rt
    fe = frontend()
    B, lens = len(rows), np.asarray([r.size for r in rows], np.int32)
    Lw = int(lens.max()) + extra_L
    wav = np.full((B, Lw), np.nan, np.float32)
    for b, r in enumerate(rows):
        wav[b, :r.size] = r
    NB = max(1, int(lens.max()) // (sr // 10) - 3) + extra_n
    st = torch.full((B, 8), SENT, device="cuda", dtype=torch.float64)
    mom = torch.full((B, NB), SENT, device="cuda", dtype=torch.float64)
    rt._check(fe.lib.mt2_loudness(fe.h, rt._stream(), rt._ptr(dev(wav)), rt._iptr(lens), Lw, B, sr, rt._ptr(st), rt._ptr(mom), NB))
    return st.cpu().numpy(), mom.cpu().numpy()


def bits64(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


# ---- true peak ----------------------------------------------------------------------------------------------------------------------

TP_RATES = (16000, 22050, 48000, 8000, 192000)
TP_LENGTHS = (1, Z, Z + 1, T - Z - 1, T - Z, T - Z + 1, T - 1, T, T + 1, 2 * T + 3)


@functools.lru_cache(maxsize=None)
def noise(L, seed=0):
    x = (0.3 * np.random.default_rng(77 * seed + L).standard_normal(L)).astype(np.float32)
    x.flags.writeable = False
    return x


def check_true_peak(x, sr, row, note=""):
    want, bound = E.true_peak(x, sr), E.chain_bound(sr, np.abs(x).max())
    sp = float(np.abs(x).max())
    err = abs(row[8] - want)
    print(f"{note}sr {sr} L {x.size}: true peak {row[8]:.7f} against {want:.7f}, error / bar {err / bound:.3g}; sample peak {sp:.7f}")
    assert err <= bound
    assert row[5] == sp and row[8] >= row[5] and row[9] == E.oversample(sr)                  # phase 0 is the sample itself
    assert float(np.float32(row[8])) == row[8]
    return err / bound


@pytest.mark.parametrize("sr", TP_RATES)
def test_true_peak_lengths_against_restatement(sr):
    """the lengths around the halo and the tile as one ragged batch"""
    rows = [noise(L) for L in TP_LENGTHS]
    st, _, _ = measure(rows, sr, momentary=False, short_term=False)
    worst = max(check_true_peak(x, sr, st[b]) for b, x in enumerate(rows))
    print(f"sr {sr}: worst error / bar {worst:.3g}")
    if sr == 192000:
        assert (st[:, 8] == st[:, 5]).all()                                                   # one phase: the samples themselves


def crest_rows():
    """(row, the position i that must hold the crest): quiet noise, and two equal samples whose crest lies between them at i
    - astride the boundary of tiles 0 and 1, the far tap of the crest's window (x[i + Z], weight 1.7e-4) loud: the last word of the halo
    - the first position of tile 1, the far tap on the other side (x[i - Z + 1]) loud: the first word of the halo
    - on the first and on the last sample"""
    L = 2 * T + 3
    out = []
    for c, far in ((T - Z - 1, T - 1), (T - Z, T - 2 * Z + 1), (0, None), (L - 2, None)):
        x = 0.02 * noise(L, 3 + c).copy()
        x[c] = x[c + 1] = 0.7
        if far is not None:
            x[far] = -0.6 if far > c else 0.6
        out.append((x.astype(np.float32), c))
    return out


@pytest.mark.parametrize("sr", TP_RATES)
def test_true_peak_crest_at_the_edges(sr):
    cases = crest_rows()
    o = E.oversample(sr)
    for x, c in cases:
        if o > 1:                                                                             # the test's own aim: the crest is where it was put
            y = np.abs(E.interpolate(x, sr))
            r, p = np.unravel_index(np.argmax(y), y.shape)
            assert r - Z == c and p > 0 and y[r, p] > 0.8, (r - Z, c, p)
    st, _, _ = measure([x for x, _ in cases], sr, momentary=False, short_term=False)
    for (x, c), row in zip(cases, st):
        check_true_peak(x, sr, row, f"crest at {c}: ")
        assert o == 1 or row[8] > 1.2 * row[5]
    alone = [measure([x], sr, momentary=False, short_term=False)[0][0] for x, _ in cases[:2]]
    assert np.array_equal(bits64(np.stack(alone)), bits64(st[:2]))


def test_true_peak_in_front_of_and_behind_the_signal():
    """a full-scale first / last sample of opposite sign to its neighbour: the largest interpolated value lies outside [0, L - 1]"""
    x = np.zeros(40, np.float32)
    x[0], x[1], x[-1], x[-2] = 0.5, -0.5, 0.5, -0.5
    y = np.abs(E.interpolate(x, 16000))
    r = np.unravel_index(np.argmax(y), y.shape)[0] - Z
    assert r in (-1, 39) and y.max() > 0.5                                                    # in front of sample 0 or behind sample L - 1
    st, _, _ = measure([x, x[:20], x[20:]], momentary=False, short_term=False)
    for row, part in zip(st, (x, x[:20], x[20:])):
        check_true_peak(part, 16000, row)
        assert row[8] > row[5]


@pytest.mark.parametrize("sr", E.RATES)
def test_true_peak_of_tones_reads_the_host_figures(sr):
    tones = [(0.5, t) for t in E.TONES] + [(1.41, (4, 45.0))]
    rows = [E.tone(sr, div, ph, amp) for amp, (div, ph) in tones]
    st, _, _ = measure(rows, sr, momentary=False, short_term=False)
    for (amp, (div, ph)), x, row in zip(tones, rows, st):
        err = E.db(row[8] / amp)
        print(f"sr {sr} fs/{div} at {ph} deg, amplitude {amp}: {err:+.4f} dB of it (restatement {E.db(E.true_peak(x, sr) / amp):+.4f})")
        assert -0.4 <= err <= 0.2                                                             # EBU Tech 3341
        assert abs(row[8] - E.true_peak(x, sr)) <= E.chain_bound(sr, amp)
        if (div, ph) == (4, 45.0):
            assert abs(E.db(row[5] / amp) - (-3.01)) <= 0.01


# ---- short-term loudness and loudness range ----------------------------------------------------------------------------------------------

NS_CASES = (29, 30, 31, 59, 285, 286, 287, 600)


@functools.lru_cache(maxsize=None)
def stepped_noise():
    """600 sub-blocks of noise: a level step of 12 dB, a stretch under the absolute gate, a swell, a tail under the relative gate - and
    its sub-block sums, of which every prefix's are a prefix (the filter is causal)"""
    ns = 600
    j = np.arange(ns)
    env = np.where(j < 20, 1.0, 0.25)
    env = np.where((j >= 100) & (j < 140), 1e-4, env)
    env = np.where(j >= 140, 10.0 ** (0.3 * np.sin(2 * np.pi * (j - 140) / 97.0)), env)
    env = np.where(j >= 400, 0.012, env)
    x = (0.2 * np.repeat(env, H) * np.random.default_rng(31).standard_normal(ns * H)).astype(np.float32)
    x.flags.writeable = False
    return x, R.sub_block_sums(x, 16000)


@functools.lru_cache(maxsize=None)
def stepped_reference(ns):
    return E.short_term_of_sums(stepped_noise()[1][:ns], H)


def check_range(m, row, sht, note=""):
    margin = E.gate_margin(m)
    assert margin >= MARGIN, f"the test input has a block within {margin:.3g} LU of a gate: choose another input, not another bar"
    nst = m["nst"]
    assert np.isneginf(sht[nst:]).all()
    s, fin = sht[:nst], np.isfinite(m["s"])
    assert np.array_equal(np.isneginf(s), np.isneginf(m["s"]))
    err = np.abs(s[fin] - m["s"][fin]).max() if fin.any() else 0.0
    print(f"{note}{nst} short-term blocks, {m['n_abs']} over -70, {m['n_rel']} over both, gate {m['gamma']:.4f}, margin {margin:.3g} LU, LRA "
          f"{row[10]:.6f} (P10 {row[15]:.6f}, P95 {row[16]:.6f}); worst short-term error / bar {err / L_BAR:.3g}")
    assert err <= L_BAR
    assert (int(row[11]), int(row[12]), int(row[13])) == (nst, m["n_abs"], m["n_rel"])
    assert row[14] == m["gamma"] if not np.isfinite(m["gamma"]) else abs(row[14] - m["gamma"]) <= 1e-8
    for got, want in ((row[15], m["p10"]), (row[16], m["p95"]), (row[10], m["lra"])):
        assert np.isnan(got) if np.isnan(want) else abs(got - want) <= 2e-10
    assert row[17] == m["smax"] if not np.isfinite(m["smax"]) else abs(row[17] - m["smax"]) <= L_BAR
    if m["n_rel"]:
        assert row[15] in s and row[16] in s and row[10] == row[16] - row[15]                 # elements of the set, selected exactly


@pytest.mark.parametrize("ns", NS_CASES)
def test_short_term_and_range_against_restatement(ns):
    """nst = ns - 29 = 0, 1, 2, 30, 256, 257, 258, 571: around the 256 partial sums of the fixed-order mean; 3 samples more than
    the sub-blocks hold"""
    x = stepped_noise()[0][:ns * H + 3] if ns < 600 else stepped_noise()[0]
    st, _, sht = measure([x])
    check_range(stepped_reference(ns), st[0], sht[0], f"ns {ns}: ")
    assert st[0, 1] == max(0, ns - 3)


def test_tech_3342_cases_and_both_gates():
    """the synthetic cases of EBU Tech 3342 (its own tolerance: 1 LU) and the two gating cases as one ragged batch, against the figures
    of the host test"""
    specs = [s for s, _ in E.TECH_3342] + [E.REL_GATE_CASE, E.ABS_GATE_CASE]
    st, _, sht = measure([E.levels(s) for s in specs], momentary=False)
    for b, s in enumerate(specs):
        check_range(E.case(s), st[b], sht[b], f"{s}: ")
    for b, (_, want) in enumerate(E.TECH_3342):
        assert abs(st[b, 10] - want) <= 1.0 and abs(st[b, 10] - want) <= 1e-3
    assert st[4, 11:14].tolist() == [171, 171, 171] and abs(st[4, 10] - 22.0) <= 1e-3         # with the gate at -18 it would read 4.31
    assert st[5, 11:14].tolist() == [221, 200, 180] and abs(st[5, 10] - 22.0) <= 1e-3


def test_shortest_utterances():
    x = R.sine(1000.0, 16000, 3.0, level=-23.0)
    st, _, sht = measure([x, x[:30 * H - 1], np.zeros(4 * 16000, np.float32)])
    assert st[0, 11:14].tolist() == [1, 1, 1] and st[0, 10] == 0.0 and st[0, 15] == st[0, 16] == st[0, 17] == sht[0, 0] and abs(sht[0, 0] + 23.0) <= 0.01
    assert st[1, 11:14].tolist() == [0, 0, 0] and np.isnan(st[1, [10, 15, 16]]).all() and st[1, 14] == -np.inf and st[1, 17] == -np.inf
    assert st[2, 11:14].tolist() == [11, 0, 0] and np.isnan(st[2, [10, 15, 16]]).all() and st[2, 8] == 0.0 and np.isneginf(sht[2]).all()
    assert np.isneginf(sht[1]).all() and np.isneginf(sht[0, 1:]).all()


def test_first_eight_fields_and_momentary_are_mt2_loudness_bit_for_bit():
    rows = [stepped_noise()[0][:L] for L in (1, 4 * H - 1, 4 * H, 48000, 68 * H + 3)] + [R.gating_case(pad=True)]
    st, mom, _ = measure(rows)
    want_st, want_mom = loudness_rows(rows)
    assert np.array_equal(bits64(st[:, :8]), bits64(want_st)) and np.array_equal(bits64(mom), bits64(want_mom))
    quiet, _, _ = measure(rows, momentary=False, short_term=False)                            # the optional outputs change nothing
    assert np.array_equal(bits64(quiet), bits64(st))


def test_frontend_method_is_the_entry_point():
    fe = frontend()
    rows = [stepped_noise()[0][:49600], noise(5 * H)]
    wav = np.zeros((2, 49600), np.float32)
    wav[0], wav[1, :5 * H] = rows[0], rows[1]
    want_st, want_mom, want_sht = measure(rows)
    st, mom, sht = fe.loudness_ebu(dev(wav), [49600, 5 * H], return_momentary=True, return_short_term=True)
    assert st.dtype == torch.float64 and st.shape == (2, NF) and mom.shape == (2, 28) and sht.shape == (2, 2)
    assert np.array_equal(bits64(st.cpu().numpy()), bits64(want_st)) and np.array_equal(mom.cpu().numpy(), want_mom[:, :28])
    assert np.array_equal(sht.cpu().numpy(), want_sht[:, :2])
    assert torch.equal(fe.loudness_ebu(dev(wav), [49600, 5 * H]).view(torch.int64), st.view(torch.int64))
    only = fe.loudness_ebu(dev(wav), [49600, 5 * H], return_short_term=True)
    assert len(only) == 2 and torch.equal(only[1], sht)
    from megatts2_amd import megatts2 as M
    plain, d = M.measure_loudness(wav[0]), M.measure_loudness(wav[0], ebu=True)
    for k, v in plain.items():
        assert np.array_equal(bits64(v), bits64(d[k]))                                        # ebu=False is today's dict, ebu=True keeps its bits
    assert set(d) - set(plain) == set(M.EBU_STATS) | {"true_peak_dbtp"}
    assert d["true_peak"][0] == want_st[0, 8] and d["lra"][0] == want_st[0, 10] and d["short_term_blocks"][0] == 2 and d["oversampling"][0] == 12
    assert d["short_term_max"][0] == want_st[0, 17] and d["true_peak_dbtp"][0] == 20.0 * np.log10(want_st[0, 8])


def test_ragged_batch_is_its_utterances_alone():
    rows = [stepped_noise()[0][:L] for L in (1, 4799, 48000, 96000)]
    first = measure(rows)
    for other in (measure(rows), measure(rows, extra_L=7 + 13), measure(rows, slots=[4, 2, 0, 1])):      # again; another L_max; other slots, a stranger
        for a, b in zip(first, other):
            assert np.array_equal(bits64(a), bits64(b))
    for b, r in enumerate(rows):
        st, mom, sht = measure([r])
        nb, nst = max(1, r.size // H - 3), max(1, r.size // H - 29)
        assert np.array_equal(bits64(st[0]), bits64(first[0][b])) and np.array_equal(bits64(mom[0, :nb]), bits64(first[1][b, :nb]))
        assert np.array_equal(bits64(sht[0, :nst]), bits64(first[2][b, :nst]))
    check_range(E.short_term_of_sums(stepped_noise()[1][:60], H), first[0][3], first[2][3], "96000 samples: ")
    check_true_peak(rows[3], 16000, first[0][3])


def test_non_finite_sample_poisons_its_own_utterance_only():
    clean = stepped_noise()[0][:96000]
    bad, worse = clean.copy(), clean.copy()
    bad[9000], worse[20000] = np.nan, np.inf
    st, mom, sht = measure([clean, bad, worse, clean[:60000]])
    alone = measure([clean])
    for a, b in zip((st, mom, sht), alone):
        assert np.array_equal(bits64(a[0]), bits64(b[0]))                                     # no bit of a neighbour changes
    short = measure([clean[:60000]])
    assert np.array_equal(bits64(st[3]), bits64(short[0][0]))
    m = E.short_term(bad, 16000)
    assert np.isnan(m["lra"]) and m["n_rel"] == m["nst"] == 31
    assert np.isnan(st[1, 10]) and np.isnan(st[1, 14]) and np.isnan(st[1, 16]) and st[1, 11:14].tolist() == [31, 31, 31] and np.isnan(sht[1, :31]).all()
    assert np.isnan(st[2, 10]) and st[2, 8] == np.inf and st[2, 5] == np.inf
    assert st[1, 8] == E.true_peak(bad, 16000) or abs(st[1, 8] - E.true_peak(bad, 16000)) <= E.chain_bound(16000, np.nanmax(np.abs(bad)))
    assert np.isfinite(st[1, 8]) and st[1, 8] >= st[1, 5] == float(np.nanmax(np.abs(bad)))


def test_calls_refuse_before_launch():
    """each case is refused on the host: nothing is launched and every output keeps its sentinel"""
    from megatts2_amd import runtime as rt
    fe = frontend()
    base = torch.full((9000,), SENT, device="cuda", dtype=torch.float32)
    x = base[:6000].view(2, 3000)
    x.copy_(dev(np.stack([noise(3000, 7), noise(3000, 8)])))
    keep = x.clone()
    st = torch.full((2 * NF,), SENT, device="cuda", dtype=torch.float64)
    mom = torch.full((8,), SENT, device="cuda", dtype=torch.float64)
    sht = torch.full((8,), SENT, device="cuda", dtype=torch.float64)
    out = torch.full((2, 3000), SENT, device="cuda", dtype=torch.float32)

    def untouched():
        torch.cuda.synchronize()
        assert (st == SENT).all() and (mom == SENT).all() and (sht == SENT).all() and (out == SENT).all() and torch.equal(x, keep)
        assert (base[6000:] == SENT).all()

    def refuse_measure(lens=(3000, 3000), B=2, sr=16000, NB=4, NST=4, s=st):
        ln = np.asarray(lens, np.int32)
        with pytest.raises(rt.NativeError):
            rt._check(fe.lib.mt2_loudness_ebu(fe.h, rt._stream(), rt._ptr(x), rt._iptr(ln), 3000, B, sr, rt._ptr(s), rt._ptr(mom), NB,
                                              rt._ptr(sht), NST))
        untouched()

    def refuse_normalize(lens=(3000, 3000), sr=16000, target=-23.0, ceiling=-1.0, o=out):
        ln = np.asarray(lens, np.int32)
        with pytest.raises(rt.NativeError):
            rt._check(fe.lib.mt2_loudness_normalize_tp(fe.h, rt._stream(), rt._ptr(x), rt._iptr(ln), 3000, 2, sr, target, ceiling, rt._ptr(o),
                                                       rt._ptr(st)))
        untouched()

    for call in (refuse_measure, refuse_normalize):
        call(lens=(3000, 0))
        call(lens=(3001, 3000))
        for sr in (7990, 16005, 192010):
            call(sr=sr)
    refuse_measure(B=0)
    refuse_measure(NB=0)
    refuse_measure(NST=0)
    refuse_measure(s=None)
    for bad in (float("nan"), float("inf")):
        refuse_normalize(target=bad)
        refuse_normalize(ceiling=bad)
    refuse_normalize(o=base[3000:9000].view(2, 3000))                                         # out's first row is wav's second
    refuse_normalize(o=base[1:6001].view(2, 3000))
    with pytest.raises(ValueError):
        fe.loudness_normalize(x, None, -23.0, 0.9, true_peak_ceiling_dbtp=-1.0)               # the ceiling stated twice
    untouched()
    rt._check(fe.lib.mt2_loudness_ebu(fe.h, rt._stream(), rt._ptr(x), rt._iptr(np.asarray([3000, 3000], np.int32)), 3000, 2, 16000, rt._ptr(st),
                                      rt._ptr(mom), 4, rt._ptr(sht), 4))                     # and the valid call goes through
    torch.cuda.synchronize()
    assert (st != SENT).all() and np.isneginf(mom.cpu().numpy()).all() and np.isneginf(sht.cpu().numpy()).all()


def test_arena_high_water_is_the_querys_figure():
    from megatts2_amd import runtime as rt
    fe = rt.MelFrontEnd()
    try:
        for L in (3000, 48000, 68 * H + 3):
            x = stepped_noise()[0][:L]
            measure([x], fe=fe)
            assert fe.workspace_high_water() == rt.ebu_query(16000, L)[4]
            normalize([x], -23.0, -1.0, fe=fe)
            assert fe.workspace_high_water() == rt.ebu_query(16000, L + 7)[4] == rt.ebu_query(16000, L)[4]
        assert rt.ebu_query(16000, 68 * H + 3)[4] > rt.loudness_query(16000, 68 * H + 3)[3]
    finally:
        fe.close()


def test_stage_events_name_the_kernels():
    fe = frontend()
    fe.set_profiling(True)
    try:
        normalize([noise(48000)], -23.0, -1.0)
        assert list(fe.last_stage_ms()) == ["loud_zero_state", "loud_carry", "loud_sums", "loud_gate", "ebu_true_peak", "ebu_range", "loud_scale"]
        measure([noise(48000)])
        assert list(fe.last_stage_ms()) == ["loud_zero_state", "loud_carry", "loud_sums", "loud_gate", "ebu_true_peak", "ebu_range"]
    finally:
        fe.set_profiling(False)


# ---- normalisation under a true-peak ceiling --------------------------------------------------------------------------------------------

def normalize(rows, target, ceiling_dbtp=None, in_place=False, extra_L=7, fe=None, peak_ceiling=0.0, sr=16000):
    """-> (out [B, Lw], stats [B, 18] (or [B, 8] without a true-peak ceiling), wav as it was passed [B, Lw])"""
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
    got, st = fe.loudness_normalize(out if in_place else dev(wav), lens, target, peak_ceiling, sample_rate=sr, out=out, return_stats=True,
                                    true_peak_ceiling_dbtp=ceiling_dbtp)
    assert got.data_ptr() == out.data_ptr()
    res = buf.cpu().numpy()
    assert (res[B * Lw:] == np.float32(SENT)).all()
    return res[:B * Lw].reshape(B, Lw), st.cpu().numpy(), wav


def tp_margin(sr):
    """the factor over the ceiling that the rounding of the products through the filter allows"""
    return 1.0 + 4.0 * float(np.abs(E.table(sr).astype(np.float64)).sum(axis=1).max()) * 2.0 ** -24


def keyed_tone(sr=16000, seconds=2.0, amp=0.5):
    """the fs/4 tone at 45 degrees in 20 ms raised-cosine bursts every 100 ms: the crest lies between the samples, and the loudness
    is 11 dB under the steady tone's"""
    n = int(seconds * sr)
    x = amp * np.sin(2.0 * np.pi * np.arange(n) / 4 + np.pi / 4)
    w = np.zeros(sr // 10)
    w[:sr // 50] = 0.5 - 0.5 * np.cos(2.0 * np.pi * (np.arange(sr // 50) + 0.5) / (sr // 50))
    return (x * np.tile(w, n // w.size)).astype(np.float32)


def test_normalize_under_a_ceiling_that_does_not_bind():
    nan_row = noise(5 * H + 200, 6).copy()
    nan_row[3000] = np.nan
    steady = E.tone(16000, 4, 45.0, 0.5, 16000)                                               # the issue's tone: at -10 LUFS its amplitude is 0.33
    rows = [stepped_noise()[0][:48000], noise(4 * H - 1, 5), np.zeros(8000, np.float32), steady, nan_row, noise(5 * H, 5)]
    out, st, wav = normalize(rows, -23.0, -1.0)
    want, _, _ = measure(rows)
    assert np.array_equal(bits64(st[:, :7]), bits64(want[:, :7])) and np.array_equal(bits64(st[:, 8:]), bits64(want[:, 8:]))      # of the INPUT
    for b, r in enumerate(rows):
        g = np.float32(st[b, 7])
        assert float(g) == st[b, 7]
        assert np.array_equal(bits(out[b, :r.size]), bits(r * g)) and not out[b, r.size:].any()      # one f32 product; zeros in [L, L_max)
    for b in (1, 2, 4):                                                                               # too short, silent, one NaN: unchanged
        assert st[b, 7] == 1.0 and np.array_equal(bits(out[b, :rows[b].size]), bits(rows[b]))
    for b in (0, 3, 5):
        ref = E.gain_tp(st[b, 0], -23.0, st[b, 8], -1.0)
        assert st[b, 7] != 1.0 and abs(st[b, 7] - float(ref)) <= float(np.spacing(ref))               # pow on the device, ** on the host: one ulp
        assert st[b, 7] * st[b, 8] < 10.0 ** (-1.0 / 20.0)                                            # free
    again, _, _ = measure([out[b, :rows[b].size] for b in (0, 3, 5)])
    print("re-measured:", again[:, 0], "true peaks", again[:, 8])
    assert (np.abs(again[:, 0] - (-23.0)) <= 1e-5).all()
    loud, st_loud, _ = normalize([steady], -10.0, -1.0)                                               # the issue's case as it states it
    back, _, _ = measure([loud[0, :steady.size]])
    print(f"steady fs/4 tone to -10 LUFS under -1 dBTP: gain {st_loud[0, 7]:.6f}, {back[0, 0]:.6f} LUFS, true peak {E.db(back[0, 8]):.3f} dBTP")
    assert abs(back[0, 0] - (-10.0)) <= 1e-5 and back[0, 8] <= 10.0 ** (-1.0 / 20.0) * tp_margin(16000) and back[0, 8] < 0.4
    inp, st_inp, _ = normalize(rows, -23.0, -1.0, in_place=True)                                      # out == wav: the same bits
    assert np.array_equal(bits(inp), bits(out)) and np.array_equal(st_inp, st, equal_nan=True)
    for b, r in enumerate(rows):
        wav[b, r.size:] = 0.0
    lens = [r.size for r in rows]
    today = frontend().loudness_normalize(dev(wav), lens, -23.0)
    none = frontend().loudness_normalize(dev(wav), lens, -23.0, true_peak_ceiling_dbtp=None)           # None: today's call, today's bits
    assert np.array_equal(bits(today.cpu().numpy()), bits(none.cpu().numpy()))
    free = frontend().loudness_normalize(dev(wav), lens, -23.0, true_peak_ceiling_dbtp=-1.0)
    assert np.array_equal(bits(free.cpu().numpy()), bits(out))
    o8, st8 = frontend().loudness_normalize(dev(wav), lens, -23.0, return_stats=True, true_peak_ceiling_dbtp=None)
    assert st8.shape == (6, 8) and np.array_equal(bits(o8.cpu().numpy()), bits(today.cpu().numpy()))


@pytest.mark.parametrize("sr", [16000, 48000])
def test_normalize_under_a_ceiling_that_binds(sr):
    """the keyed fs/4 tone at 45 degrees to -10 LUFS under -1 dBTP"""
    x = keyed_tone(sr)
    ceiling = 10.0 ** (-1.0 / 20.0)
    free, st_free, _ = normalize([x], -10.0, sr=sr)
    assert E.true_peak(free[0, :x.size], sr) > 1.05 * ceiling                                         # it binds
    out, st, _ = normalize([x], -10.0, -1.0, sr=sr)
    g = np.float32(st[0, 7])
    assert float(g) == st[0, 7] and g < np.float32(st_free[0, 7]) and np.array_equal(bits(out[0, :x.size]), bits(x * g))
    cap = ceiling / st[0, 8]
    assert float(g) <= cap < float(np.nextafter(g, np.float32(4))) or abs(float(g) - cap) <= 2 * float(np.spacing(g))
    assert float(g) <= cap * (1 + 2.0 ** -50)                                                         # toward zero: never over the cap
    inp, st_inp, _ = normalize([x], -10.0, -1.0, in_place=True, sr=sr)
    assert np.array_equal(bits(inp), bits(out)) and np.array_equal(st_inp, st, equal_nan=True)
    back, _, _ = measure([out[0, :x.size]], sr)
    tp, sp = back[0, 8], back[0, 5]
    print(f"sr {sr}: gain {float(g):.6f} (free {st_free[0, 7]:.6f}); true peak {E.db(tp):.4f} dBTP, {tp / ceiling - 1:+.3g} of the ceiling (room "
          f"{tp_margin(sr) - 1:.3g}); sample peak {E.db(sp):.3f} dBFS; {back[0, 0]:.3f} LUFS reached")
    assert tp <= ceiling * tp_margin(sr) and tp >= ceiling * (1 - 1e-5)
    assert abs(E.db(tp / sp) - 3.01) <= 0.05                                                          # the crest the samples do not show
    assert back[0, 0] < -10.5                                                                         # one gain, no limiter: the loudness gives way
    old, _, _ = normalize([x], -10.0, peak_ceiling=ceiling, sr=sr)                                    # the sample-peak form at the same ceiling
    over = measure([old[0, :x.size]], sr)[0][0]
    print(f"sr {sr}: with peak_ceiling={ceiling:.4f} the sample peak is {over[5]:.4f} and the true peak {E.db(over[8]):+.3f} dBTP")
    assert over[5] <= ceiling and over[8] > 1.15 * ceiling                                            # the accident this removes


# ---- the model: tiny synthetic weights ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny_tts(with_hifigan):
    from megatts2_amd import megatts2 as M
    (g, p, a, h), (sd_g, sd_p, sd_a, sd_h) = synth_models("tiny")
    return M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)), hifi_gan=M.HIFIGAN(h, sd_h) if with_hifigan else None), g


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifigan"])
def test_synthesize_under_a_true_peak_ceiling(vocoder):
    from megatts2_amd import megatts2 as M
    tts, g = tiny_tts(vocoder == "hifigan")
    rng = np.random.default_rng(21)
    B, Np, Tp = 3, 8, 24
    phone = dev(rng.integers(0, g.mrte.phone_vocab_size, (B, Np)).astype(np.int64))
    mels = dev((0.5 * rng.standard_normal((B, Tp, 80)) - 4.0).astype(np.float32))
    dur = np.asarray([[6] * 8, [4, 5, 4, 5, 4, 5, 4, 5], [2] * 8], np.int32)                # 48, 36 and 16 frames: the last is under 0.4 s
    kw = dict(forced_durations=dur, return_aux=True)
    kw.update({"griffin_lim": {"n_iter": 3, "seeds": 5}} if vocoder == "griffin_lim" else {"vocoder": True})
    mel0, lens0, aux0 = tts.synthesize(phone, mels, loudness_lufs=-23.0, **kw)
    mel1, lens1, aux1 = tts.synthesize(phone, mels, loudness_lufs=-23.0, true_peak_ceiling_dbtp=None, **kw)      # None: today's path, today's bits
    assert torch.equal(mel0, mel1) and torch.equal(aux0["wav"], aux1["wav"]) and np.array_equal(lens0, lens1)
    n = (np.asarray(lens0) - 1) * 256 if vocoder == "griffin_lim" else np.asarray(lens0) * 256
    ceiling, room = 10.0 ** (-1.0 / 20.0), tp_margin(16000)
    for target in (-23.0, 0.0):                                                               # at 0 LUFS the ceiling binds
        mel, lens, aux = tts.synthesize(phone, mels, loudness_lufs=target, true_peak_ceiling_dbtp=-1.0, **kw)
        assert torch.equal(mel, mel0) and np.array_equal(lens, lens0)
        after = M.measure_loudness(aux["wav"], 16000, lens=n, ebu=True)
        print(f"{vocoder} to {target}: {after['integrated_lufs']} LUFS, true peaks {after['true_peak_dbtp']} dBTP")
        bound = 0
        for b in range(2):
            assert after["true_peak"][b] <= ceiling * room
            if after["true_peak"][b] < ceiling * (1 - 1e-4):
                assert abs(after["integrated_lufs"][b] - target) <= 1e-4                      # the ceiling does not bind: the target is met
            else:
                assert after["integrated_lufs"][b] < target
                bound += 1
        assert bound == (2 if target == 0.0 else 0)
        assert not np.isfinite(after["integrated_lufs"][2])                                   # under 0.4 s: left as it was
    with pytest.raises(ValueError):
        tts.synthesize(phone, mels, true_peak_ceiling_dbtp=-1.0, **kw)                        # a ceiling on a gain that is not formed
    with pytest.raises(ValueError):
        tts.synthesize(phone, mels, loudness_lufs=-23.0, peak_ceiling=0.9, true_peak_ceiling_dbtp=-1.0, **kw)


@pytest.mark.parametrize("vocoder", ["griffin_lim", "hifigan"])
def test_forward_keeps_both_parts_of_the_file_under_the_ceiling(tmp_path, vocoder):
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
    for target in (-23.0, 0.0):
        out = tmp_path / f"out{int(target)}.wav"
        mel, lens, aux = tts.forward(str(wavs), phone_tokens=phone, out_path=str(out), loudness_lufs=target, true_peak_ceiling_dbtp=-1.0, **kw)
        y, sr = audio_io.read_wav(str(out))
        assert sr == 16000 and np.isfinite(y).all() and y.size > split + 4 * H
        parts = [M.measure_loudness(part, ebu=True) for part in (y[:split], y[split:])]
        print(f"{vocoder} to {target}: parts read {[float(p['integrated_lufs'][0]) for p in parts]} LUFS, {[float(p['true_peak_dbtp'][0]) for p in parts]} dBTP")
        for p in parts:
            # the file holds 16-bit samples: each moves by at most half a step of 2^-15, through the filter sum |h| times that
            assert p["true_peak"][0] <= ceiling * tp_margin(16000) + 2.0 ** -16 * 2.21
            if target == -23.0:
                assert abs(p["integrated_lufs"][0] - target) <= 0.05
            else:
                assert p["integrated_lufs"][0] < target and p["true_peak"][0] >= ceiling - 2.0 ** -16 * 2.21 - 1e-4
    with pytest.raises(ValueError):
        tts.forward(str(wavs), phone_tokens=phone, out_path=None, true_peak_ceiling_dbtp=-1.0, **kw)
