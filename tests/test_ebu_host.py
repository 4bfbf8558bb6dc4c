"""Host side of the EBU-mode stage (no GPU): the float64 restatement of the rules (tests/ebu_ref.py) against ground truth that needs
no outside meter - the true peak of a band-limited tone is its amplitude whatever the sampling phase (bar: EBU Tech 3341's +0.2 /
-0.4 dB); the loudness range of a two-level tone is the difference of the levels (EBU Tech 3342 cases 1-4, its own tolerance of
1 LU) - both gates of the range on inputs whose blocks keep a stated distance from them, the percentile rule against Tech 3342's
rounding formula, and the library's host-only entry points mt2_ebu_query and mt2_true_peak_table, the refusals and the exports."""
import ctypes as C
import math
import os

import numpy as np
import pytest

import ebu_ref as E
import loudness_ref as R

MARGIN = 1e-3


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


@pytest.mark.parametrize("sr, o", [(8000, 24), (16000, 12), (22050, 9), (44100, 5), (48000, 4), (192000, 1)])
def test_table_is_the_restatements_after_one_rounding(rt, sr, o):
    assert E.oversample(sr) == o and rt.ebu_query(sr, 1)[:3] == (o, E.TAPS, rt.TP_TILE)
    got = rt.true_peak_table(sr)
    assert got.shape == (o, 24) and got.dtype == np.float32
    assert np.array_equal(got, E.table(sr))
    assert got[0, E.Z - 1] == 1.0 and not np.delete(got[0], E.Z - 1).any()              # phase 0: the unit sample
    dc = E.table64(sr).sum(axis=1)
    print(f"sr {sr}: o {o}, DC gain of the phases in [{dc.min():.6f}, {dc.max():.6f}], sum |h| at most {np.abs(E.table64(sr)).sum(axis=1).max():.4f}")
    assert np.abs(dc - 1.0).max() <= 2e-3


@pytest.mark.parametrize("sr", E.RATES)
def test_true_peak_of_a_tone_is_its_amplitude(sr):
    """the crest of every tone falls between the samples: fs/4 at 45 degrees has samples at +-A / sqrt 2 alone"""
    worst = [0.0, 0.0]
    for amp, (div, ph) in [(0.5, t) for t in E.TONES] + [(1.41, (4, 45.0))]:
        x = E.tone(sr, div, ph, amp)
        tp, sp = E.true_peak(x, sr), E.sample_peak(x)
        err = E.db(tp / amp)
        worst = [max(worst[0], err), min(worst[1], err)]
        print(f"sr {sr} fs/{div} at {ph} deg, amplitude {amp}: true peak {err:+.4f} dB of it, sample peak {E.db(sp / amp):+.4f} dB")
        assert -0.4 <= err <= 0.2 and tp >= sp
        if (div, ph) == (4, 45.0):
            assert abs(E.db(sp / amp) - (-3.01)) <= 0.01                                    # the sample peak cannot see the crest
    print(f"sr {sr}: worst {worst[0]:+.4f} / {worst[1]:+.4f} dB")
    assert worst[0] <= 0.003 + 5e-4 and worst[1] >= -0.108 - 5e-4                           # the figures the header states


def test_true_peak_is_never_under_the_sample_peak():
    rng = np.random.default_rng(5)
    for sr in (16000, 22050, 48000):
        x = (0.3 * rng.standard_normal(4001)).astype(np.float32)
        assert E.true_peak(x, sr) >= E.sample_peak(x) > 0
    x = (0.3 * rng.standard_normal(4001)).astype(np.float32)
    assert E.oversample(192000) == 1 and E.true_peak(x, 192000) == E.sample_peak(x)         # one phase: the samples themselves
    bad = x.copy()
    bad[100], bad[2000] = np.nan, np.inf
    assert E.true_peak(bad, 16000) == np.inf                                                # a NaN never wins, an Inf does
    bad[2000] = 0.0
    assert np.isfinite(E.true_peak(bad, 16000)) and E.true_peak(bad, 16000) >= E.sample_peak(np.nan_to_num(bad))


def test_ringing_in_front_of_and_behind_the_signal_counts():
    """one full-scale sample: the interpolated crest beside it lies in front of sample 0 as often as behind it"""
    x = np.zeros(1, np.float32)
    x[0] = 1.0
    y = E.interpolate(x, 16000)
    assert y.shape == (1 + E.Z, 12) and E.true_peak(x, 16000) == 1.0
    h = E.table(16000).astype(np.float64)
    assert np.array_equal(y[0, 1:], h[1:, 23]) and np.array_equal(y[E.Z, 1:], h[1:, E.Z - 1]) and np.array_equal(y[E.Z - 1, 1:], h[1:, E.Z])


@pytest.mark.parametrize("spec, want", E.TECH_3342)
def test_tech_3342_synthetic_cases(spec, want):
    m = E.case(spec)
    assert E.gate_margin(m) >= MARGIN, "a block lies on a gate: choose another input, not another bar"
    print(f"{spec}: LRA {m['lra']:.4f} (P10 {m['p10']:.4f}, P95 {m['p95']:.4f}), {m['nst']} / {m['n_abs']} / {m['n_rel']} blocks, "
          f"gate {m['gamma']:.4f}, margin {E.gate_margin(m):.3g} LU")
    assert abs(m["lra"] - want) <= 1.0                                                      # Tech 3342's own tolerance
    assert abs(m["lra"] - want) <= 1e-3                                                     # and what this rule reads


def test_relative_gate_of_the_range():
    m = E.case(E.REL_GATE_CASE)
    margin = E.gate_margin(m)
    assert margin >= MARGIN, "a block lies on a gate: choose another input, not another bar"
    print(f"relative gate: LRA {m['lra']:.4f}, gate {m['gamma']:.4f}, margin {margin:.3f} LU")
    assert (m["nst"], m["n_abs"], m["n_rel"]) == (171, 171, 171) and abs(margin - 0.98) <= 0.01
    assert abs(m["lra"] - 22.0) <= 1e-3
    wrong = E.case(E.REL_GATE_CASE, -18.0)                                                  # the gate 2 LU higher cuts the quiet half off
    print(f"with the gate at -18: LRA {wrong['lra']:.4f}, {wrong['n_rel']} blocks")
    assert abs(wrong["lra"] - 4.31) <= 0.01 and wrong["n_rel"] < 171


def test_absolute_gate_of_the_range():
    m = E.case(E.ABS_GATE_CASE)
    margin = E.gate_margin(m)
    assert margin >= MARGIN, "a block lies on a gate: choose another input, not another bar"
    print(f"absolute gate: LRA {m['lra']:.4f}, gate {m['gamma']:.4f}, margin {margin:.3f} LU")
    assert (m["nst"], m["n_abs"], m["n_rel"]) == (221, 200, 180) and abs(margin - 0.10) <= 0.01
    assert abs(m["lra"] - 22.0) <= 1e-3


def test_shortest_and_poisoned_utterances():
    one = E.short_term(R.sine(1000.0, 16000, 3.0, level=-23.0), 16000)
    assert (one["nst"], one["n_abs"], one["n_rel"]) == (1, 1, 1) and one["lra"] == 0.0 and abs(one["p10"] - (-23.0)) <= 0.01
    assert one["smax"] == one["p10"] == one["p95"] == one["s"][0]
    none = E.short_term(R.sine(1000.0, 16000, 2.9, level=-23.0), 16000)
    assert none["nst"] == 0 and np.isnan(none["lra"]) and np.isnan(none["p10"]) and none["gamma"] == -np.inf and none["smax"] == -np.inf
    silent = E.short_term(np.zeros(4 * 16000, np.float32), 16000)
    assert (silent["nst"], silent["n_abs"], silent["n_rel"]) == (11, 0, 0) and np.isnan(silent["lra"])
    x = R.sine(1000.0, 16000, 5.0, level=-23.0).copy()
    x[30000] = np.nan
    bad = E.short_term(x, 16000)
    assert bad["nst"] == 21 and bad["n_rel"] == 21 and np.isnan(bad["lra"]) and np.isnan(bad["gamma"]) and np.isnan(bad["p95"])


@pytest.mark.parametrize("n", [1, 2, 6, 7, 11, 20, 21, 101])
def test_percentile_index_is_tech_3342s_rounding(n):
    """Tech 3342: the element round((n - 1) p / 100 + 1) of the 1-based sorted list, halves away from zero"""
    for p in (10, 95):
        want = int(math.floor((n - 1) * p / 100.0 + 1.0 + 0.5)) - 1
        assert E.percentile_index(n, p) == want and 0 <= want < n


def test_gain_rule_under_a_true_peak_ceiling():
    free = E.gain_tp(-30.0, -23.0, 0.1, -1.0)
    assert free == np.float32(10.0 ** (7.0 / 20.0))                                         # the ceiling does not bind: to nearest
    g = E.gain_tp(-30.0, -10.0, 0.9, -1.0)
    cap = 10.0 ** (-1.0 / 20.0) / 0.9
    assert float(g) <= cap < float(np.nextafter(g, np.float32(2)))                           # binds: the largest f32 at or under the cap
    assert E.gain_tp(-np.inf, -23.0, 0.5, -1.0) == E.gain_tp(np.nan, -23.0, 0.5, -1.0) == np.float32(1.0)
    assert E.gain_tp(-30.0, -23.0, 0.0, -1.0) == free                                       # no peak, no cap


def ws_formula(B, ns, o):
    r = lambda v: max(256, (v + 255) & ~255)
    return (r(4 * (4 * ((B + 3) // 4) + 32 + 24 * o)) + r(32 * B * ns) + r(8 * B * ns) + r(12 * B) + r(64 * B) + r(8 * B * max(ns - 29, 0)))


@pytest.mark.parametrize("sr, L", [(16000, 1), (16000, 47999), (16000, 48000), (16000, 49600), (16000, 57600000), (22050, 70000), (8000, 30000),
                                   (48000, 144001), (192000, 600000)])
def test_query_geometry_and_bytes(rt, sr, L):
    o, taps, tile, nst, ws = rt.ebu_query(sr, L)
    h = sr // 10
    assert (o, taps, tile) == (E.oversample(sr), 24, 1024) and nst == max(0, L // h - 29)
    assert ws == ws_formula(1, L // h, o)
    if L <= 50000:
        assert nst == E.short_term_of_sums(np.zeros(L // h), h)["nst"]


@pytest.mark.parametrize("sr, L", [(0, 1000), (7990, 1000), (16001, 1000), (192010, 1000), (-16000, 1000), (16000, 0), (16000, -3), (16000, 2 ** 31)])
def test_query_rejects(rt, sr, L):
    with pytest.raises(rt.NativeError):
        rt.ebu_query(sr, L)
    assert rt.load_library().mt2_last_error()


def test_table_call_rejects(rt):
    lib = rt.load_library()
    buf = np.zeros(24 * 24, np.float32)
    for sr in (0, 7990, 16005, 192010):
        assert lib.mt2_true_peak_table(sr, buf.ctypes.data_as(C.c_void_p)) != 0 and b"sample_rate" in lib.mt2_last_error()
    assert lib.mt2_true_peak_table(16000, None) != 0 and b"null table" in lib.mt2_last_error()
    assert not buf.any()


def test_calls_refuse_on_the_host_with_a_null_handle(rt):
    """every refusal is decided before the handle is looked at, let alone the device: with a NULL handle and pointers that are never
    followed, each bad argument is named in the error - and the valid call gets as far as the handle"""
    lib = rt.load_library()
    lens = np.array([3000, 3000], np.int32)
    wav, out, stats, mom, sht = (C.c_void_p(a) for a in (0x10000, 0x100000, 0x200000, 0x300000, 0x400000))

    def measure(lens=lens, L_max=3000, B=2, sr=16000, wav=wav, stats=stats, mom=mom, NB_max=1, sht=sht, NST_max=1):
        return lib.mt2_loudness_ebu(None, None, wav, rt._iptr(lens), L_max, B, sr, stats, mom, NB_max, sht, NST_max)

    def normalize(lens=lens, L_max=3000, B=2, sr=16000, target=-23.0, ceiling=-1.0, wav=wav, out=out, stats=stats):
        return lib.mt2_loudness_normalize_tp(None, None, wav, rt._iptr(lens), L_max, B, sr, target, ceiling, out, stats)

    def refused(rc, word):
        assert rc != 0
        msg = lib.mt2_last_error().decode()
        assert word in msg, msg

    refused(measure(), "null model handle")
    refused(measure(mom=None, NB_max=0, sht=None, NST_max=0), "null model handle")
    refused(normalize(), "null model handle")
    refused(normalize(out=wav, stats=None), "null model handle")                              # in place is allowed
    for call in (measure, normalize):
        refused(call(B=0), "B outside")
        refused(call(B=65536), "B outside")
        refused(call(lens=np.array([3000, 0], np.int32)), "length outside")
        refused(call(lens=np.array([3001, 3000], np.int32)), "length outside")
        for sr in (7990, 16005, 192010, 0):
            refused(call(sr=sr), "sample_rate")
        refused(call(wav=None), "bad buffers")
    refused(measure(stats=None), "null stats")
    refused(measure(lens=np.array([16000, 3000], np.int32), L_max=16000, NB_max=6), "NB_max")      # 7 blocks
    refused(measure(NB_max=0), "NB_max")
    refused(measure(lens=np.array([49600, 3000], np.int32), L_max=49600, NB_max=28, NST_max=1), "NST_max")      # 2 short-term blocks
    refused(measure(NST_max=0), "NST_max")
    refused(measure(stats=C.c_void_p(0x10000 + 8)), "overlapping")
    refused(measure(stats=C.c_void_p(0x300000 - 8 * 18)), "overlapping")                      # the second row reaches into momentary
    refused(measure(sht=C.c_void_p(0x200000 + 8 * 18)), "overlapping")                        # short_term inside stats
    refused(measure(sht=C.c_void_p(0x300000 + 8)), "overlapping")                             # short_term inside momentary
    refused(measure(sht=C.c_void_p(0x10000 + 16)), "overlapping")
    refused(normalize(out=None), "null out")
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(normalize(target=bad), "finite")
        refused(normalize(ceiling=bad), "finite")
    refused(normalize(out=C.c_void_p(0x10000 + 4 * 3000)), "out overlaps wav")                 # out's first row is wav's second
    refused(normalize(out=C.c_void_p(0x10000 + 4)), "out overlaps wav")
    refused(normalize(stats=C.c_void_p(0x100000 + 64)), "overlapping")
    refused(normalize(stats=C.c_void_p(0x10000 + 4 * 6000 - 8)), "overlapping")


def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_ebu_query", "mt2_true_peak_table", "mt2_loudness_ebu", "mt2_loudness_normalize_tp"):
        assert hasattr(lib, name) and name in header
    assert "MT2_EBU_FIELDS 18" in header and rt.EBU_FIELDS == 18
    assert f"MT2_TP_TILE {rt.TP_TILE}" in header and f"MT2_TP_TAPS {rt.TP_TAPS}" in header and f"MT2_TP_ZERO_CROSSINGS {rt.TP_ZERO_CROSSINGS}" in header
    assert (rt.TP_ZERO_CROSSINGS, rt.TP_TAPS) == (E.Z, E.TAPS)
    for word in ("Tech 3342", "Annex 2", "beta = 8", "((n - 1) 95 + 50) / 100", "unpinned"):
        assert word in header
    assert callable(rt.MelFrontEnd.loudness_ebu) and callable(rt.ebu_query) and callable(rt.true_peak_table)
    import inspect
    from megatts2_amd import megatts2
    assert inspect.signature(rt.MelFrontEnd.loudness_normalize).parameters["true_peak_ceiling_dbtp"].default is None
    assert inspect.signature(megatts2.measure_loudness).parameters["ebu"].default is False
    assert inspect.signature(megatts2.Megatts.synthesize).parameters["true_peak_ceiling_dbtp"].default is None
    assert inspect.signature(megatts2.Megatts.forward).parameters["true_peak_ceiling_dbtp"].default is None
