"""Host side of the integrated-loudness stage (no GPU): the float64 restatement of the rule (tests/loudness_ref.py) against the
standard's own figures - the 48 kHz coefficient table, -3.01 LKFS for a full-scale 997 Hz sine at 48 kHz - and the analytic
steady-state reading of a sine at other rates; both gates on inputs whose blocks keep a stated distance from them; the chunked form
of the recurrence against the serial one; and the library's host-only entry point mt2_loudness_query, its refusals and exports."""
import ctypes as C
import os

import numpy as np
import pytest

import loudness_ref as R

# ITU-R BS.1770-4, table 1 and 2 (48 kHz)
STD_SHELF = (1.53512485958697, -2.69169618940638, 1.19839281085285, -1.69065929318241, 0.73248077421585)
STD_HP = (1.0, -2.0, 1.0, -1.99004745483398, 0.99007225036621)
MARGIN = 1e-3


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


def test_coefficients_at_48k_are_the_standards_table(rt):
    want = np.array(STD_SHELF + STD_HP)
    assert np.abs(R.coeffs(48000) - want).max() <= 1e-12
    h, nb, c, _ = rt.loudness_query(48000, 3 * 48000)
    assert (h, nb) == (4800, 27)
    assert np.abs(c - want).max() <= 1e-12


@pytest.mark.parametrize("sr", [8000, 16000, 22050, 44100, 96000, 192000])
def test_query_coefficients_match_restatement(rt, sr):
    c = rt.loudness_query(sr, sr)[2]
    ref = R.coeffs(sr)
    assert np.abs(c - ref).max() <= 1e-13 * np.abs(ref).max()


def test_standard_ground_truth_997_hz_at_48k():
    m = R.measure(R.sine(997.0, 48000, 3.0), 48000)
    assert abs(m["I"] - (-3.01)) <= 0.01
    assert m["nb"] == m["n_abs"] == m["n_rel"] == 27


@pytest.mark.parametrize("sr, printed", [(16000, -2.9701), (22050, -2.9810), (24000, -2.9843), (44100, -3.0075)])
def test_analytic_ground_truth_of_sines(sr, printed):
    """the steady-state reading follows from the transfer function; the start-up transient of the first blocks is the whole
    difference.  100 Hz sits on the high-pass's slope, 4 kHz on the shelf's; at 100 Hz the transient is a larger share of the
    reading (1.05e-3 LU of a 3 s clip at 16 kHz), so that tone runs 6 s, which halves it."""
    want = R.sine_reading(997.0, sr)
    assert abs(want - printed) <= 5e-5 and abs(want - (-3.01)) <= 0.1          # EBU Tech 3341's tolerance
    for f, seconds in R.SINE_CASES:
        got = R.measure(R.sine(f, sr, seconds), sr)["I"]
        print(f"sr {sr} f {f}: {got:.6f} against {R.sine_reading(f, sr):.6f}")
        assert abs(got - R.sine_reading(f, sr)) <= 1e-3
    assert R.sine_reading(100.0, sr) < R.sine_reading(997.0, sr) < R.sine_reading(4000.0, sr)


def test_scaling_by_20_db_lowers_the_reading_by_20_lu():
    x = (0.3 * np.random.default_rng(1).standard_normal(3 * 16000)).astype(np.float64)
    a, b = R.measure(x, 16000), R.measure(x * 10.0 ** (-20.0 / 20.0), 16000)
    assert R.gate_margin(a) >= MARGIN and R.gate_margin(b) >= MARGIN
    assert (a["n_abs"], a["n_rel"]) == (b["n_abs"], b["n_rel"])               # no block changed sides of a gate
    assert abs((a["I"] - b["I"]) - 20.0) <= 1e-9


def test_relative_gate():
    m = R.measure(R.gating_case(), 16000)
    assert R.gate_margin(m) >= MARGIN, "a block lies on a gate: choose another input, not another bar"
    assert (m["nb"], m["n_abs"], m["n_rel"]) == (97, 97, 63)
    assert abs(m["I"] - (-23.201)) <= 1e-3
    assert abs(m["I"] - (-23.0)) <= 0.25 and abs(m["I"] - m["ungated"]) > 1.5


def test_absolute_gate():
    m, p = R.measure(R.gating_case(), 16000), R.measure(R.gating_case(pad=True), 16000)
    assert R.gate_margin(p) >= MARGIN, "a block lies on a gate: choose another input, not another bar"
    assert p["nb"] == 137 and p["n_rel"] == 63 and p["n_abs"] < 137
    assert abs(p["I"] - m["I"]) < 1e-9


@pytest.mark.parametrize("sr", [16000, 22050])
def test_shortest_utterances(sr):
    x = R.sine(997.0, sr, 0.5)
    n = 4 * (sr // 10)
    short, one = R.measure(x[:n - 1], sr), R.measure(x[:n], sr)
    assert short["nb"] == 0 and short["I"] == -np.inf and short["gamma"] == -np.inf and short["lmax"] == -np.inf
    assert R.gain(short["I"], -23.0) == np.float32(1.0)
    assert (one["nb"], one["n_abs"], one["n_rel"]) == (1, 1, 1) and np.isfinite(one["I"]) and one["I"] == one["lmax"]
    assert R.measure(np.zeros(sr), sr)["I"] == -np.inf and R.measure(np.zeros(sr), sr)["nb"] == 7


def test_nan_poisons_its_own_reading():
    x = R.sine(997.0, 16000, 1.0).copy()
    x[9000] = np.nan
    m = R.measure(x, 16000)
    assert np.isnan(m["I"]) and R.gain(m["I"], -23.0) == np.float32(1.0)
    assert np.isfinite(m["l"][:2]).all() and np.isnan(m["l"][2:]).all()          # from the sub-block that holds it on
    assert m["peak"] == float(np.nanmax(np.abs(x)))


@pytest.mark.parametrize("c", [25, 100, 1600])
def test_chunked_form_is_the_serial_one(c):
    x = (0.1 * np.random.default_rng(2).standard_normal(3 * 16000)).astype(np.float32)
    x[20000:30000] *= 1e-3                                                       # a quiet stretch behind a loud one
    S, Sc = R.sub_block_sums(x, 16000), R.sub_block_sums_chunked(x, 16000, c)
    print(f"c {c}: worst relative difference {np.max(np.abs(Sc - S) / S):.3g}")
    assert (np.abs(Sc - S) <= 1e-12 * S).all()
    rho = np.abs(np.linalg.eigvals(R.carry_matrix(16000, c))).max()
    assert rho < 1.0 and (c != 1600 or rho < 1e-9)


def test_agrees_with_scipy_lfilter():
    sig = pytest.importorskip("scipy.signal")
    x = (0.1 * np.random.default_rng(3).standard_normal(3 * 16000)).astype(np.float32)
    c = R.coeffs(16000)
    y = sig.lfilter(c[5:8], [1.0, c[8], c[9]], sig.lfilter(c[0:3], [1.0, c[3], c[4]], x.astype(np.float64)))
    assert np.abs(R.kweight(x, 16000) - y).max() <= 1e-12 * np.abs(y).max()


def test_gain_rule():
    assert R.gain(-30.0, -23.0) == np.float32(10.0 ** (7.0 / 20.0))
    g = R.gain(-30.0, -23.0, peak=0.9, ceiling=1.0)                            # the ceiling binds: 0.9 g <= 1 in f32
    assert g < np.float32(10.0 ** (7.0 / 20.0)) and float(np.float32(0.9) * g) <= 1.0
    assert float(np.float32(0.9) * np.nextafter(g, np.float32(2))) > 1.0 - 3 * 2.0 ** -24
    assert R.gain(-np.inf, -23.0) == R.gain(np.nan, -23.0) == np.float32(1.0)


def ws_formula(B, ns):
    r = lambda v: max(256, (v + 255) & ~255)
    return r(4 * (4 * ((B + 3) // 4) + 32)) + r(32 * B * ns) + r(8 * B * ns) + r(8 * B)


@pytest.mark.parametrize("sr, L", [(16000, 1), (16000, 1599), (16000, 1600), (16000, 6400), (16000, 480000), (22050, 70000), (48000, 144001)])
def test_query_geometry_and_bytes(rt, sr, L):
    h, nb, _, ws = rt.loudness_query(sr, L)
    assert h == sr // 10 == R.sub_block(sr) and nb == max(0, L // h - 3) == R.measure(np.zeros(min(L, 8 * h)), sr)["nb"] + max(0, L // h - 8)
    assert ws == ws_formula(1, L // h)


@pytest.mark.parametrize("sr, L", [(0, 1000), (7990, 1000), (16001, 1000), (44105, 1000), (192010, 1000), (-16000, 1000), (16000, 0),
                                   (16000, -3), (16000, 2 ** 31)])
def test_query_rejects(rt, sr, L):
    with pytest.raises(rt.NativeError):
        rt.loudness_query(sr, L)
    assert rt.load_library().mt2_last_error()


def test_calls_refuse_on_the_host_with_a_null_handle(rt):
    """every refusal is decided before the handle is looked at, let alone the device: with a NULL handle and pointers that are never
    followed, each bad argument is named in the error - and the valid call gets as far as the handle"""
    lib = rt.load_library()
    lens = np.array([3000, 3000], np.int32)
    wav, out, stats, mom = (C.c_void_p(a) for a in (0x10000, 0x100000, 0x200000, 0x300000))

    def measure(lens=lens, L_max=3000, B=2, sr=16000, wav=wav, stats=stats, mom=mom, NB_max=1):
        return lib.mt2_loudness(None, None, wav, rt._iptr(lens), L_max, B, sr, stats, mom, NB_max)

    def normalize(lens=lens, L_max=3000, B=2, sr=16000, target=-23.0, ceiling=0.0, wav=wav, out=out, stats=stats):
        return lib.mt2_loudness_normalize(None, None, wav, rt._iptr(lens), L_max, B, sr, target, ceiling, out, stats)

    def refused(rc, word):
        assert rc != 0
        msg = lib.mt2_last_error().decode()
        assert word in msg, msg

    refused(measure(), "null model handle")
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
    refused(measure(stats=C.c_void_p(0x10000 + 8)), "overlapping")
    refused(measure(mom=C.c_void_p(0x200000 + 8)), "overlapping")
    refused(normalize(out=None), "null out")
    for bad in (float("nan"), float("inf"), -float("inf")):
        refused(normalize(target=bad), "finite")
        refused(normalize(ceiling=bad), "finite")
    refused(normalize(out=C.c_void_p(0x10000 + 4 * 3000)), "out overlaps wav")                 # out's first row is wav's second
    refused(normalize(out=C.c_void_p(0x10000 + 4)), "out overlaps wav")
    refused(normalize(stats=C.c_void_p(0x100000 + 64)), "overlapping")


def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_loudness_query", "mt2_loudness", "mt2_loudness_normalize"):
        assert hasattr(lib, name) and name in header
    assert "MT2_LOUDNESS_FIELDS 8" in header and rt.LOUDNESS_FIELDS == 8
    for word in ("1681.974450955533", "38.13547087602444", "True peak", "loudness range"):
        assert word in header
    assert callable(rt.MelFrontEnd.loudness) and callable(rt.MelFrontEnd.loudness_normalize) and callable(rt.loudness_query)
    from megatts2_amd import megatts2
    assert callable(megatts2.measure_loudness)
    import inspect
    assert inspect.signature(megatts2.Megatts.synthesize).parameters["loudness_lufs"].default is None
    assert inspect.signature(megatts2.Megatts.forward).parameters["loudness_lufs"].default is None
