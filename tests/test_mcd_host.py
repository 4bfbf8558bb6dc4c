"""Host side of the mel-cepstral distortion (no GPU): the restatement of the rule (tests/mcd_ref.py) against ground truth that needs no
outside tool - a cosine added to every frame of a log-mel reads (10 / ln 10) a / sqrt 2 dB, a gain or a cosine beyond the order reads
0, a copy with repeated frames reads exactly 0 - inside a bound derived from the number formats (mcd_ref.db_bound), and what the
library decides without a HIP call: its exports, mt2_mcd_table against the double formula, mt2_mcd_query against the carve, and every
refusal with the outputs untouched."""
import math
import os

import numpy as np
import pytest

import dtw_ref
import mcd_ref as R

TS = (1, 2, 37, 130)
N, K = 80, 13


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


# ---- the restatement itself ------------------------------------------------------------------------------------------------------

def test_fma32_is_one_rounding():
    """against exact rational arithmetic, on operands chosen to land near f32 midpoints"""
    from fractions import Fraction
    rng = np.random.default_rng(0)
    a = rng.standard_normal(4000).astype(np.float32)
    b = rng.standard_normal(4000).astype(np.float32)
    c = (-(a.astype(np.float64) * b.astype(np.float64)) * (1 + rng.integers(-3, 4, 4000) * 2.0 ** -24)).astype(np.float32)
    c[::3] = rng.standard_normal(c[::3].size).astype(np.float32) * 1e-3
    got = R.fma32(a, b, c)
    for x, y, z, g in zip(a[:600], b[:600], c[:600], got[:600]):
        exact = Fraction(float(x)) * Fraction(float(y)) + Fraction(float(z))
        lo, hi = np.nextafter(g, np.float32(-np.inf)), np.nextafter(g, np.float32(np.inf))
        assert abs(exact - Fraction(float(g))) <= min(abs(exact - Fraction(float(lo))), abs(exact - Fraction(float(hi))))


def test_chain_is_inside_the_coefficient_bound():
    for T in TS:
        mel = R.log_mel(T, N, seed=T)
        err = np.abs(R.cepstrum32_chain(mel, K).astype(np.float64) - R.cepstrum64(mel, K))
        bound = R.coefficient_bound(mel, K)
        assert (err <= bound).all()
        print(f"T={T}: chain error at most {float((err / bound).max()):.3f} of the bound")


def test_table_makes_the_cosines_orthogonal():
    """sum_m cos(theta_m k0) tab[k-1][m] = 1/2 for k = k0 in 1 .. K, 0 otherwise (k0 = 0 and k0 = K + 1 included)"""
    tab = R.table64(N, K)
    for k0 in range(0, K + 2):
        c = tab @ np.cos(np.pi * (np.arange(N) + 0.5) * k0 / N)
        want = np.zeros(K)
        if 1 <= k0 <= K:
            want[k0 - 1] = 0.5
        assert np.abs(c - want).max() < 1e-14


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("a, k0, db", [(0.5, 1, 1.535463), (1.0, 13, 3.070926), (0.25, 7, None)])
def test_a_cosine_reads_its_rms_in_db(T, a, k0, db):
    A = R.log_mel(T, N, seed=10 + T)
    Bm = R.cos_mel(A, a, k0)
    r = R.distortion(A, Bm, K)
    want = R.DB * a / math.sqrt(2.0)
    if db is not None:
        assert abs(want - db) < 5e-7
    delta = np.zeros(K)
    delta[k0 - 1] = a / 2
    bound = R.db_bound(A, Bm, K, delta)
    print(f"T={T} a={a} k0={k0}: mcd {r['row'][1]:.9f}, {want:.9f} expected, off by {abs(r['row'][1] - want):.3g} = "
          f"{abs(r['row'][1] - want) / bound:.4f} of the bound {bound:.3g}")
    assert r["steps"] == T and r["lo"].tolist() == r["hi"].tolist() == list(range(T)) and r["row"][0] == T
    assert abs(r["row"][1] - want) <= bound and abs(r["row"][2] - want) <= bound
    assert (r["row"][3:] == 0).all()


@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("a, k0", [(0.7, 0), (1.0, K + 1)])
def test_a_gain_or_a_cosine_beyond_the_order_reads_zero(T, a, k0):
    A = R.log_mel(T, N, seed=20 + T)
    Bm = R.cos_mel(A, a, k0)
    r = R.distortion(A, Bm, K)
    bound = R.db_bound(A, Bm, K, np.zeros(K))
    print(f"T={T} k0={k0}: mcd {r['row'][1]:.3g} = {r['row'][1] / bound:.4f} of the bound {bound:.3g}")
    assert r["steps"] == T and r["row"][0] == T
    assert 0.0 <= r["row"][1] <= r["row"][2] <= bound


@pytest.mark.parametrize("T", TS)
def test_a_copy_with_repeated_frames_reads_exactly_zero(T):
    rng = np.random.default_rng(30 + T)
    A = R.log_mel(T, N, seed=30 + T)
    Bm = dtw_ref.warp_rows(A, rng.integers(1, 4, T))
    r = R.distortion(A, Bm, K)
    assert r["steps"] == Bm.shape[0] and r["total"] == 0.0
    assert r["row"][0] == Bm.shape[0] and r["row"][1] == 0.0 and r["row"][2] == 0.0


def test_f0_fields_follow_rule_5():
    """a track against itself raised by c cents: RMSE |c|, offset -c (a over b); unvoiced and NaN frames are voicing errors on one
    side only and nothing on both"""
    T, c = 9, 35.0
    cost = np.zeros((T, T), np.float32)
    lo = hi = np.arange(T, dtype=np.int32)
    fa = np.linspace(100, 180, T).astype(np.float32)
    fb = (fa.astype(np.float64) * 2.0 ** (c / 1200)).astype(np.float32)
    row = R.path_row(cost, lo, hi, fa, fb)
    assert row[0] == T and row[3] == T and row[6] == 0 and abs(row[4] - c) < 1e-3 and abs(row[5] + c) < 1e-3
    fa[0], fa[1], fb[1], fb[2], fa[3], fb[3] = 0.0, np.nan, 0.0, np.nan, -5.0, np.nan
    row = R.path_row(cost, lo, hi, fa, fb)
    assert row[3] == T - 4 and row[6] == 2 and row[7] == 2 / T           # frames 0 and 2: one side; 1 and 3: neither
    assert (R.path_row(cost, lo, hi)[3:] == 0).all()


def test_path_row_order_is_the_kernels():
    """one column with a long run and 600 columns of one cell: the partial sums are per thread, the tree joins them"""
    rng = np.random.default_rng(5)
    cost = rng.random((3, 600)).astype(np.float32)
    lo, hi = np.ones(600, np.int32), np.ones(600, np.int32)
    lo[0], hi[-1] = 0, 2
    row = R.path_row(cost, lo, hi)
    db = R.cell_db(cost)
    part = np.zeros(R.THREADS)
    for j in range(600):
        for i in range(lo[j], hi[j] + 1):
            part[j % R.THREADS] += db[i, j]
    assert row[0] == 602 and row[1] == R.tree_sum(part) / 602 and row[2] == max(db[1].max(), db[0, 0], db[2, -1])


# ---- the library without a device ------------------------------------------------------------------------------------------------

def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_mcd_table", "mt2_mcd_query", "mt2_mel_cepstrum", "mt2_path_distortion", "mt2_mel_cepstral_distortion"):
        assert hasattr(lib, name) and name in header
    assert "MT2_MCD_FIELDS 8" in header and "MT2_MCD_MAX_ORDER 32" in header
    assert (rt.MCD_FIELDS, rt.MCD_MAX_ORDER, rt.MCD_NAMES) == (R.FIELDS, R.MAX_ORDER, R.NAMES)
    from megatts2_amd import megatts2 as M
    assert hasattr(M, "mel_cepstral_distortion") and hasattr(M, "compare_audio")
    for cls in (rt.NativeModel, rt.MelFrontEnd):
        assert all(hasattr(cls, n) for n in ("mel_cepstrum", "path_distortion", "mcd"))


@pytest.mark.parametrize("n_mels, order", [(2, 1), (80, 13), (80, 32), (128, 32), (33, 32), (8, 7)])
def test_table_is_the_double_formula_rounded_once(rt, n_mels, order):
    got = rt.mcd_table(n_mels, order)
    assert got.dtype == np.float32 and got.shape == (order, n_mels)
    assert np.array_equal(got, R.table32(n_mels, order))


@pytest.mark.parametrize("n_mels, order", [(1, 1), (129, 13), (80, 0), (80, 33), (8, 8), (2, 2), (80, -1)])
def test_table_and_query_refuse_n_and_k_outside_their_ranges(rt, n_mels, order):
    with pytest.raises(rt.NativeError):
        rt.mcd_table(n_mels, order)
    with pytest.raises(rt.NativeError):
        rt.mcd_query(10, 10, n_mels, order, 1)


def carve(Ta, Tb, Kk, B):
    """mcd_carve by hand: every piece rounded up to 256 bytes, never none"""
    r = lambda n: max(256, (n + 255) // 256 * 256)
    skewed = 4 * B * ((Ta + 63) // 64) * 64 * ((Tb + 63 + 63) // 64) * 64
    return (r(4 * (4 * ((B + 3) // 4) + B)) + r(skewed) + r(4 * B * Ta * ((Tb + 15) // 16)) + r(4 * B * Ta * Kk) + r(4 * B * Tb * Kk)
            + 2 * r(4 * B * Tb) + 2 * r(4 * B))


@pytest.mark.parametrize("Ta, Tb, Kk, B", [(1, 1, 1, 1), (431, 500, 13, 1), (1875, 1875, 13, 8), (4096, 4096, 32, 1), (63, 17, 5, 3), (4096, 1, 13, 2)])
def test_query_is_the_carve(rt, Ta, Tb, Kk, B):
    assert rt.mcd_query(Ta, Tb, 80, Kk, B) == carve(Ta, Tb, Kk, B)
    assert rt.mcd_query(Ta, Tb, 128, Kk, B) == carve(Ta, Tb, Kk, B)           # n_mels does not enter


@pytest.mark.parametrize("Ta, Tb, B", [(0, 5, 1), (5, 0, 1), (4097, 5, 1), (5, 4097, 1), (5, 5, 0), (5, 5, 65536), (5, 5, -1)])
def test_query_refuses(rt, Ta, Tb, B):
    with pytest.raises(rt.NativeError):
        rt.mcd_query(Ta, Tb, 80, 13, B)


SENT = -77.25


def buffers(B, Ta, Tb, n_mels, order):
    """host arrays standing in for device buffers: a refused call never reads or writes them"""
    f = lambda *s: np.full(s, SENT, np.float32)
    return {"mel_a": f(B, Ta, n_mels), "mel_b": f(B, Tb, n_mels), "ca": f(B, Ta, order), "cb": f(B, Tb, order), "f0_a": f(B, Ta), "f0_b": f(B, Tb),
            "lo": np.full((B, Tb), -7, np.int32), "hi": np.full((B, Tb), -7, np.int32), "out": np.full((B, 8), SENT, np.float64)}


def untouched(bufs):
    return all((v == (-7 if v.dtype == np.int32 else SENT)).all() for v in bufs.values())


def test_mel_cepstrum_refuses_on_the_host(rt):
    lib = rt.load_library()

    def why(lens, T, n_mels=80, order=13, B=None, overlap=False, null=False):
        lens = np.asarray(lens, np.int32)
        n = lens.size if B is None else B
        bufs = buffers(max(min(n, 2), 1), max(T, 1), 1, max(n_mels, 1), max(n_mels, 1))
        cep = bufs["mel_a"] if overlap else bufs["ca"]
        rc = lib.mt2_mel_cepstrum(None, None, None if null else rt._iptr(bufs["mel_a"]), rt._iptr(lens), T, n, n_mels, order, rt._iptr(cep))
        assert rc != 0 and untouched(bufs)
        return lib.mt2_last_error().decode()

    assert "null model handle" in why([5, 3], 5)
    assert "B outside" in why([5], 5, B=0)
    assert "B outside" in why([5], 5, B=65536)
    assert "n_mels" in why([5], 5, n_mels=1)
    assert "n_mels" in why([5], 5, n_mels=129)
    assert "order" in why([5], 5, order=0)
    assert "order" in why([5], 5, n_mels=8, order=8)
    assert "order" in why([5], 5, order=33)
    assert "T_max" in why([5], 0)
    assert "T_max" in why([5], 4097)
    assert "frame count" in why([5, 6], 5)
    assert "frame count" in why([0, 5], 5)
    assert "overlapping" in why([5], 5, overlap=True)
    assert "bad buffers" in why([5], 5, null=True)


def pair_refusals(rt, call):
    """what mt2_path_distortion and mt2_mel_cepstral_distortion refuse alike; call(a_lens, Ta, b_lens, Tb, **kw) -> the error text"""
    assert "null model handle" in call([5, 3], 5, [9, 9], 9)
    assert "null model handle" in call([5, 3], 5, [9, 9], 9, f0="both")
    assert "a length" in call([5, 6], 5, [9, 9], 9)
    assert "a length" in call([0, 5], 5, [9, 9], 9)
    assert "b length" in call([5, 3], 5, [9, 10], 9)
    assert "b length" in call([5, 3], 5, [0, 9], 9)
    assert "Ta_max" in call([5], 4097, [9], 9)
    assert "Ta_max" in call([5], 0, [9], 9)
    assert "Tb_max" in call([5], 5, [9], 4097)
    assert "Tb_max" in call([5], 5, [9], 0)
    assert "B outside" in call([5], 5, [9], 9, B=0)
    assert "B outside" in call([5], 5, [9], 9, B=65536)
    assert "order" in call([5], 5, [9], 9, order=0)
    assert "order" in call([5], 5, [9], 9, order=33)
    assert "one F0 track" in call([5], 5, [9], 9, f0="a")
    assert "one F0 track" in call([5], 5, [9], 9, f0="b")
    assert "overlapping" in call([5], 5, [9], 9, overlap="out-a")
    assert "overlapping" in call([5], 5, [9], 9, overlap="out-f0")


def test_path_distortion_refuses_on_the_host(rt):
    lib = rt.load_library()

    def why(al, Ta, bl, Tb, order=13, B=None, f0=None, overlap=None, no_path=False):
        al, bl = np.asarray(al, np.int32), np.asarray(bl, np.int32)
        n = al.size if B is None else B
        bufs = buffers(max(min(n, 2), 1), max(Ta, 2), max(Tb, 1), 80, max(order, 1))
        p = {k: rt._iptr(v) for k, v in bufs.items()}
        out = {None: p["out"], "out-a": p["ca"], "out-f0": p["f0_a"]}[overlap]
        f0 = "both" if overlap == "out-f0" else f0
        rc = lib.mt2_path_distortion(None, None, p["ca"], rt._iptr(al), Ta, p["cb"], rt._iptr(bl), Tb, order, n, None if no_path else p["lo"],
                                     p["hi"], p["f0_a"] if f0 in ("a", "both") else None, p["f0_b"] if f0 in ("b", "both") else None, out)
        assert rc != 0 and untouched(bufs)
        return lib.mt2_last_error().decode()

    pair_refusals(rt, why)
    assert "lo / hi" in why([5], 5, [9], 9, no_path=True)


def test_whole_chain_refuses_on_the_host(rt):
    lib = rt.load_library()

    def why(al, Ta, bl, Tb, order=13, B=None, f0=None, overlap=None, n_mels=80):
        al, bl = np.asarray(al, np.int32), np.asarray(bl, np.int32)
        n = al.size if B is None else B
        bufs = buffers(max(min(n, 2), 1), max(Ta, 2), max(Tb, 1), max(n_mels, 1), 1)
        p = {k: rt._iptr(v) for k, v in bufs.items()}
        out = {None: p["out"], "out-a": p["mel_a"], "out-f0": p["f0_a"], "lo-hi": p["out"]}[overlap]
        f0 = "both" if overlap == "out-f0" else f0
        rc = lib.mt2_mel_cepstral_distortion(None, None, p["mel_a"], rt._iptr(al), Ta, p["mel_b"], rt._iptr(bl), Tb, n_mels, order, n,
                                             p["f0_a"] if f0 in ("a", "both") else None, p["f0_b"] if f0 in ("b", "both") else None, out,
                                             p["lo"], p["lo"] if overlap == "lo-hi" else p["hi"])
        assert rc != 0 and untouched(bufs)
        return lib.mt2_last_error().decode()

    pair_refusals(rt, why)
    assert "n_mels" in why([5], 5, [9], 9, n_mels=1)
    assert "n_mels" in why([5], 5, [9], 9, n_mels=129)
    assert "order" in why([5], 5, [9], 9, n_mels=8, order=8)
    assert "overlapping" in why([5], 5, [9], 9, overlap="lo-hi")
