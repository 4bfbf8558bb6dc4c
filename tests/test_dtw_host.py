"""Host side of the DTW prompt aligner (no GPU): the float32 restatement of the rule (tests/dtw_ref.py) on the hand cases of the rule's
own statement, the known-warp and X-against-X recoveries, the path invariants on random shapes, and what the library decides
without a HIP call: its exports, mt2_dtw_query against the documented workspace, and the refusals made on the host."""
import os

import numpy as np
import pytest

import dtw_ref as R


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    return runtime


# ---- hand cases: all-zero costs, so every choice is a tie ------------------------------------------------------------------

def test_all_zero_costs_3x5():
    r = R.align(np.zeros((3, 5), np.float32))
    assert r["lo"].tolist() == r["hi"].tolist() == [0, 0, 0, 1, 2] and r["steps"] == 5 and r["total"] == 0.0


def test_all_zero_costs_5x3():
    r = R.align(np.zeros((5, 3), np.float32))
    assert r["lo"].tolist() == [0, 3, 4] and r["hi"].tolist() == [2, 3, 4] and r["steps"] == 5


def test_all_zero_costs_4x4_is_the_diagonal():
    r = R.align(np.zeros((4, 4), np.float32))
    assert r["lo"].tolist() == r["hi"].tolist() == [0, 1, 2, 3] and r["steps"] == 4


def test_single_row_and_single_column():
    r = R.align(np.ones((1, 6), np.float32))
    assert r["lo"].tolist() == r["hi"].tolist() == [0] * 6 and r["steps"] == 6 and r["total"] == 6.0
    r = R.align(np.ones((6, 1), np.float32))
    assert r["lo"].tolist() == [0] and r["hi"].tolist() == [5] and r["steps"] == 6 and r["total"] == 6.0
    r = R.align(np.full((1, 1), 2.5, np.float32))
    assert r["lo"].tolist() == r["hi"].tolist() == [0] and r["steps"] == 1 and r["total"] == 2.5


def choice(diag, up, left):
    """the direction at (1, 1) of the 2 x 2 matrix whose three neighbours accumulate to (diag, up, left) - small integers, exact"""
    A, d = R.accumulate(np.asarray([[diag, up - diag], [left - diag, 0]], np.float32))
    assert (A[0, 0], A[0, 1], A[1, 0]) == (diag, up, left) and A[1, 1] == min(diag, up, left)
    return d[1, 1]


def test_tie_order_is_diagonal_then_up_then_left():
    assert choice(3, 3, 3) == R.DIAG                                  # three-way tie
    assert choice(3, 3, 5) == R.DIAG and choice(3, 5, 3) == R.DIAG    # the diagonal ties with one neighbour
    assert choice(5, 3, 3) == R.UP                                    # up ties with left below the diagonal
    assert choice(5, 3, 4) == R.UP and choice(5, 4, 3) == R.LEFT      # and strict minima
    assert choice(2, 3, 4) == R.DIAG and choice(4, 5, 3) == R.LEFT and choice(4, 3, 5) == R.UP
    _, d = R.accumulate(np.zeros((3, 3), np.float32))
    assert d[0].tolist() == [R.LEFT] * 3 and d[:, 0].tolist() == [R.LEFT, R.UP, R.UP]          # row 0 left, column 0 up


def test_up_left_tie_on_the_path_goes_up():
    """x = (1, -1, 1) against y = -x: A = [[4, 4, 8], [4, 8, 4], [8, 4, 8]]; at (2, 2) the diagonal is 8 and up = left = 4"""
    x = np.asarray([[1], [-1], [1]], np.float32)
    r = R.align(R.cost32_chain(x, -x))
    assert r["acc"].tolist() == [[4, 4, 8], [4, 8, 4], [8, 4, 8]]
    assert r["lo"].tolist() == [0, 0, 1] and r["hi"].tolist() == [0, 0, 2] and r["steps"] == 4 and r["total"] == 8.0


# ---- recoveries ----------------------------------------------------------------------------------------------------------------

def distinct_rows(n, D, seed):
    """rows whose neighbours - and all others - differ: integers, so every square is exact in f32"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (n, D)).astype(np.float32)
    x[:, 0] = np.arange(n) * 3.0              # strictly increasing in one column: no two rows are equal
    return x


@pytest.mark.parametrize("seed", range(4))
def test_known_warp_is_recovered_in_both_directions(seed):
    rng = np.random.default_rng(100 + seed)
    x = distinct_rows(int(rng.integers(3, 40)), 5, seed)
    reps = rng.integers(1, 4, x.shape[0])
    y = R.warp_rows(x, reps)
    ends = np.cumsum(reps)
    r = R.align(R.cost32_chain(x, y))                       # X onto its stretched self: column j sits on the row it repeats
    owner = np.repeat(np.arange(x.shape[0]), reps)
    assert r["total"] == 0.0 and r["lo"].tolist() == r["hi"].tolist() == owner.tolist() and r["steps"] == y.shape[0]
    r = R.align(R.cost32_chain(y, x))                       # the stretched onto the original: column i spans its repeats
    assert r["total"] == 0.0 and r["lo"].tolist() == (ends - reps).tolist() and r["hi"].tolist() == (ends - 1).tolist()
    assert r["steps"] == y.shape[0]
    # the durations of phones of one synthetic frame each are the repeat counts
    assert R.durations(R.align(R.cost32_chain(x, y))["hi"], np.ones(x.shape[0], np.int64)).tolist() == reps.tolist()


@pytest.mark.parametrize("seed", range(4))
def test_x_against_x_returns_the_synthetic_durations_zeros_included(seed):
    rng = np.random.default_rng(200 + seed)
    s = rng.integers(0, 5, int(rng.integers(2, 15)))
    s[rng.integers(0, s.size)] = 0
    if s.sum() == 0:
        s[0] = 3
    x = distinct_rows(int(s.sum()), 4, seed)
    r = R.align(R.cost32_chain(x, x))
    assert r["total"] == 0.0 and r["hi"].tolist() == list(range(x.shape[0]))
    assert R.durations(r["hi"], s).tolist() == s.tolist()


def test_path_invariants_and_duration_sums_on_random_shapes():
    rng = np.random.default_rng(7)
    for _ in range(30):
        Tx, Ty = int(rng.integers(1, 60)), int(rng.integers(1, 60))
        c = rng.random((Tx, Ty)).astype(np.float32)
        if rng.random() < 0.5:
            c = np.round(c * 3).astype(np.float32)          # many ties
        r = R.align(c)
        assert R.check_path(r["lo"], r["hi"], Tx, Ty) == r["steps"]
        assert max(Tx, Ty) <= r["steps"] <= Tx + Ty - 1
        cuts = np.sort(rng.integers(0, Tx + 1, int(rng.integers(1, 9))))
        s = np.diff(np.concatenate([[0], cuts, [Tx]]))      # >= 0, zeros whenever two cuts meet, sum = Tx
        assert s.min() >= 0 and s.sum() == Tx
        dur = R.durations(r["hi"], s)
        assert dur.sum() == Ty and dur.min() >= 0 and (dur[s == 0] == 0).all()


# ---- the library without a device ----------------------------------------------------------------------------------------------

def test_exports(rt):
    lib = rt.load_library()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "megatts2_hip.h")).read()
    for name in ("mt2_dtw_query", "mt2_dtw_align", "mt2_align_durations"):
        assert hasattr(lib, name) and name in header
    assert "MT2_DTW_MAX_LEN 4096" in header and "MT2_DTW_DIR_COLS 16" in header
    assert (rt.DTW_MAX_LEN, rt.DTW_DIR_COLS) == (4096, 16)
    from megatts2_amd import megatts2 as M
    for name in ("align_prompt", "synthesize_prompt_conditioned", "synthesize_prosody_interpolated"):
        assert hasattr(M.Megatts, name)
    assert hasattr(rt.NativeModel, "dtw") and hasattr(rt.NativeModel, "align_durations") and hasattr(rt.MelFrontEnd, "dtw")


def documented_workspace(Tx, Ty, B):
    r = lambda n: (n + 255) // 256 * 256
    skewed = 4 * B * ((Tx + 63) // 64) * 64 * ((Ty + 63 + 63) // 64) * 64
    return r(skewed) + r(4 * B * Tx * ((Ty + 15) // 16)) + r(4 * (2 * B + 8))


@pytest.mark.parametrize("Tx, Ty, B", [(1, 1, 1), (431, 431, 1), (1875, 1875, 8), (4096, 4096, 1), (63, 17, 3), (4096, 1, 2)])
def test_query_is_the_documented_workspace(rt, Tx, Ty, B):
    assert rt.dtw_query(Tx, Ty, 80, B) == documented_workspace(Tx, Ty, B)
    assert rt.dtw_query(Tx, Ty, 1, B) == documented_workspace(Tx, Ty, B)          # D does not enter


@pytest.mark.parametrize("Tx, Ty, D, B", [(0, 5, 80, 1), (5, 0, 80, 1), (4097, 5, 80, 1), (5, 4097, 80, 1), (5, 5, 0, 1), (5, 5, 80, 0),
                                          (5, 5, -1, 1), (5, 5, 80, -2)])
def test_query_rejects(rt, Tx, Ty, D, B):
    with pytest.raises(rt.NativeError):
        rt.dtw_query(Tx, Ty, D, B)
    assert rt.load_library().mt2_last_error()


def test_lengths_up_to_the_cap_are_accepted(rt):
    assert rt.dtw_query(4096, 4096, 80, 1) == documented_workspace(4096, 4096, 1)


def test_align_refuses_geometry_and_lengths_before_it_looks_at_the_handle(rt):
    """with a NULL handle a well-formed call is refused for the handle; an ill-formed one for what is wrong with it - decided first,
    on the host"""
    lib = rt.load_library()

    def why(xl, Tx, yl, Ty, D=80, B=None):
        xl, yl = np.asarray(xl, np.int32), np.asarray(yl, np.int32)
        rc = lib.mt2_dtw_align(None, None, None, rt._iptr(xl), Tx, None, rt._iptr(yl), Ty, D, xl.size if B is None else B, None, None,
                               None, None, None, None)
        assert rc != 0
        return lib.mt2_last_error().decode()

    assert "null model handle" in why([5, 3], 5, [9, 9], 9)
    assert "x length" in why([5, 6], 5, [9, 9], 9)
    assert "x length" in why([5, 0], 5, [9, 9], 9)
    assert "y length" in why([5, 3], 5, [9, 10], 9)
    assert "y length" in why([5, 3], 5, [0, 9], 9)
    assert "Tx_max" in why([5], 4097, [9], 9)
    assert "Ty_max" in why([5], 5, [9], 4097)
    assert "D < 1" in why([5], 5, [9], 9, D=0)
    assert "B outside" in why([5], 5, [9], 9, B=0)


def test_align_durations_refuses_on_the_host(rt):
    lib = rt.load_library()

    def why(yl, Ty, syn, pl, B=None):
        yl, syn, pl = np.asarray(yl, np.int32), np.asarray(syn, np.int32), np.asarray(pl, np.int32)
        out = np.full(syn.shape, -7, np.int32)
        rc = lib.mt2_align_durations(None, None, None, rt._iptr(yl), Ty, rt._iptr(syn), rt._iptr(pl), syn.shape[1],
                                     yl.size if B is None else B, rt._iptr(out))
        assert rc != 0 and (out == -7).all()
        return lib.mt2_last_error().decode()

    assert "null model handle" in why([9], 9, [[2, 3]], [2])
    assert "y length" in why([10], 9, [[2, 3]], [2])
    assert "phone count" in why([9], 9, [[2, 3]], [3])
    assert "phone count" in why([9], 9, [[2, 3]], [0])
    assert "Ty_max" in why([9], 4097, [[2, 3]], [2])
    assert "B outside" in why([9], 9, [[2, 3]], [2], B=0)
