"""The DTW prompt aligner on the GPU (csrc/dtw.hip: mt2_dtw_align, mt2_align_durations) against the restatement of its rule
(tests/dtw_ref.py), and Megatts.align_prompt on the tiny synthetic-weight model.

Bars.  Cost: each cell within (D + 3) * 2^-24 * c64 of the float64 cost of the same f32 inputs (2 u for the squared rounded
difference, D u for the chain, one u of slack, u = 2^-24); largest observed fraction of that bound on an MI355X: 0.749, at
(129, 300) with D = 1, where the bound is 4 u; at D = 80 the largest is 0.12.
Accumulation and path: acc, lo, hi, steps and total BIT-EQUAL to dtw_ref run on the kernel's own cost - no tolerance.  Durations:
equal to dtw_ref.  Padding rows beyond the lengths are NaN in X and Y (a read of one poisons a cost), every output buffer is
pre-filled with a sentinel, is wider than needed (Tx_max / Ty_max exceed the longest utterance) and has guard words behind it.

Shapes (Tx, Ty): the listed (1,1) (1,7) (7,1) (2,2) (63,65) (64,64) (65,63) (129,300) (300,129) (257,1025) at D in {1, 5, 80} - 63 / 64 /
65 also straddle the cost kernel's tile of 64 rows x 64 steps and the accumulate kernel's strip of 64 rows (one lane per row, 64 steps per
period).  The kernels' other constants, straddled by one on each side at D = 5: the 16 columns of a packed direction word and of a
staged k chunk (Ty = 15, 16, 17; D = 15, 16, 17); the half period of 32 steps whose costs are loaded at once and the backtrack
tile of 32 rows x 2 words (Tx, Ty = 31, 32, 33); the ring of 256 columns a strip's bottom row lives in (Ty = 255, 256, 257);
the 16 strips = 1024 rows one pass of the workgroup covers (Tx = 1023, 1024, 1025: the 17th strip waits for the first pass, and
reads the 16th strip's bottom row from the full-width buffer); and the pass length max(chunks + 2, 32) leaving its floor of 32
periods (chunks = ceil((Ty + 63) / 64) = 30, 31 at Ty = 1857, 1858 with Tx = 1030, two passes)."""
import functools

import numpy as np
import pytest

import dtw_ref as R
from conftest import load_golden, synth_models

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

U = 2.0 ** -24
SENT_F, SENT_I = np.float32(-77.25), np.int32(-777)
GUARD = 11
LISTED = [(1, 1), (1, 7), (7, 1), (2, 2), (63, 65), (64, 64), (65, 63), (129, 300), (300, 129), (257, 1025)]
OWN = [(5, 15), (5, 16), (5, 17), (31, 33), (32, 32), (33, 31), (70, 255), (70, 256), (70, 257), (1023, 40), (1024, 33), (1025, 40),
       (1030, 1857), (1030, 1858)]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def frontend():
    from megatts2_amd.runtime import MelFrontEnd
    return MelFrontEnd()


def mel_like(T, D, seed):
    """a smooth random walk with a little noise, in the range of a log-mel: neighbouring rows are close, far ones are not"""
    rng = np.random.default_rng(seed)
    return (np.cumsum(rng.standard_normal((T, D)), axis=0) * 0.3 + rng.standard_normal((T, D)) * 0.05 - 4.0).astype(np.float32)


def run(pairs, extra=(3, 5), fe=None, want=("cost", "acc")):
    """DTW of the (x, y) pairs as ONE batch through the C entry point, with buffers of the test's own making -> per-utterance dicts
    of the whole buffers (so that what lies outside an utterance can be looked at), plus "guards_ok" """
    from megatts2_amd import runtime as rt
    fe = fe or frontend()
    B, D = len(pairs), pairs[0][0].shape[1]
    xl, yl = np.asarray([x.shape[0] for x, _ in pairs], np.int32), np.asarray([y.shape[0] for _, y in pairs], np.int32)
    Tx, Ty = int(xl.max()) + extra[0], int(yl.max()) + extra[1]
    X, Y = np.full((B, Tx, D), np.nan, np.float32), np.full((B, Ty, D), np.nan, np.float32)
    for b, (x, y) in enumerate(pairs):
        X[b, :x.shape[0]], Y[b, :y.shape[0]] = x, y
    fbuf = lambda n: torch.full((n + GUARD,), float(SENT_F), device="cuda", dtype=torch.float32)
    ibuf = lambda n: torch.full((n + GUARD,), int(SENT_I), device="cuda", dtype=torch.int32)
    bufs = {"lo": ibuf(B * Ty), "hi": ibuf(B * Ty), "steps": ibuf(B), "total": fbuf(B),
            "cost": fbuf(B * Tx * Ty) if "cost" in want else None, "acc": fbuf(B * Tx * Ty) if "acc" in want else None}
    Xd, Yd = dev(X), dev(Y)
    rt._check(fe.lib.mt2_dtw_align(fe.h, rt._stream(), rt._ptr(Xd), rt._iptr(xl), Tx, rt._ptr(Yd), rt._iptr(yl), Ty, D, B,
                                   *(rt._ptr(bufs[k]) for k in ("lo", "hi", "steps", "total", "cost", "acc"))))
    host = {k: v.cpu().numpy() for k, v in bufs.items() if v is not None}
    sizes = {"lo": B * Ty, "hi": B * Ty, "steps": B, "total": B, "cost": B * Tx * Ty, "acc": B * Tx * Ty}
    guards_ok = all((host[k][sizes[k]:] == (SENT_I if host[k].dtype == np.int32 else SENT_F)).all() for k in host)
    out = []
    for b in range(B):
        r = {"lo": host["lo"][:B * Ty].reshape(B, Ty)[b], "hi": host["hi"][:B * Ty].reshape(B, Ty)[b], "steps": int(host["steps"][b]),
             "total": host["total"][b], "Tx": int(xl[b]), "Ty": int(yl[b]), "guards_ok": guards_ok}
        for k in ("cost", "acc"):
            if k in host:
                r[k] = host[k][:B * Tx * Ty].reshape(B, Tx, Ty)[b]
        out.append(r)
    return out


def check_cost(r, x, y):
    """-> the largest error as a fraction of the bound"""
    Tx, Ty, D = r["Tx"], r["Ty"], x.shape[1]
    c = r["cost"][:Tx, :Ty]
    assert np.isfinite(c).all()                                         # no NaN padding row was read
    worst = 0.0
    for i0 in range(0, Tx, 64):                                         # float64 cost in slabs of rows
        c64 = R.cost64(x[i0:i0 + 64], y)
        err, bound = np.abs(c[i0:i0 + 64].astype(np.float64) - c64), (D + 3) * U * c64
        assert (err <= bound).all()
        worst = max(worst, float(np.max(err / np.maximum(bound, 1e-300))))
    return worst


def check_against_ref(r):
    """accumulation and path bit-equal to the restatement run on the kernel's OWN cost; nothing outside the utterance touched"""
    Tx, Ty = r["Tx"], r["Ty"]
    ref = R.align(r["cost"][:Tx, :Ty])
    assert np.array_equal(r["acc"][:Tx, :Ty].view(np.uint32), ref["acc"].view(np.uint32))
    assert np.array_equal(r["lo"][:Ty], ref["lo"]) and np.array_equal(r["hi"][:Ty], ref["hi"])
    assert r["steps"] == ref["steps"] == R.check_path(r["lo"][:Ty], r["hi"][:Ty], Tx, Ty)
    assert np.float32(r["total"]).view(np.uint32) == np.float32(ref["total"]).view(np.uint32)
    assert (r["lo"][Ty:] == -1).all() and (r["hi"][Ty:] == -1).all()
    for k in ("cost", "acc"):
        assert (r[k][Tx:] == SENT_F).all() and (r[k][:, Ty:] == SENT_F).all()
    assert r["guards_ok"]


@pytest.mark.parametrize("D", [1, 5, 80])
@pytest.mark.parametrize("Tx, Ty", LISTED)
def test_listed_shapes(Tx, Ty, D):
    x, y = mel_like(Tx, D, 1000 + Tx), mel_like(Ty, D, 2000 + Ty)
    r, = run([(x, y)])
    print(f"({Tx}, {Ty}) D {D}: worst cost error / bound {check_cost(r, x, y):.3g}, steps {r['steps']}, total {r['total']:.6g}")
    check_against_ref(r)


@pytest.mark.parametrize("Tx, Ty", OWN)
def test_shapes_around_the_kernels_own_constants(Tx, Ty):
    x, y = mel_like(Tx, 5, 3000 + Tx), mel_like(Ty, 5, 4000 + Ty)
    if Tx >= 1023:
        x, y = np.round(x * 2) / 2, np.round(y * 2) / 2                # coarse values: ties, far from the first strip too
    r, = run([(x.astype(np.float32), y.astype(np.float32))])
    print(f"({Tx}, {Ty}): worst cost error / bound {check_cost(r, x, y):.3g}, steps {r['steps']}")
    check_against_ref(r)


@pytest.mark.parametrize("D", [15, 16, 17])
def test_feature_counts_around_the_staged_chunk(D):
    x, y = mel_like(37, D, 5000 + D), mel_like(41, D, 6000 + D)
    r, = run([(x, y)])
    check_cost(r, x, y)
    check_against_ref(r)


@pytest.mark.parametrize("Tx, Ty, lo, hi, steps", [(3, 5, [0, 0, 0, 1, 2], [0, 0, 0, 1, 2], 5), (5, 3, [0, 3, 4], [2, 3, 4], 5),
                                                   (4, 4, [0, 1, 2, 3], [0, 1, 2, 3], 4)])
def test_all_equal_rows_give_the_hand_cases(Tx, Ty, lo, hi, steps):
    row = mel_like(1, 80, 7)
    r, = run([(np.repeat(row, Tx, axis=0), np.repeat(row, Ty, axis=0))])
    assert not r["cost"][:Tx, :Ty].any() and r["total"] == 0.0
    assert r["lo"][:Ty].tolist() == lo and r["hi"][:Ty].tolist() == hi and r["steps"] == steps
    check_against_ref(r)


def alternating(n):
    """x = +1, -1, +1, ... against y = -x in one feature: c[i, j] = (x_i + x_j)^2 is symmetric, 4 on the even diagonals and 0 on the
    odd ones, so A is symmetric and every cell (i, i) sees up = left; where the dear diagonal makes both cheaper than A[i-1, i-1]
    the choice is the up / left tie of the rule"""
    x = ((-1.0) ** np.arange(n)).astype(np.float32)[:, None]
    return x, -x


def test_up_left_tie_goes_up():
    """3 x 3: A = [[4, 4, 8], [4, 8, 4], [8, 4, 8]]; at (2, 2) the diagonal is 8 and up = left = 4: up, then diagonal, then left"""
    x, y = alternating(3)
    r, = run([(x, y)])
    assert r["acc"][:3, :3].tolist() == [[4, 4, 8], [4, 8, 4], [8, 4, 8]]
    assert r["lo"][:3].tolist() == [0, 0, 1] and r["hi"][:3].tolist() == [0, 0, 2] and r["steps"] == 4 and r["total"] == 8.0
    check_against_ref(r)
    for n, m in ((67, 67), (130, 67), (67, 130)):              # ... and across strips, where the tie recurs along the path
        x, y = alternating(n)[0], alternating(m)[1]
        r, = run([(x, y)])
        A, d = R.accumulate(r["cost"][:n, :m])
        ties = (A[:-1, 1:] == A[1:, :-1]) & (A[:-1, :-1] > A[:-1, 1:])
        assert ties.any()
        check_against_ref(r)


def distinct_rows(n, D, seed):
    rng = np.random.default_rng(seed)
    x = rng.integers(-8, 9, (n, D)).astype(np.float32)
    x[:, 0] = np.arange(n) * 3.0
    return x


def test_known_warps_are_recovered_with_total_exactly_zero():
    rng = np.random.default_rng(11)
    x = distinct_rows(90, 80, 12)
    reps = rng.integers(1, 4, 90)
    y, ends = R.warp_rows(x, reps), np.cumsum(reps)
    fwd, bwd = run([(x, y), (y, x)])
    assert fwd["total"] == 0.0 and bwd["total"] == 0.0
    owner = np.repeat(np.arange(90), reps)
    assert fwd["lo"][:y.shape[0]].tolist() == fwd["hi"][:y.shape[0]].tolist() == owner.tolist()
    assert bwd["lo"][:90].tolist() == (ends - reps).tolist() and bwd["hi"][:90].tolist() == (ends - 1).tolist()
    assert fwd["steps"] == bwd["steps"] == y.shape[0]
    for r in (fwd, bwd):
        check_against_ref(r)


def test_ragged_batch_is_its_utterances_alone():
    shapes = [(129, 300), (7, 1), (65, 63), (300, 40)]
    pairs = [(mel_like(tx, 80, 20 + b), mel_like(ty, 80, 30 + b)) for b, (tx, ty) in enumerate(shapes)]
    batch = run(pairs)
    for b, (pair, r) in enumerate(zip(pairs, batch)):
        check_cost(r, *pair)
        check_against_ref(r)                                   # -1 beyond Ty_b, cost / acc untouched outside Tx_b x Ty_b, guards
        alone, = run([pair])
        Tx, Ty = r["Tx"], r["Ty"]
        for k in ("cost", "acc"):
            assert np.array_equal(r[k][:Tx, :Ty].view(np.uint32), alone[k][:Tx, :Ty].view(np.uint32))
        assert np.array_equal(r["lo"][:Ty], alone["lo"][:Ty]) and np.array_equal(r["hi"][:Ty], alone["hi"][:Ty])
        assert r["steps"] == alone["steps"] and np.float32(r["total"]).view(np.uint32) == np.float32(alone["total"]).view(np.uint32)
    # and without the optional outputs: the same path from the arena's own cost scratch
    bare = run(pairs, want=())
    for r, q in zip(batch, bare):
        assert np.array_equal(r["lo"], q["lo"]) and np.array_equal(r["hi"], q["hi"]) and r["steps"] == q["steps"]
        assert np.float32(r["total"]).view(np.uint32) == np.float32(q["total"]).view(np.uint32) and q["guards_ok"]


def test_the_call_takes_from_the_arena_what_the_query_says():
    """a fresh handle's high-water mark after one call is exactly mt2_dtw_query's figure, with and without the optional outputs"""
    import ctypes
    from megatts2_amd import runtime as rt

    def high_water(fe):
        n = ctypes.c_size_t(0)
        rt._check(fe.lib.mt2_workspace_high_water(fe.h, ctypes.byref(n)))
        return n.value

    pairs = [(mel_like(70, 5, 90), mel_like(33, 5, 91)), (mel_like(9, 5, 92), mel_like(100, 5, 93)), (mel_like(64, 5, 94), mel_like(64, 5, 95))]
    Tx, Ty, B = 70 + 3, 100 + 5, 3                             # run() pads the buffers by (3, 5)
    for want in ((), ("cost", "acc")):
        fe = rt.MelFrontEnd()
        assert high_water(fe) == 0
        run(pairs, fe=fe, want=want)
        assert high_water(fe) == rt.dtw_query(Tx, Ty, 5, B)
        fe.close()


def test_non_finite_inputs_give_a_path_inside_the_matrix():
    x, y = mel_like(70, 5, 40), mel_like(90, 5, 41)
    x[13, 2], y[50, 0], x[69, 4] = np.nan, np.inf, -np.inf
    r, = run([(x, y)])
    assert r["guards_ok"] and 1 <= r["steps"] <= 70 + 90 - 1
    lo, hi = r["lo"][:90], r["hi"][:90]
    assert (lo >= 0).all() and (hi < 70).all() and (lo <= hi).all() and lo[0] == 0 and hi[-1] == 69


# ---- durations ---------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def tiny_tts():
    from megatts2_amd import megatts2 as M
    (g, p, a, _), (sd_g, sd_p, sd_a, _) = synth_models("tiny")
    return M.Megatts(models=(M.MegaG(g, sd_g), M.MegaPLM(p, sd_p), M.MegaADM(a, sd_a)))


def split(total, n, rng, zeros=True):
    """n durations >= 0 summing to total, with zeros among them"""
    cuts = np.sort(rng.integers(0, total + 1, n - 1))
    s = np.diff(np.concatenate([[0], cuts, [total]])).astype(np.int32)
    if zeros and n > 2 and total > 2:
        s[1] += s[0]
        s[0] = 0
    return s


def test_durations_equal_the_restatement_and_sum_to_ty():
    nat, rng = tiny_tts().native, np.random.default_rng(50)
    shapes = [(129, 300), (300, 129), (64, 64), (1, 9)]
    pairs = [(mel_like(tx, 80, 60 + b), mel_like(ty, 80, 70 + b)) for b, (tx, ty) in enumerate(shapes)]
    xl, yl = np.asarray([s[0] for s in shapes], np.int32), np.asarray([s[1] for s in shapes], np.int32)
    X, Y = np.full((4, 303, 80), np.nan, np.float32), np.full((4, 305, 80), np.nan, np.float32)
    for b, (x, y) in enumerate(pairs):
        X[b, :x.shape[0]], Y[b, :y.shape[0]] = x, y
    path = nat.dtw(dev(X), dev(Y), xl, yl)
    hi = path["hi"].cpu().numpy()
    pl = np.asarray([9, 12, 3, 1], np.int32)
    syn = np.full((4, 12), 99, np.int32)                       # entries at or beyond phone_lens[b] are ignored
    for b in range(4):
        syn[b, :pl[b]] = split(int(xl[b]), int(pl[b]), rng)
    dur = nat.align_durations(path["hi"], yl, syn, pl)
    assert dur.dtype == np.int32 and dur.shape == (4, 12)
    for b in range(4):
        want = R.durations(hi[b, :yl[b]], syn[b, :pl[b]])
        assert np.array_equal(dur[b, :pl[b]], want) and dur[b].sum() == yl[b] and not dur[b, pl[b]:].any()
        assert (dur[b, :pl[b]][syn[b, :pl[b]] == 0] == 0).all()


def test_x_against_x_returns_the_synthetic_durations():
    nat, rng = tiny_tts().native, np.random.default_rng(51)
    x = distinct_rows(200, 80, 52)
    assert (R.cost64(x, x)[~np.eye(200, dtype=bool)] > 0).all()       # every off-diagonal cost, the neighbours' included, is > 0
    path = nat.dtw(dev(x[None]), dev(x[None]))
    assert float(path["total"][0]) == 0.0 and path["hi"][0].cpu().numpy().tolist() == list(range(200))
    s = split(200, 17, rng)
    s[5] += s[6]
    s[6] = 0
    assert (s == 0).sum() >= 2 and s.sum() == 200
    assert np.array_equal(nat.align_durations(path["hi"], None, s[None])[0], s)


def test_refusals_beside_their_accepted_twins():
    from megatts2_amd import runtime as rt
    fe, nat = frontend(), tiny_tts().native
    x, y = dev(mel_like(40, 80, 80)[None].repeat(2, 0)), dev(mel_like(50, 80, 81)[None].repeat(2, 0))
    lo = torch.full((2, 50), int(SENT_I), device="cuda", dtype=torch.int32)
    hi, steps = lo.clone(), torch.full((2,), int(SENT_I), device="cuda", dtype=torch.int32)
    total = torch.full((2,), float(SENT_F), device="cuda")

    def call(xl, yl, Tx=40, Ty=50, D=80, B=2):
        xl, yl = np.asarray(xl, np.int32), np.asarray(yl, np.int32)
        return fe.lib.mt2_dtw_align(fe.h, rt._stream(), rt._ptr(x), rt._iptr(xl), Tx, rt._ptr(y), rt._iptr(yl), Ty, D, B, rt._ptr(lo),
                                    rt._ptr(hi), rt._ptr(steps), rt._ptr(total), None, None)

    for bad in (dict(xl=[40, 41], yl=[50, 50]), dict(xl=[40, 0], yl=[50, 50]), dict(xl=[40, 40], yl=[51, 50]),
                dict(xl=[40, 40], yl=[50, 0]), dict(xl=[40, 40], yl=[50, 50], D=0), dict(xl=[40, 40], yl=[50, 50], B=0),
                dict(xl=[40, 40], yl=[50, 50], Tx=4097), dict(xl=[40, 40], yl=[50, 50], Ty=4097)):
        assert call(**bad) != 0
        torch.cuda.synchronize()
        assert (lo == SENT_I).all() and (hi == SENT_I).all() and (steps == SENT_I).all() and (total == float(SENT_F)).all()
    assert call([40, 39], [50, 1]) == 0                        # the accepted twin
    torch.cuda.synchronize()
    assert int(steps[1]) == 39 and 50 <= int(steps[0]) <= 89
    assert int(hi[0, 49]) == 39 and int(hi[1, 0]) == 38 and (hi[1, 1:] == -1).all()
    # durations: the sum of the synthetic durations must be the x length the path ends on, and hi must cover y_lens
    s = np.asarray([[10, 0, 30], [20, 19, 0]], np.int32)
    good = nat.align_durations(hi, [50, 1], s)
    assert good.sum(axis=1).tolist() == [50, 1]
    for bad_s, bad_yl, bad_pl in ((s + np.asarray([[1, 0, 0], [0, 0, 0]], np.int32), [50, 1], None),      # sums to 41, x length 40
                                  (s, [50, 2], None),                                                       # hi[1, 1] is -1
                                  (s, [50, 51], None), (s, [50, 1], [3, 4]), (s, [50, 1], [0, 3]),
                                  (s - np.asarray([[11, 0, 0], [0, 0, 0]], np.int32), [50, 1], None)):      # a negative duration
        with pytest.raises(rt.NativeError):
            nat.align_durations(hi, bad_yl, bad_s, bad_pl)
    assert np.array_equal(nat.align_durations(hi, [50, 1], s), good)               # the handle is still usable


# ---- the model: tiny synthetic weights -------------------------------------------------------------------------------------------

def prompted():
    z = load_golden("tiny_prompted.npz")
    return z, dev(z["phone"][None]), dev(z["prompt_mel"][None]), dev(z["prompt_phone"][None])


@pytest.mark.parametrize("B", [1, 2])
def test_align_prompt_sums_to_the_prompt_frames_and_is_the_restatement(B):
    tts = tiny_tts()
    z, _, mel, pp = prompted()
    Tp = mel.shape[1]
    # the prompt's 7 phones ten times over: the ADM gives every phone at least one frame, so the synthesis is longer than the
    # prompt's 56 frames and the path has vertical runs - lo and hi differ, and a rule that read lo would show
    mels, pps = mel.repeat(B, 1, 1), pp.repeat(B, 10)
    if B == 2:
        mels[1] = torch.flip(mels[1], dims=[0])                # another prompt of the same length
    dur, aux = tts.align_prompt(pps, mels, return_aux=True)
    assert dur.dtype == np.int32 and dur.shape == (B, pps.shape[1]) and dur.sum(axis=1).tolist() == [Tp] * B and dur.min() >= 0
    hi, lo = aux["hi"].cpu().numpy(), aux["lo"].cpu().numpy()
    assert (aux["syn_lens"] > Tp).all() and (lo != hi).any(axis=1).all()
    for b in range(B):
        assert aux["syn_dur"][b].sum() == aux["syn_lens"][b] == hi[b, Tp - 1] + 1
        assert R.check_path(lo[b], hi[b], int(aux["syn_lens"][b]), Tp) == int(aux["steps"][b])
        assert np.array_equal(dur[b], R.durations(hi[b], aux["syn_dur"][b]))
    assert np.array_equal(tts.align_prompt(pps, mels), dur)                        # greedy: deterministic


def same(a, b):
    return (np.array_equal(np.asarray(a[1]), np.asarray(b[1])) and torch.equal(a[0], b[0]) and torch.equal(a[2]["dur"], b[2]["dur"])
            and torch.equal(a[2]["codes"], b[2]["codes"]))


def test_prompt_durations_none_is_align_prompt():
    import megatts2_oracle as O
    tts = tiny_tts()
    z, phone, mel, pp = prompted()
    dur = tts.align_prompt(pp, mel)
    auto = tts.synthesize_prompt_conditioned(phone, mel, pp, return_aux=True)
    given = tts.synthesize_prompt_conditioned(phone, mel, pp, dur, return_aux=True)
    assert same(auto, given)
    assert same(tts.synthesize_prompt_conditioned_staged(phone, mel, pp, return_aux=True),
                tts.synthesize_prompt_conditioned_staged(phone, mel, pp, dur, return_aux=True))
    # the old explicit durations still take the old path: equal to the staged form, as before
    pd, fd = z["prompt_dur"][None], z["forced_dur"][None]
    fused = tts.synthesize_prompt_conditioned(phone, mel, pp, pd, forced_durations=fd, return_aux=True)
    staged = tts.synthesize_prompt_conditioned_staged(phone, mel, pp, pd, forced_durations=fd, return_aux=True)
    n, nq = int(fused[1][0]), z["p_codes"].size
    assert int(staged[1][0]) == n == z["mel"].shape[0]
    assert np.array_equal(fused[2]["codes"][0, :nq].cpu().numpy(), z["p_codes"]) and torch.equal(staged[2]["codes"][0, :nq], fused[2]["codes"][0, :nq])
    assert torch.equal(staged[2]["dur"], fused[2]["dur"]) and O.rel_l2(fused[0][0, :n].cpu().numpy(), staged[0][0, :n].cpu().numpy()) < 2e-5


def test_interpolated_durations_none_is_align_prompt():
    tts = tiny_tts()
    z, phone, mel, pp = prompted()
    rmel = dev(np.ascontiguousarray(z["prompt_mel"][::-1])[None])
    rp = dev(np.ascontiguousarray(z["prompt_phone"][::-1])[None])
    dur, rdur = tts.align_prompt(pp, mel), tts.align_prompt(rp, rmel)
    auto = tts.synthesize_prosody_interpolated(phone, mel, pp, None, rmel, rp, None, 0.5, return_aux=True)
    given = tts.synthesize_prosody_interpolated(phone, mel, pp, dur, rmel, rp, rdur, 0.5, return_aux=True)
    assert same(auto, given)
    half = tts.synthesize_prosody_interpolated(phone, mel, pp, dur, rmel, rp, None, 0.5, return_aux=True)
    assert same(half, given)
    with pytest.raises(TypeError):
        tts.synthesize_prosody_interpolated(phone, mel, pp)
