"""Formant tracks across frames on the GPU (mt2_formant_track, csrc/formant_track.hip) against the numpy restatement of the rule
(tests/formant_track_ref.py): sel, track_freq, track_bw and track_count are held BIT FOR BIT - the rule is in double with every operation
rounded on its own and has no transcendental function, so there is no tolerance to state - on a ragged batch that puts the 64-frame
tile boundary, a one-frame clip and multi-tile clips in one call, for every number of tracks and three jump costs, with NaN wherever
the call must not read; on a 4100-frame utterance of random candidates full of gaps; and hence against the truth of the synthetic
scene, where the restatement itself is held to the truth by tests/test_formant_track_host.py.  Then the figures, the arena and the
Python surfaces."""
import numpy as np
import pytest

import formant_ref as F
import formant_track_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CUTS = (192, 1, 48, 65, 64, 63, 129, 130)      # the tile of 64 from both sides, one frame, one to three tiles
T_MAX = 195
COSTS = (0.0, 1.0, 4.0)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def nan_behind_count(freq, bw, count):
    """the candidates with NaN in every slot at or behind count[t]"""
    freq, bw = freq.copy(), bw.copy()
    behind = np.arange(5)[None, :] >= count[:, None]
    freq[behind] = np.nan
    bw[behind] = np.nan
    return freq, bw


def pack(rows, T_max):
    """rows of (freq, bw, count) -> [B, T_max, ..] host arrays with NaN (count: 5) behind every row's frames, and the frame counts"""
    B = len(rows)
    freq = np.full((B, T_max, 5), np.nan, np.float32)
    bw = np.full((B, T_max, 5), np.nan, np.float32)
    count = np.full((B, T_max), 5, np.int32)
    for b, (f, w, c) in enumerate(rows):
        freq[b, :len(c)], bw[b, :len(c)], count[b, :len(c)] = f, w, c
    return freq, bw, count, np.asarray([len(r[2]) for r in rows], np.int32)


_SCENES = {}


def scene_rows(cuts=CUTS):
    """scene b (seed b, 192 frames) cut to cuts[b] frames, NaN behind count -> rows, truths"""
    key = tuple(cuts)
    if key not in _SCENES:
        rows, truths = [], []
        for seed, n in enumerate(cuts):
            freq, bw, count, truth, _ = R.scene(seed, 192)
            f, w = nan_behind_count(freq[:n], bw[:n], count[:n])
            rows.append((f, w, count[:n].copy()))
            truths.append(truth[:n])
        _SCENES[key] = (rows, truths)
    return _SCENES[key]


_REFS = {}


def reference(rows, key, K, jc, T_max):
    """the restatement of every row alone, laid out as the call lays a batch out; computed once per (batch, K, jump cost)"""
    if (key, K, jc) not in _REFS:
        B = len(rows)
        sel = -np.ones((B, T_max, 5), np.int32)
        tf = np.zeros((B, T_max, 5), np.float32)
        tb = np.zeros((B, T_max, 5), np.float32)
        tc = np.zeros((B, T_max), np.int32)
        for b, (f, w, c) in enumerate(rows):
            s, a, x, n = R.track_fast(f, w, c, K, R.DEFAULT_REF[:K], 1.0, 1.0, jc)
            sel[b, :len(c)], tf[b, :len(c)], tb[b, :len(c)], tc[b, :len(c)] = s, a, x, n
        for a in (sel, tf, tb, tc):
            a.setflags(write=False)
        _REFS[(key, K, jc)] = {"sel": sel, "track_freq": tf, "track_bw": tb, "track_count": tc}
    return _REFS[(key, K, jc)]


@pytest.fixture(scope="module")
def fe():
    from megatts2_amd.runtime import MelFrontEnd
    h = MelFrontEnd()
    yield h
    h.close()


def run(fe, freq, bw, count, lens, K, jc):
    from megatts2_amd.runtime import FormantTrack
    out = fe.formant_track(dev(freq), dev(bw), dev(count), lens, FormantTrack(tracks=K, jump_cost=jc))
    return {k: v.cpu().numpy() for k, v in out.items()}


def same(got, want, what):
    assert sorted(got) == sorted(want)
    for k in ("sel", "track_count", "track_freq", "track_bw"):
        g, w = got[k], want[k]
        assert g.dtype == w.dtype and g.shape == w.shape, (what, k)
        if g.tobytes() != w.tobytes():
            bad = np.argwhere(g.view(np.uint32 if g.dtype == np.float32 else np.int32) != w.view(np.uint32 if w.dtype == np.float32 else np.int32))
            raise AssertionError(f"{what}: {k} differs in {len(bad)} cells, first at {tuple(bad[0])}: {g[tuple(bad[0])]!r} against {w[tuple(bad[0])]!r}")


@pytest.mark.parametrize("jc", COSTS)
@pytest.mark.parametrize("K", [1, 2, 3, 4, 5])
def test_against_the_restatement(fe, K, jc):
    rows, _ = scene_rows()
    freq, bw, count, lens = pack(rows, T_MAX)
    want = reference(rows, "scenes", K, jc, T_MAX)
    got = run(fe, freq, bw, count, lens, K, jc)
    same(got, want, f"K {K} jump cost {jc}")
    tracked = want["track_count"] > 0
    assert tracked.any() and (K == 5 or tracked.sum() > 500)
    # each row of the batch alone: the same bits, whatever the slot and T_max
    for b, n in enumerate(lens):
        one = run(fe, freq[b:b + 1, :n], bw[b:b + 1, :n], count[b:b + 1, :n], lens[b:b + 1], K, jc)
        same(one, {k: v[b:b + 1, :n] for k, v in want.items()}, f"K {K} jump cost {jc} row {b} alone")


def random_utterance(T, seed):
    """random candidates in ascending order, counts 0 .. 5, a few NaN, infinite, zero and negative values: many gaps, many short segments"""
    r = np.random.default_rng(seed)
    freq = np.sort(r.uniform(150.0, 5400.0, (T, 5)), axis=1).astype(np.float32)
    bw = r.uniform(20.0, 500.0, (T, 5)).astype(np.float32)
    count = r.choice(6, T, p=(0.02, 0.02, 0.03, 0.05, 0.38, 0.5)).astype(np.int32)
    for value, target in ((np.nan, freq), (0.0, freq), (-300.0, freq), (np.inf, freq), (np.nan, bw), (-1.0, bw), (0.0, bw)):
        at = r.choice(T, 12, replace=False)
        target[at, r.integers(0, 5, 12)] = value
    return freq, bw, count


@pytest.mark.parametrize("K", [4, 2, 5])
def test_a_long_utterance_of_random_candidates(fe, K):
    """4100 frames: over 64 tiles, the last one of 4 frames"""
    T = 4100
    rows = [random_utterance(T, 77)]
    gap = R.gaps(*rows[0], K)[0]
    assert 50 < gap.sum() < T - 1000 and np.isnan(rows[0][0]).any() and (rows[0][0] <= 0).any()
    freq, bw, count, lens = pack(rows, T + 1)
    want = reference(rows, "random", K, 1.0, T + 1)
    # the candidates are random: the path is not the first K, and it leans on the transition
    first = np.broadcast_to(np.where(np.arange(5) < K, np.arange(5), -1).astype(np.int32), (T, 5))
    if K < 5:
        assert ((want["sel"][0, :T] != first).any(1) & ~gap).sum() > 500
        assert (want["sel"][0] != reference(rows, "random", K, 0.0, T + 1)["sel"][0]).any()
    same(run(fe, freq, bw, count, lens, K, 1.0), want, f"4100 random frames, K {K}")


def test_a_gap_forgets_what_came_before_it(fe):
    """delta is 0 in a gap frame, not the minimum so far: three frames that cost 1e60 in front of a gap must leave no trace in the segment
    behind it - carried along, that figure would swallow every cost of a few units and every state would tie"""
    freq, bw, count, truth, _ = R.scene(0, 192)
    freq, bw = nan_behind_count(freq, bw, count)
    head_f = np.tile(np.float32([1e-30, 2e-30, 3e-30, 4e-30, 5e-30]), (3, 1))
    head_b = np.full((3, 5), 1e30, np.float32)
    gap = np.full((1, 5), np.nan, np.float32)
    rows = [(np.concatenate([head_f, gap, freq]), np.concatenate([head_b, gap, bw]), np.concatenate([np.int32([5, 5, 5, 0]), count]))]
    f, w, c, lens = pack(rows, 196)
    want = reference(rows, "costly head", 4, 1.0, 196)
    alone = R.track_fast(freq, bw, count, 4, R.DEFAULT_REF[:4])
    assert want["sel"][0, 4:].tobytes() == alone[0].tobytes() and (want["track_count"][0, :4] == [4, 4, 4, 0]).all()
    live = count >= 4
    assert (want["sel"][0, 4:][live][:, :4] == truth[live]).all() and (truth[live] != np.arange(4)).any(1).sum() > 40
    same(run(fe, f, w, c, lens, 4, 1.0), want, "a costly segment in front of a gap")


def tied_utterance(T, seed):
    """candidates with exact ties: in about half of the frames one candidate is stored twice, in neighbouring slots, so the states that
    differ in which of the two they take cost the same to the bit - in o, in tr and in every delta built on them"""
    r = np.random.default_rng(seed)
    freq = np.sort(r.integers(1, 22, (T, 5)) * 250.0, axis=1).astype(np.float32)
    bw = (r.integers(1, 4, (T, 5)) * 50.0).astype(np.float32)
    for t in np.flatnonzero(r.random(T) < 0.5):
        a = int(r.integers(0, 4))
        freq[t, a + 1], bw[t, a + 1] = freq[t, a], bw[t, a]
    return freq, bw, r.integers(4, 6, T).astype(np.int32)


@pytest.mark.parametrize("jc", [0.0, 1.0])
@pytest.mark.parametrize("K", [2, 3, 4])
def test_ties_go_to_the_smallest_state(fe, K, jc):
    """the smallest predecessor on a tie, the smallest last state on a tie: with twin candidates the other choice is another sel"""
    rows = [tied_utterance(n, 900 + n) for n in (200, 64, 7)]
    freq, bw, count, lens = pack(rows, 201)
    want = reference(rows, "ties", K, jc, 201)
    # the ties are there and they matter: with every tie going the other way the restatement selects other slots on many frames
    other = sum(int((R.track_fast(f, w, c, K, R.DEFAULT_REF[:K], 1.0, 1.0, jc, last_wins=True)[0] != want["sel"][b, :len(c)]).any(1).sum())
                for b, (f, w, c) in enumerate(rows))
    assert other >= 20, other
    same(run(fe, freq, bw, count, lens, K, jc), want, f"ties, K {K} jump cost {jc}")


def test_the_truth_of_the_scenes(fe):
    """the kernel's tracks are the true formants on every frame with four candidates: whole scenes and cut ones"""
    for cuts in ((192,) * 8, CUTS):
        rows, truths = scene_rows(cuts)
        freq, bw, count, lens = pack(rows, 192)
        got = run(fe, freq, bw, count, lens, 4, 1.0)
        naive = frames = 0
        for b, (row, truth) in enumerate(zip(rows, truths)):
            live = row[2] >= 4
            sel = got["sel"][b, :len(live)]
            assert (sel[live][:, :4] == truth[live]).all(), (cuts[b], b)
            assert (sel[~live] == -1).all() and (got["track_count"][b, :len(live)] == 4 * live).all()
            naive += int((truth[live] != np.arange(4)).any(1).sum())
            frames += int(live.sum())
        print(f"scenes cut to {cuts}: {frames} frames with four candidates, all on the truth; the first four candidates are not on {naive}")
        assert naive > 0.25 * frames


def test_the_figures_of_tracked_formants(fe):
    """formant_stats over track_freq / track_count: the means are the float64 means of the true tracks (as the scene stores them, in f32)
    over the frames with four candidates, to 1e-9 relative - the sums are double on both sides, their orders differ"""
    rows, _ = scene_rows((192,) * 8)
    freq, bw, count, lens = pack(rows, 192)
    got = fe.formant_track(dev(freq), dev(bw), dev(count), lens)
    st = fe.formant_stats(got["track_freq"], got["track_count"], None, lens).cpu().numpy()
    raw = fe.formant_stats(dev(np.nan_to_num(freq)), dev(count), None, lens).cpu().numpy()
    true = R.true_f32(192).astype(np.float64)
    for b, row in enumerate(rows):
        live = row[2] >= 4
        want = true[live, :4].mean(0)
        print(f"scene {b}: {int(live.sum())} frames; true means {np.round(want, 2)}, tracked {np.round(st[b, 2:6], 2)}, raw candidates {np.round(raw[b, 2:6], 2)}")
        assert st[b, 0] == live.sum() == raw[b, 0]
        assert (np.abs(st[b, 2:6] - want) <= 1e-9 * want).all(), b
        assert (np.abs(raw[b, 2:6] - want) > 1e-3 * want).any(), b      # the untracked figures are off by far more


def test_the_arena_is_the_querys():
    from megatts2_amd import runtime as rt
    h = rt.MelFrontEnd()
    try:
        assert h.workspace_high_water() == 0
        rows, _ = scene_rows()
        r = lambda n: (n + 255) // 256 * 256
        # the high water is the most since the handle was made: the three geometries grow
        for K, sub, T_max in ((4, slice(1, 2), 1), (2, slice(0, 8), T_MAX), (5, slice(0, 3), 700)):
            freq, bw, count, lens = pack(rows[sub], T_max)
            run(h, freq, bw, count, lens, K, 1.0)
            B = len(lens)
            assert h.workspace_high_water() == rt.formant_track_query(K, T_max, B)[1] == r(4 * 65535) + r(16 * B * T_max), (K, B, T_max)
    finally:
        h.close()


# ---- the Python surfaces -----------------------------------------------------------------------------------------------------------------
def test_extract_formants_with_a_track():
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime as rt
    x = dev(F.voiced_signal(11000))
    plain = M.extract_formants(x, 11000)
    out = M.extract_formants(x, 11000, track=rt.FormantTrack())
    assert sorted(out) == sorted(list(plain) + ["track_freq", "track_bw", "track_count", "sel"])
    for k, v in plain.items():
        assert torch.equal(out[k], v) if hasattr(v, "is_cuda") else np.array_equal(out[k], v), k
    own = M.track_formants(out["freq"], out["bw"], out["count"], out["frame_lens"], rt.FormantTrack())
    assert sorted(own) == ["sel", "track_bw", "track_count", "track_freq"]
    for k, v in own.items():
        assert v.shape == out[k].shape and torch.equal(v, out[k]), k
    T = out["count"].shape[0]
    assert out["track_freq"].shape == (T, 5) and out["sel"].shape == (T, 5) and out["track_count"].shape == (T,)
    want = R.track_fast(out["freq"].cpu().numpy(), out["bw"].cpu().numpy(), out["count"].cpu().numpy())
    for k, w in zip(("sel", "track_freq", "track_bw", "track_count"), want):
        assert out[k].cpu().numpy().tobytes() == w.tobytes(), k
    assert int(out["track_count"].max()) == 4
    # a batch, another ceiling (ref_hz None follows it), host arrays in: the handle call on the same candidates
    two = M.extract_formants(torch.stack([x, x.flip(0)]), 11000, [11000, 7000], rt.Formants(max_formant_hz=5000.0), rt.FormantTrack(tracks=3))
    ref = M._frontend().formant_track(two["freq"], two["bw"], two["count"], two["frame_lens"], rt.FormantTrack(tracks=3), 5000.0)
    host = M.track_formants(two["freq"].cpu().numpy(), two["bw"].cpu().numpy(), two["count"].cpu().numpy(), two["frame_lens"],
                            rt.FormantTrack(tracks=3), 5000.0)
    for k in ref:
        assert torch.equal(two[k], ref[k]) and torch.equal(host[k], ref[k]), k
    assert int(two["track_count"].max()) == 3 and (two["track_count"][1, two["frame_lens"][1]:] == 0).all()


def test_output_formants_with_and_without_a_track():
    from megatts2_amd import megatts2 as M
    from megatts2_amd import runtime as rt
    from test_gpu_prosody import synth_inputs, tiny_tts
    tts = tiny_tts(None)
    phone, prompt, pl, ml = synth_inputs()
    mel, mel_lens, aux = tts.synthesize(phone, prompt, pl, ml, griffin_lim={"n_iter": 2}, return_aux=True)
    before = tts.output_formants(mel_lens, aux)
    again = tts.output_formants(mel_lens, aux, track=None)
    assert sorted(before) == sorted(again) and not {"track_freq", "sel"} & set(before)
    for k, v in before.items():
        assert torch.equal(again[k], v) if hasattr(v, "is_cuda") else np.array_equal(again[k], v, equal_nan=True), k
    out = tts.output_formants(mel_lens, aux, track=rt.FormantTrack())
    assert sorted(out) == sorted(list(before) + ["track_freq", "track_bw", "track_count", "sel"])
    for k in ("freq", "bw", "count", "f0"):
        assert torch.equal(out[k], before[k]), k
    # every tracked frame carries four candidates of its own frame, in ascending slots; the figures are formant_stats of the tracks
    fl = out["frame_lens"]
    on = out["track_count"] > 0
    assert on.any() and (out["track_count"][on] == 4).all() and (out["sel"][on][:, 4] == -1).all() and (out["sel"][~on] == -1).all()
    sel = out["sel"][on][:, :4].long()
    assert (sel[:, 1:] > sel[:, :-1]).all() and (sel[:, 3] < out["count"][on]).all()
    assert torch.equal(out["track_freq"][on][:, :4], torch.gather(out["freq"][on], 1, sel))
    st = M.formant_stats(out["track_freq"][:, :out["f0"].shape[1]], out["track_count"][:, :out["f0"].shape[1]], out["f0"], fl)
    assert all(np.array_equal(st[k], out[k]) for k in M.FORMANT_STAT_NAMES)
    # the model's handle gives the bits of the front end's
    args = (out["freq"], out["bw"], out["count"], fl, rt.FormantTrack(tracks=3, jump_cost=2.0), 5000.0)
    a, b = tts.native.formant_track(*args), M._frontend().formant_track(*args)
    assert sorted(a) == sorted(b) and all(torch.equal(a[k], b[k]) for k in a)
