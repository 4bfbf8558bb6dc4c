"""The references of tests/rowops_ref.py are the operations the model means: each against torch on the CPU (no GPU needed), and
every float32 emulation through the bar tests/test_gpu_rowops.py applies to the kernel, on the inputs that file uses."""
import ctypes

import numpy as np
import pytest

import rowops_ref as ref
from rowops_ref import F32

torch = pytest.importorskip("torch")
F = torch.nn.functional


def T(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.mark.parametrize("C", [32, 384, 1024])
def test_layernorm_reference_is_f_layer_norm(C):
    rng = np.random.default_rng(C)
    groups, rpg = 3, 7
    M = groups * rpg
    x = (rng.standard_normal((M, C)) * 3 + 1).astype(F32)
    g, b = rng.standard_normal((groups, C)).astype(F32), rng.standard_normal((groups, C)).astype(F32)
    R1, R2 = rng.standard_normal((rpg, C)).astype(F32), rng.standard_normal((M, C)).astype(F32)
    vm = (rng.random(rpg) > 0.3).astype(np.int32)
    want = []
    for q in range(groups):
        xs = T(x[q * rpg:(q + 1) * rpg]).double()
        y = torch.tanh(F.layer_norm(xs, (C,), T(g[q]).double(), T(b[q]).double(), 1e-5)) + T(R1).double() + T(R2[q * rpg:(q + 1) * rpg]).double()
        want.append((y * T(vm).double()[:, None]).numpy())
    want = np.concatenate(want)
    got = ref.layernorm(x, g, b, 1e-5, rpg, R1, rpg, R2, vm, rpg, 3)
    assert np.allclose(got, want, rtol=1e-12, atol=1e-12)
    # the float32 restatement of the same chain stays inside the GPU test's bar on these inputs
    assert ref.rel_l2(ref.layernorm(x, g, b, 1e-5, rpg, R1, rpg, R2, vm, rpg, 3, dtype=np.float32), want) < 2e-6
    relu = F.relu(F.layer_norm(T(x).double(), (C,), T(g[0]).double(), T(b[0]).double(), 1e-5)).numpy()
    assert np.allclose(ref.layernorm(x, g[0], b[0], kind=1), relu, rtol=1e-12, atol=1e-12)


def test_planes_reference_reassembles_the_value():
    rng = np.random.default_rng(1)
    h = (rng.standard_normal((5, 64)) * 10).astype(F32)
    pl = ref.planes(h).view(np.float16).reshape(5, 2, 2, 32).astype(np.float64)
    back = (pl[:, :, 0] + pl[:, :, 1] / 2048.0).reshape(5, 64)
    assert np.abs(back - h).max() <= np.abs(h).max() * 2.0 ** -21


def test_pool_reference_is_ceil_mode_max_pool():
    rng = np.random.default_rng(2)
    C, k = 6, 4
    lens = [1, 5, 8, 3, 4]
    src = (rng.standard_normal((sum(lens), C)) - 2).astype(F32)
    first, cnt = ref.pool_windows(lens, k)
    got = ref.pool_max(src, first, cnt, C)
    want, off = [], 0
    for n in lens:
        want.append(F.max_pool1d(T(src[off:off + n].T.copy())[None], k, k, ceil_mode=True)[0].numpy().T)
        off += n
    assert np.array_equal(got, np.concatenate(want))
    assert (cnt > 0).all() and cnt.min() == 1 and cnt.max() == k
    assert not ref.pool_max(src, [2], [0], C).any()                           # an empty window is a zero row


@pytest.mark.parametrize("scale", [1, 3])
def test_fill_reflect_reference_is_reflect_padding(scale):
    rng = np.random.default_rng(3)
    C, G = 8, 4
    start, len_ = np.asarray([8, 20, 34]), np.asarray([1, 2, 9])
    x = rng.standard_normal(((34 + 9) * scale + 2 * G, C)).astype(F32)
    got = ref.fill_reflect(x, C, start, len_, scale, G)
    touched = np.zeros(x.shape[0], bool)
    for s, n in zip(start, len_):
        off, L = s * scale, n * scale
        g = min(G, L - 1)                                                      # torch requires pad < length
        if g > 0:
            want = F.pad(T(x[off:off + L].T.copy())[None], (g, g), mode="reflect")[0].numpy().T
            assert np.array_equal(got[off - g:off + L + g], want)
        touched[off - g:off] = touched[off + L:off + L + g] = True
    assert np.array_equal(got[~touched], x[~touched]) and touched.sum() == (10 if scale == 1 else 20)


def test_reflect_pad_blocks_reference_frames_like_stft_and_magnitude_is_abs():
    rng = np.random.default_rng(4)
    n_fft, hop = 24, 8
    pad = n_fft // 2
    len_ = np.asarray([37, 20])
    wav = rng.standard_normal((2, 50))
    for b in range(2):
        L = int(len_[b])
        nblk = -(-(L + 2 * pad) // hop) + 2
        rows = ref.reflect_pad_blocks(wav, [b] * nblk, list(range(nblk)), len_, hop, pad)
        flat = rows.reshape(-1)
        assert np.array_equal(flat[:L + 2 * pad], F.pad(T(wav[b, :L])[None, None], (pad, pad), mode="reflect")[0, 0].numpy())
        assert not flat[L + 2 * pad:].any()
        st = torch.stft(T(wav[b, :L]), n_fft, hop, n_fft, torch.ones(n_fft, dtype=torch.float64), center=True, pad_mode="reflect",
                        return_complex=True)
        nfr = st.shape[1]
        assert nfr == 1 + L // hop
        frames = np.stack([flat[t * hop:t * hop + n_fft] for t in range(nfr)])
        spec = np.fft.rfft(frames, axis=1)
        assert np.allclose(spec, st.numpy().T, rtol=1e-10, atol=1e-10)
        packed = np.concatenate([spec.real, spec.imag], axis=1)
        assert np.allclose(ref.magnitude(packed, n_fft // 2 + 1), st.abs().numpy().T, rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize("N", [1, 3, 64, 100, 1024, 1025, 4096])
def test_argmax_reference_is_torch_argmax_nan_rows_included(N):
    x = ref.argmax_cases(N, np.random.default_rng(N))
    want = torch.argmax(T(x), dim=-1).numpy()
    assert np.array_equal(ref.argmax_rows(x), want)
    assert np.array_equal(T(x).max(-1).indices.numpy(), want)
    assert ((want >= 0) & (want < N)).all()
    nan_rows = np.isnan(x).any(1)
    assert nan_rows.sum() >= 6 and all(np.isnan(x[r, want[r]]) and not np.isnan(x[r, :want[r]]).any() for r in np.nonzero(nan_rows)[0])


@pytest.mark.parametrize("N", [3, 64, 100, 1025])
def test_vq_reference_is_the_codebook_quantize_expression(N):
    """dist = -(x.pow(2).sum(1, keepdim) - 2 * xe + ee); ind = dist.max(-1).indices, in float32 - on values whose sums are exact."""
    rng = np.random.default_rng(N)
    M, D = 9, 8
    x = (rng.integers(-8, 9, (M, D)) / 4).astype(F32)
    E = (rng.integers(-8, 9, (N, D)) / 4).astype(F32)
    E[N - 1] = E[0]                                                           # an exact tie in every row
    x[3, 5] = np.nan
    x[4, :] = np.nan
    xe = T(x) @ T(E).T
    xe[5, N // 2] = float("nan")
    ee = T(E).pow(2).sum(1)
    dist = -(T(x).pow(2).sum(1, keepdim=True) - 2 * xe + ee[None])
    want = dist.max(-1).indices.numpy()
    assert np.array_equal(ref.vq_argmin(x, xe.numpy(), ee.numpy()), want)
    assert want[3] == 0 and want[4] == 0 and want[5] == N // 2 and (want != N - 1).all() | (N == 1)


def test_finalize_reference_is_the_duration_expression():
    p = np.asarray(ref.P_EDGE, F32)[None, :]
    n = p.shape[1] - 1
    want = (T(p)[:, 1:] + 0.5).to(torch.int32).clamp(1, 128).numpy()
    dur, flt = ref.finalize_dur(p, [n], None, n, n, 1)
    assert np.array_equal(dur, want) and np.array_equal(flt, p[:, 1:])
    assert {1, 2, 3, 128}.issubset(set(want.reshape(-1).tolist()))
    dur, _ = ref.finalize_dur(p, [4], [0], n, n, 1)                            # beyond the length: zero
    assert np.array_equal(dur[0, :4], want[0, :4]) and not dur[0, 4:].any()
    codes = np.arange(40, dtype=np.int64).reshape(2, 20) + 100
    out = ref.finalize_codes(codes, [7, 2], [1, 0], 6, 6, 2, 2)
    assert out[1].tolist() == codes[0, 3:8].tolist() + [0] and not out[0].any()
    assert np.array_equal(ref.plm_init_hist(1024, codes, 3, [1, 0], 2, 6), np.asarray([[1024, 120, 121, 122, 0, 0], [1024, 100, 101, 102, 0, 0]]))
    assert np.array_equal(ref.adm_init_hist(codes.astype(F32), 0, None, 2, 4), np.zeros((2, 4), F32))


def test_embed_pe_reference_is_embedding_plus_table():
    rng = np.random.default_rng(5)
    vocab, C = 11, 32
    table, pe = rng.standard_normal((vocab, C)), rng.standard_normal((9, C))
    ids = rng.integers(0, vocab, 30)
    idmap, pos = rng.integers(0, 30, 23).astype(np.int32), rng.integers(0, 9, 23).astype(np.int32)
    emb = torch.nn.Embedding(vocab, C).double()
    with torch.no_grad():
        emb.weight.copy_(T(table))
        want = (emb(T(ids[idmap])) + T(pe)[T(pos).long()]).numpy()
    idmap2 = idmap.copy()
    idmap2[4] = -1
    got, ae, aq = ref.embed_pe(table, ids, idmap2, pos, pe)
    assert np.array_equal(np.delete(got, 4, 0), np.delete(want, 4, 0)) and not got[4].any()
    bad = ids.copy()
    bad[idmap[0]], bad[idmap[1]] = -5, vocab + 7                                # clamped, never out of the table
    got2, _, _ = ref.embed_pe(table, bad, idmap, pos, pe)
    assert np.array_equal(got2[0], table[0] + pe[pos[0]]) or idmap[0] == idmap[1]
    assert ref.check_ids(bad, idmap, vocab) and not ref.check_ids(ids, idmap, vocab)


def test_float32_emulations_stay_inside_their_float64_bounds():
    """sum_groups, avg3 and the slab sum: n float32 additions are within n * 2^-24 * sum |terms| (first order) of float64."""
    rng = np.random.default_rng(6)
    x = (rng.standard_normal((5, 13, 24)) * np.exp(rng.uniform(-3, 3, (5, 1, 1)))).astype(F32)
    d = np.abs(ref.sum_groups_f32(x).astype(np.float64) - x.astype(np.float64).sum(0))
    assert (d <= 4 * 2.0 ** -24 * np.abs(x).astype(np.float64).sum(0) * 1.001).all()
    a, b, c = (rng.standard_normal(4000).astype(F32) * F32(s) for s in (1.0, 100.0, 0.01))
    want = (a.astype(np.float64) + b + c) / 3.0
    d = np.abs(ref.avg3_f32(a, b, c, 1.0 / 3.0).astype(np.float64) - want)
    assert (d <= 4 * 2.0 ** -24 * (np.abs(a).astype(np.float64) + np.abs(b) + np.abs(c)) / 3.0 * 1.001).all()
    for S in (1, 2, 8, 9, 16):
        parts = (rng.standard_normal((S, 7, 64)) * np.exp(rng.uniform(-2, 2, (S, 1, 1)))).astype(F32)
        bias, R = rng.standard_normal(64).astype(F32), rng.standard_normal((7, 64)).astype(F32)
        x32 = ref.ln_reduce_x_f32(parts, bias, R)
        mag = np.abs(parts).astype(np.float64).sum(0) + np.abs(bias) + np.abs(R)
        assert (np.abs(x32 - ref.ln_reduce_x(parts, bias, R)) <= (S + 2) * 2.0 ** -24 * mag * 1.001).all()
        g, b2 = (1 + 0.2 * rng.standard_normal(64)).astype(F32), (0.1 * rng.standard_normal(64)).astype(F32)
        assert ref.rel_l2(ref.layernorm(x32, g, b2, dtype=np.float32), ref.layernorm(x32, g, b2)) < 2e-6


@pytest.mark.parametrize("R", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("k", [3, 7, 15])
@pytest.mark.parametrize("ch", [8, 32])
def test_conv_post_float32_chain_passes_the_gpu_bar(ch, k, R):
    xs, w, bias, valid, utts = ref.conv_post_inputs(ch, k, R)
    for three in (True, False):
        x1, x2 = (xs[1], xs[2]) if three else (None, None)
        want = ref.conv_post(xs[0], x1, x2, 1.0 / 3.0, w, bias, 0.1, valid)
        got = ref.conv_post(xs[0], x1, x2, 1.0 / 3.0, w, bias, 0.1, valid, dtype=np.float32)
        assert np.abs(want).max() < 0.9
        for a, e in utts:
            assert ref.rel_l2(got[a:e], want[a:e]) < 3e-6
    if R == 257 and ch == 8:                                                   # the reference itself: torch's conv1d on lrelu(mean)
        v = F.leaky_relu((T(xs[0]).double() + T(xs[1]).double() + T(xs[2]).double()) / 3.0, 0.1)
        y = torch.tanh(F.conv1d(v.T[None], T(w).double().T[None], T(bias).double(), padding=(k - 1) // 2))[0, 0].numpy()
        assert np.allclose(ref.conv_post(xs[0], xs[1], xs[2], 1.0 / 3.0, w, bias, 0.1), y, rtol=1e-9, atol=1e-12)


def test_row_dispatcher_checks_names_and_counts_before_any_launch():
    from megatts2_amd import runtime as rt
    null = ctypes.c_void_p(0)
    with pytest.raises(rt.NativeError, match="unknown op"):
        rt.op_row("gather_cols", None, 4, stream=null)
    with pytest.raises(rt.NativeError, match="wrong argument count"):
        rt.op_row("row_sqnorm", None, 4, None, stream=null)
    with pytest.raises(rt.NativeError, match="wrong argument count"):
        rt.op_row("avg3", None, None, None, 1, None, 4, stream=null)           # the scale as an integer
    # limits the launchers check before they launch: (256 + 14) x 129 + 15 x 128 floats exceed 64 KiB of LDS; even or long kernels
    with pytest.raises(rt.NativeError, match="hipErrorNotSupported"):
        rt.op_row("conv_post", None, None, None, 1.0, 4, 128, 15, None, None, 0.1, None, None, stream=null)
    for k in (4, 17):
        with pytest.raises(rt.NativeError, match="hipErrorInvalidValue"):
            rt.op_row("conv_post", None, None, None, 1.0, 4, 8, k, None, None, 0.1, None, None, stream=null)
    for name in ("embed_pe", "gather_rows", "pool_max", "sum_groups", "avg3", "conv_post", "fill_reflect", "pack_rows", "unpack_rows",
                 "adm_step_input", "plm_step_input", "adm_predict", "adm_finalize", "plm_finalize", "adm_init_hist", "plm_init_hist",
                 "check_ids", "copy_2d", "scatter_i64", "expand_mask", "unpack_wav", "argmax_rows", "vq_argmin", "row_sqnorm",
                 "codebook_rows", "reflect_pad_blocks", "magnitude"):
        assert hasattr(rt, "op_" + name)
        with pytest.raises(rt.NativeError, match="wrong argument count for '" + name + "'"):
            rt.op_row(name, stream=null)
