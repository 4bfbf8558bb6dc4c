"""Kernel-level parity (GPU) of the row kernels of megatts2_amd/csrc/rowops.hip, one launch at a time through the test entries of
the C ABI (mt2_op_row, mt2_op_layernorm_ex, mt2_op_ln_reduce), against the numpy restatements of tests/rowops_ref.py.

Output buffers start filled with a sentinel and have leading dimensions larger than their width: "left untouched", "zeroed" and a
stride mix-up are all observable.  No case hands a kernel an index outside its buffers: out-of-range ids go to the clamping gathers
only, and every buffer a shared-row option indexes (R1, valid) is allocated at full height."""
import numpy as np
import pytest

import rowops_ref as ref
from rowops_ref import F32, ISENT, SENTINEL

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CAP = 2048 * 8 * 256          # work items one launch of a grid-stride row kernel covers without its stride loop


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def host(t):
    return t.cpu().numpy()


def sent(*shape, dtype=np.float32):
    return dev(np.full(shape, SENTINEL if np.dtype(dtype).kind == "f" else ISENT, dtype))


def padded(a, ld, fill=None):
    """[R, C] -> device [R, ld] with junk (or `fill`) in the pad columns."""
    a = np.asarray(a)
    out = np.full((a.shape[0], ld), 12345.0 if fill is None else fill, a.dtype)
    out[:, :a.shape[1]] = a
    return dev(out)


def i32(a):
    return dev(np.asarray(a, np.int32))


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    runtime.device_check()
    return runtime


def untouched(a):
    return bool((a == (SENTINEL if a.dtype.kind == "f" else ISENT)).all())


# ---- data movement: bit-equal -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("C,lds,ldo", [(64, 72, 68), (8, 8, 12), (6, 7, 9), (8, 9, 12), (8, 8, 10), (8, 12, 8)])
def test_gather_rows_both_forms(rt, C, lds, ldo):
    """(6, 7, 9), (8, 9, 12), (8, 8, 10): C, lds_ or ldo is not a multiple of 4 - the scalar kernel; the others the float4 one."""
    rng = np.random.default_rng(C * 100 + lds)
    S, R = 19, 37
    src = rng.standard_normal((S, lds)).astype(F32)
    map_ = rng.integers(0, S, R).astype(np.int32)
    map_[[0, 5, 36]] = -1
    map_[[1, 2]] = [S - 1, 0]
    out = sent(R, ldo)
    rt.op_gather_rows(dev(src), lds, i32(map_), out, ldo, C, R)
    got = host(out)
    assert np.array_equal(got[:, :C], ref.gather_rows(src, map_, C))
    assert untouched(got[:, C:])
    out = sent(4, ldo)
    rt.op_gather_rows(dev(src), lds, i32(map_), out, ldo, C, 0)          # empty launch
    assert untouched(host(out))


@pytest.mark.parametrize("R", [CAP // 64 - 1, CAP // 64 + 64])
def test_gather_rows_grid_stride_tail(rt, R):
    """C = 256: 64 float4 items per row; one launch just below 16 384 x 256 items and one above (the stride loop's second trip)."""
    rng = np.random.default_rng(R)
    C, S = 256, 1000
    src = rng.standard_normal((S, C), dtype=F32)
    map_ = rng.integers(-1, S, R).astype(np.int32)
    out = torch.full((R, C), float(SENTINEL), device="cuda")
    rt.op_gather_rows(dev(src), C, i32(map_), out, C, C, R)
    assert np.array_equal(host(out), ref.gather_rows(src, map_, C))


@pytest.mark.parametrize("mode", ["general", "zero_pe", "zero_table"])
def test_embed_pe(rt, mode):
    rng = np.random.default_rng(5)
    C, ldo, vocab, npos, R = 32, 40, 11, 9, 23
    table = (rng.standard_normal((vocab, C)) * 3).astype(F32)
    pe = rng.standard_normal((npos, C)).astype(F32)
    if mode == "zero_pe":
        pe[:] = 0
    if mode == "zero_table":
        table[:] = 0
    ids = rng.integers(0, vocab, 30).astype(np.int64)
    ids[[3, 4, 7]] = [-3, vocab, 99]                                     # clamped to rows 0, vocab - 1, vocab - 1
    idmap = rng.integers(0, 30, R).astype(np.int32)
    idmap[:4] = [3, 4, 7, -1]
    idmap[10] = -1
    pos = rng.integers(0, npos, R).astype(np.int32)
    out = sent(R, ldo)
    rt.op_embed_pe(dev(table), C, dev(ids), i32(idmap), i32(pos), dev(pe), out, ldo, R, vocab)
    got = host(out)
    want, ae, aq = ref.embed_pe(table, ids, idmap, pos, pe)
    assert untouched(got[:, C:])
    assert not got[idmap < 0, :C].any()
    if mode == "general":
        err = np.abs(got[:, :C].astype(np.float64) - want)
        print("embed_pe max err / bound", float((err / np.maximum(2.0 ** -23 * (ae + aq), 1e-300)).max()))
        assert (err <= 2.0 ** -23 * (ae + aq)).all()
    else:
        assert np.array_equal(got[:, :C], want.astype(F32))
    out = sent(2, ldo)
    rt.op_embed_pe(dev(table), C, dev(ids), i32(idmap), i32(pos), dev(pe), out, ldo, 0, vocab)
    assert untouched(host(out))


def test_codebook_rows_clamps_and_zeroes(rt):
    rng = np.random.default_rng(6)
    Dq, ldo, bins, R = 16, 20, 13, 29
    E = rng.standard_normal((bins, Dq)).astype(F32)
    codes = rng.integers(0, bins, 12).astype(np.int64)
    codes[[0, 1]] = [-1, bins + 5]
    cmap = rng.integers(0, 12, R).astype(np.int32)
    cmap[:3] = [0, 1, -1]
    out = sent(R, ldo)
    rt.op_codebook_rows(dev(E), dev(codes), i32(cmap), out, ldo, Dq, R, bins)
    got = host(out)
    assert np.array_equal(got[:, :Dq], ref.codebook_rows(E, codes, cmap)) and untouched(got[:, Dq:])
    out = sent(2, ldo)
    rt.op_codebook_rows(dev(E), dev(codes), i32(cmap), out, ldo, Dq, 0, bins)
    assert untouched(host(out))


@pytest.mark.parametrize("use_map", [False, True])
@pytest.mark.parametrize("bad", [None, "low", "high", "unmapped"])
def test_check_ids_sets_exactly_its_bit(rt, use_map, bad):
    rng = np.random.default_rng(7)
    hi, n = 17, 700
    ids = rng.integers(0, hi, n).astype(np.int64)
    ids[0], ids[n - 1] = 0, hi - 1
    map_ = rng.permutation(n).astype(np.int32)
    map_[::7] = -1
    free = int(np.setdiff1d(np.arange(n), map_[map_ >= 0])[0])            # a position no map entry reads
    if bad == "low":
        ids[int(map_[1])] = -1
    elif bad == "high":
        ids[int(map_[n - 2])] = hi
    elif bad == "unmapped":
        ids[free] = hi + 3
    m = map_ if use_map else None
    flag = i32([4])
    rt.op_check_ids(dev(ids), None if m is None else i32(m), n, hi, flag, 2)
    want = ref.check_ids(ids, m, hi)
    assert want == (bad in ("low", "high") or (bad == "unmapped" and not use_map))
    assert int(host(flag)[0]) == (6 if want else 4)
    flag = i32([4])
    rt.op_check_ids(dev(ids), None, 0, 1, flag, 2)                        # empty: nothing is read
    assert int(host(flag)[0]) == 4


def test_pool_max_windows(rt):
    rng = np.random.default_rng(8)
    C, lds, ldo, k = 16, 20, 24, 4
    lens = [1, 5, 8, 3, 4]
    first, cnt = ref.pool_windows(lens, k)
    first = np.concatenate([first[:3], [2], first[3:]]).astype(np.int32)      # a cnt = 0 row in the middle: zeros
    cnt = np.concatenate([cnt[:3], [0], cnt[3:]]).astype(np.int32)
    src = (rng.standard_normal((sum(lens), lds)) - 2).astype(F32)              # mostly negative: a zero is not the maximum
    R = first.size
    out = sent(R, ldo)
    rt.op_pool_max(dev(src), lds, i32(first), i32(cnt), out, ldo, C, R)
    got = host(out)
    assert np.array_equal(got[:, :C], ref.pool_max(src, first, cnt, C)) and untouched(got[:, C:])
    assert not got[3, :C].any()
    out = sent(2, ldo)
    rt.op_pool_max(dev(src), lds, i32(first), i32(cnt), out, ldo, C, 0)
    assert untouched(host(out))


@pytest.mark.parametrize("scale", [1, 3])
def test_fill_reflect_short_utterances(rt, scale):
    """Utterances of 1, 2 and 9 rows (x scale): j >= L is skipped, so the gap rows there keep what they held."""
    rng = np.random.default_rng(9 + scale)
    C, ld, G = 8, 12, 4
    start, len_ = np.asarray([8, 20, 34], np.int32), np.asarray([1, 2, 9], np.int32)
    rows = (34 + 9) * scale + 2 * G
    x = rng.standard_normal((rows, ld)).astype(F32)
    buf = dev(x)
    rt.op_fill_reflect(buf, ld, C, i32(start), i32(len_), 3, scale, G)
    assert np.array_equal(host(buf), ref.fill_reflect(x, C, start, len_, scale, G))
    buf = dev(x)
    rt.op_fill_reflect(buf, ld, C, i32(start), i32(len_), 0, scale, G)        # B = 0
    rt.op_fill_reflect(buf, ld, C, i32(start), i32(len_), 3, scale, 0)        # G = 0
    assert np.array_equal(host(buf), x)


def test_reflect_pad_blocks(rt):
    rng = np.random.default_rng(10)
    hop, pad, wstride = 8, 12, 50
    len_ = np.asarray([37, 20], np.int32)
    wav = rng.standard_normal((2, wstride)).astype(F32)
    bb, bt = [], []
    for b in (1, 0):                                                          # utterance order differs from row order
        for t in range(-(-(int(len_[b]) + 2 * pad) // hop) + 2):              # two blocks beyond the padded signal: zeros
            bb.append(b)
            bt.append(t)
    R = len(bb)
    out = sent(R + 1, hop)
    rt.op_reflect_pad_blocks(dev(wav), wstride, i32(bb), i32(bt), i32(len_), hop, pad, out, R)
    got = host(out)
    assert np.array_equal(got[:R], ref.reflect_pad_blocks(wav, bb, bt, len_, hop, pad)) and untouched(got[R:])
    out = sent(2, hop)
    rt.op_reflect_pad_blocks(dev(wav), wstride, i32(bb), i32(bt), i32(len_), hop, pad, out, 0)
    assert untouched(host(out))


@pytest.mark.parametrize("cmajor", [0, 1])
def test_pack_and_unpack_rows(rt, cmajor):
    rng = np.random.default_rng(11 + cmajor)
    B, Tmax, C, ldd = 2, 7, 5, 8
    lens = [7, 4]
    rowmap = [-1, -1] + [t for t in range(lens[0])] + [-1, -1, -1] + [Tmax + t for t in range(lens[1])] + [-1]
    rowmap = np.asarray(rowmap, np.int32)
    R = rowmap.size
    src = rng.standard_normal((B, C, Tmax) if cmajor else (B, Tmax, C)).astype(F32)
    rows = sent(R, ldd)
    rt.op_pack_rows(dev(src), C, Tmax, cmajor, i32(rowmap), rows, ldd, R)
    got = host(rows)
    assert np.array_equal(got[:, :C], ref.pack_rows(src, cmajor, rowmap)) and untouched(got[:, C:])
    packed = rng.standard_normal((R, ldd)).astype(F32)
    dst = sent(*src.shape)
    rt.op_unpack_rows(dev(packed), ldd, C, Tmax, cmajor, i32(rowmap), dst, R)
    want = ref.unpack_rows(packed, C, cmajor, rowmap, np.full(src.shape, SENTINEL, F32))
    assert np.array_equal(host(dst), want)
    view = np.transpose(want, (0, 2, 1)) if cmajor else want
    assert untouched(view[1, lens[1]:])                                        # the padded positions of the short utterance
    rows, dst = sent(R, ldd), sent(*src.shape)
    rt.op_pack_rows(dev(src), C, Tmax, cmajor, i32(rowmap), rows, ldd, 0)
    rt.op_unpack_rows(dev(packed), ldd, C, Tmax, cmajor, i32(rowmap), dst, 0)
    assert untouched(host(rows)) and untouched(host(dst))


def test_copy_2d_scatter_expand_mask_unpack_wav(rt):
    rng = np.random.default_rng(12)
    src = rng.standard_normal((9, 24)).astype(F32)
    dst = sent(9, 20)
    rt.op_copy_2d(dev(src), 24, dst, 20, 16, 9)
    got = host(dst)
    assert np.array_equal(got[:, :16], src[:, :16]) and untouched(got[:, 16:])
    dst = sent(9, 20)
    rt.op_copy_2d(dev(src), 24, dst, 20, 16, 0)
    assert untouched(host(dst))
    with pytest.raises(rt.NativeError, match="hipErrorInvalidValue"):
        rt.op_copy_2d(dev(src), 24, dst, 20, 6, 9)

    R = 300                                                                    # two workgroups
    s64 = rng.integers(0, 1 << 40, R).astype(np.int64)
    map_ = rng.permutation(400)[:R].astype(np.int32)
    map_[::5] = -1
    out = sent(400, dtype=np.int64)
    rt.op_scatter_i64(dev(s64), i32(map_), out, R)
    assert np.array_equal(host(out), ref.scatter_i64(s64, map_, np.full(400, ISENT, np.int64)))
    out = sent(4, dtype=np.int64)
    rt.op_scatter_i64(dev(s64), i32(map_), out, 0)
    assert untouched(host(out))

    mask = rng.integers(0, 2, 41).astype(np.int32)
    for factor in (1, 3, 8):
        n = 41 * factor
        out = sent(n + 3, dtype=np.int32)
        rt.op_expand_mask(i32(mask), factor, out, n)
        got = host(out)
        assert np.array_equal(got[:n], mask[np.arange(n) // factor]) and untouched(got[n:])
    out = sent(4, dtype=np.int32)
    rt.op_expand_mask(i32(mask), 3, out, 0)
    assert untouched(host(out))

    wav = rng.standard_normal(3000).astype(F32)
    start, len_ = np.asarray([100, 0, 1500], np.int64), np.asarray([700, 0, 1500], np.int64)
    out = sent(3, 1600)
    rt.op_unpack_wav(dev(wav), dev(start), dev(len_), out, 1600, 1500, 3)
    assert np.array_equal(host(out), ref.unpack_wav(wav, start, len_, np.full((3, 1600), SENTINEL, F32)))
    out = sent(3, 1600)
    rt.op_unpack_wav(dev(wav), dev(start), dev(len_), out, 1600, 1500, 0)
    assert untouched(host(out))


@pytest.mark.parametrize("perm,with_flt", [(False, True), (True, True), (True, False)])
def test_adm_finalize_rounding_clamps_and_slots(rt, perm, with_flt):
    rng = np.random.default_rng(13)
    A, nmax, pstride, dstride = 4, 7, 10, 9
    p = rng.choice(np.asarray(ref.P_EDGE, F32), (A, pstride)).astype(F32)
    p[0, 1:8] = np.asarray(ref.P_EDGE[1:8], F32)
    p[1, 1:8] = np.asarray(ref.P_EDGE[8:15], F32)
    p[2, 1:7] = np.asarray(ref.P_EDGE[14:20], F32)
    lens = np.asarray([7, 7, 6, 0], np.int32)
    slot = np.asarray([2, 0, 3, 1], np.int32) if perm else None
    dur, flt = sent(A, dstride, dtype=np.int32), sent(A, dstride)
    rt.op_adm_finalize(dev(p), pstride, i32(lens), None if slot is None else i32(slot), dur, flt if with_flt else None, dstride, A, nmax)
    wd, wf = ref.finalize_dur(p, lens, slot, dstride, nmax, A)
    assert np.array_equal(host(dur), wd)
    assert np.array_equal(host(flt), wf) if with_flt else untouched(host(flt))
    assert wd[:, :nmax].max() == 128 and (wd[:, :nmax] == 1).any() and not wd[(1 if perm else 3), :nmax].any()
    dur = sent(A, dstride, dtype=np.int32)
    rt.op_adm_finalize(dev(p), pstride, i32(lens), None, dur, None, dstride, 0, nmax)
    assert untouched(host(dur))


@pytest.mark.parametrize("skip", [0, 2])
@pytest.mark.parametrize("perm", [False, True])
def test_plm_finalize_skip_and_slots(rt, skip, perm):
    rng = np.random.default_rng(14)
    A, nmax, cstride, ostride = 4, 6, 12, 8
    codes = rng.integers(1, 1024, (A, cstride)).astype(np.int64)
    lens = np.asarray([6 + skip, 3 + skip, 1, 0], np.int32)                    # 1 and 0: shorter than skip = 2 -> all zero
    slot = np.asarray([3, 1, 0, 2], np.int32) if perm else None
    out = sent(A, ostride, dtype=np.int64)
    rt.op_plm_finalize(dev(codes), cstride, i32(lens), None if slot is None else i32(slot), out, ostride, A, nmax, skip)
    assert np.array_equal(host(out), ref.finalize_codes(codes, lens, slot, ostride, nmax, skip, A))
    out = sent(A, ostride, dtype=np.int64)
    rt.op_plm_finalize(dev(codes), cstride, i32(lens), None, out, ostride, 0, nmax, skip)
    assert untouched(host(out))


@pytest.mark.parametrize("P", [0, 1, 5, 8])
@pytest.mark.parametrize("perm", [False, True])
def test_init_hist_prefix_lengths(rt, P, perm):
    """pstride = cstride = 9: P = 8 fills the history, P = 0 leaves only the first slot (0 / bos)."""
    rng = np.random.default_rng(15 + P)
    A, stride, ppitch = 3, 9, 11
    slot = np.asarray([2, 0, 1], np.int32) if perm else None
    sl = None if slot is None else i32(slot)
    prefix = (rng.standard_normal((A, max(P, 1))) + 5).astype(F32)
    p = sent(A + 1, stride)
    rt.op_adm_init_hist(p, stride, dev(prefix) if P else None, P, sl, A)
    got = host(p)
    assert np.array_equal(got[:A], ref.adm_init_hist(prefix, P, slot, A, stride)) and untouched(got[A:])
    cpre = rng.integers(1, 1024, (A, ppitch)).astype(np.int64)
    c = sent(A + 1, stride, dtype=np.int64)
    rt.op_plm_init_hist(c, stride, 1024, dev(cpre) if P else None, P, ppitch, sl, A)
    got = host(c)
    assert np.array_equal(got[:A], ref.plm_init_hist(1024, cpre, P, slot, A, stride)) and untouched(got[A:])
    p, c = sent(2, stride), sent(2, stride, dtype=np.int64)
    rt.op_adm_init_hist(p, stride, dev(prefix), P, sl, 0)
    rt.op_plm_init_hist(c, stride, 1024, dev(cpre), P, ppitch, sl, 0)
    assert untouched(host(p)) and untouched(host(c))


# ---- documented-order float32 arithmetic: bit-equal to the emulation --------------------------------------------------------------------

@pytest.mark.parametrize("groups", [1, 3, 5])
def test_sum_groups_left_to_right(rt, groups):
    rng = np.random.default_rng(20 + groups)
    R, C, ld, ldo = 13, 24, 28, 32
    strideG = R * ld + 8
    x = (rng.standard_normal((groups, strideG)) * np.exp(rng.uniform(-3, 3, (groups, 1)))).astype(F32)
    xv = np.stack([x[g, :R * ld].reshape(R, ld)[:, :C] for g in range(groups)])
    out = sent(R, ldo)
    rt.op_sum_groups(dev(x), strideG, groups, ld, out, ldo, C, R)
    got = host(out)
    assert np.array_equal(got[:, :C], ref.sum_groups_f32(xv)) and untouched(got[:, C:])
    out = sent(R, ldo)
    rt.op_sum_groups(dev(x), strideG, groups, ld, out, ldo, C, 0)
    assert untouched(host(out))


@pytest.mark.parametrize("n4", [1, 333, CAP - 1, CAP + 1000])
def test_avg3_order_and_grid_stride_tail(rt, n4):
    rng = np.random.default_rng(n4)
    n = 4 * n4
    a, b, d = (rng.standard_normal(n, dtype=F32) * F32(s) for s in (1.0, 100.0, 0.01))
    out = torch.full((n + 4,), float(SENTINEL), device="cuda")
    rt.op_avg3(dev(a), dev(b), dev(d), 1.0 / 3.0, out, n)
    got = host(out)
    assert np.array_equal(got[:n], ref.avg3_f32(a, b, d, 1.0 / 3.0)) and untouched(got[n:])
    if n4 == 1:
        rt.op_avg3(dev(a), dev(b), dev(d), 1.0 / 3.0, out, 0)
        with pytest.raises(rt.NativeError, match="hipErrorInvalidValue"):
            rt.op_avg3(dev(a), dev(b), dev(d), 1.0 / 3.0, out, 3)
        assert np.array_equal(host(out), got)


def run_ln_reduce(rt, parts, pstride, S, bias, R, g, b, M, C, ldr, ldx, ldh, xmode="out", h_planes=0, want_flag=0):
    """-> (xout [M, C] or None, hout [M, ldh] raw, pad columns of xout untouched).  xmode: out / alias (xout = R) / none."""
    Rd = None if R is None else padded(R, ldr)
    xout = None if xmode == "none" else (Rd if xmode == "alias" else sent(M, ldx))
    hout = sent(M, ldh)
    flag = i32([0])
    rt.op_ln_reduce(dev(parts), pstride, S, None if bias is None else dev(bias), Rd, ldr, dev(g), dev(b), xout,
                    ldr if xmode == "alias" else ldx, hout, ldh, M, C, 1e-5, h_planes, flag)
    assert int(host(flag)[0]) == want_flag
    return (None if xout is None else host(xout)), host(hout)


def ln_reduce_inputs(rng, S, M, C, pstride):
    parts = np.zeros((S, pstride), F32)
    parts[:, :M * C] = (rng.standard_normal((S, M * C)) * np.exp(rng.uniform(-2, 2, (S, 1)))).astype(F32)
    bias, R = rng.standard_normal(C).astype(F32), (rng.standard_normal((M, C)) * 2 + 0.5).astype(F32)
    g, b = (1 + 0.2 * rng.standard_normal(C)).astype(F32), (0.1 * rng.standard_normal(C)).astype(F32)
    return parts, bias, R, g, b


@pytest.mark.parametrize("S", [1, 2, 8, 9, 16])
@pytest.mark.parametrize("C,with_bias,with_R,xmode", [(768, True, True, "out"), (1024, True, True, "alias"), (512, False, False, "out"),
                                                       (32, True, False, "out"), (64, False, True, "none")])
def test_ln_reduce_slab_sum_and_layernorm(rt, S, C, with_bias, with_R, xmode):
    rng = np.random.default_rng(S * 2000 + C)
    M = 7
    pstride, ldr, ldx, ldh = M * C + 64, C + 8, C + 4, C + 12
    parts, bias, R, g, b = ln_reduce_inputs(rng, S, M, C, pstride)
    bias, R = (bias if with_bias else None), (R if with_R else None)
    xo, ho = run_ln_reduce(rt, parts, pstride, S, bias, R, g, b, M, C, ldr, ldx, ldh, xmode)
    want_x = ref.ln_reduce_x_f32(parts[:, :M * C].reshape(S, M, C), bias, R)
    if xo is not None:
        assert np.array_equal(xo[:, :C], want_x)
        assert (xo[:, C:] == 12345.0).all() if xmode == "alias" else untouched(xo[:, C:])
    err = ref.rel_l2(ho[:, :C], ref.layernorm(want_x, g, b))
    print("ln_reduce hout rel L2", err)
    assert err < 2e-6 and untouched(ho[:, C:])


def test_ln_reduce_both_kernels_of_the_launcher(rt):
    """M = 4096 is the last launch on the row-per-workgroup kernel, M = 4097 the first on the wave-per-row one."""
    rng = np.random.default_rng(4097)
    S, C, M = 3, 768, 4097
    pstride, ldr, ldx, ldh = M * C, C + 4, C + 4, C + 8
    parts, bias, R, g, b = ln_reduce_inputs(rng, S, M, C, pstride)
    want_x = ref.ln_reduce_x_f32(parts.reshape(S, M, C), bias, R)
    want_h = ref.layernorm(want_x, g, b)
    res = {}
    for m in (1, 4096, 4097):
        xo, ho = run_ln_reduce(rt, parts, pstride, S, bias, R[:m], g, b, m, C, ldr, ldx, ldh)
        assert np.array_equal(xo[:, :C], want_x[:m]) and untouched(xo[:, C:]) and untouched(ho[:, C:])
        err = ref.rel_l2(ho[:, :C], want_h[:m])
        print("ln_reduce M", m, "hout rel L2", err)
        assert err < 2e-6
        res[m] = (xo, ho)
    assert np.array_equal(res[4096][0], res[4097][0][:4096])
    assert ref.rel_l2(res[4097][1][:4096, :C], res[4096][1][:, :C]) < 2e-6
    # per row as well: one wrong row out of 4097 moves the whole-matrix norm by less than the bar
    d = np.linalg.norm(res[4097][1][:, :C] - want_h, axis=1) / np.linalg.norm(want_h, axis=1)
    assert d.max() < 2e-6


def test_ln_reduce_planes(rt):
    rng = np.random.default_rng(31)
    S, C, M = 4, 768, 9
    pstride, ldr, ldx, ldh = M * C, C, C, C + 32
    parts, bias, R, g, b = ln_reduce_inputs(rng, S, M, C, pstride)
    _, ho = run_ln_reduce(rt, parts, pstride, S, bias, R, g, b, M, C, ldr, ldx, ldh)
    _, hp = run_ln_reduce(rt, parts, pstride, S, bias, R, g, b, M, C, ldr, ldx, ldh, h_planes=1)
    assert np.array_equal(hp[:, :C].copy().view(np.uint16), ref.planes(ho[:, :C])) and untouched(hp[:, C:])
    gbig = g.copy()
    gbig[5] = 1e7                                                              # |h| >= 65504 in column 5: the range guard's word is set
    run_ln_reduce(rt, parts, pstride, S, bias, R, gbig, b, M, C, ldr, ldx, ldh, h_planes=1, want_flag=1)
    run_ln_reduce(rt, parts, pstride, S, bias, R, gbig, b, M, C, ldr, ldx, ldh, h_planes=0, want_flag=0)
    Mb, Cb = 4097, 32                                                          # planes beyond 4096 rows: refused; buffers at full height
    hout = sent(Mb, Cb)
    with pytest.raises(rt.NativeError, match="invalid argument"):
        rt.op_ln_reduce(dev(np.zeros((1, Mb * Cb), F32)), Mb * Cb, 1, None, None, Cb, dev(g[:Cb]), dev(b[:Cb]), None, Cb, hout, Cb, Mb, Cb,
                        1e-5, 1, None)
    assert untouched(host(hout))


# ---- LayerNorm with every field of its parameter block: relative L2 < 2e-6 against float64 ------------------------------------------------

LN_CASES = [  # C, groups, r1 (None / "full" / "shared"), r2, valid (None / "full" / "shared"), act
    (32, 3, "shared", True, "shared", 3), (64, 3, "shared", True, "shared", 3), (384, 3, "shared", True, "shared", 3),
    (512, 3, "shared", True, "shared", 3), (768, 3, "shared", True, "shared", 3), (1024, 3, "shared", True, "shared", 3),
    (512, 1, None, False, None, 0), (512, 5, None, False, None, 3), (512, 5, "shared", False, "full", 1),
    (768, 3, "full", False, "shared", 0), (384, 1, "full", True, "full", 3), (1024, 5, None, True, None, 1),
]


@pytest.mark.parametrize("C,groups,r1,r2,valid,act", LN_CASES)
def test_layernorm_ex_every_field(rt, C, groups, r1, r2, valid, act):
    rng = np.random.default_rng(C * 10 + groups)
    rpg = 7
    M = groups * rpg                                                          # 7, 21, 35: never a multiple of 4
    ldx, ldo, ldr1, ldr2 = C + 4, C + 8, C + 12, C + 16
    x = (rng.standard_normal((M, C)) * np.exp(rng.uniform(-1, 1, (M, 1))) + rng.standard_normal((M, 1))).astype(F32)
    g, b = (1 + 0.3 * rng.standard_normal((groups, C))).astype(F32), (0.3 * rng.standard_normal((groups, C))).astype(F32)
    R1, R2 = rng.standard_normal((M, C)).astype(F32), rng.standard_normal((M, C)).astype(F32)     # full height whatever is shared
    vm = (rng.random(M) > 0.3).astype(np.int32)
    vm[:rpg][[0, 3]] = [0, 1]
    r1_rows, valid_rows = (rpg if r1 == "shared" else 0), (rpg if valid == "shared" else 0)
    out = sent(M, ldo)
    flag = i32([0])
    rt.op_layernorm_ex(padded(x, ldx), ldx, dev(g), dev(b), rpg if groups > 1 else 0, None if r1 is None else padded(R1, ldr1), ldr1,
                       r1_rows, padded(R2, ldr2) if r2 else None, ldr2, None if valid is None else i32(vm), valid_rows, out, ldo, M, C,
                       1e-5, act, 0, flag)
    got = host(out)
    want = ref.layernorm(x, g, b, 1e-5, rpg if groups > 1 else 0, None if r1 is None else R1, r1_rows, R2 if r2 else None,
                         None if valid is None else vm, valid_rows, act)
    err = ref.rel_l2(got[:, :C], want)
    rows = np.linalg.norm(got[:, :C] - want, axis=1) / np.maximum(np.linalg.norm(want, axis=1), 1e-30)
    print("layernorm_ex rel L2", err, "worst row", float(rows.max()))
    assert err < 2e-6 and rows.max() < 2e-6 and untouched(got[:, C:]) and int(host(flag)[0]) == 0
    if valid is not None:
        dead = (vm[np.arange(M) % valid_rows] if valid_rows else vm) == 0
        assert dead.any() and not got[dead, :C].any()
    out = sent(M, ldo)
    rt.op_layernorm_ex(padded(x, ldx), ldx, dev(g), dev(b), 0, None, ldr1, 0, None, ldr2, None, 0, out, ldo, 0, C, 1e-5, act, 0, None)
    assert untouched(host(out))


@pytest.mark.parametrize("C,groups,act", [(512, 3, 1), (768, 1, 0), (1024, 5, 3)])
def test_layernorm_ex_planes(rt, C, groups, act):
    rng = np.random.default_rng(C + groups)
    rpg = 5
    M = groups * rpg
    x = (rng.standard_normal((M, C)) * 2 + 1).astype(F32)
    g, b = (1 + 0.3 * rng.standard_normal((groups, C))).astype(F32), (0.3 * rng.standard_normal((groups, C))).astype(F32)
    vm = np.ones(M, np.int32)
    vm[[1, M - 1]] = 0
    outs = []
    for pl in (0, 1):
        out, flag = sent(M, C + 32), i32([0])
        rt.op_layernorm_ex(dev(x), C, dev(g), dev(b), rpg if groups > 1 else 0, None, C, 0, None, C, i32(vm), 0, out, C + 32, M, C, 1e-5,
                           act, pl, flag)
        assert int(host(flag)[0]) == 0
        outs.append(host(out))
    assert ref.rel_l2(outs[0][:, :C], ref.layernorm(x, g, b, 1e-5, rpg if groups > 1 else 0, valid=vm, kind=act)) < 2e-6
    assert np.array_equal(outs[1][:, :C].copy().view(np.uint16), ref.planes(outs[0][:, :C])) and untouched(outs[1][:, C:])
    gbig = g.copy()
    gbig[0, 7] = 1e7                                                           # |y| >= 65504 in the live rows of group 0: the guard's word
    for pl, want_flag in ((1, 1), (0, 0)):
        out, flag = sent(M, C + 32), i32([0])
        rt.op_layernorm_ex(dev(x), C, dev(gbig), dev(b), rpg if groups > 1 else 0, None, C, 0, None, C, i32(vm), 0, out, C + 32, M, C, 1e-5,
                           0, pl, flag)
        assert int(host(flag)[0]) == want_flag
    with pytest.raises(rt.NativeError, match="invalid argument"):             # planes go with no residual
        rt.op_layernorm_ex(dev(x), C, dev(g), dev(b), 0, dev(x), C, 0, None, C, None, 0, out, C + 32, M, C, 1e-5, act, 1, None)


# ---- products and sums that may or may not contract to an FMA ---------------------------------------------------------------------------

@pytest.mark.parametrize("zero_pe", [False, True])
def test_adm_step_input(rt, zero_pe):
    rng = np.random.default_rng(40)
    Dc, De, n, A, ld_tc, pstride = 24, 8, 5, 3, 28, 9
    D = Dc + De
    tc_row = np.asarray([0, 9, 3], np.int32)
    tc = rng.standard_normal((9 + n, ld_tc)).astype(F32)
    w_dt, p = rng.standard_normal(De).astype(F32), (rng.standard_normal((A, pstride)) * 20).astype(F32)
    pe = np.zeros((n + 2, D), F32) if zero_pe else rng.standard_normal((n + 2, D)).astype(F32)
    x = sent(A * n + 1, D)
    rt.op_adm_step_input(dev(tc), ld_tc, i32(tc_row), dev(w_dt), dev(p), pstride, dev(pe), x, Dc, De, n, A)
    got = host(x)
    want, bound = ref.adm_step_input(tc, tc_row, w_dt, p, pe, Dc, De, n, A)
    err = np.abs(got[:A * n].astype(np.float64) - want)
    print("adm_step_input max err / bound", float((err / np.maximum(bound, 1e-300)).max()))
    assert (err <= bound).all() and untouched(got[A * n:])
    if zero_pe:
        assert np.array_equal(got[:A * n, :Dc], want[:, :Dc].astype(F32))      # the conditioning columns are copies
    x = sent(4, D)
    rt.op_adm_step_input(dev(tc), ld_tc, i32(tc_row), dev(w_dt), dev(p), pstride, dev(pe), x, Dc, De, n, 0)
    assert untouched(host(x))


@pytest.mark.parametrize("zero_pe", [False, True])
def test_plm_step_input(rt, zero_pe):
    rng = np.random.default_rng(41)
    Dc, De, n, A, ld_c, cstride, bins = 16, 16, 6, 3, 20, 10, 12
    D = Dc + De
    cond_row = np.asarray([4, 0, 11], np.int32)
    cond = rng.standard_normal((11 + n, ld_c)).astype(F32)
    emb = rng.standard_normal((bins, De)).astype(F32)
    codes = rng.integers(0, bins, (A, cstride)).astype(np.int64)
    codes[0, 0], codes[1, 2], codes[2, 5] = bins, -2, 1 << 40                  # clamped to the last / first / last row
    pe = np.zeros((n + 2, D), F32) if zero_pe else rng.standard_normal((n + 2, D)).astype(F32)
    x = sent(A * n + 1, D)
    rt.op_plm_step_input(dev(cond), ld_c, i32(cond_row), dev(emb), dev(codes), cstride, dev(pe), x, Dc, De, n, A, bins)
    got = host(x)
    want, bound = ref.plm_step_input(cond, cond_row, emb, codes, pe, Dc, De, n, A)
    err = np.abs(got[:A * n].astype(np.float64) - want)
    assert (err <= bound).all() and untouched(got[A * n:])
    if zero_pe:
        assert np.array_equal(got[:A * n], want.astype(F32))                   # both halves are copies
    x = sent(4, D)
    rt.op_plm_step_input(dev(cond), ld_c, i32(cond_row), dev(emb), dev(codes), cstride, dev(pe), x, Dc, De, n, 0, bins)
    assert untouched(host(x))


# ---- dot products: float64 with a bound from the kernel's summation depth ------------------------------------------------------------------

@pytest.mark.parametrize("D", [256, 768, 1024])
@pytest.mark.parametrize("last_only", [True, False])
def test_adm_predict(rt, D, last_only):
    rng = np.random.default_rng(D + last_only)
    A, n, pstride = 5, 4, 8
    xn = 1 if last_only else n
    x = (rng.standard_normal((A * xn, D)) * np.exp(rng.uniform(-2, 2, (A * xn, 1)))).astype(F32)
    w = rng.standard_normal(D).astype(F32)
    p = sent(A + 1, pstride)
    rt.op_adm_predict(dev(x), D, dev(w), p, pstride, n, xn, A)
    got = host(p)
    dot, mag = ref.dot_rows(x.reshape(A, xn, D)[:, xn - 1], w)
    err = np.abs(got[:A, n].astype(np.float64) - dot)
    bound = (D / 64 + 8) * 2.0 ** -24 * mag
    print("adm_predict max err / bound", float((err / bound).max()))
    assert (err <= bound).all()
    got[:A, n] = SENTINEL
    assert untouched(got)
    p = sent(2, pstride)
    rt.op_adm_predict(dev(x), D, dev(w), p, pstride, n, xn, 0)
    assert untouched(host(p))


@pytest.mark.parametrize("D", [8, 100, 256, 1024])
def test_row_sqnorm(rt, D):
    rng = np.random.default_rng(D)
    N = 7
    E = (rng.standard_normal((N, D)) * np.exp(rng.uniform(-2, 2, (N, 1)))).astype(F32)
    ee = sent(N + 1)
    rt.op_row_sqnorm(dev(E), D, ee, N)
    got = host(ee)
    dot, mag = ref.dot_rows(E, E)
    err = np.abs(got[:N].astype(np.float64) - dot)
    assert (err <= (D / 64 + 8) * 2.0 ** -24 * mag).all() and untouched(got[N:])
    ee = sent(2)
    rt.op_row_sqnorm(dev(E), D, ee, 0)
    assert untouched(host(ee))


def test_magnitude_two_ulp_and_zero_tail(rt):
    rng = np.random.default_rng(50)
    F, lds, ldo, M = 13, 30, 16, 9
    spec = (rng.standard_normal((M, lds)) * np.exp(rng.uniform(-6, 6, (M, lds)))).astype(F32)
    spec[0, :2], spec[0, F:F + 2] = 0, [0, 3]
    out = sent(M + 1, ldo)
    rt.op_magnitude(dev(spec), lds, F, out, ldo, M)
    got = host(out)
    want = ref.magnitude(spec, F)
    ulp = np.spacing(want.astype(F32)).astype(np.float64)
    err = np.abs(got[:M, :F].astype(np.float64) - want)
    print("magnitude max err in ulp", float((err / ulp).max()))
    assert (err <= 2 * ulp).all() and got[0, 0] == 0 and got[0, 1] == 3
    assert not got[:M, F:].any() and untouched(got[M:])
    out = sent(2, ldo)
    rt.op_magnitude(dev(spec), lds, F, out, ldo, 0)
    assert untouched(host(out))


# ---- conv_post: relative L2 < 3e-6 per utterance against float64 ------------------------------------------------------------------------

@pytest.mark.parametrize("R", [1, 255, 256, 257, 1000])
@pytest.mark.parametrize("k", [3, 7, 15])
@pytest.mark.parametrize("ch", [8, 32])
def test_conv_post_fused_chain(rt, ch, k, R):
    xs, w, bias, valid, utts = ref.conv_post_inputs(ch, k, R)
    slope = 0.1
    for three, masked in ((True, True), (False, False), (True, False), (False, True)):
        x1, x2 = (xs[1], xs[2]) if three else (None, None)
        out = sent(R + 1)
        rt.op_conv_post(dev(xs[0]), None if x1 is None else dev(x1), None if x2 is None else dev(x2), 1.0 / 3.0, R, ch, k, dev(w), dev(bias),
                        slope, i32(valid) if masked else None, out)
        got = host(out)
        want = ref.conv_post(xs[0], x1, x2, 1.0 / 3.0, w, bias, slope, valid if masked else None)
        assert np.abs(want).max() < 0.9
        assert untouched(got[R:])
        for a, e in utts:
            err = ref.rel_l2(got[a:e], want[a:e])
            print("conv_post", ch, k, R, three, masked, (a, e), "rel L2", err)
            assert err < 3e-6
        if masked:
            assert not got[:R][valid == 0].any()
        else:
            assert ref.rel_l2(got[:R], want) < 3e-6                           # gap rows included: tanh(bias + halo taps)


def test_conv_post_limits(rt):
    x, w, b = dev(np.zeros((4, 128), F32)), dev(np.zeros((17, 128), F32)), dev(np.zeros(1, F32))
    out = sent(4)
    with pytest.raises(rt.NativeError, match="hipErrorNotSupported"):          # (256 + 14) x 129 + 15 x 128 floats > 64 KiB of LDS
        rt.op_conv_post(x, None, None, 1.0, 4, 128, 15, w, b, 0.1, None, out)
    for k in (4, 17):
        with pytest.raises(rt.NativeError, match="hipErrorInvalidValue"):
            rt.op_conv_post(x, None, None, 1.0, 4, 8, k, w, b, 0.1, None, out)
    rt.op_conv_post(x, None, None, 1.0, 0, 8, 3, w, b, 0.1, None, out)        # R = 0
    assert untouched(host(out))


# ---- arg-max and VQ arg-min: exact indices ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("N,ldx", [(1, 1), (3, 3), (64, 68), (64, 67), (100, 104), (100, 101), (1024, 1028), (1025, 1025), (1025, 1028),
                                   (4096, 4100), (4096, 4097)])
def test_argmax_rows_ties_infinities_and_nan(rt, N, ldx):
    """(N | ldx) % 4 == 0: the float4 path; otherwise the scalar one.  The wanted index is what torch.argmax returns on the row
    (tests/test_rowops_ref_host.py pins ref.argmax_row to it)."""
    rng = np.random.default_rng(N * 7 + ldx)
    x = ref.argmax_cases(N, rng)
    A = x.shape[0]
    out = sent(A + 1, 3, dtype=np.int64)
    rt.op_argmax_rows(padded(x, ldx, fill=np.inf), ldx, N, out, 3, 1, A)       # +inf in the pad columns: reading one would win
    got = host(out)
    want = ref.argmax_rows(x)
    bad = np.nonzero(got[:A, 1] != want)[0]
    print("argmax rows that differ:", bad.tolist(), got[bad, 1].tolist(), want[bad].tolist())
    assert ((got[:A, 1] >= 0) & (got[:A, 1] < N)).all()
    assert np.array_equal(got[:A, 1], want)
    got[:A, 1] = ISENT
    assert untouched(got)                                                      # only column ooff of rows < A was written
    out = sent(2, 3, dtype=np.int64)
    rt.op_argmax_rows(padded(x, ldx), ldx, N, out, 3, 1, 0)
    assert untouched(host(out))


@pytest.mark.parametrize("N", [3, 64, 100, 1025])
def test_vq_argmin_masked_rows_ties_and_nan(rt, N):
    """x, xe and ee are multiples of 1/4: every sum is exact in float32, so the distances of the reference are the kernel's bit for
    bit and planted ties are ties.  A NaN in x makes every distance of the row NaN (index 0, as Tensor.max(-1).indices)."""
    rng = np.random.default_rng(N)
    M, D, ldx, ldxe = 11, 8, 12, N + 3                                         # M % 4 != 0
    x = (rng.integers(-8, 9, (M, D)) / 4).astype(F32)
    xe = (rng.integers(-64, 65, (M, N)) / 4).astype(F32)
    ee = (rng.integers(0, 129, N) / 4).astype(F32)
    ee[N - 1] = ee[0]
    xe[:, N - 1] = xe[:, 0]                                                   # column N - 1 ties with column 0 in every row
    xe[1, :] = 0
    valid = np.ones(M, np.int32)
    valid[[2, 10]] = 0
    x[3, 5] = np.nan                                                          # every distance NaN
    x[4, :] = np.nan
    xe[5, N // 2] = np.nan                                                    # one NaN distance: its index
    xe[6, [N // 3, N - 1]] = np.nan
    xe[7, :] = -np.inf                                                        # every distance -inf: index 0
    x[10, 0] = np.nan                                                         # masked: index 0 whatever the row holds
    idx = sent(M + 1, dtype=np.int64)
    rt.op_vq_argmin(padded(x, ldx), ldx, D, padded(xe, ldxe, fill=np.inf), ldxe, dev(ee), N, i32(valid), idx, M)
    got = host(idx)
    want = ref.vq_argmin(x, xe, ee, valid)
    print("vq_argmin got", got[:M].tolist(), "want", want.tolist())
    assert ((got[:M] >= 0) & (got[:M] < N)).all()
    assert np.array_equal(got[:M], want) and untouched(got[M:])
    idx = sent(M + 1, dtype=np.int64)
    rt.op_vq_argmin(padded(x, ldx), ldx, D, padded(xe, ldxe), ldxe, dev(ee), N, None, idx, M)      # no mask
    assert np.array_equal(host(idx)[:M], ref.vq_argmin(x, xe, ee, None))
    idx = sent(2, dtype=np.int64)
    rt.op_vq_argmin(padded(x, ldx), ldx, D, padded(xe, ldxe), ldxe, dev(ee), N, None, idx, 0)
    assert untouched(host(idx))


# ---- the dispatcher itself ---------------------------------------------------------------------------------------------------------------

def test_op_row_rejects_unknown_names_and_wrong_counts(rt):
    out = sent(4)
    with pytest.raises(rt.NativeError, match="unknown op"):
        rt.op_row("gather_cols", out, 4)
    with pytest.raises(rt.NativeError, match="wrong argument count"):
        rt.op_row("row_sqnorm", out, 4, out)                                   # one integer short
    with pytest.raises(rt.NativeError, match="wrong argument count"):
        rt.op_row("avg3", out, out, out, 1, out, 4)                            # the scale as an integer
    assert untouched(host(out))
