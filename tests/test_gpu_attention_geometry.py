"""Launch geometry of the attention kernels (GPU): the four UNIFORM forms the AR steps launch (csrc/model_stages.hip: attention_self
in ar_step_layers, encoder_layer_last on its tiled and its skinny path, encoder_layer_first_cached; tests/attn_ref.py model_form) on
every kernel of csrc/attention.hip, through mt2_op_attention_desc - every field of the launch explicit, and the kernel the routing
chose reported back, so that every case first asserts the kernel it names.

Per case, on buffers with three rows before the first and two after the last sequence (and, in the cached form, seven unwritten rows
at the end of every slot), all of them NaN in Q, K and V, and an output buffer pre-filled with a sentinel:
  1. the uniform launch and the ragged launch that names the same rows (start / len arrays, an explicit o_start, max_kvlen = the key
     count) run the same kernel and leave the same bits in the whole output buffer;
  2. float64 parity per (sequence, head) block: relative L2 < 3e-6 (the bar of tests/test_gpu_kernels.py);
  3. per row: no output row's error norm exceeds 3e-6 x the largest reference row norm of its block.  A plain float32 numpy
     softmax-attention (attn_ref.attention_f32) reaches 5.9e-7 on that measure on standard-normal data with a spike at D 32 - 128 and
     n 33 - 300, and 1.25e-6 on the cases of this file (one-row blocks and the wide heads included): the bar leaves 2.4 - 5x over f32
     arithmetic; a misplaced or stale row misses it by five orders of magnitude;
  4. the output is finite: no kernel lets a row outside its ranges into the arithmetic (a select, not a multiply by zero);
  5. exactly the rows attn_ref names are written - every other row of the buffer keeps the sentinel; with o_planes (cached form) the
     planes are the numpy split of the same kernel's f32 output, bit for bit;
  6. with ONE key the soft-max weight is exactly 1: O[b, h] = V[b, h] bit for bit (f32 kernels);
and one sequence of the batch launched alone (B = 1, pointers moved by the strides) gives the bits it has inside the batch.
test_output_rows_of_their_own moves the output rows of every kernel with o_start, in both geometries (the generic kernel's forms above
never have output rows that differ from their query rows).

Worst measured ratios per kernel over all cases of this file on an MI355X (block = relative L2 of a block, row = the per-row measure;
the bar for both is 3e-6; f32 = attention_f32's worst row measure on the same cases):
    kernel    block      row        f32       case of the worst row
    ds        2.91e-07   6.76e-07   1.25e-06  2x96 full n = 128
    reg       6.30e-07   1.13e-06   1.06e-06  1x128 cached n = 200
    generic   6.35e-07   1.46e-06   8.47e-07  1x512 full n = 40
    lds       5.00e-07   1.18e-06   1.24e-06  1x128 full n = 257, 8 query tiles
    x6        3.68e-07   1.06e-06   1.16e-06  2x64 full n = 200, 4 query tiles
    x3h       2.44e-07   6.71e-07   1.16e-06  2x96 full n = 200, 8 query tiles
No kernel comes nearer to the bar than a factor of 2.  Every case prints its three figures (pytest -s) before it asserts.
"""
import math

import numpy as np
import pytest

import attn_ref as R

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BAR = 3e-6
SENTINEL = np.float32(-1234.5)
F32_KERNELS = ("generic", "reg", "ds", "lds")


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    runtime.device_check()
    return runtime


def _cases():
    out = []
    for H, D in ((2, 64), (2, 96)):
        for form in R.FORMS:
            for n in (1, 32, 33, 128):
                out.append(("ds", H, D, form, n, 5, 0))
    for H, D in ((2, 64), (2, 96), (2, 32), (1, 128)):
        for form in R.FORMS:
            for n in (33, 129, 200):
                out.append(("reg", H, D, form, n, 3, 0))
    for H, D in ((2, 256), (1, 512)):
        for form in ("full", "last-compact"):
            out.append(("generic", H, D, form, 40, 3, 0))
    for H, D in ((2, 32), (2, 64), (1, 128)):
        for form in ("full", "cached"):
            for n in (129, 257):
                for waves in (4, 8):
                    out.append(("lds", H, D, form, n, 3, waves))
    for kernel in ("x6", "x3h"):
        for H, D in ((2, 64), (2, 96)):
            for form in ("full", "cached"):
                for n in (129, 200):
                    for waves in (4, 8):
                        out.append((kernel, H, D, form, n, 3, waves))
    return out


CASES = _cases()


def options(kernel, D, n, waves):
    """How the case forces its kernel: nothing here is a default of the library."""
    o = dict(lds_min_qlen=0, x6_min_qlen=0, lds_waves=waves, ds_short=1, x3h=0, o_planes=0)
    if kernel == "reg" and D in (64, 96) and n <= 128:
        o["ds_short"] = 0               # more than 128 keys, or a head dim of 32 / 128, get there by themselves
    elif kernel == "lds":
        o["lds_min_qlen"] = 1
    elif kernel in ("x6", "x3h"):
        o["x6_min_qlen"] = 1
        o["x3h"] = 1 if kernel == "x3h" else 0
    return o


def launch(rt, f, dev, g, out, scale, opts, flag, move=(0, 0, 0)):
    """One launch of form f with geometry g (f.g, its ragged statement, or one sequence of it with the pointers moved by `move` rows)."""
    ptr = lambda t, at, rows: t[at[1] + rows:, at[2]:]
    arr = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a, np.int32)).cuda()
    keep = [arr(a) for a in (g.q_start, g.q_len, g.kv_start, g.kv_len, g.o_start)]
    kernel = rt.op_attention_desc(ptr(dev[f.q[0]], f.q, move[0]), f.ldq, ptr(dev[f.k[0]], f.k, move[1]), f.ldk,
                                  ptr(dev[f.v[0]], f.v, move[1]), f.ldv, ptr(out, f.o, move[2]), f.ldo,
                                  B=g.B, H=g.H, D=g.D, max_qlen=g.max_qlen, max_kvlen=g.max_kvlen, scale=scale,
                                  q_start=keep[0], q_len=keep[1], kv_start=keep[2], kv_len=keep[3], o_start=keep[4],
                                  u_qstride=g.u_qstride, u_qlen=g.u_qlen, u_kvstride=g.u_kvstride, u_kvlen=g.u_kvlen, u_ostride=g.u_ostride,
                                  flag=flag, **opts)
    torch.cuda.synchronize()            # the start / len arrays stay alive until the kernel is done
    return kernel


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.mark.parametrize("kernel,H,D,form,n,A,waves", CASES,
                         ids=[f"{c[0]}{c[6] or ''}-{c[1]}x{c[2]}-{c[3]}-n{c[4]}" for c in CASES])
def test_uniform_geometry(rt, kernel, H, D, form, n, A, waves):
    f = R.model_form(form, A, n, H, D)
    g, d, scale = f.g, H * D, 1.0 / math.sqrt(D)
    rng = np.random.default_rng([H, D, n, A, waves, R.FORMS.index(form)])
    spike = A - 2
    host = R.fill(f, rng, spike_seq=spike)
    Q, K, V = (R.view(host, at) for at in (f.q, f.k, f.v))
    ref, rows = R.attention_ref(Q, K, V, g, scale, f.o_rows)         # also: every row the geometry names exists (checked on the host)
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items() if k != "o"}
    fresh = lambda: torch.full(f.bufs["o"], float(SENTINEL), device="cuda", dtype=torch.float32)
    flag = torch.zeros(4, device="cuda", dtype=torch.int32)
    opts = options(kernel, D, n, waves)

    o_uni = fresh()
    assert launch(rt, f, dev, g, o_uni, scale, opts, flag) == kernel
    # 1. the ragged statement of the same rows: same kernel, same bits, in every row of the buffer
    o_rag = fresh()
    assert launch(rt, f, dev, R.as_ragged(g), o_rag, scale, opts, flag) == kernel
    whole = o_uni.cpu().numpy()
    assert np.array_equal(bits(whole), bits(o_rag.cpu().numpy()))
    # 5. the write set: exactly the rows the reference names
    out = whole[f.o[1]:]
    written = np.zeros(whole.shape[0], bool)
    written[f.o[1] + rows] = True
    assert (bits(whole[~written]) == bits(SENTINEL)).all(), "a row outside the launch's write set changed"
    # 4. nothing of the NaN rows around and between the sequences reached the output
    assert np.isfinite(whole[written]).all()
    assert not (bits(whole[written]) == bits(SENTINEL)).all(axis=1).any(), "a row of the write set was not written"
    # 2. and 3.: float64 parity per block and per row
    errs = R.block_errors(out, ref, g)
    f32 = max(e[3] for e in R.block_errors(R.attention_f32(Q, K, V, g, scale, f.o_rows), ref, g))
    worst_block, worst_row = max(e[2] for e in errs), max(e[3] for e in errs)
    print(f"ATTN_GEOM kernel={kernel} case={H}x{D}-{form}-n{n}-w{waves} block={worst_block:.3e} row={worst_row:.3e} f32={f32:.3e}")
    assert len(errs) == A * H
    for b, h, block, row in errs:
        assert block < BAR, (b, h, block)
        assert row <= BAR, (b, h, row)
    # 6. one key: the weight is exactly 1
    if n == 1 and kernel in F32_KERNELS:
        for (_, ql, ks, _, os_) in R.ranges(g):
            assert ql == 1 and np.array_equal(bits(out[os_, :d]), bits(V[ks, :d]))
    # one sequence launched alone: the bits it has inside the batch, and nobody else's rows
    g1, move = R.one_sequence(g, spike)
    o_one = fresh()
    assert launch(rt, f, dev, g1, o_one, scale, opts, flag, move) == kernel
    alone = o_one.cpu().numpy()
    _, ql, _, _, os_ = R.ranges(g)[spike]
    mine = np.zeros(whole.shape[0], bool)
    mine[f.o[1] + os_:f.o[1] + os_ + ql] = True
    assert np.array_equal(bits(alone[mine]), bits(whole[mine])) and (bits(alone[~mine]) == bits(SENTINEL)).all()
    # 5., planes: the cached form hands its output to the out-projection as fp16 planes
    if form == "cached" and kernel != "generic":
        o_pl = fresh()
        assert launch(rt, f, dev, g, o_pl, scale, dict(opts, o_planes=1), flag) == kernel
        planes = o_pl.cpu().numpy()
        assert (bits(planes[~written]) == bits(SENTINEL)).all()
        o = whole[written]
        hi = o.astype(np.float16)
        lo = ((o - hi.astype(np.float32)) * np.float32(2048.0)).astype(np.float16)
        m = o.shape[0]
        want = np.concatenate([hi.reshape(m, d // 32, 1, 32), lo.reshape(m, d // 32, 1, 32)], axis=2).reshape(m, 2 * d)
        assert np.array_equal(np.ascontiguousarray(planes[written]).view(np.uint16), want.view(np.uint16))
    assert int(flag[0].item()) == 0         # nothing left the fp16 range


@pytest.mark.parametrize("uniform", [False, True], ids=["ragged", "uniform"])
@pytest.mark.parametrize("kernel,H,D,n,waves", [("ds", 2, 64, 33, 0), ("reg", 2, 32, 33, 0), ("generic", 2, 256, 40, 0), ("lds", 2, 64, 129, 4),
                                                ("x6", 2, 96, 129, 4), ("x3h", 2, 64, 129, 8)],
                         ids=["ds", "reg", "generic", "lds", "x6", "x3h"])
def test_output_rows_of_their_own(rt, kernel, H, D, n, waves, uniform):
    """o_start: no path of the model sets it, every kernel honours it - in the ragged geometry, and in the uniform one, where it takes
    precedence over u_ostride.  The sequences of the full form write in reverse order (sequence b to the rows of sequence A - 1 - b):
    the same bits as the plain launch, at the moved rows, and nothing else of the buffer changes."""
    from dataclasses import replace
    A = 3
    f = R.model_form("full", A, n, H, D)
    scale = 1.0 / math.sqrt(D)
    host = R.fill(f, np.random.default_rng([H, D, n, 77]), spike_seq=1)
    Q, K, V = (R.view(host, at) for at in (f.q, f.k, f.v))
    dev = {k: torch.from_numpy(v).cuda() for k, v in host.items() if k != "o"}
    fresh = lambda: torch.full(f.bufs["o"], float(SENTINEL), device="cuda", dtype=torch.float32)
    flag = torch.zeros(4, device="cuda", dtype=torch.int32)
    opts = options(kernel, D, n, waves)
    o_start = np.asarray([(A - 1 - b) * n for b in range(A)], np.int32)
    g = replace(f.g if uniform else R.as_ragged(f.g), o_start=o_start)
    ref, rows = R.attention_ref(Q, K, V, g, scale, f.o_rows)
    assert rows.tolist() == list(range(A * n)) and [r[4] for r in R.ranges(g)] == o_start.tolist()
    plain, moved = fresh(), fresh()
    assert launch(rt, f, dev, f.g, plain, scale, opts, flag) == kernel
    assert launch(rt, f, dev, g, moved, scale, opts, flag) == kernel
    plain, moved = plain.cpu().numpy(), moved.cpu().numpy()
    lead = f.o[1]
    for b in range(A):
        assert np.array_equal(bits(moved[lead + o_start[b]:lead + o_start[b] + n]), bits(plain[lead + b * n:lead + (b + 1) * n])), b
    assert (bits(moved[:lead]) == bits(SENTINEL)).all() and (bits(moved[lead + A * n:]) == bits(SENTINEL)).all()
    for _, _, block, row in R.block_errors(moved[lead:], ref, g):
        assert block < BAR and row <= BAR
