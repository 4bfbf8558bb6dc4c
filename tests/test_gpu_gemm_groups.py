"""Kernel-level parity (GPU) of GROUPED launches of the tiled GEMM engine (grid.z = groups), one launch at a time through
mt2_op_gemm_grouped: every live general tile on the stride combinations the model uses (csrc/model_stages.hip: run_stack, mel_context_rows,
splitk_params), against the same tile on one group at a time (bit for bit) and against float64; plus the two epilogue activations
that only the stage tests ran (tanh, log-clamp).  The fp16-pipe strides come from the model's own rule (runtime.x3h_group_planes)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

G = 3                                                   # groups: a stride wrong by one group and a stride of 0 both show
SENT = np.float32(-777.25)                              # what every output buffer holds before a launch
F32_CFGS = [3, 12, 15, 16, 17, 18, 20, 22, 23, 28]      # the live general f32-MFMA tiles
X6_CFGS = [51, 55, 84, 85, 86]                          # bf16 pipe: loader tiles, K-split tiles
X3H_CFGS = [103, 95, 96, 97]                            # fp16 pipe: loader tile, K-split tiles
KSPLIT = [84, 85, 86, 95, 96, 97]                       # linear layers only (taps = 1)
ROWMAP_CFGS = [3, 12, 17, 18, 22, 28]                   # what test_gemm_strided_conv_rowbase runs with a row map
SKINNY64 = 88                                           # the plain weight-streaming kernel at 33 .. 64 rows
WINDOW_CFGS = [30, 31, 32, 34, 58, 59, 98, 99, 100]
PLANE_PIPES = set(X6_CFGS + X3H_CFGS + [34, 58, 59, 98, 99, 100])


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    if dtype is not None:
        t = t.to(dtype)
    return t.cuda()


def rel(a, b):
    a = np.asarray(a, np.float64)
    b = np.asarray(b, np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    runtime.device_check()
    return runtime


@pytest.fixture(scope="module")
def cases():
    return {}            # scenario name -> operands on the device + float64 references, built once


def wide(rng, shape, decades):
    """Values over several decades, so that the low planes of the 16-bit pipes matter."""
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-decades, decades, shape))).astype(np.float32)


def finish(rt, c, X, Wbuf, bias, R, valid, refs, rowbase=None):
    """Numpy operands -> the device side of a case.  X / bias / R: flat buffers the groups step through."""
    c["X"] = dev(X.reshape(-1))
    c["wts"] = rt.GemmWeights(torch.from_numpy(np.ascontiguousarray(Wbuf)))
    c["bias"] = dev(bias.reshape(-1)) if bias is not None else None
    c["R"] = dev(R.reshape(-1)) if R is not None else None
    c["valid_np"] = valid
    c["valid"] = dev(valid) if valid is not None else None
    c["rowbase"] = dev(rowbase) if rowbase is not None else None
    c["refs"] = refs
    c["e32"] = None
    return c


def padded(R, ldr, gap):
    """[groups][M, N] -> flat, rows ldr apart, groups M * ldr + gap apart (the padding holds finite junk)."""
    g, M, N = R.shape
    buf = np.full((g, M * ldr + gap), 3.0, np.float32)
    buf[:, :M * ldr].reshape(g, M, ldr)[:, :, :N] = R
    return buf


def conv_ref(X, W, taps, dil, shift0, Cin, rows=None):
    """float64: out[m] = sum_t X[src(m) + t * dil] @ W[:, t * Cin:(t + 1) * Cin]^T, rows outside X read as zeros."""
    Rx = X.shape[0]
    src0 = np.arange(Rx) + shift0 if rows is None else np.asarray(rows)
    out = np.zeros((src0.size, W.shape[0]))
    Xd, Wd = X.astype(np.float64), W.astype(np.float64)
    for t in range(taps):
        src = src0 + t * dil
        ok = (src >= 0) & (src < Rx)
        a = np.zeros((src0.size, Cin))
        a[ok] = Xd[src[ok], :Cin]
        out += a @ Wd[:, t * Cin:(t + 1) * Cin].T
    return out


def case_branches(rt, M, shared, conv, seed):
    """Scenarios (a) / (b): the parallel branches of a conv stack (run_stack) - weights, bias, residual and output per group, one row
    mask, ReLU prologue, the input per group or shared by all (strideX = 0).  The weights start one matrix into their buffer."""
    rng = np.random.default_rng(seed)
    if conv:
        taps, Cin, N = 5, 64, 96
        lens, gap = [37, 1, 64, 5], 3
        off, rows = [], gap
        for n in lens:
            off.append(rows)
            rows += n + gap
        M = rows
        valid = np.zeros(M, np.int32)
        X = np.zeros((G, M, Cin), np.float32)
        for o, n in zip(off, lens):
            valid[o:o + n] = 1
            X[:, o:o + n] = wide(rng, (G, n, Cin), 3)
    else:
        taps, Cin, N = 1, 256, 160
        valid = (rng.random(M) > 0.1).astype(np.int32)
        valid[17] = 1                                   # (the range-guard test plants its value in this row)
        X = wide(rng, (G, M, Cin), 3)
    K = taps * Cin
    Wbuf = (rng.standard_normal(((G + 1) * N, K)) / math.sqrt(K) * np.exp(rng.uniform(-2, 2, ((G + 1) * N, K)))).astype(np.float32)
    bias = rng.standard_normal((G, N)).astype(np.float32)
    Rg = rng.standard_normal((G, M, N)).astype(np.float32)
    ldr, ldc = N + 4, N + 4
    c = dict(M=M, N=N, Cin=Cin, taps=taps, dil=1, shift0=-((taps - 1) // 2), ldx=Cin, Rx=M, ldw=K, groups=G,
             strideX=0 if shared else M * Cin, w_off=N * K, strideW=N * K, strideB=N, strideR=M * ldr + 8, ldr=ldr,
             ldc=ldc, strideC=M * ldc + 8, tail=8, pro_act=rt.ACT_RELU, conv=conv)
    refs = []
    for g in range(G):
        Xg = np.maximum(X[0 if shared else g], 0)
        Wg = Wbuf[(1 + g) * N:(2 + g) * N]
        refs.append((conv_ref(Xg, Wg, taps, 1, c["shift0"], Cin) + bias[g] + Rg[g]) * valid[:, None])
    return finish(rt, c, X[0] if shared else X, Wbuf, bias, padded(Rg, ldr, 8), valid, refs)


def case_rowmap(rt):
    """Scenario (c): mel_context_rows - a stride-4 convolution through a row map, ONE weight matrix and bias for all groups
    (strideW = strideB = 0), the input per group, fewer output rows than input rows."""
    rng = np.random.default_rng(31)
    Cin, N, k, s = 64, 96, 5, 4
    lens, gap = [150, 16, 1, 297], 2
    off, rows = [], gap
    for n in lens:
        off.append(rows)
        rows += n + gap
    X = np.zeros((G, rows, Cin), np.float32)
    for o, n in zip(off, lens):
        X[:, o:o + n] = wide(rng, (G, n, Cin), 3)
    base = []
    for o, n in zip(off, lens):
        base += [o + j * s - s // 2 for j in range((n - 1) // s + 1)]
    base = np.asarray(base, np.int32)
    M, K = base.size, k * Cin
    assert M < rows and base.min() >= 0 and base.max() + k - 1 < rows
    Wbuf = (rng.standard_normal((N, K)) / math.sqrt(K) * np.exp(rng.uniform(-2, 2, (N, K)))).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    Rg = rng.standard_normal((G, M, N)).astype(np.float32)
    valid = (rng.random(M) > 0.1).astype(np.int32)
    ldr, ldc = N + 4, N + 4
    c = dict(M=M, N=N, Cin=Cin, taps=k, dil=1, shift0=0, ldx=Cin, Rx=rows, ldw=K, groups=G, strideX=rows * Cin, w_off=0, strideW=0,
             strideB=0, strideR=M * ldr + 8, ldr=ldr, ldc=ldc, strideC=M * ldc + 8, tail=8, pro_act=rt.ACT_NONE, conv=True)
    refs = [(conv_ref(X[g], Wbuf, k, 1, 0, Cin, rows=base) + bias + Rg[g]) * valid[:, None] for g in range(G)]
    return finish(rt, c, X, Wbuf, bias, padded(Rg, ldr, 8), valid, refs, rowbase=base)


def case_kslices(rt):
    """Scenario (d): splitk_params - S = 4 slices of K = 1024 of the same rows (strideX = strideW = K / S with ldx = ldw = K), raw
    partial slabs, no bias.  The weight rows start 16 rows into their buffer."""
    rng = np.random.default_rng(41)
    M, N, K, S = 77, 128, 1024, 4
    X = wide(rng, (M, K), 3)
    Wbuf = (rng.standard_normal((16 + N, K)) / math.sqrt(K) * np.exp(rng.uniform(-2, 2, (16 + N, K)))).astype(np.float32)
    ldc = N + 4
    c = dict(M=M, N=N, Cin=K // S, taps=1, dil=1, shift0=0, ldx=K, Rx=M, ldw=K, groups=S, strideX=K // S, w_off=16 * K,
             strideW=K // S, strideB=0, strideR=0, ldr=0, ldc=ldc, strideC=M * ldc + 8, tail=8, pro_act=rt.ACT_NONE, conv=False)
    Xd, Wd = X.astype(np.float64), Wbuf[16:].astype(np.float64)
    refs = [Xd[:, g * 256:(g + 1) * 256] @ Wd[:, g * 256:(g + 1) * 256].T for g in range(S)]
    c["full"] = Xd @ Wd.T
    return finish(rt, c, X, Wbuf, None, None, None, refs)


def case_aplanes(rt):
    """Scenario (e): scenario (a) with the A operand handed over as fp16 planes by a LayerNorm (run_stack from its second block on:
    the ReLU is folded into the producer, the GEMM has no prologue).  Output gaps in whole 128-byte blocks."""
    rng = np.random.default_rng(51)
    M, N, K = 300, 160, 256
    raw = (rng.standard_normal((G * M, K)) * np.exp(rng.uniform(-2, 2, (G * M, 1)))).astype(np.float32)
    gam, bet = (1 + 0.2 * rng.standard_normal(K)).astype(np.float32), (0.1 * rng.standard_normal(K)).astype(np.float32)
    h = rt.op_layernorm(dev(raw), dev(gam), dev(bet), act=rt.ACT_RELU)
    hp = rt.op_layernorm(dev(raw), dev(gam), dev(bet), act=rt.ACT_RELU + 100)
    X = h.cpu().numpy().reshape(G, M, K)
    Wbuf = (rng.standard_normal(((G + 1) * N, K)) / math.sqrt(K) * np.exp(rng.uniform(-2, 2, ((G + 1) * N, K)))).astype(np.float32)
    bias = rng.standard_normal((G, N)).astype(np.float32)
    Rg = rng.standard_normal((G, M, N)).astype(np.float32)
    valid = (rng.random(M) > 0.1).astype(np.int32)
    ldr, ldc = N + 32, N + 32
    c = dict(M=M, N=N, Cin=K, taps=1, dil=1, shift0=0, ldx=K, Rx=M, ldw=K, groups=G, strideX=M * K, w_off=N * K, strideW=N * K,
             strideB=N, strideR=M * ldr + 32, ldr=ldr, ldc=ldc, strideC=M * ldc + 32, tail=32, pro_act=rt.ACT_NONE, conv=False)
    refs = [(X[g].astype(np.float64) @ Wbuf[(1 + g) * N:(2 + g) * N].astype(np.float64).T + bias[g] + Rg[g]) * valid[:, None]
            for g in range(G)]
    finish(rt, c, X, Wbuf, bias, padded(Rg, ldr, 32), valid, refs)
    c["X_planes"] = hp.reshape(-1)
    return c


BUILDERS = {
    "a": lambda rt: case_branches(rt, 300, False, False, 11),
    "a_shared": lambda rt: case_branches(rt, 300, True, False, 12),
    "a33": lambda rt: case_branches(rt, 33, False, False, 13),
    "a33_shared": lambda rt: case_branches(rt, 33, True, False, 14),
    "a64": lambda rt: case_branches(rt, 64, False, False, 15),
    "a64_shared": lambda rt: case_branches(rt, 64, True, False, 16),
    "b": lambda rt: case_branches(rt, 0, False, True, 21),
    "b_shared": lambda rt: case_branches(rt, 0, True, True, 22),
    "c": case_rowmap,
    "d": case_kslices,
    "e": case_aplanes,
}


def get_case(rt, cases, name):
    if name not in cases:
        cases[name] = BUILDERS[name](rt)
    return cases[name]


def new_out(c):
    n = (c["groups"] - 1) * c["strideC"] + c["M"] * c["ldc"] + c["tail"]
    return torch.full((n,), float(SENT), device="cuda", dtype=torch.float32)


def launch(rt, c, cfg, out, g0=0, groups=None, flag=None, X=None, **over):
    """Groups g0 .. g0 + groups - 1 of case c (default: all of them) in ONE launch: the pointers move by g0 strides; a single
    group is launched with groups = 1 and every stride 0."""
    n = c["groups"] if groups is None else groups
    st = (lambda v: v) if n > 1 else (lambda v: 0)
    Xf = c["X"] if X is None else X
    at = lambda t, stride: None if t is None else t[g0 * stride:]
    kw = dict(M=c["M"], N=c["N"], Cin=c["Cin"], ldx=c["ldx"], Rx=c["Rx"], ldw=c["ldw"], ldc=c["ldc"], groups=n,
              strideX=st(c["strideX"]), strideW=st(c["strideW"]), strideC=st(c["strideC"]), w_off=c["w_off"] + g0 * c["strideW"],
              taps=c["taps"], dil=c["dil"], a_mul=1, shift0=c["shift0"], rowbase=c["rowbase"], bias=at(c["bias"], c["strideB"]),
              strideB=st(c["strideB"]), R=at(c["R"], c["strideR"]), strideR=st(c["strideR"]), ldr=c["ldr"], valid=c["valid"],
              pro_act=c["pro_act"], pro_slope=0.0, epi_act=rt.ACT_NONE, out_scale=1.0, force_cfg=cfg, flag=flag)
    kw.update(over)
    return rt.op_gemm_grouped(at(Xf, c["strideX"]), c["wts"], at(out, c["strideC"]), **kw)


def group_views(c, out):
    """flat output buffer -> ([groups][M, N] views, mask of the elements a launch may write)"""
    written = np.zeros(out.size, bool)
    views = []
    for g in range(c["groups"]):
        blk = slice(g * c["strideC"], g * c["strideC"] + c["M"] * c["ldc"])
        views.append(out[blk].reshape(c["M"], c["ldc"])[:, :c["N"]])
        written[blk].reshape(c["M"], c["ldc"])[:, :c["N"]] = True
    return views, written


def singles(rt, c, cfg, flag=None, X=None, **over):
    """The groups of case c one launch each (groups = 1, offset pointers), all into one sentinel-filled buffer."""
    out = new_out(c)
    used = [launch(rt, c, cfg, out, g0=g, groups=1, flag=flag, X=X, **over) for g in range(c["groups"])]
    return out.cpu().numpy(), used


def e32_of(rt, c):
    """err_f32 of the bars: configuration 16 (the 256x128 f32 tile) on the same data, per group."""
    if c["e32"] is None:
        out, used = singles(rt, c, 16)
        assert used == [16] * c["groups"]
        c["out32"] = group_views(c, out)[0]
        c["e32"] = [rel(v, r) for v, r in zip(c["out32"], c["refs"])]
    return c["e32"]


def held_to_bar(rt, c, used, err, e32):
    """The float64 bar of the family the launch ran on (tests/test_gpu_kernels.py): f32 tiles rel < 2e-6 (linear) / 3e-6
    (convolution); bf16- and fp16-pipe tiles as accurate as the f32 tile on the same data."""
    if used in PLANE_PIPES:
        assert err < 1e-6 and err <= 2.0 * e32 + 1e-7, (used, err, e32)
    else:
        assert err < (3e-6 if c["conv"] else 2e-6), (used, err)


def run_case(rt, cases, name, cfg, X_key=None, a_planes=0):
    """One grouped launch against its groups one at a time and against float64; returns (grouped views, single views)."""
    c = get_case(rt, cases, name)
    over = dict(a_planes=a_planes) if a_planes else {}
    X = c[X_key] if X_key else None
    flag = torch.zeros(4, device="cuda", dtype=torch.int32)
    A = new_out(c)
    usedA = launch(rt, c, cfg, A, flag=flag, X=X, **over)
    B, usedB = singles(rt, c, cfg, flag=flag, X=X, **over)
    A = A.cpu().numpy()
    e32 = e32_of(rt, c)
    for name_, buf in (("grouped", A), ("single", B)):
        views, written = group_views(c, buf)
        assert (buf[~written] == SENT).all(), f"{name_}: a store outside the M x N blocks"     # 3. sentinels
        assert np.isfinite(buf[written]).all(), name_
        if c["valid_np"] is not None:
            for v in views:
                assert not v[c["valid_np"] == 0].any(), f"{name_}: masked rows"
    vA, vB = group_views(c, A)[0], group_views(c, B)[0]
    if cfg >= 0:
        assert usedA == cfg and usedB == [cfg] * c["groups"], (usedA, usedB)
        # 1. the per-tile arithmetic and K order do not depend on blockIdx.z
        for g in range(c["groups"]):
            assert np.array_equal(vA[g].view(np.uint32), vB[g].view(np.uint32)), f"group {g} differs from its single launch"
    # 2. float64 bars: every single-group baseline; the grouped launch itself too (under a forced tile it is the same bits)
    for g in range(c["groups"]):
        held_to_bar(rt, c, usedB[g], rel(vB[g], c["refs"][g]), e32[g])
        held_to_bar(rt, c, usedA, rel(vA[g], c["refs"][g]), e32[g])
    assert int(flag[0].item()) == 0                                                           # 4. the range guard stays quiet
    return vA, vB


ALL_LINEAR = F32_CFGS + X6_CFGS + X3H_CFGS + [-1]


@pytest.mark.parametrize("shared", [False, True], ids=["x_per_group", "x_shared"])
@pytest.mark.parametrize("cfg", ALL_LINEAR)
def test_grouped_branches_linear(rt, cases, cfg, shared):
    """(a) G = 3 linear branches, M = 300, N = 160, K = 256 (M and N tails on every tile up to 256x128): weights "whole"-form for the
    fp16 pipe, bf16 planes a whole buffer apart, bias / residual (ldr = N + 4) / output (ldc = N + 4, 8 floats between groups) per
    group, one row mask, ReLU prologue; X per group and shared (strideX = 0)."""
    run_case(rt, cases, "a_shared" if shared else "a", cfg)


@pytest.mark.parametrize("shared", [False, True], ids=["x_per_group", "x_shared"])
@pytest.mark.parametrize("M", [33, 64])
def test_grouped_branches_weight_streaming_kernel(rt, cases, M, shared):
    """(a) on the plain weight-streaming kernel (configurations 87 / 88 name one kernel; 33 .. 64 rows run as 88)."""
    run_case(rt, cases, f"a{M}_shared" if shared else f"a{M}", SKINNY64)
    c = cases[f"a{M}_shared" if shared else f"a{M}"]
    assert launch(rt, c, 87, new_out(c)) == SKINNY64          # forcing 87 beyond 32 rows is the same kernel under its other name


@pytest.mark.parametrize("shared", [False, True], ids=["x_per_group", "x_shared"])
@pytest.mark.parametrize("cfg", [c for c in ALL_LINEAR if c not in KSPLIT])
def test_grouped_branches_convolution(rt, cases, cfg, shared):
    """(b) the same branches as a 5-tap convolution over gap-padded rows (lengths 37, 1, 64, 5), Cin = 64, N = 96."""
    run_case(rt, cases, "b_shared" if shared else "b", cfg)


@pytest.mark.parametrize("cfg", ROWMAP_CFGS + [-1])
def test_grouped_shared_weights_with_a_row_map(rt, cases, cfg):
    """(c) mel_context_rows: stride-4 convolution through rowbase, strideW = strideB = 0, X per group, M = 118 < Rx = 474."""
    run_case(rt, cases, "c", cfg)


@pytest.mark.parametrize("cfg", ALL_LINEAR)
def test_grouped_k_slices(rt, cases, cfg):
    """(d) split-K: four slices of K = 1024 (strideX = strideW = 256, ldx = ldw = 1024), M = 77, N = 128; fp16 pipe in the "slices"
    form (shared row scales).  The slabs summed left to right in f32 (what the consumer kernel does) meet the single-launch bar
    against the float64 product over the full K."""
    vA, _ = run_case(rt, cases, "d", cfg)
    c = cases["d"]
    total = lambda v: ((v[0] + v[1]) + v[2]) + v[3]
    e32_of(rt, c)
    if cfg in PLANE_PIPES:
        err, e32 = rel(total(vA), c["full"]), rel(total(c["out32"]), c["full"])
        assert err < 1e-6 and err <= 2.0 * e32 + 1e-7, (err, e32)
    else:
        assert rel(total(vA), c["full"]) < 2e-6


@pytest.mark.parametrize("cfg", X3H_CFGS)
def test_grouped_a_operand_as_planes(rt, cases, cfg):
    """(e) X handed over as fp16 planes (op_layernorm act + 100) with G = 3 groups, strideX = M * K: bit-identical to the same grouped
    launch on the f32 rows those planes encode."""
    vf, _ = run_case(rt, cases, "e", cfg)
    vp, _ = run_case(rt, cases, "e", cfg, X_key="X_planes", a_planes=1)
    for g in range(G):
        assert np.array_equal(vf[g].view(np.uint32), vp[g].view(np.uint32)), g


@pytest.mark.parametrize("cfg", X3H_CFGS)
def test_range_guard_sees_every_group(rt, cases, cfg):
    """The fp16 pipe's range guard with groups: 7e4 in X of group 2 alone raises the flag, 6e4 (inside the fp16 range) does not."""
    c = get_case(rt, cases, "a")
    for big, want in ((7e4, 1), (6e4, 0)):
        X = c["X"].clone()
        X[2 * c["strideX"] + 17 * c["ldx"] + 33] = big
        flag = torch.zeros(4, device="cuda", dtype=torch.int32)
        assert launch(rt, c, cfg, new_out(c), flag=flag, X=X) == cfg
        assert int(flag[0].item()) == want, big


# ---- rejections: gemm_route answers before anything is launched - the output keeps its sentinel

@pytest.mark.parametrize("cfg", WINDOW_CFGS)
def test_window_configurations_reject_groups(rt, cfg):
    """The window convolutions serve one group (win_eligible): forced with groups = 3 on a square convolution they would
    otherwise take, they answer an error and launch nothing.  The group count is the only reason: the same descriptor with
    groups = 1 runs on that configuration and is right."""
    Cc = {30: 32, 31: 64, 32: 128, 34: 32, 58: 64, 59: 128, 98: 32, 99: 64, 100: 128}[cfg]
    M, k = 64, 5
    rng = np.random.default_rng(cfg)
    Xn = rng.standard_normal((G, M, Cc)).astype(np.float32)
    Wn = (rng.standard_normal((G * Cc, k * Cc)) / math.sqrt(k * Cc)).astype(np.float32)
    X = dev(Xn.reshape(-1))
    wts = rt.GemmWeights(torch.from_numpy(Wn))
    out = torch.full((G * M * Cc,), float(SENT), device="cuda", dtype=torch.float32)
    kw = dict(M=M, N=Cc, Cin=Cc, ldx=Cc, Rx=M, ldw=k * Cc, ldc=Cc, strideX=M * Cc, strideW=Cc * k * Cc, strideC=M * Cc, taps=k,
              shift0=-2, force_cfg=cfg)
    with pytest.raises(rt.NativeError, match="invalid argument"):
        rt.op_gemm_grouped(X, wts, out, groups=G, **kw)
    assert (out == float(SENT)).all()
    assert rt.op_gemm_grouped(X, wts, out, groups=1, **kw) == cfg
    got = out.cpu().numpy()
    assert (got[M * Cc:] == SENT).all()
    assert rel(got[:M * Cc].reshape(M, Cc), conv_ref(Xn[0], Wn[:Cc], k, 1, -2, Cc)) < 3e-6


@pytest.mark.parametrize("cfg", X3H_CFGS)
def test_x3h_rejects_a_group_stride_off_the_blocks(rt, cases, cfg):
    """An fp16-pipe launch whose planes are not whole 128-byte blocks apart answers an error and launches nothing (the same launch
    with the stride the rule gives is test_grouped_branches_linear)."""
    c = get_case(rt, cases, "a")
    out = new_out(c)
    with pytest.raises(rt.NativeError, match="invalid argument"):
        launch(rt, c, cfg, out, wh_gstride=c["strideW"] * 4 + 64)
    assert (out == float(SENT)).all()


@pytest.mark.parametrize("cfg", X3H_CFGS)
def test_a_planes_reject_a_group_stride_off_the_blocks(rt, cases, cfg):
    """X as fp16 planes with groups that do not start on a 128-byte block: not supported, nothing launched (the same launch
    with strideX = M * K is test_grouped_a_operand_as_planes)."""
    c = get_case(rt, cases, "e")
    out = new_out(c)
    with pytest.raises(rt.NativeError, match="not supported"):
        launch(rt, c, cfg, out, X=c["X_planes"], a_planes=1, strideX=c["strideX"] - 24)      # (stays inside the buffer)
    assert (out == float(SENT)).all()


# ---- epilogue activations that only the stage tests ran (groups = 1, mt2_op_gemm)

TANH_CFGS = F32_CFGS + [-1]


@pytest.fixture(scope="module")
def tanh_case():
    rng = np.random.default_rng(61)
    M, Cin, k = 300, 32, 7
    X = rng.standard_normal((M, Cin)).astype(np.float32)
    W = (rng.standard_normal((1, k * Cin)) * (1.5 / math.sqrt(k * Cin * 0.5))).astype(np.float32)
    b = np.asarray([0.1], np.float32)
    pre = conv_ref(np.where(X >= 0, X, X * np.float32(0.01)), W, k, 1, -3, Cin) + b
    return dev(X), dev(W), dev(b), pre


@pytest.mark.parametrize("cfg", TANH_CFGS)
def test_epilogue_tanh_on_the_vocoder_output_shape(rt, tanh_case, cfg):
    """ACT_TANH as the vocoder's conv_post uses it: N = 1, ldc = 1, 7 taps of 32 channels, LeakyReLU(0.01) prologue, against float64
    tanh - on every general f32 tile and on the un-forced route.  The convolution bar (3e-6) holds as it is."""
    X, W, b, pre = tanh_case
    assert 0.5 < np.abs(pre).std() < 3.0                 # the pre-activations cover tanh's bend
    out = rt.op_gemm(X, W, b, shift0=-3, taps=7, Cin=32, pro_act=rt.ACT_LRELU, pro_slope=0.01, epi_act=rt.ACT_TANH, force_cfg=cfg)
    assert out.shape == (300, 1)
    assert rel(out.cpu().numpy(), np.tanh(pre)) < 3e-6


@pytest.fixture(scope="module")
def logclamp_case():
    rng = np.random.default_rng(71)
    M, N, K, clip = 300, 80, 64, 1e-5
    X = (np.abs(rng.standard_normal((M, K))) * 1e-5 * np.exp(rng.uniform(-3, 3, (M, 1)))).astype(np.float32)      # magnitudes
    W = (rng.random((N, K)) * (rng.random((N, K)) < 0.3) / 8).astype(np.float32)                                # a sparse non-negative bank
    pre = X.astype(np.float64) @ W.astype(np.float64).T
    return dev(X), dev(W), pre, clip


@pytest.mark.parametrize("cfg", F32_CFGS + [-1])
def test_epilogue_logclamp_on_the_mel_front_end_shape(rt, logclamp_case, cfg):
    """ACT_LOGCLAMP as the mel front end uses it: no prologue, pro_slope = 1e-5 is the CLIP value, against log(max(v, clip)) in
    float64, with both sides of the clip exercised.  The convolution bar (3e-6) holds as it is."""
    X, W, pre, clip = logclamp_case
    below = float((pre < clip).mean())
    assert 0.1 < below < 0.9, below
    out = rt.op_gemm(X, W, pro_act=rt.ACT_NONE, pro_slope=clip, epi_act=rt.ACT_LOGCLAMP, force_cfg=cfg).cpu().numpy()
    clipped = out[pre < 0.5 * clip]                      # well below the clip: ONE value, log(clip)
    assert clipped.size and (clipped == clipped.flat[0]).all() and abs(float(clipped.flat[0]) - math.log(clip)) < 1e-5
    assert rel(out, np.log(np.maximum(pre, clip))) < 3e-6
