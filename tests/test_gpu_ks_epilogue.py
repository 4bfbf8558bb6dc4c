"""Kernel-level parity (GPU) of the two finishes of the x3h K-split tiles (gemm_x3h_ks_kernel, tiles 95 / 96 / 97): the row-major finish
with 16-byte loads and stores (option ks_epi4 = 1, where gemm_route finds the layout fit) against the dword finish (ks_epi4 = 0) of the
same kernel source.  Same sums in the same order, so C and the row-statistics pairs are compared BIT FOR BIT, over the whole output
buffer (rows and columns beyond M x N included: nothing outside [M, N] of any group changes).  Launches go through mt2_op_gemm_grouped
(every operand and stride explicit, the option per launch) and, for the pair statistics, mt2_op_gemm_x3h_ln (configuration + 8000 = the
dword finish).  C as fp16 planes (GemmP::c_planes) is not a case: gemm_route refuses it on the K-split tiles under either option
(tests/test_cpu_host.py holds that answer)."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

KS = {95: 4, 96: 2, 97: 8}                              # x3hks32x64 k4, x3hks64x64 k2, x3hks32x32 k8
BM = {95: 32, 96: 64, 97: 32}
MS = [1, 31, 32, 33, 65, 100]
NS = [64, 68, 100, 132]
SENT = -777.25
OP_W3, OP_WH, OP_STAT, OP_LNSTAT, OP_R, OP_CPLANES, MIS_C = 1, 2, 8, 16, 32, 256, 1024


@pytest.fixture(scope="module")
def rt():
    from megatts2_amd import runtime
    runtime.device_check()
    return runtime


def wide(rng, shape, decades=2):
    return (rng.standard_normal(shape) * np.exp(rng.uniform(-decades, decades, shape))).astype(np.float32)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def same_bits(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def both(rt, cfg, X, wts, pre, want=(1, 0), **kw):
    """The launch with ks_epi4 = 1 and 0, each into its own copy of `pre` (the sentinel image: for a residual in place, the residual) ->
    (out1, out0); the route's answers are asserted: the forced tile, and the finish `want` = (with the option, without)."""
    outs = []
    inplace = kw.pop("inplace", False)
    for opt, fin in zip((1, 0), want):
        out = pre.clone()
        if inplace:
            kw["R"] = out
        used, epi4 = rt.op_gemm_grouped(X, wts, out, force_cfg=cfg, ks_epi4=opt, want_epi4=True, **kw)
        assert (used, epi4) == (cfg, fin), (used, epi4, cfg, opt)
        outs.append(out)
    return outs


def untouched_outside(out, pre, M, N, ldc, groups=1, strideC=0):
    """nothing outside [M, N] of any group differs from the image the buffer started as"""
    mask = torch.ones_like(out, dtype=torch.bool)
    for g in range(groups):
        mask[g * strideC:g * strideC + M * ldc].view(M, ldc)[:, :N] = False
    return same_bits(out[mask], pre[mask])


@pytest.mark.parametrize("kmul", [1, 2, 5])
@pytest.mark.parametrize("cfg", [95, 96, 97])
def test_c_bit_identical_to_the_dword_finish(rt, cfg, kmul):
    """Every M x N of the set on one tile and one K = 32 KS kmul: no operands; bias + residual IN PLACE + row mask with a whole tile of
    masked rows; bias + residual from a strided source with the A rows gathered (a_mul = 3, shift0 = 2: the last layer's form); ReLU
    epilogue with out_scale != 1; the A operand as fp16 planes (PRO_APL); and, at kmul = 1, three split-K slabs (groups = 3, strideC)."""
    rng = np.random.default_rng(1000 * cfg + kmul)
    K, Mx, Nx = 32 * KS[cfg] * kmul, max(MS), max(NS)
    X = dev(wide(rng, (3 * Mx, K)))
    gam, bet = dev((1 + 0.2 * rng.standard_normal(64)).astype(np.float32)), dev((0.1 * rng.standard_normal(64)).astype(np.float32))
    # some A operand in the planes format: LayerNorm over runs of 64 columns written as fp16 planes (128-byte blocks per 32 columns: the
    # layout does not depend on the row length)
    Xpl = rt.op_layernorm(X.view(-1, 64), gam, bet, act=rt.ACT_NONE + 100).view(3 * Mx, K)
    wts = rt.GemmWeights(torch.from_numpy(wide(rng, (Nx, K)) / math.sqrt(K)))
    bias = dev(rng.standard_normal(Nx).astype(np.float32))
    if kmul == 1:
        X3 = dev(wide(rng, (Mx, 3 * K)))
        wts3 = rt.GemmWeights(torch.from_numpy(wide(rng, (Nx, 3 * K)) / math.sqrt(K)))
    for M in MS:
        valid = (rng.random(M) > 0.2).astype(np.int32)
        if M > BM[cfg]:
            valid[:BM[cfg]] = 0                                         # a tile whose rows are all masked
        valid = dev(valid)
        for N in NS:
            ldc, Mp = N + 4, M + 3                                      # ld > N, M padded
            sent = torch.full((Mp * ldc,), SENT, device="cuda", dtype=torch.float32)
            resid = dev(rng.standard_normal(Mp * ldc).astype(np.float32))
            ldr0 = N + 8
            rsrc = dev(rng.standard_normal(3 * M * ldr0).astype(np.float32))
            base = dict(M=M, N=N, Cin=K, ldx=K, Rx=M, ldw=K, ldc=ldc)
            runs = [
                ("plain", X, sent, dict(base)),
                ("bias + residual in place + mask", X, resid, dict(base, bias=bias, inplace=True, ldr=ldc, valid=valid)),
                ("strided residual, gathered rows", X, sent, dict(base, Rx=3 * M, a_mul=3, shift0=2, bias=bias, R=rsrc[2 * ldr0:], ldr=3 * ldr0)),
                ("relu epilogue, out_scale", X, sent, dict(base, bias=bias, valid=valid, epi_act=rt.ACT_RELU, out_scale=0.37)),
                ("A as planes", Xpl, sent, dict(base, a_planes=1)),
            ]
            for name, Xop, pre, kw in runs:
                a, b = both(rt, cfg, Xop, wts, pre, **kw)
                tag = (name, M, N)
                assert same_bits(a, b), tag
                assert untouched_outside(a, pre, M, N, ldc), tag
                body = a[:M * ldc].view(M, ldc)[:, :N]
                assert torch.isfinite(body).all() and not same_bits(body, pre[:M * ldc].view(M, ldc)[:, :N]), tag
                if "valid" in kw:
                    assert not body[valid == 0].any(), tag
            if kmul == 1:
                sC = Mp * ldc
                pre = torch.full((3 * sC,), SENT, device="cuda", dtype=torch.float32)
                a, b = both(rt, cfg, X3, wts3, pre, M=M, N=N, Cin=K, ldx=3 * K, Rx=M, ldw=3 * K, ldc=ldc, groups=3, strideX=K, strideW=K,
                            strideC=sC)
                assert same_bits(a, b), ("slabs", M, N)
                assert untouched_outside(a, pre, M, N, ldc, groups=3, strideC=sC), ("slabs", M, N)


@pytest.mark.parametrize("cfg", [95, 96, 97])
def test_pairs_and_pair_fed_layernorm_bit_identical(rt, cfg):
    """stat_out (row pairs per 32-column wave tile) and PRO_LNX (the pair-fed algebraic LayerNorm), with and without each other: C and the
    pairs of the 16-byte finish equal the dword finish's bit for bit; the route takes the 16-byte finish for these launches."""
    rng = np.random.default_rng(cfg)
    K = 32 * KS[cfg] * 2
    lw = 32
    full = OP_W3 | OP_WH
    for N in (64, 128):
        W = dev(wide(rng, (N, K)) / math.sqrt(K))
        bias = dev(rng.standard_normal(N).astype(np.float32))
        g, b = dev(rng.standard_normal(K).astype(np.float32)), dev(rng.standard_normal(K).astype(np.float32))
        for M in MS:
            assert rt.op_gemm_route_ex(M, N, K, operands=full | OP_STAT | OP_R, force_cfg=cfg)[5] == 1
            assert rt.op_gemm_route_ex(M, N, K, pro_act=5, operands=full | OP_STAT | OP_LNSTAT, force_cfg=cfg)[5] == 1
            x = dev((rng.standard_normal((M, K)) * 2.0 + 0.5).astype(np.float32))
            R = dev(rng.standard_normal((M, N)).astype(np.float32))
            t = x.double().view(M, K // lw, lw)
            mean = t.mean(2)
            pairs = torch.stack([mean, ((t - mean[:, :, None]) ** 2).sum(2)], 2).float().contiguous()
            got = []
            for off in (0, 8000):
                c1, p1, w1 = rt.op_gemm_x6_ln(x, W, bias, R=R, force_cfg=cfg + off, want_stats=True, x3h=True)
                c2, p2, w2 = rt.op_gemm_x6_ln(x, W, bias, epi_act=rt.ACT_RELU, force_cfg=cfg + off, want_stats=True, x3h=True,
                                              ln=(g, b, pairs, lw))
                assert w1 == 32 and w2 == 32 and p1.shape == (M, N // 32, 2) and p2.shape == p1.shape
                got.append((c1, p1, c2, p2))
            for u, v in zip(*got):
                assert same_bits(u, v), (M, N)
            assert torch.isfinite(got[0][1]).all() and got[0][1][:, :, 1].min() >= 0


def test_fallback_layouts_keep_the_dword_finish(rt):
    """N = 66, ldc = N + 2 and a C base 4 bytes off: the route reports the dword finish (with the option on), and the launch gives the bits
    of the same launch with the option off."""
    rng = np.random.default_rng(7)
    full = OP_W3 | OP_WH
    for cfg in (95, 96, 97):
        K, M = 32 * KS[cfg] * 2, 65
        assert rt.op_gemm_route_ex(M, 68, K, operands=full, force_cfg=cfg)[5] == 1
        assert rt.op_gemm_route_ex(M, 68, K, operands=full, force_cfg=cfg, ks_epi4=0)[5] == 0
        assert rt.op_gemm_route_ex(M, 66, K, operands=full, force_cfg=cfg)[5] == 0
        assert rt.op_gemm_route_ex(M, 68, K, operands=full, force_cfg=cfg, ld_pad=2)[5] == 0
        assert rt.op_gemm_route_ex(M, 68, K, operands=full, force_cfg=cfg, misaligned=MIS_C)[5] == 0
        assert rt.op_gemm_route_ex(M, 68, K, operands=full | OP_R, force_cfg=cfg, misaligned=OP_R)[5] == 0
        X = dev(wide(rng, (M, K)))
        wts = rt.GemmWeights(torch.from_numpy(wide(rng, (68, K)) / math.sqrt(K)))
        bias = dev(rng.standard_normal(72).astype(np.float32))
        for N, ldc, off in ((66, 68, 0), (68, 70, 0), (68, 72, 1)):
            buf = torch.full(((M + 3) * ldc + 4,), SENT, device="cuda", dtype=torch.float32)
            resid = dev(rng.standard_normal(M * ldc + 4).astype(np.float32))
            outs = []
            for opt in (1, 0):
                out = buf.clone()
                used, epi4 = rt.op_gemm_grouped(X, wts, out[off:], M=M, N=N, Cin=K, ldx=K, Rx=M, ldw=K, ldc=ldc, bias=bias, R=resid[off:], ldr=ldc,
                                                force_cfg=cfg, ks_epi4=opt, want_epi4=True)
                assert (used, epi4) == (cfg, 0), (cfg, N, ldc, off, opt)
                outs.append(out)
            assert same_bits(outs[0], outs[1])
            assert untouched_outside(outs[0][off:], buf[off:], M, N, ldc)
            assert same_bits(outs[0][:off], buf[:off])


@pytest.mark.parametrize("cfg", [95, 96, 97])
def test_accuracy_against_float64(rt, cfg):
    """The 16-byte finish at the bar of the x3h kernel tests: as accurate as the f32 tile (configuration 16) on the same data."""
    rng = np.random.default_rng(50 + cfg)
    M, N, K = 100, 132, 32 * KS[cfg] * 5
    Xh, Wh = wide(rng, (M, K), 3), wide(rng, (N, K)) / math.sqrt(K)
    bh, Rh = rng.standard_normal(N).astype(np.float32), rng.standard_normal((M, N)).astype(np.float32)
    ref = Xh.astype(np.float64) @ Wh.astype(np.float64).T + bh + Rh
    X, wts, bias, R = dev(Xh), rt.GemmWeights(torch.from_numpy(Wh)), dev(bh), dev(Rh)
    kw = dict(M=M, N=N, Cin=K, ldx=K, Rx=M, ldw=K, ldc=N, bias=bias, R=R, ldr=N)
    out, o32 = torch.empty(M, N, device="cuda"), torch.empty(M, N, device="cuda")
    assert rt.op_gemm_grouped(X, wts, out, force_cfg=cfg, want_epi4=True, **kw) == (cfg, 1)
    assert rt.op_gemm_grouped(X, wts, o32, force_cfg=16, want_epi4=True, **kw) == (16, 0)
    rel = lambda a: float(np.linalg.norm(a.cpu().numpy().astype(np.float64) - ref) / np.linalg.norm(ref))
    err, e32 = rel(out), rel(o32)
    print(f"cfg {cfg}: err {err:.3e} err_f32 {e32:.3e}")
    assert err <= 2.0 * e32 + 1e-7, (err, e32)
