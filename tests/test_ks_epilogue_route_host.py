"""Which finish an x3h K-split launch takes is decided by gemm_route alone (no GPU needed): mt2_gemm_route_ex reports GemmRoute::ks_epi4
for the dense launch of mt2_gemm_route with the rows of C and R optionally further apart and the option ks_epi4 as given."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HIP_NOT_SUPPORTED = 801
OP_W3, OP_WH, OP_STAT, OP_LNSTAT, OP_R, OP_APLANES, OP_CPLANES, MIS_X, MIS_C = 1, 2, 8, 16, 32, 128, 256, 512, 1024
FULL = OP_W3 | OP_WH
KS = {95: 4, 96: 2, 97: 8}


def test_route_reports_the_16_byte_finish_for_aligned_k_split_launches_only():
    from megatts2_amd.runtime import op_gemm_route, op_gemm_route_ex
    for cfg, ks in KS.items():
        K = 32 * ks * 3
        for M in (1, 33, 100, 864):
            for ops in (FULL, FULL | OP_R, FULL | OP_STAT | OP_R, FULL | OP_APLANES):
                r = op_gemm_route_ex(M, 768, K, operands=ops, force_cfg=cfg)
                assert r[:2] == (0, cfg) and r[5] == 1, (cfg, M, ops, r)
                assert r[:5] == op_gemm_route(M, 768, K, operands=ops, force_cfg=cfg)         # everything else is the launch it always was
                off = op_gemm_route_ex(M, 768, K, operands=ops, force_cfg=cfg, ks_epi4=0)
                assert off[:5] == r[:5] and off[5] == 0
        assert op_gemm_route_ex(100, 768, 64 * ks, pro_act=5, operands=FULL | OP_LNSTAT, force_cfg=cfg)[5] == 1      # pair-fed LayerNorm
        # columns or rows not in fours, a base off 16 bytes: the dword finish of the same tile
        assert op_gemm_route_ex(100, 66, K, operands=FULL, force_cfg=cfg)[:2] == (0, cfg)
        assert op_gemm_route_ex(100, 66, K, operands=FULL, force_cfg=cfg)[5] == 0
        assert op_gemm_route_ex(100, 768, K, operands=FULL, force_cfg=cfg, ld_pad=2)[5] == 0
        assert op_gemm_route_ex(100, 768, K, operands=FULL, force_cfg=cfg, ld_pad=4)[5] == 1
        assert op_gemm_route_ex(100, 768, K, operands=FULL, force_cfg=cfg, misaligned=MIS_C)[5] == 0
        assert op_gemm_route_ex(100, 768, K, operands=FULL | OP_R, force_cfg=cfg, misaligned=OP_R)[5] == 0
        assert op_gemm_route_ex(100, 768, K, operands=FULL, force_cfg=cfg, misaligned=MIS_X)[5] == 1          # X is not an operand of the finish
        # grouped launches (groups M x ldc floats apart) qualify like single ones
        assert op_gemm_route_ex(99, 68, K, groups=3, operands=FULL, force_cfg=cfg)[5] == 1
        assert op_gemm_route_ex(99, 68, K, groups=3, operands=FULL, force_cfg=cfg, ld_pad=2)[5] == 0
        # C as fp16 planes stays the loader tile's alone, whatever the option says
        for opt in (0, 1):
            assert op_gemm_route_ex(864, 768, K, operands=FULL | OP_CPLANES, force_cfg=cfg, ks_epi4=opt)[0] == HIP_NOT_SUPPORTED
    # other kernels never report it: the x3h loader tile, the x6 K-split tile, an f32 tile, the <= 64-row kernels, a rejected launch
    for cfg in (103, 85, 16, 12):
        assert op_gemm_route_ex(864, 768, 768, operands=FULL, force_cfg=cfg)[5] == 0
    assert op_gemm_route_ex(32, 768, 768, operands=FULL | 4)[5] == 0
    assert op_gemm_route_ex(864, 768, 776, operands=FULL, force_cfg=96)[5] == 0
    # the automatic choice for an AR-step shape lands on a K-split tile and takes the finish
    r = op_gemm_route_ex(560, 1024, 768, operands=FULL)
    assert r[1] in KS and r[5] == 1, r
