"""launch_gemm goes the way gemm_route says (GPU): for shapes of the recorded routing table (tests/gemm_routes.json's grid), the
configuration an un-forced mt2_bench_gemm launch reports is the one mt2_gemm_route names for the same launch."""
import ctypes

import pytest

pytestmark = pytest.mark.gpu

X3H_OFF = 32        # mt2_bench_gemm flag: the automatic choice without the fp16-pipe forms
# (M, N, K, taps, flags) -> the index the recorded table has for it
SHAPES = [
    (864, 4096, 1024, 1, 0, 103), (96, 768, 256, 1, 0, 95), (300, 768, 768, 1, 0, 96), (96, 768, 1024, 1, 0, 97),
    (2200, 32, 96, 3, 0, 98), (2200, 64, 192, 3, 0, 99), (2200, 128, 384, 3, 0, 100), (2200, 64, 704, 11, 0, 99),
    (32, 768, 768, 1, 0, 89), (64, 768, 768, 1, 0, 90), (33, 768, 96, 1, 0, 88), (1, 768, 100, 1, 0, 22),
    (4096, 2304, 256, 1, X3H_OFF, 51), (864, 4096, 1024, 1, X3H_OFF, 55), (96, 768, 256, 1, X3H_OFF, 84),
    (300, 768, 768, 1, X3H_OFF, 85), (96, 768, 1024, 1, X3H_OFF, 86), (2200, 32, 96, 3, X3H_OFF, 34),
    (2200, 64, 192, 3, X3H_OFF, 58), (2200, 128, 384, 3, X3H_OFF, 59),
    (300, 768, 100, 1, 0, 20), (300, 32, 256, 1, 0, 15), (4096, 768, 100, 1, 0, 12),
]


def test_unforced_launches_take_the_route_gemm_route_reports():
    from megatts2_amd import runtime as rt
    lib = rt.load_library()
    lib.mt2_gemm_config_name.restype = ctypes.c_char_p
    for M, N, K, taps, flags, want in SHAPES:
        tm = M <= 64 and taps == 1 and N % 16 == 0 and K % 64 == 0      # the operands mt2_bench_gemm attaches: W3, Wh, and Wtm where it can
        err, cfg, _, _, _ = rt.op_gemm_route(M, N, K, taps, operands=1 | 2 | (4 if tm else 0), x3h=0 if flags & X3H_OFF else 15)
        assert (err, cfg) == (0, want), (M, N, K, taps, flags, err, cfg)
        _, name = rt.bench_gemm(M, N, K, taps, force_cfg=-1, iters=1, flags=flags)
        assert name == lib.mt2_gemm_config_name(cfg).decode(), (M, N, K, taps, flags, name, cfg)
