// The tile configurations of the GEMM engine: what a row of the table holds, the public index of every live configuration, and
// the kernel units that define rows.  Each unit describes its own tiles exactly once, next to the kernels (gemm_f32.hip: the f32
// and bf16-pipe "x6" tiles; gemm_x3h.hip: the fp16-pipe "x3h" tiles); gemm_dispatch.hip puts the rows at their indices, adds the
// names of the retired ones, and routes launches.
#pragma once
#include "mt2_kernels.h"

namespace mt2 {

constexpr int BK = 32;      // K chunk (floats)
// GemmP::pro_act beyond the activations (Act): LayerNorm prologues
constexpr int PRO_LN = 3;   // LayerNorm of the A rows (the <= 64-row weight-streaming kernel only)
constexpr int PRO_LNA = 4;  // LayerNorm of the A rows, ALGEBRAIC form: statistics in the prologue, correction in the epilogue
constexpr int PRO_LNX = 5;  // ... ALGEBRAIC form on PAIR statistics written by the producer GEMM's epilogue (GemmP::ln_stat): no pass over K

// Which instantiation of a tile's kernel a launch runs: a slot of TileCfg::fn.  The host's own numbering - what a kernel takes as
// its template argument (an Act, PRO_LNX, PRO_APL) is the business of the unit that fills the slot.
enum GemmVariant : int {
    V_NONE, V_RELU, V_LRELU,    // prologue activation of the A operand (= Act)
    V_APLANES,                  // the A operand ARRIVES as fp16 planes (GemmP::a_planes; x3h loader / K-split tiles)
    V_LNX,                      // pair statistics: the pair-fed algebraic LayerNorm (pro_act == PRO_LNX) and / or the row-statistics
                                // epilogue (GemmP::stat_out) - the K loop of V_NONE
    kGemmVariants
};
static_assert((int)V_NONE == ACT_NONE && (int)V_RELU == ACT_RELU && (int)V_LRELU == ACT_LRELU, "the activation variants are indexed by Act");

enum GemmPipe : int { PIPE_F32, PIPE_X6, PIPE_X3H };   // f32 MFMA / bf16 pipe, 6 products (needs GemmP::W3) / fp16 pipe, 3 products (Wh, wh_inv)

// Public indices of the live configurations (tests, tools, bench.py and profiles/ address configurations by index; every other
// index below kNumCfgs is retired and keeps its name, gemm_dispatch.hip).
enum CfgIndex : int {
    CFG_64x64 = 3,
    CFG_DMA64x64_S3 = 12, CFG_DMA128x32_S4 = 15, CFG_DMA256x128_S3 = 16, CFG_DMA128x128_S4 = 17,
    CFG_DMA64x64_K2 = 18, CFG_DMA64x64_K4 = 20, CFG_DMA32x64_K4 = 22, CFG_DMA256x64_S3 = 23, CFG_DMA32x32_K8 = 28,
    CFG_WIN256x32 = 30, CFG_WIN256x64 = 31, CFG_WIN128x128 = 32,
    CFG_X6WIN256x32 = 34,
    CFG_X6LDR256x128 = 51, CFG_X6LDR128x128 = 55,
    CFG_X6WINL256x64 = 58, CFG_X6WINL128x128 = 59,
    CFG_X6KS32x64_K4 = 84, CFG_X6KS64x64_K2 = 85, CFG_X6KS32x32_K8 = 86,
    CFG_SKINNY32 = 87, CFG_SKINNY64 = 88, CFG_SKINNYTM32 = 89, CFG_SKINNYTM64 = 90,     // gemm_skinny.hip: names only
    CFG_X3HKS32x64_K4 = 95, CFG_X3HKS64x64_K2 = 96, CFG_X3HKS32x32_K8 = 97,
    CFG_X3HWIN256x32 = 98, CFG_X3HWIN256x64 = 99, CFG_X3HWIN128x128 = 100,
    CFG_X3HLDR128x128 = 103,
    kNumCfgs = 106
};

typedef void (*GemmKernel)(GemmP);
struct TileCfg {
    CfgIndex index;           // where the row sits in the table
    int bm, bn, threads;
    size_t lds;               // window configurations: the ring part only (the window depends on taps and dilation)
    const char* name;
    GemmKernel fn[kGemmVariants];   // by GemmVariant; nullptr: the tile has no such variant
    GemmPipe pipe = PIPE_F32;
    int win_qs = 0;           // > 0: window convolution for Cin = Cout = 32 * win_qs
    int x6_ks = 0;            // > 0: K-split tile of the x6 / x3h pipes: linear layers with K a multiple of 32 * x6_ks
    int stat_w = 0;           // > 0: the tile has the row-statistics epilogue (GemmP::stat_out: one pair per stat_w columns) and
                              // the pair-fed algebraic-LayerNorm form (pro_act == PRO_LNX)
    GemmKernel fn4[kGemmVariants] = {};   // x3h K-split tiles: the same kernels with the row-major 16-byte finish (GemmRoute::ks_epi4)
};
struct TileRows { const TileCfg* rows; int n; };
TileRows gemm_f32_tile_rows();      // gemm_f32.hip
TileRows gemm_x3h_tile_rows();      // gemm_x3h.hip

}  // namespace mt2
