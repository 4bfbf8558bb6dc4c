// What the x3h WINDOW family (gemm_x3h.hip: conv_win_x3h_kernel, conv_pair_x3h_kernel, up_mrf_x3h_kernel) shares WITHOUT a change of
// its device code: the tile constants (WinGeom: the kernels' constexpr block, and ring size / thread count of the host tile rows),
// the range guard's flag line, and the host side of the routes.  (xcd_row_tile, the row-tile map, is in gemm_common.h.)
// The device pieces with control flow - window load, weight ring, planes pass, fragment pipeline - stay written out in each kernel:
// moved into shared inlined functions they compute the same values but compile to other code (block order, registers, scalar waits),
// and conv_win_x3h_kernel measured ~1 % slower that way; profiles/x3h_window_toolkit.txt has the experiments.
// A part of the gemm_x3h.hip unit: included there behind its constants, and nowhere else.
#pragma once
#ifndef MT2_BUFFER_LOADS
#error "x3h_window.h is a part of gemm_x3h.hip: include it there and nowhere else"
#endif

namespace mt2 {

// the constants every kernel of the family opens with, and their one static_assert
template <int QS_, int BM_, int BN_, int WGM_, int WGN_, int NST_, int NL_>
struct WinGeom {
    static constexpr int QS = QS_, BM = BM_, BN = BN_, WGM = WGM_, WGN = WGN_, NST = NST_, NL = NL_;
    static constexpr int NW = WGM * WGN;
    static constexpr int WTM = BM / WGM, WTN = BN / WGN;
    static constexpr int TM = WTM / 32, TN = WTN / 32;
    static constexpr int BPIECES = BN / 8;                // 1-KiB pieces of one weight chunk: 8 rows x 128 B ([hi | lo] blocks)
    static constexpr int B_IT = (BPIECES + NL - 1) / NL;  // pieces per loader wave (the NL loader waves issue the ring refill) and chunk
    static constexpr int STAGE_B = B_IT * NL * 1024;      // BYTES per ring stage (dummy slots included)
    static constexpr int NT = (NW + NL) * 64;
    static_assert(NL > 0 && WTM % 32 == 0 && WTN % 32 == 0 && NST >= 3 && (NST - 2) * B_IT < 64 && BN == 32 * QS, "config");
    static constexpr size_t ring_bytes() { return (size_t)NST * STAGE_B; }
};

// the range guard of a kernel: any lane of the wave converted a value of fp16's maximum or more -> the host repeats the call on x6.
// A macro, not a function: through a function the same line compiles to other branches in every kernel that has it.
#define MT2_X3H_GUARD_RAISE(p, amax, lane)                                                                                  \
    do {                                                                                                                    \
        if ((p).x3h_flag != nullptr && __builtin_amdgcn_ballot_w64((amax) >= kX3hMaxIn) != 0ull && (lane) == 0) atomicOr((p).x3h_flag, 1); \
    } while (0)

// ---- host side.  LDS of the window behind the ring: C / 32 slices of bm + span rows (padded to 8) of 32 f32
inline size_t win_lds_bytes(int C, int bm, int span) { return (size_t)(C / 32) * ((bm + span + 7) & ~7) * BK * sizeof(float); }
// What the routes of the fused kernels share.  A fused kernel is bit-identical to the launches it replaces only where those would run
// on the x3h window tiles ...
inline bool x3h_window_engine(const EngineOpts& o) { return o.win_conv && o.x6_conv && (o.x3h & 4) && o.force_cfg < 0 && !o.ldr64; }
// ... its loaders have the buffer form only and its row offsets are 32-bit: every operand stays below 2 GiB
inline bool win_below_2g(long long R, long long ldx, long long ldy, long long C, long long wh_ldb) {
    const long long two_g = 1ll << 31;
    return R * ldx * 4 < two_g && R * ldy * 4 < two_g && C * wh_ldb < two_g - 1;
}
// ... and it has the 16-byte-store epilogue only (the window kernel has a scalar-store form for operands off 16 bytes): w = the weight
// planes' addresses or-ed together, v = those of the f32 operands
inline bool win_aligned(long long ldx, long long ldy, long long wh_ldb, unsigned long long w, unsigned long long v) {
    return !((ldx | ldy) & 3) && !(wh_ldb & 127) && !(w & 127) && !(v & 15);
}

}  // namespace mt2
