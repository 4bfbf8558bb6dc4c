// The tile of the true-peak interpolator (the rule of ebu.hip), shared by true_peak_kernel (ebu.hip) and limiter_envelope_kernel
// (limiter.hip): kTpThreads threads, kTpTile consecutive samples of one utterance with a halo of Z in LDS beside the o x 24 table; a
// thread runs every phase of N consecutive positions: their windows are 23 + N words, read as seven aligned 16-byte vectors
// (consecutive lanes, consecutive vectors: no bank conflict), and a phase's 24 coefficients, one address for the whole wave, are
// read once for the N chains.  A kernel keeps its tile origin, its early returns and what it does with the values.
// The device code decided the form: written this way (the chains and their fabsf in phase(), the maxima in the kernels) hipcc keeps
// both kernels' scalar v_fmac_f32 chains, ds_read_b128 and resource blocks; see profiles/meter_refactor_ab.txt.
#pragma once
#include "../../include/megatts2_hip.h"

namespace mt2 {

constexpr int kZ = MT2_TP_ZERO_CROSSINGS, kTaps = MT2_TP_TAPS, kMaxOver = 24;
constexpr int kTpThreads = 256, kPer = 4, kTpTile = kTpThreads * kPer;
constexpr int kTpXsWords = kTpTile + 2 * kZ, kTpHsWords = kMaxOver * kTaps;      // the two LDS arrays, both aligned to 16 bytes
static_assert(kTaps == 2 * kZ && kPer == 4 && kTaps % 4 == 0 && kTpXsWords % 4 == 0, "true-peak geometry");

// xs[q] = x[first + q] (0 outside [0, L)), q in [0, kTpXsWords);  hs = the table's o rows;  the workgroup meets behind both
__device__ __forceinline__ void tp_tile_load(float* xs, float* hs, const float* __restrict__ x, long long first, int L,
                                             const float* __restrict__ table, int o) {
    for (int q = threadIdx.x; q < kTpXsWords; q += kTpThreads) {
        const long long s = first + q;
        xs[q] = s >= 0 && s < L ? x[s] : 0.0f;
    }
    for (int q = threadIdx.x; q < o * kTaps; q += kTpThreads) hs[q] = table[q];
    __syncthreads();
}
// d[0 .. W) = s[0 .. W) by 16-byte reads (s aligned, W a multiple of 4)
template <int W> __device__ __forceinline__ void tp_read(float (&d)[W], const float* s) {
#pragma unroll
    for (int k = 0; k < W; k += 4) {
        const float4 v4 = *reinterpret_cast<const float4*>(s + k);
        d[k] = v4.x; d[k + 1] = v4.y; d[k + 2] = v4.z; d[k + 3] = v4.w;
    }
}

// The windows of the N <= 5 consecutive positions whose first window is xs[q0 .. q0 + 2 Z), q0 a multiple of 4: position j's is
// w[j .. j + 2 Z).  |y| of its phase 0, the sample itself (0 in front of the signal), and of a filtered phase: one f32 fma chain a
// position, each in ascending k.
template <int N> struct TpWindows {
    static_assert(N >= 1 && N <= kPer + 1, "a thread's windows are seven vectors");
    float w[kTaps + kPer];
    __device__ __forceinline__ TpWindows(const float* xs, int q0) { tp_read(w, xs + q0); }
    __device__ __forceinline__ float sample(int j) const { return fabsf(w[j + kZ - 1]); }
    __device__ __forceinline__ void phase(const float* hs, int ph, float (&a)[N]) const {
        float h[kTaps], acc[N];
        tp_read(h, hs + ph * kTaps);
#pragma unroll
        for (int j = 0; j < N; ++j) acc[j] = 0.0f;
#pragma unroll
        for (int k = 0; k < kTaps; ++k)
#pragma unroll
            for (int j = 0; j < N; ++j) acc[j] = __fmaf_rn(h[k], w[k + j], acc[j]);      // each chain in ascending k
#pragma unroll
        for (int j = 0; j < N; ++j) a[j] = fabsf(acc[j]);
    }
};

}  // namespace mt2
