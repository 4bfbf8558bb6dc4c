// Stationary-noise suppression for prompt audio (gfx950): a per-bin quantile noise floor (quantile-based noise estimation, Stahl, Fischer
// and Bippus 2000) and a spectral gate, between the two STFT GEMMs the library already has.  No reference counterpart.  Parity with any
// outside denoiser (noisereduce, RNNoise, Audacity) is unpinned, and so is audible quality on real speech; the rule is our own, stated in
// include/megatts2_hip.h and restated in tests/denoise_ref.py.  In short, for one utterance of T frames, F bins, Fp = F rounded up to 4:
//
//   P[t, f]  = fmaf(im, im, re re)                                                  f32
//   q[f]     = the value of rank k = ((T - 1) percentile + 50) / 100 among P[0 .. T, f], selected exactly;  Nf[f] = q[f] c
//   g0[t, f] = P > 0 ? max(g_min, (P - beta Nf[f]) / P) : g_min
//   g1[t, f] = mean of g0[t, f'] over the existing f' in [f - bf, f + bf];  g[t, f] = mean of g1[t', f] over the existing t' in
//              [t - bt, t + bt];  f32 sums in ascending order, one division by the count
//   S'[t, f] = g S[t, f], real and imaginary part each one product
//
// Four kernels:
//   dn_power_kernel     P, a cell a thread
//   dn_select_kernel    grid (tiles of 16 adjacent bins, B), 1024 threads: 64 rows by 16 bins a step, so every row read is one 64-byte
//                       segment.  P >= +0, so its bit pattern orders as an unsigned integer: a radix select, most significant byte
//                       first, four passes, a 256-entry histogram per bin in LDS (integer atomics; the row stride 257 keeps the 16
//                       histograms on different banks where the bins share a digit, as they do in the exponent byte), and per pass one
//                       wave per bin finds the digit by the shuffle scan of ebu.hip's range_select.  Order-free: no sum.  The column
//                       tile is NOT staged in LDS: P of a 30 s prompt is under 4 MB, passes two to four hit the L2, and a staged tile
//                       would hold 750 frames at most - a second kernel for the short case alone.
//   dn_gain_kernel      grid (tiles of 64 bins, tiles of 16 frames, B), 256 threads: g0 of the tile and its halo (at most 8 cells on
//                       every side) into LDS, g1 into LDS, then g, the optional gain output and the gated spectrum - steps 4 to 6 in one
//                       pass over P and one over the spectrum.  On request the tile's sums of P and g^2 P and its count of floored
//                       cells, in double: a thread adds its own cells in ascending order, the 256 partial sums meet in a fixed tree.
//   dn_figures_kernel   a workgroup per utterance: the tile sums and Nf in a fixed order -> MT2_DENOISE_FIELDS doubles
// No atomics on floating point; no sum is split across lanes in a way that changes its order; every order depends on the cell's index
// in its utterance alone, so a ragged batch is bit-identical to its utterances alone.  A non-finite sample cannot fault: a NaN power
// orders last in the select and takes the g_min branch of the gain.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <float.h>
#include <math.h>

namespace mt2 {

namespace {
constexpr int kThreads = 256, kSelThreads = 1024, kSelRows = kSelThreads / kDnSelBins, kHistLd = 257;
constexpr int kG0Ld = kDnTileF + 2 * kDnMaxSmooth, kTileRows = kDnTileT + 2 * kDnMaxSmooth;
static_assert(kSelThreads / 64 == kDnSelBins, "one wave per bin scans its histogram");

// One operation each, never contracted: hipcc's __fmul_rn / __fsub_rn / __dmul_rn / __dadd_rn are plain operators, and a difference or
// a sum with a product would become one fma (a single rounding where the rule has two) - the lesson of f0.hip.
__device__ __forceinline__ float dn_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float dn_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ float dn_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double dn_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double dn_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
}  // namespace

float denoise_factor(int percentile) { return (float)(1.0 / -log(1.0 - (double)percentile / 100.0)); }

__global__ __launch_bounds__(kThreads) void dn_power_kernel(DenoiseP p) {
    const int b = blockIdx.y, T = p.T[b];
    const long long total = (long long)T * p.Fp, base = (long long)p.row0[b];
    for (long long i = (long long)blockIdx.x * kThreads + threadIdx.x; i < total; i += (long long)gridDim.x * kThreads) {
        const int t = (int)(i / p.Fp), f = (int)(i % p.Fp);
        float v = 0.0f;
        if (f < p.F) {
            const float* __restrict__ row = p.spec + (base + t) * p.lds;
            const float re = row[f], im = row[p.F + f];
            v = fmaf(im, im, dn_mul(re, re));
        }
        p.P[(base + t) * p.Fp + f] = v;
    }
}

__global__ __launch_bounds__(kSelThreads) void dn_select_kernel(DenoiseP p) {
    __shared__ unsigned hist[kDnSelBins * kHistLd];
    __shared__ unsigned prefix_s[kDnSelBins], rank_s[kDnSelBins];
    const int b = blockIdx.y, f0 = blockIdx.x * kDnSelBins, tid = threadIdx.x, fb = tid & (kDnSelBins - 1), tr = tid / kDnSelBins;
    const int T = p.T[b], f = f0 + fb, w = tid >> 6, lane = tid & 63;
    const bool live = f < p.F;
    const float* __restrict__ col = p.P + (long long)p.row0[b] * p.Fp + (live ? f : 0);
    if (tid < kDnSelBins) {
        prefix_s[tid] = 0u;
        rank_s[tid] = (unsigned)((((long long)T - 1) * p.percentile + 50) / 100);
    }
    for (int shift = 24; shift >= 0; shift -= 8) {
        for (int i = tid; i < kDnSelBins * kHistLd; i += kSelThreads) hist[i] = 0u;
        __syncthreads();
        const unsigned mask = shift == 24 ? 0u : ~0u << (shift + 8), pre = prefix_s[fb];
        if (live) {
#pragma unroll 4
            for (int t = tr; t < T; t += kSelRows) {
                const unsigned key = __float_as_uint(col[(long long)t * p.Fp]);
                if ((key & mask) == pre) atomicAdd(&hist[fb * kHistLd + ((key >> shift) & 255u)], 1u);
            }
        }
        __syncthreads();
        {   // wave w, bin w: four entries a lane, a prefix sum by shuffles; the one lane whose entries hold the rank moves on
            const unsigned* h = hist + w * kHistLd;
            const unsigned rank = rank_s[w], h0 = h[4 * lane], h1 = h[4 * lane + 1], h2 = h[4 * lane + 2], h3 = h[4 * lane + 3];
            const unsigned own = (h0 + h1) + (h2 + h3);
            unsigned inc = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = __shfl_up(inc, d);
                if (lane >= d) inc += v;
            }
            const unsigned exc = inc - own;
            if (rank >= exc && rank < inc) {
                unsigned r = rank - exc, d = 4u * lane;
                if (r >= h0) { r -= h0; ++d; if (r >= h1) { r -= h1; ++d; if (r >= h2) { r -= h2; ++d; } } }
                prefix_s[w] |= d << shift;
                rank_s[w] = r;
            }
        }
        __syncthreads();
    }
    float* __restrict__ out = p.floor_out + (long long)b * p.Fp;
    if (tid < kDnSelBins && f0 + tid < p.F) out[f0 + tid] = dn_mul(__uint_as_float(prefix_s[tid]), p.c);
    if (blockIdx.x == 0 && tid < p.Fp - p.F) out[p.F + tid] = 0.0f;
}

__global__ __launch_bounds__(kThreads) void dn_gain_kernel(DenoiseP p) {
    __shared__ float g0s[kTileRows * kG0Ld];
    __shared__ float g1s[kTileRows * kDnTileF];
    __shared__ double red[kThreads];
    const int b = blockIdx.z, T = p.T[b], t0 = blockIdx.y * kDnTileT, f0 = blockIdx.x * kDnTileF, tid = threadIdx.x;
    if (t0 >= T) return;                                                      // uniform over the workgroup
    const int F = p.F, Fp = p.Fp, bf = p.bf, bt = p.bt, W0 = kDnTileF + 2 * bf, H = kDnTileT + 2 * bt;
    const long long base = (long long)p.row0[b];
    const float* __restrict__ P = p.P + base * Fp;
    const float* __restrict__ nf = p.floor + (long long)b * Fp;
    const float beta = p.beta, gmin = p.gmin;
    double sP = 0.0, sG = 0.0;
    int nfl = 0;
    for (int i = tid; i < H * W0; i += kThreads) {                             // step 4 on the tile and its halo
        const int tt = i / W0, ff = i - tt * W0, t = t0 - bt + tt, f = f0 - bf + ff;
        float g = 0.0f;
        if (t >= 0 && t < T && f >= 0 && f < F) {
            const float pw = P[(long long)t * Fp + f];
            g = pw > 0.0f ? fmaxf(gmin, __fdiv_rn(dn_sub(pw, dn_mul(beta, nf[f])), pw)) : gmin;
            if (tt >= bt && tt < bt + kDnTileT && ff >= bf && ff < bf + kDnTileF) {
                sP = dn_add(sP, (double)pw);
                nfl += g == gmin ? 1 : 0;
            }
        }
        g0s[tt * kG0Ld + ff] = g;
    }
    __syncthreads();
    for (int i = tid; i < H * kDnTileF; i += kThreads) {                       // step 5 along the bins
        const int tt = i / kDnTileF, fj = i - tt * kDnTileF, t = t0 - bt + tt, f = f0 + fj;
        float g = 0.0f;
        if (t >= 0 && t < T && f < F) {
            const int lo = max(0, f - bf), hi = min(F - 1, f + bf);
            float s = 0.0f;
            for (int q = lo; q <= hi; ++q) s = dn_add(s, g0s[tt * kG0Ld + (q - f0 + bf)]);
            g = __fdiv_rn(s, (float)(hi - lo + 1));
        }
        g1s[tt * kDnTileF + fj] = g;
    }
    __syncthreads();
    for (int i = tid; i < kDnTileT * kDnTileF; i += kThreads) {                // step 5 along the frames, step 6
        const int tj = i / kDnTileF, fj = i - tj * kDnTileF, t = t0 + tj, f = f0 + fj;
        if (t < T && f < F) {
            const int lo = max(0, t - bt), hi = min(T - 1, t + bt);
            float s = 0.0f;
            for (int q = lo; q <= hi; ++q) s = dn_add(s, g1s[(q - t0 + bt) * kDnTileF + fj]);
            const float g = __fdiv_rn(s, (float)(hi - lo + 1));
            if (p.gain_out) p.gain_out[((long long)b * p.gain_T + t) * Fp + f] = g;
            if (p.spec_out) {
                const float* src = p.spec + (base + t) * p.lds;                // dst may be src: a cell reads and writes itself alone
                float* dst = p.spec_out + (base + t) * p.lds;
                const float re = src[f], im = src[F + f];
                dst[f] = dn_mul(g, re);
                dst[F + f] = dn_mul(g, im);
            }
            if (p.part) sG = dn_add(sG, dn_mul(dn_mul((double)g, (double)g), (double)P[(long long)t * Fp + f]));
        }
    }
    if (!p.part) return;
    const double tP = block_tree_sum<kThreads>(red, sP), tG = block_tree_sum<kThreads>(red, sG);
    const double tN = block_tree_sum<kThreads>(red, (double)nfl);             // counts below 2^53 are exact in the tree
    if (tid == 0) {
        double* __restrict__ o = p.part + (((long long)b * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * 3;
        o[0] = tP; o[1] = tG; o[2] = tN;
    }
}

// the tiles of utterance b are the first ceil(T / 16) * tiles_f entries of its part of p.part: thread t takes the tiles t, t + 256, ...
__global__ __launch_bounds__(kThreads) void dn_figures_kernel(DenoiseP p) {
    __shared__ double red[kThreads];
    const int b = blockIdx.x, T = p.T[b], tid = threadIdx.x;
    const int ntf = (p.F + kDnTileF - 1) / kDnTileF, ntt_cap = (p.T_cap + kDnTileT - 1) / kDnTileT, n = ((T + kDnTileT - 1) / kDnTileT) * ntf;
    const double* __restrict__ part = p.part + (long long)b * ntt_cap * ntf * 3;
    const float* __restrict__ nf = p.floor + (long long)b * p.Fp;
    double sP = 0.0, sG = 0.0, sN = 0.0, sF = 0.0;
    for (int i = tid; i < n; i += kThreads) {
        sP = dn_add(sP, part[3 * i]);
        sG = dn_add(sG, part[3 * i + 1]);
        sN = dn_add(sN, part[3 * i + 2]);
    }
    for (int f = tid; f < p.F; f += kThreads) sF = dn_add(sF, (double)nf[f]);
    sP = block_tree_sum<kThreads>(red, sP);
    sG = block_tree_sum<kThreads>(red, sG);
    sN = block_tree_sum<kThreads>(red, sN);
    sF = block_tree_sum<kThreads>(red, sF);
    if (tid != 0) return;
    double* __restrict__ o = p.fig + (long long)b * MT2_DENOISE_FIELDS;
    const double mean = sP / (double)T;
    o[0] = 10.0 * log10(sF);
    o[1] = 10.0 * log10(fmax(mean - sF, DBL_MIN) / sF);
    o[2] = sN / ((double)T * (double)p.F);
    o[3] = 10.0 * log10(sG / sP);
    o[4] = (double)T;
    o[5] = (double)((((long long)T - 1) * p.percentile + 50) / 100);
    o[6] = mean;
    o[7] = sF;
}

namespace {
bool dn_rows_ok(const DenoiseP& p) {
    return p.B >= 1 && p.B <= 65535 && p.F >= 1 && p.Fp >= p.F && p.Fp - p.F < 4 && p.T_cap >= 1 && p.T_cap <= MT2_DENOISE_MAX_FRAMES &&
           p.row0 != nullptr && p.T != nullptr && p.P != nullptr;
}
}  // namespace

hipError_t launch_denoise_power(const DenoiseP& p, hipStream_t s) {
    if (!dn_rows_ok(p) || p.spec == nullptr || p.lds < 2 * p.F) return hipErrorInvalidValue;
    const long long g = ((long long)p.T_cap * p.Fp + kThreads - 1) / kThreads;
    hipLaunchKernelGGL(dn_power_kernel, dim3((unsigned)g, p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_denoise_select(const DenoiseP& p, hipStream_t s) {
    if (!dn_rows_ok(p) || p.floor_out == nullptr || p.percentile < 1 || p.percentile > 99) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_select_kernel, dim3((p.F + kDnSelBins - 1) / kDnSelBins, p.B), dim3(kSelThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_denoise_gain(const DenoiseP& p, hipStream_t s) {
    if (!dn_rows_ok(p) || p.floor == nullptr || p.bf < 0 || p.bf > kDnMaxSmooth || p.bt < 0 || p.bt > kDnMaxSmooth ||
        (p.spec_out && (p.spec == nullptr || p.lds < 2 * p.F)) || (p.gain_out && p.gain_T < p.T_cap) || (!p.spec_out && !p.gain_out && !p.part))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_gain_kernel, dim3((p.F + kDnTileF - 1) / kDnTileF, (p.T_cap + kDnTileT - 1) / kDnTileT, p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_denoise_figures(const DenoiseP& p, hipStream_t s) {
    if (!dn_rows_ok(p) || p.floor == nullptr || p.part == nullptr || p.fig == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dn_figures_kernel, dim3(p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
