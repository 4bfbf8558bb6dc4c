// Leading / trailing silence trimming of prompt audio (gfx950): what `librosa.effects.trim(y, top_db)` does behind
// `librosa.load` + `librosa.util.normalize` (reference models/megatts2.py:337, commented out there because its prompts are pre-cut;
// prepare_ds.py --trim_wav).  librosa is not reproduced bit for bit (parity unpinned); the rule is our own
// statement of what librosa documents for effects.trim with ref = np.max, centred frames and zero padding, frame 2048 / hop 512:
//
//   s[j] = sum of x[i]^2 over i in [512 j, 512 j + 512) and [0, L)                 (f32; 0 for j outside [0, ceil(L / 512)))
//   e[f] = ((s[f - 2] + s[f - 1]) + s[f]) + s[f + 1],  f < F = 1 + L / 512          (the window [512 f - 1024, 512 f + 1024))
//   E = max_f e[f],  c = (float)pow(10.0, -top_db / 10.0),  frame f kept iff e[f] > E * c     (one f32 product, no logarithm)
//   start = 512 * first kept frame,  end = min(L, 512 * (last kept frame + 1));  E < FLT_MIN (silence): start = 0, end = L
//   out[j] = x[start + j] for j < end - start, an exact copy
//
// A block sum has ONE order, fixed by the sample's index in its utterance: lane l of a wave owns the samples 4 l .. 4 l + 3 and
// 256 + 4 l .. 256 + 4 l + 3 of the block as one fma chain in that order, then the 64 lanes meet in a butterfly (xor 32, 16, ... 1).
// Neither the address, the batch slot nor L_max enters, so a ragged batch is bit-identical to its utterances alone, energies
// included.  A sample at or beyond L is a zero by its index, never a read.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <float.h>
#include <limits.h>
#include <math.h>

#include <algorithm>

namespace mt2 {

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kHop = MT2_TRIM_HOP;
constexpr int kTileBlocks = 16;                        // blocks of kHop samples per workgroup (4 per wave: 32 KiB of audio)
static_assert(kHop == 512 && MT2_TRIM_FRAME == 4 * kHop, "the lane layout of a block sum and the 4-block frame are written for 2048 / 512");
}  // namespace

int trim_frames(long long L) { return (int)(1 + L / kHop); }
float trim_factor(float top_db) { return (float)pow(10.0, -(double)top_db / 10.0); }

// four consecutive samples of one utterance from index i on: a 16-byte load where the address allows it and all four are real
__device__ __forceinline__ float4 load4_or_zero(const float* __restrict__ x, int i, int L) {
    if (i + 3 < L && (reinterpret_cast<uintptr_t>(x + i) & 15) == 0) return *reinterpret_cast<const float4*>(x + i);
    float4 v;
    v.x = i < L ? x[i] : 0.0f;
    v.y = i + 1 < L ? x[i + 1] : 0.0f;
    v.z = i + 2 < L ? x[i + 2] : 0.0f;
    v.w = i + 3 < L ? x[i + 3] : 0.0f;
    return v;
}

// s[b, j] for the blocks of one tile; wave w of the workgroup takes the tile's blocks w, w + 4, ...
__global__ __launch_bounds__(kThreads) void trim_block_sums_kernel(TrimP p) {
    const int b = blockIdx.y, L = p.len[b], lane = threadIdx.x & 63;
    const int nb = (L + kHop - 1) / kHop;
    const float* __restrict__ x = p.wav + (long long)b * p.L_max;
    float* __restrict__ s = p.sums + (long long)b * p.NB;
    for (int k = threadIdx.x >> 6; k < kTileBlocks; k += kWaves) {
        const int j = blockIdx.x * kTileBlocks + k;
        if (j >= nb) break;                                                 // wave-uniform
        const int i0 = j * kHop + 4 * lane;                                // < L + 512: no overflow for L < 2^31 - 1024 (checked by the caller)
        const float4 u = load4_or_zero(x, i0, L), v = load4_or_zero(x, i0 + 256, L);
        float a = u.x * u.x;
        a = fmaf(u.y, u.y, a); a = fmaf(u.z, u.z, a); a = fmaf(u.w, u.w, a);
        a = fmaf(v.x, v.x, a); a = fmaf(v.y, v.y, a); a = fmaf(v.z, v.z, a); a = fmaf(v.w, v.w, a);
#pragma unroll
        for (int d = 32; d > 0; d >>= 1) a += __shfl_xor(a, d);
        if (lane == 0) s[j] = a;
    }
}

__device__ __forceinline__ float frame_energy(const float* __restrict__ s, int f, int nb) {
    const float a = f - 2 >= 0 && f - 2 < nb ? s[f - 2] : 0.0f, b = f - 1 >= 0 && f - 1 < nb ? s[f - 1] : 0.0f;
    const float c = f < nb ? s[f] : 0.0f, d = f + 1 < nb ? s[f + 1] : 0.0f;
    return ((a + b) + c) + d;
}

// e[b, f] (written out when p.energy is given, zeros in [F_b, F_max)) and the utterance's peak energy: max over the workgroup,
// then an ordinary vector atomic max on the u32 pattern of the float (ordered like the floats while they are >= 0; a NaN never
// wins an fmaxf and is never merged)
__global__ __launch_bounds__(kThreads) void trim_frame_energy_kernel(TrimP p) {
    __shared__ float red[kWaves];
    const int b = blockIdx.y, L = p.len[b], F = 1 + L / kHop, nb = (L + kHop - 1) / kHop;
    const int f = blockIdx.x * kThreads + threadIdx.x;
    float e = 0.0f;
    if (f < F) e = frame_energy(p.sums + (long long)b * p.NB, f, nb);
    if (p.energy && f < p.F_max) p.energy[(long long)b * p.F_max + f] = e;
    block_peak_merge(e, red, p.peak + b);
}

// first / last kept frame of each utterance: vector atomic min / max of the frame index (first[] starts at UINT_MAX, last[] at -1).
// A silent utterance (peak below FLT_MIN) keeps every frame.
__global__ __launch_bounds__(kThreads) void trim_keep_bounds_kernel(TrimP p) {
    __shared__ int red_lo[kWaves], red_hi[kWaves];
    const int b = blockIdx.y, L = p.len[b], F = 1 + L / kHop, nb = (L + kHop - 1) / kHop;
    const int f = blockIdx.x * kThreads + threadIdx.x;
    const float E = __uint_as_float(p.peak[b]);
    const float thr = __fmul_rn(E, p.factor);
    bool keep = false;
    if (f < F) keep = !(E >= FLT_MIN) || frame_energy(p.sums + (long long)b * p.NB, f, nb) > thr;
    int lo = keep ? f : INT_MAX, hi = keep ? f : -1;
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        lo = min(lo, __shfl_xor(lo, d));
        hi = max(hi, __shfl_xor(hi, d));
    }
    if ((threadIdx.x & 63) == 0) { red_lo[threadIdx.x >> 6] = lo; red_hi[threadIdx.x >> 6] = hi; }
    __syncthreads();
    if (threadIdx.x == 0) {
        lo = min(min(red_lo[0], red_lo[1]), min(red_lo[2], red_lo[3]));
        hi = max(max(red_hi[0], red_hi[1]), max(red_hi[2], red_hi[3]));
        if (hi >= 0) {
            atomicMin(p.first + b, (unsigned)lo);
            atomicMax(p.last + b, hi);
        }
    }
}

// out[b, j] = wav[b, start_b + j] for j < end_b - start_b, zeros up to Lout_max.  16-byte moves where both rows allow them (start is
// a multiple of 512 samples, so only the row bases decide).
__global__ __launch_bounds__(kThreads) void trim_copy_kernel(TrimP p) {
    const int b = blockIdx.y;
    int start, end;
    trim_bounds(p.first[b], p.last[b], p.len[b], &start, &end);
    const int n = end - start;
    const float* __restrict__ x = p.wav + (long long)b * p.L_max + start;
    float* __restrict__ out = p.out + (long long)b * p.Lout_max;
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    for (long long j = ((long long)blockIdx.x * kThreads + threadIdx.x) * 4; j < p.Lout_max; j += (long long)gridDim.x * kThreads * 4) {
        if (vec && j + 3 < p.Lout_max && (j + 3 < n || j >= n)) {
            *reinterpret_cast<float4*>(out + j) = j < n ? *reinterpret_cast<const float4*>(x + j) : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            for (int q = 0; q < 4 && j + q < p.Lout_max; ++q) out[j + q] = j + q < n ? x[j + q] : 0.0f;
        }
    }
}

static bool energy_args_ok(const TrimP& p) {
    return p.B <= 65535 && p.max_len >= 1 && p.max_len <= p.L_max && p.NB >= (p.max_len + kHop - 1) / kHop &&
           (!p.energy || p.F_max >= 1 + p.max_len / kHop) && p.max_len <= INT_MAX - 4 * kHop;
}
static void launch_energy_half(const TrimP& p, hipStream_t s) {
    const int frames = std::max(1 + p.max_len / kHop, p.energy ? p.F_max : 0);
    hipLaunchKernelGGL(trim_block_sums_kernel, dim3((p.NB + kTileBlocks - 1) / kTileBlocks, p.B), dim3(kThreads), 0, s, p);
    hipLaunchKernelGGL(trim_frame_energy_kernel, dim3((frames + kThreads - 1) / kThreads, p.B), dim3(kThreads), 0, s, p);
}

hipError_t launch_trim_energy(const TrimP& p, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (!energy_args_ok(p)) return hipErrorInvalidValue;
    launch_energy_half(p, s);
    return hipGetLastError();
}

hipError_t launch_trim(const TrimP& p, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (!energy_args_ok(p) || p.Lout_max < p.max_len) return hipErrorInvalidValue;
    launch_energy_half(p, s);
    hipLaunchKernelGGL(trim_keep_bounds_kernel, dim3((1 + p.max_len / kHop + kThreads - 1) / kThreads, p.B), dim3(kThreads), 0, s, p);
    const int gx = (int)std::min<long long>(((long long)p.Lout_max + kThreads * 16 - 1) / (kThreads * 16), 1024);
    hipLaunchKernelGGL(trim_copy_kernel, dim3(gx, p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
