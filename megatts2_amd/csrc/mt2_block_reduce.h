// Block reductions of the audio analysis kernels (loudness.hip, ebu.hip, f0.hip, prosody.hip, trim.hip, resample.hip): the fixed-tree
// sum and max of doubles over a workgroup, and the merge of a non-negative float into a per-utterance peak word.  The trees depend on
// the thread's index alone, so whatever is summed in a fixed order per thread stays bit-identical from launch to launch.
#pragma once
#include <hip/hip_runtime.h>

namespace mt2 {

// the sum of the N partial sums of a workgroup in a fixed tree (stride N / 2 .. 1); the result is in every thread.  red: N doubles
template <int N> __device__ __forceinline__ double block_tree_sum(double* red, double v) {
    const int t = threadIdx.x;
    __syncthreads();                           // the previous use of red[] is over
    red[t] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (t < s) red[t] += red[t + s];
        __syncthreads();
    }
    return red[0];
}
// the same tree over a sum and a count side by side, behind one set of barriers
template <int N> __device__ __forceinline__ void block_tree_sum(double* sv, int* sn, double* v, int* n) {
    const int t = threadIdx.x;
    __syncthreads();
    sv[t] = *v; sn[t] = *n;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (t < s) { sv[t] += sv[t + s]; sn[t] += sn[t + s]; }
        __syncthreads();
    }
    *v = sv[0]; *n = sn[0];
}
// the max (fmax: a NaN never wins) of the N values of a workgroup in the same tree; the result is in every thread
template <int N> __device__ __forceinline__ double block_tree_max(double* red, double v) {
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int s = N / 2; s > 0; s >>= 1) {
        if (t < s) red[t] = fmax(red[t], red[t + s]);
        __syncthreads();
    }
    return red[0];
}

// A peak word holds the u32 pattern of a float >= 0, which is ordered like the floats themselves: the max is an ordinary vector atomic
// max - order-independent, so the peak is deterministic.  A NaN never wins an fmaxf and is never merged; the caller zeroes the word.
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v = fmaxf(v, __shfl_xor(v, d));
    return v;
}
// per wave, no LDS.  kSkipStale: the word only grows, so a wave whose max is not over the value it reads - however stale - has nothing
// to add and skips the atomic, which otherwise queues on the one cache line that holds every utterance's word
template <bool kSkipStale> __device__ __forceinline__ void wave_peak_merge(float v, unsigned* word) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0 && v > 0.0f) {
        const unsigned bits = __float_as_uint(v);
        if (!kSkipStale || bits > __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(word, bits);
    }
}
// per workgroup of 256 threads: one atomic.  red: 4 floats
__device__ __forceinline__ void block_peak_merge(float v, float* red, unsigned* word) {
    v = wave_max(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        const float m = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
        if (m > 0.0f) atomicMax(word, __float_as_uint(m));
    }
}

}  // namespace mt2
