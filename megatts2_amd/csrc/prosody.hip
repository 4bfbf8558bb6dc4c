// Per-phone prosody (gfx950): an energy contour on the mel's frames, the segment reduction of an F0 track (and that contour) over
// phone durations, and the voiced frames of an F0 track compacted to a semitone contour - the input of a DTW pitch distance.  The
// reference tree has no counterpart (it would take pitch and energy from librosa or pyworld); parity with any outside library and
// quality on real speech are unpinned and the rules are our own statements.
//
// 1. Energy (mt2_frame_energy).  For one utterance x[0 .. L):
//   T = 1 + L / hop frames;  frame t reads x over [hop t - 512, hop t + 512) - MT2_F0_FRAME, exactly the F0 frames, so energy[t],
//   f0[t] and mel frame t coincide; a sample outside [0, L) is a zero by its index, never a read
//   energy[t] = the mean square of the 1024 samples in f32, by ONE wave:  lane l runs one chain acc = fmaf(x, x, acc) from 0 over the
//   in-frame offsets 256 i + 4 l + r, i = 0 .. 3 outer, r = 0 .. 3 inner (16-byte reads where the row's address allows);  the 64
//   partial sums meet in the xor butterfly 32, 16, 8, 4, 2, 1 (as trim_block_sums_kernel's);  one product by 2^-10, which is exact
//   frames in [T_b, T_max) are written 0
//
// 2. Phone prosody (mt2_phone_prosody).  For utterance b with Np phones, T frames, dur int32 [Np], f0 and (optionally) energy [T]:
//   start[p] = sum_{q < p} max(dur[q], 0) in int64;  phone p owns the frames [min(start, T), min(start + max(dur[p], 0), T)),
//   taken in ascending order;  a frame is voiced iff f0 > 0 (a NaN is not).  out[b, p, 0 .. 8), all in double:
//     0 start (clipped)   1 frames owned   2 voiced frames among them   3 mean f0 (Hz) over the voiced frames
//     4 mean of 12 log2((double)f0 / 55) over the voiced frames (semitones above A1)   5 min f0   6 max f0 over the voiced frames
//     7 mean of energy over all owned frames (0 when energy is NULL)
//   3 - 6 are 0 without a voiced frame, 7 is 0 without a frame;  rows p >= Np, up to Np_max, are all zeros.  dur beyond Np and
//   frames beyond T are never read.  dur_sum[b] (optional, int64) = the unclipped sum of max(dur, 0): the caller compares it with T.
//   One workgroup of 256 per utterance: the durations are scanned 256 phones at a time (an integer scan is exact, so its form is
//   free), then thread i owns phones i, i + 256, ... and walks each one's frames sequentially with double accumulators.
//
// 3. Pitch contour (mt2_pitch_contour).  The voiced frames (f0 > 0) among the first T of f0 are kept in order - a stable compaction
//   by the exclusive count of voiced flags in front of each frame:  s = 12 log2((double)f0);  with `center`, mu = sum s / n in double
//   in the order of f0_stats_kernel (thread i sums the frames i, i + 256, ... ascending, the 256 partial sums meet in a fixed tree,
//   stride 128 .. 1) and st[k] = (float)(s - mu), rounded once;  without, st[k] = (float)s.  index[k] (optional) = the frame entry k
//   came from;  entries in [n, T_max) are written 0 / -1;  n_voiced[b] = n.  One workgroup of 256 per utterance.
//
// Every sum is taken in an order that depends on the sample / frame / phone index within its utterance alone: a ragged batch is
// bit-identical to its utterances alone, whatever the slot, L_max, T_max or Np_max.  A non-finite input cannot fault, cannot write
// outside the outputs and cannot change an output whose inputs do not hold it.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <math.h>

namespace mt2 {

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kFrame = MT2_F0_FRAME;
static_assert(kFrame == 1024 && kFrame == 16 * 64, "a lane owns four groups of four samples of the frame");
}  // namespace

// four consecutive samples of one utterance from index i on (i may be negative): a 16-byte load where all four are real and the
// address allows it, zeros by index otherwise
__device__ __forceinline__ float4 prosody_load4(const float* __restrict__ x, long long i, int L) {
    if (i >= 0 && i + 3 < L && (reinterpret_cast<uintptr_t>(x + i) & 15) == 0) return *reinterpret_cast<const float4*>(x + i);
    float4 v;
    v.x = i >= 0 && i < L ? x[i] : 0.0f;
    v.y = i + 1 >= 0 && i + 1 < L ? x[i + 1] : 0.0f;
    v.z = i + 2 >= 0 && i + 2 < L ? x[i + 2] : 0.0f;
    v.w = i + 3 >= 0 && i + 3 < L ? x[i + 3] : 0.0f;
    return v;
}

// a wave per frame, four frames a workgroup
__global__ __launch_bounds__(kThreads) void frame_energy_kernel(EnergyP p) {
    const int b = blockIdx.y, lane = threadIdx.x & 63;
    const int t = blockIdx.x * kWaves + (threadIdx.x >> 6);
    if (t >= p.T_max) return;                                              // wave-uniform
    const int L = p.len[b], T = 1 + L / p.hop;
    float* __restrict__ out = p.energy + (long long)b * p.T_max + t;
    if (t >= T) {
        if (lane == 0) *out = 0.0f;
        return;
    }
    const float* __restrict__ x = p.wav + (long long)b * p.L_max;
    const long long s = (long long)p.hop * t - kFrame / 2 + 4 * lane;
    float acc = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 v = prosody_load4(x, s + 256 * i, L);
        acc = fmaf(v.x, v.x, acc); acc = fmaf(v.y, v.y, acc); acc = fmaf(v.z, v.z, acc); acc = fmaf(v.w, v.w, acc);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) acc += __shfl_xor(acc, d);
    if (lane == 0) *out = acc * (1.0f / kFrame);
}

hipError_t launch_frame_energy(const EnergyP& p, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (p.B > 65535 || p.hop < 1 || p.hop > kFrame || p.max_len < 1 || p.max_len > p.L_max || p.T_max < 1 + p.max_len / p.hop ||
        p.wav == nullptr || p.len == nullptr || p.energy == nullptr)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(frame_energy_kernel, dim3((p.T_max + kWaves - 1) / kWaves, p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

// The inclusive prefix sum of one value per thread over the workgroup of 256 (wave scans by __shfl_up, the four wave totals through
// LDS): *total is the workgroup's sum.  Integer, so exact in any form.  Two barriers; wsum is free again on return.
template <typename T>
__device__ __forceinline__ T block_scan_inclusive(T v, T* wsum, T* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const T u = __shfl_up(v, o);
        if (lane >= o) v += u;
    }
    if (lane == 63) wsum[w] = v;
    __syncthreads();
    T off = 0, all = 0;
#pragma unroll
    for (int i = 0; i < kWaves; ++i) {
        const T q = wsum[i];
        if (i < w) off += q;
        all += q;
    }
    __syncthreads();
    *total = all;
    return v + off;
}

__global__ __launch_bounds__(kThreads) void phone_prosody_kernel(PhoneProsodyP p) {
    __shared__ long long wsum[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int Np = p.np_len[b], T = p.t_len[b];
    const float* __restrict__ f0 = p.f0 + (long long)b * p.T_max;
    const float* __restrict__ en = p.energy ? p.energy + (long long)b * p.T_max : nullptr;
    const int* __restrict__ dur = p.dur + (long long)b * p.Np_max;
    long long base = 0;                                                    // the durations in front of this chunk (uniform)
    for (int p0 = 0; p0 < p.Np_max; p0 += kThreads) {
        const int ph = p0 + tid;
        long long d = 0, start = 0;
        if (p0 < Np) {                                                     // uniform: the scan's barriers are met by all
            if (ph < Np) d = max(dur[ph], 0);
            long long total;
            const long long incl = block_scan_inclusive<long long>(d, wsum, &total);
            start = base + (incl - d);                                     // exclusive
            base += total;
        }
        if (ph >= p.Np_max) continue;
        double o[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (ph < Np) {
            const int t0 = (int)min(start, (long long)T), t1 = (int)min(start + d, (long long)T);
            double nv = 0.0, sum = 0.0, st = 0.0, lo = 0.0, hi = 0.0, es = 0.0;
            for (int t = t0; t < t1; ++t) {
                const float v = f0[t];
                if (v > 0.0f) {
                    const double f = (double)v;
                    lo = nv > 0.0 ? fmin(lo, f) : f;
                    hi = nv > 0.0 ? fmax(hi, f) : f;
                    nv += 1.0;
                    sum += f;
                    st += 12.0 * log2(f / 55.0);
                }
                if (en) es += (double)en[t];
            }
            o[0] = (double)t0; o[1] = (double)(t1 - t0); o[2] = nv;
            if (nv > 0.0) { o[3] = sum / nv; o[4] = st / nv; o[5] = lo; o[6] = hi; }
            if (t1 > t0) o[7] = es / (double)(t1 - t0);
        }
        double2* __restrict__ row = reinterpret_cast<double2*>(p.out + ((long long)b * p.Np_max + ph) * 8);      // 64-byte rows
        row[0] = make_double2(o[0], o[1]); row[1] = make_double2(o[2], o[3]);
        row[2] = make_double2(o[4], o[5]); row[3] = make_double2(o[6], o[7]);
    }
    if (p.dur_sum && tid == 0) p.dur_sum[b] = base;
}

hipError_t launch_phone_prosody(const PhoneProsodyP& p, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (p.B > 65535 || p.T_max < 1 || p.Np_max < 1 || p.f0 == nullptr || p.dur == nullptr || p.np_len == nullptr || p.t_len == nullptr ||
        p.out == nullptr || (reinterpret_cast<uintptr_t>(p.out) & 15) != 0)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(phone_prosody_kernel, dim3(p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

__global__ __launch_bounds__(kThreads) void pitch_contour_kernel(PitchContourP p) {
    __shared__ double red[kThreads];
    __shared__ int wsum[kWaves];
    const int b = blockIdx.x, tid = threadIdx.x, T = p.t_len[b];
    const float* __restrict__ f0 = p.f0 + (long long)b * p.T_max;
    float* __restrict__ st = p.st + (long long)b * p.T_max;
    int* __restrict__ index = p.index ? p.index + (long long)b * p.T_max : nullptr;
    double mu = 0.0;
    if (p.center) {
        double cnt = 0.0, sum = 0.0;
        for (int t = tid; t < T; t += kThreads) {
            const float v = f0[t];
            if (v > 0.0f) { cnt += 1.0; sum += 12.0 * log2((double)v); }
        }
        const double n = block_tree_sum<kThreads>(red, cnt);
        const double total = block_tree_sum<kThreads>(red, sum);
        if (n > 0.0) mu = total / n;
    }
    int base = 0;                                                          // the voiced frames in front of this chunk (uniform)
    for (int t0 = 0; t0 < T; t0 += kThreads) {
        const int t = t0 + tid;
        const float v = t < T ? f0[t] : 0.0f;
        const int flag = v > 0.0f ? 1 : 0;
        int total;
        const int incl = block_scan_inclusive<int>(flag, wsum, &total);
        if (flag) {
            const int k = base + (incl - flag);                            // exclusive: k <= t
            st[k] = (float)(12.0 * log2((double)v) - mu);
            if (index) index[k] = t;
        }
        base += total;
    }
    for (int k = base + tid; k < p.T_max; k += kThreads) {
        st[k] = 0.0f;
        if (index) index[k] = -1;
    }
    if (tid == 0) p.n_voiced[b] = base;
}

hipError_t launch_pitch_contour(const PitchContourP& p, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (p.B > 65535 || p.T_max < 1 || p.f0 == nullptr || p.t_len == nullptr || p.st == nullptr || p.n_voiced == nullptr)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(pitch_contour_kernel, dim3(p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
