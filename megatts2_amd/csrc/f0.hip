// F0 tracking of 16 kHz audio by YIN (de Cheveigne & Kawahara 2002, steps 2-5) and the per-utterance pitch moments (gfx950).  The
// reference tree has no pitch tracker (it would take one from librosa or pyworld); parity with librosa.yin / pyin is unpinned
//  and the rule is our own statement.  For one utterance x[0 .. L), frames aligned to the mel front-end's:
//
//   T = 1 + L / hop frames;  frame t reads x over [hop t - 512, hop t + 512), a sample outside [0, L) being a zero by its index;
//   s = hop t - 512;  W = 768
//   tau_min = ceil(sr / fmax), tau_max = floor(sr / fmin);  refused, not clamped, unless 2 <= tau_min < tau_max <= 256
//   d[tau]  = sum_{j = 0}^{W - 1} (x[s + j] - x[s + j + tau])^2 for tau = 0 .. 256 - all 257, whatever tau_max - as ONE f32 chain
//             over j ascending:  e = __fsub_rn(a, b);  acc = fmaf(e, e, acc)  from 0.  d[0] is exactly 0.
//   c[0] = 0, c[tau] = c[tau - 1] + d[tau]   (one f32 add each, tau ascending)
//   d'[0] = 1, d'[tau] = (d[tau] * (float)tau) / c[tau]   (one f32 product, one true f32 division);  1 where c[tau] is not > 0
//   tau0 = the smallest tau in [tau_min, tau_max] with d'[tau] < threshold; from there up while tau + 1 <= tau_max and
//          d'[tau + 1] < d'[tau]: the end of the walk is tau*.  No such tau0: tau* = the smallest tau in [tau_min, tau_max] that
//          attains the minimum of d' (a NaN never wins; all NaN: tau_min).  cmnd = d'[tau*];  voiced iff d'[tau*] < threshold
//   voiced, tau* - 1 >= 1 and tau* + 1 <= tau_max:  a, b, c = d'[tau* - 1], d'[tau*], d'[tau* + 1];  den = (a - 2 b) + c;
//          delta = (a - c) / (2 den) if den > 0, else 0.  f0 = (float)sr / ((float)tau* + delta);  unvoiced: f0 = 0
//
// The order of every sum depends on the sample's index in its utterance alone, so a ragged batch is bit-identical to its
// utterances alone.  Frames at or beyond T_b, up to T_max, are written as unvoiced (f0 0, cmnd 1, lag 0, d 0).  A non-finite sample
// cannot fault or write outside the outputs (tau* always lies in [tau_min, tau_max]) and does not change a frame whose window
// does not hold it; nothing more is promised.
//
// One workgroup per (frame, utterance): the frame's 1024 samples are staged in LDS once; thread i owns the lag i + 1, so x[s + j]
// is one broadcast word and x[s + j + tau] consecutive words for consecutive lanes (conflict-free).  d stays in LDS; thread 0 runs
// the sequential prefix sum, the workgroup the 256 divisions, wave 0 the two searches as lane reductions (the comparisons are
// exact, so the result is the rule's) and lane 0 the walk and the parabola.
//
// Moments of f0 f32 [B, T_max] over the voiced frames (f0 > 0) among the first T_b of utterance b, all in double, two passes:
//   n;  mu = sum f / n;  m_k = sum (f - mu)^k / n, k = 2, 3, 4;  out = n, n / T_b, mu, sqrt(m2), m3 / m2^1.5, m4 / m2^2 - 3
//   n = 0: all zeros;  m2 = 0: sigma = skew = kurt = 0.
// A workgroup per utterance: thread i sums the frames i, i + 256, ... ascending, then the 256 partial sums meet in a fixed tree
// (stride 128, 64, ... 1): the order depends on the frame index alone, not on the batch slot or T_max.
#include "../../include/megatts2_hip.h"
#include "mt2_kernels.h"

#include <limits.h>
#include <math.h>

namespace mt2 {

namespace {
constexpr int kThreads = 256;
constexpr int kFrame = MT2_F0_FRAME, kWindow = MT2_F0_WINDOW, kMaxLag = MT2_F0_MAX_LAG;
static_assert(kFrame == 1024 && kWindow == 768 && kMaxLag == 256 && kWindow + kMaxLag == kFrame && kMaxLag == kThreads,
              "a thread owns one lag and loads four samples; the last read is x[s + 767 + 256]");
}  // namespace

bool f0_lags(int sample_rate, float fmin, float fmax, int* lag_min, int* lag_max) {
    if (sample_rate < 1 || !std::isfinite(fmin) || !std::isfinite(fmax) || !(fmin > 0.0f) || !(fmax > 0.0f)) return false;
    const double lo = ceil((double)sample_rate / (double)fmax), hi = floor((double)sample_rate / (double)fmin);
    if (!(lo >= 2.0 && lo < hi && hi <= (double)kMaxLag)) return false;
    *lag_min = (int)lo;
    *lag_max = (int)hi;
    return true;
}

__global__ __launch_bounds__(kThreads) void f0_yin_kernel(F0P p) {
    __shared__ __attribute__((aligned(16))) float xs[kFrame];
    __shared__ float ds[kMaxLag + 1];         // d, then d'
    __shared__ float cs[kMaxLag + 1];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int L = p.len[b], T = 1 + L / p.hop;
    const long long row = (long long)b * p.T_max + t;
    if (t >= T) {                              // uniform for the workgroup: an unvoiced frame behind the utterance's own
        if (tid == 0) {
            p.f0[row] = 0.0f;
            if (p.cmnd) p.cmnd[row] = 1.0f;
            if (p.lag) p.lag[row] = 0;
        }
        if (p.diff) {
            p.diff[row * (kMaxLag + 1) + tid + 1] = 0.0f;
            if (tid == 0) p.diff[row * (kMaxLag + 1)] = 0.0f;
        }
        return;
    }
    // the frame [s, s + 1024): samples outside [0, L) are zeros by their index, never read
    const float* __restrict__ x = p.wav + (long long)b * p.L_max;
    const long long i0 = (long long)p.hop * t - kFrame / 2 + 4 * tid;
    float4 v;
    if (i0 >= 0 && i0 + 3 < L && (reinterpret_cast<uintptr_t>(x + i0) & 15) == 0) {
        v = *reinterpret_cast<const float4*>(x + i0);
    } else {
        v.x = i0 >= 0 && i0 < L ? x[i0] : 0.0f;
        v.y = i0 + 1 >= 0 && i0 + 1 < L ? x[i0 + 1] : 0.0f;
        v.z = i0 + 2 >= 0 && i0 + 2 < L ? x[i0 + 2] : 0.0f;
        v.w = i0 + 3 >= 0 && i0 + 3 < L ? x[i0 + 3] : 0.0f;
    }
    *reinterpret_cast<float4*>(xs + 4 * tid) = v;
    __syncthreads();
    // step 3: thread tid owns tau = tid + 1; one chain over j ascending
    const int tau = tid + 1;
    float acc = 0.0f;
#pragma unroll 8
    for (int j = 0; j < kWindow; j += 4) {
        const float4 a = *reinterpret_cast<const float4*>(xs + j);          // broadcast
        const float* __restrict__ y = xs + j + tau;                          // j + 3 + tau <= 1023
        float e = __fsub_rn(a.x, y[0]); acc = fmaf(e, e, acc);
        e = __fsub_rn(a.y, y[1]); acc = fmaf(e, e, acc);
        e = __fsub_rn(a.z, y[2]); acc = fmaf(e, e, acc);
        e = __fsub_rn(a.w, y[3]); acc = fmaf(e, e, acc);
    }
    ds[tau] = acc;
    if (tid == 0) ds[0] = 0.0f;
    if (p.diff) {
        p.diff[row * (kMaxLag + 1) + tau] = acc;
        if (tid == 0) p.diff[row * (kMaxLag + 1)] = 0.0f;
    }
    __syncthreads();
    // step 4: the prefix sum is sequential by the rule (one thread), the 256 divisions are not
    if (tid == 0) {
        float c = 0.0f;
#pragma unroll 8
        for (int k = 1; k <= kMaxLag; ++k) {
            c = __fadd_rn(c, ds[k]);
            cs[k] = c;
        }
    }
    __syncthreads();
    {
        const float c = cs[tau];
        const float q = c > 0.0f ? __fdiv_rn(__fmul_rn(acc, (float)tau), c) : 1.0f;
        ds[tau] = q;
        if (tid == 0) ds[0] = 1.0f;
    }
    __syncthreads();
    if (tid >= 64) return;
    // step 5 on wave 0: lane l looks at tau = l, l + 64, ...; both searches are exact comparisons, so lane reductions give the rule's result
    const int lo = p.lag_min, hi = p.lag_max;
    int first = INT_MAX, arg = INT_MAX;
    float best = INFINITY;
    for (int k = tid; k <= hi; k += 64) {
        if (k < lo) continue;
        const float q = ds[k];
        if (q < p.threshold && k < first) first = k;
        if (q < best || (q == best && k < arg)) { best = q; arg = k; }       // a NaN fails both
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        first = min(first, __shfl_xor(first, o));
        const float ob = __shfl_xor(best, o);
        const int oa = __shfl_xor(arg, o);
        if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
    }
    if (tid != 0) return;
    int ts;
    if (first != INT_MAX) {
        ts = first;
        while (ts + 1 <= hi && ds[ts + 1] < ds[ts]) ++ts;
    } else {
        ts = arg != INT_MAX ? arg : lo;
    }
    const float q = ds[ts];
    float f = 0.0f;
    if (q < p.threshold) {
        float delta = 0.0f;
        if (ts - 1 >= 1 && ts + 1 <= hi) {
            const float a = ds[ts - 1], c = ds[ts + 1];
            const float den = __fadd_rn(__fsub_rn(a, __fmul_rn(2.0f, q)), c);
            if (den > 0.0f) delta = __fdiv_rn(__fsub_rn(a, c), __fmul_rn(2.0f, den));
        }
        f = __fdiv_rn((float)p.sample_rate, __fadd_rn((float)ts, delta));
    }
    p.f0[row] = f;
    if (p.cmnd) p.cmnd[row] = q;
    if (p.lag) p.lag[row] = ts;
}

hipError_t launch_f0_yin(const F0P& p, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (p.B > 65535 || p.hop < 1 || p.hop > kFrame || p.max_len < 1 || p.max_len > p.L_max || p.T_max < 1 + p.max_len / p.hop ||
        p.lag_min < 2 || p.lag_min >= p.lag_max || p.lag_max > kMaxLag || p.f0 == nullptr)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(f0_yin_kernel, dim3(p.T_max, p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

// the 256 partial sums of a workgroup in a fixed tree; the result is in every thread
__device__ __forceinline__ double f0_tree_sum(double* red, double v) {
    __syncthreads();                           // the previous use of red[] is over
    red[threadIdx.x] = v;
    __syncthreads();
    for (int o = kThreads / 2; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kThreads) void f0_stats_kernel(const float* __restrict__ f0, const int* __restrict__ frame_len, int T_max,
                                                            double* __restrict__ stats) {
    __shared__ double red[kThreads];
    const int b = blockIdx.x, T = frame_len[b];
    const float* __restrict__ f = f0 + (long long)b * T_max;
    double cnt = 0.0, sum = 0.0;
    for (int t = threadIdx.x; t < T; t += kThreads) {
        const float v = f[t];
        if (v > 0.0f) { cnt += 1.0; sum += (double)v; }
    }
    const double n = f0_tree_sum(red, cnt);
    const double total = f0_tree_sum(red, sum);
    double* __restrict__ out = stats + 6ll * b;
    if (!(n > 0.0)) {
        if (threadIdx.x < 6) out[threadIdx.x] = 0.0;
        return;
    }
    const double mu = total / n;
    double s2 = 0.0, s3 = 0.0, s4 = 0.0;
    for (int t = threadIdx.x; t < T; t += kThreads) {
        const float v = f[t];
        if (v > 0.0f) {
            const double e = (double)v - mu, e2 = e * e;
            s2 += e2; s3 += e2 * e; s4 += e2 * e2;
        }
    }
    const double m2 = f0_tree_sum(red, s2) / n, m3 = f0_tree_sum(red, s3) / n, m4 = f0_tree_sum(red, s4) / n;
    if (threadIdx.x == 0) {
        out[0] = n; out[1] = n / (double)T; out[2] = mu;
        const bool flat = !(m2 > 0.0);
        out[3] = flat ? 0.0 : sqrt(m2);
        out[4] = flat ? 0.0 : m3 / (m2 * sqrt(m2));
        out[5] = flat ? 0.0 : m4 / (m2 * m2) - 3.0;
    }
}

hipError_t launch_f0_stats(const float* f0, const int* frame_len, int T_max, int B, double* stats, hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (T_max < 1 || f0 == nullptr || frame_len == nullptr || stats == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f0_stats_kernel, dim3(B), dim3(kThreads), 0, s, f0, frame_len, T_max, stats);
    return hipGetLastError();
}

}  // namespace mt2
