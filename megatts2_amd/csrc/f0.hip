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
// The second tracker (mt2_f0_track; off by default): a Viterbi pass over the same d', the usual cure (pYIN, RAPT) for YIN's octave
// errors - with dominant even harmonics d'[tau0 / 2] already dips under the threshold and the first dip is an octave high.  The rule
// is our own (parity with librosa.pyin unpinned).  Frames, d, c, d', tau_min and tau_max as above; n = tau_max - tau_min + 1 <= 255
// states, state k the lag tau_min + k; every operation below one f32 operation rounded on its own, no fma contraction:
//
//   lg[k]    = (float) log2((double)(tau_min + k)), built in double on the host and rounded once
//   bias[k]  = __fmul_rn(octave_cost, __fsub_rn(lg[k], lg[0]))
//   o[t, k]  = __fadd_rn(q, bias[k]),  q = d'[t, tau_min + k] if that is finite, else 1.0f: every cost is finite by construction
//   tr(j, k) = __fmul_rn(jump_cost, fabsf(__fsub_rn(lg[k], lg[j]))): the jump in octaves times a weight, all n x n pairs, no band
//   delta[0, k] = o[0, k];  t >= 1:  best = min_j __fadd_rn(delta[t - 1, j], tr(j, k)), j ascending with a strict < (the smallest j
//              wins a tie), psi[t, k] = that j;  delta'[k] = __fadd_rn(o[t, k], best);  m = min_k delta'[k];
//              delta[t, k] = __fsub_rn(delta'[k], m) - the renormalisation keeps f32 resolution on 60 s clips
//   k*[T - 1] = the smallest k attaining min delta[T - 1, .];  k*[t - 1] = psi[t, k*[t]];  T = 1: the arg-min alone
//   tau* = tau_min + k*[t];  cmnd = d'[t, tau*];  voiced iff cmnd < threshold (YIN's criterion at the tracked lag: no unvoiced
//              state, and octave_cost never enters the voicing decision);  f0 by the parabola above, 0 when unvoiced
//
// octave_cost (0.02) and jump_cost (0.5) are finite and >= 0; jump_cost 0 makes the frames independent.  A non-finite sample cannot
// fault, write outside the outputs or move tau* outside [tau_min, tau_max], but - the path being global - it may change frames
// anywhere in its utterance.  Nothing depends on the batch slot, L_max or T_max.  Kernels: f0_cmnd_kernel (steps 1-4 through the
// device function f0_yin_kernel uses, d' to scratch) and f0_viterbi_kernel (a workgroup per utterance; see there).
//
// Moments of f0 f32 [B, T_max] over the voiced frames (f0 > 0) among the first T_b of utterance b, all in double, two passes:
//   n;  mu = sum f / n;  m_k = sum (f - mu)^k / n, k = 2, 3, 4;  out = n, n / T_b, mu, sqrt(m2), m3 / m2^1.5, m4 / m2^2 - 3
//   n = 0: all zeros;  m2 = 0: sigma = skew = kurt = 0.
// A workgroup per utterance: thread i sums the frames i, i + 256, ... ascending, then the 256 partial sums meet in a fixed tree
// (stride 128, 64, ... 1): the order depends on the frame index alone, not on the batch slot or T_max.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
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

// Steps 1-4 of one frame by a workgroup of 256, shared by both trackers so that they see the same d' bits by construction: on return
// ds[0 .. 256] holds d' (behind a barrier); d goes to diff_row[0 .. 256] where that is given.  xs [1024] must be 16-byte aligned.
__device__ __forceinline__ void f0_frame_cmnd(const float* __restrict__ x, int L, int hop, int t, float* __restrict__ diff_row, float* xs,
                                              float* ds, float* cs) {
    const int tid = threadIdx.x;
    // the frame [s, s + 1024): samples outside [0, L) are zeros by their index, never read
    const long long i0 = (long long)hop * t - kFrame / 2 + 4 * tid;
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
    if (diff_row) {
        diff_row[tau] = acc;
        if (tid == 0) diff_row[0] = 0.0f;
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
}

// a frame in [T_b, T_max) by a workgroup of 256: f0 0, cmnd 1, lag 0, d 0
__device__ __forceinline__ void f0_unvoiced_frame(const F0P& p, long long row) {
    const int tid = threadIdx.x;
    if (tid == 0) {
        p.f0[row] = 0.0f;
        if (p.cmnd) p.cmnd[row] = 1.0f;
        if (p.lag) p.lag[row] = 0;
    }
    if (p.diff) {
        p.diff[row * (kMaxLag + 1) + tid + 1] = 0.0f;
        if (tid == 0) p.diff[row * (kMaxLag + 1)] = 0.0f;
    }
}

__global__ __launch_bounds__(kThreads) void f0_yin_kernel(F0P p) {
    __shared__ __attribute__((aligned(16))) float xs[kFrame];
    __shared__ float ds[kMaxLag + 1];         // d, then d'
    __shared__ float cs[kMaxLag + 1];
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int L = p.len[b], T = 1 + L / p.hop;
    const long long row = (long long)b * p.T_max + t;
    if (t >= T) {                              // uniform for the workgroup: an unvoiced frame behind the utterance's own
        f0_unvoiced_frame(p, row);
        return;
    }
    f0_frame_cmnd(p.wav + (long long)b * p.L_max, L, p.hop, t, p.diff ? p.diff + row * (kMaxLag + 1) : nullptr, xs, ds, cs);
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

// ---- the second tracker: a Viterbi pass over d' (the rule is in the header of this file) --------------------------------------------

void f0_track_table(int lag_min, int lag_max, float* lg) {
    for (int k = 0; k < kThreads; ++k) lg[k] = lag_min + k <= lag_max ? (float)log2((double)(lag_min + k)) : 0.0f;
}

// d' of every frame to scratch (one workgroup per frame, as f0_yin_kernel); frames in [T_b, T_max) are written as unvoiced here
__global__ __launch_bounds__(kThreads) void f0_cmnd_kernel(F0TrackP q) {
    __shared__ __attribute__((aligned(16))) float xs[kFrame];
    __shared__ float ds[kMaxLag + 1];
    __shared__ float cs[kMaxLag + 1];
    const F0P& p = q.y;
    const int t = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    const int L = p.len[b], T = 1 + L / p.hop;
    const long long row = (long long)b * p.T_max + t;
    if (t >= T) {
        f0_unvoiced_frame(p, row);
        return;
    }
    f0_frame_cmnd(p.wav + (long long)b * p.L_max, L, p.hop, t, p.diff ? p.diff + row * (kMaxLag + 1) : nullptr, xs, ds, cs);
    float* __restrict__ out = q.dprime + row * (kMaxLag + 1);
    out[tid + 1] = ds[tid + 1];
    if (tid == 0) out[0] = ds[0];
}

// One f32 operation each, never contracted: hipcc's __fmul_rn / __fadd_rn are plain operators, and an add of a product would become
// one fma (a single rounding where the rule has two).
__device__ __forceinline__ float f0_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ float f0_add(float a, float b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ float f0_sub(float a, float b) {
#pragma clang fp contract(off)
    return a - b;
}

// One workgroup per utterance, thread k owning state k (the lag tau_min + k); threads at or beyond n hold +inf and never win.
// Forward: delta is double-buffered in LDS beside lg; the predecessor scan reads both as 16-byte broadcasts, j ascending with a
// strict <, so it IS the direct form.  States in [n, n4) are padding (+inf, lg 0): +inf is never < best.  Frame t + 1's
// observation is loaded before frame t's scan.  psi goes out one byte per state, coalesced.
// Tail: the path is walked backwards by ONE lane over psi staged in LDS a tile of kTile frames at a time (no dependent global
// load per frame), then the tile's frames are refined in parallel, a thread per frame, by YIN's step 6.
constexpr int kTile = 128;
__global__ __launch_bounds__(kThreads) void f0_viterbi_kernel(F0TrackP q) {
    __shared__ __attribute__((aligned(16))) float dl[2][kThreads];
    __shared__ __attribute__((aligned(16))) float lgs[kThreads];
    __shared__ __attribute__((aligned(16))) unsigned char ps[kTile * kThreads];
    __shared__ float red[kThreads / 64];
    __shared__ int ks[kTile];
    __shared__ int kcur;
    const F0P& p = q.y;
    const int b = blockIdx.x, k = threadIdx.x;
    const int T = 1 + p.len[b] / p.hop;
    const int lo = p.lag_min, hi = p.lag_max, n = hi - lo + 1, n4 = (n + 3) & ~3;
    const bool live = k < n;
    const float* dp = q.dprime + (long long)b * p.T_max * (kMaxLag + 1);
    unsigned char* psi = q.psi + (long long)b * p.T_max * kThreads;
    const float jc = q.jump_cost;
    const float lgk = q.lg[k];                                     // 0 at or beyond n
    const float bias = f0_mul(q.octave_cost, f0_sub(lgk, q.lg[0]));
    lgs[k] = lgk;
    float qn = live ? dp[lo + k] : 0.0f;                           // d'[0, tau]
    {
        const float o = f0_add(isfinite(qn) ? qn : 1.0f, bias);
        dl[0][k] = live ? o : INFINITY;
        psi[k] = 0;                                                // row 0 has no predecessor
    }
    if (T > 1 && live) qn = dp[(long long)(kMaxLag + 1) + lo + k];
    __syncthreads();
    int cur = 0;
    for (int t = 1; t < T; ++t) {
        const float qt = qn;
        if (t + 1 < T && live) qn = dp[(long long)(t + 1) * (kMaxLag + 1) + lo + k];
        const float* dprev = dl[cur];
        float dn = INFINITY;
        int arg = 0;
        if (live) {
            float best = f0_add(dprev[0], f0_mul(jc, fabsf(f0_sub(lgk, lgs[0]))));
#pragma unroll 4
            for (int j = 0; j < n4; j += 4) {
                const float4 d4 = *reinterpret_cast<const float4*>(dprev + j);       // broadcasts
                const float4 l4 = *reinterpret_cast<const float4*>(lgs + j);
                float v = f0_add(d4.x, f0_mul(jc, fabsf(f0_sub(lgk, l4.x))));
                if (v < best) { best = v; arg = j; }
                v = f0_add(d4.y, f0_mul(jc, fabsf(f0_sub(lgk, l4.y))));
                if (v < best) { best = v; arg = j + 1; }
                v = f0_add(d4.z, f0_mul(jc, fabsf(f0_sub(lgk, l4.z))));
                if (v < best) { best = v; arg = j + 2; }
                v = f0_add(d4.w, f0_mul(jc, fabsf(f0_sub(lgk, l4.w))));
                if (v < best) { best = v; arg = j + 3; }
            }
            dn = f0_add(f0_add(isfinite(qt) ? qt : 1.0f, bias), best);
        }
        psi[(long long)t * kThreads + k] = (unsigned char)arg;
        float m = dn;                                              // the minimum is exact: its order is free
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fminf(m, __shfl_xor(m, o));
        if ((k & 63) == 0) red[k >> 6] = m;
        __syncthreads();
        m = fminf(fminf(red[0], red[1]), fminf(red[2], red[3]));
        dl[cur ^ 1][k] = f0_sub(dn, m);
        __syncthreads();
        cur ^= 1;
    }
    // the end of the path: the smallest k that attains the minimum (wave 0, exact comparisons)
    if (k < 64) {
        int arg = INT_MAX;
        float best = INFINITY;
        for (int i = k; i < n; i += 64) {
            const float v = dl[cur][i];
            if (v < best || (v == best && i < arg)) { best = v; arg = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const float ob = __shfl_xor(best, o);
            const int oa = __shfl_xor(arg, o);
            if (ob < best || (ob == best && oa < arg)) { best = ob; arg = oa; }
        }
        if (k == 0) kcur = arg != INT_MAX ? arg : 0;
    }
    __syncthreads();                                               // also: every psi row of this workgroup is visible to it
    for (int t0 = (T - 1) / kTile * kTile; t0 >= 0; t0 -= kTile) {
        const int rows = min(kTile, T - t0);
        const uint4* src = reinterpret_cast<const uint4*>(psi + (long long)t0 * kThreads);
        for (int i = k; i < rows * (kThreads / 16); i += kThreads) reinterpret_cast<uint4*>(ps)[i] = src[i];
        __syncthreads();
        if (k == 0) {
            int kk = kcur;
            for (int r = rows - 1; r >= 0; --r) {
                ks[r] = kk;
                kk = min((int)ps[r * kThreads + kk], n - 1);       // k*[t - 1] = psi[t, k*[t]]; row 0 holds zeros
            }
            kcur = kk;
        }
        __syncthreads();
        if (k < rows) {
            const int t = t0 + k, ts = lo + ks[k];
            const long long row = (long long)b * p.T_max + t;
            const float* __restrict__ d = dp + (long long)t * (kMaxLag + 1);
            const float c0 = d[ts];
            float f = 0.0f;
            if (c0 < p.threshold) {
                float delta = 0.0f;
                if (ts - 1 >= 1 && ts + 1 <= hi) {
                    const float a = d[ts - 1], c = d[ts + 1];
                    const float den = __fadd_rn(__fsub_rn(a, __fmul_rn(2.0f, c0)), c);
                    if (den > 0.0f) delta = __fdiv_rn(__fsub_rn(a, c), __fmul_rn(2.0f, den));
                }
                f = __fdiv_rn((float)p.sample_rate, __fadd_rn((float)ts, delta));
            }
            p.f0[row] = f;
            if (p.cmnd) p.cmnd[row] = c0;
            if (p.lag) p.lag[row] = ts;
        }
        __syncthreads();                                           // ps and ks are reused by the next tile
    }
}

static bool f0_track_ok(const F0TrackP& q) {
    const F0P& p = q.y;
    return p.B <= 65535 && p.hop >= 1 && p.hop <= kFrame && p.max_len >= 1 && p.max_len <= p.L_max && p.T_max >= 1 + p.max_len / p.hop &&
           p.lag_min >= 2 && p.lag_min < p.lag_max && p.lag_max <= kMaxLag && p.f0 != nullptr && q.lg != nullptr && q.dprime != nullptr &&
           q.psi != nullptr && std::isfinite(q.octave_cost) && std::isfinite(q.jump_cost) && q.octave_cost >= 0.0f && q.jump_cost >= 0.0f;
}

hipError_t launch_f0_cmnd(const F0TrackP& q, hipStream_t s) {
    if (q.y.B <= 0) return hipSuccess;
    if (!f0_track_ok(q)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f0_cmnd_kernel, dim3(q.y.T_max, q.y.B), dim3(kThreads), 0, s, q);
    return hipGetLastError();
}

hipError_t launch_f0_viterbi(const F0TrackP& q, hipStream_t s) {
    if (q.y.B <= 0) return hipSuccess;
    if (!f0_track_ok(q)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(f0_viterbi_kernel, dim3(q.y.B), dim3(kThreads), 0, s, q);
    return hipGetLastError();
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
    const double n = block_tree_sum<kThreads>(red, cnt);
    const double total = block_tree_sum<kThreads>(red, sum);
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
    const double m2 = block_tree_sum<kThreads>(red, s2) / n, m3 = block_tree_sum<kThreads>(red, s3) / n, m4 = block_tree_sum<kThreads>(red, s4) / n;
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
