// Seeded temperature / top-k / top-p sampling of the PLM's prosody codes: the decoding control the reference lacks (its
// loop is greedy, models/megatts2.py:165-181; greedy stays the default and the parity path - argmax_rows_kernel).
//
// The rule, for one row of N <= 1024 f32 logits z, temperature tau > 0, top_k (0 = all), top_p in (0, 1], uniform u:
//   rank order  value descending, then index ascending (decided on the f32 z themselves);
//   K           the first top_k entries in rank order (all N when top_k = 0);
//   w_i         exp((z_i - z_max) / tau) on K (w = 1 at the maximum, so sum_K w >= 1);
//   R           the shortest rank-order prefix of K with sum_R w >= top_p * sum_K w;
//   draw        walk R in ASCENDING INDEX order and pick the first i whose running sum is > u * sum_R w (the last index of
//               R when rounding leaves none).
// u = (x0 >> 8) * 2^-24 with x0 the first word of Philox4x32-10 (key = the utterance's 64-bit seed, counter = (target
// position, 0, 0, 0)): a code depends on (seed, position, logits) only - not on the batch, the slot, the stream groups or
// a repeated call.  top_k = 1 (or a tiny top_p) is exactly the argmax with lowest-index ties on rows without NaN; the rule does not
// order NaN logits (argmax_rows_kernel's NaN-is-greatest rule is the greedy path's alone).
//
// One wave64 per row, four rows per 256-thread block (as argmax_rows_kernel); lane l owns logits [16 l, 16 l + 16), so an
// index-order prefix sum is a per-lane partial sum plus a wave scan.  The top-k cut is a bisection over order-preserving
// u32 keys of z (ballot / popcount counts, index tie-break by a lane scan), the top-p cut a bisection over the f32 bit
// patterns of w (w >= 0: the patterns order like the values) with wave sums.  No LDS, no scratch.
#include "mt2_kernels.h"
#include "philox.h"
#include <math.h>

namespace mt2 {
namespace {

constexpr int kPer = 16;           // logits per lane
constexpr int kMaxN = 64 * kPer;   // one wave covers the row

// larger value <-> larger key; -0 and +0 are one value
__device__ __forceinline__ uint32_t order_key(float z) {
    uint32_t b = __float_as_uint(z);
    if (z == 0.0f) b = 0u;
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

// xor butterflies: every lane ends with the same value
__device__ __forceinline__ float wave_sum_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max_f(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}
// inclusive prefix over lanes 0..lane
__device__ __forceinline__ int lane_scan_i(int v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    return v;
}
__device__ __forceinline__ float lane_scan_f(float v, int lane) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const float y = __shfl_up(v, o);
        if (lane >= o) v += y;
    }
    return v;
}

// Bit e of the result: this lane's element e is among the first k elements of `mask` (bit e per element) in rank order
// (key descending, index ascending).  1 <= k <= the number of masked elements of the wave.  T ends as the k-th largest key.
__device__ __forceinline__ uint32_t select_first_k(const uint32_t (&key)[kPer], uint32_t mask, int k, int lane) {
    uint32_t T = 0u;
    for (int bit = 31; bit >= 0; --bit) {
        const uint32_t cand = T | (1u << bit);
        int c = 0;
#pragma unroll
        for (int e = 0; e < kPer; ++e) c += wave_count(((mask >> e) & 1u) && key[e] >= cand);
        if (c >= k) T = cand;
    }
    int gt = 0, eq = 0;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const bool m = (mask >> e) & 1u;
        gt += wave_count(m && key[e] > T);
        eq += (m && key[e] == T) ? 1 : 0;
    }
    const int need = k - gt;                       // ties at T taken in index order
    int r = lane_scan_i(eq, lane) - eq;
    uint32_t in = 0u;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        const bool m = (mask >> e) & 1u;
        if (m && key[e] > T) in |= 1u << e;
        else if (m && key[e] == T) {
            if (r < need) in |= 1u << e;
            ++r;
        }
    }
    return in;
}

__global__ __launch_bounds__(256) void sample_rows_kernel(const float* __restrict__ x, int ldx, int N, int64_t* out, int ostride,
                                                          int ooff, int A, float tau, int top_k, float top_p,
                                                          const uint32_t* __restrict__ seeds, const int* __restrict__ slot,
                                                          const int* __restrict__ pos, int pos0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 4 + wave;
    if (j >= A) return;
    const float* xr = x + (long long)j * ldx;
    const int n0 = lane * kPer;
    float z[kPer];
    uint32_t valid = 0u;
    if (((ldx & 3) == 0) && n0 + kPer <= N) {      // four float4 loads in flight per lane
#pragma unroll
        for (int q = 0; q < kPer / 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(xr + n0 + 4 * q);
            z[4 * q] = v.x; z[4 * q + 1] = v.y; z[4 * q + 2] = v.z; z[4 * q + 3] = v.w;
        }
        valid = 0xffffu;
    } else {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const bool ok = n0 + e < N;
            z[e] = ok ? xr[n0 + e] : -INFINITY;
            valid |= ok ? (1u << e) : 0u;
        }
    }
    float zmax = -INFINITY;
    uint32_t key[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        zmax = fmaxf(zmax, z[e]);
        key[e] = order_key(z[e]);
    }
    zmax = wave_max_f(zmax);

    // top-k
    const uint32_t inK = (top_k > 0 && top_k < N) ? select_first_k(key, valid, top_k, lane) : valid;
    float w[kPer];
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        w[e] = ((inK >> e) & 1u) ? expf((z[e] - zmax) / tau) : 0.0f;
        s += w[e];
    }
    // top-p: the largest bit pattern T with sum(w >= T) >= top_p * sum_K w; R = the elements above T, then the first m of the
    // elements AT T in rank order (equal w may come from distinct z)
    uint32_t inR = inK;
    if (top_p < 1.0f) {
        const float target = top_p * wave_sum_f(s);
        uint32_t T = 0u;
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = T | (1u << bit);
            float t = 0.0f;
#pragma unroll
            for (int e = 0; e < kPer; ++e) t += __float_as_uint(w[e]) >= cand ? w[e] : 0.0f;
            if (wave_sum_f(t) >= target) T = cand;
        }
        if (T != 0u) {
            const float wT = __uint_as_float(T);
            float above = 0.0f;
            uint32_t gt = 0u, eq = 0u;
            int m_eq = 0;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                const uint32_t b = __float_as_uint(w[e]);
                const bool k_ = (inK >> e) & 1u;
                if (k_ && b > T) { gt |= 1u << e; above += w[e]; }
                if (k_ && b == T) eq |= 1u << e;
                m_eq += wave_count(k_ && b == T);
            }
            above = wave_sum_f(above);
            const float need = ceilf((target - above) / wT);
            const int m = need < 1.0f ? 1 : (need >= (float)m_eq ? m_eq : (int)need);
            inR = gt | (m >= m_eq ? eq : select_first_k(key, eq, m, lane));
        }
    }

    // the draw: u * sum_R w against the running sum of R in index order
    const int b = slot ? slot[j] : j;
    const uint32_t ctr = (uint32_t)(pos ? pos[j] : pos0);
    const uint32_t x0 = philox_x0(ctr, 0u, 0u, 0u, seeds[2 * b], seeds[2 * b + 1]);
    const float u = (float)(x0 >> 8) * (1.0f / 16777216.0f);
    float part = 0.0f;
#pragma unroll
    for (int e = 0; e < kPer; ++e) part += ((inR >> e) & 1u) ? w[e] : 0.0f;
    const float incl = lane_scan_f(part, lane);
    const float S = __shfl(incl, 63);
    const float thr = u * S;
    float run = __shfl_up(incl, 1);
    if (lane == 0) run = 0.0f;
    int pick = 0x7fffffff, last = -1;
#pragma unroll
    for (int e = 0; e < kPer; ++e)
        if ((inR >> e) & 1u) {
            run += w[e];
            if (pick == 0x7fffffff && run > thr) pick = n0 + e;
            last = n0 + e;
        }
    pick = wave_min_i(pick);
    if (pick == 0x7fffffff) pick = wave_max_i(last);
    if (lane == 0) out[(long long)j * ostride + ooff] = pick;
}

// ---- prosody interpolation: the draw on a MIXTURE of two rows (Mega-TTS 2, section 3.3; rule in include/megatts2_hip.h).
//   wA_i = exp((zA_i - max zA) / tau), SA = sum wA (same for B);  m_i = (1 - gamma) * wA_i / SA + gamma * wB_i / SB
// and the single-row rule's cuts and draw run on m: rank order = m descending, index ascending - decided on the computed f32 m,
// NOT on the logits (two logit rows have no order of their own) -, K = the first top_k, R = the shortest rank-order prefix of K
// with sum_R m >= top_p * sum_K m, the draw walks R in index order.  GREEDY: the arg-max of m at tau = 1, lowest index on
// ties, no cut and no u.  One wave64 per PAIR (rows 2j and 2j + 1 of x), the same lane layout, select_first_k over
// order_key(m), the same bit-pattern bisection (m >= 0) and lane scan as sample_rows_kernel; the code goes to both histories.
template <bool GREEDY>
__global__ __launch_bounds__(256) void sample_mix_rows_kernel(const float* __restrict__ x, int ldx, int N, int64_t* out, int ostride,
                                                              int ooff, int A, float tau, int top_k, float top_p,
                                                              const uint32_t* __restrict__ seeds, const int* __restrict__ slot,
                                                              const int* __restrict__ pos, int pos0,
                                                              const float* __restrict__ gamma) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 4 + wave;
    if (j >= A) return;
    const float* xa = x + (long long)(2 * j) * ldx;
    const float* xb = xa + ldx;
    const int n0 = lane * kPer;
    const int b = slot ? slot[j] : j;
    const float g = gamma[b];
    float za[kPer], zb[kPer];
    uint32_t valid = 0u;
    if (((ldx & 3) == 0) && n0 + kPer <= N) {      // eight float4 loads in flight per lane
#pragma unroll
        for (int q = 0; q < kPer / 4; ++q) {
            const float4 v = *reinterpret_cast<const float4*>(xa + n0 + 4 * q);
            za[4 * q] = v.x; za[4 * q + 1] = v.y; za[4 * q + 2] = v.z; za[4 * q + 3] = v.w;
            const float4 t = *reinterpret_cast<const float4*>(xb + n0 + 4 * q);
            zb[4 * q] = t.x; zb[4 * q + 1] = t.y; zb[4 * q + 2] = t.z; zb[4 * q + 3] = t.w;
        }
        valid = 0xffffu;
    } else {
#pragma unroll
        for (int e = 0; e < kPer; ++e) {
            const bool ok = n0 + e < N;
            za[e] = ok ? xa[n0 + e] : -INFINITY;
            zb[e] = ok ? xb[n0 + e] : -INFINITY;
            valid |= ok ? (1u << e) : 0u;
        }
    }
    float amax = -INFINITY, bmax = -INFINITY;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        amax = fmaxf(amax, za[e]);
        bmax = fmaxf(bmax, zb[e]);
    }
    amax = wave_max_f(amax);
    bmax = wave_max_f(bmax);
    float sa = 0.0f, sb = 0.0f;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {               // (-inf behind N: exp = 0)
        za[e] = expf((za[e] - amax) / tau);
        zb[e] = expf((zb[e] - bmax) / tau);
        sa += za[e];
        sb += zb[e];
    }
    const float ca = (1.0f - g) / wave_sum_f(sa), cb = g / wave_sum_f(sb);      // SA, SB >= 1: w = 1 at each row's maximum
    float m[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) m[e] = ca * za[e] + cb * zb[e];             // an end point (gamma 0 or 1) leaves the other row out: 0 * w

    if (GREEDY) {
        float best = -1.0f;
        int at = 0x7fffffff;
#pragma unroll
        for (int e = 0; e < kPer; ++e)
            if (((valid >> e) & 1u) && m[e] > best) { best = m[e]; at = n0 + e; }
        const float top = wave_max_f(best);
        int pick = wave_min_i(best == top ? at : 0x7fffffff);
        if (pick == 0x7fffffff) pick = 0;          // a NaN row has no order (as in sample_rows_kernel): any in-range code
        if (lane == 0) {
            out[(long long)(2 * j) * ostride + ooff] = pick;
            out[(long long)(2 * j + 1) * ostride + ooff] = pick;
        }
        return;
    }

    uint32_t key[kPer];
#pragma unroll
    for (int e = 0; e < kPer; ++e) key[e] = order_key(m[e]);
    // top-k on m
    const uint32_t inK = (top_k > 0 && top_k < N) ? select_first_k(key, valid, top_k, lane) : valid;
    float s = 0.0f;
#pragma unroll
    for (int e = 0; e < kPer; ++e) {
        m[e] = ((inK >> e) & 1u) ? m[e] : 0.0f;
        s += m[e];
    }
    // top-p: as in sample_rows_kernel, on the bit patterns of m; elements AT the threshold are equal in m, so their rank order is
    // the index order select_first_k gives equal keys
    uint32_t inR = inK;
    if (top_p < 1.0f) {
        const float target = top_p * wave_sum_f(s);
        uint32_t T = 0u;
        for (int bit = 30; bit >= 0; --bit) {
            const uint32_t cand = T | (1u << bit);
            float t = 0.0f;
#pragma unroll
            for (int e = 0; e < kPer; ++e) t += __float_as_uint(m[e]) >= cand ? m[e] : 0.0f;
            if (wave_sum_f(t) >= target) T = cand;
        }
        if (T != 0u) {
            const float mT = __uint_as_float(T);
            float above = 0.0f;
            uint32_t gt = 0u, eq = 0u;
            int n_eq = 0;
#pragma unroll
            for (int e = 0; e < kPer; ++e) {
                const uint32_t bits = __float_as_uint(m[e]);
                const bool k_ = (inK >> e) & 1u;
                if (k_ && bits > T) { gt |= 1u << e; above += m[e]; }
                if (k_ && bits == T) eq |= 1u << e;
                n_eq += wave_count(k_ && bits == T);
            }
            above = wave_sum_f(above);
            const float need = ceilf((target - above) / mT);
            const int take = need < 1.0f ? 1 : (need >= (float)n_eq ? n_eq : (int)need);
            inR = gt | (take >= n_eq ? eq : select_first_k(key, eq, take, lane));
        }
    }

    // the draw: u * sum_R m against the running sum of R in index order
    const uint32_t ctr = (uint32_t)(pos ? pos[j] : pos0);
    const uint32_t x0 = philox_x0(ctr, 0u, 0u, 0u, seeds[2 * b], seeds[2 * b + 1]);
    const float u = (float)(x0 >> 8) * (1.0f / 16777216.0f);
    float part = 0.0f;
#pragma unroll
    for (int e = 0; e < kPer; ++e) part += ((inR >> e) & 1u) ? m[e] : 0.0f;
    const float incl = lane_scan_f(part, lane);
    const float S = __shfl(incl, 63);
    const float thr = u * S;
    float run = __shfl_up(incl, 1);
    if (lane == 0) run = 0.0f;
    int pick = 0x7fffffff, last = -1;
#pragma unroll
    for (int e = 0; e < kPer; ++e)
        if ((inR >> e) & 1u) {
            run += m[e];
            if (pick == 0x7fffffff && run > thr) pick = n0 + e;
            last = n0 + e;
        }
    pick = wave_min_i(pick);
    if (pick == 0x7fffffff) pick = wave_max_i(last);
    if (lane == 0) {
        out[(long long)(2 * j) * ostride + ooff] = pick;
        out[(long long)(2 * j + 1) * ostride + ooff] = pick;
    }
}

}  // namespace

hipError_t launch_sample_rows(const float* x, int ldx, int N, int64_t* out, int ostride, int ooff, int A, float tau, int top_k,
                              float top_p, const uint32_t* seeds, const int* slot, const int* pos, int pos0, hipStream_t s) {
    if (A <= 0) return hipSuccess;
    if (N < 1 || N > kMaxN || ldx < N || !(tau > 0.0f) || top_k < 0 || top_k > N || !(top_p > 0.0f && top_p <= 1.0f) ||
        !seeds)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_rows_kernel, dim3((A + 3) / 4), dim3(256), 0, s, x, ldx, N, out, ostride, ooff, A, tau, top_k,
                       top_p, seeds, slot, pos, pos0);
    return hipGetLastError();
}

hipError_t launch_sample_mix_rows(const float* x, int ldx, int N, int64_t* out, int ostride, int ooff, int A, bool greedy, float tau,
                                  int top_k, float top_p, const uint32_t* seeds, const int* slot, const int* pos, int pos0,
                                  const float* gamma, hipStream_t s) {
    if (A <= 0) return hipSuccess;
    if (N < 1 || N > kMaxN || ldx < N || !gamma) return hipErrorInvalidValue;
    if (greedy) {
        hipLaunchKernelGGL(sample_mix_rows_kernel<true>, dim3((A + 3) / 4), dim3(256), 0, s, x, ldx, N, out, ostride, ooff, A, 1.0f, 0,
                           1.0f, nullptr, slot, nullptr, 0, gamma);
        return hipGetLastError();
    }
    if (!(tau > 0.0f) || top_k < 0 || top_k > N || !(top_p > 0.0f && top_p <= 1.0f) || !seeds) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sample_mix_rows_kernel<false>, dim3((A + 3) / 4), dim3(256), 0, s, x, ldx, N, out, ostride, ooff, A, tau, top_k,
                       top_p, seeds, slot, pos, pos0, gamma);
    return hipGetLastError();
}

}  // namespace mt2
