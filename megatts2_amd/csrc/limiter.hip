// True-peak look-ahead limiter for a ragged batch of mono utterances (gfx950): a gain s[i] <= 1 per sample that keeps the true peak of
// G x under a ceiling, so that loudness normalisation under a ceiling reaches its target where one gain (ebu.hip) cannot.  Offline
// and symmetric; no reference counterpart.  Parity with any outside limiter and audible quality on real speech are unpinned; the
// kernels are held to the properties of the rule (s <= need <= 1, s = 1 exactly away from every crest, the ceiling) and to
// tests/limiter_ref.py.  The rule is stated in include/megatts2_hip.h; in short, with o, Z, h[p][k] and y of the true-peak rule:
//
//   H = round(sr window_ms / 1000), W = 2 H + 1;  w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (2 H + 2)) / (their sum), f32
//   e[i] = max_p |y[i o + p]| for i in [-1, L);  E[i] = max(e[i - 1], e[i])                    once a call, from x
//   a = G E[i];  need[i] = a > c ? c / a : 1 (1 outside [0, L));  m[i] = min of need over [i - H, i + H]
//   d[i] = sum_k w[k] (1 - m[i - H + k]), one f32 fma chain, k ascending;  s[i] = min(need[i], 1 - d[i]);  out[i] = (x[i] G) s[i]
//   TP' = true peak of out (ebu.hip);  t = min(1, c / TP') toward zero;  out *= t (loudness.hip's scale kernel)
//
// Kernels:
//   limiter_envelope_kernel  grid (tiles, B): the interpolator's tile of true_peak_tile.h, but five positions a thread, 4 t - 1 ..
//                            4 t + 3 of the tile, so that E of its four samples needs no neighbour; writes E to the arena
//   limiter_gain_kernel      grid (tiles, B), once a pass: need on kTile samples with a halo of 2 H each side in LDS; m by log-step
//                            doubling between two LDS buffers (min over 2^k, then two overlapping windows: an element of need, hence
//                            exact); 1 - m in LDS; the Hann chains of a thread's four samples from 16-byte LDS reads (consecutive
//                            lanes, consecutive vectors; the weights one address for the wave); d through LDS to a coalesced last
//                            phase that forms need again (the same two operations, the same bits), s and the two products; the
//                            wave's min and count merged by atomics, skipped where they cannot change the word
//   limiter_step_kernel      a thread per utterance: the pre-gain of the first pass, the trim, the next pass's pre-gain, the stats
// The max, the min and the count are order-free and every chain's order depends on the sample's index in its utterance alone, so a
// ragged batch is bit-identical to its utterances alone.  A sample at or beyond L is never read.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"
#include "true_peak_tile.h"

#include <limits.h>
#include <math.h>

#include <algorithm>
#include <vector>

namespace mt2 {

namespace {
constexpr int kTile = MT2_LIMITER_TILE, kThreads = kTpThreads, kChains = kPer + 1, kMaxH = MT2_LIMITER_MAX_HALF_WINDOW;
constexpr double kPi = 3.14159265358979323846;
static_assert(kTile == kTpTile && kTile == kThreads * kPer, "both limiter kernels work on the shared tile");

// the words of one of the gain kernel's two LDS buffers: need over the tile and its halo, and room for the zeros behind 1 - m
__host__ __device__ constexpr int gain_buffer_words(int H) { return (kTile + 4 * H + 8 + 3) & ~3; }
size_t gain_lds_bytes(int H) { return sizeof(float) * (2 * (size_t)gain_buffer_words(H) + (size_t)limiter_window_words(H)); }

// ordered like the floats (s is never a NaN), inverted: the word only grows, 0 says that no s < 1 was merged
__device__ __forceinline__ unsigned min_word(float s) {
    const unsigned u = __float_as_uint(s);
    return ~((u >> 31) ? ~u : u | 0x80000000u);
}
__device__ __forceinline__ float min_unword(unsigned w) {
    const unsigned k = ~w;
    return __uint_as_float((k >> 31) ? k ^ 0x80000000u : ~k);
}
__device__ __forceinline__ float need_of(float G, float E, float c) {
    const float a = __fmul_rn(G, E);
    return a > c ? __fdiv_rn(c, a) : 1.0f;
}
}  // namespace

int limiter_half_window(int sample_rate, double window_ms) {
    if (!std::isfinite(window_ms)) return -1;
    const double h = floor((double)sample_rate * window_ms / 1000.0 + 0.5);
    return h >= 1.0 && h <= (double)kMaxH ? (int)h : -1;
}

void limiter_window(int H, float* w) {
    const int W = 2 * H + 1;
    std::vector<double> v((size_t)W);
    double sum = 0.0;
    for (int k = 0; k < W; ++k) {
        v[k] = 0.5 - 0.5 * cos(2.0 * kPi * (double)(k + 1) / (double)(2 * H + 2));
        sum += v[k];
    }
    for (int k = 0; k < W; ++k) w[k] = (float)(v[k] / sum);
}

// samples i in [tile * kTile, (tile + 1) * kTile) of one utterance, by the tile of true_peak_tile.h: xs[q] = x[i0 - Z + q], so that the
// window of position i0 - 1 + q, x[i - Z + 1 .. i + Z], is xs[q .. q + 2 Z).  Thread t takes the five positions from q = 4 t, so that
// E of its four samples needs no neighbour.  e of a position at or beyond L is formed and dropped.
__global__ __launch_bounds__(kThreads) void limiter_envelope_kernel(LimiterP p) {
    __shared__ __attribute__((aligned(16))) float xs[kTpXsWords];
    __shared__ __attribute__((aligned(16))) float hs[kTpHsWords];
    const int b = blockIdx.y, L = p.len[b], t = threadIdx.x, o = p.o;
    const long long i0 = (long long)blockIdx.x * kTile;
    if (i0 >= L) return;                                                      // uniform over the workgroup
    tp_tile_load(xs, hs, p.wav + (long long)b * p.L_max, i0 - kZ, L, p.table, o);
    const int q0 = t * kPer;
    if (i0 + q0 >= L) return;
    const TpWindows<kChains> win(xs, q0);
    float e[kChains];
#pragma unroll
    for (int j = 0; j < kChains; ++j) {                                       // phase 0
        const float v = win.sample(j);
        e[j] = v > 0.0f ? v : 0.0f;
    }
#pragma unroll 1
    for (int ph = 1; ph < o; ++ph) {
        float a[kChains];
        win.phase(hs, ph, a);
#pragma unroll
        for (int j = 0; j < kChains; ++j)
            if (a[j] > e[j]) e[j] = a[j];                                     // a NaN never wins, an Inf does
    }
    float E[kPer];
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        E[j] = e[j];
        if (e[j + 1] > E[j]) E[j] = e[j + 1];
        if (i0 + q0 + j >= L) E[j] = 0.0f;                                    // never read: the row's last vector is written whole
    }
    *reinterpret_cast<float4*>(p.env + (long long)b * p.E_ld + i0 + q0) = make_float4(E[0], E[1], E[2], E[3]);
}

// samples i in [tile * kTile, (tile + 1) * kTile) of one utterance.  A[q] = need[i0 - 2 H + q], q in [0, kTile + 4 H);
// u[r] = 1 - m[i0 - H + r], r in [0, kTile + 2 H), zeros in the eight words behind (the weights end in up to three zeros, and
// fma(0, 0, acc) is acc);  d of sample i0 + j = sum_k w[k] u[j + k].  `out` may be the input: x[i] is read by the thread that
// writes out[i], and by no other.
__global__ __launch_bounds__(kThreads) void limiter_gain_kernel(LimiterP p) {
    extern __shared__ __attribute__((aligned(16))) float lds[];
    const int H = p.H, W = 2 * H + 1, NA = kTile + 4 * H, NM = kTile + 2 * H, NB = gain_buffer_words(H), Wp = limiter_window_words(H);
    float* cur = lds;
    float* nxt = lds + NB;
    float* ws = lds + 2 * NB;
    const int b = blockIdx.y, L = p.len[b], t = threadIdx.x;
    const long long i0 = (long long)blockIdx.x * kTile;
    const float* __restrict__ x = p.wav + (long long)b * p.L_max;
    float* __restrict__ out = p.out + (long long)b * p.out_ld;
    float* __restrict__ gain = p.gain ? p.gain + (long long)b * p.out_ld : nullptr;
    float* __restrict__ need = p.need ? p.need + (long long)b * p.out_ld : nullptr;
    if (i0 >= L || p.bypass[b]) {                                             // uniform: behind the utterance, or copied unchanged
        for (int q = t; q < kTile; q += kThreads) {
            const long long i = i0 + q;
            if (i >= p.out_ld) break;
            out[i] = i < L ? x[i] : 0.0f;
            if (gain) gain[i] = 1.0f;
            if (need) need[i] = 1.0f;
        }
        return;
    }
    const float G = p.G[b], c = p.c;
    const float* __restrict__ E = p.env + (long long)b * p.E_ld;
    for (int q = t; q < NA; q += kThreads) {
        const long long i = i0 - 2 * H + q;
        cur[q] = i >= 0 && i < L ? need_of(G, E[i], c) : 1.0f;
    }
    for (int q = t; q < Wp; q += kThreads) ws[q] = p.win[q];
    __syncthreads();
    int span = 1;                                                             // cur[q] = min of need over [q, q + span), cut at NA
    for (; 2 * span <= W; span *= 2) {
        for (int q = t; q < NA; q += kThreads) {
            float v = cur[q];
            if (q + span < NA) v = fminf(v, cur[q + span]);
            nxt[q] = v;
        }
        __syncthreads();
        float* const sw = cur; cur = nxt; nxt = sw;
    }
    for (int r = t; r < NM + 8; r += kThreads)                                // span <= W < 2 span: two windows cover [r, r + W)
        nxt[r] = r < NM ? __fsub_rn(1.0f, fminf(cur[r], cur[r + W - span])) : 0.0f;
    __syncthreads();
    {
        const float* __restrict__ u = nxt + t * kPer;
        float d[kPer] = {0.0f, 0.0f, 0.0f, 0.0f};
        float4 lo = *reinterpret_cast<const float4*>(u);
#pragma unroll 2
        for (int k = 0; k < Wp; k += 4) {
            const float4 hi = *reinterpret_cast<const float4*>(u + k + 4), w4 = *reinterpret_cast<const float4*>(ws + k);
            const float uu[7] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z}, ww[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int kk = 0; kk < 4; ++kk)
#pragma unroll
                for (int j = 0; j < kPer; ++j) d[j] = __fmaf_rn(ww[kk], uu[kk + j], d[j]);      // each chain in ascending k
            lo = hi;
        }
        *reinterpret_cast<float4*>(cur + t * kPer) = make_float4(d[0], d[1], d[2], d[3]);        // cur is read no more
    }
    __syncthreads();
    unsigned word = 0u, cnt = 0u;
#pragma unroll
    for (int r = 0; r < kPer; ++r) {
        const int q = t + r * kThreads;
        const long long i = i0 + q;
        if (i >= p.out_ld) break;
        float v = 0.0f, s = 1.0f, nd = 1.0f;
        if (i < L) {
            nd = need_of(G, E[i], c);
            s = fminf(nd, __fsub_rn(1.0f, cur[q]));
            v = __fmul_rn(__fmul_rn(x[i], G), s);
            if (s < 1.0f) {
                ++cnt;
                word = max(word, min_word(s));
            }
        }
        out[i] = v;
        if (gain) gain[i] = s;
        if (need) need[i] = nd;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        word = max(word, (unsigned)__shfl_xor((int)word, d));
        cnt += (unsigned)__shfl_xor((int)cnt, d);
    }
    if ((t & 63) == 0 && cnt > 0u) {                                          // most waves hold no limited sample
        atomicAdd(p.count + b, cnt);
        if (word > __hip_atomic_load(p.minkey + b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(p.minkey + b, word);
    }
}

// a thread per utterance
__global__ __launch_bounds__(64) void limiter_step_kernel(LimiterP p, int step) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= p.B) return;
    if (step == kLimStepInit) {
        float g = p.G_host;
        int bypass = 0;
        if (p.normalizing) {                                                  // the loudness rule's gain, and its convention for silence
            const double I = p.row18[(long long)b * MT2_EBU_FIELDS];
            g = isfinite(I) ? (float)pow(10.0, (p.target_lufs - I) / 20.0) : 1.0f;
            bypass = !isfinite(I) || !isfinite(g);
            if (bypass) g = 1.0f;
        }
        p.G[b] = g; p.bypass[b] = bypass; p.t[b] = 1.0f;
    } else if (step == kLimStepTrim) {
        const float tp = __uint_as_float(p.tp[b]);
        p.t[b] = !p.bypass[b] && tp > p.c ? __double2float_rz((double)p.c / (double)tp) : 1.0f;      // toward zero: never over the ceiling
    } else if (step == kLimStepNext) {
        const double I = p.rowk[(long long)b * 8];
        if (!p.bypass[b] && isfinite(I)) {
            const float g = (float)((double)p.G[b] * pow(10.0, (p.target_lufs - I) / 20.0));
            if (isfinite(g)) p.G[b] = g;
        }
    } else {
        double* __restrict__ o = p.stats + (long long)b * MT2_LIMITER_FIELDS;
        const double* __restrict__ row = p.row18 + (long long)b * MT2_EBU_FIELDS;
#pragma unroll
        for (int q = 0; q < MT2_EBU_FIELDS; ++q) o[q] = row[q];
        const unsigned w = p.minkey[b];
        o[7] = (double)p.G[b];
        o[18] = (double)p.H;
        o[19] = w ? (double)min_unword(w) : 1.0;
        o[20] = (double)p.count[b];
        o[21] = (double)__uint_as_float(p.tp[b]);
        o[22] = (double)p.t[b];
        o[23] = p.rowk ? p.rowk[(long long)b * 8] : nan("");
    }
}

namespace {
bool limiter_geometry_ok(const LimiterP& p) {
    return p.B >= 1 && p.B <= 65535 && p.max_len >= 1 && p.max_len <= p.L_max && p.E_ld >= p.max_len && p.E_ld % 4 == 0 && p.env != nullptr;
}
}  // namespace

hipError_t launch_limiter_envelope(const LimiterP& p, hipStream_t s) {
    if (!limiter_geometry_ok(p) || p.o < 1 || p.o > kMaxOver || p.table == nullptr) return hipErrorInvalidValue;
    const long long tiles = ((long long)p.max_len + kTile - 1) / kTile;
    hipLaunchKernelGGL(limiter_envelope_kernel, dim3((unsigned)tiles, p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_limiter_gain(const LimiterP& p, hipStream_t s) {
    if (!limiter_geometry_ok(p) || p.H < 1 || p.H > kMaxH || p.win == nullptr || p.out == nullptr || p.out_ld < p.max_len || p.G == nullptr ||
        p.bypass == nullptr || p.minkey == nullptr || p.count == nullptr)
        return hipErrorInvalidValue;
    static std::atomic<unsigned long long> done{0};                           // H = 1024 takes 49232 bytes: over the default dynamic LDS
    const hipError_t e = dyn_lds_once(done, reinterpret_cast<const void*>(limiter_gain_kernel), gain_lds_bytes(kMaxH));
    if (e != hipSuccess) return e;
    const long long tiles = ((long long)p.out_ld + kTile - 1) / kTile;       // the zeros (and ones) behind every utterance up to out_ld
    hipLaunchKernelGGL(limiter_gain_kernel, dim3((unsigned)tiles, p.B), dim3(kThreads), gain_lds_bytes(p.H), s, p);
    return hipGetLastError();
}
hipError_t launch_limiter_step(const LimiterP& p, int step, hipStream_t s) {
    if (p.B < 1 || step < kLimStepInit || step > kLimStepStats || p.G == nullptr || p.bypass == nullptr || p.t == nullptr ||
        (step == kLimStepStats && p.stats == nullptr))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(limiter_step_kernel, dim3((p.B + 63) / 64), dim3(64), 0, s, p, step);
    return hipGetLastError();
}

}  // namespace mt2
