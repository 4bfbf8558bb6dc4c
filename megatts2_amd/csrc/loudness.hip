// Integrated loudness by ITU-R BS.1770-4 (what EBU R 128 builds on) and loudness normalisation of a ragged batch (gfx950).  No
// reference counterpart - the reference peak-normalises its prompts and leaves the output level alone.  Parity with pyloudnorm /
// libebur128 is unpinned; the kernels are held to the standard's own figures and to tests/loudness_ref.py.  The rule is stated in
// include/megatts2_hip.h; in short, for one utterance x[0 .. L) at an integer sample rate sr (a multiple of 10):
//
//   h = sr / 10 (100 ms),  ns = L / h complete sub-blocks,  nb = max(0, ns - 3) blocks of 400 ms every 100 ms
//   y = highpass(shelf((double)x)), two biquads in transposed direct form II, in double, zero state in front of sample 0
//   S[j] = sum of y[i]^2 over sub-block j;  z[k] = (((S[k] + S[k+1]) + S[k+2]) + S[k+3]) / (4 h);  l[k] = -0.691 + 10 log10 z[k]
//   Gamma = -0.691 + 10 log10(mean of z over l > -70) - 10;  I = -0.691 + 10 log10(mean of z over l > -70 and l > Gamma)
//
// The recurrence is serial, the clip is long.  The cascade is a linear system with a 4-vector state, so for a chunk of c samples
// state_out = M state_in + (the state the chunk reaches from zero), M = A^c.  The chunk IS the sub-block (c = h, which depends on the
// rate alone), M is built on the host, and the filter runs in three launches:
//   1  loudness_zero_state_kernel   a thread per chunk runs its h samples from zero state -> the state it ends in;  the sample peak
//   2  loudness_carry_kernel        a wave per utterance carries the states chunk to chunk: e[j + 1] = M e[j] + zero[j], e[0] = 0
//   3  loudness_sums_kernel         a thread per chunk runs its samples again from e[j] -> S[j]
// then loudness_gate_kernel (a workgroup per utterance: blocks, both gates, the gain, the eight doubles) and, for the normalising
// call, loudness_scale_kernel, which reads the gain from the device word.
//
// Every arithmetic order is a function of the sample's, chunk's or block's index in its utterance alone (a chunk is one fma chain in
// ascending samples; thread i of the gate kernel sums the blocks i, i + 256, ... ascending and the 256 partial sums meet in a fixed
// tree).  Neither the slot, L_max, the batch size nor the grid enters, so a ragged batch is bit-identical to its utterances alone.
// A sample at or beyond L is never read.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <limits.h>
#include <math.h>

#include <algorithm>

namespace mt2 {

namespace {
constexpr int kChunkThreads = 64;        // chunks of one utterance per workgroup of kernels 1 and 3: one wave, so 5 workgroups on 5 CUs
                                         // share the 300 chunk streams of a 30 s clip and each keeps its 64 open cache lines to itself
constexpr int kGateThreads = 256;
constexpr int kGroup = 8;                // samples loaded ahead of the recurrence that consumes them
constexpr double kPi = 3.14159265358979323846;

// one step of the cascade: shelf, then high-pass, each y = b0 v + s1; s1 = b1 v - a1 y + s2; s2 = b2 v - a2 y.  c = b0 b1 b2 a1 a2
// of the shelf, then of the high-pass; st = s1 s2 of the shelf, s1 s2 of the high-pass.  __host__ too: the carry matrix is made of it.
__host__ __device__ __forceinline__ double kweight_step(const double* __restrict__ c, double* __restrict__ st, double v) {
    const double y1 = fma(c[0], v, st[0]);
    st[0] = fma(-c[3], y1, fma(c[1], v, st[1]));
    st[1] = fma(-c[4], y1, c[2] * v);
    const double y2 = fma(c[5], y1, st[2]);
    st[2] = fma(-c[8], y2, fma(c[6], y1, st[3]));
    st[3] = fma(-c[9], y2, c[7] * y1);
    return y2;
}

// the samples [i0, i1) of one utterance through the cascade from the state in st, i1 <= L;  -> sum of y^2 as one fma chain in
// ascending samples, and max |x| (fmaxf: a NaN never wins).  The loads of a group stand in front of its recurrence.
__device__ __forceinline__ double run_chunk(const float* __restrict__ x, int i0, int i1, const double* __restrict__ c, double* st,
                                            float* peak) {
    double acc = 0.0;
    float pk = 0.0f;
    int i = i0;
    for (; i + kGroup <= i1; i += kGroup) {
        float v[kGroup];
#pragma unroll
        for (int q = 0; q < kGroup; ++q) v[q] = x[i + q];
#pragma unroll
        for (int q = 0; q < kGroup; ++q) {
            pk = fmaxf(pk, fabsf(v[q]));
            const double y = kweight_step(c, st, (double)v[q]);
            acc = fma(y, y, acc);
        }
    }
    for (; i < i1; ++i) {
        const float v = x[i];
        pk = fmaxf(pk, fabsf(v));
        const double y = kweight_step(c, st, (double)v);
        acc = fma(y, y, acc);
    }
    *peak = pk;
    return acc;
}

__device__ __forceinline__ double lane_double(double v, int src) {
    // src is wave-uniform: a lane read, no LDS traffic
    const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
    return __hiloint2double(hi, lo);
}
}  // namespace

bool loudness_rate_ok(int sample_rate) { return sample_rate >= 8000 && sample_rate <= 192000 && sample_rate % 10 == 0; }

void loudness_coeffs(int sample_rate, double* c) {
    const double sr = (double)sample_rate;
    {   // shelf
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(kPi * f0 / sr), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
        c[0] = (Vh + Vb * K / Q + K * K) / a0;
        c[1] = 2.0 * (K * K - Vh) / a0;
        c[2] = (Vh - Vb * K / Q + K * K) / a0;
        c[3] = 2.0 * (K * K - 1.0) / a0;
        c[4] = (1.0 - K / Q + K * K) / a0;
    }
    {   // high-pass
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(kPi * f0 / sr), a0 = 1.0 + K / Q + K * K;
        c[5] = 1.0;
        c[6] = -2.0;
        c[7] = 1.0;
        c[8] = 2.0 * (K * K - 1.0) / a0;
        c[9] = (1.0 - K / Q + K * K) / a0;
    }
}

// M = A^h, row-major: column k is the state the cascade reaches in h steps of zero input from the unit state e_k - the very
// arithmetic the kernels run, so the chunked form and the serial one differ by rounding alone
void loudness_carry_matrix(const double* c, int h, double* M) {
    for (int k = 0; k < 4; ++k) {
        double st[4] = {0.0, 0.0, 0.0, 0.0};
        st[k] = 1.0;
        for (int i = 0; i < h; ++i) (void)kweight_step(c, st, 0.0);
        for (int r = 0; r < 4; ++r) M[4 * r + k] = st[r];
    }
}

// 1: the zero-state end state of every complete chunk, and the utterance's sample peak (the tail behind the last complete chunk
// included: thread ns takes it, for the peak alone)
__global__ __launch_bounds__(kChunkThreads) void loudness_zero_state_kernel(LoudnessP p) {
    const int b = blockIdx.y, L = p.len[b], h = p.h, ns = L / h;
    const int j = blockIdx.x * kChunkThreads + threadIdx.x;
    float pk = 0.0f;
    if (j <= ns && (long long)j * h < L) {
        const float* __restrict__ x = p.wav + (long long)b * p.L_max;
        double st[4] = {0.0, 0.0, 0.0, 0.0};
        const int i0 = j * h;
        (void)run_chunk(x, i0, j < ns ? i0 + h : L, p.c, st, &pk);
        if (j < ns) {
            double2* __restrict__ out = reinterpret_cast<double2*>(p.state + ((long long)b * p.NS + j) * 4);
            out[0] = make_double2(st[0], st[1]);
            out[1] = make_double2(st[2], st[3]);
        }
    }
    wave_peak_merge<false>(pk, p.peak + b);
}

// 2: state[b, j] (the zero-state end of chunk j) becomes the state chunk j is ENTERED with.  One wave per utterance: 64 chunks are
// loaded at once, then walked in order with the lane's values broadcast - every lane runs the same chain, lane t keeps the entry of
// chunk base + t.  e' [r] = fma chain over M[r][0..3] in that order, started from zero[r].
__global__ __launch_bounds__(64) void loudness_carry_kernel(LoudnessP p) {
    const int b = blockIdx.x, lane = threadIdx.x, ns = p.len[b] / p.h;
    const double* __restrict__ Mp = reinterpret_cast<const double*>(p.M);
    double M[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) M[q] = Mp[q];
    double e0 = 0.0, e1 = 0.0, e2 = 0.0, e3 = 0.0;
    for (int base = 0; base < ns; base += 64) {
        const int j = base + lane;
        double2* __restrict__ row = reinterpret_cast<double2*>(p.state + ((long long)b * p.NS + j) * 4);
        double2 za = make_double2(0.0, 0.0), zb = za;
        if (j < ns) { za = row[0]; zb = row[1]; }
        double m0 = 0.0, m1 = 0.0, m2 = 0.0, m3 = 0.0;
        const int n = min(64, ns - base);                                     // wave-uniform
        for (int t = 0; t < n; ++t) {
            if (lane == t) { m0 = e0; m1 = e1; m2 = e2; m3 = e3; }
            const double z0 = lane_double(za.x, t), z1 = lane_double(za.y, t), z2 = lane_double(zb.x, t), z3 = lane_double(zb.y, t);
            const double n0 = fma(M[3], e3, fma(M[2], e2, fma(M[1], e1, fma(M[0], e0, z0))));
            const double n1 = fma(M[7], e3, fma(M[6], e2, fma(M[5], e1, fma(M[4], e0, z1))));
            const double n2 = fma(M[11], e3, fma(M[10], e2, fma(M[9], e1, fma(M[8], e0, z2))));
            const double n3 = fma(M[15], e3, fma(M[14], e2, fma(M[13], e1, fma(M[12], e0, z3))));
            e0 = n0; e1 = n1; e2 = n2; e3 = n3;
        }
        if (j < ns) { row[0] = make_double2(m0, m1); row[1] = make_double2(m2, m3); }
    }
}

// 3: S[b, j] of every complete chunk from its true entry state
__global__ __launch_bounds__(kChunkThreads) void loudness_sums_kernel(LoudnessP p) {
    const int b = blockIdx.y, L = p.len[b], h = p.h, ns = L / h;
    const int j = blockIdx.x * kChunkThreads + threadIdx.x;
    if (j >= ns) return;
    const double2* __restrict__ in = reinterpret_cast<const double2*>(p.state + ((long long)b * p.NS + j) * 4);
    const double2 a = in[0], c = in[1];
    double st[4] = {a.x, a.y, c.x, c.y};
    float pk;
    p.sums[(long long)b * p.NS + j] = run_chunk(p.wav + (long long)b * p.L_max, j * h, j * h + h, p.c, st, &pk);
}

namespace {
__device__ __forceinline__ double block_loudness(const double* __restrict__ S, int k, double inv4h, double* z) {
    *z = (((S[k] + S[k + 1]) + S[k + 2]) + S[k + 3]) * inv4h;
    return -0.691 + 10.0 * log10(*z);
}
}  // namespace

// blocks, both gates, the gain and the eight doubles of one utterance.  A block is over a gate unless l <= gate: a NaN block counts,
// so that a non-finite sample makes its utterance's loudness NaN, as the serial recurrence would.
__global__ __launch_bounds__(kGateThreads) void loudness_gate_kernel(LoudnessP p) {
    __shared__ double sv[kGateThreads];
    __shared__ int sn[kGateThreads];
    const int b = blockIdx.x, t = threadIdx.x, ns = p.len[b] / p.h, nb = ns > 3 ? ns - 3 : 0;
    const double* __restrict__ S = p.sums + (long long)b * p.NS;
    const double inv4h = 1.0 / (4.0 * (double)p.h), ninf = -HUGE_VAL;
    double sum = 0.0, lmax = ninf;
    int cnt = 0;
    for (int k = t; k < nb; k += kGateThreads) {
        double z;
        const double l = block_loudness(S, k, inv4h, &z);
        if (p.momentary) p.momentary[(long long)b * p.NB_max + k] = l;
        lmax = fmax(lmax, l);
        if (!(l <= -70.0)) { sum += z; ++cnt; }
    }
    if (p.momentary)
        for (int k = nb + t; k < p.NB_max; k += kGateThreads) p.momentary[(long long)b * p.NB_max + k] = ninf;
    block_tree_sum<kGateThreads>(sv, sn, &sum, &cnt);
    const int n_abs = cnt;
    const double gamma = n_abs > 0 ? -0.691 + 10.0 * log10(sum / (double)n_abs) - 10.0 : ninf;
    sum = 0.0; cnt = 0;
    for (int k = t; k < nb; k += kGateThreads) {
        double z;
        const double l = block_loudness(S, k, inv4h, &z);
        if (!(l <= -70.0) && !(l <= gamma)) { sum += z; ++cnt; }
    }
    block_tree_sum<kGateThreads>(sv, sn, &sum, &cnt);
    lmax = block_tree_max<kGateThreads>(sv, lmax);
    if (t != 0) return;
    const double I = cnt > 0 ? -0.691 + 10.0 * log10(sum / (double)cnt) : ninf;
    const float peak = __uint_as_float(p.peak[b]);
    float g = 1.0f;
    if (p.gain) {
        if (isfinite(I)) {
            double gd = pow(10.0, (p.target_lufs - I) / 20.0);
            const bool capped = p.peak_ceiling > 0.0 && peak > 0.0f && p.peak_ceiling / (double)peak < gd;
            if (capped) gd = p.peak_ceiling / (double)peak;
            g = (float)gd;
            // a ceiling that binds holds for the f32 product the scale kernel forms, and g is the largest f32 for which it does
            if (p.peak_ceiling > 0.0 && isfinite(g)) {
                for (int q = 0; q < 4 && g > 0.0f && (double)__fmul_rn(peak, g) > p.peak_ceiling; ++q) g = __uint_as_float(__float_as_uint(g) - 1u);
                for (int q = 0; capped && q < 4; ++q) {
                    const float up = __uint_as_float(__float_as_uint(g) + 1u);
                    if (!(isfinite(up) && (double)__fmul_rn(peak, up) <= p.peak_ceiling)) break;
                    g = up;
                }
            }
            if (!isfinite(g)) g = 1.0f;
        }
        p.gain[b] = g;
    }
    if (p.stats) {
        double* __restrict__ o = p.stats + (long long)b * 8;
        o[0] = I; o[1] = (double)nb; o[2] = (double)n_abs; o[3] = (double)cnt; o[4] = gamma; o[5] = (double)peak; o[6] = lmax; o[7] = (double)g;
    }
}

// out[b, i] = x[b, i] * gain[b] (one f32 product; an exact copy where the gain is 1) for i < len[b], zeros up to L_max; out may be x
__global__ __launch_bounds__(256) void loudness_scale_kernel(LoudnessP p) {
    const int b = blockIdx.y, L = p.len[b];
    const float g = p.gain[b];
    const float* __restrict__ x = p.wav + (long long)b * p.L_max;
    float* __restrict__ out = p.out + (long long)b * p.L_max;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < p.L_max; i += (long long)gridDim.x * 256) {
        float v = 0.0f;
        if (i < L) {
            v = x[i];
            if (g != 1.0f) v = __fmul_rn(v, g);
        }
        out[i] = v;
    }
}

hipError_t launch_loudness_filter(const LoudnessP& p, hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.h < 800 || p.h > 19200 || p.max_len < 1 || p.max_len > p.L_max || p.max_len > INT_MAX - 8 * 19200 ||
        p.NS < p.max_len / p.h)
        return hipErrorInvalidValue;
    const int chunks = p.max_len / p.h + 1;          // the tail's thread included
    hipLaunchKernelGGL(loudness_zero_state_kernel, dim3((chunks + kChunkThreads - 1) / kChunkThreads, p.B), dim3(kChunkThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_loudness_carry(const LoudnessP& p, hipStream_t s) {
    if (p.max_len / p.h < 1) return hipSuccess;
    hipLaunchKernelGGL(loudness_carry_kernel, dim3(p.B), dim3(64), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_loudness_sums(const LoudnessP& p, hipStream_t s) {
    const int ns = p.max_len / p.h;
    if (ns < 1) return hipSuccess;
    hipLaunchKernelGGL(loudness_sums_kernel, dim3((ns + kChunkThreads - 1) / kChunkThreads, p.B), dim3(kChunkThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_loudness_gate(const LoudnessP& p, hipStream_t s) {
    if (p.momentary && p.NB_max < std::max(p.max_len / p.h - 3, 0)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(loudness_gate_kernel, dim3(p.B), dim3(kGateThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_loudness_scale(const LoudnessP& p, hipStream_t s) {
    if (p.out == nullptr || p.gain == nullptr) return hipErrorInvalidValue;
    const int gx = (int)std::min<long long>(((long long)p.L_max + 256 * 8 - 1) / (256 * 8), 1024);
    hipLaunchKernelGGL(loudness_scale_kernel, dim3(gx, p.B), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
