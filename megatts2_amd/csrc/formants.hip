// Formant candidates of audio by linear prediction (Markel & Gray 1976): per frame an all-pole fit by the autocorrelation method, the
// roots of its polynomial by Aberth-Ehrlich iteration (Aberth 1973, Ehrlich 1967), the roots turned into frequencies and bandwidths;
// and per utterance the formant means, the formant dispersion (Fitch 1997) and a vocal-tract length (gfx950).  The reference tree has no
// formant tracker; parity with Praat (Burg's method) is unpinned and the rule is our own statement - include/megatts2_hip.h has it in
// full, tests/formant_ref.py restates it in numpy.  In short, for one frame of W samples at offsets j = 0 .. W - 1, i = hop t - W/2 + j:
//
//   v[j]  = (x[i] - alpha x[i - 1]) w[j]        in double, three roundings; 0 where i lies outside [0, L); alpha = 0: x[i - 1] is not read
//   r[k]  = sum_j v[j] v[j + k], k = 0 .. P     lane l runs ONE chain acc = fma(v[j], v[j + k], acc) from 0 over j = l, l + 64, ... with
//                                               j + k < W, the 64 partial sums meet in the xor butterfly 32 .. 1;  r[0] *= 1 + 1e-9
//   a, e  = Levinson-Durbin on r                every operation rounded on its own (lv_* below), the dot product one chain over i ascending
//   z_k   = the roots of z^P + a1 z^(P-1) + ..  Aberth-Ehrlich from 0.9 exp(i (2 pi k / P + 0.4)), all roots updated together
//   f, bw = arg z sr / 2 pi, -ln|z| sr / pi     of the roots with Im z > 0, kept inside (fmin, sr/2 - fmin) and under max_bandwidth,
//                                               sorted by f (a tie: the smaller root index), the first five written
//
// formants_kernel: one wave per frame, four frames per workgroup.  The windowed frame v lies in LDS (8 KiB per wave, written once, then
// read only - the ONE barrier of the kernel stands between the two, at a point every wave reaches); everything behind it is wave-local
// and lives in registers: lane k holds r[k], a[k] and root k, and lanes talk by shuffles alone, so the data-dependent trip count of the
// root iteration needs no barrier.  The Levinson chain is run by every lane alike (a wave-uniform result without a broadcast); lane i
// supplies the product a[i] r[m - i].  Lanes at or beyond P idle in the root phase.  No atomics, no scratch; nothing but the frame's own
// samples enters, and every order depends on the in-frame offset alone: a ragged batch is bit-identical to its utterances alone.
// formant_stats_kernel: one workgroup per utterance, thread i sums the frames i, i + 256, ... ascending, the partial sums meet in the
// fixed tree of mt2_f0_stats; two passes, all in double.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <math.h>

namespace mt2 {

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxW = MT2_FORMANT_MAX_WINDOW, kMaxP = MT2_FORMANT_MAX_ORDER, kOut = MT2_FORMANT_MAX, kMaxIter = MT2_FORMANT_MAX_ITERS;
constexpr int kStat = MT2_FORMANT_STAT_FIELDS;
static_assert(kMaxW == 1024 && kMaxP == 32 && kMaxP < 64 && kOut == 5 && kStat == 12, "a lane owns one coefficient and one root; 16 doubles of v per lane");
constexpr double kTwoPi = 6.283185307179586476925286766559, kPi = 3.141592653589793238462643383279;

// One double operation each, never contracted: an add of a product would otherwise become one fma (one rounding where the rule has two).
__device__ __forceinline__ double lv_mul(double a, double b) {
#pragma clang fp contract(off)
    return a * b;
}
__device__ __forceinline__ double lv_add(double a, double b) {
#pragma clang fp contract(off)
    return a + b;
}
__device__ __forceinline__ double lv_sub(double a, double b) {
#pragma clang fp contract(off)
    return a - b;
}
__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_fmax(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
}  // namespace

void formant_window_table(int W, int kind, double* table) {
    for (int j = 0; j < W; ++j) table[j] = kind == MT2_FORMANT_HANN ? 0.5 - 0.5 * cos(kTwoPi * ((double)j + 0.5) / (double)W) : 1.0;
}

double formant_alpha(double preemphasis_hz, int sample_rate) {
    return preemphasis_hz > 0.0 ? exp(-kTwoPi * preemphasis_hz / (double)sample_rate) : 0.0;
}

__global__ __launch_bounds__(kThreads) void formants_kernel(FormantP p) {
    __shared__ double vs[kWaves][kMaxW];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, b = blockIdx.y;
    const long long t = (long long)blockIdx.x * kWaves + wv;
    const int L = p.len[b], T = 1 + L / p.hop, W = p.W, P = p.P;
    const bool live = t < T;                                   // wave-uniform
    double* __restrict__ v = vs[wv];
    if (live) {
        // the frame: a sample outside [0, L) is a zero by its index and is never read; x[i - 1] is read only with pre-emphasis on
        const float* __restrict__ x = p.wav + (long long)b * p.L_max;
        const long long s = (long long)p.hop * t - W / 2;
        const double alpha = p.alpha;
        for (int j = lane; j < W; j += 64) {
            const long long i = s + j;
            double y = 0.0;
            if (i >= 0 && i < L) {
                y = (double)x[i];
                if (alpha != 0.0) y = lv_sub(y, lv_mul(alpha, i >= 1 ? (double)x[i - 1] : 0.0));
                y = lv_mul(y, p.window[j]);
            }
            v[j] = y;
        }
    }
    __syncthreads();                                           // the one barrier: v is read-only from here on
    if (t >= p.T_max) return;
    const long long row = (long long)b * p.T_max + t;
    float* __restrict__ freq = p.freq + row * kOut;
    float* __restrict__ bwo = p.bw + row * kOut;
    // what an empty frame, and a frame in [T_b, T_max), leaves in the outputs of the stages it did not reach
    bool have_r = false, have_a = false, have_z = false;
    double rk = 0.0, ak = 0.0, err = 0.0, zr = 0.0, zi = 0.0;    // lane k: r[k], a[k], root k
    int iters = 0, count = 0;
    if (live) {
        iters = -1;
        // step 4: r[k] into lane k
        for (int k = 0; k <= P; ++k) {
            double acc = 0.0;
            for (int j = lane; j + k < W; j += 64) acc = fma(v[j], v[j + k], acc);
            acc = wave_sum(acc);
            if (lane == k) rk = acc;
        }
        if (lane == 0) rk = lv_mul(rk, 1.0 + 1e-9);
        have_r = true;
        const double r0 = __shfl(rk, 0);
        bool ok = r0 > 1e-300 && isfinite(r0);
        // step 5: Levinson-Durbin; every lane runs the chain, lane i holds a[i]
        if (ok) {
            double e = r0;
            ak = lane == 0 ? 1.0 : 0.0;
            for (int m = 1; m <= P; ++m) {
                const double prod = lv_mul(ak, __shfl(rk, (m - lane) & 63));      // lane i: a[i] r[m - i], used for 1 <= i < m
                double acc = __shfl(rk, m);
                for (int i = 1; i < m; ++i) acc = lv_add(acc, __shfl(prod, i));
                const double k = -acc / e;
                if (!(fabs(k) < 1.0)) { ok = false; break; }
                const double mirror = __shfl(ak, (m - lane) & 63);                // lane i: a[m - i]
                if (lane >= 1 && lane < m) ak = lv_add(ak, lv_mul(k, mirror));
                if (lane == m) ak = k;
                e = lv_mul(e, lv_sub(1.0, lv_mul(k, k)));
                if (!(e > 0.0) || !isfinite(e)) { ok = false; break; }
            }
            if (ok) ok = !__any(lane <= P && !isfinite(ak));
            if (ok) { err = e; have_a = true; } else ak = 0.0;
        }
        // step 6: Aberth-Ehrlich, lane k < P on root k
        if (ok) {
            const bool mine = lane < P;
            {
                double sn, cs;
                sincos(kTwoPi * (double)lane / (double)P + 0.4, &sn, &cs);
                zr = 0.9 * cs; zi = 0.9 * sn;
            }
            ok = false;
            for (int it = 1; it <= kMaxIter; ++it) {
                // q = p(z) / p'(z) by Horner over a[1 .. P]
                double pr = 1.0, pi = 0.0, dr = 0.0, di = 0.0;
                for (int i = 1; i <= P; ++i) {
                    const double ai = __shfl(ak, i);
                    const double ndr = dr * zr - di * zi + pr, ndi = dr * zi + di * zr + pi;
                    const double npr = pr * zr - pi * zi + ai, npi = pr * zi + pi * zr;
                    dr = ndr; di = ndi; pr = npr; pi = npi;
                }
                const double dd = dr * dr + di * di;
                const double qr = (pr * dr + pi * di) / dd, qi = (pi * dr - pr * di) / dd;
                // s = sum over j != k of 1 / (z_k - z_j), j ascending
                double sr = 0.0, si = 0.0;
                for (int j = 0; j < P; ++j) {
                    const double ur = zr - __shfl(zr, j), ui = zi - __shfl(zi, j);
                    if (j != lane) {
                        const double uu = ur * ur + ui * ui;
                        sr += ur / uu; si -= ui / uu;
                    }
                }
                // w = q / (1 - q s)
                const double cr = 1.0 - (qr * sr - qi * si), ci = -(qr * si + qi * sr);
                const double cc = cr * cr + ci * ci;
                const double wr = (qr * cr + qi * ci) / cc, wi = (qi * cr - qr * ci) / cc;
                if (mine) { zr -= wr; zi -= wi; }
                if (__any(mine && !(isfinite(wr) && isfinite(wi)))) break;
                const double big = wave_fmax(mine ? wr * wr + wi * wi : 0.0);      // the same bits in every lane: a uniform decision
                if (big < 1e-26) { ok = true; iters = it; break; }
            }
            if (ok) have_z = true; else { zr = 0.0; zi = 0.0; }
        }
        // step 7: candidates, ranked by (f, root index)
        if (ok) {
            const double srate = (double)p.sample_rate;
            double f = 0.0, bw = 0.0;
            bool keep = false;
            if (lane < P && zi > 0.0) {
                f = atan2(zi, zr) * srate / kTwoPi;
                bw = -0.5 * log(zr * zr + zi * zi) * srate / kPi;
                keep = f > p.fmin && f < 0.5 * srate - p.fmin && bw < p.max_bw;
            }
            int rank = 0, kept = 0;
            for (int j = 0; j < P; ++j) {
                const double fj = __shfl(f, j);
                const int kj = __shfl((int)keep, j);
                kept += kj;
                if (kj && (fj < f || (fj == f && j < lane))) ++rank;
            }
            count = min(kept, kOut);
            if (keep && rank < kOut) {
                freq[rank] = (float)f;
                bwo[rank] = (float)bw;
            }
        }
    }
    if (lane >= count && lane < kOut) { freq[lane] = 0.0f; bwo[lane] = 0.0f; }
    if (lane == 0) {
        p.count[row] = count;
        if (p.iters) p.iters[row] = iters;
        if (p.err) p.err[row] = have_a ? err : 0.0;
    }
    if (lane <= P) {
        if (p.autocorr) p.autocorr[row * (P + 1) + lane] = have_r ? rk : 0.0;
        if (p.lpc) p.lpc[row * (P + 1) + lane] = have_a ? ak : 0.0;
    }
    if (lane < P && p.roots) {
        p.roots[(row * P + lane) * 2] = have_z ? zr : 0.0;
        p.roots[(row * P + lane) * 2 + 1] = have_z ? zi : 0.0;
    }
}

hipError_t launch_formants(const FormantP& p, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (p.B > 65535 || p.hop < 1 || p.hop > 1024 || p.W < 64 || p.W > kMaxW || (p.W & 1) || p.P < 2 || p.P > kMaxP || (p.P & 1) || p.P >= p.W ||
        p.max_len < 1 || p.max_len > p.L_max || p.T_max < 1 + p.max_len / p.hop || !p.wav || !p.len || !p.window || !p.freq || !p.bw || !p.count)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(formants_kernel, dim3((unsigned)(((long long)p.T_max + kWaves - 1) / kWaves), p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

// stats[b] = n, n / T_b, mean F1 .. F4, sigma F1 .. F4, (mean F4 - mean F1) / 3, VTL in cm; over the frames with count >= 4 (and f0 > 0)
__global__ __launch_bounds__(kThreads) void formant_stats_kernel(const float* __restrict__ freq, const int* __restrict__ count,
                                                                 const float* __restrict__ f0, const int* __restrict__ frame_len, int T_max,
                                                                 double* __restrict__ stats) {
    __shared__ double red[kThreads];
    const int b = blockIdx.x, T = frame_len[b];
    const float* __restrict__ fr = freq + (long long)b * T_max * kOut;
    const int* __restrict__ cn = count + (long long)b * T_max;
    const float* __restrict__ fz = f0 ? f0 + (long long)b * T_max : nullptr;
    double cnt = 0.0, s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int t = threadIdx.x; t < T; t += kThreads) {
        if (cn[t] >= 4 && (!fz || fz[t] > 0.0f)) {
            cnt += 1.0;
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] += (double)fr[(long long)t * kOut + k];
        }
    }
    const double n = block_tree_sum<kThreads>(red, cnt);
    double mu[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) mu[k] = block_tree_sum<kThreads>(red, s[k]);
    double* __restrict__ out = stats + (long long)kStat * b;
    if (!(n > 0.0)) {
        if (threadIdx.x < kStat) out[threadIdx.x] = 0.0;
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) { mu[k] = mu[k] / n; s[k] = 0.0; }
    for (int t = threadIdx.x; t < T; t += kThreads) {
        if (cn[t] >= 4 && (!fz || fz[t] > 0.0f)) {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const double e = (double)fr[(long long)t * kOut + k] - mu[k];
                s[k] += e * e;
            }
        }
    }
    double m2[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) m2[k] = block_tree_sum<kThreads>(red, s[k]) / n;
    if (threadIdx.x == 0) {
        out[0] = n; out[1] = n / (double)T;
#pragma unroll
        for (int k = 0; k < 4; ++k) { out[2 + k] = mu[k]; out[6 + k] = m2[k] > 0.0 ? sqrt(m2[k]) : 0.0; }
        out[10] = (mu[3] - mu[0]) / 3.0;
        out[11] = 2187.5 * (((1.0 / mu[0] + 3.0 / mu[1]) + 5.0 / mu[2]) + 7.0 / mu[3]);
    }
}

hipError_t launch_formant_stats(const float* freq, const int* count, const float* f0, const int* frame_len, int T_max, int B, double* stats,
                                hipStream_t s) {
    if (B <= 0) return hipSuccess;
    if (B > 65535 || T_max < 1 || !freq || !count || !frame_len || !stats) return hipErrorInvalidValue;
    hipLaunchKernelGGL(formant_stats_kernel, dim3(B), dim3(kThreads), 0, s, freq, count, f0, frame_len, T_max, stats);
    return hipGetLastError();
}

}  // namespace mt2
