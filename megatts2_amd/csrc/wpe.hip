// De-reverberation of prompt audio by weighted prediction error (gfx950): single-channel WPE (Nakatani, Yoshioka, Kinoshita, Miyoshi and
// Juang 2010; Yoshioka and Nakatani 2012) between the two STFT GEMMs the library already has.  No reference counterpart.  Parity with
// nara_wpe or any other implementation is unpinned, and so is audible quality on real speech; the rule is our own, stated in
// include/megatts2_hip.h and restated in tests/wpe_ref.py.  In short, for one utterance of T frames and one bin f, everything in double:
//
//   x_k[t]  = Y[t - delay - k], 0 where the index is negative;  D = Y
//   I times:  P[t] = mean of |D[t']|^2 over the existing t' in [t - c, t + c];  w[t] = 1 / max(P[t], eps max_t P)
//             R[j][k] = sum_t x_j conj(x_k) w,  p[j] = sum_t x_j conj(Y) w;  R[j][j] += load tr(R) / K;  R = L L^H;  g = R^-1 p
//             D[t] = Y[t] - sum_k conj(g[k]) x_k[t]
//   a bin whose max P is 0 or not finite, or whose Cholesky meets a pivot that is not a positive finite number, passes through: D = Y
//
// Four kernels:
//   wpe_to_bins_kernel     grid (tiles of 32 bins, tiles of 32 frames, B), 256 threads: the frame-major spectrum [T, S] through an LDS
//                          tile into bin-major complex f32 columns [F, Tp] (Tp = T rounded up to 4, zeros behind T), 16-byte loads
//                          along the bins and 16-byte stores along the frames
//   wpe_bin_kernel         grid (F, B), 512 threads: ONE workgroup runs the whole iteration of one (utterance, bin) - no grid-wide
//                          synchronisation and no second launch per iteration.  w[] lives in LDS (8 T bytes); the column Y lives in LDS
//                          beside it when the launch's longest utterance has at most kWpeLdsFrames frames (16 T bytes in all: two
//                          workgroups a CU at 4096 frames), beyond that it streams from the bin-major scratch, which the L2 holds.  Both
//                          forms run the same instructions on the same values through one pointer: the bits cannot differ.
//                          D is never stored: |D[t']|^2 and the output recompute it from g (K products), so the only arrays are Y and w.
//                          R and p: entry e of the K (K + 1) / 2 + K is wave (e mod 8)'s; lane l adds its frames l, l + 64, ... in
//                          ascending order, then a butterfly over the 64 lanes - an order that depends on (t, T) alone.
//                          Cholesky: a column a step, lane i of wave 0 owns row i, R and L share one 16 x 16 LDS tile.  The two
//                          triangular solves: wave 0, the right-hand side in registers, a column a step, broadcast by a shuffle.
//   wpe_from_bins_kernel   the way back into [T, S] rows: 16-byte stores where a chunk lies inside the run of re or of im cells, single
//                          words at its edges - the pad columns and the frames at or beyond T are never written
//   wpe_figures_kernel     a workgroup per utterance: the bins' sums in dn_figures_kernel's order -> MT2_WPE_FIELDS doubles
// No atomics; every loop has a trip count fixed by T, K, I and c, so non-finite input can neither fault nor hang.
// Registers, from the ISA (-save-temps): wpe_bin_kernel 60 VGPRs, 104 SGPRs, no scratch and no spills at any K - the loops over K are
// not unrolled and nothing is indexed in registers; R is not Toeplitz (w varies with t) and every entry is summed.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <float.h>
#include <math.h>

namespace mt2 {

namespace {
constexpr int kTrThreads = 256, kTile = 32, kTileLd = kTile + 1, kFigThreads = 256;
constexpr int kWaves = kWpeThreads / 64;
// the fixed part of wpe_bin_kernel's LDS, in carve order; every piece a multiple of 16 bytes
constexpr size_t kFixedLds = sizeof(double2) * (kWpeMaxTaps * kWpeMaxTaps + 2 * kWpeMaxTaps) + sizeof(double) * (kWpeThreads + 2);
static_assert(kFixedLds % 16 == 0, "the arrays behind the fixed part start on 16 bytes");

__device__ __forceinline__ double wave_tree_sum(double v) {
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d);
    return v;
}

// D[t] = Y[t] - sum_k conj(g[k]) Y[t - delay - k], k ascending; the terms with a negative index are zero and are left out
__device__ __forceinline__ double2 wpe_resid(const float2* __restrict__ y, const double2* g, int t, int delay, int K, bool have) {
    const float2 v = y[t];
    double2 d = make_double2((double)v.x, (double)v.y);
    if (have) {
        double sr = 0.0, si = 0.0;
        for (int k = 0; k < K; ++k) {
            const int u = t - delay - k;
            if (u < 0) break;
            const float2 x = y[u];
            const double2 c = g[k];
            sr += c.x * (double)x.x + c.y * (double)x.y;
            si += c.x * (double)x.y - c.y * (double)x.x;
        }
        d.x -= sr;
        d.y -= si;
    }
    return d;
}
}  // namespace

size_t wpe_lds_bytes(int T_cap) {
    const size_t Tq = ((size_t)T_cap + 3) & ~size_t(3);
    return kFixedLds + sizeof(double) * Tq + (T_cap <= kWpeLdsFrames ? sizeof(float2) * Tq : 0);
}

__global__ __launch_bounds__(kTrThreads) void wpe_to_bins_kernel(WpeP p) {
    __shared__ float re[kTile * kTileLd], im[kTile * kTileLd];
    const int b = blockIdx.z, T = min(p.T[b], p.T_cap), Tp = (T + 3) & ~3, t0 = blockIdx.y * kTile, f0 = blockIdx.x * kTile, tid = threadIdx.x;
    if (t0 >= Tp) return;                                                     // uniform over the workgroup
    const int F = p.F;
    const float* __restrict__ rows = p.spec + (long long)p.row0[b] * p.lds;
    for (int i = tid; i < kTile * kTileLd; i += kTrThreads) { re[i] = 0.0f; im[i] = 0.0f; }
    __syncthreads();
    const int a0 = (F + f0) & ~3;                                             // the 16-byte chunk that holds the first im cell of the tile
    for (int i = tid; i < kTile * 17; i += kTrThreads) {                      // a frame: 8 chunks of re, 9 of im
        const int tt = i / 17, c = i - tt * 17, t = t0 + tt;
        if (t >= T) continue;
        const float* __restrict__ row = rows + (long long)t * p.lds;
        if (c < 8) {
            const int f = f0 + 4 * c;
            if (f >= F) continue;                                             // f + 3 < lds: f is a multiple of 4 below F
            const float4 v = *reinterpret_cast<const float4*>(row + f);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (f + q < F) re[tt * kTileLd + 4 * c + q] = e[q];
        } else {
            const int idx = a0 + 4 * (c - 8);
            if (idx >= p.lds) continue;                                       // lds and idx are multiples of 4: idx + 3 < lds
            const float4 v = *reinterpret_cast<const float4*>(row + idx);
            const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int fi = idx + q - F - f0;
                if (fi >= 0 && fi < kTile && f0 + fi < F) im[tt * kTileLd + fi] = e[q];
            }
        }
    }
    __syncthreads();
    float2* __restrict__ cols = p.cols + (long long)p.c0[b];
    for (int i = tid; i < kTile * (kTile / 2); i += kTrThreads) {             // a bin: 16 pairs of frames
        const int fb = i / (kTile / 2), pr = i - fb * (kTile / 2), f = f0 + fb, t = t0 + 2 * pr;
        if (f >= F || t >= Tp) continue;                                      // Tp is even: t + 1 < Tp
        const float4 v = make_float4(re[2 * pr * kTileLd + fb], im[2 * pr * kTileLd + fb], re[(2 * pr + 1) * kTileLd + fb],
                                     im[(2 * pr + 1) * kTileLd + fb]);
        *reinterpret_cast<float4*>(cols + (long long)f * Tp + t) = v;
    }
}

__global__ __launch_bounds__(kTrThreads) void wpe_from_bins_kernel(WpeP p) {
    __shared__ float re[kTile * kTileLd], im[kTile * kTileLd];
    const int b = blockIdx.z, T = min(p.T[b], p.T_cap), Tp = (T + 3) & ~3, t0 = blockIdx.y * kTile, f0 = blockIdx.x * kTile, tid = threadIdx.x;
    if (t0 >= T) return;                                                      // uniform over the workgroup
    const int F = p.F;
    const float2* __restrict__ cols = p.cols_out + (long long)p.c0[b];
    for (int i = tid; i < kTile * (kTile / 2); i += kTrThreads) {
        const int fb = i / (kTile / 2), pr = i - fb * (kTile / 2), f = f0 + fb, t = t0 + 2 * pr;
        float4 v = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (f < F && t < Tp) v = *reinterpret_cast<const float4*>(cols + (long long)f * Tp + t);
        re[2 * pr * kTileLd + fb] = v.x; im[2 * pr * kTileLd + fb] = v.y;
        re[(2 * pr + 1) * kTileLd + fb] = v.z; im[(2 * pr + 1) * kTileLd + fb] = v.w;
    }
    __syncthreads();
    float* __restrict__ rows = p.spec_out + (long long)p.row0[b] * p.lds;
    const int nf = min(kTile, F - f0);                                        // the bins of this tile: >= 1 by the grid
    for (int i = tid; i < kTile * 18; i += kTrThreads) {                      // a frame: the run of re cells and the run of im cells, 9 chunks each
        const int tt = i / 18, c = i - tt * 18, t = t0 + tt;
        if (t >= T) continue;
        const bool is_im = c >= 9;
        const int start = (is_im ? F : 0) + f0, end = start + nf, idx = (start & ~3) + 4 * (is_im ? c - 9 : c);
        if (idx >= end) continue;
        const float* src = (is_im ? im : re) + tt * kTileLd;                  // src[cell - start] for start <= cell < end
        float* __restrict__ row = rows + (long long)t * p.lds;
        const int o = idx - start;
        if (o >= 0 && idx + 3 < end) {
            *reinterpret_cast<float4*>(row + idx) = make_float4(src[o], src[o + 1], src[o + 2], src[o + 3]);
        } else {
#pragma unroll
            for (int q = 0; q < 4; ++q)
                if (o + q >= 0 && idx + q < end) row[idx + q] = src[o + q];
        }
    }
}

__global__ __launch_bounds__(kWpeThreads) void wpe_bin_kernel(WpeP p) {
    extern __shared__ __attribute__((aligned(16))) char wpe_lds[];
    double2* A = reinterpret_cast<double2*>(wpe_lds);                          // [16][16]: the lower triangle of R, then of L
    double2* pv = A + kWpeMaxTaps * kWpeMaxTaps;                               // [16]
    double2* gv = pv + kWpeMaxTaps;                                            // [16]
    double* red = reinterpret_cast<double*>(gv + kWpeMaxTaps);                 // [512]
    double* piv = red + kWpeThreads;                                           // [2]
    double* w = piv + 2;                                                       // [Tq]
    const int b = blockIdx.y, f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = min(p.T[b], p.T_cap), Tp = (T + 3) & ~3, Tq = (p.T_cap + 3) & ~3;
    const int K = p.taps, delay = p.delay, ctx = p.ctx;
    const float2* __restrict__ gcol = p.cols + (long long)p.c0[b] + (long long)f * Tp;
    const float2* y = gcol;
    if (p.T_cap <= kWpeLdsFrames) {                                            // uniform over the launch
        float2* ylds = reinterpret_cast<float2*>(w + Tq);
        for (int i = tid; i < Tp / 2; i += kWpeThreads)
            reinterpret_cast<float4*>(ylds)[i] = reinterpret_cast<const float4*>(gcol)[i];
        y = ylds;
    }
    if (tid < kWpeMaxTaps) gv[tid] = make_double2(0.0, 0.0);
    __syncthreads();

    bool pass = p.run[b] == 0, have = false;
    int done = 0;
    const int nE = K * (K + 1) / 2 + K;
    for (int it = 0; it < p.iters && !pass; ++it) {
        // steps 1 and 2: the variance, its floor, the weight
        double mx = 0.0;
        for (int t = tid; t < T; t += kWpeThreads) {
            const int lo = max(0, t - ctx), hi = min(T - 1, t + ctx);
            double s = 0.0;
            for (int q = lo; q <= hi; ++q) {
                const double2 d = wpe_resid(y, gv, q, delay, K, have);
                s += d.x * d.x + d.y * d.y;
            }
            const double P = s / (double)(hi - lo + 1);
            w[t] = P;
            mx = fmax(mx, P);
        }
        mx = block_tree_max<kWpeThreads>(red, mx);
        if (!(mx > 0.0) || !isfinite(mx)) { pass = true; break; }              // red[0]: the same in every thread
        const double lam_min = p.eps * mx;
        for (int t = tid; t < T; t += kWpeThreads) w[t] = 1.0 / fmax(w[t], lam_min);
        __syncthreads();
        // step 3: entry e = j (j + 1) / 2 + k is R[j][k], k <= j; the last K entries are p[j]
        for (int e = wave; e < nE; e += kWaves) {
            int j = 0, k = 0;
            const bool is_p = e >= nE - K;
            if (is_p) {
                j = e - (nE - K);
            } else {
                while ((j + 1) * (j + 2) / 2 <= e) ++j;
                k = e - j * (j + 1) / 2;
            }
            const int oj = delay + j, ok = is_p ? 0 : delay + k;               // x_j[t] = Y[t - oj]; the other factor is Y[t - ok]
            double sr = 0.0, si = 0.0;
            for (int t = lane; t < T; t += 64) {
                if (t < oj) continue;                                          // x_j[t] = 0 (ok <= oj)
                const float2 a = y[t - oj], c = y[t - ok];
                const double wt = w[t], ar = (double)a.x * wt, ai = (double)a.y * wt;
                sr += ar * (double)c.x + ai * (double)c.y;
                si += ai * (double)c.x - ar * (double)c.y;
            }
            sr = wave_tree_sum(sr);
            si = wave_tree_sum(si);
            if (lane == 0) {
                if (is_p) pv[j] = make_double2(sr, si);
                else A[j * kWpeMaxTaps + k] = make_double2(sr, si);
            }
        }
        __syncthreads();
        // step 4
        if (tid == 0) {
            double tr = 0.0;
            for (int j = 0; j < K; ++j) tr += A[j * kWpeMaxTaps + j].x;
            const double add = p.load * tr / (double)K;
            for (int j = 0; j < K; ++j) A[j * kWpeMaxTaps + j].x += add;
        }
        __syncthreads();
        // step 5: column j of L, lane i >= j its row
        bool bad = false;
        for (int j = 0; j < K; ++j) {
            const bool mine = tid < K && tid >= j;
            double2 s = make_double2(0.0, 0.0);
            if (mine) {
                s = A[tid * kWpeMaxTaps + j];
                for (int m = 0; m < j; ++m) {
                    const double2 a = A[tid * kWpeMaxTaps + m], c = A[j * kWpeMaxTaps + m];
                    s.x -= a.x * c.x + a.y * c.y;
                    s.y -= a.y * c.x - a.x * c.y;
                }
                if (tid == j) piv[0] = s.x;
            }
            __syncthreads();
            const double d = piv[0];
            if (!(d > 0.0) || !isfinite(d)) { bad = true; break; }             // uniform
            const double r = sqrt(d);
            if (mine) A[tid * kWpeMaxTaps + j] = tid == j ? make_double2(r, 0.0) : make_double2(s.x / r, s.y / r);
            __syncthreads();
        }
        if (bad) { pass = true; break; }
        // step 6: L z = p, then L^H g = z, in wave 0
        if (wave == 0) {
            double2 acc = lane < K ? pv[lane] : make_double2(0.0, 0.0);
            for (int j = 0; j < K; ++j) {
                const double dj = A[j * kWpeMaxTaps + j].x;
                const double zx = __shfl(acc.x, j) / dj, zy = __shfl(acc.y, j) / dj;
                if (lane == j) {
                    acc = make_double2(zx, zy);
                } else if (lane > j && lane < K) {
                    const double2 l = A[lane * kWpeMaxTaps + j];
                    acc.x -= l.x * zx - l.y * zy;
                    acc.y -= l.x * zy + l.y * zx;
                }
            }
            for (int j = K - 1; j >= 0; --j) {
                const double dj = A[j * kWpeMaxTaps + j].x;
                const double gx = __shfl(acc.x, j) / dj, gy = __shfl(acc.y, j) / dj;
                if (lane == j) {
                    acc = make_double2(gx, gy);
                } else if (lane < j) {
                    const double2 l = A[j * kWpeMaxTaps + lane];                // conj(L[j][lane]) g[j]
                    acc.x -= l.x * gx + l.y * gy;
                    acc.y -= l.x * gy - l.y * gx;
                }
            }
            if (lane < K) gv[lane] = acc;
        }
        __syncthreads();
        have = true;
        ++done;
    }
    __syncthreads();

    // the output, each part rounded to f32 once, and the bin's sums: a thread its own frames in ascending order, then the fixed tree
    float2* __restrict__ out = p.cols_out + (long long)p.c0[b] + (long long)f * Tp;
    double sY = 0.0, sD = 0.0;
    for (int t = tid; t < Tp; t += kWpeThreads) {
        float2 o = make_float2(0.0f, 0.0f);
        if (t < T) {
            const float2 v = y[t];
            o = v;
            if (!pass) {
                const double2 d = wpe_resid(y, gv, t, delay, K, true);
                o = make_float2((float)d.x, (float)d.y);
            }
            sY += (double)v.x * (double)v.x + (double)v.y * (double)v.y;
            sD += (double)o.x * (double)o.x + (double)o.y * (double)o.y;
        }
        out[t] = o;
    }
    sY = block_tree_sum<kWpeThreads>(red, sY);
    sD = block_tree_sum<kWpeThreads>(red, sD);
    if (p.filters && tid < K) {
        double* __restrict__ fo = p.filters + (((long long)b * p.Fp + f) * K + tid) * 2;
        fo[0] = pass ? 0.0 : gv[tid].x;
        fo[1] = pass ? 0.0 : gv[tid].y;
    }
    if (tid == 0) {
        double gmax = 0.0;
        if (!pass)
            for (int k = 0; k < K; ++k) gmax = fmax(gmax, sqrt(gv[k].x * gv[k].x + gv[k].y * gv[k].y));
        double* __restrict__ st = p.stat + ((long long)b * p.F + f) * kWpeStat;
        st[0] = sY; st[1] = sD; st[2] = pass ? 0.0 : 1.0; st[3] = gmax; st[4] = (double)done;
    }
}

// thread t takes the bins t, t + 256, ... in ascending order; the 256 partial sums meet in the fixed tree
__global__ __launch_bounds__(kFigThreads) void wpe_figures_kernel(WpeP p) {
    __shared__ double red[kFigThreads];
    const int b = blockIdx.x, tid = threadIdx.x;
    const double* __restrict__ st = p.stat + (long long)b * p.F * kWpeStat;
    double sY = 0.0, sD = 0.0, nf = 0.0, gm = 0.0, im = 0.0;
    for (int f = tid; f < p.F; f += kFigThreads) {
        sY += st[f * kWpeStat];
        sD += st[f * kWpeStat + 1];
        nf += st[f * kWpeStat + 2];
        gm = fmax(gm, st[f * kWpeStat + 3]);
        im = fmax(im, st[f * kWpeStat + 4]);
    }
    sY = block_tree_sum<kFigThreads>(red, sY);
    sD = block_tree_sum<kFigThreads>(red, sD);
    nf = block_tree_sum<kFigThreads>(red, nf);                                 // counts below 2^53 are exact in the tree
    gm = block_tree_max<kFigThreads>(red, gm);
    im = block_tree_max<kFigThreads>(red, im);
    if (tid != 0) return;
    double* __restrict__ o = p.fig + (long long)b * MT2_WPE_FIELDS;
    o[0] = sY;
    o[1] = sD;
    o[2] = 10.0 * log10(sD / sY);
    o[3] = (double)min(p.T[b], p.T_cap);
    o[4] = nf;
    o[5] = (double)p.F - nf;
    o[6] = gm;
    o[7] = im;
}

namespace {
bool wpe_rows_ok(const WpeP& p) {
    return p.B >= 1 && p.B <= 65535 && p.F >= 1 && p.Fp >= p.F && p.Fp - p.F < 4 && p.lds >= 2 * p.F && p.lds % 4 == 0 && p.T_cap >= 1 &&
           p.T_cap <= MT2_WPE_MAX_FRAMES && p.row0 != nullptr && p.T != nullptr && p.c0 != nullptr;
}
dim3 wpe_tile_grid(const WpeP& p) { return dim3((p.F + kTile - 1) / kTile, (p.T_cap + kTile - 1) / kTile, p.B); }
}  // namespace

hipError_t launch_wpe_to_bins(const WpeP& p, hipStream_t s) {
    if (!wpe_rows_ok(p) || p.spec == nullptr || p.cols == nullptr || ((uintptr_t)p.spec & 15) || ((uintptr_t)p.cols & 15)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wpe_to_bins_kernel, wpe_tile_grid(p), dim3(kTrThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_wpe_from_bins(const WpeP& p, hipStream_t s) {
    if (!wpe_rows_ok(p) || p.spec_out == nullptr || p.cols_out == nullptr || ((uintptr_t)p.spec_out & 15) || ((uintptr_t)p.cols_out & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(wpe_from_bins_kernel, wpe_tile_grid(p), dim3(kTrThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_wpe_bins(const WpeP& p, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};
    if (!wpe_rows_ok(p) || p.cols == nullptr || p.cols_out == nullptr || p.cols == p.cols_out || p.run == nullptr || p.stat == nullptr ||
        ((uintptr_t)p.cols & 15) || ((uintptr_t)p.cols_out & 15) || p.taps < 1 || p.taps > kWpeMaxTaps || p.delay < 1 || p.delay > 8 ||
        p.iters < 1 || p.iters > 8 || p.ctx < 0 || p.ctx > 4)
        return hipErrorInvalidValue;
    const hipError_t e = dyn_lds_once(done, reinterpret_cast<const void*>(wpe_bin_kernel), wpe_lds_bytes(MT2_WPE_MAX_FRAMES));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(wpe_bin_kernel, dim3(p.F, p.B), dim3(kWpeThreads), wpe_lds_bytes(p.T_cap), s, p);
    return hipGetLastError();
}
hipError_t launch_wpe_figures(const WpeP& p, hipStream_t s) {
    if (!wpe_rows_ok(p) || p.stat == nullptr || p.fig == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(wpe_figures_kernel, dim3(p.B), dim3(kFigThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
