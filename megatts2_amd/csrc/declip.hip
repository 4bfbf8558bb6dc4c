// Declipping of prompt audio by sparsity (gfx950): A-SPADE (Kitic, Bertin and Gribonval 2015; the analysis variant of Zaviska, Rajmic,
// Ozerov and Rencker 2021).  No reference counterpart.  Parity with any outside declipper is unpinned, and so is audible quality on real
// speech; the rule is our own, stated in include/megatts2_hip.h and restated in tests/declip_ref.py.  In short, for one frame of N
// samples (hop N / 4, square-root Hann window), everything in double, A the N-point real DFT scaled by 1 / sqrt(N):
//
//   F = y w;  x = F, u = 0, k = s
//   max_iter times:  v = A x + u;  zb = the bins of v whose |v|^2 >= the k-th largest |v|^2 of the half spectrum (ties all kept)
//                    x = proj(A^H (zb - u)): F on reliable samples, max(., F) on samples clipped high, min(., F) on those clipped low
//                    d = A x - zb;  stop if |d| <= eps |F|;  u += d;  every r-th iteration k += s
//
// Four kernels:
//   dc_detect_kernel   grid (B), 1024 threads: max, min, the non-finite flag, then the two counts against the f32 thresholds - f32
//                      comparisons and integer sums only, so the answer is held bit for bit
//   dc_frame_kernel    grid (T_cap, B), 256 threads: ONE workgroup runs the whole iteration of one (utterance, frame) out of LDS - no
//                      launch per iteration and no grid-wide synchronisation.  It windows the frame and builds F and the masks itself.
//                      The transform is an N / 2 point complex radix-2 on the even / odd packing of the frame: forward decimation in
//                      frequency (natural order in, bit-reversed out), inverse decimation in time (bit-reversed in, natural out), so no
//                      pass reorders; the split into / from the half spectrum reads and writes the bit-reversed positions directly.
//                      A x is needed once per iteration: A x = d + zb gives the next v = A x + u without a third transform, so an
//                      iteration costs one inverse and one forward real FFT.
//                      LDS index swizzle: cell p of the work array and of the twiddle table sits at p + p / 16 + p / 256 (complex
//                      cells of 16 bytes, 16 to a row of 64 banks).  Butterflies take consecutive p per lane and are conflict-free
//                      as they stand; the swizzle is for the bit-reversed gathers and scatters (stride M / 64 cells between lanes)
//                      and for the twiddle reads of the late forward / early inverse stages (stride N / 2h), which would otherwise
//                      all land in one bank.
//                      Selection: an exact radix select, most significant byte first, over the 64-bit patterns of |v|^2 (>= +0, so
//                      they order as unsigned integers; a NaN orders above everything and harms nothing): a 256-bin histogram by
//                      integer LDS atomics, a shuffle scan in the first wave - the form of ebu.hip's range_select, from the top.
//                      Norms: thread t adds its bins t, t + 256, ... in ascending order, then block_tree_sum - an order that depends
//                      on the bin index alone.  The stop is workgroup-uniform (every thread reads red[0]).
//   dc_overlap_kernel  a thread per output sample: its four frames in ascending order, the sum of w^2 beside them, one rounding to f32,
//                      then the write rule (reliable: the input's bits; H: max(rounded, y); L: min(rounded, y))
//   dc_figures_kernel  a workgroup per utterance: the eight doubles
// No floating-point atomics; every loop has a trip count fixed by N, len and max_iter, so non-finite values can neither fault nor hang.
// LDS of dc_frame_kernel, bytes: N 256: 15 888;  512: 28 688;  1024: 54 320;  2048: 105 584 (F, x, the work array, u, v, the twiddles,
// the masks, 256 doubles and 258 words for the reductions) - three workgroups a CU at the default N = 1024, one at 2048.
// Registers, from the ISA (-save-temps): dc_frame_kernel 60 VGPRs, 90 SGPRs, no scratch and no spills - one kernel serves every N;
// dc_detect_kernel 44 VGPRs, dc_overlap_kernel 22, dc_figures_kernel 22, none with scratch.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <float.h>
#include <math.h>

namespace mt2 {

namespace {
constexpr int kFigThreads = 256;

__host__ __device__ __forceinline__ int dc_pad(int p) { return p + (p >> 4) + (p >> 8); }

// the f32 thresholds of the rule: two roundings each, never a fused multiply-add
__device__ __forceinline__ float dc_thr_hi(float hi, float tol) { return __fsub_rn(hi, __fmul_rn(tol, fabsf(hi))); }
__device__ __forceinline__ float dc_thr_lo(float lo, float tol) { return __fadd_rn(lo, __fmul_rn(tol, fabsf(lo))); }

__device__ __forceinline__ unsigned long long dc_key(const double2 v) {
    return (unsigned long long)__double_as_longlong(fma(v.x, v.x, v.y * v.y));
}
__device__ __forceinline__ double2 cadd(double2 a, double2 b) { return make_double2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ double2 csub(double2 a, double2 b) { return make_double2(a.x - b.x, a.y - b.y); }
__device__ __forceinline__ double2 cmul(double2 a, double2 w) { return make_double2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x); }
__device__ __forceinline__ double2 cmulc(double2 a, double2 w) { return make_double2(a.x * w.x + a.y * w.y, a.y * w.x - a.x * w.y); }

struct DcLds {
    double* F; double* X; double2* W; double2* U; double2* V; double2* tw; double* red; unsigned* hist; unsigned* pick; unsigned char* mask;
};
__host__ __device__ inline size_t dc_carve(int N, char* base, DcLds* l) {
    const size_t M = N / 2, K = M + 1, cells = (size_t)dc_pad((int)M - 1) + 1;
    size_t at = 0;
    auto take = [&](size_t bytes) { char* q = base + at; at += (bytes + 15) & ~size_t(15); return q; };
    char* F = take(sizeof(double) * N); char* X = take(sizeof(double) * N); char* W = take(sizeof(double2) * cells);
    char* U = take(sizeof(double2) * K); char* V = take(sizeof(double2) * K); char* tw = take(sizeof(double2) * cells);
    char* red = take(sizeof(double) * kDcThreads); char* hist = take(sizeof(unsigned) * 256); char* pick = take(sizeof(unsigned) * 2);
    char* mask = take((size_t)N);
    if (l) {
        l->F = reinterpret_cast<double*>(F); l->X = reinterpret_cast<double*>(X); l->W = reinterpret_cast<double2*>(W);
        l->U = reinterpret_cast<double2*>(U); l->V = reinterpret_cast<double2*>(V); l->tw = reinterpret_cast<double2*>(tw);
        l->red = reinterpret_cast<double*>(red); l->hist = reinterpret_cast<unsigned*>(hist); l->pick = reinterpret_cast<unsigned*>(pick);
        l->mask = reinterpret_cast<unsigned char*>(mask);
    }
    return at;
}

// forward: X (N / 2 complex cells, natural order, not swizzled) -> W (swizzled; Z[k] at position bitrev(k)).  Ends behind a barrier.
__device__ __forceinline__ void dc_fft_forward(const double2* X, double2* W, const double2* tw, int M, int logM) {
    const int tid = threadIdx.x;
    for (int lh = logM - 1; lh >= 0; --lh) {
        const int h = 1 << lh;
        const bool first = lh == logM - 1;
        for (int j = tid; j < M / 2; j += kDcThreads) {
            const int idx = j & (h - 1), pp = ((j >> lh) << (lh + 1)) + idx;
            const double2 a = first ? X[pp] : W[dc_pad(pp)], b = first ? X[pp + h] : W[dc_pad(pp + h)];
            const double2 w = tw[dc_pad(idx << (logM - lh))];              // e^(-2 pi i idx / 2h) = table[idx N / 2h]
            W[dc_pad(pp)] = cadd(a, b);
            W[dc_pad(pp + h)] = cmul(csub(a, b), w);
        }
        __syncthreads();
    }
}
// inverse, unnormalised, in place on W: bit-reversed in, natural out.  Ends behind a barrier.
__device__ __forceinline__ void dc_fft_inverse(double2* W, const double2* tw, int M, int logM) {
    const int tid = threadIdx.x;
    for (int lh = 0; lh < logM; ++lh) {
        const int h = 1 << lh;
        for (int j = tid; j < M / 2; j += kDcThreads) {
            const int idx = j & (h - 1), pp = ((j >> lh) << (lh + 1)) + idx;
            const double2 a = W[dc_pad(pp)], b = cmulc(W[dc_pad(pp + h)], tw[dc_pad(idx << (logM - lh))]);
            W[dc_pad(pp)] = cadd(a, b);
            W[dc_pad(pp + h)] = csub(a, b);
        }
        __syncthreads();
    }
}

// the k-th largest (k in [1, K]) of the K keys of V, exactly; the result is in every thread
__device__ unsigned long long dc_select(const double2* V, int K, unsigned k, unsigned* hist, unsigned* pick) {
    const int t = threadIdx.x;
    unsigned long long prefix = 0;
    unsigned rank = k - 1;                                                     // 0-based, from the top
    for (int shift = 56; shift >= 0; shift -= 8) {
        const unsigned long long mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        __syncthreads();
        hist[t] = 0u;
        __syncthreads();
        for (int i = t; i < K; i += kDcThreads) {
            const unsigned long long key = dc_key(V[i]);
            if ((key & mask) == prefix) atomicAdd(&hist[255u - ((unsigned)(key >> shift) & 255u)], 1u);
        }
        __syncthreads();
        if (t < 64) {                                                          // four bins a lane, a prefix sum by shuffles
            const unsigned h0 = hist[4 * t], h1 = hist[4 * t + 1], h2 = hist[4 * t + 2], h3 = hist[4 * t + 3], own = (h0 + h1) + (h2 + h3);
            unsigned inc = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = __shfl_up(inc, d);
                if (t >= d) inc += v;
            }
            const unsigned exc = inc - own;
            if (rank >= exc && rank < inc) {                                   // one lane: rank is under the number of keys counted
                unsigned r = rank - exc, d = 4u * t;
                if (r >= h0) { r -= h0; ++d; if (r >= h1) { r -= h1; ++d; if (r >= h2) { r -= h2; ++d; } } }
                pick[0] = d; pick[1] = r;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)(255u - pick[0]) << shift;
        rank = pick[1];
    }
    return prefix;
}
}  // namespace

size_t dc_lds_bytes(int N) { return dc_carve(N, nullptr, nullptr); }
size_t dc_table_doubles(int N) { return 2 * ((size_t)dc_pad(N / 2 - 1) + 1) + (size_t)N; }
// host only: the twiddles e^(-2 pi i k / N), k < N / 2, at their swizzled cells, then the window
void dc_table(int N, double* t) {
    const size_t cells = (size_t)dc_pad(N / 2 - 1) + 1;
    for (size_t i = 0; i < 2 * cells; ++i) t[i] = 0.0;
    const double two_pi = 6.283185307179586476925286766559;
    for (int k = 0; k < N / 2; ++k) {
        t[2 * dc_pad(k)] = cos(two_pi * k / N);
        t[2 * dc_pad(k) + 1] = -sin(two_pi * k / N);
    }
    for (int n = 0; n < N; ++n) t[2 * cells + n] = sqrt(0.5 - 0.5 * cos(two_pi * n / N));
}

__global__ __launch_bounds__(kDcDetThreads) void dc_detect_kernel(DeclipP p) {
    __shared__ float smx[kDcDetThreads / 64], smn[kDcDetThreads / 64];
    __shared__ int sbad[kDcDetThreads / 64], snh[kDcDetThreads / 64], snl[kDcDetThreads / 64];
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, len = min(p.len[b], p.L_max);
    const float* __restrict__ y = p.wav + (long long)b * p.L_max;
    float mx = -INFINITY, mn = INFINITY;
    int bad = 0;
    for (int j = tid; j < len; j += kDcDetThreads) {
        const float v = y[j];
        mx = fmaxf(mx, v); mn = fminf(mn, v);
        bad |= !isfinite(v);
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) {
        mx = fmaxf(mx, __shfl_xor(mx, d)); mn = fminf(mn, __shfl_xor(mn, d)); bad |= __shfl_xor(bad, d);
    }
    if (lane == 0) { smx[wave] = mx; smn[wave] = mn; sbad[wave] = bad; }
    __syncthreads();
    mx = smx[0]; mn = smn[0]; bad = sbad[0];
    for (int i = 1; i < kDcDetThreads / 64; ++i) { mx = fmaxf(mx, smx[i]); mn = fminf(mn, smn[i]); bad |= sbad[i]; }
    const float hi = p.level == p.level ? p.level : mx, lo = p.level == p.level ? -p.level : mn;
    const float th = dc_thr_hi(hi, p.tol), tl = dc_thr_lo(lo, p.tol);
    int nh = 0, nl = 0;
    for (int j = tid; j < len; j += kDcDetThreads) {
        const float v = y[j];
        nh += (hi > 0.0f && v >= th) ? 1 : 0;
        nl += (lo < 0.0f && v <= tl) ? 1 : 0;
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) { nh += __shfl_xor(nh, d); nl += __shfl_xor(nl, d); }
    if (lane == 0) { snh[wave] = nh; snl[wave] = nl; }
    __syncthreads();
    if (tid != 0) return;
    nh = 0; nl = 0;
    for (int i = 0; i < kDcDetThreads / 64; ++i) { nh += snh[i]; nl += snl[i]; }
    int* __restrict__ o = p.det + (long long)b * kDcDet;
    const int need = p.need[b];
    o[0] = __float_as_int(hi); o[1] = __float_as_int(lo); o[2] = nh; o[3] = nl;
    o[4] = (!bad && nh >= need) ? 1 : 0; o[5] = (!bad && nl >= need) ? 1 : 0; o[6] = bad ? 1 : 0; o[7] = 0;
}

__global__ __launch_bounds__(kDcThreads) void dc_frame_kernel(DeclipP p) {
    extern __shared__ __attribute__((aligned(16))) char dc_lds[];
    DcLds l;
    dc_carve(p.N, dc_lds, &l);
    const int b = blockIdx.y, t = blockIdx.x, tid = threadIdx.x;
    const int N = p.N, hop = N >> 2, M = N >> 1, K = M + 1, logM = 31 - __clz(M);
    const int len = min(p.len[b], p.L_max), T = (len + hop - 1) / hop + 3;
    if (t >= T) return;                                                        // uniform over the workgroup
    const int* __restrict__ det = p.det + (long long)b * kDcDet;
    const bool clipH = det[4] != 0, clipL = det[5] != 0;
    if (!clipH && !clipL) return;                                              // the utterance passes through: the overlap kernel copies it
    const long long row = (long long)p.row0[b] + t;
    const float th = dc_thr_hi(__int_as_float(det[0]), p.tol), tl = dc_thr_lo(__int_as_float(det[1]), p.tol);
    const double* __restrict__ win = p.table + 2 * ((size_t)dc_pad(M - 1) + 1);
    const float* __restrict__ y = p.wav + (long long)b * p.L_max;
    double* __restrict__ frame = p.frames + row * N;

    // the frame, its masks and its norm
    double sF = 0.0, nc = 0.0, nr = 0.0;
    for (int n = tid; n < N; n += kDcThreads) {
        const long long j = (long long)t * hop - 3 * hop + n;
        double f = 0.0;
        unsigned char m = 0;
        if (j >= 0 && j < len) {
            const float v = y[j];
            m = (clipH && v >= th) ? 1 : ((clipL && v <= tl) ? 2 : 0);
            f = (double)v * win[n];
            nr += m ? 0.0 : 1.0;                                               // a reliable sample of the utterance's own: pads anchor nothing
        }
        l.F[n] = f; l.X[n] = f; l.mask[n] = m;
        sF += f * f;
        nc += m ? 1.0 : 0.0;
    }
    sF = block_tree_sum<kDcThreads>(l.red, sF);
    nc = block_tree_sum<kDcThreads>(l.red, nc);
    nr = block_tree_sum<kDcThreads>(l.red, nr);
    int done = 0;
    if (sF > 0.0 && nc > 0.0 && nr > 0.0) {                                                // uniform: red[0]
        const double bar = p.eps * sqrt(sF), scale_f = 1.0 / sqrt((double)N), scale_i = 2.0 / sqrt((double)N);
        const int cells = dc_pad(M - 1) + 1;
        for (int i = tid; i < cells; i += kDcThreads) l.tw[i] = reinterpret_cast<const double2*>(p.table)[i];
        for (int i = tid; i < K; i += kDcThreads) l.U[i] = make_double2(0.0, 0.0);
        __syncthreads();
        const double2* Xc = reinterpret_cast<const double2*>(l.X);
        // v = A x (u = 0)
        dc_fft_forward(Xc, l.W, l.tw, M, logM);
        for (int k = tid; k < M; k += kDcThreads) {
            if (k == 0) {
                const double2 z = l.W[0];
                l.V[0] = make_double2((z.x + z.y) * scale_f, 0.0);
                l.V[M] = make_double2((z.x - z.y) * scale_f, 0.0);
            } else {
                const double2 zk = l.W[dc_pad((int)(__brev((unsigned)k) >> (32 - logM)))];
                double2 zc = l.W[dc_pad((int)(__brev((unsigned)(M - k)) >> (32 - logM)))];
                zc.y = -zc.y;
                const double2 e = make_double2(0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y));
                const double2 o = make_double2(0.5 * (zk.y - zc.y), -0.5 * (zk.x - zc.x));      // -i / 2 (zk - zc)
                const double2 a = cadd(e, cmul(o, l.tw[dc_pad(k)]));
                l.V[k] = make_double2(a.x * scale_f, a.y * scale_f);
            }
        }
        int kk = p.step;
        for (int it = 1; it <= p.max_iter; ++it) {
            const unsigned long long thr = dc_select(l.V, K, (unsigned)min(kk, K), l.hist, l.pick);      // barriers inside: V is whole
            // A^H (zb - u): the half spectrum into the N / 2 point one, at its bit-reversed cells
            for (int k = tid; k < M; k += kDcThreads) {
                const double2 vk = l.V[k], vm = l.V[M - k];
                double2 yk = dc_key(vk) >= thr ? vk : make_double2(0.0, 0.0), ym = dc_key(vm) >= thr ? vm : make_double2(0.0, 0.0);
                yk = csub(yk, l.U[k]); ym = csub(ym, l.U[M - k]);
                ym.y = -ym.y;
                const double2 e = make_double2(0.5 * (yk.x + ym.x), 0.5 * (yk.y + ym.y));
                const double2 o = cmulc(make_double2(0.5 * (yk.x - ym.x), 0.5 * (yk.y - ym.y)), l.tw[dc_pad(k)]);
                l.W[dc_pad((int)(__brev((unsigned)k) >> (32 - logM)))] = make_double2(e.x - o.y, e.y + o.x);      // e + i o
            }
            __syncthreads();
            dc_fft_inverse(l.W, l.tw, M, logM);
            for (int m = tid; m < M; m += kDcThreads) {
                const double2 z = l.W[dc_pad(m)];
                const double c[2] = {z.x * scale_i, z.y * scale_i};
#pragma unroll
                for (int q = 0; q < 2; ++q) {
                    const int n = 2 * m + q;
                    const double f = l.F[n];
                    const unsigned char mk = l.mask[n];
                    l.X[n] = mk == 1 ? fmax(c[q], f) : (mk == 2 ? fmin(c[q], f) : f);
                }
            }
            __syncthreads();
            dc_fft_forward(Xc, l.W, l.tw, M, logM);
            // d = A x - zb;  u += d;  v = A x + u;  |d|^2 over the full spectrum: the inner bins twice
            double sd = 0.0;
            for (int k = tid; k < M; k += kDcThreads) {
                if (k == 0) {
                    const double2 z = l.W[0];
                    const double a0 = (z.x + z.y) * scale_f, aM = (z.x - z.y) * scale_f;
                    const double2 v0 = l.V[0], vM = l.V[M];
                    const double2 d0 = make_double2(a0 - (dc_key(v0) >= thr ? v0.x : 0.0), 0.0 - (dc_key(v0) >= thr ? v0.y : 0.0));
                    const double2 dM = make_double2(aM - (dc_key(vM) >= thr ? vM.x : 0.0), 0.0 - (dc_key(vM) >= thr ? vM.y : 0.0));
                    const double2 u0 = cadd(l.U[0], d0), uM = cadd(l.U[M], dM);
                    l.U[0] = u0; l.U[M] = uM;
                    l.V[0] = make_double2(a0 + u0.x, u0.y);
                    l.V[M] = make_double2(aM + uM.x, uM.y);
                    sd += (d0.x * d0.x + d0.y * d0.y) + (dM.x * dM.x + dM.y * dM.y);
                } else {
                    const double2 zk = l.W[dc_pad((int)(__brev((unsigned)k) >> (32 - logM)))];
                    double2 zc = l.W[dc_pad((int)(__brev((unsigned)(M - k)) >> (32 - logM)))];
                    zc.y = -zc.y;
                    const double2 e = make_double2(0.5 * (zk.x + zc.x), 0.5 * (zk.y + zc.y));
                    const double2 o = make_double2(0.5 * (zk.y - zc.y), -0.5 * (zk.x - zc.x));
                    double2 a = cadd(e, cmul(o, l.tw[dc_pad(k)]));
                    a.x *= scale_f; a.y *= scale_f;
                    const double2 v = l.V[k];
                    const double2 d = dc_key(v) >= thr ? csub(a, v) : a;
                    const double2 u = cadd(l.U[k], d);
                    l.U[k] = u;
                    l.V[k] = cadd(a, u);
                    sd += 2.0 * (d.x * d.x + d.y * d.y);
                }
            }
            sd = block_tree_sum<kDcThreads>(l.red, sd);                        // its barriers also close the writes of U and V
            done = it;
            if (sqrt(sd) <= bar) break;                                        // uniform: red[0]
            if (it % p.every == 0) kk += p.step;
        }
    }
    __syncthreads();
    for (int n = tid; n < N; n += kDcThreads) frame[n] = l.X[n];
    if (tid == 0) {
        p.it[row] = done;
        if (p.iters_out) p.iters_out[(long long)b * p.T_max + t] = done;
    }
}

__global__ __launch_bounds__(256) void dc_overlap_kernel(DeclipP p) {
    const int b = blockIdx.y, len = min(p.len[b], p.L_max);
    const long long j = (long long)blockIdx.x * 256 + threadIdx.x;
    if (j >= len) return;
    const int* __restrict__ det = p.det + (long long)b * kDcDet;
    const bool clipH = det[4] != 0, clipL = det[5] != 0;
    const float v = p.wav[(long long)b * p.L_max + j];
    float o = v;
    if (clipH || clipL) {
        const float th = dc_thr_hi(__int_as_float(det[0]), p.tol), tl = dc_thr_lo(__int_as_float(det[1]), p.tol);
        const int m = (clipH && v >= th) ? 1 : ((clipL && v <= tl) ? 2 : 0);
        if (m) {
            const int N = p.N, hop = N >> 2, t0 = (int)(j / hop), r = (int)(j - (long long)t0 * hop);
            const double* __restrict__ win = p.table + 2 * ((size_t)dc_pad(N / 2 - 1) + 1);
            const double* __restrict__ fr = p.frames + ((long long)p.row0[b] + t0) * N;
            double num = 0.0, den = 0.0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {                                      // the frames t0 .. t0 + 3 < T
                const int n = r + (3 - q) * hop;
                const double w = win[n];
                num += fr[(long long)q * N + n] * w;
                den += w * w;
            }
            const float s = (float)(num / den);
            o = m == 1 ? fmaxf(s, v) : fminf(s, v);
        }
    }
    p.out[(long long)b * p.Lout_max + j] = o;
}

// thread t takes the samples (and the frames) t, t + 256, ... in ascending order; the partial sums meet in the fixed tree
__global__ __launch_bounds__(kFigThreads) void dc_figures_kernel(DeclipP p) {
    __shared__ double red[kFigThreads];
    const int b = blockIdx.x, tid = threadIdx.x, len = min(p.len[b], p.L_max);
    const int* __restrict__ det = p.det + (long long)b * kDcDet;
    const bool clipH = det[4] != 0, clipL = det[5] != 0, restored = p.out != nullptr && (clipH || clipL);
    double sy = 0.0, so = 0.0, ni = 0.0, si = 0.0, mi = 0.0;
    if (restored) {                                                            // uniform
        const float* __restrict__ y = p.wav + (long long)b * p.L_max;
        const float* __restrict__ o = p.out + (long long)b * p.Lout_max;
        for (int j = tid; j < len; j += kFigThreads) {
            sy += (double)y[j] * (double)y[j];
            so += (double)o[j] * (double)o[j];
        }
        const int hop = p.N >> 2, T = (len + hop - 1) / hop + 3;
        const int* __restrict__ it = p.it + p.row0[b];
        for (int t = tid; t < T; t += kFigThreads) {
            const double v = (double)it[t];
            ni += v > 0.0 ? 1.0 : 0.0; si += v; mi = fmax(mi, v);
        }
        sy = block_tree_sum<kFigThreads>(red, sy);
        so = block_tree_sum<kFigThreads>(red, so);
        ni = block_tree_sum<kFigThreads>(red, ni);                             // counts below 2^53 are exact in the tree
        si = block_tree_sum<kFigThreads>(red, si);
        mi = block_tree_max<kFigThreads>(red, mi);
    }
    if (tid != 0) return;
    double* __restrict__ f = p.fig + (long long)b * MT2_DECLIP_FIELDS;
    for (int i = 0; i < MT2_DECLIP_FIELDS; ++i) f[i] = 0.0;
    if (det[6]) { f[1] = f[2] = __longlong_as_double(0x7ff8000000000000ll); return; }
    f[0] = (clipH || clipL) ? 1.0 : 0.0;
    f[1] = (double)__int_as_float(det[0]);
    f[2] = (double)__int_as_float(det[1]);
    f[3] = (double)((clipH ? det[2] : 0) + (clipL ? det[3] : 0)) / (double)len;
    if (restored) {
        f[4] = ni;
        f[5] = ni > 0.0 ? si / ni : 0.0;
        f[6] = mi;
        f[7] = 10.0 * log10(so / sy);
    }
}

namespace {
bool dc_ok(const DeclipP& p) {
    return p.B >= 1 && p.B <= 65535 && p.wav != nullptr && p.len != nullptr && p.det != nullptr && p.L_max >= 1 &&
           (p.N == 256 || p.N == 512 || p.N == 1024 || p.N == 2048) && p.tol >= 0.0f && p.tol <= 0.1f;
}
bool dc_frames_ok(const DeclipP& p) {
    return dc_ok(p) && p.row0 != nullptr && p.table != nullptr && p.frames != nullptr && p.it != nullptr && p.T_cap >= 1 &&
           p.T_cap <= MT2_DECLIP_MAX_FRAMES && (long long)(p.T_cap - 3) * (p.N / 4) >= 1;
}
}  // namespace

hipError_t launch_dc_detect(const DeclipP& p, hipStream_t s) {
    if (!dc_ok(p) || p.need == nullptr) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dc_detect_kernel, dim3(p.B), dim3(kDcDetThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_dc_frames(const DeclipP& p, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};
    if (!dc_frames_ok(p) || p.step < 1 || p.every < 1 || p.max_iter < 1 || (p.iters_out != nullptr && p.T_max < p.T_cap)) return hipErrorInvalidValue;
    const hipError_t e = dyn_lds_once(done, reinterpret_cast<const void*>(dc_frame_kernel), dc_lds_bytes(2048));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(dc_frame_kernel, dim3(p.T_cap, p.B), dim3(kDcThreads), dc_lds_bytes(p.N), s, p);
    return hipGetLastError();
}
hipError_t launch_dc_overlap(const DeclipP& p, int max_len, hipStream_t s) {
    if (!dc_frames_ok(p) || p.out == nullptr || max_len < 1 || max_len > p.L_max || max_len > p.Lout_max) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dc_overlap_kernel, dim3((max_len + 255) / 256, p.B), dim3(256), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_dc_figures(const DeclipP& p, hipStream_t s) {
    if (!dc_ok(p) || p.fig == nullptr || (p.out != nullptr && (p.it == nullptr || p.row0 == nullptr))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dc_figures_kernel, dim3(p.B), dim3(kFigThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
