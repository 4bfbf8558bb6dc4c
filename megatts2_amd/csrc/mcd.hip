// Mel-cepstral distortion along a DTW path (gfx950): how far one log-mel is from another of the same sentence, in dB, with the F0
// error and the voicing error along the SAME path.  The rule is our own, stated in include/megatts2_hip.h and restated in float64 in
// tests/mcd_ref.py; parity with any outside tool (SPTK / WORLD mel-generalised cepstra, the ESPnet or Coqui MCD scripts) is unpinned:
// this cepstrum is a DCT of an N-bin log-mel, not a mel-generalised cepstrum of a spectral envelope.  Per pair of utterances, A f32
// [Ta, N] and B f32 [Tb, N] (natural-log mels), N in [2, 128], order K in [1, min(N - 1, 32)]:
//
//   table     tab[k-1][m] = cos(pi (m + 1/2) k / N) / N in double, rounded once to f32 (k = 1 .. K; c0, the level, is left out)
//   cepstrum  c[t][k-1] = sum_m M[t][m] tab[k-1][m] in f32 as ONE fma chain over m ascending from 0: acc = 0; acc = fmaf(M, tab, acc)
//   warp      the DTW rule of dtw.hip, unchanged, on the cepstra (D = K): lo[j] <= i <= hi[j] are the path's cells in column j
//   cell      q = sum_k (ca[i][k] - cb[j][k])^2, the DTW's own cost chain;  dB(i, j) = (10 / ln 10) sqrt(2 (double) q), in double:
//             one exact doubling, one square root, one product
//   F0        a frame is voiced iff f0 > 0 (a NaN is not);  on a cell voiced on both sides D = 1200 log2((double) f0_a / (double)
//             f0_b) cents: one division, one log2, one product;  a cell voiced on exactly one side is a voicing error
//   sums      in double, one workgroup of 256 threads per utterance: thread t takes the columns j = t, t + 256, ... ascending and in
//             a column i ascending, every term ONE add (no contraction with the product in front of it);  the 256 partial sums meet
//             in block_tree_sum<256>, the maximum in block_tree_max<256>.  The order depends on the frame index alone: a ragged batch
//             is bit-identical to its utterances alone.
//   row       8 doubles: cells | mean dB | largest dB | cells voiced on both sides | sqrt(mean D^2) | mean D | cells voiced on one side
//             | that over the cells.  Fields 3-7 are 0 without F0 tracks, 4 and 5 are 0 without a cell voiced on both sides.
//
// Two kernels.  cepstrum: one launch over (tiles of 32 frames, b); the table sits in LDS (at most 32 x 128 floats) beside the tile's
// mel rows, each staged once with coalesced loads and serving its K chains;  thread e of the tile owns the outputs e, e + 256, ... of
// the tile's 32 K consecutive floats, so a wave's stores are one run.  Rows at or beyond an utterance's length are never read and
// their cepstra are written 0.  path: the reduction above;  a thread holds the cb row of its column in registers across the column's
// vertical run and reads the ca rows of the run from global memory.  lo / hi are read as mt2_dtw_align left them;  whatever they hold,
// a run is cut to the rows [0, Ta) and to the columns [0, Tb), so nothing outside the two cepstra is read.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <cmath>

namespace mt2 {

namespace {
constexpr int kCepRows = 32;                   // cepstrum: frames per workgroup
constexpr int kThreads = 256;
constexpr int kMaxN = 128;                     // the widest mel
constexpr int kMaxK = MT2_MCD_MAX_ORDER;
constexpr double kDbScale = 4.342944819032518; // the double nearest 10 / ln 10
static_assert(kMaxK * (kMaxN + 1) * 4 + kCepRows * (kMaxN + 1) * 4 <= 64 * 1024, "table and tile share the LDS");
}  // namespace

bool mcd_geometry_ok(int n_mels, int order) {
    return n_mels >= 2 && n_mels <= kMaxN && order >= 1 && order <= std::min(n_mels - 1, kMaxK);
}

void mcd_table(int n_mels, int order, float* table) {
    for (int k = 1; k <= order; ++k)
        for (int m = 0; m < n_mels; ++m) table[(size_t)(k - 1) * n_mels + m] = (float)(std::cos(M_PI * (m + 0.5) * k / n_mels) / n_mels);
}

// rows t0 .. t0 + 31 of utterance b.  LDS rows are N + 1 floats apart: lanes that differ in k read different banks of the table, lanes
// that share a row read one word of the tile.
__global__ __launch_bounds__(kThreads) void mcd_cepstrum_kernel(McdCepP p) {
    __shared__ float tab[kMaxK * (kMaxN + 1)], tile[kCepRows * (kMaxN + 1)];
    const int b = blockIdx.y, t0 = blockIdx.x * kCepRows, T = p.len[b], N = p.N, K = p.K, ld = N + 1;
    const int rows = min(kCepRows, p.T_max - t0);                           // of the caller's buffer; t0 < T_max by the grid
    float* __restrict__ out = p.cep + ((long long)b * p.T_max + t0) * K;
    if (t0 >= T) {                                                          // workgroup-uniform, before any barrier: nothing is read
        for (int e = threadIdx.x; e < rows * K; e += kThreads) out[e] = 0.0f;
        return;
    }
    for (int e = threadIdx.x; e < K * N; e += kThreads) tab[(e / N) * ld + e % N] = p.table[e];
    const float* __restrict__ M = p.mel + ((long long)b * p.T_max + t0) * N;
    const int live = min(rows, T - t0);
    for (int e = threadIdx.x; e < live * N; e += kThreads) tile[(e / N) * ld + e % N] = M[e];
    __syncthreads();
    for (int e = threadIdx.x; e < rows * K; e += kThreads) {
        const int r = e / K, k = e - r * K;
        float acc = 0.0f;
        if (r < live) {
            const float* __restrict__ x = tile + r * ld;
            const float* __restrict__ w = tab + k * ld;
            for (int m = 0; m < N; ++m) acc = fmaf(x[m], w[m], acc);
        }
        out[e] = acc;
    }
}

// one workgroup per utterance;  the seven sums and the maximum of the header
__global__ __launch_bounds__(kThreads) void mcd_path_kernel(McdPathP p) {
    __shared__ double red[kThreads];
    const int b = blockIdx.x, Ta = p.a_len[b], Tb = p.b_len[b], K = p.K;
    const float* __restrict__ ca = p.ca + (long long)b * p.Ta_max * K;
    const float* __restrict__ cb = p.cb + (long long)b * p.Tb_max * K;
    const int* __restrict__ lo = p.lo + (long long)b * p.Tb_max;
    const int* __restrict__ hi = p.hi + (long long)b * p.Tb_max;
    const bool pitch = p.f0_a != nullptr && p.f0_b != nullptr;
    const float* __restrict__ fa = pitch ? p.f0_a + (long long)b * p.Ta_max : nullptr;
    const float* __restrict__ fb = pitch ? p.f0_b + (long long)b * p.Tb_max : nullptr;
    double s_db = 0.0, m_db = 0.0, s_d2 = 0.0, s_d = 0.0;
    int cells = 0, both = 0, one = 0;
    for (int j = threadIdx.x; j < Tb; j += kThreads) {
        // every load of a row is issued whatever K is - entries at or beyond K read the row's last word again and are not used - so
        // that a row costs one trip to memory, not one per coefficient behind a branch on k < K
        float y[kMaxK];
#pragma unroll
        for (int k = 0; k < kMaxK; ++k) y[k] = cb[(long long)j * K + min(k, K - 1)];
        const float gb = pitch ? fb[j] : 0.0f;
        const bool vb = gb > 0.0f;
        const int i0 = max(lo[j], 0), i1 = min(hi[j], Ta - 1);
        for (int i = i0; i <= i1; ++i) {
            const float* __restrict__ x = ca + (long long)i * K;
            float xv[kMaxK];
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) xv[k] = x[min(k, K - 1)];
            float q = 0.0f;
#pragma unroll
            for (int k = 0; k < kMaxK; ++k) {
                const float d = __fsub_rn(xv[k], y[k]);
                q = k < K ? fmaf(d, d, q) : q;
            }
            const double db = __dmul_rn(kDbScale, sqrt(2.0 * (double)q));
            s_db = __dadd_rn(s_db, db);
            m_db = fmax(m_db, db);
            ++cells;
            if (pitch) {
                const float ga = fa[i];
                const bool va = ga > 0.0f;
                if (va && vb) {
                    const double d = __dmul_rn(1200.0, log2((double)ga / (double)gb));
                    s_d2 = __dadd_rn(s_d2, __dmul_rn(d, d));
                    s_d = __dadd_rn(s_d, d);
                    ++both;
                } else if (va != vb) {
                    ++one;
                }
            }
        }
    }
    const double n = block_tree_sum<kThreads>(red, (double)cells);         // counts below 2^53 are exact in the tree
    const double sum_db = block_tree_sum<kThreads>(red, s_db);
    const double max_db = block_tree_max<kThreads>(red, m_db);
    const double n2 = block_tree_sum<kThreads>(red, (double)both);
    const double sum_d2 = block_tree_sum<kThreads>(red, s_d2);
    const double sum_d = block_tree_sum<kThreads>(red, s_d);
    const double n1 = block_tree_sum<kThreads>(red, (double)one);
    if (threadIdx.x == 0) {
        double* __restrict__ o = p.out + (long long)b * MT2_MCD_FIELDS;
        o[0] = n;
        o[1] = n > 0.0 ? sum_db / n : 0.0;
        o[2] = max_db;
        o[3] = n2;
        o[4] = n2 > 0.0 ? sqrt(sum_d2 / n2) : 0.0;
        o[5] = n2 > 0.0 ? sum_d / n2 : 0.0;
        o[6] = n1;
        o[7] = n > 0.0 ? n1 / n : 0.0;
    }
}

hipError_t launch_mcd_cepstrum(const McdCepP& p, hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.T_max < 1 || !mcd_geometry_ok(p.N, p.K) || !p.mel || !p.len || !p.table || !p.cep) return hipErrorInvalidValue;
    hipLaunchKernelGGL(mcd_cepstrum_kernel, dim3((p.T_max + kCepRows - 1) / kCepRows, p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_mcd_path(const McdPathP& p, hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.Ta_max < 1 || p.Tb_max < 1 || p.K < 1 || p.K > kMaxK || !p.ca || !p.cb || !p.a_len || !p.b_len || !p.lo ||
        !p.hi || !p.out || (p.f0_a == nullptr) != (p.f0_b == nullptr))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(mcd_path_kernel, dim3(p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
