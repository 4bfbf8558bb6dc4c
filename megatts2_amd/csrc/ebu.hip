// The rest of an "EBU mode" meter (EBU R 128 / Tech 3341) beside the integrated loudness of loudness.hip: true peak (ITU-R BS.1770-4
// Annex 2, with a filter of this library's own), short-term loudness (3 s blocks every 100 ms) and loudness range (EBU Tech 3342),
// for a ragged batch of mono utterances (gfx950).  No reference counterpart.  Parity with libebur128 / pyloudnorm is unpinned; the
// kernels are held to analytic truths (the true peak of a band-limited tone is its amplitude; the range of a two-level tone is the
// difference of the levels) and to tests/ebu_ref.py.  The rule is stated in include/megatts2_hip.h; in short, with h, ns and S[j] of
// the loudness rule:
//
//   o = ceil(192000 / sr) phases;  phase 0 is the sample;  phase p: y[i o + p] = sum_k h[p][k] x[i - Z + 1 + k], k = 0 .. 2 Z - 1
//   ascending in one f32 fma chain, h a Kaiser-windowed sinc (Z = 12, beta = 8), x = 0 outside [0, L), i in [-Z, L);  TP = max |y|
//   nst = max(0, ns - 29);  z3[k] = (S[k] + ... + S[k + 29]) / (30 h) ascending;  s[k] = -0.691 + 10 log10 z3[k]
//   Gamma_r = -0.691 + 10 log10(mean of z3 over s > -70) - 20;  g[0 .. n) = the s over both gates, ascending
//   LRA = g[((n - 1) 95 + 50) / 100] - g[((n - 1) 10 + 50) / 100]
//
// Two kernels behind the four of the loudness call, which run unchanged and leave S[j] and their eight doubles in the arena:
//   true_peak_kernel        grid (tiles, B): the interpolator's tile of true_peak_tile.h, four positions a thread; wave max by
//                           shuffles, one atomicMax per wave, skipped where it cannot raise the word
//   loudness_range_kernel   a workgroup per utterance: z3 (kept in the arena), the counts, Gamma_r and max s in the fixed order of the
//                           gate kernel; the s over both gates as order-preserving 64-bit keys in the arena and the two order
//                           statistics by an exact radix select (8 bits a pass); then the 18 doubles and, for the normalising call,
//                           the gain word that loudness_scale_kernel reads
// The max and the select are order-free and every sum's order depends on the block's index in its utterance alone, so a ragged batch
// is bit-identical to its utterances alone.  A sample at or beyond L is never read.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"
#include "true_peak_tile.h"

#include <limits.h>
#include <math.h>

#include <algorithm>

namespace mt2 {

namespace {
constexpr int kTile = MT2_TP_TILE, kRangeThreads = 256;
constexpr double kBeta = 8.0, kPi = 3.14159265358979323846;
static_assert(kTile == kTpTile, "the true-peak kernel's tile is the shared one");

// I0 by its power series: the terms fall below 2^-53 of the sum within 40 steps for x <= 8
double bessel_i0(double x) {
    double term = 1.0, sum = 1.0;
    const double q = 0.25 * x * x;
    for (int k = 1; k < 64; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
}  // namespace

int true_peak_oversample(int sample_rate) { return (192000 + sample_rate - 1) / sample_rate; }

// table [o][24] f32: row 0 is the unit sample (phase 0 is never filtered; the row is there so that the table is the whole interpolator)
void true_peak_table(int sample_rate, float* table) {
    const int o = true_peak_oversample(sample_rate);
    const double i0b = bessel_i0(kBeta);
    for (int p = 0; p < o; ++p)
        for (int k = 0; k < kTaps; ++k) {
            const double t = (double)(k - kZ + 1) - (double)p / (double)o;
            const double u = t / (double)kZ, w = u * u < 1.0 ? bessel_i0(kBeta * sqrt(1.0 - u * u)) / i0b : 0.0;
            const double s = t == 0.0 ? 1.0 : sin(kPi * t) / (kPi * t);
            table[p * kTaps + k] = p == 0 ? (k == kZ - 1 ? 1.0f : 0.0f) : (float)(s * w);
        }
}

// positions i in [tile * kTile - Z, (tile + 1) * kTile - Z) of one utterance, by the tile of true_peak_tile.h: xs[q] = x[i0 - Z + 1 + q], so
// that the window of position i0 + q, x[i - Z + 1 .. i + Z], is xs[q .. q + 2 Z).  Thread t takes the kPer positions from q = kPer t.
// The windows use kTile + 2 Z - 1 words of xs; the last word only fills the seventh vector of the last thread.
__global__ __launch_bounds__(kTpThreads) void true_peak_kernel(EbuP p) {
    __shared__ __attribute__((aligned(16))) float xs[kTpXsWords];
    __shared__ __attribute__((aligned(16))) float hs[kTpHsWords];
    const int b = blockIdx.y, L = p.len[b], t = threadIdx.x, o = p.o;
    const long long i0 = (long long)blockIdx.x * kTile - kZ;
    float pk = 0.0f;
    if (i0 < L) {                                                             // uniform over the workgroup
        tp_tile_load(xs, hs, p.wav + (long long)b * p.L_max, i0 - kZ + 1, L, p.table, o);
        const int q0 = t * kPer;
        const long long left = (long long)L - (i0 + q0);                     // positions of this thread in front of L
        if (left > 0) {
            const TpWindows<kPer> win(xs, q0);
#pragma unroll
            for (int j = 0; j < kPer; ++j) {                                  // phase 0
                const float v = win.sample(j);
                if (j < left && v > pk) pk = v;
            }
#pragma unroll 1
            for (int ph = 1; ph < o; ++ph) {
                float a[kPer];
                win.phase(hs, ph, a);
#pragma unroll
                for (int j = 0; j < kPer; ++j)
                    if (j < left && a[j] > pk) pk = a[j];                     // a NaN never wins, an Inf does
            }
        }
    }
    wave_peak_merge<true>(pk, p.tp + b);      // most waves skip the atomic
}

namespace {
// ordered like the doubles, a NaN of either sign last; never 0, which marks a block under a gate
__device__ __forceinline__ unsigned long long range_key(double s) {
    if (s != s) return ~0ull;
    const unsigned long long u = (unsigned long long)__double_as_longlong(s);
    return (u >> 63) ? ~u : u | (1ull << 63);
}
__device__ __forceinline__ double range_unkey(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? k ^ (1ull << 63) : ~k));
}
// the key of rank `rank` (0-based, ascending) among the non-zero keys K[0 .. n): most significant byte first, a histogram of the
// keys that share the bytes chosen so far.  Thread t reads the keys t, t + 256, ..., which it wrote itself.
__device__ unsigned long long range_select(const unsigned long long* K, int n, unsigned rank, unsigned* hist, unsigned* pick) {
    const int t = threadIdx.x;
    unsigned long long prefix = 0;
    for (int shift = 56; shift >= 0; shift -= 8) {
        const unsigned long long mask = shift == 56 ? 0ull : ~0ull << (shift + 8);
        __syncthreads();
        hist[t] = 0u;
        __syncthreads();
        for (int k = t; k < n; k += kRangeThreads) {
            const unsigned long long key = K[k];
            if (key != 0ull && (key & mask) == prefix) atomicAdd(&hist[(unsigned)(key >> shift) & 255u], 1u);
        }
        __syncthreads();
        if (t < 64) {                                                         // the first wave: four bins a lane, a prefix sum by shuffles
            const unsigned h0 = hist[4 * t], h1 = hist[4 * t + 1], h2 = hist[4 * t + 2], h3 = hist[4 * t + 3], own = (h0 + h1) + (h2 + h3);
            unsigned inc = own;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = __shfl_up(inc, d);
                if (t >= d) inc += v;
            }
            const unsigned exc = inc - own;
            if (rank >= exc && rank < inc) {                                  // one lane: rank is under the number of keys counted
                unsigned r = rank - exc, d = 4u * t;
                if (r >= h0) { r -= h0; ++d; if (r >= h1) { r -= h1; ++d; if (r >= h2) { r -= h2; ++d; } } }
                pick[0] = d; pick[1] = r;
            }
        }
        __syncthreads();
        prefix |= (unsigned long long)pick[0] << shift;
        rank = pick[1];
    }
    return prefix;
}
}  // namespace

// short-term loudness, both gates of Tech 3342, the two percentiles and the 18 doubles of one utterance; the gain word of the
// normalising call.  A block is over a gate unless s <= gate, as in the gate kernel.
__global__ __launch_bounds__(kRangeThreads) void loudness_range_kernel(EbuP p) {
    __shared__ double sv[kRangeThreads];
    __shared__ int sn[kRangeThreads];
    __shared__ unsigned hist[256];
    __shared__ unsigned pick[2];
    const int b = blockIdx.x, t = threadIdx.x, ns = p.len[b] / p.h, nst = ns > 29 ? ns - 29 : 0;
    const double* __restrict__ S = p.sums + (long long)b * p.NS;
    double* Z3 = p.keys + (long long)b * p.NST;
    unsigned long long* K = reinterpret_cast<unsigned long long*>(Z3);
    const double den = 30.0 * (double)p.h, ninf = -HUGE_VAL;
    double sum = 0.0, smax = ninf;
    int cnt = 0;
    for (int k = t; k < nst; k += kRangeThreads) {
        double a = S[k];
#pragma unroll
        for (int q = 1; q < 30; ++q) a += S[k + q];
        const double z = a / den, s = -0.691 + 10.0 * log10(z);
        Z3[k] = z;
        if (p.short_term) p.short_term[(long long)b * p.NST_max + k] = s;
        smax = fmax(smax, s);
        if (!(s <= -70.0)) { sum += z; ++cnt; }
    }
    if (p.short_term)
        for (int k = nst + t; k < p.NST_max; k += kRangeThreads) p.short_term[(long long)b * p.NST_max + k] = ninf;
    block_tree_sum<kRangeThreads>(sv, sn, &sum, &cnt);
    const int n_abs = cnt;
    const double gamma = n_abs > 0 ? -0.691 + 10.0 * log10(sum / (double)n_abs) - 20.0 : ninf;
    sum = 0.0; cnt = 0;
    for (int k = t; k < nst; k += kRangeThreads) {
        const double s = -0.691 + 10.0 * log10(Z3[k]);
        const bool over = !(s <= -70.0) && !(s <= gamma);
        K[k] = over ? range_key(s) : 0ull;
        cnt += over ? 1 : 0;
    }
    block_tree_sum<kRangeThreads>(sv, sn, &sum, &cnt);
    const int n = cnt;
    smax = block_tree_max<kRangeThreads>(sv, smax);
    double p10 = nan(""), p95 = nan("");
    if (n > 0) {                                                              // uniform over the workgroup
        p10 = range_unkey(range_select(K, nst, (unsigned)(((long long)(n - 1) * 10 + 50) / 100), hist, pick));
        p95 = range_unkey(range_select(K, nst, (unsigned)(((long long)(n - 1) * 95 + 50) / 100), hist, pick));
    }
    if (t != 0) return;
    const double* __restrict__ row = p.row8 + (long long)b * 8;
    const float tp = __uint_as_float(p.tp[b]);
    double g7 = row[7];
    if (p.gain) {
        const double I = row[0];
        float g = 1.0f;
        if (isfinite(I)) {
            const double gd = pow(10.0, (p.target_lufs - I) / 20.0), cap = pow(10.0, p.ceiling_dbtp / 20.0) / (double)tp;
            g = tp > 0.0f && cap < gd ? __double2float_rz(cap) : (float)gd;   // toward zero where the cap binds: never over the ceiling
            if (!isfinite(g)) g = 1.0f;
        }
        p.gain[b] = g;
        g7 = (double)g;
    }
    if (p.stats) {
        double* __restrict__ o = p.stats + (long long)b * MT2_EBU_FIELDS;
#pragma unroll
        for (int q = 0; q < 7; ++q) o[q] = row[q];
        o[7] = g7; o[8] = (double)tp; o[9] = (double)p.o; o[10] = p95 - p10; o[11] = (double)nst; o[12] = (double)n_abs; o[13] = (double)n;
        o[14] = gamma; o[15] = p10; o[16] = p95; o[17] = smax;
    }
}

hipError_t launch_true_peak(const EbuP& p, hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.max_len < 1 || p.max_len > p.L_max || p.o < 1 || p.o > kMaxOver || p.table == nullptr || p.tp == nullptr)
        return hipErrorInvalidValue;
    const long long tiles = ((long long)p.max_len + kZ + kTile - 1) / kTile;
    hipLaunchKernelGGL(true_peak_kernel, dim3((unsigned)tiles, p.B), dim3(kTpThreads), 0, s, p);
    return hipGetLastError();
}
hipError_t launch_loudness_range(const EbuP& p, hipStream_t s) {
    if (p.B < 1 || p.h < 800 || p.NS < p.max_len / p.h || p.NST < std::max(p.max_len / p.h - 29, 0) || p.row8 == nullptr || p.keys == nullptr ||
        (p.short_term && p.NST_max < std::max(p.max_len / p.h - 29, 0)))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(loudness_range_kernel, dim3(p.B), dim3(kRangeThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
