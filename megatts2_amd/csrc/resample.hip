// Sample-rate conversion of prompt audio (gfx950): what `librosa.load(wav, sr=16000)` + `librosa.util.normalize` do in
// front of the mel front-end (reference models/megatts2.py:335-336).  librosa's soxr filter is not reproduced (parity
// unpinned); the rule is the Kaiser-windowed-sinc polyphase filter in the form torchaudio documents for
// resample(..., resampling_method="sinc_interp_kaiser") with its "kaiser_best" constants:
//
//   g = gcd(sr_in, sr_out), o = sr_in / g, n = sr_out / g, base = min(o, n) * rolloff, width = ceil(lpw * o / base)
//   K = 2 * width + o taps per phase
//   t[p][k] = clamp((-p / n + (k - width) / o) * base, -lpw, +lpw)
//   h[p][k] = sinc(pi t) * I0(beta * sqrt(1 - (t / lpw)^2)) / I0(beta) * (base / o)              (double, rounded ONCE to f32)
//   y[i * n + p] = sum_{k < K} h[p][k] * x[i * o - width + k],  x = 0 outside [0, L),  y cut to ceil(n * L / o) samples
//
// Every output sample is ONE f32 fma chain over k ascending: it depends on its utterance's samples and on (o, n) only - not on
// the tile size, the batch, the slot or L_max - so a ragged batch is bit-identical to its utterances resampled one by one.
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <float.h>
#include <math.h>

#include <algorithm>
#include <numeric>

namespace mt2 {

namespace {
constexpr double kLpw = 64.0;                          // zero crossings on each side
constexpr double kRolloff = 0.9475937167399596;
constexpr double kBeta = 14.769656459379492;
constexpr int kThreads = 256;
constexpr int kHead = 16;                              // floats in front of the window: the peak reduction's scratch (keeps the window on 16 bytes)
constexpr int kLdsPreferred = 8192;                    // floats of LDS a workgroup takes when the filter leaves it the choice (32 KiB: 5 workgroups / CU)
constexpr int kLdsMost = 16384;                        // ... and at the most (64 KiB: no opt-in needed)
constexpr int kChains = 4;                             // samples a lane accumulates at a time (each its own chain)
constexpr int kTileOutputs = 4096;                     // outputs of one workgroup at the most (short filters: keeps the grid wide)
constexpr long long kTableBytesMost = 8ll << 20;

// I0 by its power series (all terms positive: no cancellation; x <= beta here)
double bessel_i0(double x) {
    const double q = 0.25 * x * x;
    double sum = 1.0, term = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < sum * 1e-18) break;
    }
    return sum;
}
}  // namespace

const char* resample_rule(int sr_in, int sr_out, ResampleRule* r) {
    if (sr_in <= 0 || sr_out <= 0) return "sample rates must be positive";
    if (sr_in == sr_out) return "sr_in == sr_out: there is nothing to resample";
    const int g = std::gcd(sr_in, sr_out);
    const long long o = sr_in / g, n = sr_out / g;
    const double base = (double)std::min(o, n) * kRolloff;
    const double width = std::ceil(kLpw * (double)o / base);
    const double taps = 2.0 * width + (double)o;
    if ((double)n * taps * 4.0 > (double)kTableBytesMost) return "the filter table of this ratio (n * taps * 4 bytes) exceeds 8 MiB";
    if (taps + kHead + 8 > kLdsMost) return "one phase of this ratio's filter does not fit the 64 KiB LDS window";
    r->o = (int)o; r->n = (int)n; r->width = (int)width; r->taps = (int)taps;
    const int spare = kLdsPreferred - kHead - 8 - r->taps;
    r->tb = std::min(spare >= 0 ? spare / r->o + 1 : 1, std::max(1, kTileOutputs / r->n));
    return nullptr;
}

long long resample_out_len(const ResampleRule& r, long long L) { return (r.n * L + r.o - 1) / r.o; }

static size_t resample_lds_bytes(const ResampleRule& r) {
    // window of (tb - 1) * o + taps floats, up to 3 in front (the start is moved down to a 16-byte boundary of the input) and
    // rounded up to whole float4
    return sizeof(float) * (size_t)(kHead + (((r.tb - 1) * r.o + r.taps + 3 + 3) & ~3));
}

void resample_table(const ResampleRule& r, float* table, bool tap_major) {
    const double PI = 3.14159265358979323846;
    const double base = (double)std::min(r.o, r.n) * kRolloff, scale = base / (double)r.o, i0_beta = bessel_i0(kBeta);
    for (int p = 0; p < r.n; ++p)
        for (int k = 0; k < r.taps; ++k) {
            double t = (-(double)p / (double)r.n + (double)(k - r.width) / (double)r.o) * base;
            t = std::min(std::max(t, -kLpw), kLpw);
            const double u = t / kLpw, window = bessel_i0(kBeta * std::sqrt(1.0 - u * u)) / i0_beta;
            const double a = t * PI, sinc = a == 0.0 ? 1.0 : std::sin(a) / a;
            table[tap_major ? (size_t)k * r.n + p : (size_t)p * r.taps + k] = (float)(sinc * (window * scale));
        }
}

// One workgroup = one utterance's run of tb consecutive output blocks (block i = outputs i * n .. i * n + n - 1, all fed by the
// inputs i * o - width .. i * o - width + taps - 1).  The run's input window is staged ONCE in LDS with 16-byte loads; a sample
// outside [0, len) is a zero by its index, never a read.  Lanes walk the run's outputs, phase fastest; the table is tap-major [taps][n],
// so lanes of consecutive phase read consecutive floats (n = 1: one address for the wave) and lanes of one block read one LDS word.
__global__ __launch_bounds__(kThreads) void resample_rows_kernel(ResampleP p) {
    extern __shared__ __attribute__((aligned(16))) float rs_lds[];
    float* const red = rs_lds;
    float* const win = rs_lds + kHead;
    const int b = p.tile_b[blockIdx.x], i0 = p.tile_i0[blockIdx.x];
    const int o = p.r.o, n = p.r.n, K = p.r.taps;
    const int L = p.len[b], Lout = p.lout[b];
    const long long j0 = (long long)i0 * n;
    const long long j1 = min(j0 + (long long)p.r.tb * n, (long long)p.Lout_max);       // end of what this workgroup writes
    const long long jv = min(j1, (long long)Lout);                                     // ... of its real samples
    float* __restrict__ out = p.out + (long long)b * p.Lout_max;
    float peak = 0.0f;
    if (j0 < jv) {
        const int nb = (int)((jv - j0 + n - 1) / n);                                   // blocks with a real sample
        const long long row = (long long)b * p.L_max, s0 = (long long)i0 * o - p.r.width;
        const int sh = (int)((p.a0 + row + s0) & 3);                                   // window element q holds x[s0 - sh + q]
        const int W4 = ((nb - 1) * o + K + sh + 3) & ~3;
        const float* __restrict__ x = p.wav + row;
        for (int q = threadIdx.x * 4; q < W4; q += kThreads * 4) {
            const long long s = s0 - sh + q;
            float4 v;
            if (s >= 0 && s + 3 < L) {
                v = *reinterpret_cast<const float4*>(x + s);
            } else {
                v.x = s >= 0 && s < L ? x[s] : 0.0f;
                v.y = s + 1 >= 0 && s + 1 < L ? x[s + 1] : 0.0f;
                v.z = s + 2 >= 0 && s + 2 < L ? x[s + 2] : 0.0f;
                v.w = s + 3 >= 0 && s + 3 < L ? x[s + 3] : 0.0f;
            }
            *reinterpret_cast<float4*>(win + q) = v;
        }
        __syncthreads();
        // a lane's work item = one phase of kChains blocks G apart: a table value is read once for kChains samples, whose
        // chains run side by side; lanes of one phase run through consecutive blocks (LDS stride o)
        const int G = (nb + kChains - 1) / kChains;
        for (int w = threadIdx.x; w < G * n; w += kThreads) {
            const int g = w / n, ph = w - g * n;
            const float* __restrict__ h = p.table + ph;
            const float* xw[kChains];
            float acc[kChains];
#pragma unroll
            for (int r = 0; r < kChains; ++r) {
                xw[r] = win + sh + min(g + r * G, nb - 1) * o;      // a block past the run: a copy of the last one, not stored
                acc[r] = 0.0f;
            }
#pragma unroll 2
            for (int k = 0; k < K; ++k) {
                const float hk = h[(size_t)k * n];
#pragma unroll
                for (int r = 0; r < kChains; ++r) acc[r] = fmaf(hk, xw[r][k], acc[r]);
            }
#pragma unroll
            for (int r = 0; r < kChains; ++r) {
                const long long j = j0 + (long long)(g + r * G) * n + ph;
                if (g + r * G < nb && j < jv) {
                    out[j] = acc[r];
                    peak = fmaxf(peak, fabsf(acc[r]));
                }
            }
        }
    }
    for (long long j = max(j0, (long long)Lout) + threadIdx.x; j < j1; j += kThreads) out[j] = 0.0f;
    if (p.peak) block_peak_merge(peak, red, p.peak + b);
}

hipError_t launch_resample_rows(const ResampleP& p, hipStream_t s) {
    if (p.tiles <= 0) return hipSuccess;
    const size_t lds = resample_lds_bytes(p.r);
    if (lds > sizeof(float) * (size_t)kLdsMost || p.r.tb < 1 || ((uintptr_t)p.wav & 3)) return hipErrorInvalidValue;
    ResampleP q = p;
    q.a0 = (int)(((uintptr_t)p.wav >> 2) & 3);
    hipLaunchKernelGGL(resample_rows_kernel, dim3(q.tiles), dim3(kThreads), lds, s, q);
    return hipGetLastError();
}

// peak[b] = max(peak[b], max_{j < len[b]} |x[b, j]|) as the u32 pattern (the caller zeroes the words); samples beyond len[b] are not read
__global__ __launch_bounds__(kThreads) void peak_rows_kernel(const float* x, long long stride, const int* len, unsigned* peak) {
    __shared__ float red[4];
    const int b = blockIdx.y, L = len[b];
    const float* __restrict__ xr = x + (long long)b * stride;
    float v = 0.0f;
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < L; j += (long long)gridDim.x * kThreads)
        v = fmaxf(v, fabsf(xr[j]));
    block_peak_merge(v, red, peak + b);
}
hipError_t launch_peak_rows(const float* x, long long stride, const int* len, int max_len, int B, unsigned* peak, hipStream_t s) {
    if (B <= 0 || max_len <= 0) return hipSuccess;
    const int gx = (int)std::min<long long>(((long long)max_len + kThreads * 8 - 1) / (kThreads * 8), 256);
    hipLaunchKernelGGL(peak_rows_kernel, dim3(gx, B), dim3(kThreads), 0, s, x, stride, len, peak);
    return hipGetLastError();
}

// librosa.util.normalize per utterance: out[b, j] = x[b, j] / peak[b] (correctly rounded f32 division; unchanged while the peak is
// below FLT_MIN) for j < len[b], 0 for len[b] <= j < width.  x may be out (in place).
__global__ __launch_bounds__(kThreads) void scale_rows_kernel(const float* x, long long xstride, const int* len, const unsigned* peak,
                                                              float* out, long long ostride, int width) {
    const int b = blockIdx.y, L = len[b];
    const float pk = __uint_as_float(peak[b]);
    const bool scale = pk >= FLT_MIN;
    const float* xr = x + (long long)b * xstride;
    float* outr = out + (long long)b * ostride;
    for (long long j = (long long)blockIdx.x * kThreads + threadIdx.x; j < width; j += (long long)gridDim.x * kThreads) {
        float v = 0.0f;
        if (j < L) v = scale ? __fdiv_rn(xr[j], pk) : xr[j];
        outr[j] = v;
    }
}
hipError_t launch_scale_rows(const float* x, long long xstride, const int* len, const unsigned* peak, float* out, long long ostride,
                             int width, int B, hipStream_t s) {
    if (B <= 0 || width <= 0) return hipSuccess;
    const int gx = (int)std::min<long long>(((long long)width + kThreads * 4 - 1) / (kThreads * 4), 1024);
    hipLaunchKernelGGL(scale_rows_kernel, dim3(gx, B), dim3(kThreads), 0, s, x, xstride, len, peak, out, ostride, width);
    return hipGetLastError();
}

}  // namespace mt2
