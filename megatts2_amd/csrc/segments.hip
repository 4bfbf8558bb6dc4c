// Speech segments of prompt audio by frame energy, and the cut that takes the pauses out (gfx950).  The frames and their energies are
// trim.hip's, by its two kernels as they are; everything behind them is here.  The rule is our own (parity with librosa.effects.split,
// webrtcvad or a model-based VAD is unpinned), stated in include/megatts2_hip.h and restated in
// tests/segments_ref.py.  For one utterance of F frames with energies e[f], E = max(0, max_f e[f]), c = trim_factor(top_db):
//
//   a[f] = e[f] > E * c (one f32 product);  E < FLT_MIN: every frame                                         raw activity
//   b[f] = a[f], or f lies in an inactive run BETWEEN two active frames that is shorter than min_pause         close
//   c[f] = b[f] and the run of b that holds f is at least min_speech frames long                               open
//   d[f] = some g with |g - f| <= pad has c[g];  c empty: d is all true ("nothing found")                      pad
//   segment k = the k-th maximal run [f0, f1] of d;  kept frames (d, or !d with keep = pauses) move to 512 * (kept frames before)
//
// segments_smooth_kernel: ONE workgroup of 256 threads per utterance walks the frames in chunks of 256, one frame per thread, seven
// times.  Each step of the rule is a forward pass and a backward pass over the frames:
//   forward   an inclusive max-scan of "f if the flag holds, else -1" = the nearest flagged frame at or before f, kept in prv[]
//   backward  the same as a min-scan from the right = the nearest flagged frame at or after f, met with prv[f] to decide the step
// A scan is 6 shuffle steps in the wave, the 4 wave totals through LDS, and ONE register per pass that carries the total of the
// chunks already seen - so F is bounded by the buffers alone.  The backward passes give thread t the frame 255 - t of the chunk and
// take the chunks from the last to the first, which makes them the same forward scan over threads.  The seventh pass numbers the
// runs of d and the kept frames by two add-scans.  No atomics; nothing but the utterance's own frames enters, so a ragged batch is
// bit-identical to its utterances alone.
// segments_figures_kernel: one workgroup per utterance, the two energy sums in double - thread-strided ascending, then block_tree_sum.
// segments_copy_kernel: a grid over (tiles of 8 frames, b); a kept frame is 512 samples = 128 16-byte moves when both row bases are
// 16-byte aligned (both offsets are multiples of 512 samples); the last frame is partial, samples at or beyond len[b] are never read.
#include "../../include/megatts2_hip.h"
#include "mt2_block_reduce.h"
#include "mt2_kernels.h"

#include <float.h>
#include <limits.h>

#include <algorithm>

namespace mt2 {

namespace {
constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kHop = MT2_TRIM_HOP;
constexpr int kCopyFrames = 8;                         // frames of a copy tile (16 KiB of audio), two at a time
static_assert(kThreads == MT2_SEGMENTS_CHUNK, "the chunk of the smoothing passes is one frame per thread");
static_assert(kHop == 512 && kThreads * 4 == 2 * kHop, "a copy step is two frames of 128 16-byte moves");

struct OpMax { static constexpr int id = -1;      static __device__ __forceinline__ int f(int a, int b) { return max(a, b); } };
struct OpMin { static constexpr int id = INT_MAX; static __device__ __forceinline__ int f(int a, int b) { return min(a, b); } };
struct OpAdd { static constexpr int id = 0;       static __device__ __forceinline__ int f(int a, int b) { return a + b; } };
}  // namespace

long long segments_bound(long long F, int min_pause, int min_speech) {
    return std::max<long long>(1, (F + (long long)min_pause) / ((long long)min_speech + (long long)min_pause));
}

// the inclusive scan of one value per thread over the workgroup, in thread order; *total = the scan's last value, in every thread.
// red: kWaves ints
template <class Op> __device__ __forceinline__ int block_scan(int v, int* red, int* total) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int u = __shfl_up(v, d);
        if (lane >= d) v = Op::f(v, u);
    }
    __syncthreads();                           // the previous use of red[] is over
    if (lane == 63) red[w] = v;
    __syncthreads();
    int pre = Op::id, tot = Op::id;
#pragma unroll
    for (int k = 0; k < kWaves; ++k) {
        const int r = red[k];
        if (k < w) pre = Op::f(pre, r);
        tot = Op::f(tot, r);
    }
    *total = tot;
    return Op::f(pre, v);
}

__global__ __launch_bounds__(kThreads) void segments_smooth_kernel(SegP p) {
    __shared__ int red[kWaves];
    __shared__ float redf[kWaves];
    const int b = blockIdx.x, F = p.flen[b], t = threadIdx.x;
    const size_t row = (size_t)b * p.W;
    const float* __restrict__ e = p.energy + (size_t)b * p.E_pitch;
    int* __restrict__ prv = p.prv + row;
    unsigned char* __restrict__ fb = p.fb + row;
    unsigned char* __restrict__ fc = p.fc + row;
    unsigned char* __restrict__ fd = p.flags ? p.flags + (size_t)b * p.D_pitch : p.fd + row;
    const int nch = (F + kThreads - 1) / kThreads;
    int tot;

    // E: a max is the same in any order; a NaN never wins an fmaxf, as in trim's peak
    float m = 0.0f;
    for (int f = t; f < F; f += kThreads) m = fmaxf(m, e[f]);
    m = wave_max(m);
    if ((t & 63) == 0) redf[t >> 6] = m;
    __syncthreads();
    const float E = fmaxf(fmaxf(redf[0], redf[1]), fmaxf(redf[2], redf[3]));
    const bool silent = !(E >= FLT_MIN);
    const float thr = __fmul_rn(E, p.factor);

    // 1  a, forward: prv[f] = the nearest active frame at or before f
    int carry = -1, raw = 0;
    for (int c = 0; c < nch; ++c) {
        const int f = c * kThreads + t;
        const bool a = f < F && (silent || e[f] > thr);
        raw += a;
        const int v = max(block_scan<OpMax>(a ? f : -1, red, &tot), carry);
        if (f < F) prv[f] = v;
        carry = max(carry, tot);
    }
    __syncthreads();
    // 2  a, backward: close
    carry = INT_MAX;
    for (int c = nch - 1; c >= 0; --c) {
        const int f = c * kThreads + (kThreads - 1 - t);
        const bool a = f < F && (silent || e[f] > thr);
        const int nx = min(block_scan<OpMin>(a ? f : INT_MAX, red, &tot), carry);
        if (f < F) {
            const int pv = prv[f];
            fb[f] = a || (pv >= 0 && nx != INT_MAX && nx - pv - 1 < p.min_pause);
        }
        carry = min(carry, tot);
    }
    __syncthreads();
    // 3  b, forward: prv[f] = the nearest run start at or before f
    carry = -1;
    for (int c = 0; c < nch; ++c) {
        const int f = c * kThreads + t;
        const bool st = f < F && fb[f] && (f == 0 || !fb[f - 1]);
        const int v = max(block_scan<OpMax>(st ? f : -1, red, &tot), carry);
        if (f < F) prv[f] = v;
        carry = max(carry, tot);
    }
    __syncthreads();
    // 4  b, backward: the nearest run end at or after f; open
    carry = INT_MAX;
    for (int c = nch - 1; c >= 0; --c) {
        const int f = c * kThreads + (kThreads - 1 - t);
        const bool on = f < F && fb[f];
        const bool en = on && (f == F - 1 || !fb[f + 1]);
        const int nx = min(block_scan<OpMin>(en ? f : INT_MAX, red, &tot), carry);
        if (f < F) fc[f] = on && nx - prv[f] + 1 >= p.min_speech;
        carry = min(carry, tot);
    }
    __syncthreads();
    // 5  c, forward: prv[f] = the nearest frame of c at or before f
    carry = -1;
    for (int c = 0; c < nch; ++c) {
        const int f = c * kThreads + t;
        const bool on = f < F && fc[f];
        const int v = max(block_scan<OpMax>(on ? f : -1, red, &tot), carry);
        if (f < F) prv[f] = v;
        carry = max(carry, tot);
    }
    const bool found = carry >= 0;
    __syncthreads();
    // 6  c, backward: pad (clamped to [0, F) by the scans themselves); nothing found: all true
    carry = INT_MAX;
    for (int c = nch - 1; c >= 0; --c) {
        const int f = c * kThreads + (kThreads - 1 - t);
        const bool on = f < F && fc[f];
        const int nx = min(block_scan<OpMin>(on ? f : INT_MAX, red, &tot), carry);
        if (f < F) {
            const int pv = prv[f];
            fd[f] = !found || (pv >= 0 && f - pv <= p.pad) || (nx != INT_MAX && nx - f <= p.pad);
        }
        carry = min(carry, tot);
    }
    __syncthreads();
    // 7  d, forward: the runs and the kept frames numbered, the longest pause between two runs
    const int L = p.len ? p.len[b] : 0;
    int* __restrict__ seg = p.seg ? p.seg + (size_t)b * p.S_max * 2 : nullptr;
    int* __restrict__ dst = p.dst + row;
    int nk = 0, ns = 0, last = -1, longest = 0;
    for (int c = 0; c < nch; ++c) {
        const int f = c * kThreads + t;
        const bool in = f < F;
        const bool on = in && fd[f];
        const bool st = on && (f == 0 || !fd[f - 1]), en = on && (f == F - 1 || !fd[f + 1]);
        const bool kept = in && (p.keep ? !on : on);
        const int ik = nk + block_scan<OpAdd>(kept, red, &tot);
        nk += tot;
        const int is = ns + block_scan<OpAdd>(st, red, &tot);
        ns += tot;
        const int ld = max(block_scan<OpMax>(on ? f : -1, red, &tot), last);
        last = max(last, tot);
        if (in) dst[f] = kept ? ik - 1 : -1;
        if (seg && is - 1 < p.S_max) {
            if (st) seg[2 * (is - 1)] = p.len ? kHop * f : f;
            if (en) seg[2 * (is - 1) + 1] = p.len ? (int)min((long long)L, (long long)kHop * (f + 1)) : f + 1;
        }
        // the last frame of a pause that a run follows: the pause began behind the nearest frame of d before it
        if (in && !on && f + 1 < F && fd[f + 1] && ld >= 0) longest = max(longest, f - ld);
    }
    block_scan<OpMax>(longest, red, &longest);
    block_scan<OpAdd>(raw, red, &raw);
    if (seg)
        for (int k = 2 * ns + t; k < 2 * p.S_max; k += kThreads) seg[k] = -1;
    if (t == 0) {
        const bool kept_last = p.keep ? !fd[F - 1] : fd[F - 1];      // written in pass 6, behind its barrier
        long long samples = (long long)kHop * nk;
        if (p.len && kept_last) samples -= kHop - (L - kHop * (F - 1));      // what the last frame lacks: it owns [512 (F - 1), L)
        int* w = p.words + (size_t)b * kSegWords;
        w[0] = F; w[1] = raw; w[2] = nk; w[3] = found ? ns : -ns; w[4] = longest;
        w[5] = (int)min(samples, (long long)INT_MAX);
        w[6] = 0; w[7] = 0;
        if (p.counts) p.counts[b] = ns;
    }
}

// figures[b] = F, raw active frames, kept frames, segments (negative: nothing found), kept samples, longest pause, mean e over the
// kept frames, mean e over the dropped ones
__global__ __launch_bounds__(kThreads) void segments_figures_kernel(SegP p) {
    __shared__ double red[kThreads];
    const int b = blockIdx.x, F = p.flen[b];
    const float* __restrict__ e = p.energy + (size_t)b * p.E_pitch;
    const unsigned char* __restrict__ fd = p.flags ? p.flags + (size_t)b * p.D_pitch : p.fd + (size_t)b * p.W;
    double sk = 0.0, sd = 0.0;
    for (int f = threadIdx.x; f < F; f += kThreads) {
        const bool kept = p.keep ? !fd[f] : fd[f];
        if (kept) sk += (double)e[f]; else sd += (double)e[f];
    }
    sk = block_tree_sum<kThreads>(red, sk);
    sd = block_tree_sum<kThreads>(red, sd);
    if (threadIdx.x == 0) {
        const int* w = p.words + (size_t)b * kSegWords;
        double* g = p.fig + (size_t)b * MT2_SEGMENTS_FIELDS;
        const int nk = w[2], nd = F - w[2];
        g[0] = F; g[1] = w[1]; g[2] = nk; g[3] = w[3];
        g[4] = p.len ? (double)w[5] : (double)kHop * (double)nk;
        g[5] = w[4];
        g[6] = nk ? sk / nk : 0.0;
        g[7] = nd ? sd / nd : 0.0;
    }
}

// out[b, 512 dst[f] + i] = wav[b, 512 f + i] for the kept frames, zeros from the kept samples on up to Lout_max
__global__ __launch_bounds__(kThreads) void segments_copy_kernel(SegP p) {
    const int b = blockIdx.y, L = p.len[b], F = p.flen[b];
    const float* __restrict__ x = p.wav + (size_t)b * p.L_max;
    float* __restrict__ out = p.out + (size_t)b * p.Lout_max;
    const int* __restrict__ dst = p.dst + (size_t)b * p.W;
    const bool vec = ((reinterpret_cast<uintptr_t>(x) | reinterpret_cast<uintptr_t>(out)) & 15) == 0;
    const int i = 4 * (threadIdx.x & 127);
    for (int k = threadIdx.x >> 7; k < kCopyFrames; k += 2) {
        const long long f = (long long)blockIdx.x * kCopyFrames + k;
        if (f >= F) break;
        const int g = dst[f];
        if (g < 0) continue;
        const long long s0 = f * kHop + i, d0 = (long long)g * kHop + i;      // d0 <= s0 < L <= Lout_max
        if (vec && s0 + 3 < L) {
            *reinterpret_cast<float4*>(out + d0) = *reinterpret_cast<const float4*>(x + s0);
        } else {
            for (int q = 0; q < 4 && s0 + q < L; ++q) out[d0 + q] = x[s0 + q];
        }
    }
    const int n = p.words[(size_t)b * kSegWords + 5];
    for (long long j = (n & ~3) + ((long long)blockIdx.x * kThreads + threadIdx.x) * 4; j < p.Lout_max; j += (long long)gridDim.x * kThreads * 4) {
        if (vec && j >= n && j + 3 < p.Lout_max) {
            *reinterpret_cast<float4*>(out + j) = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        } else {
            for (int q = 0; q < 4 && j + q < p.Lout_max; ++q)
                if (j + q >= n) out[j + q] = 0.0f;
        }
    }
}

hipError_t launch_segments(const SegP& p, int what, hipStream_t s) {
    if (p.B <= 0) return hipSuccess;
    if (p.B > 65535 || p.max_F < 1 || p.max_F > p.W || p.max_F > p.E_pitch || (p.flags && p.D_pitch < p.max_F) || p.max_F > INT_MAX / kHop ||
        p.min_speech < 2 || p.pad < 0 || (long long)p.min_pause <= 2ll * p.pad ||
        (p.seg && p.S_max < segments_bound(p.max_F, p.min_pause, p.min_speech)) || ((what & kSegFigures) && !p.fig) ||
        ((what & kSegCopy) && (!p.out || !p.len || !p.wav || p.Lout_max < 1)))
        return hipErrorInvalidValue;
    if (what & kSegSmooth) hipLaunchKernelGGL(segments_smooth_kernel, dim3(p.B), dim3(kThreads), 0, s, p);
    if (what & kSegFigures) hipLaunchKernelGGL(segments_figures_kernel, dim3(p.B), dim3(kThreads), 0, s, p);
    if (what & kSegCopy) hipLaunchKernelGGL(segments_copy_kernel, dim3((p.max_F + kCopyFrames - 1) / kCopyFrames, p.B), dim3(kThreads), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
