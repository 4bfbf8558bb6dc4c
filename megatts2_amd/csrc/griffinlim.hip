// Griffin-Lim vocoder: a log-mel becomes audio with no weights at all - the fallback behind the HiFi-GAN generator (whose weights are
// a third-party hub model) and the project's only closed loop: istft(stft(x)) = x, mel(griffin_lim(mel(x))) ~ mel(x).  Parity with
// librosa.griffinlim / torchaudio.transforms.GriffinLim is unpinned (neither is on hand); the rule is our own statement, held to its
// restatement tests/griffinlim_ref.py.
//
// The rule, for one utterance: log-mel M f32 [T, n_mels], 64-bit seed; audio configuration (n_fft N, hop h, win_length, n_mels, ...),
// F = N/2 + 1, taps = N/h >= 2, w[k] the front-end's window (periodic Hann centred in N).  Output x f32 [L], L = (T - 1) h: the exact
// inverse of the front-end's framing (1 + L / h = T).
//   1 mel -> linear   P = fb^T (fb fb^T)^-1 by Cholesky in double from the f32 filterbank fb of the front-end, rounded once to f32 (the
//                     pseudo-inverse for full row rank; a Gram matrix that is not positive definite is refused);
//                     A[t, f] = max(0, sum_j expf(M[t, j]) P[f, j])      (one f32 exp per value, an f32-equivalent dot over j)
//   2 phase           u = (x0 >> 8) 2^-24, x0 = first word of Philox4x32-10, key = seed, counter = (t F + f, 0, 0, 0) (philox.h: the
//                     generator and convention of sampling.hip); theta = 2 pi u in f32; S0[t, f] = A[t, f] (cos theta, sin theta).
//                     The counter is local to the utterance: a batch draws what its utterances draw alone.
//   3 inverse STFT    y_t = irfft_N(S_t) w (the imaginary parts of bins 0 and N/2 ignored) - a GEMM against a basis built in double
//                     with w and the 1/N, 2/N Hermitian weights folded in, rounded once;
//                     s[p] = sum_t y_t[p - t h],  e[p] = sum_t w2[p - t h]  over the EXISTING frames 0 <= t < T that cover p, in
//                     ascending t, plain f32 adds, w2 = w^2 rounded once from double;  x[n] = s[n + N/2] / e[n + N/2], one true
//                     division (torch.istft, center=True, length = (T - 1) h).  Gather form: no atomics, no sum split across lanes.
//   4 forward STFT    exactly the front-end's: reflect padding by N/2, hop-sized blocks, windowed DFT basis, [re | im] rows.
//   5 iteration       c = (float)(momentum / (1 + momentum)), Rprev = 0; for k < n_iter:  x_k = istft(S_k),  R = stft(x_k),
//                     D = R - c Rprev (one product, one difference),  S_{k+1} = D (A / (|D| + 1e-16)),  Rprev = R
//                     (the form torchaudio documents for functional.griffinlim);  x = istft(S_{n_iter}).
//   6 residual        on request resid[k, t] = sum_f (|R_k[t, f]| - A[t, f])^2, k = 0 .. n_iter (entry n_iter: one extra STFT of x):
//                     lane l of one wave sums f = l, l + 64, ... ascending, then five-step xor butterfly - a fixed order.
// Frames of all utterances are packed rows; a sample, a frame and a residual depend on their utterance alone, and the two large GEMMs
// run on ONE tile whatever the row count (model_stages.hip), so a ragged batch is bit-identical to its utterances alone.
//
// Kernels: gl_exp_rows (expf of the packed mel rows), gl_phase_init, istft_ola_blocks (the overlap-add written straight into the
// reflect-padded hop-block buffer the STFT convolution reads: a block element computes its own mirrored source, no padding launch
// between the two GEMMs), istft_ola_wav (the last pass: the caller's [B, L_max], zero-filled) and gl_phase_update (one wave a frame).
#include "mt2_kernels.h"
#include "philox.h"
#include <math.h>

namespace mt2 {
namespace {

constexpr int kThreads = 256;
inline dim3 grid_for(long long items) {
    long long g = (items + kThreads - 1) / kThreads;
    if (g < 1) g = 1;
    if (g > (1 << 20)) g = 1 << 20;
    return dim3((unsigned)g);
}

// out[r, j] = expf(mel[rowmap[r] * C + j]); C % 4 == 0; vec: mel on 16 bytes
__global__ void gl_exp_rows_kernel(const float* mel, int C, const int* rowmap, float* out, int R, int vec) {
    const int c4n = C >> 2;
    const long long total = (long long)R * c4n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / c4n), c = (int)(i % c4n) * 4;
        const float* src = mel + (long long)rowmap[r] * C + c;
        float4 v;
        if (vec) v = *reinterpret_cast<const float4*>(src);
        else v = make_float4(src[0], src[1], src[2], src[3]);
        v.x = expf(v.x); v.y = expf(v.y); v.z = expf(v.z); v.w = expf(v.w);
        *reinterpret_cast<float4*>(out + (long long)r * C + c) = v;
    }
}

// S[r, f] = A[r, f] cos(theta), S[r, F + f] = A[r, f] sin(theta), columns 2F .. lds-1 zero; theta = 2 pi u(seed of row_b[r], row_t[r] F + f)
__global__ void gl_phase_init_kernel(const float* A, int lda, const int* row_b, const int* row_t, const uint32_t* seeds, float* S,
                                     int lds_, int F, int R) {
    const long long total = (long long)R * F;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / F), f = (int)(i % F);
        const int b = row_b[r];
        const uint32_t ctr = (uint32_t)row_t[r] * (uint32_t)F + (uint32_t)f;
        const uint32_t x0 = philox_x0(ctr, 0u, 0u, 0u, seeds[2 * b], seeds[2 * b + 1]);
        const float u = (float)(x0 >> 8) * 5.9604644775390625e-8f;      // 2^-24: exact
        const float theta = __fmul_rn(6.2831853071795864769f, u);
        float sn, cs;
        sincosf(theta, &sn, &cs);
        const float a = A ? A[(long long)r * lda + f] : 1.0f;
        float* row = S + (long long)r * lds_;
        row[f] = __fmul_rn(a, cs);
        row[F + f] = __fmul_rn(a, sn);
        if (f < lds_ - 2 * F) row[2 * F + f] = 0.0f;
    }
}

// the overlap-add of one utterance at padded position p (= sample p - N/2): frames [T, N] at fr, frames t_lo .. t_hi cover p
__device__ __forceinline__ float ola_at(const float* fr, int N, int hop, const float* w2, int T, int p) {
    const int t_hi = min(T - 1, p / hop), t_lo = p >= N ? (p - N) / hop + 1 : 0;
    float s = 0.0f, e = 0.0f;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int o = p - t * hop;
        s = __fadd_rn(s, fr[(long long)t * N + o]);
        e = __fadd_rn(e, w2[o]);
    }
    return __fdiv_rn(s, e);
}
// four consecutive positions p .. p + 3 (p % 4 == 0, hop % 4 == 0: they share their frames; N % 4 == 0: 16-byte loads)
__device__ __forceinline__ float4 ola_at4(const float* fr, int N, int hop, const float* w2, int T, int p) {
    const int t_hi = min(T - 1, p / hop), t_lo = p >= N ? (p - N) / hop + 1 : 0;
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f), e = s;
    for (int t = t_lo; t <= t_hi; ++t) {
        const int o = p - t * hop;
        const float4 y = *reinterpret_cast<const float4*>(fr + (long long)t * N + o);
        const float4 w = *reinterpret_cast<const float4*>(w2 + o);
        s.x = __fadd_rn(s.x, y.x); s.y = __fadd_rn(s.y, y.y); s.z = __fadd_rn(s.z, y.z); s.w = __fadd_rn(s.w, y.w);
        e.x = __fadd_rn(e.x, w.x); e.y = __fadd_rn(e.y, w.y); e.z = __fadd_rn(e.z, w.z); e.w = __fadd_rn(e.w, w.w);
    }
    return make_float4(__fdiv_rn(s.x, e.x), __fdiv_rn(s.y, e.y), __fdiv_rn(s.z, e.z), __fdiv_rn(s.w, e.w));
}

// out[r, c] = x_b[reflect(blk_t[r] hop + c - N/2)], x_b = the overlap-add of utterance b = blk_b[r] (rows row0[b] .. + T[b] of frames),
// L_b = (T[b] - 1) hop; an utterance owns T[b] - 1 + N / hop blocks = its whole padded signal
__global__ void istft_ola_blocks_kernel(const float* frames, int N, int hop, const float* w2, const int* blk_b, const int* blk_t,
                                        const int* row0, const int* Tlen, float* out, int Rb) {
    const int c4n = hop >> 2, pad = N >> 1;
    const long long total = (long long)Rb * c4n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int r = (int)(i / c4n), c = (int)(i % c4n) * 4;
        const int b = blk_b[r], T = Tlen[b], L = (T - 1) * hop;
        const float* fr = frames + (long long)row0[b] * N;
        const int n0 = blk_t[r] * hop + c - pad;
        float4 v;
        if ((pad & 3) == 0 && n0 >= 0 && n0 + 3 < L) {
            v = ola_at4(fr, N, hop, w2, T, n0 + pad);
        } else {
            float e[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int n = n0 + k;
                if (n < 0) n = -n;
                else if (n >= L) n = 2 * (L - 1) - n;
                e[k] = ola_at(fr, N, hop, w2, T, n + pad);
            }
            v = make_float4(e[0], e[1], e[2], e[3]);
        }
        *reinterpret_cast<float4*>(out + (long long)r * hop + c) = v;
    }
}

// wav[b, n] = x_b[n] for n < L_b, 0 for L_b <= n < L_max; vec: wav on 16 bytes and L_max % 4 == 0
__global__ void istft_ola_wav_kernel(const float* frames, int N, int hop, const float* w2, const int* row0, const int* Tlen, float* wav,
                                     int L_max, int B, int vec) {
    const int c4n = (L_max + 3) >> 2, pad = N >> 1;
    const long long total = (long long)B * c4n;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const int b = (int)(i / c4n), n0 = (int)(i % c4n) * 4;
        const int T = Tlen[b], L = (T - 1) * hop;
        const float* fr = frames + (long long)row0[b] * N;
        float e[4] = {0.f, 0.f, 0.f, 0.f};
        if ((pad & 3) == 0 && n0 + 3 < L) {
            const float4 v = ola_at4(fr, N, hop, w2, T, n0 + pad);
            e[0] = v.x; e[1] = v.y; e[2] = v.z; e[3] = v.w;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (n0 + k < L) e[k] = ola_at(fr, N, hop, w2, T, n0 + k + pad);
        }
        float* dst = wav + (long long)b * L_max + n0;
        if (vec) *reinterpret_cast<float4*>(dst) = make_float4(e[0], e[1], e[2], e[3]);
        else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (n0 + k < L_max) dst[k] = e[k];
        }
    }
}

// One wave per frame row r, four rows a workgroup.  update: D = R - c Rprev, S = D (A / (|D| + 1e-16)), Rprev = R (read before it is
// written: D is formed from the OLD Rprev).  resid != nullptr: resid[rmap[r]] = sum_f (|R| - A)^2.
__global__ void gl_phase_update_kernel(const float* Rm, float* Rprev, const float* A, int lda, float* S, int lds_, int F, float c,
                                       float* resid, const int* rmap, int rows, int update) {
    const int lane = threadIdx.x & 63, r = blockIdx.x * (kThreads / 64) + (threadIdx.x >> 6);
    if (r >= rows) return;
    const long long base = (long long)r * lds_;
    float acc = 0.0f;
    for (int f = lane; f < F; f += 64) {
        const float rr = Rm[base + f], ri = Rm[base + F + f], a = A[(long long)r * lda + f];
        if (update) {
            const float dr = __fsub_rn(rr, __fmul_rn(c, Rprev[base + f])), di = __fsub_rn(ri, __fmul_rn(c, Rprev[base + F + f]));
            const float mag = sqrtf(__fadd_rn(__fmul_rn(dr, dr), __fmul_rn(di, di)));
            const float g = __fdiv_rn(a, __fadd_rn(mag, 1e-16f));
            S[base + f] = __fmul_rn(dr, g);
            S[base + F + f] = __fmul_rn(di, g);
            Rprev[base + f] = rr;
            Rprev[base + F + f] = ri;
        }
        if (resid) {
            const float d = __fsub_rn(sqrtf(__fadd_rn(__fmul_rn(rr, rr), __fmul_rn(ri, ri))), a);
            acc = __fadd_rn(acc, __fmul_rn(d, d));
        }
    }
    if (resid) {
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) acc = __fadd_rn(acc, __shfl_xor(acc, o));
        if (lane == 0) resid[rmap[r]] = acc;
    }
}

}  // namespace

hipError_t launch_gl_exp_rows(const float* mel, int C, const int* rowmap, float* out, int R, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if ((C & 3) || (reinterpret_cast<uintptr_t>(out) & 15)) return hipErrorInvalidValue;
    const int vec = (reinterpret_cast<uintptr_t>(mel) & 15) == 0;
    hipLaunchKernelGGL(gl_exp_rows_kernel, grid_for((long long)R * (C >> 2)), dim3(kThreads), 0, s, mel, C, rowmap, out, R, vec);
    return hipGetLastError();
}
hipError_t launch_gl_phase_init(const float* A, int lda, const int* row_b, const int* row_t, const uint32_t* seeds, float* S, int lds_,
                                int F, int R, hipStream_t s) {
    if (R <= 0) return hipSuccess;
    if (F < 1 || lds_ < 2 * F || lds_ - 2 * F > F) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gl_phase_init_kernel, grid_for((long long)R * F), dim3(kThreads), 0, s, A, lda, row_b, row_t, seeds, S, lds_, F, R);
    return hipGetLastError();
}
hipError_t launch_istft_ola_blocks(const float* frames, int N, int hop, const float* w2, const int* blk_b, const int* blk_t,
                                   const int* row0, const int* Tlen, float* out, int Rb, hipStream_t s) {
    if (Rb <= 0) return hipSuccess;
    if (hop < 4 || (hop & 3) || N % hop || N / hop < 2 || ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(w2) |
                                                            reinterpret_cast<uintptr_t>(out)) & 15))
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(istft_ola_blocks_kernel, grid_for((long long)Rb * (hop >> 2)), dim3(kThreads), 0, s, frames, N, hop, w2, blk_b,
                       blk_t, row0, Tlen, out, Rb);
    return hipGetLastError();
}
hipError_t launch_istft_ola_wav(const float* frames, int N, int hop, const float* w2, const int* row0, const int* Tlen, float* wav,
                                int L_max, int B, hipStream_t s) {
    if (B <= 0 || L_max <= 0) return hipSuccess;
    if (hop < 4 || (hop & 3) || N % hop || N / hop < 2 || ((reinterpret_cast<uintptr_t>(frames) | reinterpret_cast<uintptr_t>(w2)) & 15))
        return hipErrorInvalidValue;
    const int vec = (reinterpret_cast<uintptr_t>(wav) & 15) == 0 && (L_max & 3) == 0;
    hipLaunchKernelGGL(istft_ola_wav_kernel, grid_for((long long)B * ((L_max + 3) >> 2)), dim3(kThreads), 0, s, frames, N, hop, w2, row0,
                       Tlen, wav, L_max, B, vec);
    return hipGetLastError();
}
hipError_t launch_gl_phase_update(const float* R, float* Rprev, const float* A, int lda, float* S, int lds_, int F, float c, float* resid,
                                  const int* rmap, int rows, int update, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (F < 1 || lds_ < 2 * F || (resid && !rmap) || (update && (!Rprev || !S))) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gl_phase_update_kernel, dim3((rows + kThreads / 64 - 1) / (kThreads / 64)), dim3(kThreads), 0, s, R, Rprev, A, lda,
                       S, lds_, F, c, resid, rmap, rows, update);
    return hipGetLastError();
}

}  // namespace mt2
