// Formant tracks across frames: a Viterbi pass over the per-frame candidates of mt2_lpc_formants, in the manner of Praat's "Formant:
// Track" (Xia & Espy-Wilson 2000) with a rule of our own (gfx950).  The reference tree has no formant tracker; parity with Praat is
// unpinned - include/megatts2_hip.h has the rule in full, tests/formant_track_ref.py restates it in numpy.  In short, for K tracks:
//
//   states   the C(5, K) increasing K-tuples of candidate slots in lexicographic order; state s puts candidate st[s][q] on track q
//   gap      a frame with fewer than K candidates, or a non-finite / non-positive freq or non-finite / negative bw among its first n
//   o[t, s]  = sum_q (freq_cost (|f - ref_q| / 1000)) + (bw_cost (b / f))          +inf where st[s][K - 1] >= n
//   tr(j, k) = jump_cost sum_q (2 |f' - f|) / (f' + f)                             between two non-gap frames
//   delta[t, k] = o[t, k] + min_j (delta[t - 1, j] + tr(j, k)), psi = the smallest such j;  a gap frame has delta = 0, and the frame
//   behind a gap (and frame 0) starts from o alone.  All in double, every operation rounded on its own (fp contract off in this file).
//
// formant_track_kernel: ONE wave per utterance.  The frames are taken in tiles of 64:
//   load    the tile's candidate rows (and the row in front of it) go to LDS by coalesced loads; lane r then decides frame r's gap flag
//   table   lane r computes the 25 u(a, c) = (2 |f'_c - f_a|) / (f'_c + f_a) between frame r - 1 and frame r - the ONLY divisions of the
//           transition, 25 a frame rather than K a state pair -, the local terms of its candidates on every track (25 divisions more,
//           not 2 K a state) and from them o[r, .];  then lane p builds tr(j, k) of its state pairs p, p + 64
//           for every frame of the tile from u, K LDS reads and adds each, into tr[64][100] (50 KiB)
//   walk    the recurrence, off which everything above has been taken: state k's six lanes (k, i) hold the predecessors j = i and i + 6;
//           a step is one fetch of delta[j] from lane 6 j, one add of the tabulated tr, a min of two, three guarded shuffle-down mins and
//           one add of o - psi (the smallest j attaining the minimum, by ballot) hangs off the side of that chain.  A gap frame is the
//           same step with tr = 0, which gives its psi, and then delta = 0; the frame behind a gap (and frame 0) is the same step too:
//           min_j (0 + 0) = 0 at j = 0, so delta = o + 0 = o to the bit and psi = 0.
//   psi     16 bytes a frame to the arena: byte k is state k's predecessor, bytes 10 .. 15 zero, one 16-byte store per lane
// Backtrack as f0_viterbi_kernel's: psi comes back a tile at a time into LDS, lane 0 walks it (no chain of dependent global loads), then
// lane r gathers frame r's outputs.  No atomics, no scratch; LDS 84 KiB (dynamic).  Nothing depends on the batch slot or T_max.
#include "../../include/megatts2_hip.h"
#include "mt2_kernels.h"

#include <math.h>

#include <algorithm>

#pragma clang fp contract(off)

namespace mt2 {

namespace {
constexpr int kTile = 64, kS = MT2_FORMANT_TRACK_STATES, kC = MT2_FORMANT_MAX, kG = 6, kPsi = 16;
static_assert(kS == 10 && kC == 5 && kS * kG <= 64 && 2 * kG >= kS && kS <= kPsi, "ten states of six lanes in one wave, two predecessors a lane");

struct FtLds {
    double tr[kTile * kS * kS];       // tr[r][k S + j]: frame r - 1 in state j -> frame r in state k (0 at a gap, behind one, at frame 0)
    double u[kTile * kC * kC];        // u[r][5 a + c]: candidate a of frame r - 1 -> candidate c of frame r
    double tm[kTile * kC * kC];       // tm[r][5 q + c]: the local term of candidate c of frame r on track q
    double o[kTile * kS];             // o[r][k]
    float f[(kTile + 1) * kC + 3];    // row i: frame t0 - 1 + i
    float b[(kTile + 1) * kC + 3];
    int n[kTile + 1 + 3];             // min(count, 5) of row i; -1 for a gap or a frame outside [0, T)
    __attribute__((aligned(16))) unsigned char psi[kTile * kPsi];
    int ks[kTile];
    signed char st[kS * kC];
};

// rows 0 .. 64 of the tile at t0 (frames t0 - 1 .. t0 + 63) into LDS, and their gap flags; ends behind a barrier
__device__ __forceinline__ void ft_load(FtLds& l, const float* __restrict__ fq, const float* __restrict__ bq, const int* __restrict__ cq, int t0,
                                        int T, int K, int lane) {
    const long long g0 = (long long)(t0 - 1) * kC, gT = (long long)T * kC;
    for (int i = lane; i < (kTile + 1) * kC; i += 64) {
        const long long g = g0 + i;
        const bool in = g >= 0 && g < gT;
        l.f[i] = in ? fq[g] : 0.0f;
        l.b[i] = in ? bq[g] : 0.0f;
    }
    __syncthreads();
    for (int i = lane; i < kTile + 1; i += 64) {
        const int t = t0 - 1 + i;
        int n = -1;
        if (t >= 0 && t < T) {
            n = min(cq[t], kC);
            bool gap = n < K;
#pragma unroll
            for (int c = 0; c < kC; ++c) {
                const float f = l.f[i * kC + c], w = l.b[i * kC + c];
                if (c < n && !(isfinite(f) && f > 0.0f && isfinite(w) && w >= 0.0f)) gap = true;
            }
            if (gap) n = -1;
        }
        l.n[i] = n;
    }
    __syncthreads();
}

__global__ __launch_bounds__(64) void formant_track_kernel(FormantTrackP p) {
    extern __shared__ __attribute__((aligned(16))) char ft_lds[];
    FtLds& l = *reinterpret_cast<FtLds*>(ft_lds);
    const int b = blockIdx.x, lane = threadIdx.x;
    const int T = p.len[b], K = p.K, S = p.S, T_max = p.T_max;
    const float* __restrict__ fq = p.freq + (long long)b * T_max * kC;
    const float* __restrict__ bq = p.bw + (long long)b * T_max * kC;
    const int* __restrict__ cq = p.count + (long long)b * T_max;
    unsigned char* psi = p.psi + (long long)b * T_max * kPsi;
    const double inf = INFINITY;

    if (lane < kS * kC) l.st[lane] = p.st[lane];              // the state table (formant_track_table), zeros behind S and K
    __syncthreads();

    // ---- forward
    const int k = lane / kG, i6 = lane - k * kG;
    const bool act = k < S;
    const int ja = i6, jb = i6 + kG;
    const bool has_a = act && ja < S, has_b = act && jb < S;
    const int top = act ? l.st[k * kC + K - 1] : 0;            // state k is valid in a frame with n candidates iff top < n
    const int src_a = has_a ? ja * kG : 0, src_b = has_b ? jb * kG : 0, src_k = act ? k * kG : 0;
    const int tr_a = has_a ? k * S + ja : 0, tr_b = has_b ? k * S + jb : 0;
    // the table phase: this lane's two state pairs, as the u cells they sum
    int cell[2][kC];
    bool pair[2];
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int pp = lane + 64 * h;
        pair[h] = pp < S * S;
        const int kk = pair[h] ? pp / S : 0, jj = pair[h] ? pp - kk * S : 0;
#pragma unroll
        for (int q = 0; q < kC; ++q) cell[h][q] = l.st[jj * kC + q] * kC + l.st[kk * kC + q];
    }
    double delta = 0.0;                                        // "the frame before frame 0" is a gap
    for (int t0 = 0; t0 < T; t0 += kTile) {
        const int rows = min(kTile, T - t0);
        ft_load(l, fq, bq, cq, t0, T, K, lane);
        reinterpret_cast<uint4*>(l.psi)[lane] = make_uint4(0, 0, 0, 0);
        if (lane < rows) {
            const int r = lane, nt = l.n[r + 1];
            const bool link = nt >= 0 && l.n[r] >= 0;
#pragma unroll
            for (int a = 0; a < kC; ++a) {
                const double f = (double)l.f[r * kC + a];
#pragma unroll
                for (int c = 0; c < kC; ++c) {
                    const double g = (double)l.f[(r + 1) * kC + c];
                    l.u[r * (kC * kC) + a * kC + c] = link ? (2.0 * fabs(g - f)) / (g + f) : 0.0;
                }
            }
            // the local term of candidate c on track q, 25 a frame (a candidate behind n gives whatever: only invalid states read it) ...
            double* __restrict__ tm = l.tm + r * (kC * kC);
#pragma unroll
            for (int c = 0; c < kC; ++c) {
                const double f = (double)l.f[(r + 1) * kC + c], wf = p.bc * ((double)l.b[(r + 1) * kC + c] / f);
#pragma unroll
                for (int q = 0; q < kC; ++q)
                    if (q < K) tm[q * kC + c] = (p.fc * (fabs(f - p.ref[q]) / 1000.0)) + wf;
            }
            // ... and o[r, s], their sum over the state's tracks, q ascending
            for (int s = 0; s < S; ++s) {
                double acc = 0.0;
                if (nt >= 0) {
#pragma unroll
                    for (int q = 0; q < kC; ++q)
                        if (q < K) acc = acc + tm[q * kC + l.st[s * kC + q]];
                    if (l.st[s * kC + K - 1] >= nt) acc = inf;
                }
                l.o[r * kS + s] = acc;
            }
        }
        __syncthreads();
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            if (pair[h]) {
                for (int r = 0; r < rows; ++r) {
                    const double* __restrict__ ur = l.u + r * (kC * kC);
                    double acc = 0.0;
#pragma unroll
                    for (int q = 0; q < kC; ++q)
                        if (q < K) acc = acc + ur[cell[h][q]];
                    l.tr[r * (kS * kS) + lane + 64 * h] = p.jc * acc;
                }
            }
        }
        __syncthreads();
        // ---- the walk: the serial chain carries one fetch, one add, four mins, one add
        for (int r = 0; r < rows; ++r) {
            const double da = __shfl(delta, src_a), db = __shfl(delta, src_b);
            const double* __restrict__ trr = l.tr + r * (kS * kS);
            const double va = has_a ? da + trr[tr_a] : inf, vb = has_b ? db + trr[tr_b] : inf;
            double m = fmin(va, vb);                             // a NaN (an invalid j: delta = +inf, tr whatever) never wins
            double x = __shfl_down(m, 4);
            if (i6 < 2) m = fmin(m, x);
            x = __shfl_down(m, 2);
            if (i6 < 2) m = fmin(m, x);
            x = __shfl_down(m, 1);
            if (i6 < 1) m = fmin(m, x);
            const int nt = l.n[r + 1];
            const bool valid = act && (nt < 0 || top < nt);
            // right on lane 6 k, which is where it is fetched from; a gap frame forgets what came before it: 0, not the minimum
            delta = !valid ? inf : nt < 0 ? 0.0 : l.o[r * kS + (act ? k : 0)] + m;
            // psi, off the chain: the smallest j whose sum is the minimum
            const double mk = __shfl(m, src_k);
            const unsigned long long ea = __ballot(has_a && va == mk), eb = __ballot(has_b && vb == mk);
            const unsigned ga = (unsigned)(ea >> (src_k)) & 63u, gb = (unsigned)(eb >> (src_k)) & 63u;
            int arg = 0;
            if (valid && mk < inf) arg = ga ? __builtin_ctz(ga) : (gb ? __builtin_ctz(gb) + kG : 0);
            if (act && i6 == 0) l.psi[r * kPsi + k] = (unsigned char)arg;
        }
        __syncthreads();
        if (lane < rows) reinterpret_cast<uint4*>(psi)[t0 + lane] = reinterpret_cast<const uint4*>(l.psi)[lane];
        __syncthreads();
    }
    // the end of the path: the smallest k that attains the minimum
    int kcur = 0;
    {
        const bool own = act && i6 == 0;
        const double v = own ? delta : inf;
        double m = v;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) m = fmin(m, __shfl_xor(m, o));
        const unsigned long long e = __ballot(own && v == m);
        kcur = e ? __builtin_ctzll(e) / kG : 0;
    }
    __syncthreads();                                           // every psi row of this workgroup is visible to it

    // ---- backtrack and outputs
    float* __restrict__ of = p.tfreq + (long long)b * T_max * kC;
    float* __restrict__ ob = p.tbw + (long long)b * T_max * kC;
    int* __restrict__ oc = p.tcount + (long long)b * T_max;
    int* __restrict__ os = p.sel ? p.sel + (long long)b * T_max * kC : nullptr;
    for (int t0 = (T - 1) / kTile * kTile; t0 >= 0; t0 -= kTile) {
        const int rows = min(kTile, T - t0);
        ft_load(l, fq, bq, cq, t0, T, K, lane);
        if (lane < rows) reinterpret_cast<uint4*>(l.psi)[lane] = reinterpret_cast<const uint4*>(psi)[t0 + lane];
        __syncthreads();
        if (lane == 0) {
            int kk = kcur;
            for (int r = rows - 1; r >= 0; --r) {
                l.ks[r] = kk;
                kk = min((int)l.psi[r * kPsi + kk], S - 1);     // k*[t - 1] = psi[t, k*[t]]
            }
            kcur = kk;
        }
        kcur = __shfl(kcur, 0);
        __syncthreads();
        if (lane < rows) {
            const int r = lane, nt = l.n[r + 1], s = l.ks[r];
            const long long t = t0 + r;
#pragma unroll
            for (int q = 0; q < kC; ++q) {
                const bool on = nt >= 0 && q < K;
                const int c = on ? l.st[s * kC + q] : 0;
                of[t * kC + q] = on ? l.f[(r + 1) * kC + c] : 0.0f;
                ob[t * kC + q] = on ? l.b[(r + 1) * kC + c] : 0.0f;
                if (os) os[t * kC + q] = on ? c : -1;
            }
            oc[t] = nt >= 0 ? K : 0;
        }
        __syncthreads();                                       // the tile's LDS is reused by the next one
    }
    // the frames in [T, T_max)
    for (long long i = (long long)T * kC + lane; i < (long long)T_max * kC; i += 64) {
        of[i] = 0.0f;
        ob[i] = 0.0f;
        if (os) os[i] = -1;
    }
    for (int t = T + lane; t < T_max; t += 64) oc[t] = 0;
}

}  // namespace

int formant_track_states(int K) {
    int n = 1;
    for (int q = 0; q < K; ++q) n = n * (MT2_FORMANT_MAX - q) / (q + 1);
    return n;
}

// host only: the increasing K-tuples of {0 .. 4} in lexicographic order, st[s][q] at st[5 s + q]; zeros behind
void formant_track_table(int K, signed char* st) {
    std::fill(st, st + kS * kC, (signed char)0);
    int c[kC];
    for (int q = 0; q < kC; ++q) c[q] = q;
    for (int s = 0;; ++s) {
        for (int q = 0; q < K; ++q) st[s * kC + q] = (signed char)c[q];
        // the next tuple: the last position that can still rise does, and those behind it follow on
        int i = K - 1;
        while (i >= 0 && c[i] == kC - K + i) --i;
        if (i < 0) break;
        ++c[i];
        for (int q = i + 1; q < K; ++q) c[q] = c[q - 1] + 1;
    }
}

hipError_t launch_formant_track(const FormantTrackP& p, hipStream_t s) {
    static std::atomic<unsigned long long> done{0};
    if (p.B <= 0) return hipSuccess;
    if (p.B > 65535 || p.T_max < 1 || p.K < 1 || p.K > kC || p.S != formant_track_states(p.K) || p.freq == nullptr || p.bw == nullptr ||
        p.count == nullptr || p.len == nullptr || p.psi == nullptr || p.tfreq == nullptr || p.tbw == nullptr || p.tcount == nullptr ||
        ((uintptr_t)p.psi & 15) != 0)
        return hipErrorInvalidValue;
    const hipError_t e = dyn_lds_once(done, reinterpret_cast<const void*>(formant_track_kernel), sizeof(FtLds));
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(formant_track_kernel, dim3(p.B), dim3(64), sizeof(FtLds), s, p);
    return hipGetLastError();
}

}  // namespace mt2
