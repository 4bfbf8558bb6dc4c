// Dynamic time warping of one mel onto another (gfx950): the warp that carries the phone boundaries of a SYNTHESISED prompt
// (Megatts.align_prompt: the prompt's own phones under its own timbre, durations from the ADM) onto the real prompt mel, in place
// of the Montreal Forced Aligner TextGrids the reference reads during data preparation (prepare_ds.py, utils/textgrid.py; out of
// scope here).  The same primitive is the DTW mel distance between two utterances.  The rule is our own and is
// held to its own restatement (tests/dtw_ref.py).  Per utterance b, X f32 [Tx, D] (synthetic), Y f32 [Ty, D] (real), Tx, Ty, D >= 1:
//
//   cost       c[i, j] = sum_k (x[i, k] - y[j, k])^2 in f32 as ONE chain over k ascending: acc = 0; d = x - y; acc = fmaf(d, d, acc).
//              No split across lanes, no atomics, and the order does not depend on the tile: c depends on the two rows alone, so a
//              ragged batch is bit-identical to its utterances alone.
//   accumulate one f32 add per cell:  A[0, 0] = c[0, 0];  A[i, 0] = c[i, 0] + A[i-1, 0];  A[0, j] = c[0, j] + A[0, j-1];
//              otherwise A[i, j] = c[i, j] + min(A[i-1, j-1], A[i-1, j], A[i, j-1]).
//   direction  diagonal if A[i-1, j-1] <= both others; else up (i-1, j) if A[i-1, j] <= A[i, j-1]; else left (i, j-1).
//              Row 0 is always left, column 0 always up.  Given c, A and the directions are exactly reproducible in numpy float32
//              (min is exact, each cell is one rounding).
//   path       backtracked from (Tx-1, Ty-1) to (0, 0), reported as lo[j] / hi[j], the smallest / largest i on the path in column j.
//              The path is monotone with steps (1,1), (1,0), (0,1), so lo[0] = 0, hi[Ty-1] = Tx-1, lo[j+1] in {hi[j], hi[j] + 1}
//              and lo / hi hold the whole path.  steps = the number of cells on it, total = A[Tx-1, Ty-1].  Entries j >= Ty_b of
//              lo / hi are -1.
//   durations  synthetic durations s[p] >= 0 over Np phones with sum s = Tx, cum[p] = sum_{q<p} s[q]: real frame j belongs to the
//              phone p with cum[p] <= hi[j] < cum[p+1], dur[p] is the number of such j.  hi is non-decreasing, so
//              dur[p] = lower_bound(hi, cum[p+1]) - lower_bound(hi, cum[p]) and sum dur = Ty exactly.  A phone with s[p] = 0, or one
//              swallowed by a vertical run of the path, gets 0.
//   Inputs must be finite.  A non-finite value does not fault and still gives a path inside the matrix - a failed <= falls through
//   to left, row 0 / column 0 are forced - nothing more is promised.
//
// Four kernels.  cost: one grid over (step tiles, strips, b), a workgroup the parallelogram of cells that 64 rows visit in 64 steps
// of the skewed walk below, the X and Y row tiles staged in LDS 16 columns of k at a time; rows at or beyond an utterance's lengths
// are never read.  It writes c SKEWED into scratch, c[64 s + l, t - l] at [s][t][l], so that what a strip's 64 lanes read at step t
// is one contiguous line (read row per lane from a row-major matrix, every load touched 64 lines and the accumulation was bound by
// the CU's cache-line rate: 2.5 ms at 1875 x 1875), and in the caller's row-major layout as well only when `cost` is given.  accumulate: ONE workgroup of 16 waves per utterance, nothing
// waits on another workgroup.  A wave owns a strip of 64 rows, lane l the row 64 s + l, and walks it skewed: at step t the lane is
// in column t - l, its upper neighbours A[i-1, j] and A[i-1, j-1] are the previous lane's last two values (one DPP wave shift per
// step), its left neighbour its own.  A strip's bottom row goes to LDS for the strip below.  The waves run the strips as a pipeline
// in periods of 64 steps with one barrier between periods: strip s starts at period (s / 16) P + 2 (s % 16), P = max(chunks + 2, 32),
// two periods behind the strip above it - what that one has finished by then covers the columns this one reads.  Trip counts are
// closed forms of (Tx, Ty), uniform in the workgroup.  A direction is 2 bits, 16 columns to a u32 word.  backtrack: one wave per
// utterance walks the words; a left step stays inside a word, an up or diagonal step leaves the row, so the wave keeps a tile of
// 32 rows x 2 words in its lanes (one load per tile, the walk reads it by readlane) instead of one dependent load per step.
// durations: one thread per phone, two binary searches in hi.
#include "../../include/megatts2_hip.h"
#include "mt2_kernels.h"

#include <algorithm>

namespace mt2 {

namespace {
constexpr int kTile = 64;                    // cost: cells per side of a workgroup's tile
constexpr int kKc = 16;                      // cost: columns of k staged per pass
constexpr int kCostThreads = 256;
constexpr int kAccWaves = 16;                // accumulate: waves (strips in flight) per workgroup
constexpr int kStrip = 64;                   // accumulate: rows per strip = lanes per wave = steps per period
constexpr int kHalf = 32;                   // accumulate: steps whose costs are loaded at once
constexpr int kRing = 256;                   // accumulate: columns of a strip's bottom row kept for the strip two periods behind
constexpr int kCap = MT2_DTW_MAX_LEN;        // accumulate: the last wave's bottom row waits a whole pass: kept in full
static_assert((kRing & (kRing - 1)) == 0 && (kCap & (kCap - 1)) == 0 && kRing >= 4 * kStrip, "edge buffers are indexed by a mask");
static_assert(kTile == kStrip, "a cost tile is one strip's period");
constexpr int kDiag = 0, kUp = 1, kLeft = 2;
}  // namespace

long long dtw_dir_words(int Ty_max) { return ((long long)Ty_max + MT2_DTW_DIR_COLS - 1) / MT2_DTW_DIR_COLS; }

long long dtw_skew_steps(int Ty_max) { return kStrip * (((long long)Ty_max + 2 * kStrip - 2) / kStrip); }

// c for one parallelogram of 64 rows x 64 steps: rows i0 + l, columns j = t0 + u - l (l, u < 64) - the cells the strip's 64 lanes
// visit in 64 consecutive steps of the accumulation.  Thread (tl, tu) of 16 x 16 owns the cells (l, u) = (tl + 16 r, tu + 16 c),
// each ONE fma chain over k; lanes that differ in tl write 16 consecutive floats of the skewed scratch.  127 rows of Y are staged.
__global__ __launch_bounds__(kCostThreads) void dtw_cost_kernel(DtwP p) {
    __shared__ float xs[kTile][kKc + 1], ys[2 * kTile - 1][kKc + 1];
    const int b = blockIdx.z, Tx = p.x_len[b], Ty = p.y_len[b];
    const int i0 = blockIdx.y * kTile, t0 = blockIdx.x * kTile;
    if (i0 >= Tx || t0 - (kTile - 1) >= Ty) return;                         // workgroup-uniform, before any barrier
    const float* __restrict__ X = p.X + (long long)b * p.Tx_max * p.D;
    const float* __restrict__ Y = p.Y + (long long)b * p.Ty_max * p.D;
    const int tl = threadIdx.x & 15, tu = threadIdx.x >> 4;
    const int jlo = t0 - (kTile - 1);                                       // the column of ys[0]
    float acc[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) acc[r][c] = 0.0f;
    for (int k0 = 0; k0 < p.D; k0 += kKc) {
        const int kn = min(kKc, p.D - k0);
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 2 * kTile * kKc / kCostThreads; ++q) {
            const int e = threadIdx.x + kCostThreads * q, row = e / kKc, k = e % kKc;
            const bool kin = k < kn;
            if (row < kTile) xs[row][k] = kin && i0 + row < Tx ? X[(long long)(i0 + row) * p.D + k0 + k] : 0.0f;
            if (row < 2 * kTile - 1) {
                const int j = jlo + row;
                ys[row][k] = kin && j >= 0 && j < Ty ? Y[(long long)j * p.D + k0 + k] : 0.0f;
            }
        }
        __syncthreads();
        for (int k = 0; k < kn; ++k) {
            float xv[4], yv[7];                                             // y rows (tu - tl) + 16 (c - r) + 63, c - r = -3 .. 3
#pragma unroll
            for (int r = 0; r < 4; ++r) xv[r] = xs[tl + 16 * r][k];
#pragma unroll
            for (int d = 0; d < 7; ++d) yv[d] = ys[tu - tl + 16 * (d - 3) + kTile - 1][k];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int c = 0; c < 4; ++c) {
                    const float d = __fsub_rn(xv[r], yv[c - r + 3]);
                    acc[r][c] = fmaf(d, d, acc[r][c]);
                }
        }
    }
    float* __restrict__ S = p.skew + (((long long)b * p.S_max + blockIdx.y) * p.TS + t0) * kStrip;
    float* __restrict__ C = p.cost ? p.cost + (long long)b * p.Tx_max * p.Ty_max : nullptr;
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            const int l = tl + 16 * r, u = tu + 16 * c, i = i0 + l, j = t0 + u - l;
            if (i < Tx && j >= 0 && j < Ty) {
                S[(long long)u * kStrip + l] = acc[r][c];
                if (C) C[(long long)i * p.Ty_max + j] = acc[r][c];
            }
        }
}

// the value of the lane below in the wave (lane l gets lane l - 1's; lane 0 keeps its own): one DPP move, no LDS
__device__ __forceinline__ float wave_shift_up(float v) {
    return __int_as_float(__builtin_amdgcn_update_dpp(__float_as_int(v), __float_as_int(v), 0x138 /* wave_shr:1 */, 0xf, 0xf, false));
}

__global__ __launch_bounds__(kAccWaves * 64) void dtw_accumulate_kernel(DtwP p) {
    __shared__ float edge[(kAccWaves - 1) * kRing + kCap];
    const int b = blockIdx.x, Tx = p.x_len[b], Ty = p.y_len[b];
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int nstrips = (Tx + kStrip - 1) / kStrip;
    const int nchunks = (Ty + (kStrip - 1) + kStrip - 1) / kStrip;          // a strip takes Ty + 63 steps
    const int P = max(nchunks + 2, 2 * kAccWaves);
    const int periods = ((nstrips - 1) / kAccWaves) * P + 2 * ((nstrips - 1) % kAccWaves) + nchunks;
    float* __restrict__ A = p.acc ? p.acc + (long long)b * p.Tx_max * p.Ty_max : nullptr;
    unsigned* __restrict__ dirs = p.dirs + (long long)b * p.Tx_max * p.DW;
    float* wr = edge + w * kRing;                                           // this wave's bottom rows
    const int wmask = w == kAccWaves - 1 ? kCap - 1 : kRing - 1;
    const int wp = (w + kAccWaves - 1) % kAccWaves;                         // the wave of the strip above
    const float* rd = edge + wp * kRing;
    const int rmask = wp == kAccWaves - 1 ? kCap - 1 : kRing - 1;
    float a_prev = 0.0f, up_old = 0.0f;
    unsigned pack = 0;
    for (int period = 0; period < periods; ++period) {
        const int rel = period - 2 * w;
        const int pass = rel >= 0 ? rel / P : 0, q = rel - pass * P, s = pass * kAccWaves + w;
        if (rel >= 0 && q < nchunks && s < nstrips) {                       // wave-uniform
            const int i = s * kStrip + lane, jbase = kStrip * q - lane;
            const bool row_in = i < Tx;
            const float* __restrict__ sk = p.skew + ((((long long)b * p.S_max + s) * p.TS + kStrip * q) * kStrip) + lane;
            if (q == 0) { a_prev = 0.0f; up_old = 0.0f; pack = 0; }
            for (int h = 0; h < kStrip; h += kHalf) {
                // the costs of half a period go to registers at once (the SIMD's other waves cover the loads), from the skewed
                // scratch: step t of the strip is 64 consecutive floats, one per lane.  A cell outside the matrix reads a word of
                // the scratch that nobody wrote and leaves it unused.  Lane u also fetches the value lane 0 needs from the strip
                // above at step u, A[i0 - 1, 64 q + h + u].
                float cv[kHalf];
#pragma unroll
                for (int u = 0; u < kHalf; ++u) cv[u] = sk[(h + u) * kStrip];
                const int je = kStrip * q + h + lane;
                const float above = s > 0 && lane < kHalf && je < Ty ? rd[je & rmask] : 0.0f;
#pragma unroll
                for (int u = 0; u < kHalf; ++u) {
                    const int j = jbase + h + u;
                    float up_new = wave_shift_up(a_prev);                   // A[i-1, j]: the lane above finished column j last step
                    const float edge_up = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(above), u));
                    if (lane == 0) up_new = edge_up;
                    if (row_in && j >= 0 && j < Ty) {
                        const float diag = up_old, left = a_prev;
                        int code;
                        float from;
                        if (i == 0) { code = kLeft; from = left; }
                        else if (j == 0) { code = kUp; from = up_new; }
                        else if (diag <= up_new && diag <= left) { code = kDiag; from = diag; }
                        else if (up_new <= left) { code = kUp; from = up_new; }
                        else { code = kLeft; from = left; }
                        const float a = i == 0 && j == 0 ? cv[u] : __fadd_rn(cv[u], from);
                        a_prev = a;
                        if (A) A[(long long)i * p.Ty_max + j] = a;
                        if (lane == kStrip - 1) wr[j & wmask] = a;
                        pack |= (unsigned)code << (2 * (j & (MT2_DTW_DIR_COLS - 1)));
                        if ((j & (MT2_DTW_DIR_COLS - 1)) == MT2_DTW_DIR_COLS - 1 || j == Ty - 1) {
                            dirs[(long long)i * p.DW + j / MT2_DTW_DIR_COLS] = pack;
                            pack = 0;
                        }
                        if (i == Tx - 1 && j == Ty - 1) p.total[b] = a;
                    }
                    up_old = up_new;                                        // A[i-1, j] is the next column's diagonal
                }
            }
        }
        __syncthreads();
    }
}

// one wave per utterance: lo / hi = -1 beyond Ty_b, then the walk from (Tx-1, Ty-1) to (0, 0)
__global__ __launch_bounds__(64) void dtw_backtrack_kernel(DtwP p) {
    const int b = blockIdx.x, Tx = p.x_len[b], Ty = p.y_len[b], lane = threadIdx.x;
    int* __restrict__ lo = p.lo + (long long)b * p.Ty_max;
    int* __restrict__ hi = p.hi + (long long)b * p.Ty_max;
    for (int j = Ty + lane; j < p.Ty_max; j += 64) { lo[j] = -1; hi[j] = -1; }
    const unsigned* __restrict__ dirs = p.dirs + (long long)b * p.Tx_max * p.DW;
    int i = Tx - 1, j = Ty - 1, steps = 1;
    int tile_i = -1, tile_w = -1;                        // the tile holds rows (tile_i - 32, tile_i], words (tile_w - 2, tile_w]
    unsigned held = 0;
    if (lane == 0) hi[j] = i;
    while (i > 0 || j > 0) {                             // i and j are the same in every lane
        const int wd = j / MT2_DTW_DIR_COLS;
        if (tile_i < 0 || i <= tile_i - 32 || wd <= tile_w - 2) {
            tile_i = i; tile_w = wd;
            const int r = i - (lane & 31), c = wd - (lane >> 5);
            held = r >= 0 && c >= 0 ? dirs[(long long)r * p.DW + c] : 0u;
        }
        const int src = __builtin_amdgcn_readfirstlane((tile_i - i) + 32 * (tile_w - wd));
        const unsigned word = (unsigned)__builtin_amdgcn_readlane((int)held, src);
        int code = (int)(word >> (2 * (j & (MT2_DTW_DIR_COLS - 1)))) & 3;
        if (i == 0) code = kLeft;                        // whatever the word says, the walk stays inside the matrix
        else if (j == 0) code = kUp;
        if (code == kDiag) { if (lane == 0) lo[j] = i; --i; --j; if (lane == 0) hi[j] = i; }
        else if (code == kUp) { --i; }
        else { if (lane == 0) lo[j] = i; --j; if (lane == 0) hi[j] = i; }
        ++steps;
    }
    if (lane == 0) { lo[0] = 0; p.steps[b] = steps; }
}

// dur[b, p] = lower_bound(hi_b, cum[p+1]) - lower_bound(hi_b, cum[p]) over hi_b[0 .. Ty_b); last[b] = hi_b[Ty_b - 1]
__device__ __forceinline__ int dtw_lower_bound(const int* __restrict__ hi, int n, int v) {
    int a = 0, z = n;
    while (a < z) {
        const int m = (a + z) >> 1;
        if (hi[m] < v) a = m + 1; else z = m;
    }
    return a;
}

__global__ __launch_bounds__(256) void dtw_durations_kernel(AlignDurP p) {
    const int b = blockIdx.y, ph = blockIdx.x * 256 + threadIdx.x, Ty = p.y_len[b];
    const int* __restrict__ hi = p.hi + (long long)b * p.Ty_max;
    if (ph == 0) p.last[b] = hi[Ty - 1];
    if (ph >= p.Np_max) return;
    int d = 0;
    if (ph < p.np_len[b]) {
        const int* __restrict__ cum = p.cum + (long long)b * (p.Np_max + 1);
        d = dtw_lower_bound(hi, Ty, cum[ph + 1]) - dtw_lower_bound(hi, Ty, cum[ph]);
    }
    p.dur[(long long)b * p.Np_max + ph] = d;
}

static bool dtw_args_ok(const DtwP& p) {
    return p.B >= 1 && p.B <= 65535 && p.D >= 1 && p.max_tx >= 1 && p.max_tx <= p.Tx_max && p.max_ty >= 1 && p.max_ty <= p.Ty_max &&
           p.Tx_max <= kCap && p.Ty_max <= kCap && p.DW >= dtw_dir_words(p.max_ty) && p.X && p.Y && p.skew &&
           p.S_max >= (p.max_tx + kStrip - 1) / kStrip && p.TS >= dtw_skew_steps(p.max_ty) && p.dirs && p.lo && p.hi &&
           p.steps && p.total && p.x_len && p.y_len;
}

hipError_t launch_dtw_cost(const DtwP& p, hipStream_t s) {
    if (!dtw_args_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dtw_cost_kernel, dim3((int)(dtw_skew_steps(p.max_ty) / kTile), (p.max_tx + kTile - 1) / kTile, p.B), dim3(kCostThreads), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_dtw_accumulate(const DtwP& p, hipStream_t s) {
    if (!dtw_args_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dtw_accumulate_kernel, dim3(p.B), dim3(kAccWaves * 64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_dtw_backtrack(const DtwP& p, hipStream_t s) {
    if (!dtw_args_ok(p)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(dtw_backtrack_kernel, dim3(p.B), dim3(64), 0, s, p);
    return hipGetLastError();
}

hipError_t launch_dtw_durations(const AlignDurP& p, hipStream_t s) {
    if (p.B < 1 || p.B > 65535 || p.Np_max < 1 || p.Ty_max < 1 || !p.hi || !p.y_len || !p.cum || !p.np_len || !p.dur || !p.last)
        return hipErrorInvalidValue;
    hipLaunchKernelGGL(dtw_durations_kernel, dim3((p.Np_max + 255) / 256, p.B), dim3(256), 0, s, p);
    return hipGetLastError();
}

}  // namespace mt2
