// Internal kernel-launcher interface of libmegatts2_hip (gfx950 only).
//
// Every activation lives in HBM as a time-major row matrix [rows, channels] (f32, channels
// contiguous).  A batch of utterances is a *row set*: utterance b owns rows [off_b, off_b+len_b),
// separated from its neighbours by >= G all-zero "gap" rows.  Conv taps that reach over an
// utterance edge therefore read zeros - exactly the per-utterance zero padding the reference's
// batch-1 convolutions see - and every kernel re-zeroes gap rows in its epilogue
// through the `valid` row mask.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <vector>

namespace mt2 {

// hipFuncAttributeMaxDynamicSharedMemorySize is a PER-DEVICE attribute of a kernel: a launcher that needs more than the
// default dynamic LDS sets it once per (kernel, device).  `done` is the launcher's own bit mask of devices already served
// (device ordinal mod 64; a race between two host threads only repeats the idempotent call).
inline hipError_t dyn_lds_once(std::atomic<unsigned long long>& done, const void* fn, size_t bytes) {
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    const unsigned long long bit = 1ull << (dev & 63);
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    e = hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
    done.fetch_or(bit, std::memory_order_release);
    return hipSuccess;
}

constexpr int kInvalidRow = -(1 << 30);   // rowbase sentinel: "this A row is all zeros"

enum Act : int { ACT_NONE = 0, ACT_RELU = 1, ACT_LRELU = 2, ACT_TANH = 3,
                 ACT_LOGCLAMP = 4 };   // epilogue only: log(max(v, pro_slope))  (dynamic range compression)

// C[g][m, n] = epi( sum_{tap, c} pro(X[g][src(m) + tap*dil, c]) * W[g][n, tap*Cin + c] )
//   src(m)  = rowbase ? rowbase[m] : m * a_mul + shift0           (rows outside [0, Rx) read as 0)
//   epi(v)  = mask_m * ( act(v + bias[n]) * out_scale + R[g][m, n] )
// Linear layers: taps = 1.  Conv1d(k, dilation d, "same" padding): taps = k, shift0 = -(k-1)/2*d.
// Strided conv / gathers: rowbase.  Groups (blockIdx.z) batch independent problems of one shape
// (the parallel branches of ConvNetDouble) - a stride of 0 shares the operand between groups.
struct GemmP {
    const float* X; long long strideX; int ldx; int Rx;
    const int* rowbase; int a_mul; int shift0; int taps; int dil; int Cin;
    const float* W; long long strideW; int ldw;
    unsigned long long* dbg = nullptr;   // MT2_PHASE_TIMING builds only: per-phase cycle sums of one wave (tools/x6_phase_timing.py)
    int epi_t4 = 1;             // 16-byte-store epilogue where the layout allows it (always on: launch_gemm sets it)
    int sk_nw = 8;              // gemm_skinny_tm_kernel: waves per workgroup that split K (8; 16 = option skinny_nw, set by launch_gemm)
    int a_planes = 0;           // 1: X holds fp16 planes ([32 hi | 32 lo] per 32 k of a row, x3h_planes.h's block layout without a row scale)
                                // written by a producer kernel (LnP::out_planes): x3h loader / K-split tiles only, no prologue, Cin % 32 = 0
    int c_planes = 0;           // 1: C RECEIVES fp16 planes (the same block layout: the A operand of the next launch's a_planes) instead of f32 -
                                // x3h loader tile only (16-byte-store epilogue), N % 32 = ldc % 32 = 0, C on 128 bytes, no residual, groups = 1
    int ldr64 = 0;              // x3h loaders: 1 = the 64-bit global_load_lds form even where buffer loads would do (EngineOpts::ldr64)
    int ldr_prio = 0;           // s_setprio of the loader waves of the loader-wave kernels (set by launch_gemm from EngineOpts::ldr_prio)
    const void* W3 = nullptr;   // optional: the same weights as three bf16 planes (truncation split, exact sum), addressed like
    long long w3_plane = 0;     // W (same ldw / strideW, in bf16 elements), planes w3_plane elements apart (0: N * ldw) -
                                // lets launch_gemm run on the bf16 matrix pipe in the f32-equivalent 6-product form
    const void* Wh = nullptr;   // optional: the same weights as two fp16 planes (hi, lo * 2^11) of the ROW-SCALED matrix, chunk-interleaved
    long long wh_ldb = 0;       // (x3h_planes.h: row n = blocks of 128 B, block c = [hi | lo] of k = 32 c ..): Wh points at the block of
    long long wh_gstride = 0;   // W's first element, wh_ldb = BYTES between rows (0: 4 * ceil32(ldw)), wh_gstride = bytes between groups;
    const float* wh_inv = nullptr;   // wh_inv[n] = the inverse (an exact power of two) of the scale of weight row n, n = 0 being W's first
    long long wh_inv_stride = 0;     // row; group g: + g * wh_inv_stride.  Lets launch_gemm run on the fp16 matrix pipe in the f32-equivalent
                                     // 3-product form (gemm_x3h.hip)
    int* x3h_flag = nullptr;    // device word: |= 1 when an x3h launch converted an activation with |a| >= 65504 (fp16 range; set by launch_gemm
                                // from EngineOpts::x3h_flag - the caller repeats the call without x3h)
    const float* Wtm = nullptr; // optional: the WHOLE matrix W points into, as tile-major blocks of 16 columns x 64 k (gemm_skinny.hip;
    int tm_n0 = 0, tm_k0 = 0;   // model_load.hip TmRange); (tm_n0, tm_k0) = block coordinates of W's first element (row / 16, column /
    int tm_kb = 0;              // 64), tm_kb = column blocks per block row (ldw / 64).  Lets launch_gemm stream the weights of a
                                // launch with <= 64 rows in 1-KiB pieces
    const float* bias; long long strideB;
    const float* R; long long strideR; int ldr;
    const int* valid;
    float* C; long long strideC; int ldc;
    int M, N, K, groups;
    int pro_act; float pro_slope; int epi_act; float out_scale;   // pro_slope doubles as the epilogue parameter (ACT_LOGCLAMP)
    // pro_act == 3 (LayerNorm prologue, linear layers with K <= 1024 only): A rows are normalised on the fly,
    // C = LN(X; ln_g, ln_b, ln_eps) W^T ...  launch_gemm returns hipErrorNotSupported when the tile configuration
    // it would choose has no such variant (big tiles) - callers then run launch_layernorm + a plain GEMM.
    // pro_act == 4 (ALGEBRAIC LayerNorm, K <= 1024): W = gamma-scaled weights W', bias = c, ln_g = s (see EncLayerW):
    // C = rstd * (X W'^T - mean * s) + c = LN(X) W^T + b; statistics in the prologue, K loop untouched.
    const float* ln_g; const float* ln_b; float ln_eps;
    // ---- LayerNorm statistics handed from GEMM to GEMM (round 5: the AR layers' stand-alone LayerNorm launches).
    // Producer side (any pro_act; groups == 1): stat_out != nullptr asks the epilogue to also write, per output row m and
    // per wave tile of `stat_w` columns, the pair (mean_t, M2_t) of the FINAL values C[m, tile] (after bias, activation,
    // residual and mask) as stat_out[(m * stat_nt + t) * 2 + {0, 1}], stat_nt = N / stat_w.  launch_gemm fills stat_nt /
    // stat_w for the tile it chooses (x6 K-split tiles: 32 columns; 128x128 loader tile: 64) and reports them in
    // EngineOpts::last_stat_nt / last_stat_w - 0 when that tile has no such epilogue (the launch itself still succeeds).
    float* stat_out = nullptr; int stat_nt = 0, stat_w = 0;
    // Consumer side, pro_act == 5 (ALGEBRAIC LayerNorm on PAIR statistics): like pro_act == 4 (W = W', bias = c, ln_g = s), but
    // mean / rstd of source row r come from merging the ln_nt pairs ln_stat[(r * ln_nt + t) * 2 ...] of ln_w columns each
    // (Chan's formula, fixed order) - no pass over K.  x6 tiles 55 / 84 / 85 / 86 only; hipErrorNotSupported otherwise.
    const float* ln_stat = nullptr; int ln_nt = 0, ln_w = 0;
};
// Tuning / measurement switches of the engine.  They live in the model handle (mt2_model::opts) or in a local
// object of a kernel-level entry point - never in process globals: two handles (or two threads) do not see each
// other's settings.  The defaults are what the product path runs.
struct TraceRec { int cfg; double flops; hipEvent_t e0, e1; int M, N, K, groups; };
struct EngineOpts {
    int force_cfg = -1;                                    // >= 0: tile configuration index for every GEMM launch
    int t_ks4 = 256, t_ks2 = 640, t32 = 64, t32x32 = 160;  // tile-choice thresholds in tiles (tools/gemm_sweep.py; t32 / t32x32 re-swept in the model after
                                                           // the x3h K-split tiles changed their ranking: the 64x64 k2 tile takes over from the 32x64 k4 and
                                                           // 32x32 k8 tiles earlier - C2 -2.5 ... -3 %, C3 -0.5 %, profiles/r06_opts_ab_block5_ks_thresholds.txt)
    bool splitk = true;          // split-K through the LayerNorm in the AR layers
    int voc_streams = 3;         // resblock chains of a vocoder stage in flight (1 = serial)
    bool win_conv = true;        // window-convolution kernel for narrow square convs (Cin = Cout in {32, 64, 128})
    bool x6_conv = true;         // ... on the bf16 matrix pipe, f32-equivalent 3-way split (6 products), where W3 planes exist
    bool x6_gemm = true;         // the implicit GEMMs likewise (loader-wave and K-split tiles)
    int x3h = 15;                // f32-equivalent THREE-product form on the fp16 pipe (gemm_x3h.hip) wherever an x6 tile has one and the
                                 // weights come with fp16 planes (GemmP::Wh); bits: 1 the 128x128 loader tile, 2 the K-split tiles of the
                                 // AR steps, 4 the window convolutions, 8 the long-sequence attention kernel (AttnP::x3h: C5 -3.3 %,
                                 // profiles/r06_opts_ab_block6_attention_x3h.txt); 0: everything stays x6
    int pair_fuse = 3;           // the vocoder's resblock conv pairs as ONE launch (PairP, conv_pair_x3h_kernel): bit 0 the 32-channel stage,
                                 // bit 1 the 64-channel stage, bit 2 the 128-channel stage (profiles/conv_pair_fusion_ab.txt)
    int up_fuse = 3;             // the vocoder's MRF mean + the next stage's stride-2 upsampler as ONE launch (UpMrfP, up_mrf_x3h_kernel): bit 0 the
                                 // 64-channel boundary (64 -> 32), bit 1 the 128-channel one (128 -> 64) (profiles/up_mrf_fusion_ab.txt)
    int* x3h_flag = nullptr;     // device word of the range guard (GemmP::x3h_flag); the model handle owns one
    int t_x3h_128 = 72;          // x3h: from this many 128x128 tiles on the loader tile instead of the K-split tiles (t_x6_128's role)
    int t_x6_256 = 160, t_x6_128 = 72;   // ... from this many 256x128 / 128x128 tiles on (profiles/r02_gemm_sweep_x6.txt)
    int x6_ks = 4;               // x6 arithmetic + eight loader waves for the AR steps' K-split tiles (gemm_x6_ks_kernel): 0 off;
                                 // 1, 3: the 32x64 k4 and 64x64 k2/k4 tiles (84, 85); 2, 4: + the 32x32 k8 tile (86); 5: the
                                 // 64x64 tile only.  Default 4: isolated launches +10..50 %
                                 // (profiles/r03_gemm_sweep_x6k.txt), C3 step -1.6 % (profiles/r03_ab_interleaved_v1.txt)
    int a_planes = 3;            // producers of fp16 planes for x3h GEMMs that take their A operand as planes (GemmP::a_planes; wherever
                                 // gemm_takes_planes() says so).  Bit 0: LayerNorm -> Linear pairs of the AR layers and LayerNorm -> Conv1d inside
                                 // the conv stacks (LnP::out_planes); bit 1: ff.0's epilogue stores relu(..) as planes for ff.3 (GemmP::c_planes);
                                 // bit 2: the attention kernels store their output as planes for the out-projection (AttnP::o_planes) -
                                 // bit-identical, measured neutral, off by default (profiles/r06_opts_ab_block4_planes_producers.txt)
    int ks_epi4 = 1;             // x3h K-split tiles: finish the tile row-major with 16-byte residual loads and stores where gemm_route finds the
                                 // layout fit (GemmRoute::ks_epi4); 0: the dword finish everywhere.  Bit-identical (profiles/ks_epilogue_ab.txt)
    bool ldr64 = false;          // tests / measurement: the x3h loaders' 64-bit global_load_lds form (what operands of 2 GiB or more get)
    int ldr_prio = 3;            // issue priority (s_setprio 0..3) of the loader waves (gemm_x6_ldr / gemm_x6_ks / conv_win_x6 kernels)
    int skinny_rows = 64;        // linear layers with at most this many rows (<= 64) run on the weight-streaming kernel of
    int attn_lds_min = 640;      // attention: from this many queries per sequence on the LDS-tiled kernel (AttnP::lds_min_qlen; 0 never)
    int attn_x6_min = 192;       // attention on the bf16 pipe (f32-equivalent, AttnP::x6_min_qlen) from this many queries on; 0: never
                                 // (C5 step 5525 -> 5314 ms at 192, 5376 at 448: profiles/r03_opts_ab.txt)
    bool skinny_tm = true;       // ... on the tile-major weight copy where one exists (gemm_skinny_tm_kernel; LayerNorm prologue included)
    int skinny_pairs = 1;        // launches of at most skinny_rows rows: the residual GEMM's epilogue leaves (mean, M2) pairs per 16-column block
                                 // and the LayerNorm prologue of the consuming launch merges them instead of re-reading all M x K rows
    int skinny_nw = 16;          // waves of the tile-major weight-streaming kernel that split K (8; 16: four per SIMD - twelve for K = 768 -
                                 // at M <= 32: C1 -1.8 %, profiles/r05_opts_ab.txt)
    bool markers = false;        // a named no-op kernel at every stage boundary: lets tools/pmc_stage_summary.py attribute
                                 // the rocprofv3 --pmc rows of one step to stages (measurement only)
    bool trace_on = false;       // HIP events around every GEMM launch (measurement only)
    std::vector<TraceRec> trace;
    const char* last_cfg = "";   // name of the tile configuration the last launch used
    int last_stat_nt = 0, last_stat_w = 0;   // GemmP::stat_out of the last launch: pairs per row / columns per pair (0: none written)
    int last_ks_epi4 = 0;        // GemmRoute::ks_epi4 of the last launch
    int last_sk_nw = 0;          // waves that split K in the last launch, if it ran on the tile-major weight-streaming kernel (else 0)
    int ln_pairs = 0;            // (the value in force for the stage that is running: ln_pairs_adm inside the ADM, 0 elsewhere)
    int ln_pairs_adm = 2;        // ADM layers with more than skinny_rows rows: the residual GEMMs (out-projection, ff.3) write row statistics
                                 // as (mean, M2) pairs per wave tile in their epilogue and LN1 -> QKV / LN2 -> ff.0 run as ONE pair-fed
                                 // algebraic-LayerNorm GEMM - no stand-alone LayerNorm launch (1: where the producer is not K-split anyway;
                                 // 2: also un-split the producers with K <= ln_pairs_maxk).  The ADM alone (d = 768: both residual GEMMs
                                 // have K <= 1024) is where the hand-off pays at B = 32: interleaved C3 -0.43 %, C2 -1.3 %; in the PLM and
                                 // globally it measured +0.65 .. +2.0 % and was retired (profiles/r05_opts_ab.txt)
    int ln_pairs_maxk = 1024;    // ... ln_pairs = 2: the longest K chain that is taken out of the K split
    int ln_pairs_maxm = 1280;    // ... only for launches of at most this many rows: beyond, the consumers run on the 256x128 tile
                                 // (no pair-fed form) and a LayerNorm launch is no longer a latency item (C5: 5342 vs 5210 ms without a cap,
                                 // +0.46 % for the ADM alone at 2048, +0.1 % at 1280)
};
// gemm_dispatch.hip: the front door of the engine.  gemm_route decides, without a HIP call, what launch_gemm does with a launch:
// the error it returns (hipSuccess: it launches), the configuration index (gemm_config_name; 87..90: the <= 64-row kernels of
// gemm_skinny.hip; -1: nothing to launch or rejected before a choice), the variant of that tile's kernel (GemmVariant, gemm_tiles.h),
// the dynamic LDS bytes, and the row-statistics layout it writes (0: none - a stat_out the chosen kernel cannot serve is dropped)
// ks_epi4: 1 - an x3h K-split tile finishes the launch with 16-byte loads and stores (EngineOpts::ks_epi4 and N, ldc, ldr, the group
// strides in fours, C / R / bias / wh_inv / ln_g on 16 bytes); 0 - the dword finish of the same kernel, or another kernel altogether
struct GemmRoute { hipError_t err; int cfg; int variant; size_t lds; int stat_nt, stat_w; int ks_epi4; };
GemmRoute gemm_route(const GemmP& p, const EngineOpts& o);
hipError_t launch_gemm(const GemmP& p, hipStream_t s, EngineOpts* o = nullptr);
// The vocoder's resblock pair  Y = X + conv2(lrelu(conv1(lrelu(X))))  as ONE launch (conv_pair_x3h_kernel, gemm_x3h.hip): conv1 with
// `taps` taps and dilation `dil`, conv2 with `taps` taps and dilation 1, both "same" convolutions C -> C over the R gap-padded rows of
// X, the leaky ReLU's slope `slope`, rows with valid[m] == 0 written as zeros (and read as zeros by conv2).  The weights come as the fp16
// planes of GemmP::Wh ([C][taps * C / 32] blocks of 128 bytes, wh_ldb bytes between rows, both matrices alike) with the inverse row
// scales inv1 / inv2.  Bit-identical to the two launch_gemm calls on the x3h window tiles that it replaces.
struct PairP {
    const float* X; int ldx;
    int R, C, taps, dil;
    float slope;
    const void* Wh1; const float* inv1; const float* bias1;
    const void* Wh2; const float* inv2; const float* bias2;
    long long wh_ldb;
    const int* valid;
    float* Y; int ldy;
    int reflect = 0;            // 1: the caller runs the vocoder with reflect padding (halo rows between the two convolutions): never fused
    int* x3h_flag = nullptr;    // set by launch_conv_pair from EngineOpts::x3h_flag
    int ldr_prio = 0;           // ... from EngineOpts::ldr_prio
};
// conv_pair_route decides, without a HIP call, what launch_conv_pair does (the gemm_route pattern).  err: hipSuccess - it launches (or
// R <= 0: nothing to launch, grid 0); hipErrorNotSupported - the caller keeps the two-launch form: C not in {32, 64, 128} or its bit
// of EngineOpts::pair_fuse clear, reflect padding, (taps - 1) dil > 64, missing planes, an operand of 2 GiB or more, an operand off its alignment (X, Y,
// biases on 16 bytes, planes and wh_ldb on 128, ldx / ldy multiples of 4), or engine options under which the two launches would not
// run on the x3h window tiles (win_conv / x6_conv / x3h bit 2 off, a forced configuration, ldr64); hipErrorInvalidValue - taps < 2,
// dil < 1, C <= 0, X or Y null, ldx / ldy < C, wh_ldb < 4 taps C.  tile: 0 / 1 / 2 = 32 / 64 / 128 channels; bm rows per pass, bmo = bm - (taps - 1) output rows per
// workgroup, grid = ceil(R / bmo), lds = ring + (C / 32) * ceil8(bm + (taps - 1) dil) * 128 bytes.
struct PairRoute { hipError_t err; int tile; size_t lds; unsigned grid, block; int bm, bmo; };
PairRoute conv_pair_route(const PairP& p, const EngineOpts& o);
hipError_t launch_conv_pair(const PairP& p, hipStream_t s, EngineOpts* o = nullptr);
// The MRF mean of a vocoder stage and the stride-2 ConvTranspose1d of the next stage as ONE launch (up_mrf_x3h_kernel, gemm_x3h.hip), with
// co = ch / 2, h(n) = (n >= co), rows outside [0, R) reading as zeros:
//   m[r, c] = lrelu(((X0[r, c] + X1[r, c]) + X2[r, c]) * scale; slope)                      (avg3_kernel's operation order)
//   Y[q, n] = valid[q] ? bias[n mod co] + sum_c m[q - 1 + h, c] Wcat[n, c] + sum_c m[q + h, c] Wcat[n, ch + c] : 0
// Y is [R, 2 co] = [2 R, co] time-major.  Wcat [2 co][2 ch] (rows 0 .. co - 1: UpW::wlo, rows co ..: UpW::whi) comes as the fp16 planes
// of GemmP::Wh with its inverse row scales; products in the x3h form.  Replaces launch_avg3 + the two GEMM halves of the upsampler.
struct UpMrfP {
    const float* X0; const float* X1; const float* X2; int ldx;     // the three resblock outputs [R, ch], one row stride
    int R, ch, stride;
    float scale, slope;
    const void* Wh; const float* inv; const float* bias; long long wh_ldb;
    const int* valid;
    float* Y; int ldy;
    int* x3h_flag = nullptr;    // set by launch_up_mrf from EngineOpts::x3h_flag
    int ldr_prio = 0;           // ... from EngineOpts::ldr_prio
};
// up_mrf_route decides, without a HIP call, what launch_up_mrf does (the conv_pair_route pattern).  err: hipSuccess - it launches (or
// R <= 0: nothing to launch, grid 0); hipErrorNotSupported - the caller keeps the three launches: ch not in {64, 128} or its bit of
// EngineOpts::up_fuse clear, stride != 2, missing planes, engine options under which the window kernels do not run in the x3h form
// (win_conv / x6_conv / x3h bit 2 off, a forced configuration, ldr64), an operand of 2 GiB or more, an operand off its alignment (X0 /
// X1 / X2 / Y / bias on 16 bytes, planes and wh_ldb on 128, ldx / ldy multiples of 4); hipErrorInvalidValue - X0 / X1 / X2 / Y null, ldx /
// ldy < ch, wh_ldb < 8 ch.  tile: 0 / 1 = 64 / 128 channels; bm rows (output row pairs) per workgroup, grid = ceil(R / bm), lds = ring +
// (ch / 32) * ceil8(bm + 2) * 128 bytes.
struct UpMrfRoute { hipError_t err; int tile; size_t lds; unsigned grid, block; int bm; };
UpMrfRoute up_mrf_route(const UpMrfP& p, const EngineOpts& o);
hipError_t launch_up_mrf(const UpMrfP& p, hipStream_t s, EngineOpts* o = nullptr);
// would launch_gemm run this launch (planes attached, no prologue) on an x3h tile that takes its A operand as fp16 planes (a_planes)?
bool gemm_takes_planes(const GemmP& p, const EngineOpts& o);
// would launch_gemm run this launch on an x3h loader tile whose epilogue can store C as fp16 planes (GemmP::c_planes)?
bool gemm_writes_planes(const GemmP& p, const EngineOpts& o);
// gemm_skinny.hip: weight-streaming linear layer for M <= 64 rows (taps = 1, no rowbase, K a multiple of 32)
bool gemm_skinny_eligible(const GemmP& p, int max_rows);
hipError_t launch_gemm_skinny(const GemmP& p, hipStream_t s);
// ... on a tile-major weight copy (GemmP::Wtm), optionally with the LayerNorm prologue (pro_act == 3, groups == 1, K <= 1024)
bool gemm_skinny_tm_eligible(const GemmP& p, int max_rows);
hipError_t launch_gemm_skinny_tm(const GemmP& p, hipStream_t s);
int gemm_skinny_tm_waves(const GemmP& p);      // the waves that split K in that launch: 8, 12 or 16 (GemmP::sk_nw, M, K, prologue)
hipError_t launch_tile_major(const float* W, int N, int K, float* out, hipStream_t s);   // row-major [N, K] -> tile-major blocks
int gemm_num_configs();
const char* gemm_config_name(int idx);
// per tile configuration: launches, executed FLOPs, summed ms; last entry "union" (see gemm_dispatch.hip); -1 on error
int gemm_trace_collect(EngineOpts& o, int cap, const char** names, int64_t* launches, double* flops, double* ms);
// text table "config M N K groups launches ms tflops" of the traced launches grouped by shape, slowest first (call
// BEFORE gemm_trace_collect, which frees the records); returns the number of bytes written (< cap)
int gemm_trace_shapes(EngineOpts& o, char* buf, int cap, int top);

// Row LayerNorm over C channels (biased variance, eps inside the sqrt), one wave per row:
//   out[m, :] = mask_m * ( act( LN(x[m, :]) * gamma[g] + beta[g] ) + R1[m, :] + R2[m, :] )
// rows_per_group > 0: gamma/beta of group g = m / rows_per_group start at g * C.
// valid_rows > 0: the mask index is m % valid_rows (one mask shared by all groups);
// r1_rows > 0: the R1 row is m % r1_rows (one residual input shared by all groups).
struct LnP {
    const float* x; int ldx;
    const float* gamma; const float* beta; int rows_per_group;
    const float* R1; int ldr1; int r1_rows; const float* R2; int ldr2;
    const int* valid; int valid_rows;
    float* out; int ldo;
    int M, C; float eps; int act;
    int out_planes = 0;         // 1: `out` receives fp16 planes ([32 hi | 32 lo] per 32 channels, the A operand of a GemmP::a_planes launch;
                                // same bytes and row stride as f32; C % 32 == 0) instead of f32; x3h_flag: the range guard's device word
    int* x3h_flag = nullptr;
};
hipError_t launch_layernorm(const LnP& p, hipStream_t s);

// Split-K consumer (rowops.hip): x_new = R + bias + sum_g parts[g] (g = 0..S-1, fixed order);
// xout = x_new (may alias R; nullable), hout = LayerNorm(x_new) * gamma + beta.  parts[g] = parts + g*pstride, [M, C] dense.
struct LnReduceP {
    const float* parts; long long pstride; int S;
    const float* bias; const float* R; int ldr;
    const float* gamma; const float* beta;
    float* xout; int ldx; float* hout; int ldh;
    int M, C; float eps;
    int h_planes = 0;           // 1: hout receives fp16 planes (LnP::out_planes); the one-row-per-workgroup kernel only (M <= 4096)
    int* x3h_flag = nullptr;
};
hipError_t launch_ln_reduce(const LnReduceP& p, hipStream_t s);

// Non-causal multi-head attention over per-utterance row ranges (flash-style, f32 MFMA).
//   Q rows of utterance b: [q_start[b], q_start[b]+q_len[b]) in Q (ld ldq), head h at column h*D.
//   K/V likewise with kv_start/kv_len.  If q_start == nullptr the batch is uniform:
//   start = b * u_qstride (q) / b * u_kvstride (kv), len = u_qlen / u_kvlen.
//   Output rows: o_start[b] + i (default q_start), uniform: b * u_ostride + i (default u_qstride).
struct AttnP {
    const float* Q; int ldq; const float* K; int ldk; const float* V; int ldv;
    float* O; int ldo;
    const int* q_start; const int* q_len; const int* kv_start; const int* kv_len; const int* o_start;
    int u_qstride, u_qlen, u_kvstride, u_kvlen, u_ostride;
    int B, H, D, max_qlen; float scale;
    int max_kvlen;   // ragged launches: longest key range (0 = unknown), sizes the split-KV width
    int lds_min_qlen = 640;   // from this many queries on (and D <= 128) the LDS-tiled kernel shares K / V tiles between 8 query
                              // tiles of a workgroup (attn_f32_lds_kernel); 0: never
    int x6_min_qlen = 0;      // from this many queries on (D = 64 / 96) the f32-equivalent bf16-pipe kernel (attn_x6_kernel); 0: never
    int lds_waves = 0;        // query tiles per workgroup of that kernel: 8, otherwise 4
    int ds_short = 1;         // D = 64 / 96 and at most 128 keys: key tiles x head-dim slices per workgroup (attn_f32_ds_kernel)
    int x3h = 0;              // 1: the long-sequence kernel in its fp16-pipe form (two planes, three products; range-guarded through x3h_flag)
    int o_planes = 0;         // 1: O receives fp16 planes (planes_store.h: the A operand of the out-projection's GemmP::a_planes launch; same
    int* x3h_flag = nullptr;  // bytes and row stride as f32; D % 32 == 0, ldo % 32 == 0, O on 128 bytes); x3h_flag: the range guard's device word
};
// attn_route decides, without a HIP call, what launch_attention does with a launch - the one place where a kernel is chosen:
// err (hipSuccess: it launches, or there is nothing to launch: kernel == ATTN_NONE), the kernel, the template arguments that
// matter for it, and the launch geometry.  launch_attention launches from this result and decides nothing itself.
enum AttnKernel {
    ATTN_NONE = 0,      // nothing to launch (B, H or max_qlen <= 0) or rejected
    ATTN_GENERIC = 1,   // attn_f32_kernel<dt>: wide heads, nwv waves of dt 32-column tiles each
    ATTN_REG = 2,       // attn_f32_reg_kernel<d>: nwv split-KV waves
    ATTN_DS = 3,        // attn_f32_ds_kernel<d>: nkv key tiles x d / 32 head-dim slices
    ATTN_LDS = 4,       // attn_f32_lds_kernel<d, nwq>
    ATTN_X6 = 5,        // attn_x6_kernel<d, nwq>: bf16 pipe, six products
    ATTN_X3H = 6,       // attn_x6_kernel<d, nwq, true>: fp16 pipe, three products
};
struct AttnRoute {
    hipError_t err; int kernel;
    int d;              // template head dim D (reg, ds, lds, x6, x3h); generic: DT, the 32-column tiles per wave
    int nwq;            // query tiles (= waves) per workgroup (lds, x6, x3h; otherwise 1)
    int nkv;            // key tiles per workgroup (ds; otherwise 0)
    int nwv;            // split-KV waves (reg), waves across the head dim (generic); otherwise 0
    unsigned gx, gy, gz, block;
    size_t lds;         // dynamic LDS bytes
};
AttnRoute attn_route(const AttnP& p);
hipError_t launch_attention(const AttnP& p, hipStream_t s);

// ---- row utilities (rowops.hip) ------------------------------------------------------------------
// out[r, :] = table[ids[idmap[r]], :] + pe[pos[r], :]   (idmap[r] < 0 -> zero row)
hipError_t launch_embed_pe(const float* table, int C, const int64_t* ids, const int* idmap, const int* pos,
                           const float* pe, float* out, int ldo, int R, int vocab, hipStream_t s);
// out[r, 0:C] = src[map[r], 0:C] (map[r] < 0 -> zeros);  generic row gather
hipError_t launch_gather_rows(const float* src, int lds_, const int* map, float* out, int ldo, int C, int R,
                              hipStream_t s);
// out[r, :] = max_{i < cnt[r]} src[first[r] + i, 0:C]   (cnt[r] == 0 -> zeros): ceil-mode max-pool
hipError_t launch_pool_max(const float* src, int lds_, const int* first, const int* cnt, float* out, int ldo,
                           int C, int R, hipStream_t s);
// out[r, :] = sum_g x[g*strideG + r*ld + :]
hipError_t launch_sum_groups(const float* x, long long strideG, int groups, int ld, float* out, int ldo, int C,
                             int R, hipStream_t s);
// dst[r, c] = (a[r,c] + b[r,c] + d[r,c]) * scale  (HiFi-GAN MRF mean)
hipError_t launch_avg3(const float* a, const float* b, const float* d, float scale, float* out, long long n,
                       hipStream_t s);
// MRF mean of the last stage + leaky ReLU + conv_post (Cout = 1) + tanh in one pass; x1 = x2 = nullptr: x0 is the mean already
hipError_t launch_conv_post(const float* x0, const float* x1, const float* x2, float scale, long long R, int ch, int k,
                            const float* w, const float* bias, float slope, const int* valid, float* out, hipStream_t s);
// padded [B, Tmax, C] (or channel-major [B, C, Tmax] when cmajor) <-> packed rows; rowmap[r] = b*Tmax + t or -1
hipError_t launch_pack_rows(const float* src, int C, int Tmax, int cmajor, const int* rowmap, float* dst, int ldd,
                            int R, hipStream_t s);
hipError_t launch_unpack_rows(const float* src, int lds_, int C, int Tmax, int cmajor, const int* rowmap,
                              float* dst, int R, hipStream_t s);
// AR step input rows (models/megatts2.py:172-176,264-269): uniform length n = t+1, A active sequences
//   ADM: x[j*n+i] = [tc_emb[tc_row[j]+i, 0:Dc] , w_dt[0:De] * p[j*pstride + i]] + pe[i]
hipError_t launch_adm_step_input(const float* tc_emb, int ld_tc, const int* tc_row, const float* w_dt,
                                 const float* p, int pstride, const float* pe, float* x, int Dc, int De,
                                 int n, int A, hipStream_t s);
//   PLM: x[j*n+i] = [cond[cond_row[j]+i, 0:Dc], emb[codes[j*cstride+i], 0:De]] + pe[i]
hipError_t launch_plm_step_input(const float* cond, int ld_c, const int* cond_row, const float* emb,
                                 const int64_t* codes, int cstride, const float* pe, float* x, int Dc, int De,
                                 int n, int A, int emb_rows, hipStream_t s);
// ADM head: p[j*pstride + n] = dot(x[j*xn + xn-1, 0:D], w)    (predict_layer, last position only; xn = rows
// per sequence in x: n for the full step matrix, 1 for the last-row matrix of the last layer)
hipError_t launch_adm_predict(const float* x, int D, const float* w, float* p, int pstride, int n, int xn, int A,
                              hipStream_t s);
// dur[i] = clamp(trunc(p + 0.5), 1, 128)  (models/megatts2.py:275)
hipError_t launch_adm_finalize(const float* p, int pstride, const int* lens, const int* slot_b, int32_t* dur,
                               float* flt, int dstride, int A, int nmax, hipStream_t s);
// out[slot_b[j]*ostride + t] = codes[j*cstride + 1 + skip + t] for t < lens[j] - skip (skip = prompt prefix length)
hipError_t launch_plm_finalize(const int64_t* codes, int cstride, const int* lens, const int* slot_b, int64_t* out,
                               int ostride, int A, int nmax, int skip, hipStream_t s);
// AR history initialisation (one launch instead of a host-staged copy):
//   ADM  p[j*pstride + 0] = 0 (models/megatts2.py:262), p[j*pstride + 1 + i] = prefix[slot_b[j]*P + i], rest 0
//   PLM  codes[j*cstride + 0] = bos (:170), codes[j*cstride + 1 + i] = prefix[slot_b[j]*pstride + i], rest 0
hipError_t launch_adm_init_hist(float* p, int pstride, const float* prefix, int P, const int* slot_b, int A,
                                hipStream_t s);
hipError_t launch_plm_init_hist(int64_t* codes, int cstride, int64_t bos, const int64_t* prefix, int P, int pstride,
                                const int* slot_b, int A, hipStream_t s);
// flag |= bit when an id used by the call is outside [0, hi): ids[map[r]] for map[r] >= 0 (map == nullptr: ids[r])
hipError_t launch_check_ids(const int64_t* ids, const int* map, int R, long long hi, int* flag, int bit,
                            hipStream_t s);
// dst[j*dpitch + c] = src[j*spitch + c], c < width, j < rows (float4 granularity)
hipError_t launch_copy_2d(const float* src, long long spitch, float* dst, long long dpitch, long long width, int rows,
                          hipStream_t s);
hipError_t launch_scatter_i64(const int64_t* src, const int* map, int64_t* out, int R, hipStream_t s);
hipError_t launch_expand_mask(const int* in, int factor, int* out, long long n, hipStream_t s);
hipError_t launch_unpack_wav(const float* src, const long long* start, const long long* len, float* out,
                             long long out_stride, long long max_len, int B, hipStream_t s);
// row arg-max with lowest-index ties (torch.argmax): out[j*ostride + ooff] = argmax_n x[j, 0:N]
hipError_t launch_argmax_rows(const float* x, int ldx, int N, int64_t* out, int ostride, int ooff, int A,
                              hipStream_t s);
// seeded temperature / top-k / top-p draw (sampling.hip; N <= 1024): out[j*ostride + ooff] = the code of row j under the rule
// of sampling.hip with Philox key = seeds[2b], seeds[2b+1] (lo, hi) of utterance b = slot ? slot[j] : j and counter
// = pos ? pos[j] : pos0.  top_k = 1 is launch_argmax_rows on rows without NaN (the rule orders finite and infinite logits only; a NaN
// row is launch_argmax_rows' alone to define).  hipErrorInvalidValue for parameters outside the rule.
hipError_t launch_sample_rows(const float* x, int ldx, int N, int64_t* out, int ostride, int ooff, int A, float tau, int top_k,
                              float top_p, const uint32_t* seeds, const int* slot, const int* pos, int pos0, hipStream_t s);
// the same draw on the MIXTURE of two rows (prosody interpolation; rule in sampling.hip): pair j = rows 2j, 2j + 1 of x, utterance
// b = slot ? slot[j] : j gives the seed and gamma[b] in [0, 1] (device f32); the code goes to out[(2j)*ostride + ooff] AND
// out[(2j+1)*ostride + ooff].  greedy: arg-max of the mixture at temperature 1 (tau / top_k / top_p / seeds / pos unused).
hipError_t launch_sample_mix_rows(const float* x, int ldx, int N, int64_t* out, int ostride, int ooff, int A, bool greedy, float tau,
                                  int top_k, float top_p, const uint32_t* seeds, const int* slot, const int* pos, int pos0,
                                  const float* gamma, hipStream_t s);
// EuclideanCodebook.quantize (core_vq.py:175-183) given xe = x @ E^T:
//   idx[m] = argmax_j -((|x_m|^2 - 2*xe[m,j]) + ee[j]), lowest index on ties
hipError_t launch_vq_argmin(const float* x, int ldx, int D, const float* xe, int ldxe, const float* ee, int N,
                            const int* valid, int64_t* idx, int M, hipStream_t s);
// ee[j] = sum_d E[j,d]^2
hipError_t launch_row_sqnorm(const float* E, int D, float* ee, int N, hipStream_t s);
// zq rows (modules/vqpe.py:59-61): out[r] = E[codes[codemap[r]]]
hipError_t launch_codebook_rows(const float* E, const int64_t* codes, const int* codemap, float* out, int ldo,
                                int Dq, int R, int bins, hipStream_t s);
// mel front-end helpers (rowops.hip)
hipError_t launch_reflect_pad_blocks(const float* wav, long long wstride, const int* blk_b, const int* blk_t,
                                     const int* len, int hop, int pad, float* out, int R, hipStream_t s);
hipError_t launch_magnitude(const float* spec, int lds_, int F, float* out, int ldo, int M, hipStream_t s);
// reflect halo rows of every utterance (rows start[b]*scale .. +len[b]*scale) in front of a "same" convolution
hipError_t launch_fill_reflect(float* x, int ld, int C, const int* start, const int* len, int B, long long scale, int G,
                               hipStream_t s);
// no-op kernel named mt2::stage_marker_kernel<ID> (ID 0..15): stage boundary in a kernel trace
hipError_t launch_stage_marker(int id, hipStream_t s);

// ---- sample-rate conversion of prompt audio (resample.hip; reference models/megatts2.py:335-336) --------------------------
// The polyphase rule of one (sr_in, sr_out) pair, reduced by their gcd: o input samples per block of n output samples, `taps`
// = 2 * width + o filter taps per phase; tb = output blocks per workgroup (the window of (tb - 1) * o + taps inputs sits in LDS).
struct ResampleRule { int o, n, width, taps, tb; };
// host only, no HIP call: nullptr and *r filled, or the reason the pair is refused (rates <= 0, equal rates, a table n * taps * 4
// bytes over 8 MiB, a phase that does not fit the LDS window)
const char* resample_rule(int sr_in, int sr_out, ResampleRule* r);
long long resample_out_len(const ResampleRule& r, long long L);      // ceil(n * L / o)
// the filter in double, rounded once to f32: [n][taps] phase-major, or [taps][n] tap-major (what the kernel reads)
void resample_table(const ResampleRule& r, float* table, bool tap_major);
// out[b, j] = sum_k table[k][j % n] * wav[b, (j / n) * o - width + k] for j < lout[b] (wav = 0 outside [0, len[b])), 0 for
// lout[b] <= j < Lout_max.  Workgroup t owns the output blocks [tile_i0[t], tile_i0[t] + tb) of utterance tile_b[t]; the tiles cover
// [0, Lout_max) of every utterance.  peak != nullptr: peak[b] = max(peak[b], max_j |out[b, j]|) as the u32 pattern of the float.
struct ResampleP {
    const float* wav; int L_max;              // [B, L_max]
    int a0;                                   // (address of wav / 4) % 4 - which elements sit on 16 bytes; set by the launcher
    const float* table; ResampleRule r;
    const int* tile_b; const int* tile_i0; int tiles;
    const int* len; const int* lout;
    float* out; int Lout_max;
    unsigned* peak;
};
hipError_t launch_resample_rows(const ResampleP& p, hipStream_t s);
// peak[b] = max(peak[b], max_{j < len[b]} |x[b * stride + j]|), same encoding (zero the words first)
hipError_t launch_peak_rows(const float* x, long long stride, const int* len, int max_len, int B, unsigned* peak, hipStream_t s);
// librosa.util.normalize per utterance: out[b, j] = x[b, j] / peak[b] for j < len[b] (unchanged while peak[b] < FLT_MIN), 0 for
// len[b] <= j < width; out may be x
hipError_t launch_scale_rows(const float* x, long long xstride, const int* len, const unsigned* peak, float* out, long long ostride,
                             int width, int B, hipStream_t s);

// ---- leading / trailing silence of prompt audio (trim.hip; reference models/megatts2.py:337, librosa.effects.trim) ------------
// host only, no HIP call: F = 1 + L / 512 frames, c = (float)pow(10.0, -top_db / 10.0)
int trim_frames(long long L);
float trim_factor(float top_db);
// The cut of one utterance from the two words the kernels leave (first kept frame by atomic min from UINT_MAX, last by atomic max
// from -1): [512 first, min(L, 512 (last + 1))).  Words that name no kept frame - or no frame of this utterance, which only a
// non-finite sample can bring about - leave the utterance whole, so the cut is inside [0, L] whatever the input.
__host__ __device__ inline void trim_bounds(unsigned first, int last, int L, int* start, int* end) {
    const bool whole = last < 0 || last >= 1 + L / 512 || first > (unsigned)last;
    const long long e = 512ll * ((long long)last + 1);
    *start = whole ? 0 : 512 * (int)first;
    *end = whole || e > L ? L : (int)e;
}
// Four launches on one stream, each one grid over the ragged batch: block sums -> frame energies + peak -> first / last kept frame
// -> compaction copy.  The caller zeroes peak[], sets first[] to UINT_MAX and last[] to -1 in front.
struct TrimP {
    const float* wav; int L_max;              // [B, L_max]; samples at or beyond len[b] are never read
    const int* len; int max_len, B;           // device [B]; max_b len[b]
    float factor;                             // trim_factor(top_db)
    float* sums; int NB;                      // scratch [B, NB], NB >= ceil(max_len / 512)
    unsigned* peak; unsigned* first; int* last;      // scratch [B] each
    float* out; int Lout_max;                 // [B, Lout_max], Lout_max >= max_len
    float* energy; int F_max;                 // optional [B, F_max], F_max >= 1 + max_len / 512: e[f], zeros in [F_b, F_max)
};
hipError_t launch_trim(const TrimP& p, hipStream_t s);
// the first two launches alone: sums, peak and - where asked for - energy; out, first and last are not looked at
hipError_t launch_trim_energy(const TrimP& p, hipStream_t s);

// ---- speech segments by frame energy and the cut that takes the pauses out (segments.hip; the rule is in its header) ------------
// host only: the most segments an utterance of F frames can have, max(1, (F + min_pause) / (min_speech + min_pause)) in 64 bits
long long segments_bound(long long F, int min_pause, int min_speech);
constexpr int kSegWords = 8;      // per utterance: F, raw active, kept frames, +-segments, longest pause, kept samples, 0, 0
// Up to three launches on one stream, picked by `what`: smoothing and enumeration (one workgroup per utterance) -> figures -> copy.
enum { kSegSmooth = 1, kSegFigures = 2, kSegCopy = 4 };
struct SegP {
    const float* energy; int E_pitch;         // [B, E_pitch]: e[f] of each utterance, read for f < flen[b] only
    const int* flen; int max_F, B;            // device [B]: frames; max_b flen[b]
    const int* len;                           // device [B]: samples (segments in samples, cutting) or NULL (the staged form: frames)
    float factor; int min_pause, min_speech, pad, keep;
    int* prv; int* dst; unsigned char* fb; unsigned char* fc; unsigned char* fd; int W;      // scratch [B, W] each, W >= max_F
    int* words;                               // scratch [B, kSegWords]
    unsigned char* flags; int D_pitch;        // optional [B, D_pitch]: d, in place of fd (bytes at or beyond flen[b] are left alone)
    int* seg; int S_max;                      // optional [B, S_max, 2], -1 behind the segments found; S_max >= segments_bound(max_F)
    int* counts;                              // optional [B]
    double* fig;                              // optional [B, MT2_SEGMENTS_FIELDS]
    const float* wav; int L_max;              // cutting: [B, L_max]; samples at or beyond len[b] are never read
    float* out; int Lout_max;                 // optional [B, Lout_max], Lout_max >= max_b len[b]
};
hipError_t launch_segments(const SegP& p, int what, hipStream_t s);

// ---- dynamic time warping of a synthesised mel onto a real one (dtw.hip; the rule is in its header and in megatts2_hip.h) --------
// host only, no HIP call: u32 words of packed directions per row
long long dtw_dir_words(int Ty_max);
long long dtw_skew_steps(int Ty_max);          // 64 ceil((Ty_max + 63) / 64): steps a strip of 64 skewed rows takes, in whole periods
// Three launches on one stream, each over the ragged batch: cost -> accumulate (one workgroup per utterance) -> backtrack (one wave
// per utterance).  Cells outside an utterance's Tx_b x Ty_b are neither read nor written.
struct DtwP {
    const float* X; int Tx_max;               // [B, Tx_max, D]; rows at or beyond x_len[b] are never read
    const float* Y; int Ty_max;               // [B, Ty_max, D]; likewise y_len[b]
    int D, B;
    const int* x_len; const int* y_len;       // device [B]
    int max_tx, max_ty;                       // max_b of the lengths
    float* cost;                              // optional [B, Tx_max, Ty_max]: c in the caller's layout
    float* skew; int S_max, TS;               // scratch [B, S_max, TS, 64]: c[64 s + l, t - l] at [s][t][l] - what the 64 lanes of a strip
                                              // read at step t is one contiguous line; S_max >= ceil(max_tx / 64), TS >= dtw_skew_steps(max_ty)
    unsigned* dirs; int DW;                   // scratch [B, Tx_max, DW], DW >= dtw_dir_words(max_ty): 2 bits a cell, 16 columns a word
    float* acc;                               // optional [B, Tx_max, Ty_max]: A itself
    int* lo; int* hi;                         // [B, Ty_max]; -1 in [Ty_b, Ty_max)
    int* steps; float* total;                 // [B]
};
hipError_t launch_dtw_cost(const DtwP& p, hipStream_t s);
hipError_t launch_dtw_accumulate(const DtwP& p, hipStream_t s);
hipError_t launch_dtw_backtrack(const DtwP& p, hipStream_t s);
// dur[b, p] = lower_bound(hi_b, cum[b, p+1]) - lower_bound(hi_b, cum[b, p]) for p < np_len[b], 0 up to Np_max; last[b] = hi_b[Ty_b - 1]
struct AlignDurP {
    const int* hi; int Ty_max;                // [B, Ty_max]
    const int* y_len; const int* cum;         // device [B]; [B, Np_max + 1] exclusive prefix sums of the synthetic durations
    const int* np_len; int Np_max, B;         // device [B]
    int* dur; int* last;                      // [B, Np_max]; [B]
};
hipError_t launch_dtw_durations(const AlignDurP& p, hipStream_t s);

// ---- mel-cepstral distortion along a DTW path (mcd.hip; the rule is in its header and in megatts2_hip.h) ----------------------------
// host only, no HIP call: n_mels in [2, 128] and order in [1, min(n_mels - 1, MT2_MCD_MAX_ORDER)];  tab[k-1][m] = cos(pi (m + 1/2) k / N) / N
bool mcd_geometry_ok(int n_mels, int order);
void mcd_table(int n_mels, int order, float* table);
// cep[b, t, k-1] = sum_m mel[b, t, m] table[k-1][m], one f32 fma chain over m ascending; zeros for t in [len[b], T_max)
struct McdCepP {
    const float* mel; int T_max, N;           // [B, T_max, N]; rows at or beyond len[b] are never read
    int K, B;
    const int* len;                           // device [B]
    const float* table;                       // device [K][N]: mcd_table
    float* cep;                               // [B, T_max, K]
};
hipError_t launch_mcd_cepstrum(const McdCepP& p, hipStream_t s);
// the path's row of MT2_MCD_FIELDS doubles, one workgroup per utterance
struct McdPathP {
    const float* ca; int Ta_max;              // [B, Ta_max, K]
    const float* cb; int Tb_max;              // [B, Tb_max, K]
    int K, B;
    const int* a_len; const int* b_len;       // device [B]
    const int* lo; const int* hi;             // [B, Tb_max], as launch_dtw_backtrack left them
    const float* f0_a; const float* f0_b;     // optional [B, Ta_max], [B, Tb_max]: both or neither
    double* out;                              // [B, MT2_MCD_FIELDS]
};
hipError_t launch_mcd_path(const McdPathP& p, hipStream_t s);

// ---- stationary-noise suppression between the two STFT GEMMs (denoise.hip; the rule is in its header and in megatts2_hip.h) ----------
// Utterance b owns the rows row0[b] .. row0[b] + T[b] of the spectrum ([rows, lds]: re(0..F-1) | im(0..F-1) | pad) and of P ([rows, Fp]);
// a row at or beyond T[b] and a column at or beyond F is never read.
constexpr int kDnSelBins = 16;                // adjacent bins a select workgroup takes: a 64-byte segment of every row of P
constexpr int kDnTileT = 16, kDnTileF = 64;   // the gain kernel's tile of cells; its halo is at most kDnMaxSmooth on every side
constexpr int kDnMaxSmooth = 8;
// host only: c = (float)(1 / -ln(1 - percentile / 100)) and the rank k = ((T - 1) percentile + 50) / 100
float denoise_factor(int percentile);
inline int denoise_rank(int T, int percentile) { return (int)((((long long)T - 1) * percentile + 50) / 100); }
struct DenoiseP {
    const float* spec; int lds;               // the spectrum rows
    float* spec_out;                          // the gated rows in the same row numbering (may be spec itself), or nullptr
    const int* row0; const int* T;            // device [B]
    int B, F, Fp, T_cap;                      // T_cap >= max_b T[b]: sizes the grids and the partial sums
    float* P;                                 // [rows, Fp]: written by launch_denoise_power, read by the other two
    float* floor_out;                         // launch_denoise_select: [B, Fp], zeros in the columns F .. Fp-1
    const float* floor;                       // launch_denoise_gain / _figures: [B, Fp]
    float* gain_out; int gain_T;              // optional [B, gain_T, Fp]: only the cells (t < T[b], f < F) are written
    int percentile, bf, bt;
    float c, beta, gmin;
    double* part;                             // optional [B, tiles_t(T_cap), tiles_f, 3]: sum P, sum g^2 P and the floored cells of a tile
    double* fig;                              // launch_denoise_figures: [B, MT2_DENOISE_FIELDS]
};
hipError_t launch_denoise_power(const DenoiseP& p, hipStream_t s);
hipError_t launch_denoise_select(const DenoiseP& p, hipStream_t s);
hipError_t launch_denoise_gain(const DenoiseP& p, hipStream_t s);
hipError_t launch_denoise_figures(const DenoiseP& p, hipStream_t s);

// ---- de-reverberation by weighted prediction error between the two STFT GEMMs (wpe.hip; the rule is in its header and in megatts2_hip.h)
// Utterance b owns the rows row0[b] .. row0[b] + T[b] of the spectrum ([rows, lds], as above) and the bin-major complex f32 columns
// cols[c0[b] + f Tp .. + Tp], f < F, Tp = T[b] rounded up to 4 (c0 in float2 units, a multiple of 4); run[b] = 0: every bin of b passes through.
constexpr int kWpeThreads = 512, kWpeMaxTaps = 16;
constexpr int kWpeLdsFrames = 4096;           // the column sits in LDS beside its weights up to here: 16 bytes a frame, two workgroups a CU
constexpr int kWpeStat = 5;                   // per bin: sum |Y|^2, sum |D|^2, filtered (1) or passed (0), max_k |g|, iterations completed
size_t wpe_lds_bytes(int T_cap);              // host only: the dynamic LDS of launch_wpe_bins
struct WpeP {
    const float* spec; int lds;               // launch_wpe_to_bins: the spectrum rows (16-byte aligned)
    float* spec_out;                          // launch_wpe_from_bins: the same row numbering; only the cells (t < T[b], f < F) are written
    const int* row0; const int* T; const int* c0; const int* run;      // device [B]
    int B, F, Fp, T_cap;                      // T_cap >= max_b T[b]: sizes the grids and the LDS
    float2* cols; float2* cols_out;           // Y and D, bin-major; written whole (zeros in the frames T[b] .. Tp-1)
    int delay, taps, iters, ctx;
    double eps, load;
    double* filters;                          // optional [B, Fp, taps, 2]: the rows f < F are written (zeros for a bin that passed through)
    double* stat;                             // [B, F, kWpeStat]
    double* fig;                              // launch_wpe_figures: [B, MT2_WPE_FIELDS]
};
hipError_t launch_wpe_to_bins(const WpeP& p, hipStream_t s);
hipError_t launch_wpe_bins(const WpeP& p, hipStream_t s);
hipError_t launch_wpe_from_bins(const WpeP& p, hipStream_t s);
hipError_t launch_wpe_figures(const WpeP& p, hipStream_t s);

// ---- declipping by sparsity, A-SPADE (declip.hip; the rule is in its header and in megatts2_hip.h)
// Utterance b owns the frames row0[b] .. row0[b] + T_b of `frames` ([rows, N] doubles) and of `it` ([rows]), T_b = ceil(len[b] / hop) + 3,
// hop = N / 4.  det: kDcDet words an utterance: the bits of hi and lo, n_hi, n_lo, side clipped high / low (0 / 1), non-finite, 0.
constexpr int kDcThreads = 256, kDcDetThreads = 1024, kDcDet = 8;
size_t dc_lds_bytes(int N);                   // host only: the dynamic LDS of launch_dc_frames
size_t dc_table_doubles(int N);               // host only: the size of the table below
void dc_table(int N, double* t);              // host only: the twiddles e^(-2 pi i k / N), k < N / 2, at their swizzled cells, then the window [N]
struct DeclipP {
    const float* wav; int L_max;              // [B, L_max]; samples at or beyond len[b] are never read
    const int* len; const int* need; const int* row0;      // device [B]; need: the count from which a side is clipped
    int B, T_cap;                             // T_cap >= max_b T_b: sizes the frame kernel's grid
    int N; float tol, level;                  // level NaN: detect
    int step, every, max_iter; double eps;
    const double* table;                      // dc_table(N), device
    int* det;                                 // [B, kDcDet]
    double* frames; int* it;                  // written for the utterances with a clipped side only, and read for those only
    int32_t* iters_out; int T_max;            // optional [B, T_max] (the caller zeroes it): the frames t < T_b of those utterances
    float* out; int Lout_max;                 // launch_dc_overlap: the samples j < len[b]; launch_dc_figures: NULL = detection only
    double* fig;                              // launch_dc_figures: [B, MT2_DECLIP_FIELDS]
};
hipError_t launch_dc_detect(const DeclipP& p, hipStream_t s);
hipError_t launch_dc_frames(const DeclipP& p, hipStream_t s);
hipError_t launch_dc_overlap(const DeclipP& p, int max_len, hipStream_t s);
hipError_t launch_dc_figures(const DeclipP& p, hipStream_t s);

// ---- Griffin-Lim vocoder (griffinlim.hip; the rule is in its header and in megatts2_hip.h) -------------------------------------------
// Frames of a ragged batch are packed rows: utterance b owns rows row0[b] .. row0[b] + T[b] of S / R / Rprev ([rows, lds]: re(0..F-1) |
// im(0..F-1) | zero pad, lds = 2F rounded up to 4), of A ([rows, lda]) and of the inverse-DFT GEMM's frames ([rows, N]).
// out[r, :] = expf(mel[rowmap[r], :]), C % 4 == 0
hipError_t launch_gl_exp_rows(const float* mel, int C, const int* rowmap, float* out, int R, hipStream_t s);
// S[r] = A[r] (cos, sin)(2 pi u), u the Philox draw of (seeds[2 b], seeds[2 b + 1]) at counter row_t[r] F + f, b = row_b[r]; A == nullptr: A = 1
hipError_t launch_gl_phase_init(const float* A, int lda, const int* row_b, const int* row_t, const uint32_t* seeds, float* S, int lds_,
                                int F, int R, hipStream_t s);
// the overlap-add (s / e, existing frames in ascending t; w2 [N] = the squared window) in gather form, written as the reflect-padded
// hop-block buffer of the STFT convolution (the layout of launch_reflect_pad_blocks: utterance b owns T[b] - 1 + N / hop blocks) ...
hipError_t launch_istft_ola_blocks(const float* frames, int N, int hop, const float* w2, const int* blk_b, const int* blk_t,
                                   const int* row0, const int* Tlen, float* out, int Rb, hipStream_t s);
// ... and as wav[b, n] for n < (T[b] - 1) hop, zeros up to L_max (L_max >= every length)
hipError_t launch_istft_ola_wav(const float* frames, int N, int hop, const float* w2, const int* row0, const int* Tlen, float* wav,
                                int L_max, int B, hipStream_t s);
// update != 0: D = R - c Rprev, S = D (A / (|D| + 1e-16)), Rprev = R.  resid != nullptr: resid[rmap[r]] = sum_f (|R[r, f]| - A[r, f])^2
hipError_t launch_gl_phase_update(const float* R, float* Rprev, const float* A, int lda, float* S, int lds_, int F, float c, float* resid,
                                  const int* rmap, int rows, int update, hipStream_t s);

// ---- F0 by YIN and the pitch moments (f0.hip; the rule is in its header and in megatts2_hip.h) ------------------------------------
// host only, no HIP call: tau_min = ceil(sr / fmax), tau_max = floor(sr / fmin); false where the rule refuses (non-finite or
// non-positive frequencies, or not 2 <= tau_min < tau_max <= MT2_F0_MAX_LAG)
bool f0_lags(int sample_rate, float fmin, float fmax, int* lag_min, int* lag_max);
// One launch over (frames, b) of a ragged batch, one workgroup per frame.  Frames in [T_b, T_max) are written as unvoiced.
struct F0P {
    const float* wav; int L_max;              // [B, L_max]; samples at or beyond len[b] are never read
    const int* len; int max_len, B;           // device [B]; max_b len[b]
    int sample_rate, hop, lag_min, lag_max;
    float threshold;
    float* f0; int T_max;                     // [B, T_max], T_max >= 1 + max_len / hop
    float* cmnd; int* lag;                    // optional [B, T_max]: d'[tau*], tau*
    float* diff;                              // optional [B, T_max, MT2_F0_MAX_LAG + 1]: d
};
hipError_t launch_f0_yin(const F0P& p, hipStream_t s);
// The second tracker (mt2_f0_track): a Viterbi pass over d'.  lg [256] (device): f0_track_table's; dprime [B, T_max, 257] and psi
// [B, T_max, 256] are scratch.  Two launches: d' of every frame (a workgroup per frame), then a workgroup per utterance for the
// recurrence, the backtrack and the refinement, in this order on one stream.  y.diff / y.cmnd / y.lag are optional as in launch_f0_yin.
struct F0TrackP {
    F0P y;
    float octave_cost, jump_cost;             // finite, >= 0
    const float* lg;
    float* dprime;
    unsigned char* psi;
};
// host only: lg[k] = (float)log2((double)(lag_min + k)) for lag_min + k <= lag_max, 0 behind; 256 entries
void f0_track_table(int lag_min, int lag_max, float* lg);
hipError_t launch_f0_cmnd(const F0TrackP& p, hipStream_t s);          // d' -> p.dprime; frames in [T_b, T_max) written as unvoiced
hipError_t launch_f0_viterbi(const F0TrackP& p, hipStream_t s);       // p.dprime -> f0, cmnd, lag of the frames below T_b
// stats[b, 0 .. 6) (double) = n, n / T_b, mean, sigma, skewness, excess kurtosis of f0[b, t] > 0 over t < frame_len[b]; a workgroup per utterance
hipError_t launch_f0_stats(const float* f0, const int* frame_len, int T_max, int B, double* stats, hipStream_t s);

// ---- formant candidates by linear prediction and the formant figures (formants.hip; the rule is in its header and in megatts2_hip.h) --
// host only, no HIP call: the window table w[0 .. W) in double and the pre-emphasis coefficient exp(-2 pi hz / sample_rate) (0 for hz = 0)
void formant_window_table(int W, int kind, double* table);
double formant_alpha(double preemphasis_hz, int sample_rate);
// One launch over (frames, utterances), a wave per frame; frames in [T_b, T_max) are written count 0, zeros, iters 0.
struct FormantP {
    const float* wav; int L_max;              // [B, L_max]; samples at or beyond len[b] are never read
    const int* len; int max_len, B;           // device [B]; max_b len[b]
    int sample_rate, hop, W, P;
    const double* window;                     // device [W]: formant_window_table
    double alpha, fmin, max_bw;
    float* freq; float* bw; int* count; int T_max;      // [B, T_max, 5], [B, T_max, 5], [B, T_max]
    double* lpc; double* err; double* autocorr; double* roots; int* iters;      // optional [B, T_max, P + 1], [B, T_max], [B, T_max, P + 1], [B, T_max, P, 2], [B, T_max]
};
hipError_t launch_formants(const FormantP& p, hipStream_t s);
// stats[b, 0 .. 12) (double) over the frames t < frame_len[b] with count >= 4 (and f0 > 0 where f0 is given); a workgroup per utterance
hipError_t launch_formant_stats(const float* freq, const int* count, const float* f0, const int* frame_len, int T_max, int B, double* stats,
                                hipStream_t s);

// ---- formant tracks across frames: Viterbi over the candidates (formant_track.hip; the rule is in its header and in megatts2_hip.h) --
// host only, no HIP call: C(5, K), and the increasing K-tuples of {0 .. 4} in lexicographic order, st[s][q] at st[5 s + q], zeros behind
int formant_track_states(int K);
void formant_track_table(int K, signed char* st /*[50]*/);
// One launch, a workgroup (one wave) per utterance; frames in [len[b], T_max) are written zeros, count 0, sel -1.
struct FormantTrackP {
    const float* freq; const float* bw; const int* count;      // [B, T_max, 5], [B, T_max, 5], [B, T_max]
    const int* len; int T_max, B, K, S;                         // device [B], each in [1, T_max]; S = formant_track_states(K)
    double ref[5]; double fc, bc, jc;                           // ref_hz, freq_cost, bw_cost, jump_cost
    signed char st[50];                                         // formant_track_table(K)
    unsigned char* psi;                                         // scratch [B, T_max, 16], 16-byte aligned
    float* tfreq; float* tbw; int* tcount; int* sel;            // [B, T_max, 5], [B, T_max, 5], [B, T_max], [B, T_max, 5] or null
};
hipError_t launch_formant_track(const FormantTrackP& p, hipStream_t s);

// ---- per-phone prosody (prosody.hip; the rules are in its header and in megatts2_hip.h) ---------------------------------------------
// energy[b, t] = the mean square of the F0 frame t of utterance b (a wave per frame); frames in [T_b, T_max) are written 0
struct EnergyP {
    const float* wav; int L_max;              // [B, L_max]; samples at or beyond len[b] are never read
    const int* len; int max_len, B;           // device [B]; max_b len[b]
    int hop;
    float* energy; int T_max;                 // [B, T_max], T_max >= 1 + max_len / hop
};
hipError_t launch_frame_energy(const EnergyP& p, hipStream_t s);
// out[b, p, 0 .. 8) (double, 16-byte aligned) of the phones p < np_len[b] over the frames below t_len[b]; zero rows up to Np_max.
// A workgroup per utterance.
struct PhoneProsodyP {
    const float* f0; const float* energy;     // [B, T_max]; energy optional
    int T_max;
    const int* dur; int Np_max;               // device [B, Np_max]; entries at or beyond np_len[b] are never read
    const int* np_len; const int* t_len;      // device [B]
    int B;
    double* out;                              // [B, Np_max, 8]
    long long* dur_sum;                       // optional [B]: the unclipped sum of max(dur, 0)
};
hipError_t launch_phone_prosody(const PhoneProsodyP& p, hipStream_t s);
// the voiced frames of f0 below t_len[b] compacted in order to st = 12 log2 f0 (- their mean with center); a workgroup per utterance
struct PitchContourP {
    const float* f0; int T_max;               // [B, T_max]
    const int* t_len; int B;                  // device [B]
    int center;
    float* st; int* n_voiced;                 // [B, T_max] (zeros in [n, T_max)); [B]
    int* index;                               // optional [B, T_max]: the frame of entry k, -1 in [n, T_max)
};
hipError_t launch_pitch_contour(const PitchContourP& p, hipStream_t s);

// ---- integrated loudness and loudness normalisation (loudness.hip; the rule is in its header and in megatts2_hip.h) ------------------
// host only, no HIP call: the rate the rule accepts (a multiple of 10 in [8000, 192000]); c[10] = b0 b1 b2 a1 a2 of the shelf, then of
// the high-pass; M[16] = A^h row-major, the zero-input state transition of one sub-block
bool loudness_rate_ok(int sample_rate);
void loudness_coeffs(int sample_rate, double* c);
void loudness_carry_matrix(const double* c, int h, double* M);
// Four launches on one stream in this order - zero-state chunks + peak -> carry -> sub-block sums -> blocks, gates, gain, stats - and
// a fifth, scale, for the normalising call.  The caller zeroes peak[] in front.
struct LoudnessP {
    const float* wav; int L_max;              // [B, L_max]; samples at or beyond len[b] are never read
    const int* len; int max_len, B;           // device [B]; max_b len[b]
    int h;                                    // sample_rate / 10: the sub-block, which is the chunk
    double c[10];                             // loudness_coeffs
    const int* M;                             // device, 16 doubles (8-byte aligned): loudness_carry_matrix
    double* state; double* sums; int NS;      // scratch [B, NS, 4] and [B, NS], NS >= max_len / h
    unsigned* peak;                           // scratch [B]: the bit pattern of max |x|
    float* gain;                              // [B] or nullptr (the measuring call: gain 1)
    double target_lufs, peak_ceiling;         // read only with gain
    float* out;                               // [B, L_max] for launch_loudness_scale; may be wav
    double* stats;                            // optional [B, 8]
    double* momentary; int NB_max;            // optional [B, NB_max], NB_max >= max_len / h - 3: l[k], -inf behind the utterance's blocks
};
hipError_t launch_loudness_filter(const LoudnessP& p, hipStream_t s);
hipError_t launch_loudness_carry(const LoudnessP& p, hipStream_t s);
hipError_t launch_loudness_sums(const LoudnessP& p, hipStream_t s);
hipError_t launch_loudness_gate(const LoudnessP& p, hipStream_t s);
hipError_t launch_loudness_scale(const LoudnessP& p, hipStream_t s);

// ---- true peak, short-term loudness and loudness range (ebu.hip; the rule is in its header and in megatts2_hip.h) --------------------
// host only, no HIP call: o = ceil(192000 / sample_rate); table [o][MT2_TP_TAPS] f32 (row 0 the unit sample)
int true_peak_oversample(int sample_rate);
void true_peak_table(int sample_rate, float* table);
// Two launches behind the four of LoudnessP on the same stream: launch_true_peak any time after tp[] is zeroed, launch_loudness_range
// behind both it and launch_loudness_gate (which wrote row8 with gain 1).  The normalising call then runs launch_loudness_scale on `gain`.
struct EbuP {
    const float* wav; int L_max;              // [B, L_max]; samples at or beyond len[b] are never read
    const int* len; int max_len, B;           // device [B]; max_b len[b]
    int h, o;                                 // sample_rate / 10; true_peak_oversample
    const float* table;                       // device [o][MT2_TP_TAPS]: true_peak_table
    unsigned* tp;                             // scratch [B], zeroed on the stream: the bit pattern of the true peak
    const double* sums; int NS;               // S[b, j] as launch_loudness_sums left it
    const double* row8;                       // [B, 8] as launch_loudness_gate left it
    double* keys; int NST;                    // scratch [B, NST], NST >= max_len / h - 29: z3, then the keys of the select
    float* gain;                              // [B] or nullptr (the measuring call)
    double target_lufs, ceiling_dbtp;         // read only with gain
    double* stats;                            // optional [B, MT2_EBU_FIELDS]
    double* short_term; int NST_max;          // optional [B, NST_max], NST_max >= max_len / h - 29: s[k], -inf behind the utterance's blocks
};
hipError_t launch_true_peak(const EbuP& p, hipStream_t s);
hipError_t launch_loudness_range(const EbuP& p, hipStream_t s);

// ---- true-peak look-ahead limiter (limiter.hip; the rule is in its header and in megatts2_hip.h) -------------------------------------
// host only, no HIP call: H = round(sample_rate window_ms / 1000), or -1 where the rule refuses the window; the 2 H + 1 weights
int limiter_half_window(int sample_rate, double window_ms);
void limiter_window(int H, float* w);
__host__ __device__ constexpr int limiter_window_words(int H) { return (2 * H + 1 + 3) & ~3; }      // the weights as the gain kernel reads them: zeros behind
// launch_limiter_envelope once a call, behind the upload of `table`; then per pass launch_limiter_step(kLimStepTrim) behind the true
// peak of the pass's output, launch_limiter_step(kLimStepNext) behind its loudness row; kLimStepInit in front of the first pass and
// kLimStepStats behind the last.  The words of a pass are zeroed on the stream in front of it.
enum { kLimStepInit = 0, kLimStepTrim = 1, kLimStepNext = 2, kLimStepStats = 3 };
struct LimiterP {
    const float* wav; int L_max;              // [B, L_max]; samples at or beyond len[b] are never read
    const int* len; int max_len, B;           // device [B]; max_b len[b]
    int o; const float* table;                // true_peak_oversample; device [o][MT2_TP_TAPS]
    int H; const float* win;                  // device [limiter_window_words(H)]: limiter_window, zeros behind
    float c;                                  // (f32) 10^(ceiling_dbtp / 20)
    float* env; int E_ld;                     // scratch [B, E_ld], E_ld >= max_len, a multiple of 4: E[i]
    float* G; int* bypass; float* t;          // device [B] each: the pass's pre-gain; 1 = copied unchanged; the trim
    float* out; int out_ld;                   // the pass's output [B, out_ld]; may be wav (out_ld == L_max then)
    float* gain; float* need;                 // optional [B, out_ld]: s and need of this pass, 1 behind len[b]
    unsigned* minkey; unsigned* count;        // [B] each, zeroed: the inverted key of min s; samples with s < 1
    const unsigned* tp;                       // [B]: the true peak of the pass's output before the trim
    // launch_limiter_step
    int normalizing; float G_host;            // kLimStepInit: G from row18's I and target_lufs, or G_host
    double target_lufs;
    const double* row18;                      // [B, MT2_EBU_FIELDS] of the input as launch_loudness_range left it
    const double* rowk;                       // [B, 8] of the pass's output as launch_loudness_gate left it (kLimStepNext; kLimStepStats: or nullptr)
    double* stats;                            // [B, MT2_LIMITER_FIELDS] (kLimStepStats)
};
hipError_t launch_limiter_envelope(const LimiterP& p, hipStream_t s);
hipError_t launch_limiter_gain(const LimiterP& p, hipStream_t s);
hipError_t launch_limiter_step(const LimiterP& p, int step, hipStream_t s);

}  // namespace mt2
