// Front door of the GEMM engine (host only): the index -> tile table, the tile choice, gemm_route (what launch_gemm will do
// with a launch, decided without a HIP call), launch_gemm itself and the launch trace.  The tiles are described where their
// kernels are (gemm_tiles.h: gemm_f32.hip, gemm_x3h.hip); the <= 64-row weight-streaming kernels live in gemm_skinny.hip.
#include "gemm_tiles.h"

#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <utility>
#include <vector>

namespace mt2 {

// ---------------------------------------------------------------------------------------------------
// the table: every index below kNumCfgs is either a live row of one of the kernel units or a retired name

// names only: the weight-streaming kernels for M <= 64 rows (gemm_skinny.hip; gemm_route sends launches there)
static const TileCfg kSkinnyRows[] = {
    { CFG_SKINNY32, 32, 32, 512, 0, "skinny32_f32", {} },
    { CFG_SKINNY64, 64, 32, 512, 0, "skinny64_f32", {} },
    { CFG_SKINNYTM32, 32, 32, 512, 0, "skinnytm32_f32", {} },      // the same on tile-major weights
    { CFG_SKINNYTM64, 64, 32, 512, 0, "skinnytm64_f32", {} },      //   (+ LayerNorm prologue)
};
// Configurations that were measured, documented (profiles/) and are no longer built: the index keeps its
// meaning in the profiles of earlier rounds, launch_gemm answers hipErrorNotSupported
static const struct { int index; const char* name; } kRetired[] = {
    {0, "retired:128x128_2x2"}, {1, "retired:64x128_2x2"}, {2, "retired:128x64_2x2"}, {4, "retired:32x128_1x4"},
    {5, "retired:32x64_1x2"}, {6, "retired:128x32_4x1"}, {7, "retired:64x32_2x1"},
    {8, "retired:dma128x128_2x2_s3"}, {9, "retired:dma128x128_2x2_s4"}, {10, "retired:dma64x128_2x2_s4"},
    {11, "retired:dma64x64_2x2_s4"}, {13, "retired:dma32x128_1x4_s4"}, {14, "retired:dma32x64_1x2_s4"},
    {19, "retired:dma64x64_2x2_k2_s4"}, {21, "retired:dma32x64_1x2_k4_s3"}, {24, "retired:dma128x64_4x2_s4"},
    {25, "retired:dma128x64_4x2_s2"}, {26, "retired:dma64x64_2x2_k1_s2"}, {27, "retired:dma128x64_4x2_k2_s2"},
    {29, "retired:dma32x32_1x1_k4_s3"}, {33, "retired:win128x64_4x2_s3"},
    {35, "retired:x6win256x64_8x1_s3"}, {36, "retired:x6win128x128_4x2_s2"},
    // x6 with both operands through the ring, self-refilling (37-44); with the A operand through registers (45-50)
    {37, "retired:x6dma256x128_4x2_s2"}, {38, "retired:x6dma128x128_4x2_s3"}, {39, "retired:x6dma128x128_4x2_s2"},
    {40, "retired:x6dma128x256_2x4_s2"}, {41, "retired:x6dma256x128_8x2_s2"}, {42, "retired:x6dma256x128_8x1_s2"},
    {43, "retired:x6dma128x128_4x1_s2"}, {44, "retired:x6dma128x256_4x1_s2"},
    {45, "retired:x6areg256x128_8x1_s3"}, {46, "retired:x6areg256x128_4x2_s3"}, {47, "retired:x6areg128x128_4x2_s3"},
    {48, "retired:x6areg128x128_4x1_s3"}, {49, "retired:x6areg64x128_2x2_s3"}, {50, "retired:x6areg128x256_4x2_s2"},
    // loader-wave forms: other loader counts and ring depths, cross-chunk prefetch (56, 57), de-phased groups (62), small tiles (63-66)
    {52, "retired:x6ldr256x128_4x2+2_s2"}, {53, "retired:x6ldr128x128_4x2+4_s2"}, {54, "retired:x6ldr128x128_4x2+2_s2"},
    {56, "retired:x6ldrx128x128_4x2+4_s3"}, {57, "retired:x6ldrx128x128_4x2+2_s3"},
    {60, "retired:x6winl128x128_4x2+2_s2"}, {61, "retired:x6winl256x64_8x1+2_s3"}, {62, "retired:x6ldrd128x128_4x2+4_s3"},
    {63, "retired:x6ldr64x128_2x4+4_s3"}, {64, "retired:x6ldr128x64_4x2+4_s3"}, {65, "retired:x6ldr64x128_2x4+2_s3"},
    {66, "retired:x6ldr128x64_4x2+2_s3"},
    // mid-chunk barrier (67-73; 72-74: one compute wave per SIMD), free-running compute waves on LDS counters (75-78)
    {67, "retired:x6ldm128x128_4x2+4_s3"}, {68, "retired:x6ldm256x128_4x2+4_s2"}, {69, "retired:x6ldm128x64_4x2+4_s3"},
    {70, "retired:x6ldm64x128_2x4+4_s3"}, {71, "retired:x6ldm128x128_4x2+4_s2"}, {72, "retired:x6ldm128x128_2x2+4_s3"},
    {73, "retired:x6ldm128x128_2x2+2_s3"}, {74, "retired:x6ldr128x128_2x2+4_s3"},
    {75, "retired:x6ldf128x128_4x2+4_s3"}, {76, "retired:x6ldf256x128_4x2+4_s2"}, {77, "retired:x6ldf128x64_4x2+4_s3"},
    {78, "retired:x6ldf128x128_4x2+2_s3"},
    // x6 K-split tiles with four / two loader waves (84-86 have eight)
    {79, "retired:x6ks32x64_1x2_k4+4_s2"}, {80, "retired:x6ks64x64_2x2_k2+4_s3"}, {81, "retired:x6ks32x64_1x2_k4+2_s2"},
    {82, "retired:x6ks32x32_1x1_k8+4_s2"}, {83, "retired:x6ks64x64_2x2_k2+4_s2"},
    // x3h loader tile: one barrier per chunk (91-94), one per 64-deep super-chunk (101, 102), other cross-chunk forms (104, 105)
    {91, "retired:x3hldr128x128_4x2+4_s3"}, {92, "retired:x3hldr128x128_4x2+4_s4"}, {93, "retired:x3hldr128x128_2x2+4_s3"},
    {94, "retired:x3hldr128x128_2x2+4_s4"}, {101, "retired:x3hldr128x128_4x2+4_s4c2"}, {102, "retired:x3hldr128x128_2x2+4_s4c2"},
    {104, "retired:x3hldr128x128_4x2+4_s3xc"}, {105, "retired:x3hldr128x128_2x2+4_s4xc"},
};

// Built at first use: every live row at the index its CFG_ constant says, every other index a retired name - a row without a
// place, two claims on one index or an index without a name end the process there and then.
struct CfgTable {
    const TileCfg* row[kNumCfgs] = {};      // nullptr: retired
    const char* name[kNumCfgs] = {};
    CfgTable() {
        const auto claim = [this](int i, const char* nm) {
            if (i < 0 || i >= kNumCfgs || name[i]) {
                std::fprintf(stderr, "gemm tile table: index %d of '%s' is %s\n", i, nm, i < 0 || i >= kNumCfgs ? "outside the table" : name[i]);
                std::abort();
            }
            name[i] = nm;
        };
        for (const TileRows t : {gemm_f32_tile_rows(), gemm_x3h_tile_rows(), TileRows{kSkinnyRows, 4}})
            for (int k = 0; k < t.n; ++k) { claim(t.rows[k].index, t.rows[k].name); row[t.rows[k].index] = &t.rows[k]; }
        for (const auto& r : kRetired) claim(r.index, r.name);
        for (int i = 0; i < kNumCfgs; ++i)
            if (!name[i]) { std::fprintf(stderr, "gemm tile table: index %d has neither a row nor a retired name\n", i); std::abort(); }
    }
};
static const CfgTable& cfg_table() {
    static const CfgTable t;
    return t;
}

int gemm_num_configs() { return kNumCfgs; }
const char* gemm_config_name(int idx) { return idx >= 0 && idx < kNumCfgs ? cfg_table().name[idx] : ""; }

// The same tile on the next pipe, as data: what the chooser moves a choice to when the weights come with planes
struct CfgPair { int from, to; };
static const CfgPair kX6Form[] = {          // f32 tile -> its bf16-pipe (6 products) form
    {CFG_WIN256x32, CFG_X6WIN256x32}, {CFG_WIN256x64, CFG_X6WINL256x64}, {CFG_WIN128x128, CFG_X6WINL128x128},
    {CFG_DMA32x64_K4, CFG_X6KS32x64_K4}, {CFG_DMA64x64_K4, CFG_X6KS64x64_K2}, {CFG_DMA64x64_K2, CFG_X6KS64x64_K2},
    {CFG_DMA32x32_K8, CFG_X6KS32x32_K8},
};
static const CfgPair kX3hForm[] = {         // x6 tile -> its fp16-pipe (3 products) form
    {CFG_X6WIN256x32, CFG_X3HWIN256x32}, {CFG_X6WINL256x64, CFG_X3HWIN256x64}, {CFG_X6WINL128x128, CFG_X3HWIN128x128},
    {CFG_X6LDR256x128, CFG_X3HLDR128x128}, {CFG_X6LDR128x128, CFG_X3HLDR128x128},
    {CFG_X6KS32x64_K4, CFG_X3HKS32x64_K4}, {CFG_X6KS64x64_K2, CFG_X3HKS64x64_K2}, {CFG_X6KS32x32_K8, CFG_X3HKS32x32_K8},
};
template <int N>
static int paired(const CfgPair (&t)[N], int cfg) {
    for (const CfgPair& e : t)
        if (e.from == cfg) return e.to;
    return cfg;
}

// ---------------------------------------------------------------------------------------------------
// launch trace (measurement only): HIP events around every GEMM launch, on the launch stream; the records
// live in the EngineOpts of whoever asked for the trace (the model handle).

int gemm_trace_shapes(EngineOpts& o, char* buf, int cap, int top) {
    struct Agg { int cfg, M, N, K, g; long long n; double ms, fl; };
    std::vector<Agg> v;
    for (auto& r : o.trace) {
        float dt = 0.f;
        if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&dt, r.e0, r.e1) != hipSuccess) return -1;
        bool found = false;
        for (auto& a : v)
            if (a.cfg == r.cfg && a.M == r.M && a.N == r.N && a.K == r.K && a.g == r.groups) {
                ++a.n; a.ms += dt; a.fl += r.flops; found = true;
                break;
            }
        if (!found) v.push_back({r.cfg, r.M, r.N, r.K, r.groups, 1, (double)dt, r.flops});
    }
    std::sort(v.begin(), v.end(), [](const Agg& a, const Agg& b) { return a.ms > b.ms; });
    int off = 0;
    for (int i = 0; i < (int)v.size() && i < top; ++i) {
        const Agg& a = v[i];
        const int w = snprintf(buf + off, cap - off, "%s %d %d %d %d %lld %.3f %.2f\n", gemm_config_name(a.cfg), a.M, a.N, a.K, a.g,
                               a.n, a.ms, a.fl / (a.ms > 0 ? a.ms : 1e-9) / 1e9);
        if (w < 0 || w >= cap - off) break;
        off += w;
    }
    return off;
}

// Per tile configuration: launches, executed FLOPs (2*M*N*K*groups) and summed kernel time (ms).  When the
// launches ran on several streams (AR stream groups) their intervals overlap; a last pseudo-entry named
// "union" carries the length of the UNION of all launch intervals (= time during which at least one engine
// kernel was running), the right denominator for a whole-engine throughput.
int gemm_trace_collect(EngineOpts& o, int cap, const char** names, int64_t* launches, double* flops, double* ms) {
    o.trace_on = false;
    auto& tr = o.trace;
    int n = 0;
    std::vector<std::pair<double, double>> iv;
    double fl_all = 0.0;
    bool ok = true;
    for (int i = 0; i < kNumCfgs && n < cap && ok; ++i) {
        int64_t cnt = 0;
        double fl = 0.0, t = 0.0;
        for (auto& r : tr) {
            if (r.cfg != i) continue;
            float dt = 0.f, t0 = 0.f;
            if (hipEventSynchronize(r.e1) != hipSuccess || hipEventElapsedTime(&dt, r.e0, r.e1) != hipSuccess ||
                hipEventElapsedTime(&t0, tr.front().e0, r.e0) != hipSuccess) { ok = false; break; }
            iv.emplace_back((double)t0, (double)t0 + dt);
            ++cnt; fl += r.flops; t += dt;
        }
        if (cnt == 0) continue;
        names[n] = gemm_config_name(i); launches[n] = cnt; flops[n] = fl; ms[n] = t;
        fl_all += fl;
        ++n;
    }
    if (ok && n < cap && !iv.empty()) {
        std::sort(iv.begin(), iv.end());
        double uni = 0.0, lo = iv[0].first, hi = iv[0].second;
        for (auto& x : iv) {
            if (x.first > hi) { uni += hi - lo; lo = x.first; hi = x.second; }
            else if (x.second > hi) hi = x.second;
        }
        uni += hi - lo;
        names[n] = "union"; launches[n] = (int64_t)iv.size(); flops[n] = fl_all; ms[n] = uni;
        ++n;
    }
    for (auto& r : tr) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    tr.clear();
    return ok ? n : -1;
}

// `launch()` between two events on the launch stream when the trace is on, plain otherwise
template <typename F>
static hipError_t traced_launch(EngineOpts* opts, int cfg, const GemmP& p, hipStream_t s, F&& launch) {
    if (opts) opts->last_cfg = gemm_config_name(cfg);
    if (!(opts && opts->trace_on)) return launch();
    TraceRec r;
    r.cfg = cfg;
    r.flops = 2.0 * p.M * p.N * p.K * p.groups;
    r.M = p.M; r.N = p.N; r.K = p.K; r.groups = p.groups;
    if (hipEventCreate(&r.e0) != hipSuccess || hipEventCreate(&r.e1) != hipSuccess) return hipErrorUnknown;
    (void)hipEventRecord(r.e0, s);
    const hipError_t e = launch();
    (void)hipEventRecord(r.e1, s);
    opts->trace.push_back(r);
    return e;
}

// ---------------------------------------------------------------------------------------------------
// Tile choice, from tools/gemm_sweep.py on MI355X (profiles/r01_gemm_sweep_v3.txt).  Two regimes:
//   * operand ingest: a CU sustains ~20 GB/s of global->LDS DMA however many workgroups it hosts, so a
//     tile costs about (bm + bn) * K * 4 B / 20 GB/s; 64x64 tiles (16 FLOP per operand byte) are ingest-bound
//     at ~85 TFLOP/s but fill the chip earliest - they win for every GEMM of the autoregressive steps
//     (M <= ~2200 rows);
//   * matrix issue: big tiles (32-43 FLOP/B) need >= 2 waves per SIMD to keep the MFMA pipe busy across the
//     per-chunk barrier: the 8-wave 256x128 / 128x128 tiles reach 95-106 TFLOP/s once there are enough of
//     them to load every CU (conv stacks, vocoder).
//   * chain / fill (AR steps): a launch with fewer 64x64 tiles than the chip has CUs leaves one workgroup per
//     CU at best, and a 4-wave tile then runs at the pace of ONE wave per SIMD: serial chain K/2 x 64 cycles
//     plus an exposed barrier + DMA-issue + ds_read bubble per chunk (measured ~1 us per 32-wide chunk vs
//     0.43 us of MFMA).  The K-split tiles put 2-4 waves on each SIMD of the same CU instead.
// (the thresholds, in tiles, are EngineOpts::t_ks4 / t_ks2 / t32 / t32x32)

// A CU retires one 64x64 tile of K=768 in ~12 us whatever the launch looks like, so for the AR-step shapes the
// choice is about how many CUs get a tile and how many tiles the busiest CU gets (profiles/r01_gemm_sweep_ar_*):
//   32x64 K-split tiles while they fit one per CU; 64x64 K-split tiles while THEY fit one (k4) / two (k2) per CU;
//   a big 8-wave tile when its tile count just fills the chip once (200..256); otherwise plain 64x64 tiles
//   (three workgroups per CU, de-phased) and the 8-wave tiles for the conv stacks and the vocoder.
// window convolution: plain "same" conv over contiguous rows, square, narrow (see conv_win_f32_kernel)
static bool win_eligible(const GemmP& p) {
    return p.taps >= 2 && !p.rowbase && p.a_mul == 1 && p.groups == 1 && p.N == p.Cin &&
           (p.Cin == 32 || p.Cin == 64 || p.Cin == 128) && (p.taps - 1) * p.dil <= 64 && p.pro_act < PRO_LN;
}
static int choose_cfg(const GemmP& p, const EngineOpts& o) {
    const bool forced = o.force_cfg >= 0 && o.force_cfg < kNumCfgs;
    const bool x3h_ok = p.Wh && p.wh_inv;
    if (o.win_conv && win_eligible(p) && !forced) {
        int bi = p.Cin == 32 ? CFG_WIN256x32 : (p.Cin == 64 ? CFG_WIN256x64 : CFG_WIN128x128);
        if (o.x6_conv && p.W3) {
            // the bf16-pipe forms: x6win256x32 (32 channels), and with loader waves x6winl256x64 / x6winl128x128 (64 / 128 channels:
            // +5..14 % / +2..6 % over the self-refilling forms 35 / 36, retired in round 6)
            bi = paired(kX6Form, bi);
            // the fp16-pipe forms of the 64- and 128-channel tiles (profiles/r06_gemm_sweep_x3hwin_v1.txt: +19..37 % and +35..40 %, and
            // +11..18 % more with the cross-chunk pipeline, _v3_cross_chunk.txt, +10..35 % more with the window converted to fp16
            // planes once per tile, _v4_planes_in_lds.txt).  The 32-channel convolutions too since then: 94 vs 72 TF/s with 3 taps,
            // 221 vs 123 with 11 (the first x3h build of that tile was 3..19 % SLOWER than x6)
            if ((o.x3h & 4) && x3h_ok) bi = paired(kX3hForm, bi);
        }
        return bi;
    }
    if (forced) return o.force_cfg;
    const long long t32 = (long long)((p.M + 31) / 32) * ((p.N + 63) / 64) * p.groups;
    const long long t32x32 = (long long)((p.M + 31) / 32) * ((p.N + 31) / 32) * p.groups;
    const long long t64 = (long long)((p.M + 63) / 64) * ((p.N + 63) / 64) * p.groups;
    const long long t128 = (long long)((p.M + 127) / 128) * ((p.N + 127) / 128) * p.groups;
    const long long t256 = (long long)((p.M + 255) / 256) * ((p.N + 127) / 128) * p.groups;
    int bi = CFG_DMA64x64_S3;
    if (p.N <= 32) bi = CFG_DMA128x32_S4;
    else if (p.N <= 64 && t128 >= 400) bi = CFG_DMA256x64_S3;
    else if (p.N <= 256 && t128 >= 400) bi = CFG_DMA128x128_S4;                   // two n-tiles: 128x128 beats 256x128 (vocoder)
    else if (t256 >= 400 || (t256 >= 200 && t256 <= 256)) bi = CFG_DMA256x128_S3;
    else if (t128 >= 400 || (t128 >= 200 && t128 <= 256)) bi = CFG_DMA128x128_S4;
    else if (t32x32 <= o.t32x32 && p.K >= 512) bi = CFG_DMA32x32_K8;
    else if (t32 <= o.t32) bi = CFG_DMA32x64_K4;
    else if (t64 <= o.t_ks4) bi = CFG_DMA64x64_K4;
    else if (t64 <= o.t_ks2) bi = CFG_DMA64x64_K2;
    // Launches whose weights come with planes leave the f32 MFMA for the 16-bit matrix pipe in an f32-equivalent form: the
    // loader-wave tiles (256x128 from t_x6_256 tiles on, 128x128 from t_x6_128 / t_x3h_128 on - conv stacks, vocoder stage 1, the
    // PLM / ADM QKV and ff.0 at full batch) and, below that, the K-split tiles of the AR steps (out-projection, ff.3, early steps).
    if (o.x6_gemm && p.W3 && (p.K & 7) == 0 && (p.ldw & 7) == 0 && (p.pro_act < PRO_LN || p.pro_act == PRO_LNX) && p.N > 64) {
        const bool h1 = (o.x3h & 1) && x3h_ok;      // the 128x128 tile will run in its x3h form: its own crossover against the K-split tiles
        if (t256 >= o.t_x6_256) bi = CFG_X6LDR256x128;
        else if (t128 >= (h1 ? o.t_x3h_128 : o.t_x6_128)) bi = CFG_X6LDR128x128;
        // K-split tiles on the bf16 pipe, eight loader waves (x6_ks: 0 off; 1, 3: the 32x64 k4 and 64x64 k2 tiles; 2, 4: + the 32x32
        // k8 tile; 5: the 64x64 tile only)
        if (o.x6_ks && p.taps == 1) {
            if (bi == CFG_DMA32x64_K4 && p.K % (BK * 4) == 0 && o.x6_ks != 5) bi = paired(kX6Form, bi);
            else if ((bi == CFG_DMA64x64_K4 || bi == CFG_DMA64x64_K2) && p.K % (BK * 2) == 0) bi = paired(kX6Form, bi);
            else if ((o.x6_ks == 2 || o.x6_ks == 4) && bi == CFG_DMA32x32_K8 && p.K % (BK * 8) == 0) bi = paired(kX6Form, bi);
        }
    }
    // the fp16-pipe form of the tile (three products instead of six) where one exists and the weights come with fp16 planes
    // (profiles/r06_gemm_sweep_x3h_v1_gate.txt: the 128x128 x3h tile beats BOTH x6 loader tiles on every shape of the model - 199 vs
    // 146 TF/s at 864x4096x1024, 245 vs 188 at 4096^3 on the first build; 243 and 297 with the cross-chunk pipeline and the loaders
    // on buffer loads, profiles/r06_gemm_sweep_x3hxc_v2_buffer_loads.txt)
    if ((o.x3h & 1) && x3h_ok && (bi == CFG_X6LDR128x128 || bi == CFG_X6LDR256x128)) bi = paired(kX3hForm, bi);
    // the x6 K-split tiles -> their x3h forms (profiles/r06_gemm_sweep_x3hk_v1.txt: +13..20 %, +25..50 %, +20..30 % per launch)
    if ((o.x3h & 2) && x3h_ok && cfg_table().row[bi]->pipe == PIPE_X6 && cfg_table().row[bi]->x6_ks) bi = paired(kX3hForm, bi);
    return bi;
}

// ---------------------------------------------------------------------------------------------------
// routing

// may the A operand arrive as fp16 planes (GemmP::a_planes)?  x3h loader / K-split tiles, no prologue, whole 128-byte blocks
// (`stat`: the launch writes row statistics)
static bool a_planes_ok(const GemmP& p, const TileCfg& c, bool stat) {
    return c.pipe == PIPE_X3H && !c.win_qs && p.pro_act == ACT_NONE && !stat && (p.Cin % BK) == 0 && (p.ldx % BK) == 0 &&
           !(p.groups > 1 && (p.strideX % BK) != 0) && p.a_mul == 1 && !p.rowbase && !(((unsigned long long)p.X) & 127);
}
// C as fp16 planes (GemmP::c_planes): the x3h loader tile's 16-byte-store epilogue, whole 128-byte blocks per row, one group
static bool c_planes_ok(const GemmP& p, const TileCfg& c, bool stat) {
    return c.pipe == PIPE_X3H && !c.x6_ks && !c.win_qs && p.groups == 1 && !p.R && !stat && (p.N & 31) == 0 && (p.ldc & 31) == 0 &&
           (((unsigned long long)p.C) & 127) == 0 && (((unsigned long long)p.bias) & 15) == 0 && ((p.strideC | p.strideB) & 3) == 0 && p.Wh && p.wh_inv && p.M > 64;
}
// x3h planes: chunk-interleaved rows, K padded to whole chunks; the group stride is exact for whole-chunk rows (attach_planes sets it otherwise)
static long long wh_ldb_of(const GemmP& p) { return p.wh_ldb ? p.wh_ldb : 4ll * ((p.ldw + 31) / 32 * 32); }
static long long wh_gstride_of(const GemmP& p) { return p.groups > 1 && p.wh_gstride == 0 ? p.strideW * 4 : p.wh_gstride; }

GemmRoute gemm_route(const GemmP& p, const EngineOpts& o) {
    GemmRoute r{hipSuccess, -1, V_NONE, 0, 0, 0};
    const auto fail = [&r](hipError_t e) { r.err = e; r.lds = 0; r.stat_nt = r.stat_w = 0; r.ks_epi4 = 0; return r; };
    if (p.M <= 0 || p.N <= 0 || p.groups <= 0) return r;        // nothing to launch
    if ((p.Cin & 3) || (p.ldx & 3) || (p.ldw & 3) || p.K != p.taps * p.Cin) return fail(hipErrorInvalidValue);
    if (p.pro_act < 0 || p.pro_act > PRO_LNX) return fail(hipErrorInvalidValue);
    if (p.c_planes && p.M <= 64) return fail(hipErrorNotSupported);      // (the <= 64-row kernels write f32)
    if (p.pro_act == PRO_LNX && (p.taps != 1 || p.groups != 1 || !p.ln_g || !p.ln_stat || p.ln_nt < 2 || p.ln_nt > 32 ||
                                 (p.ln_nt & 1) || p.ln_w <= 0 || p.ln_nt * p.ln_w != p.K || (((unsigned long long)p.ln_stat) & 15)))
        return fail(hipErrorInvalidValue);
    // a handful of rows: the weight-streaming kernel (gemm_skinny.hip) instead of a tile configuration
    const bool sk_forced = o.force_cfg == CFG_SKINNY32 || o.force_cfg == CFG_SKINNY64;
    const bool tm_forced = o.force_cfg == CFG_SKINNYTM32 || o.force_cfg == CFG_SKINNYTM64;
    if (tm_forced || (!p.a_planes && o.skinny_tm && o.skinny_rows > 0 && o.force_cfg < 0 &&
                      gemm_skinny_tm_eligible(p, o.skinny_rows))) {
        if (!gemm_skinny_tm_eligible(p, 64)) return fail(hipErrorInvalidValue);
        r.cfg = p.M <= 32 ? CFG_SKINNYTM32 : CFG_SKINNYTM64;
        if (p.stat_out) {       // row statistics as pairs per 16-column block (gemm_skinny_tm_kernel's epilogue): N / 16 <= 64 pairs per row
            const int nt = p.N / 16;
            if (p.groups == 1 && (nt & 1) == 0 && nt <= 64 && ((((unsigned long long)p.stat_out) & 15) == 0)) { r.stat_nt = nt; r.stat_w = 16; }
        }
        return r;
    }
    if (sk_forced || (o.skinny_rows > 0 && o.force_cfg < 0 && gemm_skinny_eligible(p, o.skinny_rows))) {
        if (!gemm_skinny_eligible(p, 64)) return fail(hipErrorInvalidValue);
        r.cfg = p.M <= 32 ? CFG_SKINNY32 : CFG_SKINNY64;
        return r;
    }
    r.cfg = choose_cfg(p, o);
    const TileCfg* c = cfg_table().row[r.cfg];
    if (!c) return fail(hipErrorNotSupported);                  // retired configuration
    const bool x3h = c->pipe == PIPE_X3H, x3h_ldr = x3h && !c->x6_ks && !c->win_qs;
    const bool has_lnx = c->stat_w && c->fn[V_LNX];
    if (p.pro_act == PRO_LNX && !has_lnx) return fail(hipErrorNotSupported);      // callers fall back to LayerNorm + GEMM
    bool stat = p.stat_out != nullptr;
    // the x3h loader tile writes through the 16-byte-store epilogue only in its pair-statistics variant: columns in fours, 16-byte bases
    if (x3h_ldr && (p.pro_act == PRO_LNX || stat)) {
        const bool t4 = ((p.N | p.ldc | (p.R ? p.ldr : 0)) & 3) == 0 && ((p.strideC | p.strideR | p.strideB) & 3) == 0 &&
                        (((unsigned long long)p.C | (unsigned long long)p.R | (unsigned long long)p.bias) & 15) == 0;
        if (!t4) {
            if (p.pro_act == PRO_LNX) return fail(hipErrorNotSupported);
            stat = false;
        }
    }
    if (stat) {             // row-statistics epilogue where the chosen tile has one; otherwise the launch simply writes none
        const int nt = c->stat_w ? p.N / c->stat_w : 0;
        stat = has_lnx && (p.pro_act == ACT_NONE || p.pro_act == PRO_LNX) && p.groups == 1 && p.N % c->stat_w == 0 && nt >= 2 &&
               nt <= 32 && (nt & 1) == 0 && ((((unsigned long long)p.stat_out) & 15) == 0);
        if (stat) { r.stat_w = c->stat_w; r.stat_nt = nt; }
    }
    if (p.a_planes && !a_planes_ok(p, *c, stat)) return fail(hipErrorNotSupported);
    if (p.c_planes && !c_planes_ok(p, *c, stat)) return fail(hipErrorNotSupported);
    // LayerNorm as a prologue of the f32 tiles (pro_act 3 / 4: rounds 1-2, measured slower than LayerNorm + GEMM) is retired: callers
    // fall back on NotSupported; the <= 64-row weight-streaming kernel (above) keeps its own LayerNorm prologue
    if (p.pro_act == PRO_LN || p.pro_act == PRO_LNA) return fail(hipErrorNotSupported);
    // pair statistics (consumer and / or producer side) run the V_LNX instantiation - the K loop of V_NONE
    r.variant = p.a_planes ? V_APLANES : ((p.pro_act == PRO_LNX || stat) ? V_LNX : (GemmVariant)p.pro_act);
    r.lds = c->lds;
    // pair-fed LayerNorm on the loader-wave tiles: + row statistics [BM][2] behind the ring.  The V_LNX instantiation also serves
    // stat_out-only producers: the same size for both, so that the cached MaxDynamicSharedMemorySize attribute covers either use
    if (r.variant == V_LNX && !c->x6_ks) r.lds += (size_t)c->bm * 2 * sizeof(float);
    if (x3h) {
        if (!p.Wh || !p.wh_inv || (p.K & 7) || (p.ldw & 7)) return fail(hipErrorInvalidValue);
        if ((((unsigned long long)p.Wh) & 127) || (wh_ldb_of(p) & 127) || (wh_gstride_of(p) & 127)) return fail(hipErrorInvalidValue);
    } else if (c->pipe == PIPE_X6 && (!p.W3 || (p.K & 7) || (p.ldw & 7))) return fail(hipErrorInvalidValue);
    if (c->x6_ks && (p.taps != 1 || p.K % (BK * c->x6_ks) != 0)) return fail(hipErrorInvalidValue);
    if (c->win_qs) {
        if (!win_eligible(p) || p.Cin != 32 * c->win_qs) return fail(hipErrorInvalidValue);
        const int wrp = (c->bm + (p.taps - 1) * p.dil + 7) & ~7;
        r.lds = c->lds + (size_t)c->win_qs * wrp * BK * sizeof(float);
    }
    if (!c->fn[r.variant]) return fail(hipErrorNotSupported);   // no variant for this prologue
    // the x3h K-split tiles finish row-major on 16 bytes (gemm_x3h_ks_kernel, EPI4) where every access of that finish is aligned: columns
    // in fours, rows and - in grouped launches - groups a multiple of four floats apart, every operand it reads as a float4 on 16 bytes
    if (o.ks_epi4 && x3h && c->x6_ks && c->fn4[r.variant]) {
        const auto on16 = [](const void* q) { return (((unsigned long long)q) & 15) == 0; };
        const bool grp4 = p.groups == 1 || ((p.strideC | (p.R ? p.strideR : 0) | (p.bias ? p.strideB : 0) | p.wh_inv_stride) & 3) == 0;
        r.ks_epi4 = ((p.N | p.ldc | (p.R ? p.ldr : 0)) & 3) == 0 && grp4 && on16(p.C) && on16(p.R) && on16(p.bias) && on16(p.wh_inv) &&
                    (p.pro_act != PRO_LNX || on16(p.ln_g));
    }
    return r;
}

// the defaults launch_gemm's callers may leave to it, for the questions about a launch not yet made
static GemmP normalise(GemmP p) {
    if (p.taps <= 0) p.taps = 1;
    if (p.groups <= 0) p.groups = 1;
    if (p.a_mul == 0) p.a_mul = 1;
    p.K = p.taps * p.Cin;
    if (p.ldw == 0) p.ldw = p.K;
    return p;
}
// The two questions the model asks about a launch it has not made yet.  They look at the tile choose_cfg picks and at the predicate
// gemm_route applies to that operand, nothing else: a launch that gemm_route rejects for another reason gets the answer it always got.
bool gemm_takes_planes(const GemmP& p_in, const EngineOpts& o) {
    const GemmP p = normalise(p_in);
    if (!(o.x3h & 3) || o.force_cfg >= 0 || p.M <= 64 || !p.Wh || !p.wh_inv) return false;
    const TileCfg* c = cfg_table().row[choose_cfg(p, o)];
    return a_planes_ok(p, *c, p.stat_out != nullptr) && c->fn[V_APLANES] != nullptr;
}
bool gemm_writes_planes(const GemmP& p_in, const EngineOpts& o) {
    const GemmP p = normalise(p_in);
    if (!(o.x3h & 1) || o.force_cfg >= 0 || p.M <= 64) return false;
    return c_planes_ok(p, *cfg_table().row[choose_cfg(p, o)], p.stat_out != nullptr);
}

// hipFuncSetAttribute(MaxDynamicSharedMemorySize) is per-DEVICE state of the code object: a "done" mask per (configuration,
// variant) with one bit per device only saves the call; the benign race (two threads setting the same value) is harmless.
static std::atomic<unsigned long long> g_attr_done[kNumCfgs][2 * kGemmVariants];   // bit per device (dyn_lds_once); [kGemmVariants ..): TileCfg::fn4

hipError_t launch_gemm(const GemmP& p_in, hipStream_t s, EngineOpts* opts) {
    static const EngineOpts kDefaults;
    const EngineOpts& o = opts ? *opts : kDefaults;
    const GemmRoute r = gemm_route(p_in, o);
    if (r.cfg < 0 && r.err == hipSuccess) return hipSuccess;    // nothing to launch
    if (opts) { opts->last_stat_nt = r.stat_nt; opts->last_stat_w = r.stat_w; opts->last_sk_nw = 0; opts->last_ks_epi4 = r.ks_epi4; }
    if (r.err != hipSuccess) return r.err;
    GemmP p = p_in;
    if (!r.stat_nt) p.stat_out = nullptr;                       // the chosen kernel has no row-statistics epilogue for this launch
    p.stat_nt = r.stat_nt; p.stat_w = r.stat_w;
    if (r.cfg == CFG_SKINNYTM32 || r.cfg == CFG_SKINNYTM64) {
        p.sk_nw = o.skinny_nw;
        if (opts) opts->last_sk_nw = gemm_skinny_tm_waves(p);
        return traced_launch(opts, r.cfg, p, s, [&] { return launch_gemm_skinny_tm(p, s); });
    }
    if (r.cfg == CFG_SKINNY32 || r.cfg == CFG_SKINNY64) return traced_launch(opts, r.cfg, p, s, [&] { return launch_gemm_skinny(p, s); });
    const TileCfg* c = cfg_table().row[r.cfg];
    if (c->pipe == PIPE_X3H) {
        p.wh_ldb = wh_ldb_of(p);
        p.wh_gstride = wh_gstride_of(p);
        p.x3h_flag = o.x3h_flag;
    }
    if (c->pipe == PIPE_X6 && p.w3_plane == 0) p.w3_plane = (long long)p.N * p.ldw;
    const GemmKernel fn = r.ks_epi4 ? c->fn4[r.variant] : c->fn[r.variant];
    // window configurations: the attribute covers the widest window (span <= 64)
    const size_t lds_attr = c->win_qs ? c->lds + (size_t)c->win_qs * ((c->bm + 64 + 7) & ~7) * BK * sizeof(float) : r.lds;
    const hipError_t e = dyn_lds_once(g_attr_done[r.cfg][r.variant + (r.ks_epi4 ? kGemmVariants : 0)], reinterpret_cast<const void*>(fn), lds_attr);
    if (e != hipSuccess) return e;
    const int tiles = ((p.M + c->bm - 1) / c->bm) * ((p.N + c->bn - 1) / c->bn);
    p.epi_t4 = 1;
    p.ldr_prio = o.ldr_prio;
    p.ldr64 = o.ldr64 ? 1 : 0;
    const dim3 grid(tiles, 1, p.groups), block(c->threads);
    return traced_launch(opts, r.cfg, p, s, [&] {
        hipLaunchKernelGGL(fn, grid, block, r.lds, s, p);
        return hipGetLastError();
    });
}

}  // namespace mt2
