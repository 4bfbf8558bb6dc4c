// Stage drivers of libmegatts2_hip: they plan row sets on the host, upload the (small) integer plans
// with one copy per call and enqueue the gfx950 kernels of mt2_kernels.h on the caller's stream.
// Each driver cites the reference function it replaces; batch semantics are "B independent batch-1
// runs" (SURVEY.md N1): per-utterance zero gaps for convolutions, per-utterance attention ranges,
// positional indices restarting at 0.
#include "mt2_model.h"
#include "x3h_planes.h"
#include "gemm_tiles.h"

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <numeric>

namespace mt2 {

// Tuning switches (split-K through the LayerNorm, vocoder stream count, tile thresholds, ...) live in the handle:
// mt2_model::opts (mt2_kernels.h EngineOpts), set through mt2_set_option.

// ---------------------------------------------------------------------------------------------------
// planning helpers

static RowSet make_rows(const int* lens, int B, int G) {
    RowSet rs;
    rs.B = B; rs.G = G;
    rs.len.assign(lens, lens + B);
    rs.off.resize(B);
    int r = G;
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(lens[b] >= 0, "negative utterance length");
        rs.off[b] = r;
        r += lens[b] + G;
        rs.maxlen = std::max(rs.maxlen, lens[b]);
    }
    rs.R = r;
    return rs;
}

// Gap rows between the utterances of a batch, per row set of the parallel stages.  Zero padding IS the gap: a "same" convolution of
// one utterance has to read zeros behind its ends, never a neighbour's rows, so the gap covers the widest halo, (k - 1) / 2, of the
// convolutions that run over the row set - the kernels come from the checkpoint's configuration.  Never less than the 2 rows (8 prompt
// rows) of the production model (kernels 3 and 5, stride 16), whose row layout is what it always was.  mt2_workspace_query counts the
// same gaps; the stage drivers refuse a row set narrower than their halo (require_gap).
static int halo_of(int k) { return (k - 1) / 2; }
static int prompt_mel_gap(const mt2_config& cfg) { return std::max({cfg.mrte_stride / 2, halo_of(cfg.mrte_kernel), 2}); }
static int mel_context_gap(const mt2_config& cfg) { return std::max(halo_of(cfg.mrte_kernel), 2); }
static int phone_gap(const mt2_config&) { return 2; }      // the conv-FF kernel is the literal 5 (encoder_layer)
static int decoder_gap(const mt2_config& cfg) { return std::max(halo_of(cfg.dec_kernel), 2); }
static int vqpe_gap(const mt2_config& cfg) { return std::max(halo_of(cfg.vq_kernel), 2); }      // frame rows and pooled rows
static void require_gap(const RowSet& rs, int halo) {
    MT2_REQUIRE(rs.G >= halo, "the gap between utterances is narrower than a convolution's halo");
}

struct RowPlanOffsets { int valid, start, len; };
static RowPlanOffsets plan_rows(IntPlan& ip, const RowSet& rs) {
    std::vector<int> valid(rs.R, 0);
    for (int b = 0; b < rs.B; ++b) std::fill(valid.begin() + rs.off[b], valid.begin() + rs.off[b] + rs.len[b], 1);
    RowPlanOffsets o;
    o.valid = ip.add(valid);
    o.start = ip.add(rs.off);
    o.len = ip.add(rs.len);
    return o;
}
static void bind_rows(const IntPlan& ip, const RowPlanOffsets& o, RowSet& rs) {
    rs.d_valid = ip.dev(o.valid);
    rs.d_start = ip.dev(o.start);
    rs.d_len = ip.dev(o.len);
}
// rowmap[r] = b * stride + t for real rows, -1 for gap rows (pack / unpack of padded tensors)
static int plan_rowmap(IntPlan& ip, const RowSet& rs, int stride) {
    std::vector<int> map(rs.R, -1);
    for (int b = 0; b < rs.B; ++b)
        for (int t = 0; t < rs.len[b]; ++t) map[rs.off[b] + t] = b * stride + t;
    return ip.add(map);
}

// ---------------------------------------------------------------------------------------------------
// kernel-call helpers

struct Ctx {
    mt2_model& m;
    hipStream_t s;
    Arena& ws;
};

// One line of the form log (mt2_model::form_log): "kind point form key=value ...".  Written only between mt2_form_log_begin and
// mt2_form_log_end and only inside ar_step_layers, hifigan_rows and the drivers of the parallel stages - mel_context_rows, tc_latent_rows,
// vqpe_rows, decoder_rows - (form_kind set); it records a decision already taken and takes none.
static void form_kind(const Ctx& c, const char* kind) {      // the layer kind of the entries that follow (nothing is written with the log off)
    if (c.m.form_log_on) c.m.form_kind = kind;
}
struct FormScope {      // ar_step_layers, hifigan_rows, the parallel stages: no kind outlives it, on any exit path - nothing outside them is logged
    mt2_model& m;
    ~FormScope() { m.form_kind = nullptr; }
};
static void form_note(const Ctx& c, const char* point, const char* form, const char* fmt = "", ...) {
    if (!c.m.form_log_on || !c.m.form_kind) return;
    char buf[256];
    int n = snprintf(buf, sizeof buf, "%s %s %s ", c.m.form_kind, point, form);
    va_list ap;
    va_start(ap, fmt);
    if (n > 0 && n < (int)sizeof buf) vsnprintf(buf + n, sizeof buf - n, fmt, ap);
    va_end(ap);
    c.m.form_log.emplace_back(buf);
}

// form log of the parallel stages (kinds mel-encoder, phone-encoder, cross, vqpe, decoder): a convolution just launched - which of
// first | block | mid | last | ff; `shared`: the groups read one input (strideX = 0), `wshared`: one weight (strideW = 0); relued: the
// input is stored ReLU'd (no prologue) - and a linear layer just launched
static void form_note_conv(const Ctx& c, const char* which, const GemmP& p, bool relued = false) {
    if (!c.m.form_log_on || !c.m.form_kind) return;
    const int G = p.groups > 0 ? p.groups : 1;
    form_note(c, "conv", which, "tile=%s M=%d N=%d taps=%d groups=%d shared=%d wshared=%d relued=%d a_planes=%d", c.m.opts.last_cfg, p.M, p.N,
              p.taps > 0 ? p.taps : 1, G, G > 1 && p.strideX == 0 ? 1 : 0, G > 1 && p.strideW == 0 ? 1 : 0, relued ? 1 : 0, p.a_planes);
}
static void form_note_linear(const Ctx& c, const char* which, int M, int N, int K) {
    form_note(c, "linear", which, "tile=%s M=%d N=%d K=%d nw=%d", c.m.opts.last_cfg, M, N, K, c.m.opts.last_sk_nw);
}

// the bf16 planes of a weight pointer, if its buffer has them (mt2_model::planes, sorted by base)
static void attach_planes(const mt2_model& m, GemmP& p) {
    if (p.W3 || m.planes.empty()) return;
    auto it = std::upper_bound(m.planes.begin(), m.planes.end(), p.W,
                               [](const float* w, const PlaneRange& r) { return w < r.base; });
    if (it == m.planes.begin()) return;
    --it;
    if (p.W < it->base + it->n) {
        p.W3 = it->p3 + (p.W - it->base);
        p.w3_plane = (long long)it->n;
        // the fp16 planes carry one scale per weight row: usable when this launch walks the buffer with the rows it was split by
        // (K slices of a row - split-K - share the row's scale): the rule is x3h_group_planes (x3h_planes.h), which the kernel tests
        // run as well
        const int ldw = p.ldw ? p.ldw : (p.taps > 0 ? p.taps : 1) * p.Cin;
        const X3hGroupPlanes g = x3h_group_planes((long long)it->row_len, (long long)(p.W - it->base), ldw, p.strideW, p.groups);
        if (it->ph && g.form != X3H_NO_PLANES) {
            p.Wh = reinterpret_cast<const char*>(it->ph) + g.wh_off;
            p.wh_ldb = g.wh_ldb;
            p.wh_gstride = g.wh_gstride;
            p.wh_inv = it->inv + g.inv_off;
            p.wh_inv_stride = g.wh_inv_stride;
        }
    }
}
// the tile-major copy of the matrix a weight pointer lies in, if it has one (mt2_model::tm, sorted by base) and the
// pointer starts on a block boundary (row multiple of 16, column multiple of 64)
static void attach_tm(const mt2_model& m, GemmP& p) {
    if (p.Wtm || m.tm.empty() || p.M > 64) return;
    auto it = std::upper_bound(m.tm.begin(), m.tm.end(), p.W, [](const float* w, const TmRange& r) { return w < r.base; });
    if (it == m.tm.begin()) return;
    --it;
    if (p.W >= it->base + it->n) return;
    const size_t off = (size_t)(p.W - it->base);
    const int n0 = (int)(off / it->K), k0 = (int)(off % it->K);
    if ((n0 & 15) || (k0 & 63) || p.ldw != it->K) return;
    p.Wtm = it->tm; p.tm_n0 = n0 / 16; p.tm_k0 = k0 / 64; p.tm_kb = it->K / 64;
}
static void gemm(const Ctx& c, GemmP p) {
    attach_planes(c.m, p);
    if (p.ldw == 0) p.ldw = p.taps > 0 ? p.taps * p.Cin : p.Cin;
    attach_tm(c.m, p);
    if (p.taps <= 0) p.taps = 1;
    if (p.dil <= 0) p.dil = 1;
    if (p.a_mul == 0) p.a_mul = 1;
    if (p.groups <= 0) p.groups = 1;
    if (p.out_scale == 0.0f) p.out_scale = 1.0f;
    p.K = p.taps * p.Cin;
    if (p.ldw == 0) p.ldw = p.K;
    MT2_HIP(launch_gemm(p, c.s, &c.m.opts));
}

// y[M, N] = x[M, K] @ W^T + b  (F.linear)
static void linear(const Ctx& c, const float* x, int ldx, int M, const float* W, const float* b, int N, int K,
                   float* y, int ldy, const float* R = nullptr, int ldr = 0, const int* valid = nullptr,
                   int epi_act = ACT_NONE, bool a_planes = false, bool c_planes = false) {
    GemmP p{};
    p.X = x; p.ldx = ldx; p.Rx = M; p.Cin = K; p.W = W; p.bias = b; p.R = R; p.ldr = ldr; p.valid = valid;
    p.C = y; p.ldc = ldy; p.M = M; p.N = N; p.epi_act = epi_act; p.a_planes = a_planes ? 1 : 0; p.c_planes = c_planes ? 1 : 0;
    gemm(c, p);
}
// the fields gemm() fills in before launch_gemm, for the queries gemm_takes_planes / gemm_writes_planes on a launch not yet made
static GemmP planned(const Ctx& c, GemmP p) {
    if (p.taps <= 0) p.taps = 1;
    if (p.dil <= 0) p.dil = 1;
    if (p.a_mul == 0) p.a_mul = 1;
    if (p.groups <= 0) p.groups = 1;
    if (p.out_scale == 0.0f) p.out_scale = 1.0f;
    p.K = p.taps * p.Cin;
    if (p.ldw == 0) p.ldw = p.K;
    attach_planes(c.m, p);
    return p;
}
// Will linear(x -> y) run on an x3h tile that takes x as fp16 planes (GemmP::a_planes)?  Then the LayerNorm that produces x writes
// planes (LnP::out_planes / LnReduceP::h_planes: same bytes, same row stride) and the GEMM's K loop holds no split arithmetic - in
// the loader tile that arithmetic is 8..18 % of a launch (profiles/r06_x3h_ablate_v3_split.txt).
static bool linear_takes_planes(const Ctx& c, const float* x, int ldx, int M, const float* W, const float* b, int N, int K,
                                float* y, int ldy, int epi_act) {
    if (!(c.m.opts.a_planes & 1)) return false;
    GemmP p{};
    p.X = x; p.ldx = ldx; p.Rx = M; p.Cin = K; p.W = W; p.bias = b; p.C = y; p.ldc = ldy; p.M = M; p.N = N; p.epi_act = epi_act;
    p.taps = 1; p.dil = 1; p.a_mul = 1; p.groups = 1; p.out_scale = 1.0f; p.K = K; p.ldw = K;
    attach_planes(c.m, p);
    return gemm_takes_planes(p, c.m.opts);
}

// y[M, N] = act(LN(x_rows)[M, K] @ W^T + b), x_rows[m] = x + (m * a_mul + shift0) * ldx.  Three forms, same result
// up to fp32 round-off:
//   at most 64 rows: ONE launch of the weight-streaming kernel, which normalises its A rows itself (from the (mean, M2) pairs
//     of the producer's epilogue where they exist);
//   pair-fed (ln_pairs; needs the folded operands Wl / s / c of EncLayerW and the producer's pairs): ONE launch,
//     rstd * (acc - mean * s) + c in the epilogue of an x6 / x3h tile, no pass over K;
//   plain: launch_layernorm into `h_scratch` + a GEMM.
// (LayerNorm as a prologue of the f32 tiles - options lnfuse / lnalg of rounds 1-2 - measured slower at every size and was
// retired in round 6: profiles/r06_retired_kernel_forms_and_options.patch.)
// What a layer hands to the next LayerNorm about the residual stream x (AR step forms below):
//   S > 0    - a residual update not yet applied: x += bias + sum_g parts[g] (split-K through the LayerNorm);
//   stat     - x is final and the GEMM that wrote it left its row statistics as (mean, M2) pairs per wave tile
//              (GemmP::stat_out): the consuming LN -> Linear pair runs as ONE pair-fed algebraic-LayerNorm GEMM.
struct Pending {
    const float* parts = nullptr; long long pstride = 0; int S = 0; const float* bias = nullptr;
    const float* stat = nullptr; int stat_nt = 0, stat_w = 0;
};
struct LnOps {                 // operands of one LN -> Linear pair, rows [n0, n0 + N) of the weight matrix
    const float *g, *b, *W, *bias;        // LayerNorm affine, Linear weight / bias
    const float *Wl, *s, *c;              // folded operands (nullptr: not available)
};
static LnOps ln_ops(const float* g, const float* b, const float* W, const float* bias, const float* Wl, const float* s,
                    const float* c, int n0, int K) {
    return LnOps{g, b, W + (size_t)n0 * K, bias + n0, Wl ? Wl + (size_t)n0 * K : nullptr, s ? s + n0 : nullptr,
                 c ? c + n0 : nullptr};
}
static void ln_linear(const Ctx& c, const float* x, int ldx, int Rx, int a_mul, int shift0, int M, const LnOps& w, int N,
                      int K, float* y, int ldy, float* h_scratch, int epi_act = ACT_NONE, const Pending* st = nullptr,
                      bool c_planes = false) {
    GemmP p{};
    p.c_planes = c_planes ? 1 : 0;      // y as fp16 planes (the caller asked gemm_writes_planes; more than 64 rows)
    p.X = x; p.ldx = ldx; p.Rx = Rx; p.a_mul = a_mul ? a_mul : 1; p.shift0 = shift0; p.taps = 1; p.dil = 1; p.Cin = K;
    p.K = K; p.W = w.W; p.ldw = K; p.bias = w.bias; p.C = y; p.ldc = ldy; p.M = M; p.N = N; p.groups = 1; p.out_scale = 1.0f;
    p.epi_act = epi_act; p.ln_eps = 1e-5f;
    if (c.m.opts.skinny_tm && M <= c.m.opts.skinny_rows && c.m.opts.force_cfg < 0) {
        // a handful of rows: the weight-streaming kernel normalises its A rows itself (gemm_skinny_tm_kernel, PRO_LN) -
        // one launch, statistics computed while the first weight pieces are in flight
        GemmP q = p;
        q.pro_act = 3; q.ln_g = w.g; q.ln_b = w.b;
        if (st && st->stat && st->stat_w == 16 && c.m.opts.skinny_pairs) {      // the rows' statistics came with them (16-column pairs)
            q.ln_stat = st->stat; q.ln_nt = st->stat_nt; q.ln_w = 16;
        }
        attach_tm(c.m, q);
        if (q.Wtm && gemm_skinny_tm_eligible(q, c.m.opts.skinny_rows)) {
            // launch_gemm routes to the tile-major kernel only when its own conditions hold too; with another routing the
            // LayerNorm-prologue form may not exist for the tile it picks: fall through like the branches below
            const hipError_t e = launch_gemm(q, c.s, &c.m.opts);
            if (e == hipSuccess) {
                form_note(c, "ln_linear", q.ln_stat ? "skinny-ln-pairs" : "skinny-ln", "M=%d N=%d tile=%s nw=%d", M, N, c.m.opts.last_cfg,
                          c.m.opts.last_sk_nw);
                return;
            }
            if (e != hipErrorNotSupported) MT2_HIP(e);
        }
    }
    // (pairs of the tile-major kernel - 16 columns each, up to 64 per row - are not what the x6 / x3h tiles merge: launch_gemm would
    // answer InvalidValue, not NotSupported)
    if (st && st->stat && st->stat_nt > 0 && st->stat_w != 16 && st->stat_nt <= 32 && (st->stat_nt & 1) == 0 && c.m.opts.ln_pairs && w.Wl &&
        c.m.opts.force_cfg < 0 && M <= c.m.opts.ln_pairs_maxm) {
        // the rows' statistics came with them (pairs from the producer GEMM's epilogue): algebraic LayerNorm with NO pass
        // over K - rstd * (x W'^T - mean * s) + c on the x6 tiles; a tile without that form answers NotSupported
        GemmP q = p;
        q.pro_act = 5; q.W = w.Wl; q.bias = w.c; q.ln_g = w.s; q.ln_stat = st->stat; q.ln_nt = st->stat_nt; q.ln_w = st->stat_w;
        attach_planes(c.m, q);
        const hipError_t e = launch_gemm(q, c.s, &c.m.opts);
        if (e == hipSuccess) {
            form_note(c, "ln_linear", "pair-fed", "M=%d N=%d tile=%s nw=0", M, N, c.m.opts.last_cfg);
            return;
        }
        if (e != hipErrorNotSupported) MT2_HIP(e);
    }
    const bool planes = linear_takes_planes(c, h_scratch, K, M, w.W, w.bias, N, K, y, ldy, epi_act);
    LnP q{};
    q.x = x + (long long)shift0 * ldx; q.ldx = ldx * p.a_mul; q.gamma = w.g; q.beta = w.b; q.out = h_scratch; q.ldo = K;
    q.M = M; q.C = K; q.eps = 1e-5f; q.act = ACT_NONE; q.out_planes = planes ? 1 : 0; q.x3h_flag = c.m.opts.x3h_flag;
    MT2_HIP(launch_layernorm(q, c.s));
    linear(c, h_scratch, K, M, w.W, w.bias, N, K, y, ldy, nullptr, 0, nullptr, epi_act, planes, c_planes);
    form_note(c, "ln_linear", planes ? "plain+planes" : "plain", "M=%d N=%d tile=%s nw=%d", M, N, c.m.opts.last_cfg, c.m.opts.last_sk_nw);
}
static LnOps ln1_qkv(const EncLayerW& w, int d, int n0 = 0) {
    return ln_ops(w.ln1g, w.ln1b, w.wqkv, w.bqkv, w.wqkv_l, w.sqkv, w.cqkv, n0, d);
}
static LnOps ln2_ff0(const EncLayerW& w, int d) {
    return ln_ops(w.ln2g, w.ln2b, w.ff0w, w.ff0b, w.ff0_l, w.sff0, w.cff0, 0, d);
}

// nn.Conv1d(k, stride 1, padding (k-1)/2 * dil, dilation dil) over gap-padded rows
static void conv_same(const Ctx& c, const float* x, int ldx, int R, const ConvW& w, float* y, int ldy,
                      const int* valid, int pro_act = ACT_NONE, float slope = 0.f, int epi_act = ACT_NONE,
                      const float* Rsd = nullptr, int ldr = 0, int dil = 1, const char* note = nullptr) {
    GemmP p{};
    p.X = x; p.ldx = ldx; p.Rx = R; p.taps = w.k; p.dil = dil; p.shift0 = -((w.k - 1) / 2) * dil; p.Cin = w.cin;
    p.W = w.w; p.bias = w.b; p.R = Rsd; p.ldr = ldr; p.valid = valid; p.C = y; p.ldc = ldy; p.M = R; p.N = w.cout;
    p.pro_act = pro_act; p.pro_slope = slope; p.epi_act = epi_act;
    gemm(c, p);
    if (note) form_note_conv(c, note, p);      // (the parallel stages; the vocoder books its convolutions itself)
}

// y = x + conv2(lrelu(conv1(lrelu(x)))) (ResBlock1's pair: conv1 dilated, conv2 dilation 1, both k taps, C -> C) as one launch of
// the fused pair kernel; false: conv_pair_route keeps the two-launch form for this pair (nothing was launched)
static bool conv_pair(const Ctx& c, const float* x, int C, int R, const ConvW& w1, const ConvW& w2, int dil, float slope,
                      bool reflect, float* y, const int* valid) {
    if (w1.k != w2.k || w1.cin != C || w1.cout != C || w2.cin != C || w2.cout != C) return false;
    GemmP g1{}, g2{};
    g1.W = w1.w; g1.taps = w1.k; g1.Cin = C; g1.groups = 1;
    g2.W = w2.w; g2.taps = w2.k; g2.Cin = C; g2.groups = 1;
    attach_planes(c.m, g1);
    attach_planes(c.m, g2);
    if (!g1.W3 || !g2.W3 || g1.wh_ldb != g2.wh_ldb) return false;        // (the two launches would not run on the x3h tiles either)
    PairP p{};
    p.X = x; p.ldx = C; p.R = R; p.C = C; p.taps = w1.k; p.dil = dil; p.slope = slope;
    p.Wh1 = g1.Wh; p.inv1 = g1.wh_inv; p.bias1 = w1.b;
    p.Wh2 = g2.Wh; p.inv2 = g2.wh_inv; p.bias2 = w2.b;
    p.wh_ldb = g1.wh_ldb ? g1.wh_ldb : 4ll * ((w1.k * C + 31) / 32 * 32);
    p.valid = valid; p.Y = y; p.ldy = C; p.reflect = reflect ? 1 : 0;
    const hipError_t e = launch_conv_pair(p, c.s, &c.m.opts);
    if (e == hipErrorNotSupported) return false;
    MT2_HIP(e);
    return true;
}

// lrelu(mean of the three resblock outputs) -> ConvTranspose1d(stride 2) of the next vocoder stage as one launch of the fused kernel;
// false: up_mrf_route keeps launch_avg3 + the two GEMM halves for this boundary (nothing was launched)
static bool up_mrf(const Ctx& c, const float* const* rb, int ch, int R, const UpW& u, float slope, float* up, const int* valid) {
    if (!u.wcat || u.cin != ch || u.cout * 2 != ch) return false;
    GemmP g{};
    g.W = u.wcat; g.taps = 2; g.Cin = ch; g.groups = 1;
    attach_planes(c.m, g);
    UpMrfP p{};
    p.X0 = rb[0]; p.X1 = rb[1]; p.X2 = rb[2]; p.ldx = ch; p.R = R; p.ch = ch; p.stride = u.stride;
    p.scale = 1.0f / 3.0f; p.slope = slope;
    p.Wh = g.Wh; p.inv = g.wh_inv; p.bias = u.bias; p.wh_ldb = g.wh_ldb ? g.wh_ldb : 8ll * ch;
    p.valid = valid; p.Y = up; p.ldy = 2 * u.cout;
    const hipError_t e = launch_up_mrf(p, c.s, &c.m.opts);
    if (e == hipErrorNotSupported) return false;
    MT2_HIP(e);
    return true;
}

static void layernorm(const Ctx& c, const float* x, int ldx, const float* g, const float* b, int M, int C,
                      float* out, int ldo, const int* valid = nullptr, int valid_rows = 0,
                      const float* R1 = nullptr, int ldr1 = 0, int r1_rows = 0, int rows_per_group = 0,
                      int act = ACT_NONE, bool out_planes = false) {
    LnP p{};
    p.x = x; p.ldx = ldx; p.gamma = g; p.beta = b; p.rows_per_group = rows_per_group;
    p.R1 = R1; p.ldr1 = ldr1; p.r1_rows = r1_rows; p.valid = valid; p.valid_rows = valid_rows;
    p.out = out; p.ldo = ldo; p.M = M; p.C = C; p.eps = 1e-5f; p.act = act;
    p.out_planes = out_planes ? 1 : 0; p.x3h_flag = c.m.opts.x3h_flag;
    MT2_HIP(launch_layernorm(p, c.s));
}

// ResidualBlockStack.forward (modules/convnet.py:69-72) for `groups` parallel branches at once:
// x = x + ConvStack(x), ConvBlock = ReLU -> Conv1d -> LayerNorm(C) (convnet.py:23-31).
// x_in: [R, C] shared by all groups (shared_in) or [groups][R, C].  Returns [groups][R, C].
static float* run_stack(const Ctx& c, const StackW& w, const float* x_in, bool shared_in, int R,
                        const int* valid) {
    const int C = w.C, G = w.groups;
    const size_t per = (size_t)R * C;
    float* T = c.ws.get<float>(per * G);
    float* Y = c.ws.get<float>(per * G);
    float* XA = c.ws.get<float>(per * G);
    float* XB = c.ws.get<float>(per * G);
    const float* cur = x_in;
    bool cur_shared = shared_in;
    float* nxt = XA;
    const size_t wsz = (size_t)C * w.k * C;
    for (int st = 0; st < w.nstack; ++st) {
        const float* bin = cur;
        bool bin_shared = cur_shared;
        bool bin_relued = false;    // a block output with ONE consumer (the next block's conv) is stored ReLU'd
        bool bin_planes = false;    // ... and as fp16 planes when that conv runs on an x3h tile that takes them (GemmP::a_planes)
        auto block_conv = [&](int blk, const float* in, bool in_shared, bool relued, bool planes) {
            const size_t e = w.idx(st, blk);
            GemmP p{};
            p.X = in; p.strideX = in_shared ? 0 : (long long)per; p.ldx = C; p.Rx = R;
            p.taps = w.k; p.shift0 = -((w.k - 1) / 2); p.Cin = C;
            p.W = w.w + e * wsz; p.strideW = (long long)wsz;
            p.bias = w.b + e * C; p.strideB = C;
            p.valid = valid; p.C = T; p.strideC = (long long)per; p.ldc = C; p.M = R; p.N = C; p.groups = G;
            p.pro_act = relued ? ACT_NONE : ACT_RELU;
            p.a_planes = planes ? 1 : 0;
            return p;
        };
        for (int blk = 0; blk < w.nblock; ++blk) {
            const size_t e = w.idx(st, blk);
            const GemmP launched = block_conv(blk, bin, bin_shared, bin_relued, bin_planes);
            gemm(c, launched);
            form_note_conv(c, "block", launched, bin_relued);
            const bool last = blk == w.nblock - 1;
            bool planes = false;
            if (!last && (c.m.opts.a_planes & 1)) {       // will the next block's conv take Y as planes?
                GemmP q = block_conv(blk + 1, Y, false, true, false);
                q.dil = 1; q.a_mul = 1; q.out_scale = 1.0f; q.K = q.taps * q.Cin; q.ldw = q.K;
                attach_planes(c.m, q);
                planes = gemm_takes_planes(q, c.m.opts);
            }
            if (last)
                layernorm(c, T, C, w.g + e * C, w.be + e * C, R * G, C, nxt, C, valid, R, cur, C,
                          cur_shared ? R : 0, R);
            else   // next ConvBlock starts with ReLU (convnet.py:24): fold it into this LayerNorm's store
                layernorm(c, T, C, w.g + e * C, w.be + e * C, R * G, C, Y, C, valid, R, nullptr, 0, 0, R, ACT_RELU, planes);
            form_note(c, "ln", last ? "residual" : "block", "out_planes=%d act=%d M=%d groups=%d", planes ? 1 : 0, last ? 0 : 1, R, G);
            bin = Y;
            bin_shared = false;
            bin_relued = !last;
            bin_planes = planes;
        }
        cur = nxt;
        cur_shared = false;
        nxt = (nxt == XA) ? XB : XA;
    }
    return const_cast<float*>(cur);
}

// TransformerEncoderLayer.forward (modules/transformer.py:88-102) over packed rows, in place on x.
//   attention geometry: per-utterance (starts/lens arrays) or uniform (AR steps).
struct AttnGeom {
    const int* start = nullptr; const int* len = nullptr;
    int u_stride = 0, u_len = 0, B = 0, max_len = 0;
};
struct EncScratch { float *h, *qkv, *att, *f, *parts, *stat; };
static EncScratch enc_scratch(const Ctx& c, const EncW& e, int M) {
    EncScratch s;
    s.h = c.ws.get<float>((size_t)M * e.d);
    s.qkv = c.ws.get<float>((size_t)M * 3 * e.d);
    s.att = c.ws.get<float>((size_t)M * e.d);
    s.f = c.ws.get<float>((size_t)M * e.ff);
    // split-K slabs [S][M, d]: the f32 rule of choose_split keeps tiles(32x64) * S <= 256 (S * M * d <= 256 * 32 * 64 *
    // d / 64); the x6 rule splits at most 8 ways at any M
    s.parts = c.ws.get<float>(std::max((size_t)256 * 32 * 64 + (size_t)16 * 32 * e.d, (size_t)8 * M * e.d));
    s.stat = c.ws.get<float>((size_t)M * 128);     // row statistics handed from GEMM to GEMM: <= 64 (mean, M2) pairs per row
    return s;
}
// the attention launch parameters that come from the engine options and the head geometry (H heads of width D): the one place
// where they are set - callers add their row ranges and pointers
static AttnP attn_params(const Ctx& c, int H, int D) {
    AttnP a{};
    a.H = H; a.D = D; a.scale = 1.0f / std::sqrt((float)D);
    a.lds_min_qlen = c.m.opts.attn_lds_min; a.x6_min_qlen = c.m.opts.attn_x6_min;
    a.x3h = (c.m.opts.x3h & 8) ? 1 : 0; a.x3h_flag = c.m.opts.x3h_flag;
    return a;
}
static AttnP attn_params(const Ctx& c, const EncW& e) { return attn_params(c, e.heads, e.d / e.heads); }
// form log: the kernel attn_route chose for a launch just made
static void form_note_attention(const Ctx& c, const AttnP& a) {
    if (!c.m.form_log_on || !c.m.form_kind) return;
    static const char* const kName[] = {"none", "generic", "reg", "ds", "lds", "x6", "x3h"};
    const int k = attn_route(a).kernel;
    form_note(c, "attention", k >= 0 && k <= ATTN_X3H ? kName[k] : "?", "o_planes=%d B=%d qlen=%d kvlen=%d D=%d", a.o_planes, a.B, a.max_qlen,
              a.kv_len ? a.max_kvlen : a.u_kvlen, a.D);      // (ragged launches: the longest key range)
}
static void attention_self(const Ctx& c, const EncW& e, const AttnGeom& g, const float* qkv, float* att, bool o_planes = false) {
    AttnP a = attn_params(c, e);
    a.o_planes = o_planes ? 1 : 0;
    const int d = e.d;
    a.Q = qkv; a.ldq = 3 * d; a.K = qkv + d; a.ldk = 3 * d; a.V = qkv + 2 * d; a.ldv = 3 * d;
    a.O = att; a.ldo = d;
    a.q_start = g.start; a.q_len = g.len; a.kv_start = g.start; a.kv_len = g.len;
    a.u_qstride = g.u_stride; a.u_qlen = g.u_len; a.u_kvstride = g.u_stride; a.u_kvlen = g.u_len;
    a.B = g.B; a.max_qlen = g.max_len; a.max_kvlen = g.max_len;
    MT2_HIP(launch_attention(a, c.s));
    form_note_attention(c, a);
}
static void encoder_layer(const Ctx& c, const EncW& e, const EncLayerW& w, float* x, int M, const AttnGeom& g,
                          const int* valid, const EncScratch& s) {
    const int d = e.d;
    layernorm(c, x, d, w.ln1g, w.ln1b, M, d, s.h, d, valid);
    form_note(c, "ln", "plain", "out_planes=0 act=0 M=%d groups=1", M);
    linear(c, s.h, d, M, w.wqkv, w.bqkv, 3 * d, d, s.qkv, 3 * d);
    form_note_linear(c, "qkv", M, 3 * d, d);
    attention_self(c, e, g, s.qkv, s.att);
    linear(c, s.att, d, M, w.wo, w.bo, d, d, x, d, x, d, valid);            // x = x + out_proj(att)
    form_note_linear(c, "out", M, d, d);
    if (e.conv_ff) {
        // x = norm2(x); x = x + conv2(relu(conv1(x)))   (transformer.py:95-99; residual from the NORMED x)
        layernorm(c, x, d, w.ln2g, w.ln2b, M, d, s.h, d, valid);
        form_note(c, "ln", "plain", "out_planes=0 act=0 M=%d groups=1", M);
        ConvW c1{w.ff0w, w.ff0b, e.ff, d, 5}, c2{w.ff1w, w.ff1b, d, e.ff, 5};
        conv_same(c, s.h, d, M, c1, s.f, e.ff, valid, ACT_NONE, 0.f, ACT_RELU, nullptr, 0, 1, "ff");
        conv_same(c, s.f, e.ff, M, c2, x, d, valid, ACT_NONE, 0.f, ACT_NONE, s.h, d, 1, "ff");
    } else {
        layernorm(c, x, d, w.ln2g, w.ln2b, M, d, s.h, d, valid);
        form_note(c, "ln", "plain", "out_planes=0 act=0 M=%d groups=1", M);
        linear(c, s.h, d, M, w.ff0w, w.ff0b, e.ff, d, s.f, e.ff, nullptr, 0, nullptr, ACT_RELU);
        form_note_linear(c, "ff", M, e.ff, d);
        linear(c, s.f, e.ff, M, w.ff1w, w.ff1b, d, e.ff, x, d, x, d, valid);
        form_note_linear(c, "ff", M, d, e.ff);
    }
}

// ---- autoregressive-step forms of the encoder layer (Linear-FF encoders only).  All of them are exact
// identities of TransformerEncoderLayer.forward (modules/transformer.py:88-102), not approximations.
//
// Split-K through the LayerNorm.  A GEMM of the early / middle steps has too few tiles for the chip, and a
// tile's serial K chain is its latency floor (K = 4096 in the PLM's second feed-forward: 45 us at any M).
// Such a GEMM runs as S independent K slices (GemmP groups: slice g reads columns [g*K/S, (g+1)*K/S) of both
// operands and writes a raw partial slab) and the NEXT LayerNorm - a launch the layer has anyway - sums the
// slabs in fixed order, adds bias and residual, writes the residual stream and its normalisation
// (launch_ln_reduce).  Deterministic, no extra launch, no inter-workgroup hand-off.
static int choose_split(const Ctx& c, int M, int N, int K) {
    if (!c.m.opts.splitk) return 1;
    // a handful of rows on the tile-major weight-streaming kernel (round 4): that kernel adds bias + residual itself and the
    // NEXT GEMM normalises its own input rows (LayerNorm prologue), so a split - whose reduction needs a LayerNorm launch of
    // its own - only pays where one column block's K range is too long for one workgroup: the PLM's ff.3 (K = 4096: 64
    // blocks x 256 KiB); there the K slices are 1024 wide (256 workgroups x 64 KiB) and the reduction rides on LN1 as before
    if (c.m.opts.skinny_tm && c.m.opts.skinny_rows > 0 && M <= c.m.opts.skinny_rows && M <= 64 && c.m.opts.force_cfg < 0 &&
        (N & 15) == 0 && (K & 63) == 0) {
        if (K <= 1536) return 1;
        int S = 1;
        const int kmin = 1024;      // narrowest K slice (two slices of 2048: C1 +2.6 %, eight of 512: +0.4 %; un-split: +7.3 %)
        while (S < 16 && K % (S * 2) == 0 && K / (S * 2) >= kmin && (K / (S * 2)) % 64 == 0) S *= 2;
        return S;
    }
    // x6 form (large M): the N = d GEMMs of a layer (out-projection, ff.3) have too few 128x128 tiles for the bf16 pipe
    // (N = 768 / 1024: 6 / 8 column tiles); K slices as GEMM groups bring them to >= t_x6_128 tiles, and the reduction
    // rides on the next LayerNorm as before (profiles/r02_gemm_sweep_x6.txt: ff.3 at M = 864 does 85 TF/s on the f32
    // K-split tile; four x6 slices of K = 1024 have the shape of ff.0, 125 TF/s)
    if (c.m.opts.x6_gemm && (N & 127) == 0 && (K & 31) == 0) {
        const long long t128 = (long long)((M + 127) / 128) * (N / 128);
        if (t128 < c.m.opts.t_x6_128) {
            int S = 1;
            while (S < 8 && t128 * S < 2 * c.m.opts.t_x6_128 && K % (S * 2) == 0 && K / (S * 2) >= 512 && (K / (S * 2)) % 32 == 0)
                S *= 2;
            if (S > 1 && t128 * S >= c.m.opts.t_x6_128) return S;
        }
    }
    const long long tiles = (long long)((M + 31) / 32) * ((N + 63) / 64);
    int S = 1;
    while (S < 16 && tiles * (S * 2) <= 256 && K % (S * 2) == 0 && K / (S * 2) >= 256 && (K / (S * 2)) % 32 == 0) S *= 2;
    return S;
}
// y_parts[g] = x[:, gK/S:(g+1)K/S] @ W[:, gK/S:(g+1)K/S]^T, g < S  (raw partial slabs [S][M, N])
static GemmP splitk_params(const float* x, int ldx, int M, const float* W, int N, int K, int S, float* parts) {
    GemmP p{};
    p.X = x; p.strideX = K / S; p.ldx = ldx; p.Rx = M; p.Cin = K / S; p.W = W; p.strideW = K / S; p.ldw = K;
    p.C = parts; p.strideC = (long long)M * N; p.ldc = N; p.M = M; p.N = N; p.groups = S;
    return p;
}
static void linear_splitk(const Ctx& c, const float* x, int ldx, int M, const float* W, int N, int K, int S,
                          float* parts, bool a_planes = false) {
    GemmP p = splitk_params(x, ldx, M, W, N, K, S, parts);
    p.a_planes = a_planes ? 1 : 0;
    gemm(c, p);
    form_note(c, "residual", "split", "S=%d stat_nt=0 stat_w=0 a_planes=%d M=%d K=%d tile=%s nw=%d", S, p.a_planes, M, K, c.m.opts.last_cfg,
              c.m.opts.last_sk_nw);
}
// h = LayerNorm(x) after applying a pending update to x (in place)
static void ln_pending(const Ctx& c, float* x, int d, int M, const Pending& in, const float* g, const float* b,
                       float* h, bool h_planes = false) {
    if (in.S == 0) {
        LnP q{};
        q.x = x; q.ldx = d; q.gamma = g; q.beta = b; q.out = h; q.ldo = d; q.M = M; q.C = d; q.eps = 1e-5f; q.act = ACT_NONE;
        q.out_planes = h_planes ? 1 : 0; q.x3h_flag = c.m.opts.x3h_flag;
        MT2_HIP(launch_layernorm(q, c.s));
        form_note(c, "ln_pending", "plain", "S=0 h_planes=%d M=%d", q.out_planes, M);
        return;
    }
    LnReduceP p{};
    p.parts = in.parts; p.pstride = in.pstride; p.S = in.S; p.bias = in.bias; p.R = x; p.ldr = d;
    p.gamma = g; p.beta = b; p.xout = x; p.ldx = d; p.hout = h; p.ldh = d; p.M = M; p.C = d; p.eps = 1e-5f;
    p.h_planes = h_planes ? 1 : 0; p.x3h_flag = c.m.opts.x3h_flag;
    MT2_HIP(launch_ln_reduce(p, c.s));
    form_note(c, "ln_pending", "reduce", "S=%d h_planes=%d M=%d", in.S, p.h_planes, M);
}
// h = LN(x (+ the pending split-K update)), y = act(h W^T + b): h travels as fp16 planes when the GEMM takes them
static void ln_pending_linear(const Ctx& c, float* x, int d, int M, const Pending& in, const float* g, const float* b, float* h,
                              const float* W, const float* bias, int N, float* y, int ldy, int epi_act = ACT_NONE,
                              bool c_planes = false) {
    const bool planes = M <= 4096 && linear_takes_planes(c, h, d, M, W, bias, N, d, y, ldy, epi_act);
    ln_pending(c, x, d, M, in, g, b, h, planes);
    linear(c, h, d, M, W, bias, N, d, y, ldy, nullptr, 0, nullptr, epi_act, planes, c_planes);
}
// everything after attention for M full rows: x += out_proj(att); h = LN2(x); f = relu(ff0(h));
// x += ff1(f) - the last update is returned as pending when it was split
// x += a @ W^T + b (residual update in the GEMM's epilogue); with ln_pairs the epilogue also leaves the row statistics of the
// new x as pairs in `stat` where the chosen tile can - the returned Pending says whether it did
static GemmP residual_params(const Ctx& c, const float* a, int lda, int M, const float* W, const float* b, int N, int K,
                             float* x, float* stat, const float* res, int ldr) {
    GemmP p{};
    p.X = a; p.ldx = lda; p.Rx = M; p.Cin = K; p.W = W; p.bias = b; p.R = res ? res : x; p.ldr = res ? ldr : N; p.C = x; p.ldc = N;
    p.M = M; p.N = N;
    const bool small = M <= 64 && M <= c.m.opts.skinny_rows && c.m.opts.skinny_tm && c.m.opts.skinny_pairs;     // tile-major kernel: pairs per 16 columns
    const bool want = stat != nullptr && c.m.opts.force_cfg < 0 &&
                      (small || (c.m.opts.ln_pairs > 0 && M > 64 && M <= c.m.opts.ln_pairs_maxm));
    if (want) p.stat_out = stat;
    return p;
}
static Pending linear_residual(const Ctx& c, const float* a, int lda, int M, const float* W, const float* b, int N, int K,
                               float* x, float* stat, const float* res = nullptr, int ldr = 0, bool a_planes = false) {
    GemmP p = residual_params(c, a, lda, M, W, b, N, K, x, stat, res, ldr);
    const bool want = p.stat_out != nullptr;
    p.a_planes = a_planes ? 1 : 0;
    gemm(c, p);
    Pending r{};
    if (want && c.m.opts.last_stat_nt > 0) { r.stat = stat; r.stat_nt = c.m.opts.last_stat_nt; r.stat_w = c.m.opts.last_stat_w; }
    form_note(c, "residual", r.stat ? "stat" : "nostat", "S=1 stat_nt=%d stat_w=%d a_planes=%d M=%d K=%d tile=%s nw=%d", r.stat_nt, r.stat_w,
              p.a_planes, M, K, c.m.opts.last_cfg, c.m.opts.last_sk_nw);
    return r;
}
// K slices of the two residual GEMMs of an AR layer (out-projection K = d, ff.3 K = ff)
static void ar_tail_splits(const Ctx& c, const EncW& e, int M, int& S1, int& S2) {
    const int d = e.d;
    // ln_pairs = 2: the residual GEMMs with a short K chain (<= 1024) are not K-split any more - a split hands its reduction
    // to a LayerNorm launch, the un-split GEMM hands the statistics to the next GEMM instead
    const bool unsplit = c.m.opts.ln_pairs >= 2 && M > 64 && M <= c.m.opts.ln_pairs_maxm && c.m.opts.force_cfg < 0;
    S1 = choose_split(c, M, d, d);
    if (unsplit && d <= c.m.opts.ln_pairs_maxk) S1 = 1;
    S2 = choose_split(c, M, d, e.ff);
    if (unsplit && e.ff <= c.m.opts.ln_pairs_maxk) S2 = 1;
}
// attention -> out-projection: will the out-projection of ar_layer_tail take `att` as fp16 planes (then the attention kernel stores
// them: AttnP::o_planes)?  The same hand-over as ff.0 -> ff.3 below, with the attention kernels as producers.
static bool ar_outproj_takes_planes(const Ctx& c, const EncW& e, const EncLayerW& w, float* x, int M, const float* att,
                                    const EncScratch& s) {
    const int d = e.d;
    if (!(c.m.opts.a_planes & 4) || M <= 64 || M > 4096 || (d & 31) || ((d / e.heads) & 31)) return false;
    int S1, S2;
    ar_tail_splits(c, e, M, S1, S2);
    const GemmP q = S1 > 1 ? splitk_params(att, d, M, w.wo, d, d, S1, s.parts)
                           : residual_params(c, att, d, M, w.wo, w.bo, d, d, x, s.stat, nullptr, 0);
    return gemm_takes_planes(planned(c, q), c.m.opts);
}
static Pending ar_layer_tail(const Ctx& c, const EncW& e, const EncLayerW& w, float* x, int M, const float* att,
                             const EncScratch& s, bool att_planes = false) {
    const int d = e.d;
    int S1, S2;
    ar_tail_splits(c, e, M, S1, S2);
    // ff.0 -> ff.3: f = relu(ff.0(h)) has ONE consumer.  Where ff.0 runs on the x3h loader tile and ff.3 on an x3h tile that takes its A
    // operand as fp16 planes, ff.0's epilogue stores f as planes (GemmP::c_planes: the split once per element, in the producer, instead of
    // once per element and column tile in the consumer's K loop) - same values, bit-identical results
    bool fpl = false;
    if ((c.m.opts.a_planes & 2) && M > 64 && M <= 4096) {
        GemmP q0{};
        q0.X = s.h; q0.ldx = d; q0.Rx = M; q0.Cin = d; q0.W = w.ff0w; q0.bias = w.ff0b; q0.C = s.f; q0.ldc = e.ff; q0.M = M; q0.N = e.ff;
        q0.epi_act = ACT_RELU;
        const GemmP q3 = S2 > 1 ? splitk_params(s.f, e.ff, M, w.ff1w, d, e.ff, S2, s.parts)
                                : residual_params(c, s.f, e.ff, M, w.ff1w, w.ff1b, d, e.ff, x, s.stat, nullptr, 0);
        fpl = gemm_writes_planes(planned(c, q0), c.m.opts) && gemm_takes_planes(planned(c, q3), c.m.opts);
    }
    form_note(c, "tail", fpl ? "fpl" : "nofpl", "S1=%d S2=%d M=%d att_planes=%d", S1, S2, M, att_planes ? 1 : 0);
    if (S1 > 1) {
        linear_splitk(c, att, d, M, w.wo, d, d, S1, s.parts, att_planes);
        Pending p1{s.parts, (long long)M * d, S1, w.bo};
        ln_pending_linear(c, x, d, M, p1, w.ln2g, w.ln2b, s.h, w.ff0w, w.ff0b, e.ff, s.f, e.ff, ACT_RELU, fpl);
    } else {
        const Pending p1 = linear_residual(c, att, d, M, w.wo, w.bo, d, d, x, s.stat, nullptr, 0, att_planes);   // x += out_proj(att)
        ln_linear(c, x, d, M, 1, 0, M, ln2_ff0(w, d), e.ff, d, s.f, e.ff, s.h, ACT_RELU, &p1, fpl);    // LN2 -> ff.0
    }
    if (S2 > 1) {
        linear_splitk(c, s.f, e.ff, M, w.ff1w, d, e.ff, S2, s.parts, fpl);
        return Pending{s.parts, (long long)M * d, S2, w.ff1b};
    }
    return linear_residual(c, s.f, e.ff, M, w.ff1w, w.ff1b, d, e.ff, x, s.stat, nullptr, 0, fpl);     // x += ff.3(f)
}

// MIDDLE layer over M = A*n compact rows
static Pending encoder_layer_ar(const Ctx& c, const EncW& e, const EncLayerW& w, float* x, int M, const AttnGeom& g,
                                const EncScratch& s, const Pending& in) {
    MT2_REQUIRE(!e.conv_ff, "AR step layers use the Linear feed-forward");
    const int d = e.d;
    form_kind(c, "mid");
    if (in.S) {
        ln_pending_linear(c, x, d, M, in, w.ln1g, w.ln1b, s.h, w.wqkv, w.bqkv, 3 * d, s.qkv, 3 * d);
    } else {
        ln_linear(c, x, d, M, 1, 0, M, ln1_qkv(w, d), 3 * d, d, s.qkv, 3 * d, s.h, ACT_NONE, &in);     // LN1 -> QKV
    }
    const bool opl = !g.start && ar_outproj_takes_planes(c, e, w, x, M, s.att, s);      // (uniform geometry: every row of att is written)
    attention_self(c, e, g, s.qkv, s.att, opl);
    return ar_layer_tail(c, e, w, x, M, s.att, s, opl);
}

// LAST layer: only row n-1 of each sequence is consumed downstream (models/megatts2.py:178,272).  LayerNorm
// and the K/V projections are row-wise and needed for all rows; attention row i depends on query row i only,
// and out-projection, norm2 and the feed-forward are row-wise - so Q, attention, out-proj, LN2 and FF are
// evaluated for the A last rows only.  x: [A*n, d] compact step rows; y: [A, d] result rows.
static void encoder_layer_last(const Ctx& c, const EncW& e, const EncLayerW& w, float* x, int n, int A,
                               const EncScratch& s, float* y, const Pending& in) {
    MT2_REQUIRE(!e.conv_ff, "AR step layers use the Linear feed-forward");
    const int d = e.d, M = A * n;
    float* kv = s.qkv;                                   // [M, 2d]: K | V
    float* q = s.att;                                    // [A, d]
    float* att = s.att + (size_t)A * d;                  // [A, d]
    AttnP a = attn_params(c, e);
    if (c.m.opts.skinny_tm && M <= c.m.opts.skinny_rows && M <= 64 && c.m.opts.force_cfg < 0) {
        // a handful of rows (one utterance's steps): Q | K | V of ALL rows in ONE weight-streaming launch - the Q rows that
        // are not the last of their sequence cost nothing measurable at M <= 64, a second launch costs ~8 us
        float* qkv = s.qkv;                              // [M, 3d]
        form_kind(c, "last-skinny");
        if (in.S) {
            ln_pending(c, x, d, M, in, w.ln1g, w.ln1b, s.h);
            linear(c, s.h, d, M, w.wqkv, w.bqkv, 3 * d, d, qkv, 3 * d);
        } else {
            ln_linear(c, x, d, M, 1, 0, M, ln1_qkv(w, d), 3 * d, d, qkv, 3 * d, s.h, ACT_NONE, &in);
        }
        a.Q = qkv + (size_t)(n - 1) * 3 * d; a.ldq = 3 * d; a.u_qstride = n;      // query of sequence j = row j * n + n - 1
        a.K = qkv + d; a.ldk = 3 * d; a.V = qkv + 2 * d; a.ldv = 3 * d;
        a.u_ostride = 1;
    } else if (in.S) {
        form_kind(c, "last-split");
        ln_pending(c, x, d, M, in, w.ln1g, w.ln1b, s.h);
        linear(c, s.h, d, M, w.wqkv + (size_t)d * d, w.bqkv + d, 2 * d, d, kv, 2 * d);
        GemmP p{};
        p.X = s.h; p.ldx = d; p.Rx = M; p.a_mul = n; p.shift0 = n - 1; p.Cin = d; p.W = w.wqkv; p.bias = w.bqkv;
        p.C = q; p.ldc = d; p.M = A; p.N = d;
        gemm(c, p);
    } else {   // LN1 fused into both consumers: K|V of all rows, Q of the last row of each sequence
        form_kind(c, "last-fused");
        ln_linear(c, x, d, M, 1, 0, M, ln1_qkv(w, d, d), 2 * d, d, kv, 2 * d, s.h, ACT_NONE, &in);
        ln_linear(c, x, d, M, n, n - 1, A, ln1_qkv(w, d), d, d, q, d, s.f, ACT_NONE, &in);
    }
    if (!a.Q) {
        a.Q = q; a.ldq = d; a.K = kv; a.ldk = 2 * d; a.V = kv + d; a.ldv = 2 * d;
        a.u_qstride = 1;
    }
    a.O = att; a.ldo = d;
    a.u_qlen = 1; a.u_kvstride = n; a.u_kvlen = n; a.B = A; a.max_qlen = 1;
    MT2_HIP(launch_attention(a, c.s));
    form_note_attention(c, a);
    // y = x[last rows] + out_proj(att): the residual rows sit n*d floats apart starting at row n-1
    const Pending py = linear_residual(c, att, d, A, w.wo, w.bo, d, d, y, s.stat, x + (size_t)(n - 1) * d, n * d);
    ln_linear(c, y, d, A, 1, 0, A, ln2_ff0(w, d), e.ff, d, s.f, e.ff, s.h, ACT_RELU, &py);   // LN2 -> ff.0
    linear(c, s.f, e.ff, A, w.ff1w, w.ff1b, d, e.ff, y, d, y, d);
}

// FIRST layer: its input rows (embeddings + positional table of positions < t) never change between steps,
// so LN1 -> QKV of position i is computed once, at step i, into a per-sequence cache with a FIXED row
// stride (slot j owns rows [j*cs, j*cs + n)); every later step only adds row n-1.  Attention reads the
// cache and writes compact rows; the rest of the layer is the ordinary full-row form.
static Pending encoder_layer_first_cached(const Ctx& c, const EncW& e, const EncLayerW& w, float* x, int n, int A,
                                          float* qkv_cache, int cs, const EncScratch& s, bool fill_all) {
    MT2_REQUIRE(!e.conv_ff, "AR step layers use the Linear feed-forward");
    const int d = e.d, M = A * n;
    form_kind(c, fill_all && n > 1 ? "first-fill" : "first-incr");
    if (fill_all && n > 1) {
        // first step of a run that starts from a forced history (prompt prefix, teacher-forced tests): the cache
        // has no rows yet - LN1 -> QKV of ALL n rows, compact, then one strided copy into the cache layout
        ln_linear(c, x, d, M, 1, 0, M, ln1_qkv(w, d), 3 * d, d, s.qkv, 3 * d, s.h);
        MT2_HIP(launch_copy_2d(s.qkv, (long long)n * 3 * d, qkv_cache, (long long)cs * 3 * d, (long long)n * 3 * d, A,
                               c.s));
    } else {
        // LN1 -> QKV of the newest row of every active sequence, written into the cache at row stride cs
        ln_linear(c, x, d, M, n, n - 1, A, ln1_qkv(w, d), 3 * d, d, qkv_cache + (size_t)(n - 1) * 3 * d, cs * 3 * d, s.h);
    }
    AttnP a = attn_params(c, e);
    a.Q = qkv_cache; a.ldq = 3 * d; a.K = qkv_cache + d; a.ldk = 3 * d; a.V = qkv_cache + 2 * d; a.ldv = 3 * d;
    a.O = s.att; a.ldo = d;
    a.u_qstride = cs; a.u_qlen = n; a.u_kvstride = cs; a.u_kvlen = n; a.u_ostride = n;
    a.B = A; a.max_qlen = n;
    const bool opl = ar_outproj_takes_planes(c, e, w, x, M, s.att, s);
    a.o_planes = opl ? 1 : 0;
    MT2_HIP(launch_attention(a, c.s));
    form_note_attention(c, a);
    return ar_layer_tail(c, e, w, x, M, s.att, s, opl);
}

// One AR step of an encoder over A sequences of n positions (x: [A*n, d], overwritten); the rows the head
// needs (position n-1 of each sequence) are returned as a [A, d] matrix.
static const float* ar_step_layers(const Ctx& c, const EncW& e, float* x, int n, int A, float* qkv_cache, int cs,
                                   const EncScratch& sc, float* ylast, bool fill_cache = false) {
    const int L = (int)e.layers.size();
    const FormScope form_scope{c.m};
    AttnGeom g;
    g.u_stride = n; g.u_len = n; g.B = A; g.max_len = n;
    Pending pend;
    for (int l = 0; l < L; ++l) {
        if (l == L - 1) encoder_layer_last(c, e, e.layers[l], x, n, A, sc, ylast, pend);
        else if (l == 0 && qkv_cache) pend = encoder_layer_first_cached(c, e, e.layers[l], x, n, A, qkv_cache, cs, sc, fill_cache);
        else pend = encoder_layer_ar(c, e, e.layers[l], x, A * n, g, sc, pend);
    }
    return ylast;
}

// ---------------------------------------------------------------------------------------------------
// stage timers (HIP events on the caller's stream)

struct Stages {
    mt2_model& m;
    hipStream_t s;
    std::vector<hipEvent_t> ev;
    std::vector<std::string> names;
    explicit Stages(mt2_model& mm, hipStream_t ss) : m(mm), s(ss) {}
    // marker ids (tools/pmc_stage_summary.py): 0 start, 1 mrte, 2 adm, 3 regulate, 4 plm, 5 decoder, 6 vocoder,
    // 8 / 9 around mt2_vqpe_forward
    int nmark = 0;
    void mark(const char* name) {
        if (m.opts.markers) MT2_HIP(launch_stage_marker(nmark, s));
        ++nmark;
        if (!m.profiling) return;
        hipEvent_t e;
        MT2_HIP(hipEventCreate(&e));
        MT2_HIP(hipEventRecord(e, s));
        ev.push_back(e);
        names.push_back(name);
    }
    void finish() {
        if (!m.profiling || ev.empty()) return;
        MT2_HIP(hipEventSynchronize(ev.back()));
        m.stage_names.clear();
        m.stage_ms.clear();
        for (size_t i = 1; i < ev.size(); ++i) {
            float ms = 0.f;
            MT2_HIP(hipEventElapsedTime(&ms, ev[i - 1], ev[i]));
            m.stage_names.push_back(names[i]);
            m.stage_ms.push_back(ms);
        }
        for (auto e : ev) (void)hipEventDestroy(e);
        ev.clear();
    }
};

// ---------------------------------------------------------------------------------------------------
// ConvNetDouble (modules/convnet.py:156-210): first conv, N parallel branches (stack1 -> middle ->
// stack2) summed, last conv.  `middle` turns [G][Rin, C] into [G][Rout, C].

// MRTE mel encoder: middle = ONE shared Conv1d(C, C, stride+1, stride, pad stride/2) (mrte.py:101-107)
static float* mel_context_rows(const Ctx& c, const float* xmel, int ld_mel, RowSet& F, RowSet& X,
                               const int* d_rowbase) {
    mt2_model& m = c.m;
    const int C = m.cfg.mrte_hidden, G = m.mel_s1.groups;
    // zero padding IS the gap: no convolution may reach across it into a neighbour (prompt_mel_gap, mel_context_gap)
    require_gap(F, std::max({halo_of(m.mel_first.k), halo_of(m.mel_s1.k), m.cfg.mrte_stride / 2}));
    require_gap(X, std::max(halo_of(m.mel_s2.k), halo_of(m.mel_last.k)));
    const FormScope form_scope{m};
    form_kind(c, "mel-encoder");
    float* h0 = c.ws.get<float>((size_t)F.R * C);
    {
        GemmP p{};
        p.X = xmel; p.ldx = ld_mel; p.Rx = F.R; p.taps = m.mel_first.k; p.shift0 = -((m.mel_first.k - 1) / 2);
        p.Cin = m.mel_first.cin; p.W = m.mel_first.w; p.bias = m.mel_first.b; p.valid = F.d_valid;
        p.C = h0; p.ldc = C; p.M = F.R; p.N = C;
        gemm(c, p);
        form_note_conv(c, "first", p);
    }
    float* s1 = run_stack(c, m.mel_s1, h0, true, F.R, F.d_valid);
    float* mid = c.ws.get<float>((size_t)G * X.R * C);
    {
        GemmP p{};
        p.X = s1; p.strideX = (long long)F.R * C; p.ldx = C; p.Rx = F.R; p.rowbase = d_rowbase;
        p.taps = m.mel_mid.k; p.Cin = C; p.W = m.mel_mid.w; p.strideW = 0; p.bias = m.mel_mid.b; p.strideB = 0;
        p.valid = X.d_valid; p.C = mid; p.strideC = (long long)X.R * C; p.ldc = C; p.M = X.R; p.N = C; p.groups = G;
        gemm(c, p);
        form_note_conv(c, "mid", p);
    }
    float* s2 = run_stack(c, m.mel_s2, mid, false, X.R, X.d_valid);
    float* sum = c.ws.get<float>((size_t)X.R * C);
    MT2_HIP(launch_sum_groups(s2, (long long)X.R * C, G, C, sum, C, C, X.R, c.s));
    float* ctx = c.ws.get<float>((size_t)X.R * C);
    conv_same(c, sum, C, X.R, m.mel_last, ctx, C, X.d_valid, ACT_NONE, 0.f, ACT_NONE, nullptr, 0, 1, "last");
    return ctx;
}

struct MelPlan {
    RowSet F, X;
    int o_rowmapF, o_rowbase, o_rowmapX;
    RowPlanOffsets oF, oX;
};
static MelPlan plan_mel(IntPlan& ip, const mt2_config& cfg, const int* mel_lens, int B, int Tp_max, int Tc_max) {
    MelPlan mp;
    const int s = cfg.mrte_stride;
    mp.F = make_rows(mel_lens, B, prompt_mel_gap(cfg));
    std::vector<int> xl(B);
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(mel_lens[b] >= 1 && mel_lens[b] <= Tp_max, "prompt mel length out of range");
        xl[b] = (mel_lens[b] - 1) / s + 1;      // Conv1d(k = s+1, stride s, pad s/2) output length
    }
    mp.X = make_rows(xl.data(), B, mel_context_gap(cfg));
    mp.oF = plan_rows(ip, mp.F);
    mp.oX = plan_rows(ip, mp.X);
    mp.o_rowmapF = plan_rowmap(ip, mp.F, Tp_max);
    mp.o_rowmapX = plan_rowmap(ip, mp.X, Tc_max > 0 ? Tc_max : 1);
    std::vector<int> base(mp.X.R, kInvalidRow);
    for (int b = 0; b < B; ++b)
        for (int j = 0; j < xl[b]; ++j) base[mp.X.off[b] + j] = mp.F.off[b] + j * s - s / 2;
    mp.o_rowbase = ip.add(base);
    return mp;
}

// internal side streams (created once per handle) + fork / join events
static void ensure_aux(mt2_model& m, int n_streams) {
    while ((int)m.aux_streams.size() < n_streams) {
        hipStream_t s;
        MT2_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
        m.aux_streams.push_back(s);
    }
    if (!m.ev_fork) MT2_HIP(hipEventCreateWithFlags(&m.ev_fork, hipEventDisableTiming));
    while ((int)m.ev_join.size() < n_streams) {
        hipEvent_t e;
        MT2_HIP(hipEventCreateWithFlags(&e, hipEventDisableTiming));
        m.ev_join.push_back(e);
    }
}

// Range check of caller-supplied gather indices: the reference raises IndexError from nn.Embedding / F.embedding
// (modules/embedding.py:43-47, core_vq.py:188-190).  Here every gather kernel CLAMPS the id into its table (never an
// out-of-bounds read), and a tiny kernel per id tensor ORs a bit into a device flag.  The checks depend on the call's
// INPUTS only, so they run on the handle's own id stream, forked from the caller's stream at the first check of the
// call; the verdict (ids_verdict) is read at the END of the API call - a host wait for the id stream only, i.e. for
// what was queued on the caller's stream BEFORE this call, never for the call's own kernels.  A server can therefore
// enqueue batch k+1 behind batch k; the error still comes back from the call that carried the bad id.
enum IdBit { ID_PHONE = 1, ID_CODE = 2, ID_PREFIX = 4 };
static void ids_begin(const Ctx& c) {
    mt2_model& m = c.m;
    if (m.id_open) return;
    if (!m.id_stream) {     // all or nothing: a half-built set (stream without its events / flags) must never be used
        hipStream_t st = nullptr;
        hipEvent_t e0 = nullptr, e1 = nullptr;
        int *fd = nullptr, *fh = nullptr;
        const bool ok = hipStreamCreateWithFlags(&st, hipStreamNonBlocking) == hipSuccess &&
                        hipEventCreateWithFlags(&e0, hipEventDisableTiming) == hipSuccess &&
                        hipEventCreateWithFlags(&e1, hipEventDisableTiming) == hipSuccess &&
                        hipMalloc((void**)&fd, 4 * sizeof(int)) == hipSuccess &&
                        hipHostMalloc((void**)&fh, 4 * sizeof(int), hipHostMallocDefault) == hipSuccess;
        if (!ok) {
            if (fh) (void)hipHostFree(fh);
            if (fd) (void)hipFree(fd);
            if (e1) (void)hipEventDestroy(e1);
            if (e0) (void)hipEventDestroy(e0);
            if (st) (void)hipStreamDestroy(st);
            (void)hipGetLastError();
            throw Error("could not create the id-check stream, events or flags");
        }
        m.id_stream = st; m.ev_id_fork = e0; m.ev_id_done = e1; m.id_flag_dev = fd; m.id_flag_host = fh;
    }
    MT2_HIP(hipEventRecord(m.ev_id_fork, c.s));                  // the ids may be produced by earlier work on c.s
    MT2_HIP(hipStreamWaitEvent(m.id_stream, m.ev_id_fork, 0));
    MT2_HIP(hipMemsetAsync(m.id_flag_dev, 0, 4 * sizeof(int), m.id_stream));
    m.id_open = true;
}
// ids[map[r]] for r < R with map[r] >= 0 (map == nullptr: ids[r]); `map` is a HOST array, uploaded on the id stream
static void ids_check(const Ctx& c, const int64_t* ids, const std::vector<int>* map, long long R, long long hi, int bit) {
    MT2_REQUIRE(R < (1ll << 31), "id tensor too large");
    if (R <= 0) return;
    ids_begin(c);
    const int* dmap = nullptr;
    if (map) {
        MT2_REQUIRE((long long)map->size() >= R, "id map shorter than the id range");
        int* hm = static_cast<int*>(c.m.pinned().alloc((size_t)R * sizeof(int)));
        std::memcpy(hm, map->data(), (size_t)R * sizeof(int));
        int* dm = c.ws.get<int>((size_t)R);
        MT2_HIP(hipMemcpyAsync(dm, hm, (size_t)R * sizeof(int), hipMemcpyHostToDevice, c.m.id_stream));
        dmap = dm;
    }
    MT2_HIP(launch_check_ids(ids, dmap, (int)R, hi, c.m.id_flag_dev, bit, c.m.id_stream));
}
// end of the API call (also on its error paths, without throwing: CallScope): wait for the id stream, read the flag
static int ids_wait(mt2_model& m) {
    if (!m.id_open) return 0;
    m.id_open = false;
    *m.id_flag_host = 0;
    if (hipMemcpyAsync(m.id_flag_host, m.id_flag_dev, sizeof(int), hipMemcpyDeviceToHost, m.id_stream) != hipSuccess) return -1;
    if (hipEventRecord(m.ev_id_done, m.id_stream) != hipSuccess) return -1;
    if (hipEventSynchronize(m.ev_id_done) != hipSuccess) return -1;
    return *m.id_flag_host;
}
static void ids_verdict(const Ctx& c) {
    const int f = ids_wait(c.m);
    MT2_REQUIRE(f >= 0, "id range check could not be read back");
    if (f == 0) return;
    std::string what = "index out of range in embedding lookup:";
    if (f & ID_PHONE) what += " phone id >= phone_vocab_size (or negative);";
    if (f & ID_CODE) what += " prosody code >= vq_bins (or negative);";
    if (f & ID_PREFIX) what += " prompt prosody code >= vq_bins + 2 (or negative);";
    throw Error(what);
}

// MRTE.tc_latent (modules/mrte.py:154-171) -> packed rows [P.R, hidden] (gap rows zero)
// Several phone sequences per utterance may share ONE mel context (prompt-conditioned synthesis: the target's phones and the
// prompt's own phones against the same prompt mel, modules/datamodule.py:161-177): sequence s * B + b = set s, utterance b.
struct TcResult { float* rows; RowSet P; };
struct PhoneSet { const int64_t* ids; const int* lens; int Np_max; };
static TcResult tc_latent_rows(const Ctx& c, const std::vector<PhoneSet>& sets, const float* mel, const int* mel_lens,
                               int Tp_max, int B) {
    mt2_model& m = c.m;
    const mt2_config& cfg = m.cfg;
    const int H = cfg.mrte_hidden, S = (int)sets.size(), BS = B * S;
    IntPlan ip;
    MelPlan mp = plan_mel(ip, cfg, mel_lens, B, Tp_max, 0);
    std::vector<int> all_lens(BS);
    for (int s_ = 0; s_ < S; ++s_)
        for (int b = 0; b < B; ++b) {
            MT2_REQUIRE(sets[s_].lens[b] >= 1 && sets[s_].lens[b] <= sets[s_].Np_max, "phone length out of range");
            all_lens[s_ * B + b] = sets[s_].lens[b];
        }
    RowSet P = make_rows(all_lens.data(), BS, phone_gap(cfg));
    require_gap(P, halo_of(5));                       // the conv-FF kernel of encoder_layer
    const FormScope form_scope{m};
    MT2_REQUIRE(P.maxlen <= cfg.max_positions, "phone sequence longer than the positional table");
    RowPlanOffsets oP = plan_rows(ip, P);
    std::vector<int> idmap(P.R, -1);                 // row -> index into ITS SET's padded [B, Np_max] id tensor (gap rows: -1)
    std::vector<int> pos(P.R, 0);
    for (int s_ = 0; s_ < S; ++s_)
        for (int b = 0; b < B; ++b) {
            const int q = s_ * B + b;
            for (int t = 0; t < P.len[q]; ++t) {
                idmap[P.off[q] + t] = b * sets[s_].Np_max + t;
                pos[P.off[q] + t] = t;
            }
        }
    const int o_idmap = ip.add(idmap);
    const int o_pos = ip.add(pos);
    // cross attention: sequence q reads the mel context of utterance q % B
    std::vector<int> kvs(BS), kvl(BS);
    int o_kvs = -1, o_kvl = -1;
    ip.upload(c.ws, c.m.pinned(), c.s);
    bind_rows(ip, mp.oF, mp.F);
    bind_rows(ip, mp.oX, mp.X);
    bind_rows(ip, oP, P);
    IntPlan ip2;                                      // kv ranges need mp.X's offsets: a second (tiny) plan when S > 1
    if (S > 1) {
        for (int q = 0; q < BS; ++q) { kvs[q] = mp.X.off[q % B]; kvl[q] = mp.X.len[q % B]; }
        o_kvs = ip2.add(kvs); o_kvl = ip2.add(kvl);
        ip2.upload(c.ws, c.m.pinned(), c.s);
    }
    // phone ids index the embedding table: range check on the id stream (verdict at the end of the API call)
    for (int s_ = 0; s_ < S; ++s_) {
        const int r0 = P.off[s_ * B] - P.G, r1 = s_ + 1 < S ? P.off[(s_ + 1) * B] - P.G : P.R;
        std::vector<int> sub(idmap.begin() + r0, idmap.begin() + r1);
        ids_check(c, sets[s_].ids, &sub, (long long)sub.size(), cfg.phone_vocab, ID_PHONE);
    }

    // The phone branch (embedding, conv-FF transformer, query projection: ~60 small launches) does not depend on
    // the mel encoder: it runs on a side stream and fills the CUs the mel stack's big launches leave idle
    // (220 tiles on 256 CUs); the two meet at the cross attention.
    ensure_aux(m, 1);
    hipStream_t side = m.aux_streams[0];
    MT2_HIP(hipEventRecord(m.ev_fork, c.s));
    m.aux_forked = true;
    MT2_HIP(hipStreamWaitEvent(side, m.ev_fork, 0));
    const Ctx cp{m, side, c.ws};

    // prompt mel -> rows, mel encoder
    float* xmel = c.ws.get<float>((size_t)mp.F.R * cfg.mel_bins);
    MT2_HIP(launch_pack_rows(mel, cfg.mel_bins, Tp_max, 0, ip.dev(mp.o_rowmapF), xmel, cfg.mel_bins, mp.F.R, c.s));
    float* ctx = mel_context_rows(c, xmel, cfg.mel_bins, mp.F, mp.X, ip.dev(mp.o_rowbase));

    // phone embedding + PE, conv-FF transformer (mrte.py:159-160,165)
    float* x = c.ws.get<float>((size_t)P.R * H);
    for (int s_ = 0; s_ < S; ++s_) {                  // one embedding launch per id tensor, over that set's rows
        const int r0 = P.off[s_ * B] - P.G, r1 = s_ + 1 < S ? P.off[(s_ + 1) * B] - P.G : P.R;
        MT2_HIP(launch_embed_pe(m.phone_emb, H, sets[s_].ids, ip.dev(o_idmap) + r0, ip.dev(o_pos) + r0, m.pe_mrte,
                                x + (size_t)r0 * H, H, r1 - r0, cfg.phone_vocab, side));
    }
    EncScratch sc = enc_scratch(c, m.phone_enc, P.R);
    AttnGeom g;
    g.start = P.d_start; g.len = P.d_len; g.B = BS; g.max_len = P.maxlen;
    form_kind(c, "phone-encoder");                    // (mel_context_rows has left no kind behind)
    for (auto& lw : m.phone_enc.layers) encoder_layer(cp, m.phone_enc, lw, x, P.R, g, P.d_valid, sc);

    // cross attention, ONE head of width H (mrte.py:131-135,167), LayerNorm, ReLU (:168-169)
    form_kind(c, "cross");
    float* q = sc.h;
    linear(cp, x, H, P.R, m.x_wq, m.x_bq, H, H, q, H);
    form_note_linear(c, "q", P.R, H, H);
    MT2_HIP(hipEventRecord(m.ev_join[0], side));
    MT2_HIP(hipStreamWaitEvent(c.s, m.ev_join[0], 0));
    float* kv = c.ws.get<float>((size_t)mp.X.R * 2 * H);
    linear(c, ctx, H, mp.X.R, m.x_wkv, m.x_bkv, 2 * H, H, kv, 2 * H);
    form_note_linear(c, "kv", mp.X.R, 2 * H, H);
    AttnP a = attn_params(c, 1, H);
    a.Q = q; a.ldq = H; a.K = kv; a.ldk = 2 * H; a.V = kv + H; a.ldv = 2 * H; a.O = sc.att; a.ldo = H;
    a.q_start = P.d_start; a.q_len = P.d_len;
    a.kv_start = S > 1 ? ip2.dev(o_kvs) : mp.X.d_start; a.kv_len = S > 1 ? ip2.dev(o_kvl) : mp.X.d_len;
    a.B = BS; a.max_qlen = P.maxlen; a.max_kvlen = mp.X.maxlen;
    MT2_HIP(launch_attention(a, c.s));
    form_note_attention(c, a);
    float* o = c.ws.get<float>((size_t)P.R * H);
    linear(c, sc.att, H, P.R, m.x_wo, m.x_bo, H, H, o, H);
    form_note_linear(c, "out", P.R, H, H);
    float* tc = c.ws.get<float>((size_t)P.R * H);
    layernorm(c, o, H, m.x_ng, m.x_nb, P.R, H, tc, H, P.d_valid, 0, nullptr, 0, 0, 0, ACT_RELU);
    form_note(c, "ln", "plain", "out_planes=0 act=1 M=%d groups=1", P.R);
    return {tc, P};
}
static TcResult tc_latent_rows(const Ctx& c, const int64_t* phone, const int* phone_lens, int Np_max,
                               const float* mel, const int* mel_lens, int Tp_max, int B) {
    return tc_latent_rows(c, std::vector<PhoneSet>{{phone, phone_lens, Np_max}}, mel, mel_lens, Tp_max, B);
}

// ---------------------------------------------------------------------------------------------------
// autoregressive models.  Utterances are visited in order of decreasing length so that the sequences
// still active at step t are always slots [0, A_t); at step t every active sequence has exactly
// n = t+1 positions, stored compactly as rows j*n + i.  ALL positions are re-encoded every step,
// non-causally, exactly as the reference does (models/megatts2.py:172-179,264-273) -
// a KV cache would change the result.

// per-stage value of an engine option for the duration of a stage driver (restored on every exit path)
struct OptGuard {
    int& slot; int saved;
    OptGuard(int& s_, int v) : slot(s_), saved(s_) { if (v >= 0) slot = v; }
    ~OptGuard() { slot = saved; }
};
struct ArOrder {
    std::vector<int> slot_b, len;   // slot j -> utterance, length
    int nmax = 0;
};
static ArOrder ar_order(const int* lens, int B) {
    ArOrder o;
    o.slot_b.resize(B);
    std::iota(o.slot_b.begin(), o.slot_b.end(), 0);
    std::stable_sort(o.slot_b.begin(), o.slot_b.end(), [&](int a, int b) { return lens[a] > lens[b]; });
    o.len.resize(B);
    for (int j = 0; j < B; ++j) o.len[j] = lens[o.slot_b[j]];
    o.nmax = B ? o.len[0] : 0;
    return o;
}

// ---- stream groups.  The sequences of an AR run are dealt round-robin (in length order) into G groups and
// every group runs its own step loop on its own HIP stream.  Nothing changes arithmetically - sequences are
// independent (batch-1 semantics) - but two independent kernel chains are in flight: one chain's launch
// boundary, workgroup-tail and prologue bubbles (~5 us fixed per launch, and the idle CUs of a launch whose
// tile count is not a multiple of the chip) are filled by the other chain's kernels.
struct ArGroups {
    int G = 1;
    std::vector<std::vector<int>> slots;   // group -> positions in the length-sorted order
    std::vector<hipStream_t> stream;
};
static ArGroups ar_groups(mt2_model& m, hipStream_t main, const ArOrder& ord, int B, int stage_groups = 0) {
    ArGroups g;
    g.G = std::max(1, std::min(stage_groups > 0 ? stage_groups : m.ar_groups, B));
    g.slots.resize(g.G);
    for (int j = 0; j < B; ++j) g.slots[j % g.G].push_back(j);
    ensure_aux(m, g.G - 1);
    g.stream.push_back(main);
    for (int i = 1; i < g.G; ++i) g.stream.push_back(m.aux_streams[i - 1]);
    return g;
}
static void ar_fork(mt2_model& m, const ArGroups& g) {
    if (g.G <= 1) return;
    MT2_HIP(hipEventRecord(m.ev_fork, g.stream[0]));
    m.aux_forked = true;
    for (int i = 1; i < g.G; ++i) MT2_HIP(hipStreamWaitEvent(g.stream[i], m.ev_fork, 0));
}
static void ar_join(mt2_model& m, const ArGroups& g) {
    for (int i = 1; i < g.G; ++i) {
        MT2_HIP(hipEventRecord(m.ev_join[i - 1], g.stream[i]));
        MT2_HIP(hipStreamWaitEvent(g.stream[0], m.ev_join[i - 1], 0));
    }
}

// A run may start from a FORCED history of P positions per sequence (uniform P): the PLM's prompt prefix (SURVEY 8f
// row f1: the layout the PLM is trained on, modules/datamodule.py:201-212) and the teacher-forced single steps of
// the long-shape parity tests.  The loop then starts at t = P and runs `max_steps` steps (0 = to the end).
struct ArPrefix {
    int P = 0;
    const void* data = nullptr;   // ADM: float [B, P] un-rounded predictions; PLM: int64 [B, P] prosody codes
    int max_steps = 0;
    int stride = 0;               // PLM: row stride of `data` in elements (0: P)
};

// ---- one driver for both AR models.  ar_run owns what they share: the length order, the stream groups with their integer
// plan (first input row, length, utterance of every sequence), history-independent scratch, fork / join and the step loop;
// a stage (AdmStage / PlmStage below, resolved at compile time - nothing is type-erased or allocated per step) supplies
//   plan(ip)                  its own integers of the call's plan, before the upload
//   begin(c, hstride, B)      what runs in front of the groups on the caller's stream; the history buffer [B, hstride]
//   init_hist(c, ip, q)       the history rows of group q (and the group's stage-specific scratch)
//   step_input(cg, ip, q, n)  x rows of the A active sequences at n positions
//   head(cg, ip, q, y, n, t)  position n of the history from the last-position rows y [A, d]
//   finalize(ip, q, s)        the group's results into the caller's buffers
// Pair mode (per = 2: prosody interpolation, PlmStage): every utterance contributes TWO sequences of its length, decoded in lock
// step - context A then context B, adjacent in their group at rows 2j and 2j + 1 of everything a step touches.  lens / the
// length order / the deal into groups stay per UTTERANCE and are then expanded, so a pair is never split across chains and the
// active set shrinks by whole pairs; row0 has per * B entries and sequence s of utterance b is id s * B + b (its row0, its slot
// in q.slot: prefix row, logits row).  per = 1 is every other call: the same plan, launches and arguments as before.
struct ArGrp {
    int g = 0, first = 0;                   // group index; sequences in the groups before it (row of the run's history buffer)
    int B = 0, nmax = 0, A = 0;             // sequences, positions of the longest, sequences still active
    int o_row = 0, o_len = 0, o_slot = 0;   // plan offsets
    int o_ulen = -1, o_uslot = -1;          // pair mode: length and utterance of every PAIR of the group
    std::vector<int> len, slot;
    float *x = nullptr, *ylast = nullptr, *qkv0 = nullptr; EncScratch sc{};
};
template <class Stage>
static void ar_run(const Ctx& c, const EncW& e, const std::vector<int>& row0, const int* lens, int B, int stage_groups,
                   const ArPrefix& pre, Stage& st, int per = 1) {
    mt2_model& m = c.m;
    const int d = e.d;
    const ArOrder ord = ar_order(lens, B);
    const ArGroups grp = ar_groups(m, c.s, ord, B, stage_groups);
    std::vector<ArGrp> gs(grp.G);
    IntPlan ip;
    for (int g = 0, first = 0; g < grp.G; ++g) {
        ArGrp& q = gs[g];
        q.g = g; q.first = first;
        std::vector<int> row, ulen, uslot;
        for (int j : grp.slots[g])
            for (int sq = 0; sq < per; ++sq) {
                row.push_back(row0[sq * B + ord.slot_b[j]]);
                q.len.push_back(ord.len[j]);
                q.slot.push_back(sq * B + ord.slot_b[j]);
            }
        q.B = q.A = (int)q.len.size();
        q.nmax = q.len[0];
        first += q.B;
        q.o_row = ip.add(row); q.o_len = ip.add(q.len); q.o_slot = ip.add(q.slot);
        if (per > 1) {
            for (int j : grp.slots[g]) { ulen.push_back(ord.len[j]); uslot.push_back(ord.slot_b[j]); }
            q.o_ulen = ip.add(ulen); q.o_uslot = ip.add(uslot);
        }
    }
    st.plan(ip);
    ip.upload(c.ws, c.m.pinned(), c.s);
    st.begin(c, ord.nmax + 1, per * B);
    for (ArGrp& q : gs) {
        const int Mmax = q.B * q.nmax;
        st.init_hist(c, ip, q);
        q.x = c.ws.get<float>((size_t)Mmax * d);
        q.sc = enc_scratch(c, e, std::max(Mmax, 2 * q.B));   // last layer: q | att rows of A sequences
        q.ylast = c.ws.get<float>((size_t)q.B * d);
        q.qkv0 = e.layers.size() >= 2 ? c.ws.get<float>((size_t)Mmax * 3 * d) : nullptr;   // layer-0 QKV cache
    }
    ar_fork(m, grp);
    const int t_end = pre.max_steps > 0 ? std::min(ord.nmax, pre.P + pre.max_steps) : ord.nmax;
    for (int t = pre.P; t < t_end; ++t)        // interleaved: all chains' queues are fed step by step
        for (int g = 0; g < grp.G; ++g) {
            ArGrp& q = gs[g];
            while (q.A > 0 && q.len[q.A - 1] <= t) --q.A;
            if (q.A == 0) continue;
            const int n = t + 1;
            const Ctx cg{m, grp.stream[g], c.ws};
            st.step_input(cg, ip, q, n);
            const float* y = ar_step_layers(cg, e, q.x, n, q.A, q.qkv0, q.nmax, q.sc, q.ylast, t == pre.P && pre.P > 0);
            st.head(cg, ip, q, y, n, t);
        }
    for (int g = 0; g < grp.G; ++g) st.finalize(ip, gs[g], grp.stream[g]);
    ar_join(m, grp);
}
static int longest(const int* lens, int B) { return B > 0 ? *std::max_element(lens, lens + B) : 0; }

// MegaADM.infer (models/megatts2.py:257-275).  tc: rows buffer (ld), utterance b's first row row0[b].
struct AdmStage {
    mt2_model& m; const float* tc; int ld_tc, tc_rows; const ArPrefix& pre;
    int32_t* dur_out; float* flt_out; int dstride;
    float *tcemb = nullptr, *p_all = nullptr; int pstride = 0;
    float* p(const ArGrp& q) const { return p_all + (size_t)q.first * pstride; }
    void plan(IntPlan&) {}
    void begin(const Ctx& c, int hstride, int B) {
        const int Dc = m.cfg.adm_tc_emb_dim;
        tcemb = c.ws.get<float>((size_t)tc_rows * Dc);
        linear(c, tc, ld_tc, tc_rows, m.adm_wtc, nullptr, Dc, m.cfg.adm_tc_dim, tcemb, Dc);   // tc_linear_emb (no bias)
        pstride = hstride;
        p_all = c.ws.get<float>((size_t)B * pstride);
    }
    void init_hist(const Ctx& c, const IntPlan& ip, const ArGrp& q) {      // p_code starts at 0.0 (:262), followed by the forced history if any
        MT2_HIP(launch_adm_init_hist(p(q), pstride, static_cast<const float*>(pre.data), pre.P, ip.dev(q.o_slot), q.B, c.s));
    }
    void step_input(const Ctx& cg, const IntPlan& ip, const ArGrp& q, int n) {
        MT2_HIP(launch_adm_step_input(tcemb, m.cfg.adm_tc_emb_dim, ip.dev(q.o_row), m.adm_wdt, p(q), pstride, m.pe_adm, q.x,
                                      m.cfg.adm_tc_emb_dim, m.cfg.adm_emb_dim, n, q.A, cg.s));
    }
    void head(const Ctx& cg, const IntPlan&, const ArGrp& q, const float* y, int n, int) {
        MT2_HIP(launch_adm_predict(y, m.adm_enc.d, m.adm_wpred, p(q), pstride, n, 1, q.A, cg.s));
    }
    void finalize(const IntPlan& ip, const ArGrp& q, hipStream_t s) {
        MT2_HIP(launch_adm_finalize(p(q), pstride, ip.dev(q.o_len), ip.dev(q.o_slot), dur_out, flt_out, dstride, q.B,
                                    dstride < q.nmax ? dstride : q.nmax, s));
    }
};
static void adm_run(const Ctx& c, const float* tc, int ld_tc, int tc_rows, const std::vector<int>& row0,
                    const int* lens, int B, int32_t* dur_out, float* flt_out, int dstride,
                    const ArPrefix& pre = ArPrefix()) {
    mt2_model& m = c.m;
    const OptGuard pairs_guard(m.opts.ln_pairs, m.opts.ln_pairs_adm);
    MT2_REQUIRE(longest(lens, B) <= m.cfg.max_positions, "ADM sequence longer than the positional table");
    for (int b = 0; b < B; ++b) MT2_REQUIRE(lens[b] > pre.P, "forced history is not shorter than the sequence");
    AdmStage st{m, tc, ld_tc, tc_rows, pre, dur_out, flt_out, dstride};
    ar_run(c, m.adm_enc, row0, lens, B, m.adm_groups, pre, st);
}

// MegaPLM.infer (models/megatts2.py:165-181).  cond rows buffer (ld), utterance b's first row row0[b]; lens[b] =
// ALL positions of the sequence (prompt prefix + target); codes_out / last_logits receive the target positions.
// smp (validated by the caller; nullptr = greedy): each step's code is drawn by launch_sample_rows instead of the argmax -
// the same launch count, utterance b's seed smp->seeds[b], counter = the target position t - P.
// gamma (host f32 [nseq], validated by the caller; nullptr = one sequence per utterance): ar_run's pair mode.  The head's GEMM
// covers the 2A rows of the A active pairs and ONE launch_sample_mix_rows (greedy on the mixture without smp) replaces the sampler /
// arg-max: the code of pair j goes to both histories.  gamma travels with the plan, bit-cast, as the seeds do.
struct PlmStage {
    mt2_model& m; const float* cond; int ld_c; int nseq; const ArPrefix& pre; const mt2_sampling* smp;
    int64_t* codes_out; int ostride; float* last_logits; int logit_tmax; const float* gamma = nullptr;
    int64_t* codes_all = nullptr; int cstride = 0, o_seed = -1, o_gamma = -1;
    std::vector<float*> logits;      // per group: [B, bins]
    int64_t* codes(const ArGrp& q) const { return codes_all + (size_t)q.first * cstride; }
    void plan(IntPlan& ip) {
        if (gamma) {
            std::vector<int> gm(nseq);
            std::memcpy(gm.data(), gamma, sizeof(float) * (size_t)nseq);
            o_gamma = ip.add(gm);
        }
        if (!smp) return;       // (lo, hi) words of every utterance's seed, uploaded once per call with the plan
        std::vector<int> sd(2 * (size_t)nseq);
        for (int b = 0; b < nseq; ++b) {
            sd[2 * b] = (int)(uint32_t)smp->seeds[b];
            sd[2 * b + 1] = (int)(uint32_t)(smp->seeds[b] >> 32);
        }
        o_seed = ip.add(sd);
    }
    void begin(const Ctx& c, int hstride, int B) {
        cstride = hstride;
        codes_all = c.ws.get<int64_t>((size_t)B * cstride);
    }
    void init_hist(const Ctx& c, const IntPlan& ip, const ArGrp& q) {
        // BOS literal 1024 (models/megatts2.py:170), then the prompt's codes if any - on the device, no host staging
        MT2_HIP(launch_plm_init_hist(codes(q), cstride, 1024, static_cast<const int64_t*>(pre.data), pre.P,
                                     pre.stride > 0 ? pre.stride : pre.P, ip.dev(q.o_slot), q.B, c.s));
        logits.push_back(c.ws.get<float>((size_t)q.B * m.cfg.plm_bins));
    }
    void step_input(const Ctx& cg, const IntPlan& ip, const ArGrp& q, int n) {
        MT2_HIP(launch_plm_step_input(cond, ld_c, ip.dev(q.o_row), m.plm_emb, codes(q), cstride, m.pe_plm, q.x, m.cfg.plm_tc_dim,
                                      m.cfg.plm_vq_dim, n, q.A, m.cfg.plm_bins + 2, cg.s));
    }
    void head(const Ctx& cg, const IntPlan& ip, const ArGrp& q, const float* y, int n, int t) {
        // predict_layer on the last position of each sequence only (:178 takes [:, -1:]), then argmax (or the seeded draw)
        const int d = m.plm_enc.d, NB = m.cfg.plm_bins;
        float* lg = logits[q.g];
        GemmP p{};
        p.X = y; p.ldx = d; p.Rx = q.A; p.Cin = d; p.W = m.plm_wpred;
        p.C = lg; p.ldc = NB; p.M = q.A; p.N = NB;
        gemm(cg, p);
        if (gamma)
            MT2_HIP(launch_sample_mix_rows(lg, NB, NB, codes(q), cstride, n, q.A / 2, !smp, smp ? smp->temperature : 1.0f,
                                           smp ? smp->top_k : 0, smp ? smp->top_p : 1.0f,
                                           smp ? reinterpret_cast<const uint32_t*>(ip.dev(o_seed)) : nullptr, ip.dev(q.o_uslot),
                                           nullptr, t - pre.P, reinterpret_cast<const float*>(ip.dev(o_gamma)), cg.s));
        else if (smp)
            MT2_HIP(launch_sample_rows(lg, NB, NB, codes(q), cstride, n, q.A, smp->temperature, smp->top_k, smp->top_p,
                                       reinterpret_cast<const uint32_t*>(ip.dev(o_seed)), ip.dev(q.o_slot), nullptr, t - pre.P,
                                       cg.s));
        else
            MT2_HIP(launch_argmax_rows(lg, NB, NB, codes(q), cstride, n, q.A, cg.s));
        if (last_logits && t - pre.P < logit_tmax)
            for (int j = 0; j < q.A; ++j)
                MT2_HIP(hipMemcpyAsync(last_logits + ((size_t)q.slot[j] * logit_tmax + (t - pre.P)) * NB, lg + (size_t)j * NB,
                                       sizeof(float) * NB, hipMemcpyDeviceToDevice, cg.s));
    }
    void finalize(const IntPlan& ip, const ArGrp& q, hipStream_t s) {
        const int nt = q.nmax - pre.P;
        if (gamma) {      // context A's history (every second row): the generated parts of a pair are identical
            MT2_HIP(launch_plm_finalize(codes(q), 2 * cstride, ip.dev(q.o_ulen), ip.dev(q.o_uslot), codes_out, ostride, q.B / 2,
                                        ostride < nt ? ostride : nt, pre.P, s));
            return;
        }
        MT2_HIP(launch_plm_finalize(codes(q), cstride, ip.dev(q.o_len), ip.dev(q.o_slot), codes_out, ostride, q.B,
                                    ostride < nt ? ostride : nt, pre.P, s));
    }
};
static void plm_run(const Ctx& c, const float* cond, int ld_c, const std::vector<int>& row0, const int* lens, int B,
                    int64_t* codes_out, int ostride, float* last_logits, int logit_tmax,
                    const ArPrefix& pre = ArPrefix(), const mt2_sampling* smp = nullptr, const float* gamma = nullptr) {
    mt2_model& m = c.m;
    const OptGuard pairs_guard(m.opts.ln_pairs, 0);      // the hand-off pays in the ADM only (profiles/r05_opts_ab.txt)
    MT2_REQUIRE(longest(lens, B) <= m.cfg.max_positions, "PLM sequence longer than the positional table");
    MT2_REQUIRE(1024 < m.cfg.plm_bins + 2, "pc_embedding too small for the BOS id 1024");
    for (int b = 0; b < B; ++b) MT2_REQUIRE(lens[b] > pre.P, "prompt prefix is not shorter than the sequence");
    PlmStage st{m, cond, ld_c, B, pre, smp, codes_out, ostride, last_logits, logit_tmax, gamma};
    ar_run(c, m.plm_enc, row0, lens, B, m.plm_groups, pre, st, gamma ? 2 : 1);
}

// ---------------------------------------------------------------------------------------------------
// length regulation, PLM conditioning, decoder

struct FramePlan {
    RowSet D;                 // mel frames, gap decoder_gap
    std::vector<int> tq;      // prosody tokens per utterance
    std::vector<int> q_row0;  // first cond row of each utterance (compact, no gaps)
    int Qrows = 0;
    int o_tcmap, o_codemap, o_first, o_cnt, o_rowmapD;
    RowPlanOffsets oD;
};
// dur: host [B, dstride]; tc rows of utterance b start at tc_row0[b]; codes are addressed as b*code_stride + q
static FramePlan plan_frames(IntPlan& ip, const mt2_config& cfg, const int* dur, int dstride, const int* lens, int B,
                             const std::vector<int>& tc_row0, int pool, int code_stride, int out_stride) {
    FramePlan fp;
    std::vector<int> tm(B);
    for (int b = 0; b < B; ++b) {
        long long s = 0;
        for (int i = 0; i < lens[b]; ++i) {
            MT2_REQUIRE(dur[(size_t)b * dstride + i] >= 0, "negative duration");
            s += dur[(size_t)b * dstride + i];
        }
        MT2_REQUIRE(s < (1 << 24), "utterance too long");
        tm[b] = (int)s;
    }
    fp.D = make_rows(tm.data(), B, decoder_gap(cfg));
    fp.oD = plan_rows(ip, fp.D);
    fp.o_rowmapD = plan_rowmap(ip, fp.D, out_stride > 0 ? out_stride : 1);
    std::vector<int> tcmap(fp.D.R, -1), codemap(fp.D.R, -1);
    fp.tq.resize(B);
    fp.q_row0.resize(B);
    int qr = 0;
    for (int b = 0; b < B; ++b) {
        int f = 0;
        for (int i = 0; i < lens[b]; ++i)                       // create_alignment, mrte.py:23-31
            for (int k = 0; k < dur[(size_t)b * dstride + i]; ++k, ++f) {
                tcmap[fp.D.off[b] + f] = tc_row0[b] + i;
                codemap[fp.D.off[b] + f] = b * code_stride + f / pool;
            }
        fp.tq[b] = (tm[b] + pool - 1) / pool;
        fp.q_row0[b] = qr;
        qr += fp.tq[b];
    }
    fp.Qrows = qr;
    std::vector<int> first(qr > 0 ? qr : 1, 0), cnt(qr > 0 ? qr : 1, 0);
    for (int b = 0; b < B; ++b)
        for (int q = 0; q < fp.tq[b]; ++q) {
            first[fp.q_row0[b] + q] = fp.D.off[b] + q * pool;
            cnt[fp.q_row0[b] + q] = std::min(pool, tm[b] - q * pool);    // ceil_mode: partial last window
        }
    fp.o_tcmap = ip.add(tcmap);
    fp.o_codemap = ip.add(codemap);
    fp.o_first = ip.add(first);
    fp.o_cnt = ip.add(cnt);
    return fp;
}

// ConvNet.forward (modules/convnet.py:115-119) on rows xdec [D.R, decoder_in] -> mel rows [D.R, mel_bins]
static float* decoder_rows(const Ctx& c, const float* xdec, const RowSet& D) {
    mt2_model& m = c.m;
    const int H = m.cfg.dec_hidden, DIN = m.dec_first.cin;
    require_gap(D, std::max({halo_of(m.dec_first.k), halo_of(m.dec_stack.k), halo_of(m.dec_last.k)}));      // decoder_gap
    const FormScope form_scope{m};
    form_kind(c, "decoder");
    float* h0 = c.ws.get<float>((size_t)D.R * H);
    conv_same(c, xdec, DIN, D.R, m.dec_first, h0, H, D.d_valid, ACT_NONE, 0.f, ACT_NONE, nullptr, 0, 1, "first");
    float* s = run_stack(c, m.dec_stack, h0, true, D.R, D.d_valid);
    float* mel = c.ws.get<float>((size_t)D.R * m.cfg.mel_bins);
    conv_same(c, s, H, D.R, m.dec_last, mel, m.cfg.mel_bins, D.d_valid, ACT_NONE, 0.f, ACT_NONE, nullptr, 0, 1, "last");
    return mel;
}

// ---------------------------------------------------------------------------------------------------
// VQ prosody encoder (modules/vqpe.py:50-62)

struct VqpeResult { float* ze; int64_t* idx; RowSet F, Q; int o_rowmapQ, o_rowmapF, o_codemapF; };
static VqpeResult vqpe_rows(const Ctx& c, IntPlan& ip, const float* mel, int mel_ld, const int* lens, int T_max,
                            int Tq_max, int B) {
    mt2_model& m = c.m;
    const mt2_config& cfg = m.cfg;
    const int C = cfg.vq_hidden, G = m.vq_s1.groups, st = cfg.vq_stride, Dq = cfg.vq_dim;
    VqpeResult r;
    r.F = make_rows(lens, B, vqpe_gap(cfg));
    std::vector<int> ql(B);
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(lens[b] >= 1 && lens[b] <= T_max, "mel length out of range");
        ql[b] = (lens[b] + st - 1) / st;
    }
    r.Q = make_rows(ql.data(), B, vqpe_gap(cfg));
    require_gap(r.F, std::max(halo_of(m.vq_first.k), halo_of(m.vq_s1.k)));
    require_gap(r.Q, std::max(halo_of(m.vq_s2.k), halo_of(m.vq_last.k)));
    const FormScope form_scope{m};
    form_kind(c, "vqpe");
    RowPlanOffsets oF = plan_rows(ip, r.F), oQ = plan_rows(ip, r.Q);
    r.o_rowmapF = plan_rowmap(ip, r.F, T_max);
    r.o_rowmapQ = plan_rowmap(ip, r.Q, Tq_max);
    std::vector<int> first(r.Q.R, 0), cnt(r.Q.R, 0), codemap(r.F.R, -1);
    for (int b = 0; b < B; ++b) {
        for (int q = 0; q < ql[b]; ++q) {
            first[r.Q.off[b] + q] = r.F.off[b] + q * st;
            cnt[r.Q.off[b] + q] = std::min(st, lens[b] - q * st);
        }
        for (int t = 0; t < lens[b]; ++t) codemap[r.F.off[b] + t] = r.Q.off[b] + t / st;
    }
    const int o_first = ip.add(first), o_cnt = ip.add(cnt);
    r.o_codemapF = ip.add(codemap);
    ip.upload(c.ws, c.m.pinned(), c.s);
    bind_rows(ip, oF, r.F);
    bind_rows(ip, oQ, r.Q);

    float* xmel = c.ws.get<float>((size_t)r.F.R * mel_ld);
    MT2_HIP(launch_pack_rows(mel, mel_ld, T_max, 0, ip.dev(r.o_rowmapF), xmel, mel_ld, r.F.R, c.s));
    float* h0 = c.ws.get<float>((size_t)r.F.R * C);
    {   // first_layer reads only the first vq_mel_bins columns (vqpe.py:55)
        GemmP p{};
        p.X = xmel; p.ldx = mel_ld; p.Rx = r.F.R; p.taps = m.vq_first.k; p.shift0 = -((m.vq_first.k - 1) / 2);
        p.Cin = m.vq_first.cin; p.W = m.vq_first.w; p.bias = m.vq_first.b; p.valid = r.F.d_valid;
        p.C = h0; p.ldc = C; p.M = r.F.R; p.N = C;
        gemm(c, p);
        form_note_conv(c, "first", p);
    }
    float* s1 = run_stack(c, m.vq_s1, h0, true, r.F.R, r.F.d_valid);
    float* mid = c.ws.get<float>((size_t)G * r.Q.R * C);     // MaxPool1d(stride, ceil_mode=True), vqpe.py:38
    for (int g = 0; g < G; ++g)
        MT2_HIP(launch_pool_max(s1 + (size_t)g * r.F.R * C, C, ip.dev(o_first), ip.dev(o_cnt),
                                mid + (size_t)g * r.Q.R * C, C, C, r.Q.R, c.s));
    float* s2 = run_stack(c, m.vq_s2, mid, false, r.Q.R, r.Q.d_valid);
    float* sum = c.ws.get<float>((size_t)r.Q.R * C);
    MT2_HIP(launch_sum_groups(s2, (long long)r.Q.R * C, G, C, sum, C, C, r.Q.R, c.s));
    r.ze = c.ws.get<float>((size_t)r.Q.R * Dq);
    conv_same(c, sum, C, r.Q.R, m.vq_last, r.ze, Dq, r.Q.d_valid, ACT_NONE, 0.f, ACT_NONE, nullptr, 0, 1, "last");
    // EuclideanCodebook.quantize: distance GEMM + ordered argmax
    float* xe = c.ws.get<float>((size_t)r.Q.R * cfg.vq_bins);
    linear(c, r.ze, Dq, r.Q.R, m.codebook, nullptr, cfg.vq_bins, Dq, xe, cfg.vq_bins);
    form_note_linear(c, "vq", r.Q.R, cfg.vq_bins, Dq);
    r.idx = c.ws.get<int64_t>(r.Q.R);
    MT2_HIP(launch_vq_argmin(r.ze, Dq, Dq, xe, cfg.vq_bins, m.codebook_sq, cfg.vq_bins, r.Q.d_valid, r.idx, r.Q.R,
                             c.s));
    return r;
}

// ---------------------------------------------------------------------------------------------------
// HiFi-GAN V1 generator on mel rows [M0.R, in_dim] -> waveform rows [M0.R * hop] (1 channel, tanh'ed).  The gap between utterances is
// vocoder_gap's (capi.inc): 4 mel rows for the production generator, 8 in reflect mode

static float* hifigan_rows(const Ctx& c, const float* xmel, const RowSet& M0) {
    mt2_model& m = c.m;
    const mt2_config& cfg = m.cfg;
    const float slope = cfg.hg_slope;
    long long R = M0.R;
    int ch = cfg.hg_init_channels;
    // reflect edge mode (speechbrain): the halo rows of every utterance are mirrored into the gap in front of each
    // "same" convolution; `scale` = output rows per mel frame at the current stage
    const bool reflect = cfg.hg_reflect_pad != 0;
    long long scale = 1;
    int min_len = M0.B ? M0.len[0] : 0;
    for (int b = 1; b < M0.B; ++b) min_len = std::min(min_len, M0.len[b]);
    auto halo = [&](const Ctx& cc, float* buf, int width, int G) {
        if (!reflect || G <= 0) return;
        MT2_REQUIRE(2ll * G <= (long long)M0.G * scale, "reflect padding needs a gap of two halos between utterances");
        // torch F.pad(mode="reflect") / speechbrain raise when the padding is not smaller than the input: so do we
        MT2_REQUIRE((long long)min_len * scale > G, "reflect padding must be smaller than the utterance (as F.pad raises): "
                                                    "utterance too short for the vocoder's reflect-padded convolutions");
        MT2_HIP(launch_fill_reflect(buf, width, width, M0.d_start, M0.d_len, M0.B, scale, G, cc.s));
        form_note(cc, "halo", "fill", "width=%d G=%d", width, G);
    };
    // form log (tests): kinds voc-pre, voc-stage<i>, voc-post; the MRF mean is booked on the stage whose resblocks it averages
    char kind[24];
    const FormScope form_scope{m};
    form_kind(c, "voc-pre");
    float* x = c.ws.get<float>((size_t)R * ch);
    if (reflect) {      // conv_pre reads its input in place: mirror the mel rows first (the rows are ours: a packed copy)
        MT2_REQUIRE((cfg.hg_in_dim & 3) == 0, "reflect padding needs a mel width that is a multiple of 4");
        halo(c, const_cast<float*>(xmel), cfg.hg_in_dim, (m.hg_pre.k - 1) / 2);
    }
    conv_same(c, xmel, cfg.hg_in_dim, (int)R, m.hg_pre, x, ch, M0.d_valid);
    form_note(c, "pre", "gemm", "ch=%d R=%lld tile=%s", ch, R, m.opts.last_cfg);
    const int* valid = M0.d_valid;
    const float* const* mrf = nullptr;        // the previous stage's three resblock outputs while their mean has not been formed yet
    float* rb[3] = {nullptr, nullptr, nullptr};
    for (int i = 0; i < cfg.hg_n_up; ++i) {
        const UpW& u = m.hg_up[i];
        const int s = u.stride, co = u.cout, hs = s / 2;
        MT2_REQUIRE(R * s < (1ll << 31), "waveform row count exceeds int32");
        // ConvTranspose1d as two phase GEMMs over the input rows; output [R, s*co] IS [R*s, co] time-major
        float* up = c.ws.get<float>((size_t)R * s * co);
        // ... or, where the input is the MRF mean of the previous stage and has no other consumer, mean -> leaky ReLU -> both phases as
        // ONE launch (up_mrf_route; option up_fuse): the mean never exists in memory.  NotSupported keeps the three launches below
        bool fused = false;
        if (mrf) {
            fused = m.opts.up_fuse && up_mrf(c, mrf, ch, (int)R, u, slope, up, valid);
            if (!fused) {
                x = c.ws.get<float>((size_t)R * ch);
                MT2_HIP(launch_avg3(mrf[0], mrf[1], mrf[2], 1.0f / 3.0f, x, R * ch, c.s));
            }
            form_note(c, "mean", fused ? "in-upsample" : "avg3", "ch=%d R=%lld", ch, R);
            mrf = nullptr;
        }
        snprintf(kind, sizeof kind, "voc-stage%d", i);
        form_kind(c, kind);
        if (fused) form_note(c, "upsample", "fused", "ch=%d R=%lld tile=%s", ch, R, m.opts.last_cfg);
        for (int half = 0; half < 2 && !fused; ++half) {
            GemmP p{};
            p.X = x; p.ldx = ch; p.Rx = (int)R; p.taps = 2; p.shift0 = half == 0 ? -1 : 0; p.Cin = ch;
            p.W = half == 0 ? u.wlo : u.whi; p.bias = u.bias; p.valid = valid;
            p.C = up + (half == 0 ? 0 : hs * co); p.ldc = s * co; p.M = (int)R; p.N = hs * co;
            p.pro_act = ACT_LRELU; p.pro_slope = slope;
            gemm(c, p);
            form_note(c, "upsample", "halves", "half=%d ch=%d R=%lld tile=%s", half, ch, R, m.opts.last_cfg);
        }
        int* v2 = c.ws.get<int>((size_t)R * s);
        MT2_HIP(launch_expand_mask(valid, s, v2, R * s, c.s));
        valid = v2;
        R *= s;
        scale *= s;
        ch = co;
        // multi-receptive-field fusion: mean of the resblocks (ResBlock1: x += conv2(lrelu(conv1(lrelu(x)))) x3)
        // The three resblocks of a stage only share their input: each runs on its own stream (the caller's + two
        // side streams), so that one chain's launch tails (868 tiles on 256 CUs at stage 1) are filled by the others.
        const size_t per = (size_t)R * ch;
        MT2_REQUIRE(cfg.hg_n_res == 3, "HiFi-GAN V1 uses three resblocks per stage");
        const int nside = m.opts.voc_streams > 1 ? 2 : 0;
        ensure_aux(m, nside);
        form_note(c, "streams", nside ? "3" : "1", "ch=%d R=%lld", ch, R);
        for (int j = 0; j < 3; ++j)      // zero padding IS the gap: no convolution of the stage may reach across it into a neighbour
            for (int n = 0; n < 3 && !reflect; ++n)
                MT2_REQUIRE((long long)(m.hg_res[i * 3 + j].k - 1) / 2 * m.hg_res[i * 3 + j].dil[n] <= (long long)M0.G * scale || M0.B < 2,
                            "the gap between utterances is narrower than a resblock convolution's halo");
        if (reflect) {     // the three chains share `up`: one halo wide enough for the widest first convolution, before the fork
            int g0 = 0;
            for (int j = 0; j < 3; ++j) g0 = std::max(g0, (m.hg_res[i * 3 + j].k - 1) / 2 * m.hg_res[i * 3 + j].dil[0]);
            halo(c, up, ch, g0);
        }
        if (nside) {
            MT2_HIP(hipEventRecord(m.ev_fork, c.s));
            m.aux_forked = true;
            for (int j = 0; j < nside; ++j) MT2_HIP(hipStreamWaitEvent(m.aux_streams[j], m.ev_fork, 0));
        }
        for (int j = 0; j < 3; ++j) {
            const ResW& r = m.hg_res[i * 3 + j];
            const Ctx cj{m, (nside && j > 0) ? m.aux_streams[j - 1] : c.s, c.ws};
            float* t1 = c.ws.get<float>(per);
            float* ha = c.ws.get<float>(per);
            float* hb = c.ws.get<float>(per);
            rb[j] = c.ws.get<float>(per);
            const float* h = up;
            for (int n = 0; n < 3; ++n) {
                float* out = n == 2 ? rb[j] : (n == 0 ? ha : hb);
                // x + conv2(lrelu(conv1(lrelu(x)))): the inner leaky ReLU has ONE consumer, so it is applied once in
                // conv1's epilogue instead of on every operand fragment of conv2 (same values, no VALU in that loop)
                if (n > 0) halo(cj, const_cast<float*>(h), ch, (r.k - 1) / 2 * r.dil[n]);
                // ... and both convolutions as ONE launch where conv_pair_route takes the pair (option pair_fuse): t1 never leaves
                // the workgroup's LDS.  Bit-identical; NotSupported keeps the two launches below
                if (m.opts.pair_fuse && conv_pair(cj, h, ch, (int)R, r.c1[n], r.c2[n], r.dil[n], slope, reflect, out, valid)) {
                    form_note(cj, "pair", "fused", "j=%d n=%d ch=%d k=%d dil=%d R=%lld tile=%s", j, n, ch, r.k, r.dil[n], R, m.opts.last_cfg);
                    h = out;
                    continue;
                }
                conv_same(cj, h, ch, (int)R, r.c1[n], t1, ch, valid, ACT_LRELU, slope, ACT_LRELU, nullptr, 0, r.dil[n]);
                const char* tile1 = m.opts.last_cfg;
                halo(cj, t1, ch, (r.k - 1) / 2);
                conv_same(cj, t1, ch, (int)R, r.c2[n], out, ch, valid, ACT_NONE, slope, ACT_NONE, h, ch, 1);
                form_note(cj, "pair", "two", "j=%d n=%d ch=%d k=%d dil=%d R=%lld tile=%s tile2=%s", j, n, ch, r.k, r.dil[n], R, tile1,
                          m.opts.last_cfg);
                h = out;
            }
        }
        for (int j = 0; j < nside; ++j) {
            MT2_HIP(hipEventRecord(m.ev_join[j], m.aux_streams[j]));
            MT2_HIP(hipStreamWaitEvent(c.s, m.ev_join[j], 0));
        }
        if (!reflect && i + 1 == cfg.hg_n_up && m.hg_post.cout == 1 && (ch & 3) == 0 && ch <= 128 && m.hg_post.k <= 15) {
            // last stage: the mean goes straight into the output layer (one pass over the three resblock outputs)
            // F.leaky_relu default slope 0.01, conv_post k7, tanh
            float* wav = c.ws.get<float>((size_t)R);
            const hipError_t e = launch_conv_post(rb[0], rb[1], rb[2], 1.0f / 3.0f, R, ch, m.hg_post.k, m.hg_post.w,
                                                  m.hg_post.b, 0.01f, valid, wav, c.s);
            if (e == hipSuccess) {
                form_note(c, "mean", "in-post", "ch=%d R=%lld", ch, R);
                form_kind(c, "voc-post");
                form_note(c, "post", "fused", "ch=%d k=%d R=%lld tile=conv_post", ch, m.hg_post.k, R);
                return wav;
            }
            if (e != hipErrorNotSupported) MT2_HIP(e);      // not supported (LDS): the two-launch form below
        }
        if (i + 1 < cfg.hg_n_up) {     // the next stage's upsampler is the mean's only consumer: it may form it itself
            mrf = rb;
            continue;
        }
        x = c.ws.get<float>(per);
        MT2_HIP(launch_avg3(rb[0], rb[1], rb[2], 1.0f / 3.0f, x, (long long)per, c.s));
        form_note(c, "mean", "avg3", "ch=%d R=%lld", ch, R);
    }
    form_kind(c, "voc-post");
    float* wav = c.ws.get<float>((size_t)R);
    halo(c, x, ch, (m.hg_post.k - 1) / 2);
    conv_same(c, x, ch, (int)R, m.hg_post, wav, 1, valid, ACT_LRELU, 0.01f, ACT_TANH);
    form_note(c, "post", "gemm", "ch=%d k=%d R=%lld tile=%s", ch, m.hg_post.k, R, m.opts.last_cfg);
    return wav;
}

// ---------------------------------------------------------------------------------------------------
// mel front-end: extract_mel_spec (modules/tokenizer.py:107-125).  Restates torchaudio's Spectrogram +
// MelScale (neither is in the reference tree; parity unpinned): periodic Hann window,
// center=True with reflect padding, one-sided magnitude (power 1), slaney mel scale and slaney area norm,
// log(clamp(., clip)).  Constants are built once per audio configuration in double precision.

static double hz_to_mel_slaney(double f) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return f >= min_log_hz ? min_log_mel + std::log(f / min_log_hz) / logstep : f / f_sp;
}
static double mel_to_hz_slaney(double mel) {
    const double f_sp = 200.0 / 3.0, min_log_hz = 1000.0, min_log_mel = min_log_hz / f_sp, logstep = std::log(6.4) / 27.0;
    return mel >= min_log_mel ? min_log_hz * std::exp(logstep * (mel - min_log_mel)) : f_sp * mel;
}
// the analysis window in double: periodic Hann of win_length, centred in n_fft (torch.stft centres a short window inside n_fft)
static std::vector<double> frontend_window(const mt2_audio_config& ac) {
    const double PI = 3.14159265358979323846;
    std::vector<double> win(ac.n_fft, 0.0);
    const int left = (ac.n_fft - ac.win_length) / 2;
    for (int k = 0; k < ac.win_length; ++k) win[left + k] = 0.5 - 0.5 * std::cos(2.0 * PI * k / ac.win_length);
    return win;
}
// torchaudio.functional.melscale_fbanks(n_freqs=F, f_min, f_max, n_mels, sample_rate, "slaney", "slaney"), rounded to f32: [n_mels, Fp]
static std::vector<float> frontend_filterbank(const mt2_audio_config& ac, int F, int Fp) {
    std::vector<float> fb((size_t)ac.n_mels * Fp, 0.0f);
    const double m_min = hz_to_mel_slaney(ac.f_min), m_max = hz_to_mel_slaney(ac.f_max);
    std::vector<double> fpts(ac.n_mels + 2);
    for (int i = 0; i < ac.n_mels + 2; ++i) fpts[i] = mel_to_hz_slaney(m_min + (m_max - m_min) * i / (ac.n_mels + 1));
    for (int j = 0; j < ac.n_mels; ++j) {
        const double enorm = 2.0 / (fpts[j + 2] - fpts[j]);
        for (int f = 0; f < F; ++f) {
            const double freq = (double)(ac.sample_rate / 2) * f / (F - 1);
            const double down = (freq - fpts[j]) / (fpts[j + 1] - fpts[j]);
            const double up = (fpts[j + 2] - freq) / (fpts[j + 2] - fpts[j + 1]);
            fb[(size_t)j * Fp + f] = (float)(std::max(0.0, std::min(down, up)) * enorm);
        }
    }
    return fb;
}
static void frontend_check(const mt2_audio_config& ac) {
    MT2_REQUIRE(ac.n_fft >= 8 && ac.hop_length >= 4 && ac.hop_length % 4 == 0 && ac.n_fft % ac.hop_length == 0,
                "n_fft must be a multiple of hop_length, hop_length a multiple of 4");
    MT2_REQUIRE(ac.win_length >= 1 && ac.win_length <= ac.n_fft && ac.n_mels >= 1 && ac.n_mels % 4 == 0,
                "win_length <= n_fft, n_mels a multiple of 4");
    MT2_REQUIRE(ac.f_max > ac.f_min && ac.sample_rate > 0 && ac.clip > 0.0f, "bad audio configuration");
}
static float* frontend_upload(mt2_model& m, const std::vector<float>& v) {
    float* d = nullptr;
    MT2_HIP(hipMalloc(reinterpret_cast<void**>(&d), v.size() * sizeof(float)));
    MT2_HIP(hipMemcpy(d, v.data(), v.size() * sizeof(float), hipMemcpyHostToDevice));
    m.dev_allocs.push_back(d);
    return d;
}
// The geometry of every spectral call, from its audio configuration: taps hop-sized blocks to a frame, pad reflected samples on either
// side, F one-sided bins; a magnitude row has Fp floats and a spectrum row (re | im | zero pad) lds
struct SpecGeom {
    int N, hop, taps, pad, F, Fp, lds;
    explicit SpecGeom(const mt2_audio_config& ac)
        : N(ac.n_fft), hop(ac.hop_length), taps(hop > 0 ? N / hop : 0), pad(N / 2), F(N / 2 + 1), Fp((F + 3) & ~3), lds((2 * F + 3) & ~3) {}
};
static void frontend_prepare(mt2_model& m, const mt2_audio_config& ac) {
    if (m.fe_basis && std::memcmp(&m.fe_cfg, &ac, sizeof(ac)) == 0) return;
    frontend_check(ac);
    const SpecGeom g(ac);
    const int N = g.N, F = g.F, Fp = g.Fp;
    const double PI = 3.14159265358979323846;
    const std::vector<double> win = frontend_window(ac);
    std::vector<float> basis((size_t)2 * F * N);
    for (int f = 0; f < F; ++f)
        for (int k = 0; k < N; ++k) {
            const double ang = 2.0 * PI * (double)(((long long)f * k) % N) / N;
            basis[(size_t)f * N + k] = (float)(win[k] * std::cos(ang));
            basis[(size_t)(F + f) * N + k] = (float)(-win[k] * std::sin(ang));
        }
    m.fe_basis = frontend_upload(m, basis);
    m.fe_fb = frontend_upload(m, frontend_filterbank(ac, F, Fp));
    m.fe_nfreq = F; m.fe_nfreq_pad = Fp;
    m.fe_cfg = ac;
    m.gl_ibasis = m.gl_w2 = m.gl_P = nullptr;      // the Griffin-Lim constants follow the configuration: rebuilt on their next use
}

// The packed rows of a ragged batch in front of the STFT convolution and behind the inverse one: utterance b owns T_b - 1 + taps hop-sized
// blocks of its reflect-padded signal and the T_b frame rows row0[b] .. ; frame t reads blocks t .. t + taps - 1.  Every call adds the
// lists it needs to its own plan
struct FrameRows {
    std::vector<int> blk_b, blk_t, rowbase, map, row0;      // map[r] = b * T_max + t
    int Rb = 0, Fr = 0;
};
// the bound every row list of a batch stays under, refused before the lists are built
static void check_row_count(const SpecGeom& g, const int* T, int B) {
    long long rows = 0;
    for (int b = 0; b < B; ++b) rows += T[b] + g.taps;
    MT2_REQUIRE(rows * (g.N + 4) <= INT_MAX, "batch too large for 32-bit row indices");
}
static FrameRows frame_rows(const SpecGeom& g, const int* T, int B, int T_max) {
    check_row_count(g, T, B);
    FrameRows r;
    r.row0.resize(B);
    for (int b = 0; b < B; ++b) { r.row0[b] = r.Fr; r.Fr += T[b]; r.Rb += T[b] - 1 + g.taps; }
    r.blk_b.resize(r.Rb); r.blk_t.resize(r.Rb); r.rowbase.resize(r.Fr); r.map.resize(r.Fr);
    for (int b = 0, blk = 0, row = 0; b < B; ++b) {
        const int blk0 = blk;
        for (int t = 0; t < T[b] - 1 + g.taps; ++t, ++blk) { r.blk_b[blk] = b; r.blk_t[blk] = t; }
        for (int t = 0; t < T[b]; ++t, ++row) { r.rowbase[row] = blk0 + t; r.map[row] = b * T_max + t; }
    }
    return r;
}
// the frame counts of a batch of waveforms in front of the STFT: T_b = 1 + L_b / hop
static std::vector<int> stft_frames(const SpecGeom& g, const int* lens, int L_max, int B, int T_max) {
    std::vector<int> T(B);
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(lens[b] > g.pad && lens[b] <= L_max, "waveform shorter than n_fft/2 + 1 samples (reflect padding) or > L_max");
        T[b] = 1 + lens[b] / g.hop;
        MT2_REQUIRE(T[b] <= T_max, "T_max smaller than 1 + L / hop_length");
    }
    return T;
}
// STFT = Conv1d over hop-sized blocks against the windowed DFT basis: spec[m] = [re(0..F-1) | im(0..F-1)] of frame m, row pitch 2F
// rounded up to 4
static void stft_gemm(const Ctx& c, const SpecGeom& g, const float* xp, int Rb, const int* rowbase, float* spec, int Fr) {
    GemmP p{};
    p.X = xp; p.ldx = g.hop; p.Rx = Rb; p.rowbase = rowbase; p.taps = g.taps; p.Cin = g.hop;
    p.W = c.m.fe_basis; p.C = spec; p.ldc = g.lds; p.M = Fr; p.N = 2 * g.F;
    gemm(c, p);
}
// the front half of the mel front-end: reflect padding into blocks, then one STFT convolution over the batch -> the packed spec [Fr, lds]
// and, on the device, the place b * T_max + t of each of its rows
struct StftOut { const float* spec; const int* map; int Fr; };
static StftOut stft_run(const Ctx& c, const mt2_audio_config& ac, const float* wav, const int* lens, int L_max, int B, int T_max) {
    frontend_prepare(c.m, ac);
    const SpecGeom g(ac);
    const std::vector<int> T = stft_frames(g, lens, L_max, B, T_max);
    const FrameRows r = frame_rows(g, T.data(), B, T_max);
    IntPlan ip;
    const int o_b = ip.add(r.blk_b), o_t = ip.add(r.blk_t), o_len = ip.add(lens, B), o_base = ip.add(r.rowbase), o_map = ip.add(r.map);
    ip.upload(c.ws, c.m.pinned(), c.s);
    float* xp = c.ws.get<float>((size_t)r.Rb * g.hop);
    MT2_HIP(launch_reflect_pad_blocks(wav, L_max, ip.dev(o_b), ip.dev(o_t), ip.dev(o_len), g.hop, g.pad, xp, r.Rb, c.s));
    float* spec = c.ws.get<float>((size_t)r.Fr * g.lds);
    stft_gemm(c, g, xp, r.Rb, ip.dev(o_base), spec, r.Fr);
    return {spec, ip.dev(o_map), r.Fr};
}

static void mel_spectrogram_run(const Ctx& c, const mt2_audio_config& ac, const float* wav, const int* lens, int L_max,
                                int B, float* mel, int T_max) {
    mt2_model& m = c.m;
    const StftOut s = stft_run(c, ac, wav, lens, L_max, B, T_max);
    const SpecGeom g(ac);
    const int Fr = s.Fr;
    float* mag = c.ws.get<float>((size_t)Fr * g.Fp);
    MT2_HIP(launch_magnitude(s.spec, g.lds, g.F, mag, g.Fp, Fr, c.s));
    float* mrows = c.ws.get<float>((size_t)Fr * ac.n_mels);
    {   // MelScale + dynamic range compression
        GemmP p{};
        p.X = mag; p.ldx = g.Fp; p.Rx = Fr; p.Cin = g.Fp; p.W = m.fe_fb; p.C = mrows; p.ldc = ac.n_mels; p.M = Fr;
        p.N = ac.n_mels; p.epi_act = ACT_LOGCLAMP; p.pro_slope = ac.clip;
        gemm(c, p);
    }
    MT2_HIP(hipMemsetAsync(mel, 0, sizeof(float) * (size_t)B * T_max * ac.n_mels, c.s));
    MT2_HIP(launch_unpack_rows(mrows, ac.n_mels, ac.n_mels, T_max, 0, s.map, mel, Fr, c.s));
}

// spec f32 [B, T_max, lds] (re | im | zero pad; zeros in frames at or beyond T_b) = the STFT the mel front-end takes its magnitude of
static void stft_only_run(const Ctx& c, const mt2_audio_config& ac, const float* wav, const int* lens, int L_max, int B, float* spec_out,
                          int T_max) {
    MT2_REQUIRE(wav != nullptr && lens != nullptr && spec_out != nullptr, "bad buffers");
    const StftOut s = stft_run(c, ac, wav, lens, L_max, B, T_max);
    const int lds = SpecGeom(ac).lds;
    MT2_HIP(hipMemsetAsync(spec_out, 0, sizeof(float) * (size_t)B * T_max * lds, c.s));
    MT2_HIP(launch_unpack_rows(s.spec, lds, lds, T_max, 0, s.map, spec_out, s.Fr, c.s));
}

// ---------------------------------------------------------------------------------------------------
// What every ragged-batch audio call decides on the host, stated once.
// The ragged-length contract: lens[b] in [1, cap], refused with `msg` (the call's own wording); -> max_b lens[b]
static int check_lens(const int* lens, int B, int cap, const char* msg) {
    int mx = 0;
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(lens[b] >= 1 && lens[b] <= cap, msg);
        mx = std::max(mx, lens[b]);
    }
    return mx;
}
// a caller's buffer; a NULL one (an optional output that was not asked for) overlaps nothing
struct Span { const void* p; size_t n; };
static bool spans_overlap(const Span& a, const Span& b) {
    const uintptr_t a0 = (uintptr_t)a.p, b0 = (uintptr_t)b.p;
    return a.p != nullptr && b.p != nullptr && a0 < b0 + b.n && b0 < a0 + a.n;
}
// does an output overlap an input or another output?
static bool outputs_overlap(std::initializer_list<Span> outs, std::initializer_list<Span> ins) {
    for (const Span* o = outs.begin(); o != outs.end(); ++o) {
        for (const Span& i : ins)
            if (spans_overlap(*o, i)) return true;
        for (const Span* q = o + 1; q != outs.end(); ++q)
            if (spans_overlap(*o, *q)) return true;
    }
    return false;
}

// what a call's layout function (its plan and its carve, a template over the arena) takes from an arena: the byte query of that call
template <class Layout> static long long arena_bytes(Layout layout) {
    ArenaCount count;
    IntPlan ip;
    layout(count, ip);
    return (long long)count.bytes;
}

// ---------------------------------------------------------------------------------------------------
// Griffin-Lim vocoder (griffinlim.hip holds the rule): mel -> linear magnitude by the filterbank's pseudo-inverse, random phase, then
// n_iter rounds of inverse STFT -> forward STFT -> phase update.  Four launches a round: the inverse-DFT GEMM, the overlap-add (which
// writes the STFT's reflect-padded block buffer itself), the STFT GEMM of the front-end and the phase update.
//
// Route of the two large GEMMs: fe_basis and the inverse basis are uploaded here, outside the weight store, so they have neither bf16
// nor fp16 planes - both launches run on the f32 MFMA tiles, never on the fp16 pipe, and the range guard (mt2_x3h_guard) has nothing to
// watch: exp of an untrained model's log-mel beyond 65504 stays an ordinary f32 number.  The tile itself is FIXED (64x64, three-stage
// ring, no K split) instead of chosen from the row count: the K-split tiles sum in another order, and a ragged batch must be
// bit-identical to its utterances alone.
struct FixedTile {
    EngineOpts& o;
    int old;
    explicit FixedTile(EngineOpts& oo) : o(oo), old(oo.force_cfg) { if (old < 0) o.force_cfg = CFG_DMA64x64_S3; }
    ~FixedTile() { o.force_cfg = old; }
};

// the geometry every Griffin-Lim entry point checks before anything else (host only)
static void gl_check_config(const mt2_audio_config& ac) {
    frontend_check(ac);
    MT2_REQUIRE(ac.n_fft / ac.hop_length >= 2, "n_fft / hop_length < 2: the overlap-added squared window has zeros");
}
static int gl_min_frames(const mt2_audio_config& ac) { return ac.n_fft / (2 * ac.hop_length) + 2; }
static void gl_check_lens(const mt2_audio_config& ac, const int* T, int T_max, int B, long long L_max) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(T != nullptr && T_max >= 1, "mel_lens is NULL or T_max < 1");
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(T[b] >= gl_min_frames(ac) && T[b] <= T_max, "a frame count outside [n_fft / (2 hop) + 2, T_max]");
        MT2_REQUIRE(L_max >= (long long)(T[b] - 1) * ac.hop_length, "L_max smaller than (max T - 1) * hop_length");
    }
    check_row_count(SpecGeom(ac), T, B);
}
// the arena of one griffin_lim_run, in carve order (the closed form is in megatts2_hip.h): the plan, exp(M), A, S / R / Rprev, the
// frames, the block buffer.  Fr frame rows and Rb hop blocks in the batch
// The plan is built here too, so that mt2_griffin_lim_query (over an ArenaCount, seeds NULL: zeros) and griffin_lim_run (over the arena)
// cannot disagree.  rstride = (n_iter + 1) T_max when the residuals are asked for, else 0: no rmap
struct GlWs {
    FrameRows r;
    int o_b, o_t, o_base, o_map, o_rb, o_rt, o_row0, o_T, o_seed, o_rmap;
    float *E, *A, *S, *R, *Rprev, *frames, *xp;
};
template <class Ws> static GlWs gl_layout(Ws& ws, IntPlan& ip, const mt2_audio_config& ac, const int* T, int T_max, int B,
                                          const uint64_t* seeds, long long rstride) {
    const SpecGeom g(ac);
    GlWs w{};
    w.r = frame_rows(g, T, B, T_max);
    const size_t Fr = w.r.Fr;
    std::vector<int> row_b(Fr), row_t(Fr), sd(2 * (size_t)B, 0);
    for (int b = 0, r = 0; b < B; ++b)
        for (int t = 0; t < T[b]; ++t, ++r) { row_b[r] = b; row_t[r] = t; }
    for (int b = 0; seeds && b < B; ++b) { sd[2 * b] = (int)(uint32_t)(seeds[b] & 0xFFFFFFFFu); sd[2 * b + 1] = (int)(uint32_t)(seeds[b] >> 32); }
    w.o_b = ip.add(w.r.blk_b); w.o_t = ip.add(w.r.blk_t); w.o_base = ip.add(w.r.rowbase); w.o_map = ip.add(w.r.map);
    w.o_rb = ip.add(row_b); w.o_rt = ip.add(row_t); w.o_row0 = ip.add(w.r.row0); w.o_T = ip.add(T, B); w.o_seed = ip.add(sd);
    w.o_rmap = -1;
    if (rstride) {
        std::vector<int> rmap(Fr);
        for (size_t r = 0; r < Fr; ++r) rmap[r] = (int)(row_b[r] * rstride + row_t[r]);
        w.o_rmap = ip.add(rmap);
    }
    ip.carve(ws);
    w.E = ws.template get<float>(Fr * ac.n_mels);
    w.A = ws.template get<float>(Fr * g.Fp);
    w.S = ws.template get<float>(Fr * g.lds);
    w.R = ws.template get<float>(Fr * g.lds);
    w.Rprev = ws.template get<float>(Fr * g.lds);
    w.frames = ws.template get<float>(Fr * g.N);
    w.xp = ws.template get<float>((size_t)w.r.Rb * g.hop);
    return w;
}

// the inverse basis [N, lds] (window and the 1/N, 2/N Hermitian weights folded in, zero columns for the imaginary parts of bins 0 and
// N/2 and for the pad) and the squared window: built in double on the first call that inverts an STFT, rounded once
static void gl_prepare_istft(mt2_model& m, const mt2_audio_config& ac) {
    gl_check_config(ac);
    const SpecGeom g(ac);
    const int N = g.N, F = g.F, lds = g.lds, hop = g.hop, pad = g.pad;
    const bool same = m.fe_basis && std::memcmp(&m.fe_cfg, &ac, sizeof(ac)) == 0;
    if (same && m.gl_ibasis) return;
    const double PI = 3.14159265358979323846;
    const std::vector<double> win = frontend_window(ac);
    std::vector<float> w2(N), ib((size_t)N * lds, 0.0f);
    for (int k = 0; k < N; ++k) w2[k] = (float)(win[k] * win[k]);
    for (int p = pad; p < pad + N; ++p) {      // the envelope at the left edge and in the interior (the right edge mirrors the left)
        float e = 0.0f;
        for (int t = p >= N ? (p - N) / hop + 1 : 0; t <= p / hop; ++t) e += w2[p - t * hop];
        MT2_REQUIRE(e > 1e-11f, "the overlap-added squared window has zeros (win_length too short for this hop)");
    }
    for (int k = 0; k < N; ++k)
        for (int f = 0; f < F; ++f) {
            const bool edge = f == 0 || 2 * f == N;
            const double ang = 2.0 * PI * (double)(((long long)f * k) % N) / N, wt = win[k] * (edge ? 1.0 : 2.0) / N;
            ib[(size_t)k * lds + f] = (float)(wt * std::cos(ang));
            ib[(size_t)k * lds + F + f] = edge ? 0.0f : (float)(-wt * std::sin(ang));
        }
    frontend_prepare(m, ac);
    m.gl_ibasis = frontend_upload(m, ib);
    m.gl_w2 = frontend_upload(m, w2);
}
// P = fb^T (fb fb^T)^-1 [Fp, n_mels] (rows F .. Fp-1 zero) by Cholesky in double from the f32 filterbank; refused when the Gram matrix
// is not positive definite (filters without a bin: n_fft too small for n_mels)
static std::vector<float> gl_pinv(const mt2_audio_config& ac) {
    const int F = SpecGeom(ac).F, Fp = SpecGeom(ac).Fp, J = ac.n_mels;
    const std::vector<float> fb = frontend_filterbank(ac, F, Fp);
    std::vector<double> G((size_t)J * J, 0.0);
    double dmax = 0.0;
    for (int i = 0; i < J; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = 0.0;
            for (int f = 0; f < F; ++f) s += (double)fb[(size_t)i * Fp + f] * (double)fb[(size_t)j * Fp + f];
            G[(size_t)i * J + j] = G[(size_t)j * J + i] = s;
            if (i == j) dmax = std::max(dmax, s);
        }
    std::vector<double> Lc((size_t)J * J, 0.0);
    for (int i = 0; i < J; ++i)
        for (int j = 0; j <= i; ++j) {
            double s = G[(size_t)i * J + j];
            for (int k = 0; k < j; ++k) s -= Lc[(size_t)i * J + k] * Lc[(size_t)j * J + k];
            if (i == j) {
                if (!(s > 1e-12 * dmax))
                    throw Error("griffin_lim: the mel filterbank is rank deficient (fb fb^T is not positive definite: a filter covers no bin)");
                Lc[(size_t)i * J + i] = std::sqrt(s);
            } else {
                Lc[(size_t)i * J + j] = s / Lc[(size_t)j * J + j];
            }
        }
    std::vector<float> P((size_t)Fp * J, 0.0f);
    std::vector<double> y(J);
    for (int f = 0; f < F; ++f) {      // G x = fb[:, f]:  P[f, :] = x
        for (int i = 0; i < J; ++i) {
            double s = fb[(size_t)i * Fp + f];
            for (int k = 0; k < i; ++k) s -= Lc[(size_t)i * J + k] * y[k];
            y[i] = s / Lc[(size_t)i * J + i];
        }
        for (int i = J - 1; i >= 0; --i) {
            double s = y[i];
            for (int k = i + 1; k < J; ++k) s -= Lc[(size_t)k * J + i] * y[k];
            y[i] = s / Lc[(size_t)i * J + i];
        }
        for (int i = 0; i < J; ++i) P[(size_t)f * J + i] = (float)y[i];
    }
    return P;
}
static void gl_prepare_pinv(mt2_model& m, const mt2_audio_config& ac) {
    gl_check_config(ac);
    if (m.fe_basis && std::memcmp(&m.fe_cfg, &ac, sizeof(ac)) == 0 && m.gl_P) return;
    const std::vector<float> P = gl_pinv(ac);      // may refuse: before anything is uploaded
    frontend_prepare(m, ac);
    m.gl_P = frontend_upload(m, P);
}

// frames[Fr, N] = S[Fr, lds] x inverse basis
static void istft_gemm(const Ctx& c, const SpecGeom& g, const float* S, float* frames, int Fr) {
    GemmP p{};
    p.X = S; p.ldx = g.lds; p.Rx = Fr; p.Cin = g.lds; p.W = c.m.gl_ibasis; p.C = frames; p.ldc = g.N; p.M = Fr; p.N = g.N;
    gemm(c, p);
}
// the back half of every inverse STFT: packed rows S [Fr, lds] -> frames on the fixed tile, overlap-added into wav [B, L_max]
static void istft_rows_to_wav(const Ctx& c, const SpecGeom& g, const float* S, float* frames, int Fr, const int* row0, const int* T,
                              float* wav, int L_max, int B) {
    {
        FixedTile ft(c.m.opts);
        istft_gemm(c, g, S, frames, Fr);
    }
    MT2_HIP(launch_istft_ola_wav(frames, g.N, g.hop, c.m.gl_w2, row0, T, wav, L_max, B, c.s));
}

// torch.istft(center=True, length = (T - 1) hop) of spec f32 [B, T_max, lds] (re | im | pad, as stft_only_run leaves it) -> wav [B, L_max]
static void istft_run(const Ctx& c, const mt2_audio_config& ac, const float* spec, const int* T, int T_max, int B, float* wav, int L_max) {
    gl_check_config(ac);
    gl_check_lens(ac, T, T_max, B, L_max);
    MT2_REQUIRE(spec != nullptr && wav != nullptr, "bad buffers");
    gl_prepare_istft(c.m, ac);
    const SpecGeom g(ac);
    const FrameRows r = frame_rows(g, T, B, T_max);
    IntPlan ip;
    const int o_map = ip.add(r.map), o_row0 = ip.add(r.row0), o_T = ip.add(T, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    float* S = c.ws.get<float>((size_t)r.Fr * g.lds);
    MT2_HIP(hipMemsetAsync(S, 0, sizeof(float) * (size_t)r.Fr * g.lds, c.s));      // the pad columns meet zero basis columns: 0 x garbage must not be NaN
    MT2_HIP(launch_pack_rows(spec, g.lds, T_max, 0, ip.dev(o_map), S, g.lds, r.Fr, c.s));
    float* frames = c.ws.get<float>((size_t)r.Fr * g.N);
    istft_rows_to_wav(c, g, S, frames, r.Fr, ip.dev(o_row0), ip.dev(o_T), wav, L_max, B);
}

// A f32 [B, T_max, Fp] = max(0, exp(mel) P^T), zeros in frames at or beyond T_b and in columns F .. Fp-1
static void mel_to_linear_rows(const Ctx& c, const mt2_audio_config& ac, const float* mel, const int* melmap, float* E, float* A, int Fr) {
    const int Fp = c.m.fe_nfreq_pad;
    MT2_HIP(launch_gl_exp_rows(mel, ac.n_mels, melmap, E, Fr, c.s));
    GemmP p{};
    p.X = E; p.ldx = ac.n_mels; p.Rx = Fr; p.Cin = ac.n_mels; p.W = c.m.gl_P; p.C = A; p.ldc = Fp; p.M = Fr; p.N = Fp; p.epi_act = ACT_RELU;
    FixedTile ft(c.m.opts);
    gemm(c, p);
}
static void mel_to_linear_run(const Ctx& c, const mt2_audio_config& ac, const float* mel, const int* T, int T_max, int B, float* out) {
    gl_check_config(ac);
    MT2_REQUIRE(B >= 1 && B <= 65535 && T != nullptr && T_max >= 1 && mel != nullptr && out != nullptr, "bad arguments");
    check_lens(T, B, T_max, "a frame count outside [1, T_max]");
    gl_prepare_pinv(c.m, ac);
    const int Fp = c.m.fe_nfreq_pad;
    std::vector<int> map;
    for (int b = 0; b < B; ++b)
        for (int t = 0; t < T[b]; ++t) map.push_back(b * T_max + t);
    const int Fr = (int)map.size();
    IntPlan ip;
    const int o_map = ip.add(map);
    ip.upload(c.ws, c.m.pinned(), c.s);
    float* E = c.ws.get<float>((size_t)Fr * ac.n_mels);
    float* A = c.ws.get<float>((size_t)Fr * Fp);
    mel_to_linear_rows(c, ac, mel, ip.dev(o_map), E, A, Fr);
    MT2_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * T_max * Fp, c.s));
    MT2_HIP(launch_unpack_rows(A, Fp, Fp, T_max, 0, ip.dev(o_map), out, Fr, c.s));
}

// every refusal of mt2_griffin_lim that needs no device (shared with mt2_griffin_lim_query)
static void gl_check_call(const mt2_audio_config& ac, const int* T, int T_max, int B, int n_iter, double momentum, long long L_max) {
    gl_check_config(ac);
    MT2_REQUIRE(n_iter >= 0 && n_iter <= 100000, "n_iter outside [0, 100000]");
    MT2_REQUIRE(momentum >= 0.0 && momentum < 1.0, "momentum outside [0, 1)");
    gl_check_lens(ac, T, T_max, B, L_max);
}

static void griffin_lim_run(const Ctx& c, const mt2_audio_config& ac, const float* mel, const int* T, int T_max, int B, int n_iter,
                            double momentum, const uint64_t* seeds, float* wav, int L_max, float* resid) {
    // everything is checked before the first launch: a refused call leaves `wav` and `resid` as they were
    gl_check_call(ac, T, T_max, B, n_iter, momentum, L_max);
    MT2_REQUIRE(mel != nullptr && seeds != nullptr && wav != nullptr, "bad buffers");
    gl_prepare_pinv(c.m, ac);
    gl_prepare_istft(c.m, ac);
    mt2_model& m = c.m;
    const SpecGeom g(ac);
    const int N = g.N, hop = g.hop, F = g.F, Fp = g.Fp, lds = g.lds;
    const float cm = (float)(momentum / (1.0 + momentum));
    if (resid) MT2_REQUIRE((long long)B * (n_iter + 1) * T_max <= INT_MAX, "resid too large for 32-bit indices");
    IntPlan ip;
    const GlWs w = gl_layout(c.ws, ip, ac, T, T_max, B, seeds, resid ? (long long)(n_iter + 1) * T_max : 0);
    const int Fr = w.r.Fr, Rb = w.r.Rb;
    ip.send(m.pinned(), c.s);
    const int *blk_b = ip.dev(w.o_b), *blk_t = ip.dev(w.o_t), *base = ip.dev(w.o_base), *row0 = ip.dev(w.o_row0), *dT = ip.dev(w.o_T);
    const int* rmap = resid ? ip.dev(w.o_rmap) : nullptr;
    Stages st(m, c.s);
    st.mark("start");
    if (resid) MT2_HIP(hipMemsetAsync(resid, 0, sizeof(float) * (size_t)B * (n_iter + 1) * T_max, c.s));
    mel_to_linear_rows(c, ac, mel, ip.dev(w.o_map), w.E, w.A, Fr);
    MT2_HIP(launch_gl_phase_init(w.A, Fp, ip.dev(w.o_rb), ip.dev(w.o_rt), reinterpret_cast<const uint32_t*>(ip.dev(w.o_seed)), w.S, lds, F, Fr, c.s));
    if (n_iter > 0) MT2_HIP(hipMemsetAsync(w.Rprev, 0, sizeof(float) * (size_t)Fr * lds, c.s));
    st.mark("gl_setup");
    FixedTile ft(m.opts);
    for (int k = 0; k < n_iter; ++k) {
        istft_gemm(c, g, w.S, w.frames, Fr);
        MT2_HIP(launch_istft_ola_blocks(w.frames, N, hop, m.gl_w2, blk_b, blk_t, row0, dT, w.xp, Rb, c.s));
        stft_gemm(c, g, w.xp, Rb, base, w.R, Fr);
        MT2_HIP(launch_gl_phase_update(w.R, w.Rprev, w.A, Fp, w.S, lds, F, cm, resid ? resid + (size_t)k * T_max : nullptr, rmap, Fr, 1, c.s));
    }
    st.mark("gl_iterations");
    istft_rows_to_wav(c, g, w.S, w.frames, Fr, row0, dT, wav, L_max, B);
    if (resid) {      // entry n_iter: one extra STFT of the output, paid only on request
        MT2_HIP(launch_istft_ola_blocks(w.frames, N, hop, m.gl_w2, blk_b, blk_t, row0, dT, w.xp, Rb, c.s));
        stft_gemm(c, g, w.xp, Rb, base, w.R, Fr);
        MT2_HIP(launch_gl_phase_update(w.R, nullptr, w.A, Fp, nullptr, lds, F, cm, resid + (size_t)n_iter * T_max, rmap, Fr, 0, c.s));
    }
    st.mark("gl_final");
    st.finish();
}

// ---------------------------------------------------------------------------------------------------
// prompt audio at any sample rate (models/megatts2.py:335-336: librosa.load(wav, sr=16000), librosa.util.normalize):
// the polyphase resampler of resample.hip and the per-utterance peak normalisation, in front of the mel front-end.

static const float* resample_prepare(mt2_model& m, const ResampleRule& r) {
    float*& d = m.rs_tables[{r.o, r.n}];
    if (d) return d;
    std::vector<float> h((size_t)r.n * r.taps);
    resample_table(r, h.data(), true);
    float* t = nullptr;
    MT2_HIP(hipMalloc(reinterpret_cast<void**>(&t), h.size() * sizeof(float)));
    m.dev_allocs.push_back(t);
    MT2_HIP(hipMemcpy(t, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return d = t;
}

static void resample_run(const Ctx& c, const float* wav, const int* lens, int L_max, int B, int sr_in, int sr_out, int flags,
                         float* out, int Lout_max, int32_t* out_lens) {
    // everything is checked before the first launch: a refused call leaves `out` as it was
    ResampleRule r{};
    if (const char* why = resample_rule(sr_in, sr_out, &r)) throw Error(std::string("mt2_resample: ") + why);
    MT2_REQUIRE((flags & ~MT2_RESAMPLE_NORMALIZE) == 0, "unknown resample flag");
    MT2_REQUIRE(wav != nullptr && out != nullptr && lens != nullptr && ((uintptr_t)wav & 3) == 0, "bad buffers");
    check_lens(lens, B, L_max, "waveform length outside [1, L_max]");
    std::vector<int> lout(B), tile_b, tile_i0;
    for (int b = 0; b < B; ++b) {
        const long long lo = resample_out_len(r, lens[b]);
        MT2_REQUIRE(lo <= Lout_max, "Lout_max smaller than ceil(n * L / o)");
        lout[b] = (int)lo;
    }
    for (int b = 0; b < B; ++b)
        for (long long i0 = 0; i0 * r.n < Lout_max; i0 += r.tb) { tile_b.push_back(b); tile_i0.push_back((int)i0); }
    ResampleP p{};
    p.table = resample_prepare(c.m, r);
    IntPlan ip;
    const int o_b = ip.add(tile_b), o_i0 = ip.add(tile_i0), o_len = ip.add(lens, B), o_lout = ip.add(lout);
    ip.upload(c.ws, c.m.pinned(), c.s);
    p.wav = wav; p.L_max = L_max; p.r = r;
    p.tile_b = ip.dev(o_b); p.tile_i0 = ip.dev(o_i0); p.tiles = (int)tile_b.size();
    p.len = ip.dev(o_len); p.lout = ip.dev(o_lout);
    p.out = out; p.Lout_max = Lout_max;
    if (flags & MT2_RESAMPLE_NORMALIZE) {
        p.peak = c.ws.get<unsigned>(B);
        MT2_HIP(hipMemsetAsync(p.peak, 0, sizeof(unsigned) * B, c.s));
    }
    MT2_HIP(launch_resample_rows(p, c.s));
    if (p.peak) MT2_HIP(launch_scale_rows(out, Lout_max, p.lout, p.peak, out, Lout_max, Lout_max, B, c.s));
    if (out_lens) std::copy(lout.begin(), lout.end(), out_lens);
}

// out[b, :] = wav[b, :] / max |wav[b, :len[b]]| (audio_io.normalize), zeros beyond len[b]
static void peak_normalize_run(const Ctx& c, const float* wav, const int* lens, int L_max, int B, float* out) {
    MT2_REQUIRE(wav != nullptr && out != nullptr && lens != nullptr, "bad buffers");
    const int mx = check_lens(lens, B, L_max, "waveform length outside [1, L_max]");
    IntPlan ip;
    const int o_len = ip.add(lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    unsigned* peak = c.ws.get<unsigned>(B);
    MT2_HIP(hipMemsetAsync(peak, 0, sizeof(unsigned) * B, c.s));
    MT2_HIP(launch_peak_rows(wav, L_max, ip.dev(o_len), mx, B, peak, c.s));
    MT2_HIP(launch_scale_rows(wav, L_max, ip.dev(o_len), peak, out, L_max, L_max, B, c.s));
}

// models/megatts2.py:337  librosa.effects.trim: leading / trailing silence cut off by the rule of trim.hip.  The cut is found and
// applied on the device; it travels to the host (one copy, one synchronise) only for a caller that asks for `bounds`.
static void trim_run(const Ctx& c, const float* wav, const int* lens, int L_max, int B, float top_db, float* out, int Lout_max,
                     int32_t* bounds, float* energy, int F_max) {
    // everything is checked before the first launch: a refused call leaves `out` as it was
    MT2_REQUIRE(std::isfinite(top_db) && top_db > 0.0f, "top_db must be finite and > 0");
    MT2_REQUIRE(wav != nullptr && out != nullptr && lens != nullptr && ((uintptr_t)wav & 3) == 0 && ((uintptr_t)out & 3) == 0, "bad buffers");
    const int mx = check_lens(lens, B, L_max, "waveform length outside [1, L_max]");
    MT2_REQUIRE(mx <= INT_MAX - 4 * MT2_TRIM_HOP && B <= 65535, "waveform too long or batch too large");
    MT2_REQUIRE(Lout_max >= mx, "Lout_max smaller than the longest utterance (the cut is not known before the call)");
    MT2_REQUIRE(energy == nullptr || F_max >= trim_frames(mx), "F_max smaller than 1 + max length / 512");
    MT2_REQUIRE(!spans_overlap({out, sizeof(float) * (size_t)B * Lout_max}, {wav, sizeof(float) * (size_t)B * L_max}), "out overlaps wav");
    IntPlan ip;
    const int o_len = ip.add(lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    TrimP p{};
    p.wav = wav; p.L_max = L_max; p.len = ip.dev(o_len); p.max_len = mx; p.B = B;
    p.factor = trim_factor(top_db);
    p.NB = (mx + MT2_TRIM_HOP - 1) / MT2_TRIM_HOP;
    p.sums = c.ws.get<float>((size_t)B * p.NB);
    unsigned* words = c.ws.get<unsigned>((size_t)3 * B);          // peak | first | last
    p.peak = words; p.first = words + B; p.last = reinterpret_cast<int*>(words + 2 * B);
    p.out = out; p.Lout_max = Lout_max; p.energy = energy; p.F_max = F_max;
    MT2_HIP(hipMemsetAsync(p.peak, 0, sizeof(unsigned) * B, c.s));
    MT2_HIP(hipMemsetAsync(p.first, 0xFF, sizeof(unsigned) * 2 * B, c.s));      // first = UINT_MAX, last = -1
    MT2_HIP(launch_trim(p, c.s));
    if (bounds) {
        unsigned* st = static_cast<unsigned*>(c.m.pinned().alloc(sizeof(unsigned) * 2 * B));      // handle-owned staging
        MT2_HIP(hipMemcpyAsync(st, p.first, sizeof(unsigned) * 2 * B, hipMemcpyDeviceToHost, c.s));
        MT2_HIP(hipStreamSynchronize(c.s));
        for (int b = 0; b < B; ++b) trim_bounds(st[b], (int)st[B + b], lens[b], &bounds[2 * b], &bounds[2 * b + 1]);
    }
}

// ---- F0 by YIN and the pitch moments (f0.hip) ------------------------------------------------------------------------------------
// The parameters of the rule, checked before anything else (host only); -> (tau_min, tau_max)
static void f0_check_rule(int sample_rate, int hop, float fmin, float fmax, int* lag_min, int* lag_max) {
    MT2_REQUIRE(sample_rate >= 1, "sample_rate < 1");
    MT2_REQUIRE(hop >= 1 && hop <= MT2_F0_FRAME, "hop outside [1, 1024]");
    MT2_REQUIRE(std::isfinite(fmin) && std::isfinite(fmax) && fmin > 0.0f && fmax > 0.0f, "fmin / fmax must be finite and > 0");
    MT2_REQUIRE(f0_lags(sample_rate, fmin, fmax, lag_min, lag_max),
                "lags refused: need 2 <= ceil(sample_rate / fmax) < floor(sample_rate / fmin) <= 256");
}
// every refusal of mt2_f0_yin, decided on the host before the first HIP call; -> max_b lens[b]
static int f0_check_call(const float* wav, const int* lens, int L_max, int B, int hop, float threshold, const float* f0, const float* cmnd,
                         const int32_t* lag, int T_max, const float* diff) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(wav != nullptr && lens != nullptr && f0 != nullptr && L_max >= 1, "bad buffers");
    MT2_REQUIRE((((uintptr_t)wav | (uintptr_t)f0 | (uintptr_t)cmnd | (uintptr_t)lag | (uintptr_t)diff) & 3) == 0, "misaligned buffers");
    MT2_REQUIRE(threshold > 0.0f && threshold <= 1.0f, "threshold outside (0, 1]");
    const int mx = check_lens(lens, B, L_max, "waveform length outside [1, L_max]");
    MT2_REQUIRE(T_max >= 1 + mx / hop, "T_max smaller than 1 + max length / hop");
    const size_t nw = sizeof(float) * (size_t)B * L_max, nt = sizeof(float) * (size_t)B * T_max;
    const Span w{wav, nw};
    MT2_REQUIRE(!spans_overlap({f0, nt}, w) && !spans_overlap({cmnd, nt}, w) && !spans_overlap({lag, nt}, w) &&
                    !spans_overlap({diff, nt * (MT2_F0_MAX_LAG + 1)}, w),
                "an output overlaps wav");
    return mx;
}
// what mt2_f0_yin and mt2_f0_track share of their arguments, and the kernels' F0P of it (`len`: the lengths on the device)
struct F0Args {
    const float* wav; const int* lens; int L_max, B, max_len, sample_rate, hop, lag_min, lag_max; float threshold;
    float* f0; float* cmnd; int32_t* lag; int T_max; float* diff;
};
static F0P f0_params(const F0Args& a, const int* len) {
    F0P p{};
    p.wav = a.wav; p.L_max = a.L_max; p.len = len; p.max_len = a.max_len; p.B = a.B;
    p.sample_rate = a.sample_rate; p.hop = a.hop; p.lag_min = a.lag_min; p.lag_max = a.lag_max; p.threshold = a.threshold;
    p.f0 = a.f0; p.T_max = a.T_max; p.cmnd = a.cmnd; p.lag = a.lag; p.diff = a.diff;
    return p;
}
// enqueues only: the lengths travel in the call's one IntPlan upload
static void f0_run(const Ctx& c, const F0Args& a) {
    IntPlan ip;
    const int o_len = ip.add(a.lens, a.B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    MT2_HIP(launch_f0_yin(f0_params(a, ip.dev(o_len)), c.s));
}
// mt2_f0_track: the two costs
static void f0_track_check_costs(float octave_cost, float jump_cost) {
    MT2_REQUIRE(std::isfinite(octave_cost) && octave_cost >= 0.0f, "octave_cost must be finite and >= 0");
    MT2_REQUIRE(std::isfinite(jump_cost) && jump_cost >= 0.0f, "jump_cost must be finite and >= 0");
}
// ... and the arena of a call with B utterances and T_max frames, in carve order: the plan (the lengths and the lg table), d', psi
struct F0TrackWs { float* dprime; unsigned char* psi; };
template <class Ws> static F0TrackWs f0_track_carve(Ws& ws, IntPlan& ip, size_t B, size_t T_max) {
    F0TrackWs w{};
    ip.carve(ws);
    w.dprime = ws.template get<float>(B * T_max * (MT2_F0_MAX_LAG + 1));
    w.psi = ws.template get<unsigned char>(B * T_max * 256);
    return w;
}
static long long f0_track_arena_bytes(int B, long long T_max) {
    IntPlan ip;
    ip.add_fill(B, 0);
    ip.add_fill(256, 0);
    ArenaCount count;
    f0_track_carve(count, ip, B, T_max);
    return (long long)count.bytes;
}
// enqueues only: the lengths and the lg table travel in the call's one IntPlan upload
static void f0_track_run(const Ctx& c, const F0Args& a, float octave_cost, float jump_cost) {
    float lg[256];
    f0_track_table(a.lag_min, a.lag_max, lg);
    IntPlan ip;
    const int o_len = ip.add(a.lens, a.B), o_lg = ip.add_bits(lg, 256);
    const F0TrackWs w = f0_track_carve(c.ws, ip, a.B, a.T_max);
    ip.send(c.m.pinned(), c.s);
    F0TrackP q{};
    q.y = f0_params(a, ip.dev(o_len));
    q.octave_cost = octave_cost; q.jump_cost = jump_cost;
    q.lg = reinterpret_cast<const float*>(ip.dev(o_lg));
    q.dprime = w.dprime; q.psi = w.psi;
    Stages st(c.m, c.s);
    st.mark("start");
    MT2_HIP(launch_f0_cmnd(q, c.s));
    st.mark("f0_cmnd");
    MT2_HIP(launch_f0_viterbi(q, c.s));
    st.mark("f0_viterbi");
    st.finish();
}
static void f0_stats_check(const float* f0, const int* frame_lens, int T_max, int B, const double* stats) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(f0 != nullptr && frame_lens != nullptr && stats != nullptr && T_max >= 1, "bad buffers");
    MT2_REQUIRE(((uintptr_t)f0 & 3) == 0 && ((uintptr_t)stats & 7) == 0, "misaligned buffers");
    check_lens(frame_lens, B, T_max, "frame count outside [1, T_max]");
    MT2_REQUIRE(!spans_overlap({stats, sizeof(double) * 6 * (size_t)B}, {f0, sizeof(float) * (size_t)B * T_max}), "stats overlaps f0");
}
static void f0_stats_run(const Ctx& c, const float* f0, const int* frame_lens, int T_max, int B, double* stats) {
    IntPlan ip;
    const int o_len = ip.add(frame_lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    MT2_HIP(launch_f0_stats(f0, ip.dev(o_len), T_max, B, stats, c.s));
}

// ---- formant candidates by linear prediction and the formant figures (formants.hip) -----------------------------------------------
// The parameters of the rule that mt2_formant_query shares with the call, checked before anything else (host only)
static void formant_check_rule(int sample_rate, int hop, int window, int order) {
    MT2_REQUIRE(sample_rate >= 1, "sample_rate < 1");
    MT2_REQUIRE(hop >= 1 && hop <= 1024, "hop outside [1, 1024]");
    MT2_REQUIRE(window >= 64 && window <= MT2_FORMANT_MAX_WINDOW && window % 2 == 0, "window outside [64, 1024] or odd");
    MT2_REQUIRE(order >= 2 && order <= MT2_FORMANT_MAX_ORDER && order % 2 == 0, "order outside [2, 32] or odd");
    MT2_REQUIRE(order < window, "order >= window");
}
static void formant_check_kind(int kind) { MT2_REQUIRE(kind == MT2_FORMANT_HANN || kind == MT2_FORMANT_RECT, "unknown window kind"); }
static void formant_check_config(int sample_rate, int hop, const mt2_formant_config* cfg) {
    MT2_REQUIRE(cfg != nullptr, "null formant config");
    formant_check_rule(sample_rate, hop, cfg->window, cfg->order);
    formant_check_kind(cfg->kind);
    MT2_REQUIRE(cfg->reserved == 0, "mt2_formant_config.reserved must be 0");
    MT2_REQUIRE(std::isfinite(cfg->preemphasis_hz) && cfg->preemphasis_hz >= 0.0, "preemphasis_hz must be finite and >= 0");
    MT2_REQUIRE(std::isfinite(cfg->fmin_hz) && cfg->fmin_hz >= 0.0, "fmin_hz must be finite and >= 0");
    MT2_REQUIRE(std::isfinite(cfg->max_bandwidth_hz) && cfg->max_bandwidth_hz >= 0.0, "max_bandwidth_hz must be finite and >= 0");
    MT2_REQUIRE(cfg->fmin_hz < (double)sample_rate / 4.0, "fmin_hz >= sample_rate / 4");
}
struct FormantOut { float* freq; float* bw; int32_t* count; int T_max; double* lpc; double* err; double* autocorr; double* roots; int32_t* iters; };
// every refusal of mt2_lpc_formants beyond the config, decided on the host before the first HIP call; -> max_b lens[b]
static int formant_check_call(const float* wav, const int* lens, int L_max, int B, int hop, int P, const FormantOut& o) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(wav != nullptr && lens != nullptr && o.freq != nullptr && o.bw != nullptr && o.count != nullptr && L_max >= 1, "bad buffers");
    MT2_REQUIRE((((uintptr_t)wav | (uintptr_t)o.freq | (uintptr_t)o.bw | (uintptr_t)o.count | (uintptr_t)o.iters) & 3) == 0 &&
                    (((uintptr_t)o.lpc | (uintptr_t)o.err | (uintptr_t)o.autocorr | (uintptr_t)o.roots) & 7) == 0,
                "misaligned buffers");
    const int mx = check_lens(lens, B, L_max, "waveform length outside [1, L_max]");
    MT2_REQUIRE((long long)o.T_max >= 1ll + mx / hop, "T_max smaller than 1 + max length / hop");
    const size_t nt = (size_t)B * o.T_max;
    MT2_REQUIRE(!outputs_overlap({{o.freq, 4 * nt * MT2_FORMANT_MAX}, {o.bw, 4 * nt * MT2_FORMANT_MAX}, {o.count, 4 * nt}, {o.lpc, 8 * nt * (P + 1)},
                                  {o.err, 8 * nt}, {o.autocorr, 8 * nt * (P + 1)}, {o.roots, 16 * nt * P}, {o.iters, 4 * nt}},
                                 {{wav, sizeof(float) * (size_t)B * L_max}}),
                "overlapping buffers");
    return mx;
}
static const double* formant_prepare(mt2_model& m, int W, int kind) {
    double*& d = m.fm_windows[{W, kind}];
    if (d) return d;
    std::vector<double> h(W);
    formant_window_table(W, kind, h.data());
    double* t = nullptr;
    MT2_HIP(hipMalloc(reinterpret_cast<void**>(&t), h.size() * sizeof(double)));
    m.dev_allocs.push_back(t);
    MT2_HIP(hipMemcpy(t, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    return d = t;
}
// the arena of one mt2_lpc_formants call
static long long formant_arena_bytes() { return (long long)arena_round(sizeof(int) * 65535); }
// enqueues only (behind the first call with a new window, which uploads its table): the lengths travel in the call's one upload
static void formant_run(const Ctx& c, const float* wav, const int* lens, int L_max, int B, int max_len, int sample_rate, int hop,
                        const mt2_formant_config& cfg, const FormantOut& o) {
    FormantP p{};
    p.window = formant_prepare(c.m, cfg.window, cfg.kind);
    // the arena of the call: the lengths, in the room of the largest batch whatever B - so that mt2_formant_query needs no B
    int* st = static_cast<int*>(c.m.pinned().alloc(sizeof(int) * B));      // handle-owned staging
    std::copy(lens, lens + B, st);
    int* d_len = c.ws.get<int>(65535);
    MT2_HIP(hipMemcpyAsync(d_len, st, sizeof(int) * B, hipMemcpyHostToDevice, c.s));
    p.wav = wav; p.L_max = L_max; p.len = d_len; p.max_len = max_len; p.B = B;
    p.sample_rate = sample_rate; p.hop = hop; p.W = cfg.window; p.P = cfg.order;
    p.alpha = formant_alpha(cfg.preemphasis_hz, sample_rate); p.fmin = cfg.fmin_hz; p.max_bw = cfg.max_bandwidth_hz;
    p.freq = o.freq; p.bw = o.bw; p.count = o.count; p.T_max = o.T_max;
    p.lpc = o.lpc; p.err = o.err; p.autocorr = o.autocorr; p.roots = o.roots; p.iters = o.iters;
    MT2_HIP(launch_formants(p, c.s));
}
static void formant_stats_check(const float* freq, const int32_t* count, const float* f0, const int* frame_lens, int T_max, int B,
                                const double* stats) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(freq != nullptr && count != nullptr && frame_lens != nullptr && stats != nullptr && T_max >= 1, "bad buffers");
    MT2_REQUIRE((((uintptr_t)freq | (uintptr_t)count | (uintptr_t)f0) & 3) == 0 && ((uintptr_t)stats & 7) == 0, "misaligned buffers");
    check_lens(frame_lens, B, T_max, "frame count outside [1, T_max]");
    const size_t nt = (size_t)B * T_max;
    MT2_REQUIRE(!outputs_overlap({{stats, sizeof(double) * MT2_FORMANT_STAT_FIELDS * (size_t)B}},
                                 {{freq, 4 * nt * MT2_FORMANT_MAX}, {count, 4 * nt}, {f0, 4 * nt}}),
                "stats overlaps an input");
}
static void formant_stats_run(const Ctx& c, const float* freq, const int32_t* count, const float* f0, const int* frame_lens, int T_max, int B,
                              double* stats) {
    IntPlan ip;
    const int o_len = ip.add(frame_lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    MT2_HIP(launch_formant_stats(freq, count, f0, ip.dev(o_len), T_max, B, stats, c.s));
}

// ---- formant tracks across frames (formant_track.hip): every refusal is decided here, on the host, before the first HIP call -------
static_assert(sizeof(mt2_formant_track_config) == 72 && offsetof(mt2_formant_track_config, ref_hz) == 8 &&
                  offsetof(mt2_formant_track_config, freq_cost) == 48 && offsetof(mt2_formant_track_config, jump_cost) == 64,
              "runtime.MT2FormantTrackConfig mirrors this layout");
static void formant_track_check_shape(int tracks, long long T_max, int B) {
    MT2_REQUIRE(tracks >= 1 && tracks <= MT2_FORMANT_MAX, "tracks outside [1, 5]");
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(T_max >= 1 && T_max <= INT_MAX, "T_max outside [1, 2^31)");
}
static void formant_track_check_config(const mt2_formant_track_config* cfg) {
    MT2_REQUIRE(cfg != nullptr, "null formant track config");
    MT2_REQUIRE(cfg->tracks >= 1 && cfg->tracks <= MT2_FORMANT_MAX, "tracks outside [1, 5]");
    MT2_REQUIRE(cfg->reserved == 0, "mt2_formant_track_config.reserved must be 0");
    for (int q = 0; q < cfg->tracks; ++q) MT2_REQUIRE(std::isfinite(cfg->ref_hz[q]) && cfg->ref_hz[q] > 0.0, "ref_hz must be finite and > 0");
    MT2_REQUIRE(std::isfinite(cfg->freq_cost) && cfg->freq_cost >= 0.0, "freq_cost must be finite and >= 0");
    MT2_REQUIRE(std::isfinite(cfg->bw_cost) && cfg->bw_cost >= 0.0, "bw_cost must be finite and >= 0");
    MT2_REQUIRE(std::isfinite(cfg->jump_cost) && cfg->jump_cost >= 0.0, "jump_cost must be finite and >= 0");
}
struct FormantTrackIO { const float* freq; const float* bw; const int32_t* count; float* tfreq; float* tbw; int32_t* tcount; int32_t* sel; };
static void formant_track_check_call(const FormantTrackIO& a, const int* frame_lens, int T_max, int B) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(a.freq != nullptr && a.bw != nullptr && a.count != nullptr && frame_lens != nullptr && a.tfreq != nullptr && a.tbw != nullptr &&
                    a.tcount != nullptr && T_max >= 1,
                "bad buffers");
    MT2_REQUIRE((((uintptr_t)a.freq | (uintptr_t)a.bw | (uintptr_t)a.count | (uintptr_t)a.tfreq | (uintptr_t)a.tbw | (uintptr_t)a.tcount |
                  (uintptr_t)a.sel) & 3) == 0,
                "misaligned buffers");
    check_lens(frame_lens, B, T_max, "frame count outside [1, T_max]");
    const size_t nt = 4 * (size_t)B * T_max, n5 = nt * MT2_FORMANT_MAX;
    MT2_REQUIRE(!outputs_overlap({{a.tfreq, n5}, {a.tbw, n5}, {a.tcount, nt}, {a.sel, n5}}, {{a.freq, n5}, {a.bw, n5}, {a.count, nt}}),
                "overlapping buffers");
}
// the arena of one mt2_formant_track call, in carve order: the lengths in the room of the largest batch, psi
struct FormantTrackWs { int* len; unsigned char* psi; };
template <class Ws> static FormantTrackWs formant_track_carve(Ws& ws, size_t B, size_t T_max) {
    FormantTrackWs w{};
    w.len = ws.template get<int>(65535);
    w.psi = ws.template get<unsigned char>(16 * B * T_max);
    return w;
}
static long long formant_track_arena_bytes(int B, long long T_max) {
    ArenaCount count;
    formant_track_carve(count, B, T_max);
    return (long long)count.bytes;
}
// enqueues only: the lengths travel in the call's one upload
static void formant_track_run(const Ctx& c, const FormantTrackIO& a, const int* frame_lens, int T_max, int B, const mt2_formant_track_config& cfg) {
    const FormantTrackWs w = formant_track_carve(c.ws, B, T_max);
    int* st = static_cast<int*>(c.m.pinned().alloc(sizeof(int) * B));      // handle-owned staging
    std::copy(frame_lens, frame_lens + B, st);
    MT2_HIP(hipMemcpyAsync(w.len, st, sizeof(int) * B, hipMemcpyHostToDevice, c.s));
    FormantTrackP p{};
    p.freq = a.freq; p.bw = a.bw; p.count = a.count; p.len = w.len; p.T_max = T_max; p.B = B;
    p.K = cfg.tracks; p.S = formant_track_states(cfg.tracks);
    for (int q = 0; q < MT2_FORMANT_MAX; ++q) p.ref[q] = q < cfg.tracks ? cfg.ref_hz[q] : 0.0;
    p.fc = cfg.freq_cost; p.bc = cfg.bw_cost; p.jc = cfg.jump_cost;
    formant_track_table(cfg.tracks, p.st);
    p.psi = w.psi; p.tfreq = a.tfreq; p.tbw = a.tbw; p.tcount = a.tcount; p.sel = a.sel;
    Stages stg(c.m, c.s);
    stg.mark("start");
    MT2_HIP(launch_formant_track(p, c.s));
    stg.mark("formant_track");
    stg.finish();
}

// ---- per-phone prosody (prosody.hip): every refusal is decided here, on the host, before the first HIP call -------------------------
// mt2_frame_energy; -> max_b lens[b]
static int energy_check(const float* wav, const int* lens, int L_max, int B, int hop, const float* energy, int T_max) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(hop >= 1 && hop <= MT2_F0_FRAME, "hop outside [1, 1024]");
    MT2_REQUIRE(wav != nullptr && lens != nullptr && energy != nullptr && L_max >= 1, "bad buffers");
    MT2_REQUIRE((((uintptr_t)wav | (uintptr_t)energy) & 3) == 0, "misaligned buffers");
    const int mx = check_lens(lens, B, L_max, "waveform length outside [1, L_max]");
    MT2_REQUIRE(T_max >= 1 + mx / hop, "T_max smaller than 1 + max length / hop");
    MT2_REQUIRE(!spans_overlap({energy, sizeof(float) * (size_t)B * T_max}, {wav, sizeof(float) * (size_t)B * L_max}), "energy overlaps wav");
    return mx;
}
static void energy_run(const Ctx& c, const float* wav, const int* lens, int L_max, int B, int max_len, int hop, float* energy, int T_max) {
    IntPlan ip;
    const int o_len = ip.add(lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    EnergyP p{};
    p.wav = wav; p.L_max = L_max; p.len = ip.dev(o_len); p.max_len = max_len; p.B = B; p.hop = hop; p.energy = energy; p.T_max = T_max;
    MT2_HIP(launch_frame_energy(p, c.s));
}
// mt2_phone_prosody
static void phone_prosody_check(const float* f0, const float* energy, const int* dur, const int* phone_lens, int Np_max,
                                const int* frame_lens, int T_max, int B, const double* out, const long long* dur_sum) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(f0 != nullptr && dur != nullptr && phone_lens != nullptr && frame_lens != nullptr && out != nullptr && Np_max >= 1 &&
                    T_max >= 1, "bad buffers");
    MT2_REQUIRE((((uintptr_t)f0 | (uintptr_t)energy | (uintptr_t)dur) & 3) == 0 && ((uintptr_t)out & 15) == 0 && ((uintptr_t)dur_sum & 7) == 0,
                "misaligned buffers");
    check_lens(phone_lens, B, Np_max, "phone count outside [1, Np_max]");
    check_lens(frame_lens, B, T_max, "frame count outside [1, T_max]");
    const size_t nt = sizeof(float) * (size_t)B * T_max, nd = sizeof(int) * (size_t)B * Np_max, no = sizeof(double) * 8 * (size_t)B * Np_max,
                 ns = sizeof(long long) * (size_t)B;
    MT2_REQUIRE(!outputs_overlap({{out, no}, {dur_sum, ns}}, {{f0, nt}, {energy, nt}, {dur, nd}}), "overlapping buffers");
}
static void phone_prosody_run(const Ctx& c, const float* f0, const float* energy, const int* dur, const int* phone_lens, int Np_max,
                              const int* frame_lens, int T_max, int B, double* out, long long* dur_sum) {
    IntPlan ip;
    const int o_np = ip.add(phone_lens, B), o_t = ip.add(frame_lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    PhoneProsodyP p{};
    p.f0 = f0; p.energy = energy; p.T_max = T_max; p.dur = dur; p.Np_max = Np_max; p.np_len = ip.dev(o_np); p.t_len = ip.dev(o_t);
    p.B = B; p.out = out; p.dur_sum = dur_sum;
    MT2_HIP(launch_phone_prosody(p, c.s));
}
// mt2_pitch_contour
static void pitch_contour_check(const float* f0, const int* frame_lens, int T_max, int B, int center, const float* st, const int* n_voiced,
                                const int* index) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(center == 0 || center == 1, "center must be 0 or 1");
    MT2_REQUIRE(f0 != nullptr && frame_lens != nullptr && st != nullptr && n_voiced != nullptr && T_max >= 1, "bad buffers");
    MT2_REQUIRE((((uintptr_t)f0 | (uintptr_t)st | (uintptr_t)n_voiced | (uintptr_t)index) & 3) == 0, "misaligned buffers");
    check_lens(frame_lens, B, T_max, "frame count outside [1, T_max]");
    const size_t nt = sizeof(float) * (size_t)B * T_max, nb = sizeof(int) * (size_t)B;
    MT2_REQUIRE(!outputs_overlap({{st, nt}, {index, nt}, {n_voiced, nb}}, {{f0, nt}}), "overlapping buffers");
}
static void pitch_contour_run(const Ctx& c, const float* f0, const int* frame_lens, int T_max, int B, int center, float* st, int* n_voiced,
                              int* index) {
    IntPlan ip;
    const int o_t = ip.add(frame_lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    PitchContourP p{};
    p.f0 = f0; p.T_max = T_max; p.t_len = ip.dev(o_t); p.B = B; p.center = center; p.st = st; p.n_voiced = n_voiced; p.index = index;
    MT2_HIP(launch_pitch_contour(p, c.s));
}

// ---- integrated loudness and loudness normalisation (loudness.hip): every refusal is decided here, on the host, before the first HIP call
// the rule on the rate, for every function of the family, and with it the rule on the longest waveform, for its queries
constexpr int kLoudMaxLen = INT_MAX - 8 * 19200;
static void loudness_check_rate(int sample_rate) { MT2_REQUIRE(loudness_rate_ok(sample_rate), "sample_rate must be a multiple of 10 in [8000, 192000]"); }
static void loudness_check_query(int sample_rate, long long L) {
    loudness_check_rate(sample_rate);
    MT2_REQUIRE(L >= 1 && L <= kLoudMaxLen, "L outside [1, 2^31 - 153600)");
}
// the waveform batch of a loudness, EBU or limiter call; its check hands it back with max_len = max_b lens[b] filled in
struct WavArgs { const float* wav; const int* lens; int L_max, B, max_len, sample_rate; };
// out == nullptr: the measuring call
static WavArgs loudness_check(WavArgs a, double target_lufs, double peak_ceiling, const float* out, const double* stats, const double* momentary,
                              int NB_max) {
    MT2_REQUIRE(a.B >= 1 && a.B <= 65535, "B outside [1, 65535]");
    loudness_check_rate(a.sample_rate);
    MT2_REQUIRE(std::isfinite(target_lufs) && std::isfinite(peak_ceiling), "target_lufs / peak_ceiling must be finite");
    MT2_REQUIRE(a.wav != nullptr && a.lens != nullptr && a.L_max >= 1, "bad buffers");
    MT2_REQUIRE((((uintptr_t)a.wav | (uintptr_t)out) & 3) == 0 && (((uintptr_t)stats | (uintptr_t)momentary) & 7) == 0, "misaligned buffers");
    a.max_len = check_lens(a.lens, a.B, a.L_max, "waveform length outside [1, L_max]");
    MT2_REQUIRE(a.max_len <= kLoudMaxLen, "waveform too long");
    const int nb = std::max(a.max_len / (a.sample_rate / 10) - 3, 0);
    MT2_REQUIRE(momentary == nullptr || (NB_max >= 1 && NB_max >= nb), "NB_max smaller than the blocks of the longest utterance (or < 1)");
    const size_t nw = sizeof(float) * (size_t)a.B * a.L_max, nst = sizeof(double) * 8 * (size_t)a.B, nm = sizeof(double) * (size_t)a.B * std::max(NB_max, 0);
    MT2_REQUIRE(out == a.wav || !spans_overlap({out, nw}, {a.wav, nw}), "out overlaps wav without being wav");
    MT2_REQUIRE(!outputs_overlap({{stats, nst}, {momentary, nm}}, {{a.wav, nw}, {out, nw}}), "overlapping buffers");
    return a;
}
// The arena of one loudness / EBU call, in carve order: the plan (the lengths, the carry matrix and, for EBU, the filter table), the
// chunk states, S, the words (peak | gain, and EBU's true peak) and, for EBU alone, the loudness rows and z3 / the keys
struct LoudWs { double *state, *sums; unsigned* words; double *row8, *keys; };
template <class Ws> static LoudWs loudness_carve(Ws& ws, IntPlan& ip, size_t B, int NS, bool ebu) {
    LoudWs w{};
    ip.carve(ws);
    w.state = ws.template get<double>(B * NS * 4);
    w.sums = ws.template get<double>(B * NS);
    w.words = ws.template get<unsigned>((ebu ? 3 : 2) * B);
    if (ebu) {
        w.row8 = ws.template get<double>(8 * B);
        w.keys = ws.template get<double>(B * std::max(NS - 29, 0));
    }
    return w;
}
// B utterances, the longest of max_len samples
static long long loudness_arena_bytes(int sample_rate, long long max_len, int B, bool ebu) {
    IntPlan ip;
    ip.add_fill(B, 0);
    ip.add_fill(32, 0);
    if (ebu) ip.add_fill((size_t)true_peak_oversample(sample_rate) * MT2_TP_TAPS, 0);
    ArenaCount count;
    loudness_carve(count, ip, B, (int)(max_len / (sample_rate / 10)), ebu);
    return (long long)count.bytes;
}
// the four kernels of the loudness rule on p;  st: where their marks go, or nullptr (a pass of the limiter measures under one mark)
static void loudness_launches(const Ctx& c, const LoudnessP& p, Stages* st) {
    MT2_HIP(launch_loudness_filter(p, c.s));
    if (st) st->mark("loud_zero_state");
    MT2_HIP(launch_loudness_carry(p, c.s));
    if (st) st->mark("loud_carry");
    MT2_HIP(launch_loudness_sums(p, c.s));
    if (st) st->mark("loud_sums");
    MT2_HIP(launch_loudness_gate(p, c.s));
    if (st) st->mark("loud_gate");
}
// What the loudness and the EBU call share, up to and including the gate kernel and its mark.  The caller has set the gate's own
// fields of p (targets, out, stats, momentary); the rest of p is filled here.  `table`: nullptr, or what the EBU call adds - its
// filter table [o][24] as the plan's third entry, the third word row, the loudness rows and the keys.  Its gate kernel only measures,
// into the rows (ebu.hip forms the gain); the loudness call's forms the gain where there is an `out` to scale.
// -> the arena, and the table on the device
struct LoudChain { LoudWs w; const float* table; };
static LoudChain loudness_chain(const Ctx& c, Stages& st, LoudnessP& p, const WavArgs& a, const std::vector<float>* table) {
    p.h = a.sample_rate / 10;
    loudness_coeffs(a.sample_rate, p.c);
    if (c.m.loud_rate != a.sample_rate) {          // a function of the rate alone: kept by the handle
        loudness_carry_matrix(p.c, p.h, c.m.loud_M);
        c.m.loud_rate = a.sample_rate;
    }
    IntPlan ip;
    const int o_len = ip.add(a.lens, a.B), o_m = ip.add_bits(c.m.loud_M, 16), o_t = table ? ip.add_bits(table->data(), table->size()) : 0;
    p.NS = a.max_len / p.h;
    const LoudWs w = loudness_carve(c.ws, ip, a.B, p.NS, table != nullptr);
    ip.send(c.m.pinned(), c.s);
    p.wav = a.wav; p.L_max = a.L_max; p.len = ip.dev(o_len); p.max_len = a.max_len; p.B = a.B; p.M = ip.dev(o_m);
    p.state = w.state; p.sums = w.sums; p.peak = w.words;
    if (table) p.stats = w.row8;
    else if (p.out) p.gain = reinterpret_cast<float*>(w.words + a.B);
    MT2_HIP(hipMemsetAsync(w.words, 0, sizeof(unsigned) * (table ? 3 : 1) * a.B, c.s));
    st.mark("start");
    loudness_launches(c, p, &st);
    return {w, table ? reinterpret_cast<const float*>(ip.dev(o_t)) : nullptr};
}
// enqueues only: the lengths and the carry matrix travel in the call's one IntPlan upload; the gain is formed and read on the device
static void loudness_run(const Ctx& c, const WavArgs& a, double target_lufs, double peak_ceiling, float* out, double* stats, double* momentary,
                         int NB_max) {
    LoudnessP p{};
    p.target_lufs = target_lufs; p.peak_ceiling = peak_ceiling; p.out = out; p.stats = stats; p.momentary = momentary; p.NB_max = NB_max;
    Stages st(c.m, c.s);
    (void)loudness_chain(c, st, p, a, nullptr);
    if (out) {
        MT2_HIP(launch_loudness_scale(p, c.s));
        st.mark("loud_scale");
    }
    st.finish();
}

// ---- EBU-mode metering (ebu.hip) behind the loudness kernels: every refusal is decided here, on the host, before the first HIP call
// out == nullptr: the measuring call
static WavArgs ebu_check(WavArgs a, double target_lufs, double ceiling_dbtp, const float* out, const double* stats, const double* momentary,
                         int NB_max, const double* short_term, int NST_max) {
    a = loudness_check(a, target_lufs, ceiling_dbtp, out, nullptr, momentary, NB_max);
    MT2_REQUIRE((((uintptr_t)stats | (uintptr_t)short_term) & 7) == 0, "misaligned buffers");
    const int nst = std::max(a.max_len / (a.sample_rate / 10) - 29, 0);
    MT2_REQUIRE(short_term == nullptr || (NST_max >= 1 && NST_max >= nst), "NST_max smaller than the short-term blocks of the longest utterance (or < 1)");
    const size_t nw = sizeof(float) * (size_t)a.B * a.L_max, ns = sizeof(double) * MT2_EBU_FIELDS * (size_t)a.B,
                 nm = sizeof(double) * (size_t)a.B * std::max(NB_max, 0), nt = sizeof(double) * (size_t)a.B * std::max(NST_max, 0);
    MT2_REQUIRE(!outputs_overlap({{stats, ns}, {short_term, nt}}, {{a.wav, nw}, {out, nw}, {momentary, nm}}), "overlapping buffers");
    return a;
}
// The EBU meter of ebu_run and limiter_run: the filter table, loudness_chain (one IntPlan upload; the loudness kernels leave their row
// in the arena), then the true-peak and the range kernel.  The caller has set its own fields: of p as for loudness_chain, of e the
// targets and the short-term output.  gain: whether the range kernel forms the gain word.  row18(): where the 18 doubles go - asked
// behind loudness_chain, so that a caller can carve what it adds to the arena behind the meter's part.
template <class Row> static void ebu_meter(const Ctx& c, Stages& st, const WavArgs& a, LoudnessP& p, EbuP& e, bool gain, Row&& row18) {
    e.o = true_peak_oversample(a.sample_rate);
    std::vector<float> table((size_t)e.o * MT2_TP_TAPS);
    true_peak_table(a.sample_rate, table.data());
    const LoudChain ch = loudness_chain(c, st, p, a, &table);
    e.wav = a.wav; e.L_max = a.L_max; e.len = p.len; e.max_len = a.max_len; e.B = a.B; e.h = p.h;
    e.table = ch.table; e.sums = p.sums; e.NS = p.NS; e.row8 = ch.w.row8; e.NST = std::max(p.NS - 29, 0); e.keys = ch.w.keys;
    e.tp = ch.w.words + 2 * a.B;                                  // peak | gain | true peak
    e.gain = gain ? reinterpret_cast<float*>(ch.w.words + a.B) : nullptr;
    e.stats = row18();
    MT2_HIP(launch_true_peak(e, c.s));
    st.mark("ebu_true_peak");
    MT2_HIP(launch_loudness_range(e, c.s));
    st.mark("ebu_range");
}
// enqueues only; the gain is formed and read on the device
static void ebu_run(const Ctx& c, const WavArgs& a, double target_lufs, double ceiling_dbtp, float* out, double* stats, double* momentary,
                    int NB_max, double* short_term, int NST_max) {
    LoudnessP p{};
    p.momentary = momentary; p.NB_max = NB_max;
    EbuP e{};
    e.target_lufs = target_lufs; e.ceiling_dbtp = ceiling_dbtp; e.short_term = short_term; e.NST_max = NST_max;
    Stages st(c.m, c.s);
    ebu_meter(c, st, a, p, e, out != nullptr, [&] { return stats; });
    if (out) {
        p.gain = e.gain; p.out = out;
        MT2_HIP(launch_loudness_scale(p, c.s));
        st.mark("loud_scale");
    }
    st.finish();
}

// ---- true-peak look-ahead limiter (limiter.hip) behind the EBU call's kernels: every refusal is decided here, on the host, before the
// first HIP call.  -> H, the half window
static int limiter_check_window(int sample_rate, double window_ms) {
    const int H = limiter_half_window(sample_rate, window_ms);
    MT2_REQUIRE(H >= 1, "window_ms must be finite with round(sample_rate window_ms / 1000) in [1, 1024]");
    return H;
}
static WavArgs limiter_check(WavArgs a, double target_lufs, double ceiling_dbtp, double window_ms, int passes, const float* out,
                             const float* gain, const float* need, const double* stats, int* H) {
    MT2_REQUIRE(out != nullptr, "null out");
    a = ebu_check(a, target_lufs, ceiling_dbtp, out, nullptr, nullptr, 0, nullptr, 0);
    *H = limiter_check_window(a.sample_rate, window_ms);
    MT2_REQUIRE(passes >= 1 && passes <= MT2_LIMITER_MAX_PASSES, "passes outside [1, 4]");
    MT2_REQUIRE((((uintptr_t)gain | (uintptr_t)need) & 3) == 0 && ((uintptr_t)stats & 7) == 0, "misaligned buffers");
    const size_t nw = sizeof(float) * (size_t)a.B * a.L_max, ns = sizeof(double) * MT2_LIMITER_FIELDS * (size_t)a.B;
    MT2_REQUIRE(!outputs_overlap({{gain, nw}, {need, nw}, {stats, ns}}, {{a.wav, nw}, {out, nw}}), "overlapping buffers");
    return a;
}
// What a limiter call takes from the arena behind the EBU call's carve: the weights (a plan of their own), E, the output of a pass
// that is not the last (carved whatever the passes, so that the query needs none), the words of four passes, G | copy flag | t, the
// meter's row and a pass's loudness row
struct LimWs { float *env, *tmp; unsigned* words; float* ctl; double *row18, *rowk; };
template <class Ws> static LimWs limiter_carve(Ws& ws, IntPlan& ip, size_t B, size_t E_ld) {
    LimWs w{};
    ip.carve(ws);
    w.env = ws.template get<float>(B * E_ld);
    w.tmp = ws.template get<float>(B * E_ld);
    w.words = ws.template get<unsigned>(4 * MT2_LIMITER_MAX_PASSES * B);
    w.ctl = ws.template get<float>(3 * B);
    w.row18 = ws.template get<double>(MT2_EBU_FIELDS * B);
    w.rowk = ws.template get<double>(8 * B);
    return w;
}
static long long limiter_arena_bytes(int sample_rate, long long max_len, int B, int H) {
    IntPlan ip;
    ip.add_fill((size_t)limiter_window_words(H), 0);
    ArenaCount count;
    limiter_carve(count, ip, B, (size_t)((max_len + 3) & ~3ll));
    return loudness_arena_bytes(sample_rate, max_len, B, true) + (long long)count.bytes;
}
// enqueues only.  normalizing: G_1 from the input's loudness, `passes` passes;  else one pass with G_host.  The meter runs as in ebu_run,
// into the arena's row;  then the envelope, and per pass the gain kernel, the true peak of its output, the trim, loudness.hip's scale
// kernel on t and - where another pass or the stats need it - the four loudness kernels on the output.
static void limiter_run(const Ctx& c, const WavArgs& a, bool normalizing, float G_host, double target_lufs, double ceiling_dbtp, int H,
                        int passes, float* out, float* gain, float* need, double* stats) {
    const int B = a.B, max_len = a.max_len, E_ld = (max_len + 3) & ~3;
    std::vector<float> win((size_t)2 * H + 1);
    limiter_window(H, win.data());
    IntPlan ipw;
    const int o_w = ipw.add_bits(win.data(), win.size(), (size_t)limiter_window_words(H));
    LimWs w{};
    LoudnessP p{};                                                            // the meter's, kept for the passes
    EbuP e{};
    Stages st(c.m, c.s);
    ebu_meter(c, st, a, p, e, false, [&] {                                    // the limiter's part of the arena, behind the meter's
        w = limiter_carve(c.ws, ipw, B, E_ld);
        ipw.send(c.m.pinned(), c.s);
        MT2_HIP(hipMemsetAsync(w.words, 0, sizeof(unsigned) * 4 * MT2_LIMITER_MAX_PASSES * B, c.s));
        return w.row18;
    });
    LimiterP q{};
    q.wav = a.wav; q.L_max = a.L_max; q.len = p.len; q.max_len = max_len; q.B = B; q.o = e.o; q.table = e.table;
    q.H = H; q.win = reinterpret_cast<const float*>(ipw.dev(o_w));
    q.c = (float)pow(10.0, ceiling_dbtp / 20.0);
    q.env = w.env; q.E_ld = E_ld;
    q.G = w.ctl; q.bypass = reinterpret_cast<int*>(w.ctl + B); q.t = w.ctl + 2 * B;
    q.normalizing = normalizing ? 1 : 0; q.G_host = G_host; q.target_lufs = target_lufs; q.row18 = w.row18;
    MT2_HIP(launch_limiter_envelope(q, c.s));
    MT2_HIP(launch_limiter_step(q, kLimStepInit, c.s));
    st.mark("lim_envelope");
    static const char* const kGainMark[] = {"lim_gain1", "lim_gain2", "lim_gain3", "lim_gain4"};
    static const char* const kTrimMark[] = {"lim_trim1", "lim_trim2", "lim_trim3", "lim_trim4"};
    static const char* const kMeasureMark[] = {"lim_measure1", "lim_measure2", "lim_measure3", "lim_measure4"};
    for (int k = 0; k < passes; ++k) {
        const bool last = k == passes - 1;
        unsigned* const words = w.words + (size_t)4 * k * B;                  // min | count | true peak | peak
        q.out = last ? out : w.tmp; q.out_ld = last ? a.L_max : E_ld;
        q.gain = last ? gain : nullptr; q.need = last ? need : nullptr;
        q.minkey = words; q.count = words + B; q.tp = words + 2 * B;
        MT2_HIP(launch_limiter_gain(q, c.s));
        st.mark(kGainMark[k]);
        EbuP ek{};
        ek.wav = q.out; ek.L_max = q.out_ld; ek.len = p.len; ek.max_len = max_len; ek.B = B; ek.o = e.o; ek.table = e.table;
        ek.tp = words + 2 * B;
        MT2_HIP(launch_true_peak(ek, c.s));
        MT2_HIP(launch_limiter_step(q, kLimStepTrim, c.s));
        LoudnessP pk = p;
        pk.wav = q.out; pk.L_max = q.out_ld; pk.out = q.out; pk.gain = q.t; pk.peak = words + 3 * B;
        pk.stats = w.rowk; pk.momentary = nullptr; pk.NB_max = 0;
        MT2_HIP(launch_loudness_scale(pk, c.s));
        st.mark(kTrimMark[k]);
        q.rowk = nullptr;
        if (!last || stats) {
            pk.gain = nullptr; pk.out = nullptr;                              // the measuring form of the four kernels
            loudness_launches(c, pk, nullptr);
            q.rowk = w.rowk;
            if (!last && normalizing) MT2_HIP(launch_limiter_step(q, kLimStepNext, c.s));
            st.mark(kMeasureMark[k]);
        }
    }
    if (stats) {
        q.stats = stats;
        MT2_HIP(launch_limiter_step(q, kLimStepStats, c.s));
    }
    st.finish();
}

// The lengths of a DTW call, checked before anything else (host only)
static void dtw_check_geometry(int Tx_max, int Ty_max, int D, int B) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(D >= 1, "D < 1");
    MT2_REQUIRE(Tx_max >= 1 && Tx_max <= MT2_DTW_MAX_LEN, "Tx_max outside [1, MT2_DTW_MAX_LEN]");
    MT2_REQUIRE(Ty_max >= 1 && Ty_max <= MT2_DTW_MAX_LEN, "Ty_max outside [1, MT2_DTW_MAX_LEN]");
}
static void dtw_check_lens(const int* x_lens, int Tx_max, const int* y_lens, int Ty_max, int B) {
    MT2_REQUIRE(x_lens != nullptr && y_lens != nullptr, "x_lens / y_lens is NULL");
    check_lens(x_lens, B, Tx_max, "x length outside [1, Tx_max]");
    check_lens(y_lens, B, Ty_max, "y length outside [1, Ty_max]");
}
// the arena of one dtw_run, in carve order: the plan (both lengths), the costs in the skewed layout (strips of 64 rows), the packed
// directions
struct DtwWs { float* skew; unsigned* dirs; };
template <class Ws> static DtwWs dtw_carve(Ws& ws, IntPlan& ip, size_t Tx_max, int Ty_max, size_t B) {
    DtwWs w{};
    ip.carve(ws);
    w.skew = ws.template get<float>(B * ((Tx_max + 63) / 64) * dtw_skew_steps(Ty_max) * 64);
    w.dirs = ws.template get<unsigned>(B * Tx_max * dtw_dir_words(Ty_max));
    return w;
}
static long long dtw_arena_bytes(int Tx_max, int Ty_max, int B) {
    IntPlan ip;
    ip.add_fill(2 * (size_t)B + 8, 0);      // the documented figure ("at most"): room for both lengths and the gap between them
    ArenaCount count;
    dtw_carve(count, ip, Tx_max, Ty_max, B);
    return (long long)count.bytes;
}

// the three kernels of the DTW rule on p, each under its mark (dtw_run; mcd_run on the cepstra)
static void dtw_launches(const Ctx& c, const DtwP& p, Stages& st) {
    MT2_HIP(launch_dtw_cost(p, c.s));
    st.mark("dtw_cost");
    MT2_HIP(launch_dtw_accumulate(p, c.s));
    st.mark("dtw_accumulate");
    MT2_HIP(launch_dtw_backtrack(p, c.s));
    st.mark("dtw_backtrack");
}

// DTW of X onto Y by the rule of dtw.hip: cost -> accumulate -> backtrack on the caller's stream, nothing else
static void dtw_run(const Ctx& c, const float* X, const int* x_lens, int Tx_max, const float* Y, const int* y_lens, int Ty_max, int D,
                    int B, int* lo, int* hi, int* steps, float* total, float* cost, float* acc) {
    MT2_REQUIRE(X != nullptr && Y != nullptr && lo != nullptr && hi != nullptr && steps != nullptr && total != nullptr, "bad buffers");
    DtwP p{};
    p.X = X; p.Tx_max = Tx_max; p.Y = Y; p.Ty_max = Ty_max; p.D = D; p.B = B;
    p.max_tx = *std::max_element(x_lens, x_lens + B); p.max_ty = *std::max_element(y_lens, y_lens + B);
    IntPlan ip;
    const int o_x = ip.add(x_lens, B), o_y = ip.add(y_lens, B);
    const DtwWs w = dtw_carve(c.ws, ip, Tx_max, Ty_max, B);
    ip.send(c.m.pinned(), c.s);
    p.x_len = ip.dev(o_x); p.y_len = ip.dev(o_y);
    p.cost = cost;
    p.S_max = (Tx_max + 63) / 64; p.TS = (int)dtw_skew_steps(Ty_max); p.skew = w.skew;
    p.DW = (int)dtw_dir_words(Ty_max); p.dirs = w.dirs;
    p.acc = acc; p.lo = lo; p.hi = hi; p.steps = steps; p.total = total;
    Stages st(c.m, c.s);
    st.mark("start");
    dtw_launches(c, p, st);
    st.finish();
}

// phone durations of the real utterance from the path's hi[] and the synthetic durations (dtw.hip, "durations"); the x-length is
// read from the path itself (hi[Ty_b - 1] + 1) in the call's one copy to the host
static void align_durations_run(const Ctx& c, const int* hi, const int* y_lens, int Ty_max, const int* syn_dur, const int* phone_lens,
                                int Np_max, int B, int* dur_out_host) {
    std::vector<int> cum((size_t)B * (Np_max + 1), 0);
    for (int b = 0; b < B; ++b) {
        long long sum = 0;
        for (int q = 0; q < Np_max; ++q) {
            if (q < phone_lens[b]) {
                MT2_REQUIRE(syn_dur[(size_t)b * Np_max + q] >= 0, "negative synthetic duration");
                sum += syn_dur[(size_t)b * Np_max + q];
                MT2_REQUIRE(sum <= MT2_DTW_MAX_LEN, "synthetic durations sum beyond MT2_DTW_MAX_LEN");
            }
            cum[(size_t)b * (Np_max + 1) + q + 1] = (int)sum;
        }
        MT2_REQUIRE(sum >= 1, "synthetic durations sum to 0");
    }
    IntPlan ip;
    const int o_y = ip.add(y_lens, B), o_n = ip.add(phone_lens, B);
    const int o_cum = ip.add(cum);
    ip.upload(c.ws, c.m.pinned(), c.s);
    AlignDurP p{};
    p.hi = hi; p.Ty_max = Ty_max; p.y_len = ip.dev(o_y); p.cum = ip.dev(o_cum); p.np_len = ip.dev(o_n); p.Np_max = Np_max; p.B = B;
    const size_t n = (size_t)B * Np_max + B;
    p.dur = c.ws.get<int>(n); p.last = p.dur + (size_t)B * Np_max;
    MT2_HIP(launch_dtw_durations(p, c.s));
    int* st = static_cast<int*>(c.m.pinned().alloc(sizeof(int) * n));      // handle-owned staging
    MT2_HIP(hipMemcpyAsync(st, p.dur, sizeof(int) * n, hipMemcpyDeviceToHost, c.s));
    MT2_HIP(hipStreamSynchronize(c.s));
    for (int b = 0; b < B; ++b) {
        const int last = st[(size_t)B * Np_max + b], tx = cum[(size_t)b * (Np_max + 1) + Np_max];
        long long sum = 0;
        for (int q = 0; q < Np_max; ++q) sum += st[(size_t)b * Np_max + q];
        MT2_REQUIRE(last >= 0 && last < MT2_DTW_MAX_LEN && sum == y_lens[b], "hi does not cover the y length");
        MT2_REQUIRE(tx == last + 1, "synthetic durations do not sum to the x length of the path (hi[Ty - 1] + 1)");
    }
    std::copy(st, st + (size_t)B * Np_max, dur_out_host);
}

// ---- mel-cepstral distortion along the DTW path (mcd.hip): every refusal is decided here, on the host, before the first HIP call
static void mcd_check_order(int n_mels, int order, int B) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(mcd_geometry_ok(n_mels, order), "n_mels outside [2, 128] or order outside [1, min(n_mels - 1, MT2_MCD_MAX_ORDER)]");
}
static void mcd_check_max(int T_max, const char* msg) { MT2_REQUIRE(T_max >= 1 && T_max <= MT2_DTW_MAX_LEN, msg); }
static void mel_cepstrum_check(const float* mel, const int* frame_lens, int T_max, int B, int n_mels, int order, const float* cep) {
    mcd_check_order(n_mels, order, B);
    mcd_check_max(T_max, "T_max outside [1, MT2_DTW_MAX_LEN]");
    MT2_REQUIRE(mel != nullptr && frame_lens != nullptr && cep != nullptr, "bad buffers");
    MT2_REQUIRE((((uintptr_t)mel | (uintptr_t)cep) & 3) == 0, "misaligned buffers");
    check_lens(frame_lens, B, T_max, "frame count outside [1, T_max]");
    const size_t nt = sizeof(float) * (size_t)B * T_max;
    MT2_REQUIRE(!outputs_overlap({{cep, nt * order}}, {{mel, nt * n_mels}}), "overlapping buffers");
}
// the path reduction's arguments: the cepstra of width `order` (or, in the whole chain, the mels of width n_mels: `width`)
static void mcd_check_pair(const float* a, const int* a_lens, int Ta_max, const float* b, const int* b_lens, int Tb_max, int width, int B,
                           const int* lo, const int* hi, bool lo_hi_out, const float* f0_a, const float* f0_b, const double* out) {
    mcd_check_max(Ta_max, "Ta_max outside [1, MT2_DTW_MAX_LEN]");
    mcd_check_max(Tb_max, "Tb_max outside [1, MT2_DTW_MAX_LEN]");
    MT2_REQUIRE(a != nullptr && b != nullptr && a_lens != nullptr && b_lens != nullptr && out != nullptr, "bad buffers");
    MT2_REQUIRE((f0_a == nullptr) == (f0_b == nullptr), "one F0 track given without the other");
    MT2_REQUIRE((((uintptr_t)a | (uintptr_t)b | (uintptr_t)lo | (uintptr_t)hi | (uintptr_t)f0_a | (uintptr_t)f0_b) & 3) == 0 &&
                    ((uintptr_t)out & 7) == 0, "misaligned buffers");
    check_lens(a_lens, B, Ta_max, "a length outside [1, Ta_max]");
    check_lens(b_lens, B, Tb_max, "b length outside [1, Tb_max]");
    const size_t na = sizeof(float) * (size_t)B * Ta_max, nb = sizeof(float) * (size_t)B * Tb_max, no = sizeof(double) * MT2_MCD_FIELDS * (size_t)B;
    if (lo_hi_out)
        MT2_REQUIRE(!outputs_overlap({{out, no}, {lo, nb}, {hi, nb}}, {{a, na * width}, {b, nb * width}, {f0_a, na}, {f0_b, nb}}), "overlapping buffers");
    else
        MT2_REQUIRE(!outputs_overlap({{out, no}}, {{a, na * width}, {b, nb * width}, {lo, nb}, {hi, nb}, {f0_a, na}, {f0_b, nb}}), "overlapping buffers");
}
static const float* mcd_prepare(mt2_model& m, int n_mels, int order) {
    float*& d = m.mcd_tables[{n_mels, order}];
    if (d) return d;
    std::vector<float> h((size_t)n_mels * order);
    mcd_table(n_mels, order, h.data());
    float* t = nullptr;
    MT2_HIP(hipMalloc(reinterpret_cast<void**>(&t), h.size() * sizeof(float)));
    m.dev_allocs.push_back(t);
    MT2_HIP(hipMemcpy(t, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice));
    return d = t;
}
static void mcd_cepstrum_launch(const Ctx& c, const float* table, const float* mel, const int* len_dev, int T_max, int B, int n_mels, int order,
                                float* cep) {
    McdCepP p{};
    p.mel = mel; p.T_max = T_max; p.N = n_mels; p.K = order; p.B = B; p.len = len_dev; p.table = table; p.cep = cep;
    MT2_HIP(launch_mcd_cepstrum(p, c.s));
}
static void mel_cepstrum_run(const Ctx& c, const float* mel, const int* frame_lens, int T_max, int B, int n_mels, int order, float* cep) {
    const float* table = mcd_prepare(c.m, n_mels, order);
    IntPlan ip;
    const int o_t = ip.add(frame_lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    mcd_cepstrum_launch(c, table, mel, ip.dev(o_t), T_max, B, n_mels, order, cep);
}
static void mcd_path_launch(const Ctx& c, const float* ca, const int* a_dev, int Ta_max, const float* cb, const int* b_dev, int Tb_max, int order,
                            int B, const int* lo, const int* hi, const float* f0_a, const float* f0_b, double* out) {
    McdPathP p{};
    p.ca = ca; p.Ta_max = Ta_max; p.cb = cb; p.Tb_max = Tb_max; p.K = order; p.B = B; p.a_len = a_dev; p.b_len = b_dev;
    p.lo = lo; p.hi = hi; p.f0_a = f0_a; p.f0_b = f0_b; p.out = out;
    MT2_HIP(launch_mcd_path(p, c.s));
}
static void path_distortion_run(const Ctx& c, const float* ca, const int* a_lens, int Ta_max, const float* cb, const int* b_lens, int Tb_max,
                                int order, int B, const int* lo, const int* hi, const float* f0_a, const float* f0_b, double* out) {
    IntPlan ip;
    const int o_a = ip.add(a_lens, B), o_b = ip.add(b_lens, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    mcd_path_launch(c, ca, ip.dev(o_a), Ta_max, cb, ip.dev(o_b), Tb_max, order, B, lo, hi, f0_a, f0_b, out);
}
// the arena of one mcd_run, in carve order: what a DTW of this geometry takes (the plan with both lengths, the skewed costs, the packed
// directions), the two cepstra, the path (lo | hi) and the DTW's steps and total - taken whether or not the caller asks for lo / hi
struct McdWs { DtwWs dtw; float *ca, *cb; int *lo, *hi, *steps; float* total; };
template <class Ws> static McdWs mcd_carve(Ws& ws, IntPlan& ip, size_t Ta_max, int Tb_max, size_t order, size_t B) {
    McdWs w{};
    w.dtw = dtw_carve(ws, ip, Ta_max, Tb_max, B);
    w.ca = ws.template get<float>(B * Ta_max * order);
    w.cb = ws.template get<float>(B * Tb_max * order);
    w.lo = ws.template get<int>(B * Tb_max);
    w.hi = ws.template get<int>(B * Tb_max);
    w.steps = ws.template get<int>(B);
    w.total = ws.template get<float>(B);
    return w;
}
static long long mcd_arena_bytes(int Ta_max, int Tb_max, int order, int B) {
    IntPlan ip;
    ip.add_fill(B, 0);
    ip.add_fill(B, 0);
    ArenaCount count;
    mcd_carve(count, ip, Ta_max, Tb_max, order, B);
    return (long long)count.bytes;
}
// the whole chain on the arena: two cepstra, the DTW of dtw.hip on them, the path reduction.  Enqueues only.
static void mcd_run(const Ctx& c, const float* mel_a, const int* a_lens, int Ta_max, const float* mel_b, const int* b_lens, int Tb_max,
                    int n_mels, int order, int B, const float* f0_a, const float* f0_b, double* out, int* lo, int* hi) {
    const float* table = mcd_prepare(c.m, n_mels, order);
    IntPlan ip;
    const int o_a = ip.add(a_lens, B), o_b = ip.add(b_lens, B);
    const McdWs w = mcd_carve(c.ws, ip, Ta_max, Tb_max, order, B);
    ip.send(c.m.pinned(), c.s);
    Stages st(c.m, c.s);
    st.mark("start");
    mcd_cepstrum_launch(c, table, mel_a, ip.dev(o_a), Ta_max, B, n_mels, order, w.ca);
    mcd_cepstrum_launch(c, table, mel_b, ip.dev(o_b), Tb_max, B, n_mels, order, w.cb);
    st.mark("mcd_cepstrum");
    DtwP p{};
    p.X = w.ca; p.Tx_max = Ta_max; p.Y = w.cb; p.Ty_max = Tb_max; p.D = order; p.B = B;
    p.max_tx = *std::max_element(a_lens, a_lens + B); p.max_ty = *std::max_element(b_lens, b_lens + B);
    p.x_len = ip.dev(o_a); p.y_len = ip.dev(o_b);
    p.S_max = (Ta_max + 63) / 64; p.TS = (int)dtw_skew_steps(Tb_max); p.skew = w.dtw.skew;
    p.DW = (int)dtw_dir_words(Tb_max); p.dirs = w.dtw.dirs;
    p.lo = w.lo; p.hi = w.hi; p.steps = w.steps; p.total = w.total;
    dtw_launches(c, p, st);
    mcd_path_launch(c, w.ca, ip.dev(o_a), Ta_max, w.cb, ip.dev(o_b), Tb_max, order, B, w.lo, w.hi, f0_a, f0_b, out);
    if (lo) MT2_HIP(hipMemcpyAsync(lo, w.lo, sizeof(int) * (size_t)B * Tb_max, hipMemcpyDeviceToDevice, c.s));
    if (hi) MT2_HIP(hipMemcpyAsync(hi, w.hi, sizeof(int) * (size_t)B * Tb_max, hipMemcpyDeviceToDevice, c.s));
    st.mark("mcd_path");
    st.finish();
}

// ---- stationary-noise suppression (denoise.hip) between the STFT of the front-end and the inverse STFT of griffinlim.hip: every
// refusal is decided here, on the host, before the first HIP call
struct DnArgs { int percentile, bf, bt; float beta, gmin, c; };
static DnArgs denoise_check_config(const mt2_denoise_config* dc) {
    MT2_REQUIRE(dc != nullptr, "null denoise configuration");
    MT2_REQUIRE(dc->percentile >= 1 && dc->percentile <= 99, "percentile outside [1, 99]");
    MT2_REQUIRE(std::isfinite(dc->over_subtraction) && dc->over_subtraction > 0.0f, "over_subtraction must be finite and > 0");
    MT2_REQUIRE(std::isfinite(dc->floor_gain) && dc->floor_gain > 0.0f && dc->floor_gain <= 1.0f, "floor_gain outside (0, 1]");
    MT2_REQUIRE(dc->smooth_bins >= 0 && dc->smooth_bins <= kDnMaxSmooth, "smooth_bins outside [0, 8]");
    MT2_REQUIRE(dc->smooth_frames >= 0 && dc->smooth_frames <= kDnMaxSmooth, "smooth_frames outside [0, 8]");
    MT2_REQUIRE(dc->reserved == 0, "mt2_denoise_config.reserved must be 0");
    return {dc->percentile, dc->smooth_bins, dc->smooth_frames, dc->over_subtraction, dc->floor_gain, denoise_factor(dc->percentile)};
}
static void denoise_fill(DenoiseP& p, const DnArgs& a, const SpecGeom& g, int B, int T_cap) {
    p.F = g.F; p.Fp = g.Fp; p.lds = g.lds; p.B = B; p.T_cap = T_cap;
    p.percentile = a.percentile; p.bf = a.bf; p.bt = a.bt; p.beta = a.beta; p.gmin = a.gmin; p.c = a.c;
}
static size_t denoise_tiles(int T_cap, int F) { return (size_t)((T_cap + kDnTileT - 1) / kDnTileT) * ((F + kDnTileF - 1) / kDnTileF); }

// ---- the round trip of mt2_denoise and mt2_dereverb: waveforms -> STFT -> the call's own work on the packed spectrum -> inverse STFT
// the frame counts of a waveform batch, T_b = 1 + L_b / hop, each inside what the inverse STFT accepts; -> their max
static int wave_frames(const mt2_audio_config& ac, const int* lens, int L_max, int B, std::vector<int>& T) {
    gl_check_config(ac);
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(L_max >= 1, "L_max < 1");
    T.resize(B);
    int T_cap = 0;
    for (int b = 0; b < B; ++b) {
        const int L = lens ? lens[b] : L_max;
        MT2_REQUIRE(L >= 1 && L <= L_max, "waveform length outside [1, L_max]");
        T[b] = 1 + L / ac.hop_length;
        MT2_REQUIRE(T[b] >= gl_min_frames(ac), "a waveform shorter than (n_fft / (2 hop) + 1) hop samples: fewer frames than mt2_istft accepts");
        T_cap = std::max(T_cap, T[b]);
    }
    MT2_REQUIRE(T_cap <= MT2_DENOISE_MAX_FRAMES, "more than MT2_DENOISE_MAX_FRAMES frames");
    gl_check_lens(ac, T.data(), T_cap, B, (long long)(T_cap - 1) * ac.hop_length);
    return T_cap;
}
// what both calls refuse about their waveform batch, after their own configuration; a call without floors passes NULL for them, and
// `fields` doubles an utterance of figures.  -> T_cap, with T filled
static int wave_check(const mt2_audio_config& ac, const float* wav, const int* lens, int L_max, int B, const float* floor_in, const float* floor_out,
                      const double* figures, int fields, const float* out, int Lout_max, std::vector<int>& T) {
    MT2_REQUIRE(wav != nullptr && lens != nullptr && out != nullptr, "bad buffers");
    const int T_cap = wave_frames(ac, lens, L_max, B, T);
    MT2_REQUIRE((long long)Lout_max >= (long long)(T_cap - 1) * ac.hop_length, "Lout_max smaller than (max T - 1) * hop_length");
    MT2_REQUIRE((((uintptr_t)wav | (uintptr_t)out | (uintptr_t)floor_in | (uintptr_t)floor_out) & 3) == 0 && ((uintptr_t)figures & 7) == 0,
                "misaligned buffers");
    const size_t nw = sizeof(float) * (size_t)B * L_max, no = sizeof(float) * (size_t)B * Lout_max,
                 nf = sizeof(float) * (size_t)B * SpecGeom(ac).Fp, ng = sizeof(double) * fields * (size_t)B;
    MT2_REQUIRE(!outputs_overlap({{out, no}, {floor_out, nf}, {figures, ng}}, {{wav, nw}, {floor_in, nf}}), "overlapping buffers");
    return T_cap;
}
// The arena of a round trip, in carve order: the plan, the reflect-padded blocks, the packed spectrum (worked on in place), the call's
// own buffers, the frames of the inverse STFT - taken whatever the optional arguments.  trip_plan adds the plan entries both calls have
// (lens NULL, as in a query: zeros), the call adds its own behind them, and trip_carve places the plan and the buffers - over the arena
// in the run and over an ArenaCount in the query, so the two cannot disagree
struct Trip {
    FrameRows r;
    int o_b, o_t, o_len, o_base, o_map, o_row0, o_T;
    float *xp, *spec, *frames;
};
static Trip trip_plan(IntPlan& ip, const SpecGeom& g, const int* lens, const std::vector<int>& T, int T_cap) {
    Trip t{};
    const int B = (int)T.size();
    t.r = frame_rows(g, T.data(), B, T_cap);
    t.o_b = ip.add(t.r.blk_b); t.o_t = ip.add(t.r.blk_t); t.o_len = lens ? ip.add(lens, B) : ip.add_fill(B, 0);
    t.o_base = ip.add(t.r.rowbase); t.o_map = ip.add(t.r.map); t.o_row0 = ip.add(t.r.row0); t.o_T = ip.add(T);
    return t;
}
template <class Ws, class Own> static void trip_carve(Ws& ws, IntPlan& ip, const SpecGeom& g, Trip& t, Own own) {
    ip.carve(ws);
    t.xp = ws.template get<float>((size_t)t.r.Rb * g.hop);
    t.spec = ws.template get<float>((size_t)t.r.Fr * g.lds);
    own();
    t.frames = ws.template get<float>((size_t)t.r.Fr * g.N);
}
// enqueues only; `mid` works on t.spec in place and sets its own stage marks.  The STFT GEMM runs per utterance, on the tile its own row
// count chooses - what mt2_stft runs for the utterance alone; the inverse GEMM runs once on the fixed tile of mt2_istft.
template <class Mid> static void trip_run(const Ctx& c, const SpecGeom& g, IntPlan& ip, const Trip& t, const std::vector<int>& T, const float* wav,
                                          int L_max, float* out, int Lout_max, const std::string& prefix, Mid mid) {
    const int B = (int)T.size();
    ip.send(c.m.pinned(), c.s);
    Stages st(c.m, c.s);
    st.mark("start");
    MT2_HIP(launch_reflect_pad_blocks(wav, L_max, ip.dev(t.o_b), ip.dev(t.o_t), ip.dev(t.o_len), g.hop, g.pad, t.xp, t.r.Rb, c.s));
    MT2_HIP(hipMemsetAsync(t.spec, 0, sizeof(float) * (size_t)t.r.Fr * g.lds, c.s));      // the pad columns meet zero basis columns
    for (int b = 0; b < B; ++b)
        stft_gemm(c, g, t.xp, t.r.Rb, ip.dev(t.o_base) + t.r.row0[b], t.spec + (size_t)t.r.row0[b] * g.lds, T[b]);
    st.mark((prefix + "stft").c_str());
    mid(st);
    istft_rows_to_wav(c, g, t.spec, t.frames, t.r.Fr, ip.dev(t.o_row0), ip.dev(t.o_T), out, Lout_max, B);
    st.mark((prefix + "istft").c_str());
    st.finish();
}

// the buffers of denoise's own between the spectrum and the frames: P, the floor, the tile sums
struct DnWs { Trip t; float *P, *floor; double* part; };
template <class Ws> static DnWs denoise_layout(Ws& ws, IntPlan& ip, const SpecGeom& g, const int* lens, const std::vector<int>& T, int T_cap) {
    DnWs w{};
    w.t = trip_plan(ip, g, lens, T, T_cap);
    trip_carve(ws, ip, g, w.t, [&] {
        w.P = ws.template get<float>((size_t)w.t.r.Fr * g.Fp);
        w.floor = ws.template get<float>(T.size() * g.Fp);
        w.part = ws.template get<double>(T.size() * denoise_tiles(T_cap, g.F) * 3);
    });
    return w;
}
static void denoise_run(const Ctx& c, const mt2_audio_config& ac, const DnArgs& a, const float* wav, const int* lens, int L_max, int B,
                        const std::vector<int>& T, int T_cap, const float* floor_in, float* floor_out, double* figures, float* out,
                        int Lout_max) {
    gl_prepare_istft(c.m, ac);
    const SpecGeom g(ac);
    IntPlan ip;
    const DnWs w = denoise_layout(c.ws, ip, g, lens, T, T_cap);
    DenoiseP p{};
    denoise_fill(p, a, g, B, T_cap);
    p.spec = w.t.spec; p.spec_out = w.t.spec; p.row0 = ip.dev(w.t.o_row0); p.T = ip.dev(w.t.o_T); p.P = w.P; p.floor_out = w.floor;
    p.floor = floor_in ? floor_in : w.floor;
    if (figures) { p.part = w.part; p.fig = figures; }
    trip_run(c, g, ip, w.t, T, wav, L_max, out, Lout_max, "dn_", [&](Stages& st) {
        MT2_HIP(launch_denoise_power(p, c.s));
        if (!floor_in) MT2_HIP(launch_denoise_select(p, c.s));
        if (floor_out) MT2_HIP(hipMemcpyAsync(floor_out, p.floor, sizeof(float) * (size_t)B * p.Fp, hipMemcpyDeviceToDevice, c.s));
        st.mark("dn_floor");
        MT2_HIP(launch_denoise_gain(p, c.s));
        if (figures) MT2_HIP(launch_denoise_figures(p, c.s));
        st.mark("dn_gain");
    });
}

// the spectrum batch of mt2_noise_floor and mt2_spectral_gain: utterance b owns the rows b T_max .. + frame_lens[b];  -> max frame count
static int denoise_check_spec(const mt2_audio_config* ac, const float* spec, const int* frame_lens, int T_max, int B) {
    MT2_REQUIRE(ac != nullptr, "null audio configuration");
    frontend_check(*ac);
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(T_max >= 1 && T_max <= MT2_DENOISE_MAX_FRAMES, "T_max outside [1, MT2_DENOISE_MAX_FRAMES]");
    MT2_REQUIRE(spec != nullptr && frame_lens != nullptr && ((uintptr_t)spec & 3) == 0, "bad buffers");
    MT2_REQUIRE((long long)B * T_max * (ac->n_fft + 4) <= INT_MAX, "batch too large for 32-bit row indices");
    return check_lens(frame_lens, B, T_max, "a frame count outside [1, T_max]");
}
// the first two plan entries of every call on a caller's spectrum batch [B, T_max, lds]: row0[b] = b T_max, then the frame counts
struct SpecBatch { int o_row0, o_T; };
static SpecBatch spec_batch_plan(IntPlan& ip, const int* frame_lens, int T_max, int B) {
    std::vector<int> row0(B);
    for (int b = 0; b < B; ++b) row0[b] = b * T_max;
    const int o_row0 = ip.add(row0);
    return {o_row0, ip.add(frame_lens, B)};
}
// the plan and P of both calls (their whole arena: the plan of 2 B words, then 4 B T_max Fp bytes), and the power kernel
static DenoiseP denoise_spec_setup(const Ctx& c, const mt2_audio_config& ac, const DnArgs& a, const float* spec, const int* frame_lens,
                                   int T_max, int B, int T_cap) {
    IntPlan ip;
    const SpecBatch sb = spec_batch_plan(ip, frame_lens, T_max, B);
    ip.upload(c.ws, c.m.pinned(), c.s);
    DenoiseP p{};
    denoise_fill(p, a, SpecGeom(ac), B, T_cap);
    p.spec = spec; p.row0 = ip.dev(sb.o_row0); p.T = ip.dev(sb.o_T);
    p.P = c.ws.get<float>((size_t)B * T_max * p.Fp);
    MT2_HIP(launch_denoise_power(p, c.s));
    return p;
}
static void noise_floor_run(const Ctx& c, const mt2_audio_config& ac, const DnArgs& a, const float* spec, const int* frame_lens, int T_max,
                            int B, int T_cap, float* floor) {
    DenoiseP p = denoise_spec_setup(c, ac, a, spec, frame_lens, T_max, B, T_cap);
    p.floor_out = floor;
    MT2_HIP(launch_denoise_select(p, c.s));
}
static void spectral_gain_run(const Ctx& c, const mt2_audio_config& ac, const DnArgs& a, const float* spec, const int* frame_lens, int T_max,
                              int B, int T_cap, const float* floor, float* gain, float* spec_out) {
    DenoiseP p = denoise_spec_setup(c, ac, a, spec, frame_lens, T_max, B, T_cap);
    p.floor = floor; p.gain_out = gain; p.gain_T = T_max; p.spec_out = spec_out;
    if (gain) MT2_HIP(hipMemsetAsync(gain, 0, sizeof(float) * (size_t)B * T_max * p.Fp, c.s));
    if (spec_out && spec_out != spec) MT2_HIP(hipMemsetAsync(spec_out, 0, sizeof(float) * (size_t)B * T_max * p.lds, c.s));
    MT2_HIP(launch_denoise_gain(p, c.s));
}

// ---- de-reverberation by weighted prediction error (wpe.hip) between the same two transforms: every refusal is decided here, on the
// host, before the first HIP call
struct WpeArgs { int delay, taps, iters, ctx; double eps, load; };
static WpeArgs wpe_check_config(const mt2_wpe_config* wc) {
    MT2_REQUIRE(wc != nullptr, "null dereverberation configuration");
    MT2_REQUIRE(wc->delay >= 1 && wc->delay <= 8, "delay outside [1, 8]");
    MT2_REQUIRE(wc->taps >= 1 && wc->taps <= kWpeMaxTaps, "taps outside [1, 16]");
    MT2_REQUIRE(wc->iterations >= 1 && wc->iterations <= 8, "iterations outside [1, 8]");
    MT2_REQUIRE(wc->context >= 0 && wc->context <= 4, "context outside [0, 4]");
    MT2_REQUIRE(std::isfinite(wc->variance_floor) && wc->variance_floor > 0.0 && wc->variance_floor <= 1.0, "variance_floor outside (0, 1]");
    MT2_REQUIRE(std::isfinite(wc->loading) && wc->loading >= 0.0 && wc->loading <= 1e-2, "loading outside [0, 1e-2]");
    MT2_REQUIRE(wc->reserved == 0, "mt2_wpe_config.reserved must be 0");
    return {wc->delay, wc->taps, wc->iterations, wc->context, wc->variance_floor, wc->loading};
}
// the bin-major columns of a batch: utterance b starts at c0[b] (in complex cells) and holds F columns of T_b rounded up to 4; -> cells
static size_t wpe_columns(const std::vector<int>& T, int F, std::vector<int>& c0) {
    size_t at = 0;
    c0.resize(T.size());
    for (size_t b = 0; b < T.size(); ++b) {
        MT2_REQUIRE(at <= (size_t)INT_MAX, "batch too large for 32-bit column indices");
        c0[b] = (int)at;
        at += (size_t)F * ((T[b] + 3) & ~3);
    }
    MT2_REQUIRE(at <= (size_t)INT_MAX, "batch too large for 32-bit column indices");
    return at;
}
static void wpe_fill(WpeP& p, const WpeArgs& a, const SpecGeom& g, int B, int T_cap) {
    p.F = g.F; p.Fp = g.Fp; p.lds = g.lds; p.B = B; p.T_cap = T_cap;
    p.delay = a.delay; p.taps = a.taps; p.iters = a.iters; p.ctx = a.ctx; p.eps = a.eps; p.load = a.load;
}
// transposition, the bins, the way back and the figures: the four launches of both calls
static void wpe_launches(const Ctx& c, WpeP& p, double* filters, double* figures) {
    p.filters = filters; p.fig = figures;
    if (filters) MT2_HIP(hipMemsetAsync(filters, 0, sizeof(double) * 2 * (size_t)p.B * p.Fp * p.taps, c.s));      // the rows F .. Fp-1
    MT2_HIP(launch_wpe_to_bins(p, c.s));
    MT2_HIP(launch_wpe_bins(p, c.s));
    MT2_HIP(launch_wpe_from_bins(p, c.s));
    if (figures) MT2_HIP(launch_wpe_figures(p, c.s));
}
// the plan entries of dereverb's own behind the round trip's (c0, run) and its buffers between the spectrum and the frames: the columns
// of Y and of D, the bins' sums.  An utterance of fewer than delay + 4 taps frames is not filtered: its bins pass through.
struct WpeWs { Trip t; int o_c0, o_run; float2 *cols, *cols_out; double* stat; };
template <class Ws> static WpeWs dereverb_layout(Ws& ws, IntPlan& ip, const SpecGeom& g, const WpeArgs& a, const int* lens, const std::vector<int>& T,
                                                 int T_cap) {
    WpeWs w{};
    w.t = trip_plan(ip, g, lens, T, T_cap);
    std::vector<int> run(T.size()), c0;
    for (size_t b = 0; b < T.size(); ++b) run[b] = T[b] >= a.delay + 4 * a.taps;
    const size_t cells = wpe_columns(T, g.F, c0);
    w.o_c0 = ip.add(c0); w.o_run = ip.add(run);
    trip_carve(ws, ip, g, w.t, [&] {
        w.cols = reinterpret_cast<float2*>(ws.template get<float>(2 * cells));
        w.cols_out = reinterpret_cast<float2*>(ws.template get<float>(2 * cells));
        w.stat = ws.template get<double>(T.size() * g.F * kWpeStat);
    });
    return w;
}
static void dereverb_run(const Ctx& c, const mt2_audio_config& ac, const WpeArgs& a, const float* wav, const int* lens, int L_max, int B,
                         const std::vector<int>& T, int T_cap, double* figures, float* out, int Lout_max) {
    gl_prepare_istft(c.m, ac);
    const SpecGeom g(ac);
    IntPlan ip;
    const WpeWs w = dereverb_layout(c.ws, ip, g, a, lens, T, T_cap);
    WpeP p{};
    wpe_fill(p, a, g, B, T_cap);
    p.spec = w.t.spec; p.spec_out = w.t.spec; p.row0 = ip.dev(w.t.o_row0); p.T = ip.dev(w.t.o_T); p.c0 = ip.dev(w.o_c0); p.run = ip.dev(w.o_run);
    p.cols = w.cols; p.cols_out = w.cols_out; p.stat = w.stat;
    trip_run(c, g, ip, w.t, T, wav, L_max, out, Lout_max, "dr_", [&](Stages& st) {
        wpe_launches(c, p, nullptr, figures);
        st.mark("dr_wpe");
    });
}
// steps 1-3 on a caller's spectrum batch: utterance b owns the rows b T_max .. + frame_lens[b].  Its arena: the plan of 4 B words, the
// columns of Y and of D, the bins' sums
static void wpe_spectrum_run(const Ctx& c, const mt2_audio_config& ac, const WpeArgs& a, const float* spec, const int* frame_lens, int T_max,
                             int B, int T_cap, float* spec_out, double* filters, double* figures) {
    IntPlan ip;
    std::vector<int> run(B, 1), c0;
    const SpecBatch sb = spec_batch_plan(ip, frame_lens, T_max, B);
    const size_t cells = wpe_columns(std::vector<int>(frame_lens, frame_lens + B), SpecGeom(ac).F, c0);
    const int o_c0 = ip.add(c0), o_run = ip.add(run);
    ip.upload(c.ws, c.m.pinned(), c.s);
    WpeP p{};
    wpe_fill(p, a, SpecGeom(ac), B, T_cap);
    p.spec = spec; p.spec_out = spec_out; p.row0 = ip.dev(sb.o_row0); p.T = ip.dev(sb.o_T); p.c0 = ip.dev(o_c0); p.run = ip.dev(o_run);
    p.cols = reinterpret_cast<float2*>(c.ws.get<float>(2 * cells));
    p.cols_out = reinterpret_cast<float2*>(c.ws.get<float>(2 * cells));
    p.stat = c.ws.get<double>((size_t)B * p.F * kWpeStat);
    if (spec_out != spec) MT2_HIP(hipMemsetAsync(spec_out, 0, sizeof(float) * (size_t)B * T_max * p.lds, c.s));
    wpe_launches(c, p, filters, figures);
}

// ---- declipping by sparsity (declip.hip), at the audio's own sample rate: every refusal is decided here, on the host, before the
// first HIP call
struct DcArgs { int N, min_count, step, every, max_iter; float tol, level; double min_share, eps; };
static DcArgs declip_check_config(const mt2_declip_config* dc) {
    MT2_REQUIRE(dc != nullptr, "null declipping configuration");
    const int N = dc->frame;
    MT2_REQUIRE(N == 256 || N == 512 || N == 1024 || N == 2048, "frame not one of 256, 512, 1024, 2048");
    MT2_REQUIRE(std::isfinite(dc->tol) && dc->tol >= 0.0 && dc->tol <= 0.1, "tol outside [0, 0.1]");
    MT2_REQUIRE(std::isfinite(dc->min_share) && dc->min_share >= 0.0 && dc->min_share <= 1.0, "min_share outside [0, 1]");
    MT2_REQUIRE(dc->min_count >= 1, "min_count < 1");
    MT2_REQUIRE(std::isnan(dc->level) || (std::isfinite(dc->level) && dc->level > 0.0 && std::isfinite((float)dc->level) && (float)dc->level > 0.0f),
                "level neither NaN (detect) nor a positive finite f32 value");
    MT2_REQUIRE(dc->step >= 1 && dc->step <= N / 2 + 1, "step outside [1, frame / 2 + 1]");
    MT2_REQUIRE(dc->every >= 1 && dc->every <= 64, "every outside [1, 64]");
    MT2_REQUIRE(std::isfinite(dc->eps) && dc->eps > 0.0 && dc->eps < 1.0, "eps outside (0, 1)");
    MT2_REQUIRE(dc->max_iter >= 0, "max_iter < 0");
    MT2_REQUIRE(dc->reserved == 0, "mt2_declip_config.reserved must be 0");
    const int K = N / 2 + 1;
    return {N, dc->min_count, dc->step, dc->every, dc->max_iter > 0 ? dc->max_iter : dc->every * ((K + dc->step - 1) / dc->step),
            (float)dc->tol, std::isnan(dc->level) ? NAN : (float)dc->level, dc->min_share, dc->eps};
}
// the ragged lengths (lens NULL: every utterance L_max samples) -> the frames of each utterance; returns the longest length
static int declip_frames(const DcArgs& a, const int* lens, int L_max, int B, std::vector<int>& len, std::vector<int>& T) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(L_max >= 1, "L_max < 1");
    len.assign(B, L_max);
    if (lens) len.assign(lens, lens + B);
    const int mx = check_lens(len.data(), B, L_max, "waveform length outside [1, L_max]");
    const int hop = a.N / 4;
    T.resize(B);
    for (int b = 0; b < B; ++b) {
        const long long t = ((long long)len[b] + hop - 1) / hop + 3;
        MT2_REQUIRE(t <= MT2_DECLIP_MAX_FRAMES, "more than MT2_DECLIP_MAX_FRAMES frames in an utterance");
        T[b] = (int)t;
    }
    return mx;
}
// the arena of a call, in carve order: the plan, the detection words, then - for mt2_declip alone - the iteration counts and the frames
struct DcWs { int* det; int* it; double* frames; };
template <class Ws> static DcWs declip_carve(Ws& ws, IntPlan& ip, size_t B, size_t rows, size_t N, bool restore) {
    DcWs w{};
    ip.carve(ws);
    w.det = ws.template get<int>(B * kDcDet);
    if (restore) {
        w.it = ws.template get<int>(rows);
        w.frames = ws.template get<double>(rows * N);
    }
    return w;
}
static long long declip_arena_bytes(const DcArgs& a, const std::vector<int>& T, bool restore) {
    size_t rows = 0;
    for (int t : T) rows += t;
    IntPlan ip;      // the entries of declip_run's plan, by size: lengths, needs and - to restore - first rows
    for (int i = 0; i < (restore ? 3 : 2); ++i) ip.add_fill(T.size(), 0);
    ArenaCount count;
    declip_carve(count, ip, T.size(), rows, a.N, restore);
    return (long long)count.bytes;
}
static const double* declip_prepare(mt2_model& m, int N) {
    double*& d = m.dc_tables[N];
    if (d) return d;
    std::vector<double> h(dc_table_doubles(N));
    dc_table(N, h.data());
    double* t = nullptr;
    MT2_HIP(hipMalloc(reinterpret_cast<void**>(&t), h.size() * sizeof(double)));
    m.dev_allocs.push_back(t);
    MT2_HIP(hipMemcpy(t, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
    return d = t;
}
struct DcCall { DcArgs a; std::vector<int> len, T; int max_len, T_cap; };
// -> the checked call; out NULL: mt2_clip_detect
static DcCall declip_check(const mt2_declip_config* dc, const float* wav, const int* lens, int L_max, int B, const float* out, int Lout_max,
                           const double* figures, const int32_t* iters, int T_max, bool restore) {
    DcCall k{};
    k.a = declip_check_config(dc);
    MT2_REQUIRE(wav != nullptr && lens != nullptr, "bad buffers");
    k.max_len = declip_frames(k.a, lens, L_max, B, k.len, k.T);
    k.T_cap = *std::max_element(k.T.begin(), k.T.end());
    MT2_REQUIRE((((uintptr_t)wav | (uintptr_t)out | (uintptr_t)iters) & 3) == 0 && ((uintptr_t)figures & 7) == 0, "misaligned buffers");
    const size_t nw = sizeof(float) * (size_t)B * L_max, ng = sizeof(double) * MT2_DECLIP_FIELDS * (size_t)B;
    if (restore) {
        MT2_REQUIRE(out != nullptr, "null out");
        MT2_REQUIRE(Lout_max >= k.max_len, "Lout_max smaller than the longest utterance");
        MT2_REQUIRE(iters == nullptr || T_max >= k.T_cap, "T_max smaller than ceil(max length / hop) + 3");
        const size_t no = sizeof(float) * (size_t)B * Lout_max, ni = iters ? sizeof(int32_t) * (size_t)B * T_max : 0;
        MT2_REQUIRE(!outputs_overlap({{out, no}, {figures, ng}, {iters, ni}}, {{wav, nw}}), "overlapping buffers (in place is not offered)");
    } else {
        MT2_REQUIRE(figures != nullptr, "null figures");
        MT2_REQUIRE(!outputs_overlap({{figures, ng}}, {{wav, nw}}), "overlapping buffers");
    }
    return k;
}
// enqueues only (the table of a frame length is uploaded once per handle).  out NULL: detection and its figures alone
static void declip_run(const Ctx& c, const DcCall& k, const float* wav, int L_max, int B, float* out, int Lout_max, double* figures,
                       int32_t* iters, int T_max) {
    const bool restore = out != nullptr;
    const DcArgs& a = k.a;
    std::vector<int> need(B), row0(B);
    size_t rows = 0;
    for (int b = 0; b < B; ++b) {
        need[b] = (int)std::min<double>(std::max<double>(a.min_count, std::ceil(a.min_share * (double)k.len[b])), (double)INT_MAX);
        row0[b] = (int)rows;
        rows += k.T[b];
    }
    MT2_REQUIRE(rows <= (size_t)INT_MAX, "batch too large for 32-bit frame indices");
    IntPlan ip;
    const int o_len = ip.add(k.len), o_need = ip.add(need), o_row0 = restore ? ip.add(row0) : 0;
    const DcWs w = declip_carve(c.ws, ip, B, rows, a.N, restore);
    ip.send(c.m.pinned(), c.s);
    DeclipP p{};
    p.wav = wav; p.L_max = L_max; p.len = ip.dev(o_len); p.need = ip.dev(o_need); p.row0 = restore ? ip.dev(o_row0) : nullptr;
    p.B = B; p.T_cap = k.T_cap; p.N = a.N; p.tol = a.tol; p.level = a.level; p.step = a.step; p.every = a.every; p.max_iter = a.max_iter;
    p.eps = a.eps; p.det = w.det; p.frames = w.frames; p.it = w.it; p.iters_out = iters; p.T_max = T_max; p.out = out; p.Lout_max = Lout_max;
    p.fig = figures;
    if (restore) p.table = declip_prepare(c.m, a.N);
    Stages st(c.m, c.s);
    st.mark("start");
    MT2_HIP(launch_dc_detect(p, c.s));
    st.mark("dc_detect");
    if (restore) {
        if (iters) MT2_HIP(hipMemsetAsync(iters, 0, sizeof(int32_t) * (size_t)B * T_max, c.s));
        MT2_HIP(launch_dc_frames(p, c.s));
        st.mark("dc_frames");
        MT2_HIP(launch_dc_overlap(p, k.max_len, c.s));
        st.mark("dc_overlap");
    }
    if (figures) MT2_HIP(launch_dc_figures(p, c.s));
    st.mark("dc_figures");
    st.finish();
}

// ---- speech segments by frame energy and the cut of the pauses (segments.hip): every refusal is decided here, on the host, before the
// first HIP call
struct SgArgs { float factor; int min_pause, min_speech, pad, keep; };
static SgArgs segments_check_config(const mt2_segments_config* cfg) {
    MT2_REQUIRE(cfg != nullptr, "null segments configuration");
    MT2_REQUIRE(std::isfinite(cfg->top_db) && cfg->top_db > 0.0f, "top_db must be finite and > 0");
    MT2_REQUIRE(cfg->min_speech >= 2, "min_speech < 2 frames");
    MT2_REQUIRE(cfg->pad >= 0, "pad < 0");
    MT2_REQUIRE((long long)cfg->min_pause > 2ll * cfg->pad, "min_pause <= 2 pad (padded segments could touch; no merge step exists)");
    MT2_REQUIRE(cfg->keep == 0 || cfg->keep == 1, "keep neither 0 (speech) nor 1 (pauses)");
    return {trim_factor(cfg->top_db), cfg->min_pause, cfg->min_speech, cfg->pad, cfg->keep};
}
// the checked geometry of a call: lengths in samples (empty for the staged form), frames, the longest of each
struct SgCall { SgArgs a; std::vector<int> len, flen; int max_len, max_F; };
// the ragged lengths in samples (lens NULL: every utterance L_max samples) -> their frames
static void segments_lens(SgCall& k, const int* lens, int L_max, int B) {
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(L_max >= 1, "L_max < 1");
    k.len.assign(B, L_max);
    if (lens) k.len.assign(lens, lens + B);
    k.max_len = check_lens(k.len.data(), B, L_max, "waveform length outside [1, L_max]");
    MT2_REQUIRE(k.max_len <= INT_MAX - 4 * MT2_TRIM_HOP, "waveform longer than INT_MAX - 4 * 512 samples");
    k.flen.resize(B);
    for (int b = 0; b < B; ++b) k.flen[b] = trim_frames(k.len[b]);
    k.max_F = trim_frames(k.max_len);
}
// the arena of a call, in carve order: the plan, for the audio calls the block sums, the peak words and the energies, then the
// scratch of the smoothing kernel.  Optional outputs change nothing here, so the query holds for every form of a call
struct SgWs { float* sums; unsigned* peak; float* energy; int* prv; int* dst; unsigned char* fb; unsigned char* fc; unsigned char* fd; int* words; };
template <class Ws> static SgWs segments_carve(Ws& ws, IntPlan& ip, size_t B, size_t NB, size_t W, bool audio) {
    SgWs w{};
    ip.carve(ws);
    if (audio) {
        w.sums = ws.template get<float>(B * NB);
        w.peak = ws.template get<unsigned>(B);
        w.energy = ws.template get<float>(B * W);
    }
    w.prv = ws.template get<int>(B * W);
    w.dst = ws.template get<int>(B * W);
    w.fb = ws.template get<unsigned char>(B * W);
    w.fc = ws.template get<unsigned char>(B * W);
    w.fd = ws.template get<unsigned char>(B * W);
    w.words = ws.template get<int>(B * kSegWords);
    return w;
}
static long long segments_arena_bytes(size_t B, size_t NB, size_t W, bool audio) {
    IntPlan ip;      // the entries of the call's plan, by size: frames and - for the audio calls - lengths
    for (int i = 0; i < (audio ? 2 : 1); ++i) ip.add_fill(B, 0);
    ArenaCount count;
    segments_carve(count, ip, B, NB, W, audio);
    return (long long)count.bytes;
}
static size_t segments_blocks(int max_len) { return ((size_t)max_len + MT2_TRIM_HOP - 1) / MT2_TRIM_HOP; }
// what the three calls share of their checks, behind the configuration and the lengths
static void segments_check_outputs(const SgCall& k, int B, const void* in, size_t n_in, const uint8_t* flags, int F_max, const int32_t* segments,
                                   int S_max, const int32_t* counts, const double* figures, const float* energy, const float* out, size_t n_out) {
    MT2_REQUIRE((((uintptr_t)in | (uintptr_t)segments | (uintptr_t)counts | (uintptr_t)energy | (uintptr_t)out) & 3) == 0 && ((uintptr_t)figures & 7) == 0,
                "misaligned buffers");
    MT2_REQUIRE(segments == nullptr || (long long)S_max >= segments_bound(k.max_F, k.a.min_pause, k.a.min_speech),
                "S_max smaller than max(1, (F + min_pause) / (min_speech + min_pause)) (mt2_segments_query)");
    MT2_REQUIRE((flags == nullptr && energy == nullptr) || F_max >= k.max_F, "F_max smaller than the frames of the longest utterance");
    const size_t nf = flags ? (size_t)B * F_max : 0, ne = energy ? sizeof(float) * (size_t)B * F_max : 0;
    const size_t ns = segments ? sizeof(int32_t) * 2 * (size_t)B * S_max : 0, nc = sizeof(int32_t) * (size_t)B;
    const size_t ng = sizeof(double) * MT2_SEGMENTS_FIELDS * (size_t)B;
    MT2_REQUIRE(!outputs_overlap({{flags, nf}, {segments, ns}, {counts, nc}, {figures, ng}, {energy, ne}, {out, n_out}}, {{in, n_in}}), "overlapping buffers");
}
// the smoothing launch of all three calls
static SegP segments_params(const SgCall& k, const SgWs& w, const IntPlan& ip, int o_flen, const float* energy, int E_pitch, int B, int W,
                            int32_t* segments, int S_max, int32_t* counts, double* figures) {
    SegP p{};
    p.energy = energy; p.E_pitch = E_pitch; p.flen = ip.dev(o_flen); p.max_F = k.max_F; p.B = B;
    p.factor = k.a.factor; p.min_pause = k.a.min_pause; p.min_speech = k.a.min_speech; p.pad = k.a.pad; p.keep = k.a.keep;
    p.prv = w.prv; p.dst = w.dst; p.fb = w.fb; p.fc = w.fc; p.fd = w.fd; p.W = W; p.words = w.words;
    p.seg = segments; p.S_max = S_max; p.counts = counts; p.fig = figures;
    return p;
}

static SgCall segment_frames_check(const mt2_segments_config* cfg, const float* energy, const int* frame_lens, int F_max, int B, const uint8_t* flags,
                                   const int32_t* segments, int S_max, const int32_t* counts, const double* figures) {
    SgCall k{};
    k.a = segments_check_config(cfg);
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(energy != nullptr && frame_lens != nullptr, "bad buffers");
    MT2_REQUIRE(F_max >= 1 && F_max <= INT_MAX / MT2_TRIM_HOP, "F_max outside [1, INT_MAX / 512]");
    k.flen.assign(frame_lens, frame_lens + B);
    k.max_F = check_lens(frame_lens, B, F_max, "frame count outside [1, F_max]");
    segments_check_outputs(k, B, energy, sizeof(float) * (size_t)B * F_max, flags, F_max, segments, S_max, counts, figures, nullptr, nullptr, 0);
    return k;
}
// enqueues only
static void segment_frames_run(const Ctx& c, const SgCall& k, const float* energy, int F_max, int B, uint8_t* flags, int32_t* segments, int S_max,
                               int32_t* counts, double* figures) {
    IntPlan ip;
    const int o_flen = ip.add(k.flen);
    const SgWs w = segments_carve(c.ws, ip, B, 0, k.max_F, false);
    ip.send(c.m.pinned(), c.s);
    SegP p = segments_params(k, w, ip, o_flen, energy, F_max, B, k.max_F, segments, S_max, counts, figures);
    p.flags = flags; p.D_pitch = F_max;
    Stages st(c.m, c.s);
    st.mark("start");
    MT2_HIP(launch_segments(p, kSegSmooth, c.s));
    st.mark("seg_smooth");
    if (figures) MT2_HIP(launch_segments(p, kSegFigures, c.s));
    st.mark("seg_figures");
    st.finish();
}

// out NULL: mt2_speech_segments
static SgCall segments_check(const mt2_segments_config* cfg, const float* wav, const int* lens, int L_max, int B, const float* out, int Lout_max,
                             bool cut, const int32_t* segments, int S_max, const int32_t* counts, const double* figures, const float* energy,
                             int F_max) {
    SgCall k{};
    k.a = segments_check_config(cfg);
    MT2_REQUIRE(wav != nullptr && lens != nullptr, "bad buffers");
    segments_lens(k, lens, L_max, B);
    if (cut) {
        MT2_REQUIRE(out != nullptr, "null out");
        MT2_REQUIRE(Lout_max >= k.max_len, "Lout_max smaller than the longest utterance (the cut is not known before the call)");
    }
    segments_check_outputs(k, B, wav, sizeof(float) * (size_t)B * L_max, nullptr, F_max, segments, S_max, counts, figures, energy, out,
                           cut ? sizeof(float) * (size_t)B * Lout_max : 0);
    return k;
}
// enqueues only, unless out_lens asks for the one copy to the host and the one synchronise
static void segments_run(const Ctx& c, const SgCall& k, const float* wav, int L_max, int B, float* out, int Lout_max, int32_t* out_lens,
                         int32_t* segments, int S_max, int32_t* counts, double* figures, float* energy, int F_max) {
    IntPlan ip;
    const int o_flen = ip.add(k.flen), o_len = ip.add(k.len);
    const int NB = (int)segments_blocks(k.max_len), W = k.max_F;
    const SgWs w = segments_carve(c.ws, ip, B, NB, W, true);
    ip.send(c.m.pinned(), c.s);
    TrimP t{};
    t.wav = wav; t.L_max = L_max; t.len = ip.dev(o_len); t.max_len = k.max_len; t.B = B; t.factor = k.a.factor;
    t.sums = w.sums; t.NB = NB; t.peak = w.peak;
    t.energy = energy ? energy : w.energy; t.F_max = energy ? F_max : W;
    SegP p = segments_params(k, w, ip, o_flen, t.energy, t.F_max, B, W, segments, S_max, counts, figures);
    p.len = t.len; p.wav = wav; p.L_max = L_max; p.out = out; p.Lout_max = Lout_max;
    Stages st(c.m, c.s);
    st.mark("start");
    MT2_HIP(hipMemsetAsync(t.peak, 0, sizeof(unsigned) * B, c.s));
    MT2_HIP(launch_trim_energy(t, c.s));
    st.mark("seg_energy");
    MT2_HIP(launch_segments(p, kSegSmooth, c.s));
    st.mark("seg_smooth");
    if (figures) MT2_HIP(launch_segments(p, kSegFigures, c.s));
    st.mark("seg_figures");
    if (out) MT2_HIP(launch_segments(p, kSegCopy, c.s));
    st.mark("seg_copy");
    st.finish();
    if (out_lens) {
        int* host = static_cast<int*>(c.m.pinned().alloc(sizeof(int) * kSegWords * B));      // handle-owned staging
        MT2_HIP(hipMemcpyAsync(host, w.words, sizeof(int) * kSegWords * B, hipMemcpyDeviceToHost, c.s));
        MT2_HIP(hipStreamSynchronize(c.s));
        for (int b = 0; b < B; ++b) out_lens[b] = host[kSegWords * b + 5];
    }
}

}  // namespace mt2

// the C ABI lives in capi.hip and includes this translation unit's helpers
#include "capi.inc"
