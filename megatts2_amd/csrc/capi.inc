// extern "C" surface of libmegatts2_hip (declared in include/megatts2_hip.h).  Included at the end of
// model_stages.hip so that the stage drivers stay file-local.  Nothing throws across the boundary.

#include <climits>

namespace mt2 {
extern thread_local std::string g_last_error;
void finalize_model(mt2_model& m);
}  // namespace mt2

using namespace mt2;

// The normal exit of EVERY entry point reads a pending id verdict (model_stages.hip, ids_check): an entry point that gathers
// through caller-supplied ids cannot forget it - the open CallScope of this thread is asked at the `return 0`.
#define MT2_API_BEGIN try {
#define MT2_API_END                                 \
    ::CallScope::verdict_of_open_call();            \
    return 0;                                       \
    }                                               \
    catch (const std::exception& e) {               \
        g_last_error = e.what();                    \
        return -1;                                  \
    }                                               \
    catch (...) {                                   \
        g_last_error = "unknown error";             \
        return -1;                                  \
    }

enum Need { NEED_G = 1, NEED_ADM = 2, NEED_PLM = 4, NEED_VOC = 8 };
static void require_ready(mt2_model* m, int need = 0) {
    MT2_REQUIRE(m != nullptr, "null model handle");
    MT2_REQUIRE(m->finalized, "model not finalized");
    MT2_REQUIRE(!(need & NEED_G) || m->has_g, "generator (G.*) weights were not loaded into this handle");
    MT2_REQUIRE(!(need & NEED_ADM) || m->has_adm, "ADM (adm.*) weights were not loaded into this handle");
    MT2_REQUIRE(!(need & NEED_PLM) || m->has_plm, "PLM (plm.*) weights were not loaded into this handle");
    MT2_REQUIRE(!(need & NEED_VOC) || m->has_vocoder, "HiFi-GAN (hifigan.*) weights were not loaded");
}
// the parameters of a sampled call (include/megatts2_hip.h, mt2_sampling), checked before anything is launched
static void check_sampling(const mt2_sampling& s, int bins, bool host_seeds) {
    MT2_REQUIRE(std::isfinite(s.temperature) && s.temperature > 0.0f, "sampling temperature must be finite and > 0");
    MT2_REQUIRE(s.top_k >= 0 && s.top_k <= bins, "sampling top_k must be in [0, vq_bins]");
    MT2_REQUIRE(s.top_p > 0.0f && s.top_p <= 1.0f, "sampling top_p must be in (0, 1]");
    MT2_REQUIRE(s.reserved == 0, "mt2_sampling.reserved must be 0");
    MT2_REQUIRE(!host_seeds || s.seeds != nullptr, "sampling needs one seed per utterance (seeds is NULL)");
    MT2_REQUIRE(bins <= 1024, "the sampling kernel serves at most 1024 bins");
}
static std::vector<int> iota_rows(int B, int stride) {
    std::vector<int> v(B);
    for (int b = 0; b < B; ++b) v[b] = b * stride;
    return v;
}

// One API call on a handle.  The handle owns ONE activation arena and ONE set of internal streams / events, so:
//  * calls from several host threads are serialised (call_mutex);
//  * a call on a different stream than the previous one first waits for the previous call's end event - the arena
//    is reused from offset 0 by every call and the earlier call's kernels may still be reading it;
//  * host staging (PinnedPool) alternates between two pools; a pool is recycled only once the call that used it
//    two calls ago has finished on the device.
struct CallScope {
    mt2_model& m;
    hipStream_t s;
    std::unique_lock<std::mutex> lk;
    static thread_local CallScope* open_call;      // the call this thread is inside (one at a time: call_mutex is not recursive)
    static void verdict_of_open_call() {
        if (open_call && open_call->m.id_open) ids_verdict(Ctx{open_call->m, open_call->s, open_call->m.ws});
    }
    CallScope(mt2_model* mm, void* stream) : m(*mm), s((hipStream_t)stream), lk(mm->call_mutex) {
        if (!m.ev_call_end) MT2_HIP(hipEventCreateWithFlags(&m.ev_call_end, hipEventDisableTiming));
        if (m.call_pending && m.last_stream != s) MT2_HIP(hipStreamWaitEvent(s, m.ev_call_end, 0));
        m.pin_idx ^= 1;
        PinnedPool& p = m.pinned();
        if (!p.done) MT2_HIP(hipEventCreateWithFlags(&p.done, hipEventDisableTiming));
        if (p.recorded) MT2_HIP(hipEventSynchronize(p.done));
        p.reset();
        m.ws.reset();
        open_call = this;      // LAST: a constructor that throws above never runs the destructor - the pointer must not dangle
    }
    ~CallScope() {
        open_call = nullptr;
        // every exit path, exceptions included: internal streams forked during the call join the caller's stream before
        // the call's end is recorded (a join that already happened makes this a no-op on the device), and a pending id
        // verdict is drained (the error path that got here first has already been reported)
        if (m.aux_forked) {
            for (size_t i = 0; i < m.aux_streams.size() && i < m.ev_join.size(); ++i)
                if (hipEventRecord(m.ev_join[i], m.aux_streams[i]) == hipSuccess) (void)hipStreamWaitEvent(s, m.ev_join[i], 0);
            m.aux_forked = false;
        }
        if (m.vq_forked) {
            if (hipEventRecord(m.ev_vq_join, m.vq_stream) == hipSuccess) (void)hipStreamWaitEvent(s, m.ev_vq_join, 0);
            m.vq_forked = false;
        }
        if (m.id_open) (void)ids_wait(m);
        // the range-guard word of the fp16-pipe GEMMs travels to its pinned host copy before the call's end event
        if (m.x3h_flag_dev && m.x3h_flag_host && m.opts.x3h)
            (void)hipMemcpyAsync(m.x3h_flag_host, m.x3h_flag_dev, sizeof(int), hipMemcpyDeviceToHost, s);
        PinnedPool& p = m.pinned();
        if (p.done && hipEventRecord(p.done, s) == hipSuccess) p.recorded = true;
        if (m.ev_call_end && hipEventRecord(m.ev_call_end, s) == hipSuccess) { m.call_pending = true; m.last_stream = s; }
    }
};
thread_local CallScope* CallScope::open_call = nullptr;
#define MT2_CALL(m_, stream_)          \
    CallScope scope_((m_), (stream_)); \
    Ctx c{*(m_), scope_.s, (m_)->ws}
// the tail of the audio wrappers, behind their argument checks (every refusal of the arguments is decided before the handle is looked
// at, and before the first HIP call): the device, then the call.  MT2_AUDIO_CALL checks the handle first, for the wrappers whose
// argument checks have not
#define MT2_DEVICE_CALL(m_, stream_)                            \
    if (mt2_device_check() != 0) throw Error(g_last_error);     \
    MT2_CALL(m_, stream_)
#define MT2_AUDIO_CALL(m_, stream_)                             \
    MT2_REQUIRE((m_) != nullptr, "null model handle");          \
    MT2_DEVICE_CALL(m_, stream_)

// utterance rows with `pad` replicated frames on both sides (speechbrain HifiganGenerator.inference pads the mel with
// F.pad(c, (p, p), "replicate") before the generator): returns per-row source index into a [*, stride] layout
static std::vector<int> padded_src(const RowSet& M0, const std::vector<int>& first, const int* lens, int pad) {
    std::vector<int> src(M0.R, -1);
    for (int b = 0; b < M0.B; ++b)
        for (int t = 0; t < M0.len[b]; ++t) {
            int u = t - pad;
            u = u < 0 ? 0 : (u >= lens[b] ? lens[b] - 1 : u);
            src[M0.off[b] + t] = first[b] + u;
        }
    return src;
}

extern "C" {

const char* mt2_last_error(void) { return g_last_error.c_str(); }
const char* mt2_version(void) { return "megatts2_hip 0.1 (gfx950, f32 MFMA)"; }

int mt2_device_check(void) {
    MT2_API_BEGIN
    int n = 0;
    MT2_HIP(hipGetDeviceCount(&n));
    MT2_REQUIRE(n > 0, "no HIP device visible");
    hipDeviceProp_t prop;
    MT2_HIP(hipGetDeviceProperties(&prop, 0));
    MT2_REQUIRE(std::string(prop.gcnArchName).rfind("gfx950", 0) == 0,
                std::string("this library is built for gfx950 only, found ") + prop.gcnArchName);
    MT2_API_END
}

mt2_model* mt2_model_create(const mt2_config* cfg) {
    try {
        MT2_REQUIRE(cfg != nullptr, "null config");
        auto* m = new mt2_model();
        m->cfg = *cfg;
        return m;
    } catch (const std::exception& e) {
        g_last_error = e.what();
        return nullptr;
    }
}

int mt2_model_load_tensor(mt2_model* m, const char* name, const float* data, const int64_t* shape, int ndim) {
    MT2_API_BEGIN
    MT2_REQUIRE(m && !m->finalized, "model missing or already finalized");
    MT2_REQUIRE(name && data && shape && ndim >= 1 && ndim <= 4, "bad tensor arguments");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        MT2_REQUIRE(shape[i] >= 0, "negative dimension");
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(data, data + n);
    MT2_REQUIRE(m->host.count(name) == 0, std::string("duplicate tensor ") + name);
    m->host.emplace(name, std::move(t));
    MT2_API_END
}

int mt2_model_finalize(mt2_model* m) {
    MT2_API_BEGIN
    MT2_REQUIRE(m && !m->finalized, "model missing or already finalized");
    if (mt2_device_check() != 0) throw Error(g_last_error);
    finalize_model(*m);
    MT2_HIP(hipMalloc((void**)&m->x3h_flag_dev, 4 * sizeof(int)));
    MT2_HIP(hipMemset(m->x3h_flag_dev, 0, 4 * sizeof(int)));
    MT2_HIP(hipHostMalloc((void**)&m->x3h_flag_host, 4 * sizeof(int), hipHostMallocDefault));
    *m->x3h_flag_host = 0;
    m->opts.x3h_flag = m->x3h_flag_dev;
    MT2_API_END
}

// Range guard of the fp16-pipe GEMMs (gemm_x3h.hip; option "x3h").  Waits for the handle's last call to finish, then reports
// (and clears) whether one of its x3h launches converted an activation with |a| >= 65504 - the caller then repeats that call with
// option x3h = 0 (the bf16 six-product form has the f32 exponent range).  Cheap: one event wait and one pinned host word.
int mt2_x3h_guard(mt2_model* m, int* tripped) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && tripped != nullptr, "null argument");
    std::lock_guard<std::mutex> lk(m->call_mutex);
    *tripped = 0;
    if (!m->x3h_flag_dev || !m->x3h_flag_host) return 0;
    if (m->call_pending) MT2_HIP(hipEventSynchronize(m->ev_call_end));
    if (*m->x3h_flag_host) {
        *tripped = 1;
        *m->x3h_flag_host = 0;
        MT2_HIP(hipMemset(m->x3h_flag_dev, 0, sizeof(int)));
    }
    MT2_API_END
}

void mt2_model_destroy(mt2_model* m) {
    if (!m) return;
    for (hipStream_t s : m->aux_streams) (void)hipStreamDestroy(s);
    if (m->ev_fork) (void)hipEventDestroy(m->ev_fork);
    if (m->ev_call_end) (void)hipEventDestroy(m->ev_call_end);
    if (m->vq_stream) (void)hipStreamDestroy(m->vq_stream);
    if (m->id_stream) (void)hipStreamDestroy(m->id_stream);
    for (hipEvent_t e : {m->ev_id_fork, m->ev_id_done})
        if (e) (void)hipEventDestroy(e);
    if (m->id_flag_dev) (void)hipFree(m->id_flag_dev);
    if (m->id_flag_host) (void)hipHostFree(m->id_flag_host);
    if (m->x3h_flag_dev) (void)hipFree(m->x3h_flag_dev);
    if (m->x3h_flag_host) (void)hipHostFree(m->x3h_flag_host);
    for (hipEvent_t e : {m->ev_vq_fork, m->ev_vq_join, m->ev_vq_t0, m->ev_vq_t1})
        if (e) (void)hipEventDestroy(e);
    for (auto& r : m->opts.trace) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    for (hipEvent_t e : m->ev_join) (void)hipEventDestroy(e);
    for (void* p : m->dev_allocs) (void)hipFree(p);
    delete m;
}

int mt2_model_memory(const mt2_model* m, size_t* weight_bytes, size_t* workspace_bytes) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr, "null model handle");
    if (weight_bytes) *weight_bytes = m->weight_bytes;
    if (workspace_bytes) *workspace_bytes = m->ws.capacity();
    MT2_API_END
}

int mt2_workspace_high_water(const mt2_model* m, size_t* bytes) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && bytes != nullptr, "null argument");
    *bytes = m->ws.high_water();
    MT2_API_END
}

int mt2_workspace_reserve(mt2_model* m, size_t bytes) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr, "null model handle");
    std::lock_guard<std::mutex> lk(m->call_mutex);
    m->ws.reserve(bytes);
    MT2_API_END
}

// Test hooks (tests/test_gpu_workspace_poison.py): the arena is never cleared between calls, so what a call finds there is what the
// previous call left.  These two let a test decide what that is, and look at what a call left.  Both wait for the handle's pending
// call first (its kernels may still be reading the arena) and return with their own device work finished.
int mt2_workspace_fill(mt2_model* m, int byte) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr, "null model handle");
    MT2_REQUIRE(byte >= 0 && byte <= 255, "fill byte must be in 0..255");
    std::lock_guard<std::mutex> lk(m->call_mutex);
    if (m->call_pending) MT2_HIP(hipEventSynchronize(m->ev_call_end));
    m->ws.fill(byte);
    MT2_API_END
}

int mt2_workspace_peek(mt2_model* m, size_t offset, void* dst_host, size_t bytes) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && (dst_host != nullptr || bytes == 0), "null argument");
    std::lock_guard<std::mutex> lk(m->call_mutex);
    if (m->call_pending) MT2_HIP(hipEventSynchronize(m->ev_call_end));
    m->ws.peek(offset, dst_host, bytes);
    MT2_API_END
}

// Gap rows between the utterances of a vocoder batch, at the mel level.  A zero-padded "same" convolution of one utterance has to read
// zeros behind its ends, never a neighbour's rows: at every stage the gap - times the rows per mel frame there - covers the stage's
// widest halo, (k - 1) / 2 x dilation; the reflect edge mode (speechbrain) keeps TWO halos in every gap.  Never less than the 4 / 8
// rows of the production generator (x8 first: conv_pre k7 3 mel rows, stage 0 25 rows of 8, stage 1 25 of 64), so its row layout is
// what it always was; a generator whose first rate is small (x2: 25 rows of 2) gets the 13 rows it needs instead of its
// neighbours' samples.
static int vocoder_gap(const mt2_model& m) {
    const mt2_config& cfg = m.cfg;
    const long long halos = cfg.hg_reflect_pad ? 2 : 1;
    long long gap = cfg.hg_reflect_pad ? 8 : 4, scale = 1;
    const auto need = [&](long long halo) { gap = std::max(gap, (halos * halo + scale - 1) / scale); };
    need((m.hg_pre.k - 1) / 2);
    for (int i = 0; i < cfg.hg_n_up; ++i) {
        scale *= cfg.hg_up_rates[i];
        for (int j = 0; j < cfg.hg_n_res && (size_t)(i * cfg.hg_n_res + j) < m.hg_res.size(); ++j) {
            const ResW& r = m.hg_res[(size_t)i * cfg.hg_n_res + j];
            for (int n = 0; n < 3; ++n) need((long long)(r.k - 1) / 2 * r.dil[n]);
        }
    }
    need((m.hg_post.k - 1) / 2);
    return (int)gap;
}

// Upper bound of the arena bytes one mt2_synthesize_batch call of this geometry takes (every utterance at the
// maxima).  Mirrors the allocations of the stage drivers; tests/test_gpu_stages.py checks bound >= high-water.
int mt2_workspace_query(const mt2_model* m, int B, int Np_max, int Tp_max, int Tm_cap, int flags, size_t* bytes) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && bytes != nullptr && B >= 1 && Np_max >= 1 && Tp_max >= 1 && Tm_cap >= 1, "bad arguments");
    const mt2_config& cfg = m->cfg;
    auto rows = [&](long long len, int gap) { return (long long)gap + (long long)B * (len + gap); };
    auto enc = [&](long long M, long long d, long long ff) {
        return M * (5 * d + ff + 128) + std::max(256ll * 32 * 64 + 16ll * 32 * d, 8 * M * d) + 7 * 64;
    };
    // an AR run over B sequences of up to L positions: step rows, layer-0 QKV cache, last rows, encoder scratch per stream group
    auto ar = [&](long long d, long long ff, long long L, int stage_groups) {
        const long long M = (long long)B * L;
        const int G = std::max(1, std::min(stage_groups > 0 ? stage_groups : m->ar_groups, B));
        return M * d + 3 * M * d + (long long)B * d + G * enc(0, d, ff) + enc(M + 2ll * B * G, d, ff) - enc(0, d, ff);
    };
    const long long H = cfg.mrte_hidden, st = cfg.mrte_stride;
    const long long FR = rows(Tp_max, prompt_mel_gap(cfg)), XR = rows((Tp_max - 1) / st + 1, mel_context_gap(cfg)), PR = rows(Np_max, phone_gap(cfg));
    long long f = 0;                                                              // floats (ints counted as floats)
    f += 16 * (FR + XR + PR) + 64;                                               // integer plans
    f += FR * cfg.mel_bins + FR * H + 4 * FR * H * cfg.mrte_n_layer + XR * H * cfg.mrte_n_layer;
    f += 4 * XR * H * cfg.mrte_n_layer + 2 * XR * H;
    f += PR * H + enc(PR, H, cfg.content_ff_dim) + 2 * XR * H + 2 * PR * H;
    if (!(flags & MT2_SKIP_ADM)) {
        f += PR * cfg.adm_tc_emb_dim + (long long)B * (Np_max + 1) + 8ll * B;
        f += ar(cfg.adm_emb_dim + cfg.adm_tc_emb_dim, 4ll * cfg.adm_emb_dim, Np_max, m->adm_groups);
    }
    const long long DR = rows(Tm_cap, decoder_gap(cfg)), DIN = H + cfg.vq_dim, Tq = (Tm_cap + cfg.vq_stride - 1) / cfg.vq_stride;
    f += 8 * DR + 4ll * B * Tq + DR * DIN + (long long)B * Tq * H + (long long)B * Np_max;
    if (flags & MT2_RUN_PLM) {
        const long long d = cfg.plm_vq_dim + cfg.plm_tc_dim;
        f += 2ll * B * (Tq + 1) + 2ll * B * Tq + 8ll * B + (long long)B * cfg.plm_bins + 2ll * B;   // + seeds of a sampled call
        f += ar(d, 4 * d, Tq, m->plm_groups);
    }
    f += DR * cfg.dec_hidden * 5 + DR * cfg.mel_bins;
    if (flags & MT2_PROMPT_VQPE) {      // vqpe_rows on the prompt mel
        const long long VR = rows(Tp_max, vqpe_gap(cfg)), QR = rows((Tp_max + cfg.vq_stride - 1) / cfg.vq_stride, vqpe_gap(cfg));
        const long long C = cfg.vq_hidden, G = cfg.vq_n_layers;
        f += 16 * (VR + QR) + VR * cfg.mel_bins + VR * C + 4 * VR * C * G + G * QR * C + 4 * QR * C * G + QR * C;
        f += QR * cfg.vq_dim + QR * cfg.vq_bins + 2 * QR;
    }
    if (flags & MT2_RUN_VOCODER) {
        const long long pad = cfg.hg_inference_padding;
        long long R = rows(Tm_cap + 2 * pad, vocoder_gap(*m)), ch = cfg.hg_init_channels;
        f += 4 * R + R * cfg.mel_bins + R * ch;
        for (int i = 0; i < cfg.hg_n_up; ++i) {
            R *= cfg.hg_up_rates[i];
            ch /= 2;
            f += R + 14 * R * ch;
        }
        f += R + 4ll * B + 64;
    }
    // every allocation is rounded up to 256 B: < 400 allocations per call
    *bytes = (size_t)f * sizeof(float) + (size_t)400 * 256 + ((size_t)8 << 20);
    MT2_API_END
}

// The run-time options of a handle (mt2_set_option / mt2_get_option): stream-group counts, the tile-choice thresholds, and the
// switches between arithmetic forms that have a measured use (A/B records under profiles/*_opts_ab.txt).  Options whose verdict
// there was "closed" were retired with their code in rounds 3 and 6 (profiles/r06_retired_kernel_forms_and_options.patch); their names answer
// "unknown option".
static int* option_slot(mt2_model* m, const std::string& n) {
    if (n == "ar_groups") return &m->ar_groups;
    if (n == "adm_groups") return &m->adm_groups;
    if (n == "plm_groups") return &m->plm_groups;
    if (n == "force_gemm_config") return &m->opts.force_cfg;
    if (n == "t_ks4") return &m->opts.t_ks4;
    if (n == "t_ks2") return &m->opts.t_ks2;
    if (n == "t32") return &m->opts.t32;
    if (n == "t32x32") return &m->opts.t32x32;
    if (n == "t_x6_256") return &m->opts.t_x6_256;
    if (n == "t_x6_128") return &m->opts.t_x6_128;
    if (n == "t_x3h_128") return &m->opts.t_x3h_128;
    if (n == "x3h") return &m->opts.x3h;
    if (n == "x6_ks") return &m->opts.x6_ks;
    if (n == "voc_streams") return &m->opts.voc_streams;
    if (n == "ldr_prio") return &m->opts.ldr_prio;
    if (n == "skinny_rows") return &m->opts.skinny_rows;
    if (n == "skinny_nw") return &m->opts.skinny_nw;
    if (n == "skinny_pairs") return &m->opts.skinny_pairs;
    if (n == "attn_lds_min") return &m->opts.attn_lds_min;
    if (n == "attn_x6_min") return &m->opts.attn_x6_min;
    if (n == "ln_pairs_adm") return &m->opts.ln_pairs_adm;
    if (n == "ln_pairs_maxm") return &m->opts.ln_pairs_maxm;
    if (n == "a_planes") return &m->opts.a_planes;
    if (n == "pair_fuse") return &m->opts.pair_fuse;
    if (n == "up_fuse") return &m->opts.up_fuse;
    if (n == "ks_epi4") return &m->opts.ks_epi4;
    return nullptr;
}
static bool* option_flag(mt2_model* m, const std::string& n) {
    if (n == "splitk") return &m->opts.splitk;
    if (n == "stage_markers") return &m->opts.markers;
    if (n == "win_conv") return &m->opts.win_conv;
    if (n == "x6_conv") return &m->opts.x6_conv;
    if (n == "x6_gemm") return &m->opts.x6_gemm;
    if (n == "skinny_tm") return &m->opts.skinny_tm;
    if (n == "ldr64") return &m->opts.ldr64;
    return nullptr;
}
int mt2_set_option(mt2_model* m, const char* name, int value) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && name != nullptr, "null argument");
    std::lock_guard<std::mutex> lk(m->call_mutex);
    const std::string n(name);
    if (n == "ar_groups") MT2_REQUIRE(value >= 1 && value <= 8, "ar_groups must be in 1..8");
    if (int* p = option_slot(m, n)) *p = value;
    else if (bool* q = option_flag(m, n)) *q = value != 0;
    else throw Error("unknown option " + n);
    MT2_API_END
}
int mt2_get_option(mt2_model* m, const char* name, int* value) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && name != nullptr && value != nullptr, "null argument");
    const std::string n(name);
    if (int* p = option_slot(m, n)) *value = *p;
    else if (bool* q = option_flag(m, n)) *value = *q ? 1 : 0;
    else throw Error("unknown option " + n);
    MT2_API_END
}
int mt2_set_ar_groups(mt2_model* m, int groups) { return mt2_set_option(m, "ar_groups", groups); }
int mt2_set_profiling(mt2_model* m, int enable) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr, "null model handle");
    m->profiling = enable != 0;
    MT2_API_END
}
int mt2_last_stage_ms(mt2_model* m, const char** names, float* ms, int cap) {
    if (!m) return -1;
    const int n = (int)m->stage_ms.size();
    for (int i = 0; i < n && i < cap; ++i) {
        names[i] = m->stage_names[i].c_str();
        ms[i] = m->stage_ms[i];
    }
    return n;
}

// ---------------------------------------------------------------------------------------------------
int mt2_mrte_tc_latent(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens, int Np_max,
                       const float* mel, const int32_t* mel_lens, int Tp_max, int B, float* out) {
    MT2_API_BEGIN
    require_ready(m, NEED_G);
    MT2_REQUIRE(B >= 1, "empty batch");
    MT2_CALL(m, stream);
    const int H = m->cfg.mrte_hidden;
    TcResult r = tc_latent_rows(c, phone, phone_lens, Np_max, mel, mel_lens, Tp_max, B);
    IntPlan ip;
    const int o_map = plan_rowmap(ip, r.P, Np_max);
    ip.upload(c.ws, c.m.pinned(), c.s);
    MT2_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * Np_max * H, c.s));
    MT2_HIP(launch_unpack_rows(r.rows, H, H, Np_max, 0, ip.dev(o_map), out, r.P.R, c.s));
    ids_verdict(c);
    MT2_API_END
}

int mt2_mrte_mel_context(mt2_model* m, void* stream, const float* mel, const int32_t* mel_lens, int Tp_max, int B,
                         float* out, int Tc_max) {
    MT2_API_BEGIN
    require_ready(m, NEED_G);
    MT2_REQUIRE(B >= 1, "empty batch");
    MT2_CALL(m, stream);
    const mt2_config& cfg = m->cfg;
    IntPlan ip;
    MelPlan mp = plan_mel(ip, cfg, mel_lens, B, Tp_max, Tc_max);
    MT2_REQUIRE(mp.X.maxlen <= Tc_max, "Tc_max too small");
    ip.upload(c.ws, c.m.pinned(), c.s);
    bind_rows(ip, mp.oF, mp.F);
    bind_rows(ip, mp.oX, mp.X);
    float* xmel = c.ws.get<float>((size_t)mp.F.R * cfg.mel_bins);
    MT2_HIP(launch_pack_rows(mel, cfg.mel_bins, Tp_max, 0, ip.dev(mp.o_rowmapF), xmel, cfg.mel_bins, mp.F.R, c.s));
    float* ctx = mel_context_rows(c, xmel, cfg.mel_bins, mp.F, mp.X, ip.dev(mp.o_rowbase));
    const int H = cfg.mrte_hidden;
    MT2_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * Tc_max * H, c.s));
    MT2_HIP(launch_unpack_rows(ctx, H, H, Tc_max, 0, ip.dev(mp.o_rowmapX), out, mp.X.R, c.s));
    MT2_API_END
}

int mt2_adm_infer_forced(mt2_model* m, void* stream, const float* tc_latent, const int32_t* lens, int Np_max, int B,
                         const float* p_prefix, int P, int max_steps, int32_t* dur, float* dur_float) {
    MT2_API_BEGIN
    require_ready(m, NEED_ADM);
    MT2_REQUIRE(B >= 1 && P >= 0 && max_steps >= 0 && (P == 0 || p_prefix != nullptr), "bad arguments");
    for (int b = 0; b < B; ++b) MT2_REQUIRE(lens[b] >= 1 && lens[b] <= Np_max, "length out of range");
    MT2_CALL(m, stream);
    MT2_HIP(hipMemsetAsync(dur, 0, sizeof(int32_t) * (size_t)B * Np_max, c.s));
    if (dur_float) MT2_HIP(hipMemsetAsync(dur_float, 0, sizeof(float) * (size_t)B * Np_max, c.s));
    ArPrefix pre;
    pre.P = P; pre.data = p_prefix; pre.max_steps = max_steps;
    adm_run(c, tc_latent, m->cfg.adm_tc_dim, B * Np_max, iota_rows(B, Np_max), lens, B, dur, dur_float, Np_max, pre);
    MT2_API_END
}
int mt2_adm_infer(mt2_model* m, void* stream, const float* tc_latent, const int32_t* lens, int Np_max, int B,
                  int32_t* dur, float* dur_float) {
    return mt2_adm_infer_forced(m, stream, tc_latent, lens, Np_max, B, nullptr, 0, 0, dur, dur_float);
}

int mt2_length_regulate(mt2_model* m, void* stream, const float* x, const int32_t* dur, const int32_t* lens,
                        int Np_max, int D, int B, float* out, int Tm_max) {
    MT2_API_BEGIN
    require_ready(m);
    MT2_REQUIRE(B >= 1 && D >= 1, "bad arguments");
    MT2_CALL(m, stream);
    IntPlan ip;
    FramePlan fp = plan_frames(ip, m->cfg, dur, Np_max, lens, B, iota_rows(B, Np_max), 8, 0, Tm_max);
    MT2_REQUIRE(fp.D.maxlen <= Tm_max, "Tm_max smaller than the longest regulated utterance");
    ip.upload(c.ws, c.m.pinned(), c.s);
    float* rows = c.ws.get<float>((size_t)fp.D.R * D);
    MT2_HIP(launch_gather_rows(x, D, ip.dev(fp.o_tcmap), rows, D, D, fp.D.R, c.s));
    MT2_HIP(hipMemsetAsync(out, 0, sizeof(float) * (size_t)B * Tm_max * D, c.s));
    MT2_HIP(launch_unpack_rows(rows, D, D, Tm_max, 0, ip.dev(fp.o_rowmapD), out, fp.D.R, c.s));
    MT2_API_END
}

int mt2_max_pool_ceil(mt2_model* m, void* stream, const float* x, const int32_t* lens, int T_max, int D, int B,
                      int k, float* out, int Tq_max) {
    MT2_API_BEGIN
    require_ready(m);
    MT2_REQUIRE(B >= 1 && D % 4 == 0 && k >= 1, "bad arguments");
    MT2_CALL(m, stream);
    IntPlan ip;
    std::vector<int> first((size_t)B * Tq_max, 0), cnt((size_t)B * Tq_max, 0);
    for (int b = 0; b < B; ++b) {
        const int tq = (lens[b] + k - 1) / k;
        MT2_REQUIRE(lens[b] >= 0 && lens[b] <= T_max && tq <= Tq_max, "length out of range");
        for (int q = 0; q < tq; ++q) {
            first[(size_t)b * Tq_max + q] = b * T_max + q * k;
            cnt[(size_t)b * Tq_max + q] = std::min(k, lens[b] - q * k);
        }
    }
    const int o_first = ip.add(first), o_cnt = ip.add(cnt);
    ip.upload(c.ws, c.m.pinned(), c.s);
    MT2_HIP(launch_pool_max(x, D, ip.dev(o_first), ip.dev(o_cnt), out, D, D, B * Tq_max, c.s));
    MT2_API_END
}

int mt2_plm_infer_sampled(mt2_model* m, void* stream, const float* cond, const int32_t* lens, int Tq_max, int B,
                          const int64_t* prefix_codes, int P, int max_steps, int64_t* codes, float* last_logits,
                          const mt2_sampling* sampling) {
    MT2_API_BEGIN
    require_ready(m, NEED_PLM);
    MT2_REQUIRE(B >= 1 && P >= 0 && max_steps >= 0 && (P == 0 || prefix_codes != nullptr), "bad arguments");
    if (sampling) check_sampling(*sampling, m->cfg.plm_bins, true);
    std::vector<int> total(B);
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(lens[b] >= 1 && lens[b] <= Tq_max, "length out of range");
        total[b] = P + lens[b];
    }
    MT2_CALL(m, stream);
    if (P > 0)     // prompt codes index pc_embedding [bins + 2, vq_dim]
        ids_check(c, prefix_codes, nullptr, (long long)B * P, m->cfg.plm_bins + 2, ID_PREFIX);
    MT2_HIP(hipMemsetAsync(codes, 0, sizeof(int64_t) * (size_t)B * Tq_max, c.s));
    ArPrefix pre;
    pre.P = P; pre.data = prefix_codes; pre.max_steps = max_steps;
    plm_run(c, cond, m->cfg.plm_tc_dim, iota_rows(B, P + Tq_max), total.data(), B, codes, Tq_max, last_logits, Tq_max, pre,
            sampling);
    ids_verdict(c);
    MT2_API_END
}
// prosody interpolation: two contexts per utterance decoded in lock step on the mixture of their next-code distributions
int mt2_plm_infer_interpolated(mt2_model* m, void* stream, const float* cond, const int32_t* lens, int Tq_max, int B,
                               const int64_t* prefix_codes, int P, const float* gamma, int max_steps, int64_t* codes,
                               float* last_logits, const mt2_sampling* sampling) {
    MT2_API_BEGIN
    require_ready(m, NEED_PLM);
    MT2_REQUIRE(B >= 1 && P >= 0 && max_steps >= 0, "bad arguments");
    MT2_REQUIRE(P == 0 || prefix_codes != nullptr, "prefix_codes is NULL with P > 0");
    MT2_REQUIRE(gamma != nullptr, "gamma is NULL (one interpolation weight per utterance)");
    for (int b = 0; b < B; ++b) MT2_REQUIRE(gamma[b] >= 0.0f && gamma[b] <= 1.0f, "gamma must be in [0, 1]");      // (false for NaN)
    if (sampling) check_sampling(*sampling, m->cfg.plm_bins, true);
    MT2_REQUIRE(m->cfg.plm_bins <= 1024, "the mixture kernel serves at most 1024 bins");
    std::vector<int> total(B);
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(lens[b] >= 1 && lens[b] <= Tq_max, "length out of range");
        total[b] = P + lens[b];
    }
    MT2_CALL(m, stream);
    if (P > 0)     // both contexts' prompt codes index pc_embedding [bins + 2, vq_dim]
        ids_check(c, prefix_codes, nullptr, 2ll * B * P, m->cfg.plm_bins + 2, ID_PREFIX);
    MT2_HIP(hipMemsetAsync(codes, 0, sizeof(int64_t) * (size_t)B * Tq_max, c.s));
    ArPrefix pre;
    pre.P = P; pre.data = prefix_codes; pre.max_steps = max_steps;
    plm_run(c, cond, m->cfg.plm_tc_dim, iota_rows(2 * B, P + Tq_max), total.data(), B, codes, Tq_max, last_logits, Tq_max, pre,
            sampling, gamma);
    ids_verdict(c);
    MT2_API_END
}
int mt2_plm_infer_prompted(mt2_model* m, void* stream, const float* cond, const int32_t* lens, int Tq_max, int B,
                           const int64_t* prefix_codes, int P, int max_steps, int64_t* codes, float* last_logits) {
    return mt2_plm_infer_sampled(m, stream, cond, lens, Tq_max, B, prefix_codes, P, max_steps, codes, last_logits, nullptr);
}
int mt2_plm_infer(mt2_model* m, void* stream, const float* cond, const int32_t* lens, int Tq_max, int B,
                  int64_t* codes, float* last_logits) {
    return mt2_plm_infer_prompted(m, stream, cond, lens, Tq_max, B, nullptr, 0, 0, codes, last_logits);
}

int mt2_vq_decode(mt2_model* m, void* stream, const int64_t* codes, int B, int Tq_max, float* out) {
    MT2_API_BEGIN
    require_ready(m, NEED_G);
    MT2_CALL(m, stream);
    const int Dq = m->cfg.vq_dim, R = B * Tq_max;
    IntPlan ip;
    std::vector<int> ident(R);
    std::iota(ident.begin(), ident.end(), 0);
    const int o_id = ip.add(ident);
    ip.upload(c.ws, c.m.pinned(), c.s);
    ids_check(c, codes, nullptr, R, m->cfg.vq_bins, ID_CODE);
    float* rows = c.ws.get<float>((size_t)R * Dq);
    MT2_HIP(launch_codebook_rows(m->codebook, codes, ip.dev(o_id), rows, Dq, Dq, R, m->cfg.vq_bins, c.s));
    MT2_HIP(launch_unpack_rows(rows, Dq, Dq, Tq_max, 1, ip.dev(o_id), out, R, c.s));   // "b n d -> b d n"
    ids_verdict(c);
    MT2_API_END
}

int mt2_vq_quantize(mt2_model* m, void* stream, const float* x, int M, int64_t* idx) {
    MT2_API_BEGIN
    require_ready(m, NEED_G);
    MT2_CALL(m, stream);
    const mt2_config& cfg = m->cfg;
    float* xe = c.ws.get<float>((size_t)M * cfg.vq_bins);
    linear(c, x, cfg.vq_dim, M, m->codebook, nullptr, cfg.vq_bins, cfg.vq_dim, xe, cfg.vq_bins);
    MT2_HIP(launch_vq_argmin(x, cfg.vq_dim, cfg.vq_dim, xe, cfg.vq_bins, m->codebook_sq, cfg.vq_bins, nullptr, idx, M,
                             c.s));
    MT2_API_END
}

int mt2_vqpe_forward(mt2_model* m, void* stream, const float* mel, const int32_t* lens, int T_max, int mel_ld,
                     int B, float* zq, int64_t* codes, int Tq_max, float* ze) {
    MT2_API_BEGIN
    require_ready(m, NEED_G);
    MT2_REQUIRE(B >= 1 && mel_ld % 4 == 0 && mel_ld >= m->cfg.vq_mel_bins, "bad arguments");
    MT2_CALL(m, stream);
    const int Dq = m->cfg.vq_dim;
    if (m->opts.markers) MT2_HIP(launch_stage_marker(8, c.s));
    IntPlan ip;
    VqpeResult r = vqpe_rows(c, ip, mel, mel_ld, lens, T_max, Tq_max, B);
    MT2_REQUIRE(r.Q.maxlen <= Tq_max, "Tq_max too small");
    MT2_HIP(hipMemsetAsync(codes, 0, sizeof(int64_t) * (size_t)B * Tq_max, c.s));
    MT2_HIP(launch_scatter_i64(r.idx, ip.dev(r.o_rowmapQ), codes, r.Q.R, c.s));
    // zq = codebook rows repeated x stride, cropped to T (vqpe.py:59-61)
    float* zrows = c.ws.get<float>((size_t)r.F.R * Dq);
    MT2_HIP(launch_codebook_rows(m->codebook, r.idx, ip.dev(r.o_codemapF), zrows, Dq, Dq, r.F.R, m->cfg.vq_bins, c.s));
    MT2_HIP(hipMemsetAsync(zq, 0, sizeof(float) * (size_t)B * T_max * Dq, c.s));
    MT2_HIP(launch_unpack_rows(zrows, Dq, Dq, T_max, 0, ip.dev(r.o_rowmapF), zq, r.F.R, c.s));
    if (ze) {
        MT2_HIP(hipMemsetAsync(ze, 0, sizeof(float) * (size_t)B * Tq_max * Dq, c.s));
        MT2_HIP(launch_unpack_rows(r.ze, Dq, Dq, Tq_max, 0, ip.dev(r.o_rowmapQ), ze, r.Q.R, c.s));
    }
    if (m->opts.markers) MT2_HIP(launch_stage_marker(9, c.s));
    MT2_API_END
}

int mt2_mel_decoder(mt2_model* m, void* stream, const float* x, const int32_t* lens, int T_max, int B, float* mel) {
    MT2_API_BEGIN
    require_ready(m, NEED_G);
    MT2_REQUIRE(B >= 1, "empty batch");
    MT2_CALL(m, stream);
    const int DIN = m->dec_first.cin, NM = m->cfg.mel_bins;
    for (int b = 0; b < B; ++b) MT2_REQUIRE(lens[b] >= 1 && lens[b] <= T_max, "length out of range");
    IntPlan ip;
    RowSet D = make_rows(lens, B, decoder_gap(m->cfg));
    RowPlanOffsets oD = plan_rows(ip, D);
    const int o_map = plan_rowmap(ip, D, T_max);
    ip.upload(c.ws, c.m.pinned(), c.s);
    bind_rows(ip, oD, D);
    float* xrows = c.ws.get<float>((size_t)D.R * DIN);
    MT2_HIP(launch_pack_rows(x, DIN, T_max, 1, ip.dev(o_map), xrows, DIN, D.R, c.s));      // "B D T" -> rows
    float* mrows = decoder_rows(c, xrows, D);
    MT2_HIP(hipMemsetAsync(mel, 0, sizeof(float) * (size_t)B * NM * T_max, c.s));
    MT2_HIP(launch_unpack_rows(mrows, NM, NM, T_max, 1, ip.dev(o_map), mel, D.R, c.s));
    MT2_API_END
}

// Vocoder rows of B utterances: every utterance's mel frames with `hg_inference_padding` replicated frames on both sides, a gap of
// zero rows between utterances.  d_src[r] = source row of vocoder row r, utterance b's frames starting at first[b] (-1: gap row).
struct VocRows { RowSet M0; const int* d_src; };
static VocRows vocoder_rows(const Ctx& c, const std::vector<int>& first, const int* lens, int B) {
    const mt2_config& cfg = c.m.cfg;
    const int pad = cfg.hg_inference_padding;
    std::vector<int> plen(B);
    for (int b = 0; b < B; ++b) plen[b] = lens[b] + 2 * pad;
    IntPlan ip;
    VocRows v;
    v.M0 = make_rows(plen.data(), B, vocoder_gap(c.m));
    const RowPlanOffsets o = plan_rows(ip, v.M0);
    const int o_src = ip.add(padded_src(v.M0, first, lens, pad));
    ip.upload(c.ws, c.m.pinned(), c.s);
    bind_rows(ip, o, v.M0);
    v.d_src = ip.dev(o_src);
    return v;
}
// waveform rows (hifigan_rows: hop samples per vocoder row) -> wav [B, hop * T_cap], zero behind every utterance
static void hifigan_to_wav(const Ctx& c, const float* wavrows, const RowSet& M0, float* wav, int T_cap) {
    int hop = 1;
    for (int i = 0; i < c.m.cfg.hg_n_up; ++i) hop *= c.m.cfg.hg_up_rates[i];
    const size_t n = 2 * (size_t)M0.B;
    long long* st = static_cast<long long*>(c.m.pinned().alloc(n * sizeof(long long)));   // handle-owned staging
    long long mx = 0;
    for (int b = 0; b < M0.B; ++b) {
        st[b] = (long long)M0.off[b] * hop;
        st[M0.B + b] = (long long)M0.len[b] * hop;
        mx = std::max(mx, st[M0.B + b]);
    }
    long long* d = c.ws.get<long long>(n);
    MT2_HIP(hipMemcpyAsync(d, st, n * sizeof(long long), hipMemcpyHostToDevice, c.s));
    MT2_HIP(hipMemsetAsync(wav, 0, sizeof(float) * (size_t)M0.B * hop * T_cap, c.s));
    MT2_HIP(launch_unpack_wav(wavrows, d, d + M0.B, wav, (long long)hop * T_cap, mx, M0.B, c.s));
}

int mt2_hifigan(mt2_model* m, void* stream, const float* mel, const int32_t* lens, int T_max, int B, float* wav) {
    MT2_API_BEGIN
    require_ready(m, NEED_VOC);
    MT2_REQUIRE(B >= 1, "empty batch");
    MT2_CALL(m, stream);
    const int NM = m->cfg.hg_in_dim;
    for (int b = 0; b < B; ++b) MT2_REQUIRE(lens[b] >= 1 && lens[b] <= T_max, "length out of range");
    const VocRows v = vocoder_rows(c, iota_rows(B, T_max), lens, B);      // d_src[r] = b*T_max + t
    float* xrows = c.ws.get<float>((size_t)v.M0.R * NM);
    MT2_HIP(launch_pack_rows(mel, NM, T_max, 1, v.d_src, xrows, NM, v.M0.R, c.s));
    hifigan_to_wav(c, hifigan_rows(c, xrows, v.M0), v.M0, wav, T_max + 2 * m->cfg.hg_inference_padding);
    MT2_API_END
}

int mt2_mel_spectrogram(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* wav, const int32_t* lens,
                        int L_max, int B, float* mel, int T_max) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && ac != nullptr && B >= 1, "bad arguments");
    MT2_DEVICE_CALL(m, stream);
    mel_spectrogram_run(c, *ac, wav, lens, L_max, B, mel, T_max);
    MT2_API_END
}

// models/megatts2.py:335  librosa.load(wav, sr=16000): the length / ratio rule of the resampler, without a HIP call
int mt2_resample_query(int sr_in, int sr_out, long long L, long long* L_out, int* o, int* n, int* taps) {
    MT2_API_BEGIN
    ResampleRule r{};
    if (const char* why = resample_rule(sr_in, sr_out, &r)) throw Error(std::string("mt2_resample_query: ") + why);
    MT2_REQUIRE(L >= 0 && L <= INT_MAX, "L outside [0, 2^31)");
    if (L_out) *L_out = resample_out_len(r, L);
    if (o) *o = r.o;
    if (n) *n = r.n;
    if (taps) *taps = r.taps;
    MT2_API_END
}

// models/megatts2.py:335  the filter the device applies, phase-major [n][taps] (host only: lets a test pin it without a GPU)
int mt2_resample_table(int sr_in, int sr_out, float* table) {
    MT2_API_BEGIN
    ResampleRule r{};
    if (const char* why = resample_rule(sr_in, sr_out, &r)) throw Error(std::string("mt2_resample_table: ") + why);
    MT2_REQUIRE(table != nullptr, "null table");
    resample_table(r, table, false);
    MT2_API_END
}

// models/megatts2.py:335-336  librosa.load(wav, sr=16000) [+ librosa.util.normalize with MT2_RESAMPLE_NORMALIZE] for a ragged batch
int mt2_resample(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sr_in, int sr_out, int flags,
                 float* out, int Lout_max, int32_t* out_lens) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && B >= 1 && L_max >= 1 && Lout_max >= 1, "bad arguments");
    MT2_DEVICE_CALL(m, stream);
    resample_run(c, wav, lens, L_max, B, sr_in, sr_out, flags, out, Lout_max, out_lens);
    MT2_API_END
}

// models/megatts2.py:336  librosa.util.normalize alone (audio already at the model's rate)
int mt2_peak_normalize(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, float* out) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && B >= 1 && L_max >= 1, "bad arguments");
    MT2_DEVICE_CALL(m, stream);
    peak_normalize_run(c, wav, lens, L_max, B, out);
    MT2_API_END
}

// models/megatts2.py:337  librosa.effects.trim: the frame count and the f32 threshold factor of the rule, without a HIP call
int mt2_trim_query(long long L, float top_db, int* frames, float* factor) {
    MT2_API_BEGIN
    MT2_REQUIRE(L >= 1 && L <= INT_MAX - 4 * MT2_TRIM_HOP, "L outside [1, 2^31 - 2048)");
    MT2_REQUIRE(std::isfinite(top_db) && top_db > 0.0f, "top_db must be finite and > 0");
    if (frames) *frames = trim_frames(L);
    if (factor) *factor = trim_factor(top_db);
    MT2_API_END
}

// models/megatts2.py:337  librosa.effects.trim(y, top_db) for a ragged batch
int mt2_trim_silence(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, float top_db, float* out,
                     int Lout_max, int32_t* bounds, float* energy, int F_max) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && B >= 1 && L_max >= 1 && Lout_max >= 1, "bad arguments");
    MT2_DEVICE_CALL(m, stream);
    trim_run(c, wav, lens, L_max, B, top_db, out, Lout_max, bounds, energy, F_max);
    MT2_API_END
}

// F0 by YIN: the frame count, the lag range and the arena bytes of the rule, without a HIP call
int mt2_f0_query(int sample_rate, int hop, float fmin, float fmax, long long L, int* frames, int* lag_min, int* lag_max,
                 long long* workspace_bytes) {
    MT2_API_BEGIN
    int lo = 0, hi = 0;
    f0_check_rule(sample_rate, hop, fmin, fmax, &lo, &hi);
    MT2_REQUIRE(L >= 1 && L <= INT_MAX, "L outside [1, 2^31)");
    if (frames) *frames = (int)(1 + L / hop);
    if (lag_min) *lag_min = lo;
    if (lag_max) *lag_max = hi;
    if (workspace_bytes) *workspace_bytes = (long long)arena_round(sizeof(int) * 65535);      // the lengths of the largest batch, nothing else
    MT2_API_END
}

// F0, voicing and (optionally) d'[tau*], tau* and d of a ragged batch; every refusal is decided on the host before the first HIP call
int mt2_f0_yin(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate, int hop, float fmin,
               float fmax, float threshold, float* f0, float* cmnd, int32_t* lag, int T_max, float* diff) {
    MT2_API_BEGIN
    int lo = 0, hi = 0;
    f0_check_rule(sample_rate, hop, fmin, fmax, &lo, &hi);
    const int mx = f0_check_call(wav, lens, L_max, B, hop, threshold, f0, cmnd, lag, T_max, diff);
    MT2_AUDIO_CALL(m, stream);
    f0_run(c, {wav, lens, L_max, B, mx, sample_rate, hop, lo, hi, threshold, f0, cmnd, lag, T_max, diff});
    MT2_API_END
}

// F0 by the Viterbi pass over YIN's lag costs: frames, lag range, state count and arena bytes (B utterances, the longest of L
// samples), without a HIP call
int mt2_f0_track_query(int sample_rate, int hop, float fmin, float fmax, float octave_cost, float jump_cost, long long L, int B,
                       int* frames, int* lag_min, int* lag_max, int* states, long long* workspace_bytes) {
    MT2_API_BEGIN
    int lo = 0, hi = 0;
    f0_check_rule(sample_rate, hop, fmin, fmax, &lo, &hi);
    f0_track_check_costs(octave_cost, jump_cost);
    MT2_REQUIRE(L >= 1 && L <= INT_MAX, "L outside [1, 2^31)");
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    const long long T = 1 + L / hop;
    if (frames) *frames = (int)T;
    if (lag_min) *lag_min = lo;
    if (lag_max) *lag_max = hi;
    if (states) *states = hi - lo + 1;
    if (workspace_bytes) *workspace_bytes = f0_track_arena_bytes(B, T);
    MT2_API_END
}

// the same outputs as mt2_f0_yin by the second rule; every refusal is decided on the host before the first HIP call
int mt2_f0_track(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate, int hop, float fmin,
                 float fmax, float threshold, float octave_cost, float jump_cost, float* f0, float* cmnd, int32_t* lag, int T_max,
                 float* diff) {
    MT2_API_BEGIN
    int lo = 0, hi = 0;
    f0_check_rule(sample_rate, hop, fmin, fmax, &lo, &hi);
    f0_track_check_costs(octave_cost, jump_cost);
    const int mx = f0_check_call(wav, lens, L_max, B, hop, threshold, f0, cmnd, lag, T_max, diff);
    MT2_AUDIO_CALL(m, stream);
    f0_track_run(c, {wav, lens, L_max, B, mx, sample_rate, hop, lo, hi, threshold, f0, cmnd, lag, T_max, diff}, octave_cost, jump_cost);
    MT2_API_END
}

// the pitch moments of f0 tracks over their voiced frames
int mt2_f0_stats(mt2_model* m, void* stream, const float* f0, const int32_t* frame_lens, int T_max, int B, double* stats) {
    MT2_API_BEGIN
    f0_stats_check(f0, frame_lens, T_max, B, stats);
    MT2_AUDIO_CALL(m, stream);
    f0_stats_run(c, f0, frame_lens, T_max, B, stats);
    MT2_API_END
}

// formant candidates by linear prediction: the frame count and the arena bytes of the rule, without a HIP call
int mt2_formant_query(int sample_rate, int hop, int window, int order, long long L, int* frames, long long* workspace_bytes) {
    MT2_API_BEGIN
    formant_check_rule(sample_rate, hop, window, order);
    MT2_REQUIRE(L >= 1 && L <= INT_MAX, "L outside [1, 2^31)");
    MT2_REQUIRE(1 + L / hop <= INT_MAX, "2^31 frames or more");
    if (frames) *frames = (int)(1 + L / hop);
    if (workspace_bytes) *workspace_bytes = formant_arena_bytes();
    MT2_API_END
}

// the window the device applies, in double (host only: lets a test pin it without a GPU)
int mt2_formant_window(int window, int kind, double* table) {
    MT2_API_BEGIN
    MT2_REQUIRE(window >= 64 && window <= MT2_FORMANT_MAX_WINDOW && window % 2 == 0, "window outside [64, 1024] or odd");
    formant_check_kind(kind);
    MT2_REQUIRE(table != nullptr, "null table");
    formant_window_table(window, kind, table);
    MT2_API_END
}

// formant candidates (and, optionally, every intermediate) of a ragged batch; every refusal is decided on the host before the first HIP call
int mt2_lpc_formants(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate, int hop,
                     const mt2_formant_config* cfg, float* freq, float* bw, int32_t* count, int T_max, double* lpc, double* err,
                     double* autocorr, double* roots, int32_t* iters) {
    MT2_API_BEGIN
    formant_check_config(sample_rate, hop, cfg);
    const FormantOut o{freq, bw, count, T_max, lpc, err, autocorr, roots, iters};
    const int mx = formant_check_call(wav, lens, L_max, B, hop, cfg->order, o);
    MT2_AUDIO_CALL(m, stream);
    formant_run(c, wav, lens, L_max, B, mx, sample_rate, hop, *cfg, o);
    MT2_API_END
}

// the formant figures of candidate tracks over their frames with four candidates (voiced ones, where an F0 track is given)
int mt2_formant_stats(mt2_model* m, void* stream, const float* freq, const int32_t* count, const float* f0, const int32_t* frame_lens,
                      int T_max, int B, double* stats) {
    MT2_API_BEGIN
    formant_stats_check(freq, count, f0, frame_lens, T_max, B, stats);
    MT2_AUDIO_CALL(m, stream);
    formant_stats_run(c, freq, count, f0, frame_lens, T_max, B, stats);
    MT2_API_END
}

// formant tracks across frames: the states and the arena bytes of a call, without a HIP call
int mt2_formant_track_query(int tracks, long long T_max, int B, int* states, long long* workspace_bytes) {
    MT2_API_BEGIN
    formant_track_check_shape(tracks, T_max, B);
    if (states) *states = formant_track_states(tracks);
    if (workspace_bytes) *workspace_bytes = formant_track_arena_bytes(B, T_max);
    MT2_API_END
}

// the K candidates per frame on the cheapest smooth path (formant_track.hip); every refusal is decided on the host before the first HIP call
int mt2_formant_track(mt2_model* m, void* stream, const float* freq, const float* bw, const int32_t* count, const int32_t* frame_lens, int T_max,
                      int B, const mt2_formant_track_config* cfg, float* track_freq, float* track_bw, int32_t* track_count, int32_t* sel) {
    MT2_API_BEGIN
    formant_track_check_config(cfg);
    const FormantTrackIO a{freq, bw, count, track_freq, track_bw, track_count, sel};
    formant_track_check_call(a, frame_lens, T_max, B);
    MT2_AUDIO_CALL(m, stream);
    formant_track_run(c, a, frame_lens, T_max, B, *cfg);
    MT2_API_END
}

// the energy contour on the F0 / mel frames (prosody.hip); every refusal is decided on the host before the first HIP call
int mt2_frame_energy(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int hop, float* energy,
                     int T_max) {
    MT2_API_BEGIN
    const int mx = energy_check(wav, lens, L_max, B, hop, energy, T_max);
    MT2_AUDIO_CALL(m, stream);
    energy_run(c, wav, lens, L_max, B, mx, hop, energy, T_max);
    MT2_API_END
}

// the segment reduction of an F0 track (and an energy contour) over phone durations
int mt2_phone_prosody(mt2_model* m, void* stream, const float* f0, const float* energy, const int32_t* dur, const int32_t* phone_lens,
                      int Np_max, const int32_t* frame_lens, int T_max, int B, double* out, long long* dur_sum) {
    MT2_API_BEGIN
    phone_prosody_check(f0, energy, dur, phone_lens, Np_max, frame_lens, T_max, B, out, dur_sum);
    MT2_AUDIO_CALL(m, stream);
    phone_prosody_run(c, f0, energy, dur, phone_lens, Np_max, frame_lens, T_max, B, out, dur_sum);
    MT2_API_END
}

// the voiced frames of F0 tracks compacted to semitone contours
int mt2_pitch_contour(mt2_model* m, void* stream, const float* f0, const int32_t* frame_lens, int T_max, int B, int center, float* st,
                      int32_t* n_voiced, int32_t* index) {
    MT2_API_BEGIN
    pitch_contour_check(f0, frame_lens, T_max, B, center, st, n_voiced, index);
    MT2_AUDIO_CALL(m, stream);
    pitch_contour_run(c, f0, frame_lens, T_max, B, center, st, n_voiced, index);
    MT2_API_END
}

// integrated loudness (loudness.hip): the sub-block, the block count, the K-weighting coefficients (b0 b1 b2 a1 a2 of the shelf, then
// of the high-pass) and the arena bytes of a call with ONE utterance of L samples, without a HIP call (outputs may be NULL)
int mt2_loudness_query(int sample_rate, long long L, int* sub_block, int* blocks, double* coeffs, long long* workspace_bytes) {
    MT2_API_BEGIN
    loudness_check_query(sample_rate, L);
    const int h = sample_rate / 10;
    if (sub_block) *sub_block = h;
    if (blocks) *blocks = (int)std::max(L / h - 3, 0ll);
    if (coeffs) loudness_coeffs(sample_rate, coeffs);
    if (workspace_bytes) *workspace_bytes = loudness_arena_bytes(sample_rate, L, 1, false);
    MT2_API_END
}

// integrated loudness of a ragged batch; every refusal is decided on the host before the first HIP call
int mt2_loudness(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate, double* stats,
                 double* momentary, int NB_max) {
    MT2_API_BEGIN
    MT2_REQUIRE(stats != nullptr, "null stats");
    const WavArgs a = loudness_check({wav, lens, L_max, B, 0, sample_rate}, 0.0, 0.0, nullptr, stats, momentary, NB_max);
    MT2_AUDIO_CALL(m, stream);
    loudness_run(c, a, 0.0, 0.0, nullptr, stats, momentary, NB_max);
    MT2_API_END
}

// each utterance brought to target_lufs, the gain formed and read on the device; every refusal is decided on the host before the first HIP call
int mt2_loudness_normalize(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate,
                           double target_lufs, double peak_ceiling, float* out, double* stats) {
    MT2_API_BEGIN
    MT2_REQUIRE(out != nullptr, "null out");
    const WavArgs a = loudness_check({wav, lens, L_max, B, 0, sample_rate}, target_lufs, peak_ceiling, out, stats, nullptr, 0);
    MT2_AUDIO_CALL(m, stream);
    loudness_run(c, a, target_lufs, peak_ceiling, out, stats, nullptr, 0);
    MT2_API_END
}

// EBU-mode metering (ebu.hip): the oversampling factor, the taps per phase, the tile of the true-peak kernel, the short-term blocks and
// the arena bytes of a call with ONE utterance of L samples, without a HIP call (outputs may be NULL)
int mt2_ebu_query(int sample_rate, long long L, int* oversample, int* taps, int* tile, int* short_term_blocks, long long* workspace_bytes) {
    MT2_API_BEGIN
    loudness_check_query(sample_rate, L);
    if (oversample) *oversample = true_peak_oversample(sample_rate);
    if (taps) *taps = MT2_TP_TAPS;
    if (tile) *tile = MT2_TP_TILE;
    if (short_term_blocks) *short_term_blocks = (int)std::max(L / (sample_rate / 10) - 29, 0ll);
    if (workspace_bytes) *workspace_bytes = loudness_arena_bytes(sample_rate, L, 1, true);
    MT2_API_END
}

// the true-peak interpolation table [o][24] of a rate, without a HIP call
int mt2_true_peak_table(int sample_rate, float* table) {
    MT2_API_BEGIN
    loudness_check_rate(sample_rate);
    MT2_REQUIRE(table != nullptr, "null table");
    true_peak_table(sample_rate, table);
    MT2_API_END
}

// integrated, momentary and short-term loudness, loudness range and true peak of a ragged batch; every refusal is decided on the host
// before the first HIP call
int mt2_loudness_ebu(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate, double* stats,
                     double* momentary, int NB_max, double* short_term, int NST_max) {
    MT2_API_BEGIN
    MT2_REQUIRE(stats != nullptr, "null stats");
    const WavArgs a = ebu_check({wav, lens, L_max, B, 0, sample_rate}, 0.0, 0.0, nullptr, stats, momentary, NB_max, short_term, NST_max);
    MT2_AUDIO_CALL(m, stream);
    ebu_run(c, a, 0.0, 0.0, nullptr, stats, momentary, NB_max, short_term, NST_max);
    MT2_API_END
}

// each utterance brought to target_lufs under a true-peak ceiling, the gain formed and read on the device; every refusal is decided on
// the host before the first HIP call
int mt2_loudness_normalize_tp(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate,
                              double target_lufs, double ceiling_dbtp, float* out, double* stats) {
    MT2_API_BEGIN
    MT2_REQUIRE(out != nullptr, "null out");
    const WavArgs a = ebu_check({wav, lens, L_max, B, 0, sample_rate}, target_lufs, ceiling_dbtp, out, stats, nullptr, 0, nullptr, 0);
    MT2_AUDIO_CALL(m, stream);
    ebu_run(c, a, target_lufs, ceiling_dbtp, out, stats, nullptr, 0, nullptr, 0);
    MT2_API_END
}

// True-peak look-ahead limiter (limiter.hip): the half window, the tile of its kernels and the arena bytes of a call with ONE utterance
// of L samples, without a HIP call (outputs may be NULL)
int mt2_limiter_query(int sample_rate, long long L, double window_ms, int* half_window, int* tile, long long* workspace_bytes) {
    MT2_API_BEGIN
    loudness_check_query(sample_rate, L);
    const int H = limiter_check_window(sample_rate, window_ms);
    if (half_window) *half_window = H;
    if (tile) *tile = MT2_LIMITER_TILE;
    if (workspace_bytes) *workspace_bytes = limiter_arena_bytes(sample_rate, L, 1, H);
    MT2_API_END
}

// the limiter's 2 H + 1 weights, without a HIP call
int mt2_limiter_window(int sample_rate, double window_ms, float* w) {
    MT2_API_BEGIN
    loudness_check_rate(sample_rate);
    const int H = limiter_check_window(sample_rate, window_ms);
    MT2_REQUIRE(w != nullptr, "null w");
    limiter_window(H, w);
    MT2_API_END
}

// one pass of the limiter with a host-given gain; every refusal is decided on the host before the first HIP call
int mt2_limit_true_peak(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate,
                        double pre_gain_db, double ceiling_dbtp, double window_ms, float* out, float* gain, float* need, double* stats) {
    MT2_API_BEGIN
    int H = 0;
    const WavArgs a = limiter_check({wav, lens, L_max, B, 0, sample_rate}, 0.0, ceiling_dbtp, window_ms, 1, out, gain, need, stats, &H);
    MT2_REQUIRE(std::isfinite(pre_gain_db), "pre_gain_db must be finite");
    const float G = (float)pow(10.0, pre_gain_db / 20.0);
    MT2_REQUIRE(std::isfinite(G) && G > 0.0f, "the pre-gain is not a positive finite f32");
    MT2_AUDIO_CALL(m, stream);
    limiter_run(c, a, false, G, 0.0, ceiling_dbtp, H, 1, out, gain, need, stats);
    MT2_API_END
}

// each utterance brought to target_lufs under a true-peak ceiling by `passes` passes of the limiter, every gain formed and read on the
// device; every refusal is decided on the host before the first HIP call
int mt2_loudness_normalize_limited(mt2_model* m, void* stream, const float* wav, const int32_t* lens, int L_max, int B, int sample_rate,
                                   double target_lufs, double ceiling_dbtp, double window_ms, int passes, float* out, float* gain,
                                   float* need, double* stats) {
    MT2_API_BEGIN
    int H = 0;
    const WavArgs a = limiter_check({wav, lens, L_max, B, 0, sample_rate}, target_lufs, ceiling_dbtp, window_ms, passes, out, gain, need, stats, &H);
    MT2_AUDIO_CALL(m, stream);
    limiter_run(c, a, true, 1.0f, target_lufs, ceiling_dbtp, H, passes, out, gain, need, stats);
    MT2_API_END
}

// the STFT the mel front-end takes its magnitude of, for a ragged batch (the front half of mt2_mel_spectrogram, shared with it)
int mt2_stft(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* wav, const int32_t* lens, int L_max, int B, float* spec,
             int T_max) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && ac != nullptr && B >= 1, "bad arguments");
    MT2_DEVICE_CALL(m, stream);
    stft_only_run(c, *ac, wav, lens, L_max, B, spec, T_max);
    MT2_API_END
}

// torch.istft(center=True, length = (T - 1) hop) by the rule of griffinlim.hip; every refusal is decided on the host before the first HIP call
int mt2_istft(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* spec, const int32_t* frame_lens, int T_max, int B,
              float* wav, int L_max) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && ac != nullptr, "null model handle or audio configuration");
    gl_check_config(*ac);
    gl_check_lens(*ac, frame_lens, T_max, B, L_max);
    MT2_DEVICE_CALL(m, stream);
    istft_run(c, *ac, spec, frame_lens, T_max, B, wav, L_max);
    MT2_API_END
}

// log-mel -> linear magnitude by the pseudo-inverse of the front-end's filterbank (griffinlim.hip, step 1)
int mt2_mel_to_linear(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* mel, const int32_t* mel_lens, int T_max, int B,
                      float* mag) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && ac != nullptr && B >= 1, "bad arguments");
    gl_check_config(*ac);
    (void)gl_pinv(*ac).size();      // the rank-deficient filterbank is refused without a HIP call
    MT2_DEVICE_CALL(m, stream);
    mel_to_linear_run(c, *ac, mel, mel_lens, T_max, B, mag);
    MT2_API_END
}

// Griffin-Lim: the arena bytes and the output length of one call, without a HIP call - and every refusal of mt2_griffin_lim (L_max,
// which is not an argument here, aside)
int mt2_griffin_lim_query(const mt2_audio_config* ac, const int32_t* mel_lens, int T_max, int B, int n_iter, double momentum,
                          int want_resid, long long* workspace_bytes, long long* L_out) {
    MT2_API_BEGIN
    MT2_REQUIRE(ac != nullptr, "null audio configuration");
    gl_check_config(*ac);
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    std::vector<int> T(B, T_max);
    if (mel_lens) T.assign(mel_lens, mel_lens + B);
    const long long L = (long long)(*std::max_element(T.begin(), T.end()) - 1) * ac->hop_length;
    gl_check_call(*ac, T.data(), T_max, B, n_iter, momentum, std::max(L, 0ll));
    (void)gl_pinv(*ac).size();      // the rank-deficient filterbank
    const long long rstride = want_resid ? (long long)(n_iter + 1) * T_max : 0;
    if (workspace_bytes) *workspace_bytes = arena_bytes([&](ArenaCount& count, IntPlan& ip) { gl_layout(count, ip, *ac, T.data(), T_max, B, nullptr, rstride); });
    if (L_out) *L_out = L;
    MT2_API_END
}

// every refusal is decided on the host before the first HIP call
int mt2_griffin_lim(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* mel, const int32_t* mel_lens, int T_max, int B,
                    int n_iter, double momentum, const uint64_t* seeds, float* wav, int L_max, float* resid) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr && ac != nullptr, "null model handle or audio configuration");
    gl_check_call(*ac, mel_lens, T_max, B, n_iter, momentum, L_max);
    MT2_REQUIRE(mel != nullptr && seeds != nullptr && wav != nullptr, "bad buffers");
    if (!(m->gl_P && std::memcmp(&m->fe_cfg, ac, sizeof(*ac)) == 0)) (void)gl_pinv(*ac).size();      // rank-deficient filterbank: refused here
    MT2_DEVICE_CALL(m, stream);
    griffin_lim_run(c, *ac, mel, mel_lens, T_max, B, n_iter, momentum, seeds, wav, L_max, resid);
    MT2_API_END
}

// DTW of a synthesised mel onto a real one (dtw.hip): the arena bytes of one call, without a HIP call
int mt2_dtw_query(int Tx_max, int Ty_max, int D, int B, long long* workspace_bytes) {
    MT2_API_BEGIN
    dtw_check_geometry(Tx_max, Ty_max, D, B);
    if (workspace_bytes) *workspace_bytes = dtw_arena_bytes(Tx_max, Ty_max, B);
    MT2_API_END
}

// every refusal is decided on the host before the first HIP call
int mt2_dtw_align(mt2_model* m, void* stream, const float* X, const int32_t* x_lens, int Tx_max, const float* Y, const int32_t* y_lens,
                  int Ty_max, int D, int B, int32_t* lo, int32_t* hi, int32_t* steps, float* total, float* cost, float* acc) {
    MT2_API_BEGIN
    dtw_check_geometry(Tx_max, Ty_max, D, B);
    dtw_check_lens(x_lens, Tx_max, y_lens, Ty_max, B);
    MT2_AUDIO_CALL(m, stream);
    dtw_run(c, X, x_lens, Tx_max, Y, y_lens, Ty_max, D, B, lo, hi, steps, total, cost, acc);
    MT2_API_END
}

int mt2_align_durations(mt2_model* m, void* stream, const int32_t* hi, const int32_t* y_lens, int Ty_max, const int32_t* syn_dur,
                        const int32_t* phone_lens, int Np_max, int B, int32_t* dur_out_host) {
    MT2_API_BEGIN
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(Np_max >= 1, "Np_max < 1");
    MT2_REQUIRE(Ty_max >= 1 && Ty_max <= MT2_DTW_MAX_LEN, "Ty_max outside [1, MT2_DTW_MAX_LEN]");
    MT2_REQUIRE(y_lens != nullptr && syn_dur != nullptr && phone_lens != nullptr && dur_out_host != nullptr, "a host array is NULL");
    check_lens(y_lens, B, Ty_max, "y length outside [1, Ty_max]");
    check_lens(phone_lens, B, Np_max, "phone count outside [1, Np_max]");
    MT2_REQUIRE(m != nullptr && hi != nullptr, "null model handle or hi");
    MT2_DEVICE_CALL(m, stream);
    align_durations_run(c, hi, y_lens, Ty_max, syn_dur, phone_lens, Np_max, B, dur_out_host);
    MT2_API_END
}

// mel-cepstral distortion along the DTW path (mcd.hip): the table and the arena bytes of the whole chain, without a HIP call
int mt2_mcd_table(int n_mels, int order, float* table) {
    MT2_API_BEGIN
    MT2_REQUIRE(mcd_geometry_ok(n_mels, order), "n_mels outside [2, 128] or order outside [1, min(n_mels - 1, MT2_MCD_MAX_ORDER)]");
    MT2_REQUIRE(table != nullptr, "null table");
    mcd_table(n_mels, order, table);
    MT2_API_END
}

int mt2_mcd_query(int Ta_max, int Tb_max, int n_mels, int order, int B, long long* workspace_bytes) {
    MT2_API_BEGIN
    mcd_check_order(n_mels, order, B);
    mcd_check_max(Ta_max, "Ta_max outside [1, MT2_DTW_MAX_LEN]");
    mcd_check_max(Tb_max, "Tb_max outside [1, MT2_DTW_MAX_LEN]");
    if (workspace_bytes) *workspace_bytes = mcd_arena_bytes(Ta_max, Tb_max, order, B);
    MT2_API_END
}

// every refusal of the three calls is decided on the host before the first HIP call
int mt2_mel_cepstrum(mt2_model* m, void* stream, const float* mel, const int32_t* frame_lens, int T_max, int B, int n_mels, int order,
                     float* cep) {
    MT2_API_BEGIN
    mel_cepstrum_check(mel, frame_lens, T_max, B, n_mels, order, cep);
    MT2_AUDIO_CALL(m, stream);
    mel_cepstrum_run(c, mel, frame_lens, T_max, B, n_mels, order, cep);
    MT2_API_END
}

int mt2_path_distortion(mt2_model* m, void* stream, const float* ca, const int32_t* a_lens, int Ta_max, const float* cb,
                        const int32_t* b_lens, int Tb_max, int order, int B, const int32_t* lo, const int32_t* hi, const float* f0_a,
                        const float* f0_b, double* out) {
    MT2_API_BEGIN
    MT2_REQUIRE(B >= 1 && B <= 65535, "B outside [1, 65535]");
    MT2_REQUIRE(order >= 1 && order <= MT2_MCD_MAX_ORDER, "order outside [1, MT2_MCD_MAX_ORDER]");
    MT2_REQUIRE(lo != nullptr && hi != nullptr, "null lo / hi");
    mcd_check_pair(ca, a_lens, Ta_max, cb, b_lens, Tb_max, order, B, lo, hi, false, f0_a, f0_b, out);
    MT2_AUDIO_CALL(m, stream);
    path_distortion_run(c, ca, a_lens, Ta_max, cb, b_lens, Tb_max, order, B, lo, hi, f0_a, f0_b, out);
    MT2_API_END
}

int mt2_mel_cepstral_distortion(mt2_model* m, void* stream, const float* mel_a, const int32_t* a_lens, int Ta_max, const float* mel_b,
                                const int32_t* b_lens, int Tb_max, int n_mels, int order, int B, const float* f0_a, const float* f0_b,
                                double* out, int32_t* lo, int32_t* hi) {
    MT2_API_BEGIN
    mcd_check_order(n_mels, order, B);
    mcd_check_pair(mel_a, a_lens, Ta_max, mel_b, b_lens, Tb_max, n_mels, B, lo, hi, true, f0_a, f0_b, out);
    MT2_AUDIO_CALL(m, stream);
    mcd_run(c, mel_a, a_lens, Ta_max, mel_b, b_lens, Tb_max, n_mels, order, B, f0_a, f0_b, out, lo, hi);
    MT2_API_END
}

// stationary-noise suppression (denoise.hip): the arena bytes of one mt2_denoise call, its output length and the rank and factor of the
// longest utterance, without a HIP call
int mt2_denoise_query(const mt2_audio_config* ac, const mt2_denoise_config* dc, const int32_t* lens, int L_max, int B,
                      long long* workspace_bytes, long long* L_out, int* rank, float* factor) {
    MT2_API_BEGIN
    MT2_REQUIRE(ac != nullptr, "null audio configuration");
    const DnArgs a = denoise_check_config(dc);
    std::vector<int> T;
    const int T_cap = wave_frames(*ac, lens, L_max, B, T);
    if (workspace_bytes) *workspace_bytes = arena_bytes([&](ArenaCount& count, IntPlan& ip) { denoise_layout(count, ip, SpecGeom(*ac), lens, T, T_cap); });
    if (L_out) *L_out = (long long)(T_cap - 1) * ac->hop_length;
    if (rank) *rank = denoise_rank(T_cap, a.percentile);
    if (factor) *factor = a.c;
    MT2_API_END
}

// every refusal of the three calls is decided on the host before the first HIP call
int mt2_noise_floor(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_denoise_config* dc, const float* spec,
                    const int32_t* frame_lens, int T_max, int B, float* floor) {
    MT2_API_BEGIN
    const DnArgs a = denoise_check_config(dc);
    const int T_cap = denoise_check_spec(ac, spec, frame_lens, T_max, B);
    MT2_REQUIRE(floor != nullptr && ((uintptr_t)floor & 3) == 0, "bad floor");
    const size_t Fp = SpecGeom(*ac).Fp, lds = SpecGeom(*ac).lds;
    MT2_REQUIRE(!outputs_overlap({{floor, sizeof(float) * B * Fp}}, {{spec, sizeof(float) * (size_t)B * T_max * lds}}), "overlapping buffers");
    MT2_AUDIO_CALL(m, stream);
    noise_floor_run(c, *ac, a, spec, frame_lens, T_max, B, T_cap, floor);
    MT2_API_END
}

int mt2_spectral_gain(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_denoise_config* dc, const float* spec,
                      const int32_t* frame_lens, int T_max, int B, const float* floor, float* gain, float* spec_out) {
    MT2_API_BEGIN
    const DnArgs a = denoise_check_config(dc);
    const int T_cap = denoise_check_spec(ac, spec, frame_lens, T_max, B);
    MT2_REQUIRE(floor != nullptr && (gain != nullptr || spec_out != nullptr), "null floor, or neither output asked for");
    MT2_REQUIRE((((uintptr_t)floor | (uintptr_t)gain | (uintptr_t)spec_out) & 3) == 0, "misaligned buffers");
    const size_t Fp = SpecGeom(*ac).Fp, lds = SpecGeom(*ac).lds;
    const size_t ns = sizeof(float) * (size_t)B * T_max * lds, ng = sizeof(float) * (size_t)B * T_max * Fp, nf = sizeof(float) * B * Fp;
    MT2_REQUIRE(!outputs_overlap({{gain, ng}, {spec_out == spec ? nullptr : spec_out, ns}}, {{spec, ns}, {floor, nf}}), "overlapping buffers");
    MT2_AUDIO_CALL(m, stream);
    spectral_gain_run(c, *ac, a, spec, frame_lens, T_max, B, T_cap, floor, gain, spec_out);
    MT2_API_END
}

int mt2_denoise(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_denoise_config* dc, const float* wav, const int32_t* lens,
                int L_max, int B, const float* floor_in, float* floor_out, double* figures, float* out, int Lout_max) {
    MT2_API_BEGIN
    MT2_REQUIRE(ac != nullptr, "null audio configuration");
    const DnArgs a = denoise_check_config(dc);
    std::vector<int> T;
    const int T_cap = wave_check(*ac, wav, lens, L_max, B, floor_in, floor_out, figures, MT2_DENOISE_FIELDS, out, Lout_max, T);
    MT2_AUDIO_CALL(m, stream);
    denoise_run(c, *ac, a, wav, lens, L_max, B, T, T_cap, floor_in, floor_out, figures, out, Lout_max);
    MT2_API_END
}

// de-reverberation by weighted prediction error (wpe.hip): the arena bytes of one mt2_dereverb call and its output length, without a HIP
// call
int mt2_dereverb_query(const mt2_audio_config* ac, const mt2_wpe_config* wc, const int32_t* lens, int L_max, int B, long long* workspace_bytes,
                       long long* L_out) {
    MT2_API_BEGIN
    MT2_REQUIRE(ac != nullptr, "null audio configuration");
    const WpeArgs a = wpe_check_config(wc);
    std::vector<int> T;
    const int T_cap = wave_frames(*ac, lens, L_max, B, T);
    if (workspace_bytes) *workspace_bytes = arena_bytes([&](ArenaCount& count, IntPlan& ip) { dereverb_layout(count, ip, SpecGeom(*ac), a, lens, T, T_cap); });
    if (L_out) *L_out = (long long)(T_cap - 1) * ac->hop_length;
    MT2_API_END
}

// every refusal of the two calls is decided on the host before the first HIP call
int mt2_wpe_spectrum(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_wpe_config* wc, const float* spec,
                     const int32_t* frame_lens, int T_max, int B, float* spec_out, double* filters, double* figures) {
    MT2_API_BEGIN
    const WpeArgs a = wpe_check_config(wc);
    const int T_cap = denoise_check_spec(ac, spec, frame_lens, T_max, B);
    MT2_REQUIRE(spec_out != nullptr, "null spec_out");
    MT2_REQUIRE((((uintptr_t)spec | (uintptr_t)spec_out) & 15) == 0 && ((((uintptr_t)filters | (uintptr_t)figures) & 7) == 0),
                "misaligned buffers: the spectra on 16 bytes, the doubles on 8");
    const size_t F = SpecGeom(*ac).F, Fp = SpecGeom(*ac).Fp, lds = SpecGeom(*ac).lds;
    const size_t ns = sizeof(float) * (size_t)B * T_max * lds, nf = sizeof(double) * 2 * (size_t)B * Fp * a.taps,
                 ng = sizeof(double) * MT2_WPE_FIELDS * (size_t)B;
    MT2_REQUIRE(!outputs_overlap({{spec_out == spec ? nullptr : spec_out, ns}, {filters, nf}, {figures, ng}}, {{spec, ns}}), "overlapping buffers");
    {
        std::vector<int> c0;
        wpe_columns(std::vector<int>(frame_lens, frame_lens + B), (int)F, c0);
    }
    MT2_AUDIO_CALL(m, stream);
    wpe_spectrum_run(c, *ac, a, spec, frame_lens, T_max, B, T_cap, spec_out, filters, figures);
    MT2_API_END
}

int mt2_dereverb(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_wpe_config* wc, const float* wav, const int32_t* lens,
                 int L_max, int B, double* figures, float* out, int Lout_max) {
    MT2_API_BEGIN
    MT2_REQUIRE(ac != nullptr, "null audio configuration");
    const WpeArgs a = wpe_check_config(wc);
    std::vector<int> T;
    const int T_cap = wave_check(*ac, wav, lens, L_max, B, nullptr, nullptr, figures, MT2_WPE_FIELDS, out, Lout_max, T);
    MT2_AUDIO_CALL(m, stream);
    dereverb_run(c, *ac, a, wav, lens, L_max, B, T, T_cap, figures, out, Lout_max);
    MT2_API_END
}

// declipping by sparsity (declip.hip): the arena bytes of one mt2_declip and of one mt2_clip_detect call and the frames of the longest
// utterance, without a HIP call
int mt2_declip_query(const mt2_declip_config* dc, const int32_t* lens, int L_max, int B, long long* workspace_bytes, long long* detect_bytes,
                     long long* T_max) {
    MT2_API_BEGIN
    const DcArgs a = declip_check_config(dc);
    std::vector<int> len, T;
    declip_frames(a, lens, L_max, B, len, T);
    if (workspace_bytes) *workspace_bytes = declip_arena_bytes(a, T, true);
    if (detect_bytes) *detect_bytes = declip_arena_bytes(a, T, false);
    if (T_max) *T_max = *std::max_element(T.begin(), T.end());
    MT2_API_END
}

// every refusal of the two calls is decided on the host before the first HIP call
int mt2_clip_detect(mt2_model* m, void* stream, const mt2_declip_config* dc, const float* wav, const int32_t* lens, int L_max, int B,
                    double* figures) {
    MT2_API_BEGIN
    const DcCall k = declip_check(dc, wav, lens, L_max, B, nullptr, 0, figures, nullptr, 0, false);
    MT2_AUDIO_CALL(m, stream);
    declip_run(c, k, wav, L_max, B, nullptr, 0, figures, nullptr, 0);
    MT2_API_END
}

int mt2_declip(mt2_model* m, void* stream, const mt2_declip_config* dc, const float* wav, const int32_t* lens, int L_max, int B, float* out,
               int Lout_max, double* figures, int32_t* iters, int T_max) {
    MT2_API_BEGIN
    const DcCall k = declip_check(dc, wav, lens, L_max, B, out, Lout_max, figures, iters, T_max, true);
    MT2_AUDIO_CALL(m, stream);
    declip_run(c, k, wav, L_max, B, out, Lout_max, figures, iters, T_max);
    MT2_API_END
}

// speech segments by frame energy (segments.hip): the frames of the longest utterance, the f32 factor, the most segments one can have and
// the arena bytes of one mt2_speech_segments / mt2_cut_pauses call, without a HIP call
int mt2_segments_query(const mt2_segments_config* cfg, const int32_t* lens, int L_max, int B, int* frames, float* factor, long long* max_segments,
                       long long* workspace_bytes) {
    MT2_API_BEGIN
    SgCall k{};
    k.a = segments_check_config(cfg);
    segments_lens(k, lens, L_max, B);
    if (frames) *frames = k.max_F;
    if (factor) *factor = k.a.factor;
    if (max_segments) *max_segments = segments_bound(k.max_F, k.a.min_pause, k.a.min_speech);
    if (workspace_bytes) *workspace_bytes = segments_arena_bytes((size_t)B, segments_blocks(k.max_len), (size_t)k.max_F, true);
    MT2_API_END
}

// every refusal of the three calls is decided on the host before the first HIP call
int mt2_segment_frames(mt2_model* m, void* stream, const mt2_segments_config* cfg, const float* energy, const int32_t* frame_lens, int F_max, int B,
                       uint8_t* flags, int32_t* segments, int S_max, int32_t* counts, double* figures) {
    MT2_API_BEGIN
    const SgCall k = segment_frames_check(cfg, energy, frame_lens, F_max, B, flags, segments, S_max, counts, figures);
    MT2_AUDIO_CALL(m, stream);
    segment_frames_run(c, k, energy, F_max, B, flags, segments, S_max, counts, figures);
    MT2_API_END
}

int mt2_speech_segments(mt2_model* m, void* stream, const mt2_segments_config* cfg, const float* wav, const int32_t* lens, int L_max, int B,
                        int32_t* segments, int S_max, int32_t* counts, double* figures, float* energy, int F_max) {
    MT2_API_BEGIN
    const SgCall k = segments_check(cfg, wav, lens, L_max, B, nullptr, 0, false, segments, S_max, counts, figures, energy, F_max);
    MT2_AUDIO_CALL(m, stream);
    segments_run(c, k, wav, L_max, B, nullptr, 0, nullptr, segments, S_max, counts, figures, energy, F_max);
    MT2_API_END
}

int mt2_cut_pauses(mt2_model* m, void* stream, const mt2_segments_config* cfg, const float* wav, const int32_t* lens, int L_max, int B, float* out,
                   int Lout_max, int32_t* out_lens, int32_t* segments, int S_max, int32_t* counts, double* figures) {
    MT2_API_BEGIN
    const SgCall k = segments_check(cfg, wav, lens, L_max, B, out, Lout_max, true, segments, S_max, counts, figures, nullptr, 0);
    MT2_AUDIO_CALL(m, stream);
    segments_run(c, k, wav, L_max, B, out, Lout_max, out_lens, segments, S_max, counts, figures, nullptr, 0);
    MT2_API_END
}

// :361-368 [+370]  zq = vq.decode(p_codes) repeated x8, cat([tc_latent_expand, zq]), decoder, optional vocoder - the part of
// Megatts.forward behind the PLM, shared by mt2_synthesize_batch and mt2_synthesize_prompt_conditioned.  xdec: [D.R, H + Dq]
// rows whose first H columns already hold the length-regulated tc_latents.
static void decode_and_vocode(const Ctx& c, Stages& st, float* xdec, const FramePlan& fp, const IntPlan& ip, const int64_t* codes,
                              int flags, float* mel, int Tm_cap, float* wav, int B) {
    mt2_model* m = &c.m;
    const mt2_config& cfg = m->cfg;
    const int H = cfg.mrte_hidden, Dq = cfg.vq_dim, NM = cfg.mel_bins, DIN = H + Dq;
    MT2_HIP(launch_codebook_rows(m->codebook, codes, ip.dev(fp.o_codemap), xdec + H, DIN, Dq, fp.D.R, cfg.vq_bins, c.s));
    float* mrows = decoder_rows(c, xdec, fp.D);
    MT2_HIP(hipMemsetAsync(mel, 0, sizeof(float) * (size_t)B * Tm_cap * NM, c.s));
    MT2_HIP(launch_unpack_rows(mrows, NM, NM, Tm_cap, 0, ip.dev(fp.o_rowmapD), mel, fp.D.R, c.s));
    st.mark("decoder");
    if (flags & MT2_RUN_VOCODER) {   // :370  hifi_gan.decode_batch(x)
        MT2_REQUIRE(m->has_vocoder && wav != nullptr, "vocoder requested but not available");
        MT2_REQUIRE(cfg.hg_in_dim == NM, "vocoder input width differs from the mel width");
        const VocRows v = vocoder_rows(c, fp.D.off, fp.D.len.data(), B);
        float* xm = c.ws.get<float>((size_t)v.M0.R * NM);
        MT2_HIP(launch_gather_rows(mrows, NM, v.d_src, xm, NM, NM, v.M0.R, c.s));
        hifigan_to_wav(c, hifigan_rows(c, xm, v.M0), v.M0, wav, Tm_cap + 2 * cfg.hg_inference_padding);
        st.mark("vocoder");
    }
}

// :355  dt = adm.infer(tc_latent) on the first B row ranges of tc.P -> device durations [B, Np_max] (dur_out, or arena rows) ->
// the HOST durations everything behind the ADM is planned on: forced_dur where given, otherwise read back - the output length
// depends on them: one D2H + sync, as the reference (mrte.py:53).  The one seam between the ADM and the frame plan.
static const int32_t* adm_durations(const Ctx& c, Stages& st, const TcResult& tc, const int32_t* phone_lens, int Np_max, int B,
                                    bool run_adm, const int32_t* forced_dur, int32_t* dur_out, std::vector<int32_t>& dur_host) {
    int32_t* dur_dev = dur_out ? dur_out : c.ws.get<int32_t>((size_t)B * Np_max);
    if (run_adm) {
        MT2_HIP(hipMemsetAsync(dur_dev, 0, sizeof(int32_t) * (size_t)B * Np_max, c.s));
        adm_run(c, tc.rows, c.m.cfg.mrte_hidden, tc.P.R, tc.P.off, phone_lens, B, dur_dev, nullptr, Np_max);
    } else {
        MT2_REQUIRE(forced_dur != nullptr, "MT2_SKIP_ADM needs forced durations");
    }
    st.mark("adm");
    if (forced_dur) return forced_dur;
    dur_host.resize((size_t)B * Np_max);
    MT2_HIP(hipMemcpyAsync(dur_host.data(), dur_dev, dur_host.size() * sizeof(int32_t), hipMemcpyDeviceToHost, c.s));
    MT2_HIP(hipStreamSynchronize(c.s));
    return dur_host.data();
}
// the frame plan of the target utterances against the caller's capacities; publishes the mel lengths
static void check_frames(const FramePlan& fp, int B, int Tm_cap, int Tq_cap, int32_t* mel_lens) {
    MT2_REQUIRE(fp.D.maxlen <= Tm_cap, "Tm_cap smaller than the longest utterance");
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(fp.tq[b] <= Tq_cap, "Tq_cap smaller than the longest prosody sequence");
        MT2_REQUIRE(fp.D.len[b] >= 1, "utterance with zero frames");
        if (mel_lens) mel_lens[b] = fp.D.len[b];
    }
}
// where the PLM's codes go: the caller's codes_out [B, Tq_cap] or arena rows, zeroed
static int64_t* codes_buffer(const Ctx& c, int64_t* codes_out, int B, int Tq_cap) {
    int64_t* cdev = codes_out ? codes_out : c.ws.get<int64_t>((size_t)B * Tq_cap);
    MT2_HIP(hipMemsetAsync(cdev, 0, sizeof(int64_t) * (size_t)B * Tq_cap, c.s));
    return cdev;
}
// the caller's stream waits for the prompt VQ-PE of prompt_vqpe_side
static void join_vqpe_side(const Ctx& c) {
    MT2_HIP(hipStreamWaitEvent(c.s, c.m.ev_vq_join, 0));
    c.m.vq_forked = false;
}

// the optional VQProsodyEncoder.forward on the PROMPT mel on the handle's own stream (MT2_PROMPT_VQPE and the prompt-conditioned
// entry point): forked from the caller's stream here, joined by the caller of this function (ev_vq_join) or by CallScope
static void prompt_vqpe_side(const Ctx& c, const float* prompt_mel, const int32_t* prompt_lens, int Tp_max, int B,
                             int64_t* prompt_codes) {
    mt2_model* m = &c.m;
    const mt2_config& cfg = m->cfg;
    MT2_REQUIRE(prompt_codes != nullptr, "the prompt VQ-PE needs a prompt_codes output");
    if (!m->vq_stream) {
        MT2_HIP(hipStreamCreateWithFlags(&m->vq_stream, hipStreamNonBlocking));
        MT2_HIP(hipEventCreateWithFlags(&m->ev_vq_fork, hipEventDisableTiming));
        MT2_HIP(hipEventCreateWithFlags(&m->ev_vq_join, hipEventDisableTiming));
        MT2_HIP(hipEventCreate(&m->ev_vq_t0));
        MT2_HIP(hipEventCreate(&m->ev_vq_t1));
    }
    MT2_HIP(hipEventRecord(m->ev_vq_fork, c.s));
    m->vq_forked = true;
    MT2_HIP(hipStreamWaitEvent(m->vq_stream, m->ev_vq_fork, 0));
    const Ctx cv{*m, m->vq_stream, m->ws};
    const int Tqp = (Tp_max + cfg.vq_stride - 1) / cfg.vq_stride;
    if (m->profiling) MT2_HIP(hipEventRecord(m->ev_vq_t0, cv.s));
    if (m->opts.markers) MT2_HIP(launch_stage_marker(8, cv.s));
    IntPlan ipv;
    VqpeResult vr = vqpe_rows(cv, ipv, prompt_mel, cfg.mel_bins, prompt_lens, Tp_max, Tqp, B);
    MT2_HIP(hipMemsetAsync(prompt_codes, 0, sizeof(int64_t) * (size_t)B * Tqp, cv.s));
    MT2_HIP(launch_scatter_i64(vr.idx, ipv.dev(vr.o_rowmapQ), prompt_codes, vr.Q.R, cv.s));
    if (m->opts.markers) MT2_HIP(launch_stage_marker(9, cv.s));
    if (m->profiling) MT2_HIP(hipEventRecord(m->ev_vq_t1, cv.s));
    MT2_HIP(hipEventRecord(m->ev_vq_join, cv.s));
}

// ---------------------------------------------------------------------------------------------------
// Megatts.forward's no_grad block (models/megatts2.py:353-368 [+370]) on a batch
int mt2_synthesize_batch_sampled(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens, int Np_max,
                                 const float* prompt_mel, const int32_t* prompt_lens, int Tp_max, int B,
                                 const int32_t* forced_dur, const int64_t* forced_codes, int Tq_cap, int flags, float* mel,
                                 int Tm_cap, int32_t* mel_lens, int32_t* dur_out, int64_t* codes_out, float* wav,
                                 int64_t* prompt_codes, const mt2_sampling* sampling) {
    MT2_API_BEGIN
    require_ready(m, NEED_G);
    MT2_REQUIRE(B >= 1, "empty batch");
    if (sampling) check_sampling(*sampling, m->cfg.plm_bins, true);
    MT2_CALL(m, stream);
    const mt2_config& cfg = m->cfg;
    const int H = cfg.mrte_hidden, Dq = cfg.vq_dim;
    if (!(flags & MT2_SKIP_ADM)) {
        require_ready(m, NEED_ADM);
        MT2_REQUIRE(cfg.adm_tc_dim == H, "ADM tc_latent_dim differs from the MRTE hidden size");
    }
    if (!forced_codes) {
        require_ready(m, NEED_PLM);
        MT2_REQUIRE(cfg.plm_tc_dim == H, "PLM tc_latent_dim differs from the MRTE hidden size");
        MT2_REQUIRE(cfg.plm_bins == cfg.vq_bins, "PLM vq_bins differs from the generator's codebook size");
    }
    Stages st(*m, c.s);
    st.mark("start");
    // caller-supplied gather indices (phone ids here, forced codes once their extent is known) are range-checked on the
    // handle's id stream; the gathers clamp, the verdict is read at the end of the call (model_stages.hip, ids_check)
    // :354  tc_latent = generator.mrte.tc_latent(phone_tokens, mels)
    TcResult tc = tc_latent_rows(c, phone, phone_lens, Np_max, prompt_mel, prompt_lens, Tp_max, B);
    st.mark("mrte");
    // optional (MT2_PROMPT_VQPE): VQProsodyEncoder.forward on the PROMPT mel (modules/vqpe.py:50-62) - the prosody codes
    // a prompt-conditioned PLM (datamodule.py:201-212) or stage-2 extraction (prepare_ds.py:224-258) consume.  It does
    // not depend on anything else of the call: it runs on its own internal stream from here on, filling the CUs the
    // ADM's latency-bound step launches leave idle, and joins back before the call ends.
    const bool vq_side = (flags & MT2_PROMPT_VQPE) != 0;
    if (vq_side) prompt_vqpe_side(c, prompt_mel, prompt_lens, Tp_max, B, prompt_codes);
    std::vector<int32_t> dur_host;
    const int32_t* dur = adm_durations(c, st, tc, phone_lens, Np_max, B, !(flags & MT2_SKIP_ADM), forced_dur, dur_out, dur_host);
    // :356-358  length regulation (gather) and max_pool1d(8, ceil) conditioning
    IntPlan ip;
    FramePlan fp = plan_frames(ip, cfg, dur, Np_max, phone_lens, B, tc.P.off, cfg.vq_stride, Tq_cap, Tm_cap);
    check_frames(fp, B, Tm_cap, Tq_cap, mel_lens);
    ip.upload(c.ws, c.m.pinned(), c.s);
    bind_rows(ip, fp.oD, fp.D);
    if (forced_codes) {      // only the positions the decoder will read: q < ceil(frames / 8) of each utterance
        std::vector<int> cmap;
        for (int b = 0; b < B; ++b)
            for (int q = 0; q < fp.tq[b]; ++q) cmap.push_back(b * Tq_cap + q);
        ids_check(c, forced_codes, &cmap, (long long)cmap.size(), cfg.vq_bins, ID_CODE);
    }
    const int DIN = H + Dq;
    float* xdec = c.ws.get<float>((size_t)fp.D.R * DIN);
    MT2_HIP(launch_gather_rows(tc.rows, H, ip.dev(fp.o_tcmap), xdec, DIN, H, fp.D.R, c.s));
    float* cond = c.ws.get<float>((size_t)std::max(fp.Qrows, 1) * H);
    MT2_HIP(launch_pool_max(xdec, DIN, ip.dev(fp.o_first), ip.dev(fp.o_cnt), cond, H, H, fp.Qrows, c.s));
    st.mark("regulate");
    // :359  p_codes = plm.infer(tc_latent)
    const int64_t* codes = forced_codes;
    if (!codes) {
        MT2_REQUIRE(flags & MT2_RUN_PLM, "neither forced codes nor MT2_RUN_PLM given");
        int64_t* cdev = codes_buffer(c, codes_out, B, Tq_cap);
        plm_run(c, cond, H, fp.q_row0, fp.tq.data(), B, cdev, Tq_cap, nullptr, 0, ArPrefix(), sampling);
        codes = cdev;
    } else if (codes_out && codes_out != forced_codes) {
        MT2_HIP(hipMemcpyAsync(codes_out, forced_codes, sizeof(int64_t) * (size_t)B * Tq_cap,
                               hipMemcpyDeviceToDevice, c.s));
    }
    st.mark("plm");
    decode_and_vocode(c, st, xdec, fp, ip, codes, flags, mel, Tm_cap, wav, B);
    if (vq_side) join_vqpe_side(c);                                       // the side stream joins before the call ends
    st.finish();
    ids_verdict(c);
    if (vq_side && m->profiling) {      // its own (overlapped) duration on the side stream
        float ms = 0.f;
        MT2_HIP(hipEventSynchronize(m->ev_vq_t1));
        MT2_HIP(hipEventElapsedTime(&ms, m->ev_vq_t0, m->ev_vq_t1));
        m->stage_names.push_back("vqpe_side");
        m->stage_ms.push_back(ms);
    }
    MT2_API_END
}
int mt2_synthesize_batch(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens, int Np_max,
                         const float* prompt_mel, const int32_t* prompt_lens, int Tp_max, int B,
                         const int32_t* forced_dur, const int64_t* forced_codes, int Tq_cap, int flags, float* mel,
                         int Tm_cap, int32_t* mel_lens, int32_t* dur_out, int64_t* codes_out, float* wav,
                         int64_t* prompt_codes) {
    return mt2_synthesize_batch_sampled(m, stream, phone, phone_lens, Np_max, prompt_mel, prompt_lens, Tp_max, B, forced_dur,
                                        forced_codes, Tq_cap, flags, mel, Tm_cap, mel_lens, dur_out, codes_out, wav,
                                        prompt_codes, nullptr);
}

// ---------------------------------------------------------------------------------------------------
// Prompt-conditioned synthesis as ONE call (SURVEY 8f row f1): the layout the PLM is trained on (modules/datamodule.py:161-177,
// 196-212) at inference - the prompt's length-regulated, max-pooled tc_latents in front of the target's, the prompt's VQ-PE
// codes behind the BOS, greedy decoding from there, then Megatts.forward's decoder (+ vocoder).  One mel-encoder pass serves
// the prompt's and the target's tc_latent (the mel context is shared; only the phone branch differs: both phone sets run
// through the phone encoder as one batch of 2 B sequences); the prompt's VQ-PE runs on the handle's side stream beside the
// ADM; nothing leaves the device between the stages except the durations (one D2H, as in the reference).
int mt2_synthesize_prompt_conditioned_sampled(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens,
                                              int Np_max, const float* prompt_mel, const int32_t* prompt_lens, int Tp_max, int B,
                                              const int64_t* prompt_phone, const int32_t* prompt_phone_lens, int Npp_max,
                                              const int32_t* prompt_dur, const int32_t* forced_dur, int Tq_cap, int flags,
                                              float* mel, int Tm_cap, int32_t* mel_lens, int32_t* dur_out, int64_t* codes_out,
                                              float* wav, int64_t* prompt_codes, const mt2_sampling* sampling) {
    MT2_API_BEGIN
    require_ready(m, NEED_G | NEED_ADM | NEED_PLM);
    MT2_REQUIRE(B >= 1 && prompt_phone && prompt_phone_lens && prompt_dur && prompt_codes, "bad arguments");
    if (sampling) check_sampling(*sampling, m->cfg.plm_bins, true);
    MT2_CALL(m, stream);
    const mt2_config& cfg = m->cfg;
    const int H = cfg.mrte_hidden, Dq = cfg.vq_dim, pool = cfg.vq_stride;
    MT2_REQUIRE(cfg.adm_tc_dim == H && cfg.plm_tc_dim == H, "ADM / PLM tc_latent_dim differs from the MRTE hidden size");
    MT2_REQUIRE(cfg.plm_bins == cfg.vq_bins, "PLM vq_bins differs from the generator's codebook size");
    // the prompt's alignment covers the prompt mel exactly (datamodule.py:198 assert) and all prompts pool to ONE prefix
    // length P (pad-free prefix layout)
    const int P = (prompt_lens[0] + pool - 1) / pool;
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(prompt_phone_lens[b] >= 1 && prompt_phone_lens[b] <= Npp_max, "prompt phone length out of range");
        long long sum = 0;
        for (int i = 0; i < prompt_phone_lens[b]; ++i) sum += prompt_dur[(size_t)b * Npp_max + i];
        MT2_REQUIRE(sum == prompt_lens[b], "prompt durations must sum to the prompt's mel frames");
        MT2_REQUIRE((prompt_lens[b] + pool - 1) / pool == P, "prompt-conditioned batches need prompts of one pooled length");
    }
    Stages st(*m, c.s);
    st.mark("start");
    // :354  tc_latent of the target's phones AND of the prompt's own phones from one mel-encoder pass
    TcResult tc = tc_latent_rows(c, std::vector<PhoneSet>{{phone, phone_lens, Np_max}, {prompt_phone, prompt_phone_lens, Npp_max}},
                                 prompt_mel, prompt_lens, Tp_max, B);
    st.mark("mrte");
    prompt_vqpe_side(c, prompt_mel, prompt_lens, Tp_max, B, prompt_codes);      // side stream, beside the ADM
    std::vector<int32_t> dur_host;      // (the target sequences are the first B row ranges of tc.P)
    const int32_t* dur = adm_durations(c, st, tc, phone_lens, Np_max, B, true, forced_dur, dur_out, dur_host);
    // :356-358 for both sides: length regulation (gather) into ONE row buffer [prompt frames | target frames], then ONE
    // ceil-mode max-pool launch that writes the PLM conditioning of utterance b as [P prompt rows | tq[b] target rows]
    IntPlan ip;
    FramePlan fp = plan_frames(ip, cfg, dur, Np_max, phone_lens, B, tc.P.off, pool, Tq_cap, Tm_cap);
    std::vector<int> prow0(tc.P.off.begin() + B, tc.P.off.end());
    FramePlan pp = plan_frames(ip, cfg, prompt_dur, Npp_max, prompt_phone_lens, B, prow0, pool, 0, 0);
    check_frames(fp, B, Tm_cap, Tq_cap, mel_lens);
    std::vector<int> total(B), q0(B);
    int qr = 0;
    for (int b = 0; b < B; ++b) {
        MT2_REQUIRE(pp.tq[b] == P, "prompt alignment does not pool to the prefix length");
        q0[b] = qr;
        total[b] = P + fp.tq[b];
        qr += total[b];
    }
    std::vector<int> first(qr, 0), cnt(qr, 0);
    for (int b = 0; b < B; ++b) {
        for (int q = 0; q < P; ++q) {
            first[q0[b] + q] = pp.D.off[b] + q * pool;
            cnt[q0[b] + q] = std::min(pool, pp.D.len[b] - q * pool);
        }
        for (int q = 0; q < fp.tq[b]; ++q) {
            first[q0[b] + P + q] = pp.D.R + fp.D.off[b] + q * pool;
            cnt[q0[b] + P + q] = std::min(pool, fp.D.len[b] - q * pool);
        }
    }
    const int o_first = ip.add(first), o_cnt = ip.add(cnt);
    ip.upload(c.ws, c.m.pinned(), c.s);
    bind_rows(ip, fp.oD, fp.D);
    const int DIN = H + Dq;
    float* rows = c.ws.get<float>((size_t)(pp.D.R + fp.D.R) * DIN);
    float* xdec = rows + (size_t)pp.D.R * DIN;
    MT2_HIP(launch_gather_rows(tc.rows, H, ip.dev(pp.o_tcmap), rows, DIN, H, pp.D.R, c.s));
    MT2_HIP(launch_gather_rows(tc.rows, H, ip.dev(fp.o_tcmap), xdec, DIN, H, fp.D.R, c.s));
    float* cond = c.ws.get<float>((size_t)qr * H);
    MT2_HIP(launch_pool_max(rows, DIN, ip.dev(o_first), ip.dev(o_cnt), cond, H, H, qr, c.s));
    st.mark("regulate");
    // :359  p_codes = plm.infer(...) continued from the prompt's codes: they come from the side stream
    join_vqpe_side(c);
    int64_t* cdev = codes_buffer(c, codes_out, B, Tq_cap);
    ArPrefix pre;
    pre.P = P; pre.data = prompt_codes; pre.stride = (Tp_max + pool - 1) / pool;
    plm_run(c, cond, H, q0, total.data(), B, cdev, Tq_cap, nullptr, 0, pre, sampling);
    st.mark("plm");
    decode_and_vocode(c, st, xdec, fp, ip, cdev, flags, mel, Tm_cap, wav, B);
    st.finish();
    MT2_API_END
}
int mt2_synthesize_prompt_conditioned(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens, int Np_max,
                                      const float* prompt_mel, const int32_t* prompt_lens, int Tp_max, int B,
                                      const int64_t* prompt_phone, const int32_t* prompt_phone_lens, int Npp_max,
                                      const int32_t* prompt_dur, const int32_t* forced_dur, int Tq_cap, int flags, float* mel,
                                      int Tm_cap, int32_t* mel_lens, int32_t* dur_out, int64_t* codes_out, float* wav,
                                      int64_t* prompt_codes) {
    return mt2_synthesize_prompt_conditioned_sampled(m, stream, phone, phone_lens, Np_max, prompt_mel, prompt_lens, Tp_max, B,
                                                     prompt_phone, prompt_phone_lens, Npp_max, prompt_dur, forced_dur, Tq_cap,
                                                     flags, mel, Tm_cap, mel_lens, dur_out, codes_out, wav, prompt_codes,
                                                     nullptr);
}

// ---------------------------------------------------------------------------------------------------
// kernel-level entry points (parity tests, micro-benchmarks)

int mt2_gemm_trace_begin(mt2_model* m) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr, "null model handle");
    std::lock_guard<std::mutex> lk(m->call_mutex);
    for (auto& r : m->opts.trace) { (void)hipEventDestroy(r.e0); (void)hipEventDestroy(r.e1); }
    m->opts.trace.clear();
    m->opts.trace_on = true;
    MT2_API_END
}
int mt2_gemm_trace_end(mt2_model* m, int cap, const char** names, int64_t* launches, double* flops, double* ms) {
    if (!m) return -1;
    std::lock_guard<std::mutex> lk(m->call_mutex);
    return gemm_trace_collect(m->opts, cap, names, launches, flops, ms);
}
int mt2_gemm_trace_shapes(mt2_model* m, char* buf, int cap, int top) {
    if (!m || !buf || cap <= 0) return -1;
    std::lock_guard<std::mutex> lk(m->call_mutex);
    return gemm_trace_shapes(m->opts, buf, cap, top);
}
// Form log of the AR step wiring, the vocoder wiring and the parallel stages - MRTE mel encoder, phone encoder and cross attention, VQ
// prosody encoder, mel decoder - (mt2_model::form_log; written by form_note in model_stages.hip): host-side text only
int mt2_form_log_begin(mt2_model* m) {
    MT2_API_BEGIN
    MT2_REQUIRE(m != nullptr, "null model handle");
    std::lock_guard<std::mutex> lk(m->call_mutex);
    m->form_log.clear();
    m->form_kind = nullptr;
    m->form_log_on = true;
    MT2_API_END
}
int mt2_form_log_end(mt2_model* m, char* buf, int cap) {
    if (!m || !buf || cap <= 0) return -1;
    std::lock_guard<std::mutex> lk(m->call_mutex);
    m->form_log_on = false;
    m->form_kind = nullptr;
    size_t need = 0;
    for (const std::string& l : m->form_log) need += l.size() + 1;
    int off = -1;
    if (need < (size_t)cap) {
        off = 0;
        for (const std::string& l : m->form_log) {
            std::memcpy(buf + off, l.data(), l.size());
            off += (int)l.size();
            buf[off++] = '\n';
        }
        buf[off] = 0;
    }
    m->form_log.clear();
    m->form_log.shrink_to_fit();
    return off;
}
int mt2_gemm_config_count(void) { return gemm_num_configs(); }
const char* mt2_gemm_config_name(int idx) { return gemm_config_name(idx); }

// What launch_gemm would do with a launch, without making it (gemm_route; no device needed - the routing tests).  The launch is the
// dense one of mt2_bench_gemm: Cin = K / taps, ldx = Cin, ldw = K, ldc = ldr = N, Rx = M + taps * dil, groups laid out back to back.
// `operands`: which optional operands exist (dummy pointers, never dereferenced) - 1 W3, 2 Wh + wh_inv, 4 Wtm, 8 stat_out, 16 ln_stat
// (with ln_g / ln_b and pairs of 64 columns), 32 R, 64 rowbase, 128 a_planes, 256 c_planes.  Every pointer sits on 128 bytes except
// those whose bit is set in `misaligned` (same bits; 512: X, 1024: C), which sit 4 bytes further.  variant: GemmVariant; planes: bit 0
// gemm_takes_planes, bit 1 gemm_writes_planes for the same launch.
// mt2_gemm_route_ex: the same launch with the rows of C and R ld_pad floats apart beyond N and the option ks_epi4 as given; *epi4 = 1
// when an x3h K-split tile would finish it with 16-byte loads and stores (GemmRoute::ks_epi4).
int mt2_gemm_route(int M, int N, int K, int taps, int dil, int groups, int pro_act, int operands, int misaligned, int force_cfg,
                   int x3h, int* err, int* cfg, int* variant, long long* lds, int* planes) {
    return mt2_gemm_route_ex(M, N, K, taps, dil, groups, pro_act, operands, misaligned, force_cfg, x3h, 0, 1, err, cfg, variant, lds,
                             planes, nullptr);
}
int mt2_gemm_route_ex(int M, int N, int K, int taps, int dil, int groups, int pro_act, int operands, int misaligned, int force_cfg,
                      int x3h, int ld_pad, int ks_epi4, int* err, int* cfg, int* variant, long long* lds, int* planes, int* epi4) {
    alignas(128) static char dummy[12 * 128];
    const auto ptr = [&](int slot, int bit) { return (void*)(dummy + 128 * slot + ((misaligned & bit) ? 4 : 0)); };
    GemmP p{};
    const int Cin = taps > 0 ? K / taps : K;
    p.X = (const float*)ptr(0, 512); p.ldx = Cin; p.Rx = M + taps * dil; p.a_mul = 1; p.taps = taps; p.dil = dil; p.Cin = Cin;
    p.W = (const float*)ptr(1, 0); p.ldw = K; p.C = (float*)ptr(2, 1024); p.ldc = N; p.M = M; p.N = N; p.K = K; p.groups = groups;
    p.strideX = (long long)p.Rx * Cin; p.strideW = (long long)N * K; p.strideC = (long long)M * N; p.strideB = N; p.strideR = (long long)M * N;
    p.pro_act = pro_act; p.out_scale = 1.0f;
    if (operands & 1) p.W3 = ptr(3, 1);
    if (operands & 2) { p.Wh = ptr(4, 2); p.wh_inv = (const float*)ptr(5, 0); }
    if (operands & 4) { p.Wtm = (const float*)ptr(6, 4); p.tm_kb = K / 64; }
    if (operands & 8) p.stat_out = (float*)ptr(7, 8);
    if (operands & 16) { p.ln_stat = (const float*)ptr(8, 16); p.ln_g = p.ln_b = (const float*)ptr(9, 0); p.ln_w = 64; p.ln_nt = K / 64; }
    if (operands & 32) { p.R = (const float*)ptr(10, 32); p.ldr = N; }
    if (operands & 64) p.rowbase = (const int*)ptr(11, 64);
    p.a_planes = (operands & 128) ? 1 : 0;
    p.c_planes = (operands & 256) ? 1 : 0;
    p.ldc += ld_pad;
    if (p.R) p.ldr += ld_pad;
    p.strideC = (long long)M * p.ldc; p.strideR = (long long)M * p.ldc;
    EngineOpts o;
    o.force_cfg = force_cfg;
    o.x3h = x3h;
    o.ks_epi4 = ks_epi4;
    const GemmRoute r = gemm_route(p, o);
    if (epi4) *epi4 = r.ks_epi4;
    if (err) *err = (int)r.err;
    if (cfg) *cfg = r.cfg;
    if (variant) *variant = r.variant;
    if (lds) *lds = (long long)r.lds;
    if (planes) *planes = (gemm_takes_planes(p, o) ? 1 : 0) | (gemm_writes_planes(p, o) ? 2 : 0);
    return 0;
}

// What launch_conv_pair would do with a resblock conv pair, without making it (conv_pair_route; no device needed).  Dense rows (ldx = ldy
// = C), dummy pointers that are never dereferenced.  flags: 1 reflect padding, 2 no fp16 planes, 4 R is taken as the row count of an
// operand of 2 GiB (ldx = 2^31 / (4 R) rounded up), 8 the output sits 4 bytes off its alignment.
int mt2_conv_pair_route(int R, int C, int taps, int dil, int flags, int pair_fuse, int x3h, int* err, long long* lds, int* grid,
                        int* block, int* bm, int* bmo) {
    alignas(128) static char dummy[8 * 128];
    PairP p{};
    p.X = (const float*)dummy; p.ldx = C; p.R = R; p.C = C; p.taps = taps; p.dil = dil; p.slope = 0.1f;
    if (!(flags & 2)) { p.Wh1 = dummy + 128; p.inv1 = (const float*)(dummy + 256); p.Wh2 = dummy + 384; p.inv2 = (const float*)(dummy + 512); }
    p.bias1 = (const float*)(dummy + 640); p.bias2 = (const float*)(dummy + 768);
    p.wh_ldb = 4ll * (((long long)taps * C + 31) / 32 * 32);
    p.Y = (float*)(dummy + 896 + ((flags & 8) ? 4 : 0)); p.ldy = C;
    p.reflect = (flags & 1) ? 1 : 0;
    if ((flags & 4) && R > 0) p.ldx = (int)((((1ll << 31) / 4 + R - 1) / R + 3) & ~3ll);
    EngineOpts o;
    o.pair_fuse = pair_fuse;
    o.x3h = x3h;
    const PairRoute r = conv_pair_route(p, o);
    if (err) *err = (int)r.err;
    if (lds) *lds = (long long)r.lds;
    if (grid) *grid = (int)r.grid;
    if (block) *block = (int)r.block;
    if (bm) *bm = r.bm;
    if (bmo) *bmo = r.bmo;
    return 0;
}
// Kernel test of the fused pair: one launch_conv_pair with the per-call EngineOpts of mt2_op_gemm (pair_fuse: the mask)
int mt2_op_conv_pair(void* stream, const float* X, int ldx, int R, int C, int taps, int dil, float slope, const void* Wh1,
                     const float* inv1, const float* bias1, const void* Wh2, const float* inv2, const float* bias2,
                     const int32_t* valid, float* Y, int ldy, int pair_fuse, int32_t* range_flag) {
    MT2_API_BEGIN
    PairP p{};
    p.X = X; p.ldx = ldx; p.R = R; p.C = C; p.taps = taps; p.dil = dil; p.slope = slope;
    p.Wh1 = Wh1; p.inv1 = inv1; p.bias1 = bias1; p.Wh2 = Wh2; p.inv2 = inv2; p.bias2 = bias2;
    p.wh_ldb = 4ll * (((long long)taps * C + 31) / 32 * 32);
    p.valid = valid; p.Y = Y; p.ldy = ldy;
    EngineOpts o;
    o.pair_fuse = pair_fuse;
    o.x3h_flag = range_flag;
    MT2_HIP(launch_conv_pair(p, (hipStream_t)stream, &o));
    MT2_API_END
}

// What launch_up_mrf would do with a fused MRF mean + stride-`stride` upsampler of `ch` input channels over R rows, without making it
// (up_mrf_route; no device needed).  Dense rows (ldx = ldy = ch), dummy pointers that are never dereferenced.  flags: 1 no fp16 planes,
// 2 R is taken as the row count of an operand of 2 GiB (ldx = 2^31 / (4 R) rounded up), 4 the output sits 4 bytes off its alignment,
// 8 the planes sit 16 bytes off theirs, 16 ldx = ch + 2 (no multiple of 4), 32 X1 is null, 64 ldy = ch - 4 (below the width),
// 128 the bias sits 4 bytes off its alignment.  off: engine options switched away from their defaults - 1 win_conv off, 2 x6_conv off,
// 4 a forced configuration, 8 ldr64.
int mt2_up_mrf_route(int R, int ch, int stride, int flags, int up_fuse, int x3h, int off, int* err, long long* lds, int* grid, int* block,
                     int* bm) {
    alignas(128) static char dummy[8 * 128];
    UpMrfP p{};
    p.X0 = (const float*)dummy; p.X1 = (flags & 32) ? nullptr : (const float*)(dummy + 128); p.X2 = (const float*)(dummy + 256);
    p.ldx = ch; p.R = R; p.ch = ch; p.stride = stride; p.scale = 1.0f / 3.0f; p.slope = 0.1f;
    if (!(flags & 1)) { p.Wh = dummy + 384 + ((flags & 8) ? 16 : 0); p.inv = (const float*)(dummy + 512); }
    p.bias = (const float*)(dummy + 640 + ((flags & 128) ? 4 : 0));
    p.wh_ldb = 8ll * ch;
    p.Y = (float*)(dummy + 768 + ((flags & 4) ? 4 : 0)); p.ldy = ch;
    if ((flags & 2) && R > 0) p.ldx = (int)((((1ll << 31) / 4 + R - 1) / R + 3) & ~3ll);
    if (flags & 16) p.ldx = ch + 2;
    if (flags & 64) p.ldy = ch - 4;
    EngineOpts o;
    o.up_fuse = up_fuse;
    o.x3h = x3h;
    if (off & 1) o.win_conv = false;
    if (off & 2) o.x6_conv = false;
    if (off & 4) o.force_cfg = 0;
    if (off & 8) o.ldr64 = true;
    const UpMrfRoute r = up_mrf_route(p, o);
    if (err) *err = (int)r.err;
    if (lds) *lds = (long long)r.lds;
    if (grid) *grid = (int)r.grid;
    if (block) *block = (int)r.block;
    if (bm) *bm = r.bm;
    return 0;
}
// Kernel test of the fused MRF mean + upsampler: one launch_up_mrf with per-call EngineOpts (up_fuse: the mask)
int mt2_op_up_mrf(void* stream, const float* X0, const float* X1, const float* X2, int ldx, int R, int ch, float scale, float slope,
                  const void* Wh, const float* inv, const float* bias, const int32_t* valid, float* Y, int ldy, int up_fuse,
                  int32_t* range_flag) {
    MT2_API_BEGIN
    UpMrfP p{};
    p.X0 = X0; p.X1 = X1; p.X2 = X2; p.ldx = ldx; p.R = R; p.ch = ch; p.stride = 2; p.scale = scale; p.slope = slope;
    p.Wh = Wh; p.inv = inv; p.bias = bias; p.wh_ldb = 8ll * ch;
    p.valid = valid; p.Y = Y; p.ldy = ldy;
    EngineOpts o;
    o.up_fuse = up_fuse;
    o.x3h_flag = range_flag;
    MT2_HIP(launch_up_mrf(p, (hipStream_t)stream, &o));
    MT2_API_END
}

int mt2_op_gemm(void* stream, const float* X, int ldx, int Rx, const int32_t* rowbase, int a_mul, int shift0,
                int taps, int dil, int Cin, const float* W, int ldw, const float* bias, const float* R, int ldr,
                const int32_t* valid, float* C, int ldc, int M, int N, int pro_act, float pro_slope, int epi_act,
                float out_scale, int force_cfg) {
    MT2_API_BEGIN
    GemmP p{};
    p.X = X; p.ldx = ldx; p.Rx = Rx; p.rowbase = rowbase; p.a_mul = a_mul ? a_mul : 1; p.shift0 = shift0;
    p.taps = taps; p.dil = dil; p.Cin = Cin; p.W = W; p.ldw = ldw; p.bias = bias; p.R = R; p.ldr = ldr;
    p.valid = valid; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = taps * Cin; p.groups = 1;
    p.pro_act = pro_act; p.pro_slope = pro_slope; p.epi_act = epi_act; p.out_scale = out_scale;
    EngineOpts o;            // per call: no state is shared with any handle or thread
    o.force_cfg = force_cfg;
    MT2_HIP(launch_gemm(p, (hipStream_t)stream, &o));
    MT2_API_END
}

// The same with the weights ALSO given as three bf16 planes W3 [3][N][K] (device, uint16): window convolutions may
// then run on the bf16 matrix pipe (f32-equivalent 6-product form; force_cfg 34 / 58 / 59 or -1).
int mt2_op_gemm_x6(void* stream, const float* X, int ldx, int Rx, int shift0, int taps, int dil, int Cin, const float* W,
                   const void* W3, const float* bias, const float* R, int ldr, const int32_t* valid, float* C, int ldc,
                   int M, int N, int pro_act, float pro_slope, int epi_act, int force_cfg) {
    MT2_API_BEGIN
    GemmP p{};
    p.X = X; p.ldx = ldx; p.Rx = Rx; p.a_mul = 1; p.shift0 = shift0; p.taps = taps; p.dil = dil; p.Cin = Cin; p.W = W;
    p.W3 = W3; p.ldw = taps * Cin; p.bias = bias; p.R = R; p.ldr = ldr; p.valid = valid; p.C = C; p.ldc = ldc; p.M = M;
    p.N = N; p.K = taps * Cin; p.groups = 1; p.pro_act = pro_act; p.pro_slope = pro_slope; p.epi_act = epi_act;
    p.out_scale = 1.0f;
    EngineOpts o;
    o.force_cfg = force_cfg;
    MT2_HIP(launch_gemm(p, (hipStream_t)stream, &o));
    MT2_API_END
}

// ... and ALSO as two fp16 planes of the row-scaled matrix in the chunk-interleaved layout of x3h_planes.h (Wh: [N][ceil32(K) / 32]
// blocks of 128 bytes, [hi | lo]) with the inverse row scales wh_inv [N]: the fp16-pipe tiles (three products; force_cfg 103, 95..100 or -1).  range_flag: device int32, |= 1 when an activation left the fp16 range.
int mt2_op_gemm_x3h(void* stream, const float* X, int ldx, int Rx, int shift0, int taps, int dil, int Cin, const float* W,
                    const void* W3, const void* Wh, const float* wh_inv, const float* bias, const float* R, int ldr,
                    const int32_t* valid, float* C, int ldc, int M, int N, int pro_act, float pro_slope, int epi_act, int force_cfg,
                    int32_t* range_flag) {
    MT2_API_BEGIN
    GemmP p{};
    p.X = X; p.ldx = ldx; p.Rx = Rx; p.a_mul = 1; p.shift0 = shift0; p.taps = taps; p.dil = dil; p.Cin = Cin; p.W = W;
    p.W3 = W3; p.Wh = Wh; p.wh_inv = wh_inv; p.ldw = taps * Cin; p.bias = bias; p.R = R; p.ldr = ldr; p.valid = valid; p.C = C;
    p.ldc = ldc; p.M = M; p.N = N; p.K = taps * Cin; p.groups = 1; p.pro_act = pro_act; p.pro_slope = pro_slope; p.epi_act = epi_act;
    p.out_scale = 1.0f;
    EngineOpts o;
    if (force_cfg >= 8000) { o.ks_epi4 = 0; force_cfg -= 8000; }        // tests: configuration + 8000 = the K-split tiles' dword finish (option ks_epi4 = 0)
    if (force_cfg >= 4000) { p.c_planes = 1; force_cfg -= 4000; }       // tests: configuration + 4000 = C receives fp16 planes (GemmP::c_planes)
    if (force_cfg >= 2000) { p.a_planes = 1; force_cfg -= 2000; }       // tests: configuration + 2000 = X holds fp16 planes (GemmP::a_planes)
    o.ldr64 = force_cfg >= 1000;            // tests: configuration + 1000 = the same launch with the loaders' 64-bit address form
    o.force_cfg = force_cfg >= 1000 ? force_cfg - 1000 : force_cfg;
    o.x3h_flag = range_flag;
    MT2_HIP(launch_gemm(p, (hipStream_t)stream, &o));
    MT2_API_END
}
// host helper: the x3h operand format of a row-major [rows, row_len] f32 matrix (x3h_planes.h) - planes [rows][2 * ceil32(row_len)]
// uint16 (per row and 32-k chunk: 32 hi, then 32 lo), inv [rows]
int mt2_x3h_split(const float* W, long long rows, long long row_len, uint16_t* planes, float* inv) {
    MT2_API_BEGIN
    MT2_REQUIRE(W && planes && inv && rows > 0 && row_len > 0, "bad arguments");
    x3h_split_rows(W, (size_t)rows, (size_t)row_len, planes, inv);
    MT2_API_END
}
// host helper: the plane-stride rule of the model's launches (x3h_planes.h, x3h_group_planes; model_stages.hip attach_planes calls the same function)
int mt2_x3h_group_planes(long long row_len, long long w_off, long long ldw, long long strideW, long long groups, int32_t* form,
                         long long* wh_off, long long* wh_ldb, long long* wh_gstride, long long* inv_off, long long* wh_inv_stride) {
    MT2_API_BEGIN
    MT2_REQUIRE(row_len > 0 && w_off >= 0 && groups >= 1 && form && wh_off && wh_ldb && wh_gstride && inv_off && wh_inv_stride,
                "bad arguments");
    const X3hGroupPlanes g = x3h_group_planes(row_len, w_off, ldw, strideW, groups);
    *form = g.form; *wh_off = g.wh_off; *wh_ldb = g.wh_ldb; *wh_gstride = g.wh_gstride; *inv_off = g.inv_off;
    *wh_inv_stride = g.wh_inv_stride;
    MT2_API_END
}

// Kernel tests of grouped launches: every field of GemmP a caller of the model sets, given explicitly (no defaults, no offsets on
// force_cfg).  The per-call EngineOpts of mt2_op_gemm.
int mt2_op_gemm_grouped(void* stream, const mt2_gemm_desc* d) {
    MT2_API_BEGIN
    MT2_REQUIRE(d != nullptr, "null descriptor");
    MT2_REQUIRE(d->struct_bytes == (int32_t)sizeof(mt2_gemm_desc), "descriptor size mismatch");
    if (d->cfg_out) *d->cfg_out = -1;
    if (d->epi4_out) *d->epi4_out = 0;
    GemmP p{};
    p.X = d->X; p.strideX = d->strideX; p.ldx = d->ldx; p.Rx = d->Rx;
    p.rowbase = d->rowbase; p.a_mul = d->a_mul; p.shift0 = d->shift0; p.taps = d->taps; p.dil = d->dil; p.Cin = d->Cin;
    p.W = d->W; p.strideW = d->strideW; p.ldw = d->ldw;
    p.W3 = d->W3; p.w3_plane = d->w3_plane;
    p.Wh = d->Wh; p.wh_inv = d->wh_inv; p.wh_ldb = d->wh_ldb; p.wh_gstride = d->wh_gstride; p.wh_inv_stride = d->wh_inv_stride;
    p.a_planes = d->a_planes;
    p.bias = d->bias; p.strideB = d->strideB; p.R = d->R; p.strideR = d->strideR; p.ldr = d->ldr; p.valid = d->valid;
    p.C = d->C; p.strideC = d->strideC; p.ldc = d->ldc;
    p.M = d->M; p.N = d->N; p.K = d->taps * d->Cin; p.groups = d->groups;
    p.pro_act = d->pro_act; p.pro_slope = d->pro_slope; p.epi_act = d->epi_act; p.out_scale = d->out_scale;
    MT2_REQUIRE(p.X && p.W && p.C && p.taps >= 1 && p.dil >= 1 && p.a_mul >= 1 && p.groups >= 1, "bad arguments");
    EngineOpts o;            // per call: no state is shared with any handle or thread
    o.force_cfg = d->force_cfg;
    o.x3h_flag = d->range_flag;
    o.ks_epi4 = d->ks_epi4;
    const GemmRoute rt = gemm_route(p, o);
    if (d->cfg_out) *d->cfg_out = rt.cfg;
    if (d->epi4_out) *d->epi4_out = rt.err == hipSuccess ? rt.ks_epi4 : 0;
    MT2_HIP(launch_gemm(p, (hipStream_t)stream, &o));
    MT2_API_END
}

// Kernel tests of the GEMM -> GEMM LayerNorm hand-off (round 5; GemmP::stat_out / ln_stat): ONE linear launch on an x6 tile.
// stat_out != nullptr: the epilogue also writes (mean, M2) pairs of the final C rows ([M][*stat_nt][2]; *stat_nt = 0 when the
// chosen tile has no such epilogue).  ln_stat != nullptr: pair-fed algebraic LayerNorm - W / W3 are the gamma-folded weights,
// bias = c, ln_s = s (mt2_model.h EncLayerW), statistics of source row r = ln_stat[r][ln_nt][2] with ln_w columns per pair.
static int op_gemm_ln_impl(void* stream, const float* X, int ldx, int Rx, int a_mul, int shift0, const float* W, const void* W3,
                           const void* Wh, const float* wh_inv, const float* bias, const float* R, int ldr, float* C, int ldc, int M,
                           int N, int K, int epi_act, int force_cfg, float* stat_out, int32_t* stat_nt, int32_t* stat_w,
                           const float* ln_stat, int ln_nt, int ln_w, const float* ln_s, float ln_eps);
int mt2_op_gemm_x6_ln(void* stream, const float* X, int ldx, int Rx, int a_mul, int shift0, const float* W, const void* W3,
                      const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N, int K, int epi_act,
                      int force_cfg, float* stat_out, int32_t* stat_nt, int32_t* stat_w, const float* ln_stat, int ln_nt,
                      int ln_w, const float* ln_s, float ln_eps) {
    return op_gemm_ln_impl(stream, X, ldx, Rx, a_mul, shift0, W, W3, nullptr, nullptr, bias, R, ldr, C, ldc, M, N, K, epi_act, force_cfg,
                           stat_out, stat_nt, stat_w, ln_stat, ln_nt, ln_w, ln_s, ln_eps);
}
// the same with the fp16 planes of W as well (mt2_op_gemm_x3h): the pair hand-off on the fp16-pipe tile (force_cfg 103)
int mt2_op_gemm_x3h_ln(void* stream, const float* X, int ldx, int Rx, int a_mul, int shift0, const float* W, const void* W3,
                       const void* Wh, const float* wh_inv, const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N,
                       int K, int epi_act, int force_cfg, float* stat_out, int32_t* stat_nt, int32_t* stat_w, const float* ln_stat,
                       int ln_nt, int ln_w, const float* ln_s, float ln_eps) {
    return op_gemm_ln_impl(stream, X, ldx, Rx, a_mul, shift0, W, W3, Wh, wh_inv, bias, R, ldr, C, ldc, M, N, K, epi_act, force_cfg,
                           stat_out, stat_nt, stat_w, ln_stat, ln_nt, ln_w, ln_s, ln_eps);
}
static int op_gemm_ln_impl(void* stream, const float* X, int ldx, int Rx, int a_mul, int shift0, const float* W, const void* W3,
                           const void* Wh, const float* wh_inv, const float* bias, const float* R, int ldr, float* C, int ldc, int M,
                           int N, int K, int epi_act, int force_cfg, float* stat_out, int32_t* stat_nt, int32_t* stat_w,
                           const float* ln_stat, int ln_nt, int ln_w, const float* ln_s, float ln_eps) {
    MT2_API_BEGIN
    GemmP p{};
    p.Wh = Wh; p.wh_inv = wh_inv;
    p.X = X; p.ldx = ldx; p.Rx = Rx; p.a_mul = a_mul ? a_mul : 1; p.shift0 = shift0; p.taps = 1; p.dil = 1; p.Cin = K; p.W = W;
    p.W3 = W3; p.ldw = K; p.bias = bias; p.R = R; p.ldr = ldr; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.K = K; p.groups = 1;
    p.epi_act = epi_act; p.out_scale = 1.0f; p.stat_out = stat_out;
    if (ln_stat) { p.pro_act = 5; p.ln_stat = ln_stat; p.ln_nt = ln_nt; p.ln_w = ln_w; p.ln_g = ln_s; p.ln_eps = ln_eps; }
    EngineOpts o;
    if (force_cfg >= 8000) { o.ks_epi4 = 0; force_cfg -= 8000; }        // tests: configuration + 8000 = the K-split tiles' dword finish (option ks_epi4 = 0)
    o.ldr64 = force_cfg >= 1000;
    o.force_cfg = force_cfg >= 1000 ? force_cfg - 1000 : force_cfg;
    const hipError_t e = launch_gemm(p, (hipStream_t)stream, &o);
    MT2_REQUIRE(e != hipErrorNotSupported, "this tile configuration has no pair-fed LayerNorm form");
    MT2_HIP(e);
    if (stat_nt) *stat_nt = o.last_stat_nt;
    if (stat_w) *stat_w = o.last_stat_w;
    MT2_API_END
}

int mt2_op_tile_major(void* stream, const float* W, int N, int K, float* out) {
    MT2_API_BEGIN
    MT2_REQUIRE(W && out && N > 0 && K > 0 && N % 16 == 0 && K % 64 == 0, "tile-major layout needs N % 16 == 0 and K % 64 == 0");
    MT2_HIP(launch_tile_major(W, N, K, out, (hipStream_t)stream));
    MT2_API_END
}

int mt2_op_gemm_tm(void* stream, const float* X, long long x_gstride, int ldx, int Rx, int a_mul, int shift0, const float* Wtm,
                   int Kw, int n0, int k0, long long w_gstride, int groups, const float* bias, const float* R, int ldr,
                   const int32_t* valid, float* C, long long c_gstride, int ldc, int M, int N, int K, int pro_act, float pro_slope,
                   int epi_act, const float* ln_gamma, const float* ln_beta, float ln_eps) {
    MT2_API_BEGIN
    MT2_REQUIRE(X && Wtm && C && Kw % 64 == 0 && n0 % 16 == 0 && k0 % 64 == 0 && groups >= 1, "bad arguments");
    GemmP p{};
    p.X = X; p.strideX = x_gstride; p.ldx = ldx; p.Rx = Rx; p.a_mul = a_mul ? a_mul : 1; p.shift0 = shift0; p.taps = 1; p.dil = 1;
    p.Cin = K; p.K = K; p.W = nullptr; p.strideW = w_gstride; p.ldw = Kw; p.Wtm = Wtm; p.tm_n0 = n0 / 16; p.tm_k0 = k0 / 64;
    p.tm_kb = Kw / 64; p.bias = bias; p.R = R; p.ldr = ldr; p.valid = valid; p.C = C; p.strideC = c_gstride; p.ldc = ldc;
    p.M = M; p.N = N; p.groups = groups; p.pro_act = ln_gamma ? 3 : (pro_act & 0xff); p.pro_slope = pro_slope; p.epi_act = epi_act;
    p.sk_nw = (pro_act & 0x100) ? 8 : 16;       // + 0x100: the eight-wave form (the model's default is sixteen / twelve waves at M <= 32)
    p.out_scale = 1.0f; p.ln_g = ln_gamma; p.ln_b = ln_beta; p.ln_eps = ln_eps;
    MT2_REQUIRE(gemm_skinny_tm_eligible(p, 64), "shape not served by the tile-major weight-streaming kernel");
    MT2_HIP(launch_gemm_skinny_tm(p, (hipStream_t)stream));
    MT2_API_END
}

// Kernel test of the pair hand-off at a handful of rows (round 5): the tile-major weight-streaming kernel with stat_out != nullptr
// (epilogue writes (mean, M2) per row and 16-column block: stat_out[M][N / 16][2]) and / or ln_stat != nullptr (LayerNorm prologue
// fed by such pairs of the SOURCE rows, ln_nt = K / 16 per row, instead of a pass over the rows).
int mt2_op_gemm_tm_pairs(void* stream, const float* X, int ldx, int Rx, int a_mul, int shift0, const float* Wtm, int Kw,
                         const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N, int K, int epi_act,
                         const float* ln_gamma, const float* ln_beta, float ln_eps, float* stat_out, const float* ln_stat, int ln_nt) {
    MT2_API_BEGIN
    MT2_REQUIRE(X && Wtm && C && Kw % 64 == 0, "bad arguments");
    GemmP p{};
    p.X = X; p.ldx = ldx; p.Rx = Rx; p.a_mul = a_mul ? a_mul : 1; p.shift0 = shift0; p.taps = 1; p.dil = 1; p.Cin = K; p.K = K;
    p.ldw = Kw; p.Wtm = Wtm; p.tm_kb = Kw / 64; p.bias = bias; p.R = R; p.ldr = ldr; p.C = C; p.ldc = ldc; p.M = M; p.N = N; p.groups = 1;
    p.pro_act = ln_gamma ? 3 : 0; p.epi_act = epi_act; p.out_scale = 1.0f; p.ln_g = ln_gamma; p.ln_b = ln_beta; p.ln_eps = ln_eps;
    p.stat_out = stat_out; p.ln_stat = ln_stat; p.ln_nt = ln_nt; p.ln_w = ln_stat ? 16 : 0;
    EngineOpts o;
    hipError_t e = launch_gemm(p, (hipStream_t)stream, &o);
    MT2_HIP(e);
    MT2_REQUIRE(!stat_out || o.last_stat_w == 16, "the launch did not take the tile-major route with the statistics epilogue");
    MT2_API_END
}

int mt2_op_layernorm(void* stream, const float* x, int ldx, const float* gamma, const float* beta, const float* R1,
                     int ldr1, const int32_t* valid, float* out, int ldo, int M, int C, float eps, int act) {
    MT2_API_BEGIN
    LnP p{};
    p.x = x; p.ldx = ldx; p.gamma = gamma; p.beta = beta; p.R1 = R1; p.ldr1 = ldr1; p.valid = valid;
    p.out = out; p.ldo = ldo; p.M = M; p.C = C; p.eps = eps; p.act = act >= 100 ? act - 100 : act;
    p.out_planes = act >= 100 ? 1 : 0;        // tests: act + 100 = the output as fp16 planes (LnP::out_planes)
    MT2_HIP(launch_layernorm(p, (hipStream_t)stream));
    MT2_API_END
}

// ---- test-only entries into the row kernels (rowops.hip): every field of the parameter block, nothing defaulted
int mt2_op_layernorm_ex(void* stream, const float* x, int ldx, const float* gamma, const float* beta, int rows_per_group,
                        const float* R1, int ldr1, int r1_rows, const float* R2, int ldr2, const int32_t* valid, int valid_rows,
                        float* out, int ldo, int M, int C, float eps, int act, int out_planes, int32_t* x3h_flag) {
    MT2_API_BEGIN
    LnP p{};
    p.x = x; p.ldx = ldx; p.gamma = gamma; p.beta = beta; p.rows_per_group = rows_per_group;
    p.R1 = R1; p.ldr1 = ldr1; p.r1_rows = r1_rows; p.R2 = R2; p.ldr2 = ldr2; p.valid = valid; p.valid_rows = valid_rows;
    p.out = out; p.ldo = ldo; p.M = M; p.C = C; p.eps = eps; p.act = act; p.out_planes = out_planes; p.x3h_flag = x3h_flag;
    MT2_HIP(launch_layernorm(p, (hipStream_t)stream));
    MT2_API_END
}

int mt2_op_ln_reduce(void* stream, const float* parts, long long pstride, int S, const float* bias, const float* R, int ldr,
                     const float* gamma, const float* beta, float* xout, int ldx, float* hout, int ldh, int M, int C, float eps,
                     int h_planes, int32_t* x3h_flag) {
    MT2_API_BEGIN
    LnReduceP p{};
    p.parts = parts; p.pstride = pstride; p.S = S; p.bias = bias; p.R = R; p.ldr = ldr; p.gamma = gamma; p.beta = beta;
    p.xout = xout; p.ldx = ldx; p.hout = hout; p.ldh = ldh; p.M = M; p.C = C; p.eps = eps; p.h_planes = h_planes;
    p.x3h_flag = x3h_flag;
    MT2_HIP(launch_ln_reduce(p, (hipStream_t)stream));      // the launcher's own choice between its two kernels (M = 4096)
    MT2_API_END
}

// an integer argument of mt2_op_row that the launcher takes as int
static int row_int(long long v) {
    MT2_REQUIRE(v >= INT_MIN && v <= INT_MAX, "mt2_op_row: integer argument does not fit the launcher's int parameter");
    return (int)v;
}
// One dispatcher for the launch_* row utilities of mt2_kernels.h: `op` is the launcher's name without "launch_"; its arguments arrive
// in the launcher's order, split by kind - pointers in ptrs, integers in ints, floats in flts.  The counts are checked against the
// table BEFORE anything is unpacked: a wrong count or an unknown name is an error, never a launch.
int mt2_op_row(void* stream, const char* op, void* const* ptrs, int nptrs, const long long* ints, int nints, const float* flts,
               int nflts) {
    MT2_API_BEGIN
    // one line per op: its name, how many pointers / integers / floats it takes, and the call that unpacks them
    struct RowOp { const char* name; int np, ni, nf; hipError_t (*run)(void* const*, const long long*, const float*, hipStream_t); };
#define ROW_ARGS void* const* ptrs, const long long* ints, const float* flts, hipStream_t s
#define ROW_PF(i) static_cast<const float*>(ptrs[i])
#define ROW_PFW(i) static_cast<float*>(ptrs[i])
#define ROW_PI(i) static_cast<const int*>(ptrs[i])
#define ROW_PIW(i) static_cast<int*>(ptrs[i])
#define ROW_PL(i) static_cast<const int64_t*>(ptrs[i])
#define ROW_PLW(i) static_cast<int64_t*>(ptrs[i])
#define ROW_PLL(i) static_cast<const long long*>(ptrs[i])
#define ROW_INT(i) row_int(ints[i])
#define ROW_LONG(i) (ints[i])
    static const RowOp kOps[] = {
        {"embed_pe", 6, 4, 0, [](ROW_ARGS) { return launch_embed_pe(ROW_PF(0), ROW_INT(0), ROW_PL(1), ROW_PI(2), ROW_PI(3), ROW_PF(4), ROW_PFW(5), ROW_INT(1), ROW_INT(2), ROW_INT(3), s); }},
        {"gather_rows", 3, 4, 0, [](ROW_ARGS) { return launch_gather_rows(ROW_PF(0), ROW_INT(0), ROW_PI(1), ROW_PFW(2), ROW_INT(1), ROW_INT(2), ROW_INT(3), s); }},
        {"pool_max", 4, 4, 0, [](ROW_ARGS) { return launch_pool_max(ROW_PF(0), ROW_INT(0), ROW_PI(1), ROW_PI(2), ROW_PFW(3), ROW_INT(1), ROW_INT(2), ROW_INT(3), s); }},
        {"sum_groups", 2, 6, 0, [](ROW_ARGS) { return launch_sum_groups(ROW_PF(0), ROW_LONG(0), ROW_INT(1), ROW_INT(2), ROW_PFW(1), ROW_INT(3), ROW_INT(4), ROW_INT(5), s); }},
        {"avg3", 4, 1, 1, [](ROW_ARGS) { return launch_avg3(ROW_PF(0), ROW_PF(1), ROW_PF(2), flts[0], ROW_PFW(3), ROW_LONG(0), s); }},
        {"conv_post", 7, 3, 2, [](ROW_ARGS) { return launch_conv_post(ROW_PF(0), ROW_PF(1), ROW_PF(2), flts[0], ROW_LONG(0), ROW_INT(1), ROW_INT(2), ROW_PF(3), ROW_PF(4), flts[1], ROW_PI(5), ROW_PFW(6), s); }},
        {"fill_reflect", 3, 5, 0, [](ROW_ARGS) { return launch_fill_reflect(ROW_PFW(0), ROW_INT(0), ROW_INT(1), ROW_PI(1), ROW_PI(2), ROW_INT(2), ROW_LONG(3), ROW_INT(4), s); }},
        {"pack_rows", 3, 5, 0, [](ROW_ARGS) { return launch_pack_rows(ROW_PF(0), ROW_INT(0), ROW_INT(1), ROW_INT(2), ROW_PI(1), ROW_PFW(2), ROW_INT(3), ROW_INT(4), s); }},
        {"unpack_rows", 3, 5, 0, [](ROW_ARGS) { return launch_unpack_rows(ROW_PF(0), ROW_INT(0), ROW_INT(1), ROW_INT(2), ROW_INT(3), ROW_PI(1), ROW_PFW(2), ROW_INT(4), s); }},
        {"adm_step_input", 6, 6, 0, [](ROW_ARGS) { return launch_adm_step_input(ROW_PF(0), ROW_INT(0), ROW_PI(1), ROW_PF(2), ROW_PF(3), ROW_INT(1), ROW_PF(4), ROW_PFW(5), ROW_INT(2), ROW_INT(3), ROW_INT(4), ROW_INT(5), s); }},
        {"plm_step_input", 6, 7, 0, [](ROW_ARGS) { return launch_plm_step_input(ROW_PF(0), ROW_INT(0), ROW_PI(1), ROW_PF(2), ROW_PL(3), ROW_INT(1), ROW_PF(4), ROW_PFW(5), ROW_INT(2), ROW_INT(3), ROW_INT(4), ROW_INT(5), ROW_INT(6), s); }},
        {"adm_predict", 3, 5, 0, [](ROW_ARGS) { return launch_adm_predict(ROW_PF(0), ROW_INT(0), ROW_PF(1), ROW_PFW(2), ROW_INT(1), ROW_INT(2), ROW_INT(3), ROW_INT(4), s); }},
        {"adm_finalize", 5, 4, 0, [](ROW_ARGS) { return launch_adm_finalize(ROW_PF(0), ROW_INT(0), ROW_PI(1), ROW_PI(2), static_cast<int32_t*>(ptrs[3]), ROW_PFW(4), ROW_INT(1), ROW_INT(2), ROW_INT(3), s); }},
        {"plm_finalize", 4, 5, 0, [](ROW_ARGS) { return launch_plm_finalize(ROW_PL(0), ROW_INT(0), ROW_PI(1), ROW_PI(2), ROW_PLW(3), ROW_INT(1), ROW_INT(2), ROW_INT(3), ROW_INT(4), s); }},
        {"adm_init_hist", 3, 3, 0, [](ROW_ARGS) { return launch_adm_init_hist(ROW_PFW(0), ROW_INT(0), ROW_PF(1), ROW_INT(1), ROW_PI(2), ROW_INT(2), s); }},
        {"plm_init_hist", 3, 5, 0, [](ROW_ARGS) { return launch_plm_init_hist(ROW_PLW(0), ROW_INT(0), (int64_t)ROW_LONG(1), ROW_PL(1), ROW_INT(2), ROW_INT(3), ROW_PI(2), ROW_INT(4), s); }},
        {"check_ids", 3, 3, 0, [](ROW_ARGS) { return launch_check_ids(ROW_PL(0), ROW_PI(1), ROW_INT(0), ROW_LONG(1), ROW_PIW(2), ROW_INT(2), s); }},
        {"copy_2d", 2, 4, 0, [](ROW_ARGS) { return launch_copy_2d(ROW_PF(0), ROW_LONG(0), ROW_PFW(1), ROW_LONG(1), ROW_LONG(2), ROW_INT(3), s); }},
        {"scatter_i64", 3, 1, 0, [](ROW_ARGS) { return launch_scatter_i64(ROW_PL(0), ROW_PI(1), ROW_PLW(2), ROW_INT(0), s); }},
        {"expand_mask", 2, 2, 0, [](ROW_ARGS) { return launch_expand_mask(ROW_PI(0), ROW_INT(0), ROW_PIW(1), ROW_LONG(1), s); }},
        {"unpack_wav", 4, 3, 0, [](ROW_ARGS) { return launch_unpack_wav(ROW_PF(0), ROW_PLL(1), ROW_PLL(2), ROW_PFW(3), ROW_LONG(0), ROW_LONG(1), ROW_INT(2), s); }},
        {"argmax_rows", 2, 5, 0, [](ROW_ARGS) { return launch_argmax_rows(ROW_PF(0), ROW_INT(0), ROW_INT(1), ROW_PLW(1), ROW_INT(2), ROW_INT(3), ROW_INT(4), s); }},
        {"vq_argmin", 5, 5, 0, [](ROW_ARGS) { return launch_vq_argmin(ROW_PF(0), ROW_INT(0), ROW_INT(1), ROW_PF(1), ROW_INT(2), ROW_PF(2), ROW_INT(3), ROW_PI(3), ROW_PLW(4), ROW_INT(4), s); }},
        {"row_sqnorm", 2, 2, 0, [](ROW_ARGS) { return launch_row_sqnorm(ROW_PF(0), ROW_INT(0), ROW_PFW(1), ROW_INT(1), s); }},
        {"codebook_rows", 4, 4, 0, [](ROW_ARGS) { return launch_codebook_rows(ROW_PF(0), ROW_PL(1), ROW_PI(2), ROW_PFW(3), ROW_INT(0), ROW_INT(1), ROW_INT(2), ROW_INT(3), s); }},
        {"reflect_pad_blocks", 5, 4, 0, [](ROW_ARGS) { return launch_reflect_pad_blocks(ROW_PF(0), ROW_LONG(0), ROW_PI(1), ROW_PI(2), ROW_PI(3), ROW_INT(1), ROW_INT(2), ROW_PFW(4), ROW_INT(3), s); }},
        {"magnitude", 2, 4, 0, [](ROW_ARGS) { return launch_magnitude(ROW_PF(0), ROW_INT(0), ROW_INT(1), ROW_PFW(1), ROW_INT(2), ROW_INT(3), s); }},
        {"gl_exp_rows", 3, 2, 0, [](ROW_ARGS) { return launch_gl_exp_rows(ROW_PF(0), ROW_INT(0), ROW_PI(1), ROW_PFW(2), ROW_INT(1), s); }},
        {"gl_phase_init", 5, 4, 0, [](ROW_ARGS) { return launch_gl_phase_init(ROW_PF(0), ROW_INT(0), ROW_PI(1), ROW_PI(2), static_cast<const uint32_t*>(ptrs[3]), ROW_PFW(4), ROW_INT(1), ROW_INT(2), ROW_INT(3), s); }},
        {"istft_ola_blocks", 7, 3, 0, [](ROW_ARGS) { return launch_istft_ola_blocks(ROW_PF(0), ROW_INT(0), ROW_INT(1), ROW_PF(1), ROW_PI(2), ROW_PI(3), ROW_PI(4), ROW_PI(5), ROW_PFW(6), ROW_INT(2), s); }},
        {"istft_ola_wav", 5, 4, 0, [](ROW_ARGS) { return launch_istft_ola_wav(ROW_PF(0), ROW_INT(0), ROW_INT(1), ROW_PF(1), ROW_PI(2), ROW_PI(3), ROW_PFW(4), ROW_INT(2), ROW_INT(3), s); }},
        {"gl_phase_update", 6, 5, 1, [](ROW_ARGS) { return launch_gl_phase_update(ROW_PF(0), ROW_PFW(1), ROW_PF(2), ROW_INT(0), ROW_PFW(3), ROW_INT(1), ROW_INT(2), flts[0], ROW_PFW(4), ROW_PI(5), ROW_INT(3), ROW_INT(4), s); }},
    };
#undef ROW_ARGS
#undef ROW_PF
#undef ROW_PFW
#undef ROW_PI
#undef ROW_PIW
#undef ROW_PL
#undef ROW_PLW
#undef ROW_PLL
#undef ROW_INT
#undef ROW_LONG
    MT2_REQUIRE(op != nullptr, "mt2_op_row: null op name");
    const std::string name(op);
    int id = -1;
    for (size_t i = 0; i < sizeof(kOps) / sizeof(kOps[0]); ++i)
        if (name == kOps[i].name) id = (int)i;
    MT2_REQUIRE(id >= 0, "mt2_op_row: unknown op '" + name + "'");
    MT2_REQUIRE(nptrs == kOps[id].np && nints == kOps[id].ni && nflts == kOps[id].nf,
                "mt2_op_row: wrong argument count for '" + name + "' (wants " + std::to_string(kOps[id].np) + " pointers, " +
                    std::to_string(kOps[id].ni) + " integers, " + std::to_string(kOps[id].nf) + " floats)");
    MT2_REQUIRE((nptrs == 0 || ptrs) && (nints == 0 || ints) && (nflts == 0 || flts), "mt2_op_row: null argument array");
    const hipError_t e = kOps[id].run(ptrs, ints, flts, (hipStream_t)stream);
    if (e != hipSuccess) throw Error("mt2_op_row(" + name + "): " + hipGetErrorName(e) + " (" + hipGetErrorString(e) + ")");
    MT2_API_END
}

int mt2_op_sample_rows(void* stream, const float* logits, int ld, int N, int A, const mt2_sampling* s, const uint64_t* seeds_dev,
                       const int32_t* positions_dev, int64_t* out) {
    MT2_API_BEGIN
    MT2_REQUIRE(logits && s && seeds_dev && positions_dev && out && A >= 0 && N >= 1 && ld >= N, "bad arguments");
    check_sampling(*s, N, false);
    MT2_HIP(launch_sample_rows(logits, ld, N, out, 1, 0, A, s->temperature, s->top_k, s->top_p,
                               reinterpret_cast<const uint32_t*>(seeds_dev), nullptr, positions_dev, 0, (hipStream_t)stream));
    MT2_API_END
}

int mt2_op_sample_mix_rows(void* stream, const float* logits, int ld, int N, int A, const mt2_sampling* s,
                           const uint64_t* seeds_dev, const int32_t* positions_dev, const float* gamma_dev, int64_t* out) {
    MT2_API_BEGIN
    MT2_REQUIRE(logits && gamma_dev && out && A >= 0 && N >= 1 && ld >= N, "bad arguments");
    MT2_REQUIRE(!s || (seeds_dev && positions_dev), "bad arguments: a sampled draw needs seeds_dev and positions_dev");
    if (s) check_sampling(*s, N, false);
    MT2_REQUIRE(N <= 1024, "the mixture kernel serves at most 1024 bins");
    MT2_HIP(launch_sample_mix_rows(logits, ld, N, out, 1, 0, A, s == nullptr, s ? s->temperature : 1.0f, s ? s->top_k : 0,
                                   s ? s->top_p : 1.0f, reinterpret_cast<const uint32_t*>(seeds_dev), nullptr, positions_dev, 0,
                                   gamma_dev, (hipStream_t)stream));
    MT2_API_END
}

int mt2_op_attention(void* stream, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                     float* O, int ldo, const int32_t* q_start, const int32_t* q_len, const int32_t* kv_start,
                     const int32_t* kv_len, int B, int H, int D, int max_qlen, float scale) {
    MT2_API_BEGIN
    AttnP a{};
    a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.V = V; a.ldv = ldv; a.O = O; a.ldo = ldo;
    a.q_start = q_start; a.q_len = q_len; a.kv_start = kv_start; a.kv_len = kv_len;
    a.B = B; a.H = H; a.D = D; a.max_qlen = max_qlen; a.scale = scale;
    MT2_HIP(launch_attention(a, (hipStream_t)stream));
    MT2_API_END
}
// the same with the kernel choice exposed (measurement / kernel tests): lds_min_qlen = first query count that uses the
// LDS-tiled kernel (0: never, < 0: default), lds_waves = query tiles per workgroup of that kernel (8, otherwise 4),
// x6_min_qlen = first query count served by the bf16-pipe kernel (f32-equivalent; D = 64 / 96; 0: never, < 0: default)
int mt2_op_attention_tuned(void* stream, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                           float* O, int ldo, const int32_t* q_start, const int32_t* q_len, const int32_t* kv_start,
                           const int32_t* kv_len, int B, int H, int D, int max_qlen, float scale, int lds_min_qlen,
                           int lds_waves, int x6_min_qlen, int max_kvlen) {
    MT2_API_BEGIN
    AttnP a{};
    a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.V = V; a.ldv = ldv; a.O = O; a.ldo = ldo;
    a.q_start = q_start; a.q_len = q_len; a.kv_start = kv_start; a.kv_len = kv_len;
    a.B = B; a.H = H; a.D = D; a.max_qlen = max_qlen; a.scale = scale; a.max_kvlen = max_kvlen;
    if (lds_min_qlen >= 0) a.lds_min_qlen = lds_min_qlen;
    a.ds_short = (lds_waves & 32) ? 0 : 1;        // + 32: the register kernel instead of the head-dim-split kernel (measurement / tests)
    a.o_planes = (lds_waves & 64) ? 1 : 0;        // + 64: O receives fp16 planes (AttnP::o_planes; tests)
    a.x3h = (lds_waves & 128) ? 1 : 0;            // + 128: the long-sequence kernel in its fp16-pipe form (AttnP::x3h)
    lds_waves &= ~(32 | 64 | 128);
    MT2_REQUIRE(lds_waves == 0 || lds_waves == 4 || lds_waves == 8, "lds_waves must be 0, 4 or 8 (+ 32)");
    a.lds_waves = lds_waves;
    if (x6_min_qlen >= 0) a.x6_min_qlen = x6_min_qlen;
    MT2_HIP(launch_attention(a, (hipStream_t)stream));
    MT2_API_END
}

// the fp16-pipe form of the long-sequence kernel (AttnP::x3h) with its range guard exposed: range_flag (device int32) |= 1 when a
// Q / K / V value at or beyond 65504 was converted - the model repeats such a call on the bf16-pipe kernel
int mt2_op_attention_x3h(void* stream, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                         float* O, int ldo, const int32_t* q_start, const int32_t* q_len, const int32_t* kv_start,
                         const int32_t* kv_len, int B, int H, int D, int max_qlen, float scale, int lds_waves, int max_kvlen,
                         int32_t* range_flag) {
    MT2_API_BEGIN
    MT2_REQUIRE(D == 64 || D == 96, "the fp16-pipe attention kernel serves head dims 64 and 96");
    MT2_REQUIRE(lds_waves == 0 || lds_waves == 4 || lds_waves == 8, "lds_waves must be 0, 4 or 8");
    AttnP a{};
    a.Q = Q; a.ldq = ldq; a.K = K; a.ldk = ldk; a.V = V; a.ldv = ldv; a.O = O; a.ldo = ldo;
    a.q_start = q_start; a.q_len = q_len; a.kv_start = kv_start; a.kv_len = kv_len;
    a.B = B; a.H = H; a.D = D; a.max_qlen = max_qlen; a.scale = scale; a.max_kvlen = max_kvlen;
    a.lds_waves = lds_waves; a.x6_min_qlen = 1; a.x3h = 1; a.x3h_flag = range_flag;
    MT2_HIP(launch_attention(a, (hipStream_t)stream));
    MT2_API_END
}

// Kernel tests of the launch geometry: every field of AttnP given explicitly (mt2_attn_desc), and the route that launch takes
static_assert(MT2_ATTN_NONE == ATTN_NONE && MT2_ATTN_GENERIC == ATTN_GENERIC && MT2_ATTN_REG == ATTN_REG && MT2_ATTN_DS == ATTN_DS &&
              MT2_ATTN_LDS == ATTN_LDS && MT2_ATTN_X6 == ATTN_X6 && MT2_ATTN_X3H == ATTN_X3H, "kernel ids of the C ABI");
static AttnP attn_from_desc(const mt2_attn_desc& d) {
    AttnP a{};
    a.Q = d.Q; a.ldq = d.ldq; a.K = d.K; a.ldk = d.ldk; a.V = d.V; a.ldv = d.ldv; a.O = d.O; a.ldo = d.ldo;
    a.q_start = d.q_start; a.q_len = d.q_len; a.kv_start = d.kv_start; a.kv_len = d.kv_len; a.o_start = d.o_start;
    a.u_qstride = d.u_qstride; a.u_qlen = d.u_qlen; a.u_kvstride = d.u_kvstride; a.u_kvlen = d.u_kvlen; a.u_ostride = d.u_ostride;
    a.B = d.B; a.H = d.H; a.D = d.D; a.max_qlen = d.max_qlen; a.max_kvlen = d.max_kvlen; a.scale = d.scale;
    a.lds_min_qlen = d.lds_min_qlen; a.x6_min_qlen = d.x6_min_qlen; a.lds_waves = d.lds_waves; a.ds_short = d.ds_short;
    a.x3h = d.x3h; a.o_planes = d.o_planes; a.x3h_flag = d.range_flag;
    return a;
}
int mt2_op_attention_desc(void* stream, const mt2_attn_desc* d) {
    MT2_API_BEGIN
    MT2_REQUIRE(d != nullptr, "null descriptor");
    MT2_REQUIRE(d->struct_bytes == (int32_t)sizeof(mt2_attn_desc), "descriptor size mismatch");
    if (d->kernel_out) *d->kernel_out = MT2_ATTN_NONE;
    const bool ragged = d->q_start != nullptr;
    MT2_REQUIRE(d->Q && d->K && d->V && d->O, "bad arguments");
    MT2_REQUIRE(ragged ? (d->q_len && d->kv_start && d->kv_len) : (!d->q_len && !d->kv_start && !d->kv_len),
                "bad arguments: q_start, q_len, kv_start and kv_len come together or not at all");
    MT2_REQUIRE(ragged || (d->u_qstride >= 0 && d->u_kvstride >= 0 && d->u_ostride >= 0 && d->u_qlen >= 0 && d->u_kvlen >= 0),
                "bad arguments: negative uniform geometry");
    MT2_REQUIRE(d->lds_waves == 0 || d->lds_waves == 4 || d->lds_waves == 8, "lds_waves must be 0, 4 or 8");
    const AttnP a = attn_from_desc(*d);
    if (d->kernel_out) *d->kernel_out = attn_route(a).kernel;
    MT2_HIP(launch_attention(a, (hipStream_t)stream));
    MT2_API_END
}
int mt2_attention_route(const mt2_attn_desc* d, int32_t* err, int32_t* kernel, int32_t* tmpl, int32_t* launch, long long* lds) {
    if (!d || d->struct_bytes != (int32_t)sizeof(mt2_attn_desc)) return -1;
    const AttnRoute r = attn_route(attn_from_desc(*d));
    if (err) *err = (int32_t)r.err;
    if (kernel) *kernel = r.kernel;
    if (tmpl) { tmpl[0] = r.d; tmpl[1] = r.nwq; tmpl[2] = r.nkv; tmpl[3] = r.nwv; }
    if (launch) { launch[0] = (int32_t)r.gx; launch[1] = (int32_t)r.gy; launch[2] = (int32_t)r.gz; launch[3] = (int32_t)r.block; }
    if (lds) *lds = (long long)r.lds;
    return 0;
}

int mt2_bench_gemm(void* stream, int M, int N, int K, int taps, int dil, int flags, int force_cfg, int iters,
                   int w_copies, float* avg_ms, char* cfg_name, int cfg_name_cap, double* sustained_ghz) {
    MT2_API_BEGIN
    MT2_REQUIRE(taps >= 1 && K % taps == 0 && (K / taps) % 4 == 0 && iters >= 1 && dil >= 1, "bad GEMM shape");
    if (w_copies < 1) w_copies = 1;
    hipStream_t s = (hipStream_t)stream;
    const int Cin = K / taps;
    float *X, *W, *C, *R = nullptr, *bias = nullptr;
    int* valid = nullptr;
    MT2_HIP(hipMalloc((void**)&X, sizeof(float) * ((size_t)M + taps * dil) * Cin));
    MT2_HIP(hipMalloc((void**)&W, sizeof(float) * (size_t)N * K * w_copies));
    MT2_HIP(hipMalloc((void**)&C, sizeof(float) * (size_t)M * N));
    std::vector<float> h(std::max(std::max(((size_t)M + taps * dil) * Cin, (size_t)N * K), (size_t)M * N));
    unsigned rng = 12345u;
    for (auto& v : h) { rng = rng * 1664525u + 1013904223u; v = ((rng >> 8) & 0xffff) / 32768.0f - 1.0f; }
    MT2_HIP(hipMemcpy(X, h.data(), sizeof(float) * ((size_t)M + taps * dil) * Cin, hipMemcpyHostToDevice));
    if (flags & 2) {   // fused epilogue operands: bias, residual, row mask
        MT2_HIP(hipMalloc((void**)&R, sizeof(float) * (size_t)M * N));
        MT2_HIP(hipMalloc((void**)&bias, sizeof(float) * (size_t)N));
        MT2_HIP(hipMalloc((void**)&valid, sizeof(int) * (size_t)M));
        MT2_HIP(hipMemcpy(R, h.data(), sizeof(float) * (size_t)M * N, hipMemcpyHostToDevice));
        MT2_HIP(hipMemcpy(bias, h.data(), sizeof(float) * (size_t)N, hipMemcpyHostToDevice));
        std::vector<int> ones(M, 1);
        MT2_HIP(hipMemcpy(valid, ones.data(), sizeof(int) * (size_t)M, hipMemcpyHostToDevice));
    }
    for (int i = 0; i < w_copies; ++i)
        MT2_HIP(hipMemcpy(W + (size_t)i * N * K, h.data(), sizeof(float) * (size_t)N * K, hipMemcpyHostToDevice));
    // the same weights as three bf16 planes (plane stride = all copies), for the bf16-pipe configurations
    uint16_t* W3 = nullptr;
    const size_t wn = (size_t)N * K, wall = wn * w_copies;
    {
        std::vector<uint16_t> pl(3 * wall);
        for (size_t i = 0; i < wn; ++i) {
            float r = h[i];
            for (int k = 0; k < 3; ++k) {
                uint32_t bits;
                std::memcpy(&bits, &r, 4);
                bits &= 0xffff0000u;
                float top;
                std::memcpy(&top, &bits, 4);
                for (int cidx = 0; cidx < w_copies; ++cidx) pl[k * wall + cidx * wn + i] = (uint16_t)(bits >> 16);
                r -= top;
            }
        }
        MT2_HIP(hipMalloc((void**)&W3, pl.size() * sizeof(uint16_t)));
        MT2_HIP(hipMemcpy(W3, pl.data(), pl.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    }
    // ... as two fp16 planes of the row-scaled matrix, chunk-interleaved (+ inverse row scales), for the fp16-pipe configurations
    uint16_t* Wh = nullptr;
    float* wh_inv = nullptr;
    const size_t whn = (size_t)N * 2 * x3h_padded_k((size_t)K);      // fp16 elements of one copy
    {
        std::vector<uint16_t> one(whn), pl(whn * w_copies);
        std::vector<float> inv((size_t)N);
        x3h_split_rows(h.data(), (size_t)N, (size_t)K, one.data(), inv.data());
        for (int cidx = 0; cidx < w_copies; ++cidx) std::memcpy(pl.data() + cidx * whn, one.data(), whn * sizeof(uint16_t));
        MT2_HIP(hipMalloc((void**)&Wh, pl.size() * sizeof(uint16_t)));
        MT2_HIP(hipMemcpy(Wh, pl.data(), pl.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
        MT2_HIP(hipMalloc((void**)&wh_inv, inv.size() * sizeof(float)));
        MT2_HIP(hipMemcpy(wh_inv, inv.data(), inv.size() * sizeof(float), hipMemcpyHostToDevice));
    }
    // ... and as tile-major blocks, for the weight-streaming kernel of launches with at most 64 rows
    float* Wtm = nullptr;
    const bool tm = M <= 64 && taps == 1 && N % 16 == 0 && K % 64 == 0;
    if (tm) {
        MT2_HIP(hipMalloc((void**)&Wtm, sizeof(float) * wall));
        for (int i = 0; i < w_copies; ++i) MT2_HIP(launch_tile_major(W + (size_t)i * wn, N, K, Wtm + (size_t)i * wn, s));
    }
    GemmP p{};
    p.X = X; p.ldx = Cin; p.Rx = M + taps * dil; p.a_mul = 1; p.shift0 = 0; p.taps = taps; p.dil = dil; p.Cin = Cin;
    p.Wh = Wh; p.wh_inv = wh_inv;
    p.W = W; p.W3 = W3; p.w3_plane = (long long)wall; p.ldw = K; p.C = C; p.ldc = N; p.M = M; p.N = N; p.K = K; p.groups = 1;
    p.out_scale = 1.0f;
    if (tm) { p.Wtm = Wtm; p.tm_kb = K / 64; }
    if (flags & 1) { p.pro_act = ACT_LRELU; p.pro_slope = 0.1f; }
    p.R = R; p.ldr = N; p.bias = bias; p.valid = valid;
    unsigned long long* dbg = nullptr;
    if (flags & 4) {    // MT2_PHASE_TIMING builds: per-phase cycle sums of one wave of the x6 kernel (last launch wins)
        MT2_HIP(hipMalloc((void**)&dbg, 16 * sizeof(unsigned long long)));
        MT2_HIP(hipMemset(dbg, 0, 16 * sizeof(unsigned long long)));
        p.dbg = dbg;
    }
    EngineOpts o;
    o.force_cfg = force_cfg;
    if (flags & 16) o.ldr_prio = 0;         // measurement: loader waves at the default issue priority
    if (flags & 32) o.x3h = 0;              // measurement: the automatic choice without the fp16-pipe forms
    if (flags & 64) o.ks_epi4 = 0;          // measurement: the x3h K-split tiles' dword finish
    hipError_t e = launch_gemm(p, s, &o);   // warm-up
    hipEvent_t e0, e1;
    MT2_HIP(hipEventCreate(&e0));
    MT2_HIP(hipEventCreate(&e1));
    MT2_HIP(hipEventRecord(e0, s));
    for (int i = 0; i < iters && e == hipSuccess; ++i) {   // rotate the weight copy: as in the model, a launch
        p.W = W + (size_t)(i % w_copies) * N * K;          // does not find its weights in L2 from the last one
        p.W3 = W3 + (size_t)(i % w_copies) * N * K;
        p.Wh = Wh + (size_t)(i % w_copies) * whn;
        if (tm) p.Wtm = Wtm + (size_t)(i % w_copies) * N * K;
        e = launch_gemm(p, s, &o);
    }
    MT2_HIP(hipEventRecord(e1, s));
    MT2_HIP(hipEventSynchronize(e1));
    float ms = 0.f;
    MT2_HIP(hipEventElapsedTime(&ms, e0, e1));
    if (avg_ms) *avg_ms = ms / iters;
    if (sustained_ghz) *sustained_ghz = 0.0;
    if (cfg_name && cfg_name_cap > 0) {
        std::strncpy(cfg_name, o.last_cfg, cfg_name_cap - 1);
        cfg_name[cfg_name_cap - 1] = 0;
    }
    if (dbg) {
        unsigned long long hd[16] = {0};
        (void)hipMemcpy(hd, dbg, sizeof(hd), hipMemcpyDeviceToHost);
        const double nkd = hd[6] ? (double)hd[6] : 1.0;
        if (hd[0] + hd[1] + hd[5])
        std::fprintf(stderr, "x6 phase cycles per chunk (one wave, %llu chunks): dma_wait %.0f barrier %.0f refill_issue %.0f "
                             "first_fetch %.0f fetch2+split %.0f mfma_steps %.0f\n",
                     hd[6], hd[0] / nkd, hd[1] / nkd, hd[2] / nkd, hd[3] / nkd, hd[4] / nkd, hd[5] / nkd);
        if (hd[11] + hd[12] + hd[13])
            std::fprintf(stderr, "loader wave 0, cycles per chunk: vmcnt_wait %.0f barrier %.0f issue %.0f\n", hd[11] / nkd, hd[12] / nkd, hd[13] / nkd);
        // clock probe: s_memtime (shader cycles) against s_memrealtime (constant rate) over the same K loop of one wave
        int wall_khz = 0, sclk_khz = 0;
        (void)hipDeviceGetAttribute(&wall_khz, hipDeviceAttributeWallClockRate, 0);
        (void)hipDeviceGetAttribute(&sclk_khz, hipDeviceAttributeClockRate, 0);
        if (hd[7] && wall_khz > 0 && (flags & 8) == 0 && (hd[9] || hd[10]))
            std::fprintf(stderr, "one workgroup: entry -> K loop %.2f us, K loop %.2f us, epilogue %.2f us (launch average %.2f us)\n",
                         hd[9] / (wall_khz * 1e-3), hd[7] / (wall_khz * 1e-3), hd[10] / (wall_khz * 1e-3), ms / iters * 1e3);
        if (hd[7] && wall_khz > 0 && sustained_ghz) *sustained_ghz = (double)hd[8] / ((double)hd[7] / (wall_khz * 1e3)) / 1e9;
        if (hd[7] && wall_khz > 0 && (flags & 8) == 0)
            std::fprintf(stderr, "clock probe: %llu shader cycles in %llu ticks of the %d kHz wall clock -> %.3f GHz sustained in "
                                 "the K loop (device max %d kHz)\n", hd[8], hd[7], wall_khz,
                         (double)hd[8] / ((double)hd[7] / (wall_khz * 1e3)) / 1e9, sclk_khz);
        (void)hipFree(dbg);
    }
    (void)hipEventDestroy(e0);
    (void)hipEventDestroy(e1);
    (void)hipFree(X);
    (void)hipFree(W);
    (void)hipFree(W3);
    (void)hipFree(Wh);
    (void)hipFree(wh_inv);
    if (Wtm) (void)hipFree(Wtm);
    (void)hipFree(C);
    if (R) (void)hipFree(R);
    if (bias) (void)hipFree(bias);
    if (valid) (void)hipFree(valid);
    MT2_HIP(e);
    MT2_API_END
}

}  // extern "C"
