/* libmegatts2_hip - C ABI of the MI355X (gfx950) Mega-TTS 2 synthesis path.
 *
 * The reference (LSimon95/megatts2) has no plugin / FFI layer: its drop-in boundary is the Python
 * object surface of `models/megatts2.py`.  Each entry point below replaces one
 * method of that surface; the Python mirror in megatts2_amd/ binds them with ctypes and keeps the
 * reference's class / method names and tensor layouts.
 *
 * Conventions
 *  - Every `const float*` / `float*` / `int64_t*` / `int32_t*` NOT marked (host) is a DEVICE pointer
 *    (PyTorch-ROCm `tensor.data_ptr()`), f32 / int64 / int32, contiguous, 16-byte aligned.
 *  - Batched tensors use the reference's padded batch-first layouts; per-utterance true lengths are
 *    passed as (host) int32 arrays.  Padding positions of outputs are written as zeros.
 *  - `stream` is a hipStream_t (pass `torch.cuda.current_stream().cuda_stream`); all work is
 *    enqueued on it.  Calls that must size their output (mt2_adm_infer -> durations) document
 *    their host synchronisation.
 *  - Return value: 0 = ok, < 0 = error; `mt2_last_error()` gives the message (thread-local).
 *    Nothing throws across the boundary.
 *  - A model handle's weights are immutable after `mt2_model_finalize`.  The handle owns ONE activation
 *    workspace and its internal streams: calls on one handle are serialised (a mutex makes concurrent host
 *    threads safe; a call on a different stream than the previous call first waits, on the device, for that
 *    call's end).  For concurrency use one handle per thread / stream.  Apart from the handle there is no
 *    mutable global state in the library.  Batch semantics: every utterance is computed exactly as if it
 *    were alone (the reference is batch-1).
 */
#ifndef MEGATTS2_HIP_H
#define MEGATTS2_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct mt2_model mt2_model;

/* Hyper-parameters = the `model:` sub-trees of the reference's configs/config_{gan,plm,adm}.yaml
 * (reference models/megatts2.py:87-104,184-191,278-286) + the HiFi-GAN V1 generator topology. */
typedef struct mt2_config {
    /* MRTE (modules/mrte.py:64-84) */
    int32_t mel_bins, mrte_hidden, mrte_kernel, mrte_stride, mrte_n_layer, mrte_n_stack, mrte_n_block;
    int32_t content_ff_dim, content_n_heads, content_n_layers, phone_vocab;
    /* VQ prosody encoder (modules/vqpe.py:14-26) */
    int32_t vq_mel_bins, vq_stride, vq_hidden, vq_kernel, vq_n_layers, vq_n_stacks, vq_n_blocks, vq_bins, vq_dim;
    /* mel decoder (models/megatts2.py:31-54) */
    int32_t dec_kernel, dec_hidden, dec_n_stack, dec_n_block;
    /* PLM (models/megatts2.py:121-146) */
    int32_t plm_layers, plm_heads, plm_vq_dim, plm_tc_dim, plm_bins;
    /* ADM (models/megatts2.py:202-231) */
    int32_t adm_layers, adm_heads, adm_emb_dim, adm_tc_dim, adm_tc_emb_dim;
    /* HiFi-GAN V1 generator (speechbrain hub model in the reference, models/megatts2.py:321-323) */
    int32_t hg_in_dim, hg_init_channels, hg_n_up, hg_up_rates[8], hg_up_kernels[8];
    int32_t hg_n_res, hg_res_kernels[4], hg_res_dilations[4][3];
    float hg_slope;
    int32_t max_positions;   /* rows of the sine positional tables (embedding.py:66 builds 4000) */
    /* speechbrain HifiganGenerator.inference(): the mel is replicate-padded by this many frames on both sides
     * before the generator (hub model: 5), so decode_batch returns (T + 2*pad)*hop samples; 0 = plain forward */
    int32_t hg_inference_padding;
    /* edge mode of the generator's "same" convolutions (conv_pre, every ResBlock conv, conv_post): 0 = zero padding
     * (torch nn.Conv1d / transformers.SpeechT5HifiGan), 1 = per-utterance REFLECT padding - speechbrain's
     * nnet.CNN.Conv1d(padding="same") default padding_mode, what the hub model of the reference
     * (models/megatts2.py:321-323) is trained and run with.  The transposed convolutions are unaffected. */
    int32_t hg_reflect_pad;
} mt2_config;

const char* mt2_last_error(void);
const char* mt2_version(void);
/* 0 when a gfx950 device is visible and usable, < 0 otherwise (never falls back to a CPU path). */
int mt2_device_check(void);

/* ---- model lifetime (replaces MegaG/MegaPLM/MegaADM.from_pretrained, models/megatts2.py:107-117,
 * 184-198, 278-292).  Tensors are pushed one by one under their reference state_dict names, prefixed
 * by "G." / "plm." / "adm." / "hifigan."; `data` is a HOST pointer to `numel` f32 values (copied).
 * Additional tensors "pe.mrte" [max_positions, hidden], "pe.adm", "pe.plm": the sine tables of
 * modules/embedding.py:68-92 already multiplied by `alpha` (computed by the host mirror exactly
 * as the reference does).  finalize() checks the inventory strictly (load_state_dict(strict=True)),
 * repacks weights into GEMM-ready layouts and uploads them. */
mt2_model* mt2_model_create(const mt2_config* cfg);
int mt2_model_load_tensor(mt2_model* m, const char* name, const float* data /*host*/, const int64_t* shape /*host*/,
                          int ndim);
int mt2_model_finalize(mt2_model* m);
void mt2_model_destroy(mt2_model* m);
/* bytes of device memory held (weights, workspace) */
int mt2_model_memory(const mt2_model* m, size_t* weight_bytes, size_t* workspace_bytes);
/* ---- activation workspace.  The handle owns a bump arena over persistent hipMalloc chunks, reset by every call.
 * mt2_workspace_query: upper bound (bytes) of what ONE mt2_synthesize_batch call of this geometry takes (every
 * utterance at the maxima; flags as for mt2_synthesize_batch) - so that a server can pre-size the arena with
 * mt2_workspace_reserve and no hipMalloc happens on the hot path.  mt2_workspace_high_water: most bytes any call
 * has had in use so far. */
int mt2_workspace_query(const mt2_model* m, int B, int Np_max, int Tp_max, int Tm_cap, int flags, size_t* bytes);
int mt2_workspace_reserve(mt2_model* m, size_t bytes);
int mt2_workspace_high_water(const mt2_model* m, size_t* bytes);
/* test hooks: control and inspect what the arena holds.  A call resets the arena to offset 0 and never clears it, so the bytes it finds
 * there are the previous call's (or the driver's); no result may depend on them (tests/test_gpu_workspace_poison.py).  Both wait for
 * the handle's pending call, whatever stream it is on, and return with their own device work finished.
 * mt2_workspace_fill: every byte of every arena chunk (its whole size, used or not) := `byte` (0..255); capacity, high-water mark and
 * options are untouched.  mt2_workspace_peek: `bytes` arena bytes from `offset` -> `dst_host`; `offset` runs over the chunks in
 * allocation order; a range that leaves the capacity (mt2_model_memory) is an error. */
int mt2_workspace_fill(mt2_model* m, int byte);
int mt2_workspace_peek(mt2_model* m, size_t offset, void* dst_host /*host*/, size_t bytes);

/* ---- MRTE.tc_latent(phone, mel) (modules/mrte.py:154-171)
 * phone int64 [B, Np_max], mel f32 [B, Tp_max, mel_bins] -> out f32 [B, Np_max, hidden]. */
int mt2_mrte_tc_latent(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens /*host*/,
                       int Np_max, const float* mel, const int32_t* mel_lens /*host*/, int Tp_max, int B,
                       float* out);
/* the mel-encoder part alone (mrte.mel_encoder, modules/convnet.py:202-210): -> [B, Tc_max, hidden],
 * Tc = (T-1)/stride + 1 */
int mt2_mrte_mel_context(mt2_model* m, void* stream, const float* mel, const int32_t* mel_lens /*host*/,
                         int Tp_max, int B, float* out, int Tc_max);

/* ---- MegaADM.infer(tc_latents) (models/megatts2.py:257-275)
 * tc_latent f32 [B, Np_max, tc_dim] -> dur int32 [B, Np_max] (0 in padding); `dur_float` (optional, may
 * be NULL) receives the un-rounded predictions.  Asynchronous on `stream`. */
int mt2_adm_infer(mt2_model* m, void* stream, const float* tc_latent, const int32_t* lens /*host*/, int Np_max,
                  int B, int32_t* dur, float* dur_float);
/* The same loop started from a FORCED history (no reference counterpart; parity tests of long sequences): the
 * un-rounded predictions of the first P positions of every sequence are given (p_prefix f32 [B, P], device), the
 * loop continues at position P for `max_steps` positions (0 = to the end).  P = n-1, max_steps = 1 is exactly the
 * reference's step t = n-1 (models/megatts2.py:264-273) on that history. */
int mt2_adm_infer_forced(mt2_model* m, void* stream, const float* tc_latent, const int32_t* lens /*host*/,
                         int Np_max, int B, const float* p_prefix, int P, int max_steps, int32_t* dur,
                         float* dur_float);

/* ---- LengthRegulator.forward(x, duration_tokens) (modules/mrte.py:42-60)
 * x f32 [B, Np_max, D], dur int32 (HOST) [B, Np_max] -> out f32 [B, Tm_max, D] (zero rows beyond sum(dur_b)).
 * Durations are taken from the host because the output size depends on them (the reference also
 * moves them to the CPU, mrte.py:53). */
int mt2_length_regulate(mt2_model* m, void* stream, const float* x, const int32_t* dur /*host*/,
                        const int32_t* lens /*host*/, int Np_max, int D, int B, float* out, int Tm_max);

/* ---- F.max_pool1d(x.transpose(1,2), k, ceil_mode=True).transpose(1,2) (models/megatts2.py:357-358)
 * x f32 [B, T_max, D] -> out f32 [B, Tq_max, D], Tq = ceil(T/k). */
int mt2_max_pool_ceil(mt2_model* m, void* stream, const float* x, const int32_t* lens /*host*/, int T_max, int D,
                      int B, int k, float* out, int Tq_max);

/* ---- MegaPLM.infer(tc_latent) (models/megatts2.py:165-181)
 * cond f32 [B, Tq_max, tc_dim] -> codes int64 [B, Tq_max] (0 in padding); `last_logits` optional
 * f32 [B, Tq_max, bins] receives the logits of every step's last position. */
int mt2_plm_infer(mt2_model* m, void* stream, const float* cond, const int32_t* lens /*host*/, int Tq_max, int B,
                  int64_t* codes, float* last_logits);
/* Prompt-conditioned decoding in the layout the PLM is trained on (modules/datamodule.py:201-212: the prompt's
 * pooled tc_latents and VQ-PE prosody codes in FRONT of the target's, BOS first): cond f32 [B, P + Tq_max, tc_dim]
 * holds P prompt rows then the target rows, prefix_codes int64 [B, P] (device) the prompt's codes; the history
 * starts as [BOS, prefix...] and decoding continues at position P for `max_steps` positions (0 = all).  lens =
 * TARGET lengths; codes / last_logits receive the target positions only.  P = 0 is mt2_plm_infer. */
int mt2_plm_infer_prompted(mt2_model* m, void* stream, const float* cond, const int32_t* lens /*host*/, int Tq_max,
                           int B, const int64_t* prefix_codes, int P, int max_steps, int64_t* codes,
                           float* last_logits);

/* ---- seeded sampling of the PLM's prosody codes (no reference counterpart: the reference decodes greedily,
 * models/megatts2.py:165-181; greedy stays the default and the parity path).  Per step and utterance, over the vq_bins
 * logits z: rank order = value descending, index ascending; K = the first top_k (all when 0); w = exp((z - max z) /
 * temperature) on K; R = the shortest rank-order prefix of K holding top_p of sum_K w; the code is the first index of R,
 * walked in ascending index order, whose running sum of w exceeds u * sum_R w (the last index of R when rounding leaves
 * none).  u = (x0 >> 8) * 2^-24, x0 = the first word of Philox4x32-10 with key = the utterance's seed (lo, hi) and counter
 * = (target position, 0, 0, 0) - position 0 is the first code after the BOS and after any prompt prefix.  A code depends on
 * (seed, position, logits) only: batch, slot, stream groups and a repeated call do not change it.  top_k = 1 (or a tiny
 * top_p) is the greedy argmax exactly.  Invalid parameters (temperature <= 0 or not finite, top_k outside [0, vq_bins],
 * top_p outside (0, 1], reserved != 0, seeds == NULL) are an error before anything is launched. */
typedef struct mt2_sampling {
    float temperature;        /* > 0 */
    int32_t top_k;            /* 0 = all vq_bins */
    float top_p;              /* (0, 1]; 1 = off */
    int32_t reserved;         /* must be 0 */
    const uint64_t* seeds;    /* HOST, one per utterance of the call */
} mt2_sampling;
/* mt2_plm_infer_prompted with sampling (NULL: greedy, identical to mt2_plm_infer_prompted) */
int mt2_plm_infer_sampled(mt2_model* m, void* stream, const float* cond, const int32_t* lens /*host*/, int Tq_max, int B,
                          const int64_t* prefix_codes, int P, int max_steps, int64_t* codes, float* last_logits,
                          const mt2_sampling* sampling);

/* ---- prosody interpolation (Mega-TTS 2, section 3.3; no reference counterpart): the PLM decoded against TWO prosody prompts
 * at once - context A (the target speaker's) and context B (a second, "rhythmic" speaker's).  Per step and utterance, over the
 * two rows of vq_bins logits zA, zB, with gamma in [0, 1] and the temperature / top_k / top_p / u of mt2_sampling:
 *   wA_i = exp((zA_i - max zA) / temperature), SA = sum wA (same for B);
 *   m_i  = (1 - gamma) * wA_i / SA + gamma * wB_i / SB            (the mixture; sum m = 1 up to rounding);
 *   rank order = m descending, index ascending; K = the first top_k (all when 0); R = the shortest rank-order prefix of K
 *   with sum_R m >= top_p * sum_K m; the code is the first index of R, walked in ascending index order, whose running sum of m
 *   exceeds u * sum_R m (the last index of R when rounding leaves none).
 * Unlike the single-row rule, the rank order is decided on the COMPUTED f32 m, not on the logits (two logit rows have no
 * common order).  u is the same Philox4x32-10 draw: key = the utterance's seed, counter = (target position, 0, 0, 0); a code
 * depends on (seed, position, the two logit rows, gamma) only - not on the batch, the slot, the stream groups or a repeated
 * call.  The code is fed back to BOTH contexts.  gamma = 0 decodes context A alone, gamma = 1 context B alone.  sampling ==
 * NULL is greedy on the mixture: temperature 1, the arg-max of m with the lowest index on ties.
 * cond f32 [2, B, P + Tq_max, tc_dim] (context A, then context B: P prompt rows, then the target rows), prefix_codes int64
 * [2, B, P] (device; NULL when P = 0), gamma HOST f32 [B], lens = TARGET lengths; codes int64 [B, Tq_max] (0 in padding);
 * last_logits optional f32 [2, B, Tq_max, bins].  Invalid parameters (gamma NULL, NaN or outside [0, 1]; P > 0 without
 * prefix_codes; the mt2_sampling errors) are an error before anything is launched; prefix codes are range-checked like those of
 * mt2_plm_infer_prompted. */
int mt2_plm_infer_interpolated(mt2_model* m, void* stream, const float* cond, const int32_t* lens /*host*/, int Tq_max, int B,
                               const int64_t* prefix_codes, int P, const float* gamma /*host*/, int max_steps, int64_t* codes,
                               float* last_logits, const mt2_sampling* sampling);

/* ---- generator.vqpe.vq.decode(codes) (modules/quantization/vq.py:109-113)
 * codes int64 [n_q=1, B, Tq_max] -> out f32 [B, vq_dim, Tq_max]. */
int mt2_vq_decode(mt2_model* m, void* stream, const int64_t* codes, int B, int Tq_max, float* out);

/* ---- EuclideanCodebook.quantize (modules/quantization/core_vq.py:175-183): L2-argmin
 * x f32 [M, vq_dim] -> idx int64 [M] (lowest index on ties). */
int mt2_vq_quantize(mt2_model* m, void* stream, const float* x, int M, int64_t* idx);

/* ---- VQProsodyEncoder.forward(mel) (modules/vqpe.py:50-62), eval mode
 * mel f32 [B, T_max, mel_bins_full] (only the first vq_mel_bins are read) ->
 * zq f32 [B, T_max, vq_dim], codes int64 [1, B, Tq_max], ze (optional) f32 [B, Tq_max, vq_dim]. */
int mt2_vqpe_forward(mt2_model* m, void* stream, const float* mel, const int32_t* lens /*host*/, int T_max,
                     int mel_ld, int B, float* zq, int64_t* codes, int Tq_max, float* ze);

/* ---- generator.decoder(x) = ConvNet.forward (modules/convnet.py:115-119)
 * x f32 [B, decoder_in, T_max] ("B D T") -> mel f32 [B, mel_bins, T_max]. */
int mt2_mel_decoder(mt2_model* m, void* stream, const float* x, const int32_t* lens /*host*/, int T_max, int B,
                    float* mel);

/* ---- hifi_gan.decode_batch(mel) (speechbrain; models/megatts2.py:370): HiFi-GAN V1 generator
 * mel f32 [B, in_dim, T_max] -> wav f32 [B, 1, hop*(T_max + 2*hg_inference_padding)]; utterance b holds
 * hop*(len_b + 2*pad) samples (its own first / last frame replicated `pad` times, as
 * HifiganGenerator.inference does for a batch-1 call), zeros beyond. */
int mt2_hifigan(mt2_model* m, void* stream, const float* mel, const int32_t* lens /*host*/, int T_max, int B,
                float* wav);

/* ---- extract_mel_spec(samples) (modules/tokenizer.py:107-125): speechbrain `mel_spectogram` = torchaudio
 * Spectrogram(n_fft, win_length, hop_length, power=1, center=True, pad_mode="reflect", periodic Hann) ->
 * MelScale(n_mels, f_min, f_max, norm="slaney", mel_scale="slaney") -> log(clamp(x, clip)).
 * wav f32 [B, L_max] (16 kHz mono in the reference) -> mel f32 [B, T_max, n_mels], T_b = 1 + L_b / hop.
 * The STFT is an implicit conv on the GEMM engine: frame t = n_fft/hop consecutive hop-sized blocks of the
 * reflect-padded signal against a windowed DFT basis [2*(n_fft/2+1), n_fft].  n_fft % hop == 0, hop % 4 == 0. */
typedef struct mt2_audio_config {
    int32_t sample_rate, n_fft, hop_length, win_length, n_mels;
    float f_min, f_max, clip;
} mt2_audio_config;
int mt2_mel_spectrogram(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* wav,
                        const int32_t* lens /*host*/, int L_max, int B, float* mel, int T_max);

/* ---- prompt audio at any sample rate (models/megatts2.py:335-336: `librosa.load(wav, sr=16000)`, `librosa.util.normalize`).
 * librosa's soxr resampler is not reproduced (parity unpinned); the rule is the Kaiser-windowed-sinc polyphase filter in the form
 * torchaudio documents for resample(..., resampling_method="sinc_interp_kaiser") with its "kaiser_best" constants (lpw = 64 zero
 * crossings, rolloff = 0.9475937167399596, beta = 14.769656459379492), table arithmetic in double, rounded once to f32:
 *   g = gcd(sr_in, sr_out), o = sr_in / g, n = sr_out / g, base = min(o, n) * rolloff, width = ceil(lpw * o / base), taps = 2 width + o
 *   t[p][k] = clamp((-p / n + (k - width) / o) * base, -lpw, +lpw)
 *   h[p][k] = sinc(pi t) * I0(beta * sqrt(1 - (t / lpw)^2)) / I0(beta) * (base / o)
 *   y[i * n + p] = sum_{k < taps} h[p][k] * x[i * o - width + k]   (x = 0 outside [0, L); one f32 fma chain, k ascending)
 *   L_out = ceil(n * L / o)
 * so a sample depends on its utterance and the ratio alone, never on the batch around it.  Refused (error, never a clamp):
 * sr_in <= 0 or sr_out <= 0; sr_in == sr_out (nothing to do: do not call); a reduced ratio whose table n * taps * 4 bytes exceeds
 * 8 MiB (16001 -> 16000 would need about 8 GB) or whose taps exceed the kernel's 64 KiB window of on-chip memory; lens[b] < 1 or
 * > L_max; Lout_max < max_b L_out_b.  A refused call launches nothing and leaves `out` untouched. */
#define MT2_RESAMPLE_NORMALIZE 1 /* models/megatts2.py:336: y / max |y| per utterance in f32 (unchanged while the peak is below FLT_MIN) */
/* models/megatts2.py:335  the rule's integers for one pair of rates and one length; host only, no HIP call (outputs may be NULL) */
int mt2_resample_query(int sr_in, int sr_out, long long L, long long* L_out, int* o, int* n, int* taps);
/* models/megatts2.py:335  the f32 filter the device applies; host only, no HIP call */
int mt2_resample_table(int sr_in, int sr_out, float* table /*host, [n][taps] phase-major*/);
/* models/megatts2.py:335-336  wav f32 [B, L_max] (device) at sr_in -> out f32 [B, Lout_max] (device) at sr_out, zeros in
 * [L_out_b, Lout_max); samples beyond lens[b] are never read.  The filter table of a ratio is built and uploaded on the first call
 * that uses it (a synchronous copy) and kept in the handle; `m` may be a bare handle (no weights), as for mt2_mel_spectrogram. */
int mt2_resample(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                 int sr_in, int sr_out, int flags, float* out /*[B, Lout_max]*/, int Lout_max, int32_t* out_lens /*host, may be NULL*/);
/* models/megatts2.py:336  the normalisation alone, for audio that already has the model's rate: out[b, j] = wav[b, j] / max_j |wav[b, j]|
 * for j < lens[b] (same rule as MT2_RESAMPLE_NORMALIZE, same kernels), zeros in [lens[b], L_max).  out f32 [B, L_max] may be wav. */
int mt2_peak_normalize(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                       float* out);

/* ---- leading / trailing silence of prompt audio (models/megatts2.py:337: `librosa.effects.trim(y, top_db=20)`, commented out there
 * because its prompts are pre-cut; prepare_ds.py --trim_wav).  librosa is not on hand to compare with, so parity with it is unpinned,
 * as for the resampler; the rule is our own statement of what librosa documents for effects.trim with ref = np.max, centred frames
 * and zero padding, with the frame and hop FIXED (128 ms / 32 ms at 16 kHz; the hop is a multiple of the mel hop of 256, so every
 * cut falls on a mel-frame boundary).  For one utterance x[0 .. L), L >= 1:
 *   s[j] = sum of x[i]^2 over i in [512 j, 512 j + 512) and [0, L), in f32, j = 0 .. ceil(L / 512) - 1;  s[j] = 0 outside
 *   F = 1 + L / 512 frames;  e[f] = s[f - 2] + s[f - 1] + s[f] + s[f + 1]    (the zero-padded window [512 f - 1024, 512 f + 1024))
 *   E = max_f e[f];  c = (float)pow(10.0, -top_db / 10.0), computed in double and rounded once
 *   frame f is kept iff e[f] > E * c   (one f32 product: 10 log10(mse / max mse) > -top_db without the logarithm)
 *   start = 512 f_first,  end = min(L, 512 (f_last + 1)) over the kept frames (the frame holding E is kept, so end > start)
 *   E < FLT_MIN (all zeros, or squares that underflow): the utterance is left whole, start = 0, end = L - the convention of the peak
 *   normalisation, and unlike librosa, which returns an empty signal
 *   out[j] = x[start + j] for j < end - start, an exact copy; zeros up to Lout_max
 * The order of a block's sum depends on the sample's index in its utterance alone, so a batch is bit-identical to its utterances
 * trimmed one by one, energies included.  Input must be finite; a non-finite sample does not fault and still gives bounds inside
 * [0, L], nothing more.  Refused (error, nothing launched, `out` untouched): top_db not finite or <= 0; lens[b] < 1 or > L_max;
 * Lout_max < max_b lens[b] (the cut is not known before the call: size `out` for no trimming); F_max < 1 + max_b lens[b] / 512 while
 * `energy` is given; `out` overlapping `wav`. */
#define MT2_TRIM_FRAME 2048
#define MT2_TRIM_HOP 512
/* models/megatts2.py:337  F = 1 + L / 512 and the f32 factor c of one length and one top_db; host only, no HIP call (outputs may be NULL) */
int mt2_trim_query(long long L, float top_db, int* frames, float* factor);
/* models/megatts2.py:337  wav f32 [B, L_max] (device) -> out f32 [B, Lout_max] (device); samples beyond lens[b] are never read.
 * bounds (host, int32 [B][2] = start, end; may be NULL): the cut is found on the device and the copy reads it there, so only a
 * caller that asks for `bounds` pays for it - one copy of 2 B ints to the host and ONE stream synchronise inside the call, as
 * mt2_synthesize_batch does for the durations; with bounds == NULL the call only enqueues.  energy (device f32 [B, F_max], may be
 * NULL): e[f] of each utterance, zeros in [F_b, F_max).  Scratch comes from the handle's arena; `m` may be a bare handle. */
int mt2_trim_silence(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                     float top_db, float* out /*[B, Lout_max]*/, int Lout_max, int32_t* bounds /*host [B][2], may be NULL*/,
                     float* energy /*[B, F_max] or NULL*/, int F_max);

/* ---- dynamic time warping of one mel onto another (csrc/dtw.hip).  Megatts.align_prompt warps the model's own synthesis of the
 * prompt's phones onto the real prompt mel and carries the phone boundaries through the warp: the `prompt_durations` of
 * mt2_synthesize_prompt_conditioned without the Montreal Forced Aligner TextGrids the reference reads (prepare_ds.py,
 * utils/textgrid.py; out of scope here).  The same call is the DTW mel distance between two utterances.  The rule is our own, held
 * to its own restatement (tests/dtw_ref.py); alignment quality on real speech is unpinned.  Per utterance b, X f32 [Tx, D] (the
 * synthetic mel), Y f32 [Ty, D] (the real one), Tx, Ty >= 1, D >= 1 (80 in the model):
 *   cost        c[i, j] = sum_k (x[i, k] - y[j, k])^2 in f32, ONE chain over k ascending: acc = 0; d = x - y; acc = fmaf(d, d, acc).
 *               No split across lanes, no atomics, an order that does not depend on the tile: c depends on the two rows alone,
 *               and a ragged batch is bit-identical to its utterances alone.
 *   accumulate  one f32 add per cell: A[0, 0] = c[0, 0];  A[i, 0] = c[i, 0] + A[i-1, 0];  A[0, j] = c[0, j] + A[0, j-1];
 *               otherwise A[i, j] = c[i, j] + min(A[i-1, j-1], A[i-1, j], A[i, j-1])
 *   direction   diagonal if A[i-1, j-1] <= both others; else up (i-1, j) if A[i-1, j] <= A[i, j-1]; else left (i, j-1).
 *               Row 0 is always left, column 0 always up.  Given c, A and the directions are exactly reproducible in numpy float32.
 *   path        backtracked from (Tx-1, Ty-1) to (0, 0); reported as lo[j] / hi[j], the smallest / largest i on the path in column
 *               j.  Steps are (1,1), (1,0), (0,1), so lo[0] = 0, hi[Ty-1] = Tx-1, lo[j+1] in {hi[j], hi[j] + 1}: lo / hi hold the
 *               whole path.  steps = its number of cells, total = A[Tx-1, Ty-1].  Entries j >= Ty_b of lo / hi are -1.
 *   durations   synthetic durations s[p] >= 0 over Np phones, sum s = Tx, cum[p] = sum_{q<p} s[q]: real frame j belongs to the phone
 *               p with cum[p] <= hi[j] < cum[p+1]; dur[p] counts them = lower_bound(hi, cum[p+1]) - lower_bound(hi, cum[p]) (hi is
 *               non-decreasing); sum dur = Ty exactly.  A phone with s[p] = 0, or one swallowed by a vertical run, gets 0
 *               (mt2_synthesize_prompt_conditioned accepts zero durations).
 * Inputs must be finite; a non-finite value does not fault and still gives a path inside the matrix, nothing more.
 * Refused (error, nothing launched, outputs untouched - never a clamp or a silent band): B < 1 or D < 1; Tx_max or Ty_max outside
 * [1, MT2_DTW_MAX_LEN]; a length outside [1, its max]; B > 65535. */
#define MT2_DTW_MAX_LEN 4096        /* cap of Tx_max and Ty_max */
#define MT2_DTW_DIR_COLS 16         /* columns of 2-bit directions per u32 scratch word */
/* Arena bytes one mt2_dtw_align call of this geometry takes at most; host only, no HIP call.  With r(n) = n rounded up to 256:
 *   r(4 B ceil(Tx_max / 64) 64 ceil((Ty_max + 63) / 64) 64)  the costs in the skewed layout the accumulation reads (strips of 64
 *   rows, each 64 lanes wide over the Ty + 63 steps of its walk, in whole periods of 64; taken whether or not `cost` is given)
 *   + r(4 B Tx_max ceil(Ty_max / 16))  the packed directions  +  r(4 (2 B + 8))  the lengths' one upload */
int mt2_dtw_query(int Tx_max, int Ty_max, int D, int B, long long* workspace_bytes);
/* X f32 [B, Tx_max, D], Y f32 [B, Ty_max, D] (device; rows at or beyond x_lens[b] / y_lens[b] are never read) -> lo, hi int32
 * [B, Ty_max], steps int32 [B], total f32 [B] (device).  x_lens, y_lens: host int32 [B].  cost, acc (device f32 [B, Tx_max, Ty_max],
 * each may be NULL): c and A; cells outside an utterance's Tx_b x Ty_b are left untouched.  Scratch comes from the handle's arena;
 * `m` may be a bare handle.  The call only enqueues, it does not synchronise. */
int mt2_dtw_align(mt2_model* m, void* stream, const float* X, const int32_t* x_lens /*host*/, int Tx_max, const float* Y,
                  const int32_t* y_lens /*host*/, int Ty_max, int D, int B, int32_t* lo, int32_t* hi, int32_t* steps, float* total,
                  float* cost /*or NULL*/, float* acc /*or NULL*/);
/* The durations rule for a batch: hi int32 [B, Ty_max] (device, as mt2_dtw_align left it for these y_lens), syn_dur host int32
 * [B, Np_max] (entries at or beyond phone_lens[b] are ignored), phone_lens host int32 [B] -> dur_out_host int32 [B, Np_max], zeros at
 * or beyond phone_lens[b].  One copy to the host and ONE stream synchronise inside the call, as mt2_trim_silence does for its
 * bounds.  The x-length is not an argument: by the path rule it is hi[b, y_lens[b] - 1] + 1, which travels to the host in the same
 * copy, and sum_p syn_dur[b, p] is compared with it there.  Refused before anything is launched: B < 1, Np_max < 1, Ty_max outside
 * [1, MT2_DTW_MAX_LEN], a y-length outside [1, Ty_max], a phone count outside [1, Np_max], a negative synthetic duration, a sum
 * of them outside [1, MT2_DTW_MAX_LEN].  Refused behind the copy, with dur_out_host untouched: hi not covering Ty
 * (hi[b, y_lens[b] - 1] < 0, or the durations not summing to y_lens[b]), or sum_p syn_dur[b, p] != hi[b, y_lens[b] - 1] + 1. */
int mt2_align_durations(mt2_model* m, void* stream, const int32_t* hi, const int32_t* y_lens /*host*/, int Ty_max,
                        const int32_t* syn_dur /*host*/, const int32_t* phone_lens /*host*/, int Np_max, int B,
                        int32_t* dur_out_host);

/* ---- Mel-cepstral distortion along the DTW path (csrc/mcd.hip): how far one log-mel is from another of the same sentence, in dB, with
 * the F0 error and the voicing error along the SAME path - the spectral leg beside the pitch, prosody, rhythm and level measures.  No
 * counterpart in the reference.  This cepstrum is a DCT of an N-bin log-mel, NOT a mel-generalised cepstrum of a spectral envelope:
 * parity with SPTK / WORLD or with the ESPnet / Coqui MCD scripts is unpinned (none is on hand and they differ among themselves), and
 * the figures are comparable only with themselves.  The rule is our own, held to its float64 restatement tests/mcd_ref.py.  THE RULE,
 * for one pair A f32 [Ta, N], B f32 [Tb, N] of natural-log mels (as mt2_mel_spectrogram writes them), optionally f0_a f32 [Ta] and f0_b
 * f32 [Tb] frame-aligned to them;  N = n_mels in [2, 128], order K in [1, min(N - 1, MT2_MCD_MAX_ORDER)], 13 by convention:
 *  1 Table.  tab[k-1][m] = cos(pi (m + 1/2) k / N) / N, k = 1 .. K, m = 0 .. N-1, in double, rounded once to f32.  Under this scaling
 *    logmel[m] = c0 + 2 sum_k c_k cos(pi (m + 1/2) k / N), the convention under which (10 / ln 10) sqrt 2 turns cepstral differences
 *    into the RMS dB difference of the K-term-smoothed spectra.  c0, the level, is left out: a gain change is not distortion.
 *  2 Cepstrum.  c[t][k-1] = sum_m M[t][m] tab[k-1][m] in f32 as ONE fma chain over m ascending from 0; never split across lanes, no
 *    atomics.
 *  3 Warp.  The DTW rule above, unchanged, with X = the cepstra of A, Y = those of B, D = K: lo, hi, steps.  The path's cells are
 *    (i, j), lo[j] <= i <= hi[j], j < Tb.
 *  4 Per cell.  q = sum_k (ca[i][k] - cb[j][k])^2, exactly the DTW's cost chain;  dB(i, j) = (10 / ln 10) sqrt(2 (double) q) in double.
 *  5 F0 along the path, only when both tracks are given.  A frame is voiced iff f0 > 0 (a NaN is not).  On a cell voiced on both
 *    sides D = 1200 log2((double) f0_a[i] / (double) f0_b[j]) cents;  a cell voiced on exactly one side is a voicing error.
 *  6 Sums, in double, in an order that depends on the frame index in the utterance alone: one workgroup of 256 threads per utterance,
 *    thread t takes the columns j = t, t + 256, ... ascending and in a column i ascending, one add per term;  the 256 partial sums meet
 *    in a fixed tree (stride 128 .. 1), the maximum likewise.  A ragged batch is bit-identical to its utterances alone, whatever the
 *    slot and the padded lengths.
 *  7 Row of MT2_MCD_FIELDS = 8 doubles:  0 cells (= steps)   1 MCD = mean of dB over the cells   2 largest cell dB   3 cells voiced
 *    on both sides   4 sqrt(mean D^2) in cents over those (0 if field 3 is 0)   5 mean D in cents, signed: the register offset
 *    6 cells voiced on exactly one side   7 field 6 / field 0.  Fields 3-7 are 0 without F0 tracks.
 * A non-finite input cannot fault, write outside the outputs or change another utterance's row;  nothing more is promised for its own.
 * Refused, on the host before the first HIP call, every output as it was - never a clamp:  B outside [1, 65535];  N or K outside their
 * ranges;  a length outside [1, its max];  a max over MT2_DTW_MAX_LEN;  one F0 track without the other;  overlapping buffers.
 * `m` may be a bare handle;  scratch comes from its arena;  the table is built and uploaded once per (N, K) and handle.  Every call only
 * enqueues. */
#define MT2_MCD_FIELDS 8
#define MT2_MCD_MAX_ORDER 32
/* the table f32 [order][n_mels] of rule 1;  host only, no HIP call */
int mt2_mcd_table(int n_mels, int order, float* table /*host [order][n_mels]*/);
/* Arena bytes of one mt2_mel_cepstral_distortion call of this geometry - exactly its high water;  host only, no HIP call.  With r(n) =
 * max(256, n rounded up to 256):  r(4 (4 ceil(B / 4) + B))  both lengths  +  the skewed costs and the packed directions that
 * mt2_dtw_query states for (Ta_max, Tb_max)  +  r(4 B Ta_max K) + r(4 B Tb_max K)  the cepstra  +  2 r(4 B Tb_max)  lo and hi
 * +  2 r(4 B)  steps and total. */
int mt2_mcd_query(int Ta_max, int Tb_max, int n_mels, int order, int B, long long* workspace_bytes);
/* Rule 2 for a ragged batch:  mel f32 [B, T_max, n_mels] (device; rows at or beyond frame_lens[b] are never read), frame_lens host
 * int32 [B] -> cep f32 [B, T_max, order] (device), zeros in the rows at or beyond frame_lens[b]. */
int mt2_mel_cepstrum(mt2_model* m, void* stream, const float* mel /*[B, T_max, n_mels]*/, const int32_t* frame_lens /*host*/, int T_max,
                     int B, int n_mels, int order, float* cep /*[B, T_max, order]*/);
/* Rules 4-7 on a path the caller supplies:  ca f32 [B, Ta_max, order], cb f32 [B, Tb_max, order], lo, hi int32 [B, Tb_max] (device, as
 * mt2_dtw_align leaves them;  whatever they hold, a column's run is cut to the rows [0, a_lens[b]) and only the columns below b_lens[b]
 * are walked), f0_a f32 [B, Ta_max] and f0_b f32 [B, Tb_max] (device; both or neither) -> out f64 [B, 8] (device). */
int mt2_path_distortion(mt2_model* m, void* stream, const float* ca, const int32_t* a_lens /*host*/, int Ta_max, const float* cb,
                        const int32_t* b_lens /*host*/, int Tb_max, int order, int B, const int32_t* lo, const int32_t* hi,
                        const float* f0_a /*or NULL*/, const float* f0_b /*or NULL*/, double* out /*f64 [B, 8]*/);
/* The whole chain in one call on the arena: both cepstra, the DTW on them, the path reduction.  mel_a f32 [B, Ta_max, n_mels], mel_b f32
 * [B, Tb_max, n_mels] (device) -> out f64 [B, 8] and, on request, the path lo, hi int32 [B, Tb_max] (device; -1 at or beyond b_lens[b]). */
int mt2_mel_cepstral_distortion(mt2_model* m, void* stream, const float* mel_a, const int32_t* a_lens /*host*/, int Ta_max,
                                const float* mel_b, const int32_t* b_lens /*host*/, int Tb_max, int n_mels, int order, int B,
                                const float* f0_a /*or NULL*/, const float* f0_b /*or NULL*/, double* out /*f64 [B, 8]*/,
                                int32_t* lo /*or NULL*/, int32_t* hi /*or NULL*/);

/* ---- Griffin-Lim vocoder (csrc/griffinlim.hip): log-mel -> audio with no weights, the fallback behind mt2_hifigan (whose weights are a
 * third-party hub model) and a debugging aid - intelligible but buzzy, not a replacement.  No counterpart in the reference; parity with
 * librosa.griffinlim / torchaudio.transforms.GriffinLim is unpinned, the rule is our own, held to tests/griffinlim_ref.py.  With the
 * audio configuration's n_fft N, hop h, F = N / 2 + 1, taps = N / h >= 2, S = 2 F rounded up to 4, Fp = F rounded up to 4, w the
 * front-end's window, for one utterance with log-mel M f32 [T, n_mels] and a 64-bit seed; output x f32 [L], L = (T - 1) h (the exact
 * inverse of the front-end's framing: 1 + L / h = T, no inference padding):
 *   mel -> linear  P = fb^T (fb fb^T)^-1 by Cholesky in double from the f32 filterbank fb, rounded once to f32;
 *                  A[t, f] = max(0, sum_j expf(M[t, j]) P[f, j]).  A Gram matrix that is not positive definite is refused
 *                  (n_fft 64 with 80 mels: 32 filters cover no bin).
 *   phase          u = (x0 >> 8) 2^-24, x0 the first word of Philox4x32-10 with key = seed and counter (t F + f, 0, 0, 0) - the generator
 *                  of mt2_sampling; theta = 2 pi u in f32; S0[t, f] = A[t, f] (cos theta, sin theta).
 *   inverse STFT   y_t = irfft_N(S_t) w (imaginary parts of bins 0 and N / 2 ignored), a GEMM against a basis built in double and
 *                  rounded once; s[p] = sum_t y_t[p - t h], e[p] = sum_t w2[p - t h] over the existing frames 0 <= t < T covering p, in
 *                  ascending t, plain f32 adds, w2 = w^2 rounded once from double; x[n] = s[n + N/2] / e[n + N/2]
 *                  (torch.istft, center=True, length = (T - 1) h).  No atomics, no sum split across lanes.
 *   forward STFT   exactly mt2_mel_spectrogram's before its magnitude.
 *   iteration      c = (float)(momentum / (1 + momentum)), Rprev = 0; for k < n_iter: x_k = istft(S_k), R = stft(x_k), D = R - c Rprev,
 *                  S_{k+1} = D (A / (|D| + 1e-16)), Rprev = R; x = istft(S_{n_iter}).  n_iter = 0: the inverse STFT of S0.
 *   residual       resid[k, t] = sum_f (|R_k[t, f]| - A[t, f])^2 for k = 0 .. n_iter (entry n_iter costs one extra STFT of x; paid only
 *                  when the buffer is given); spectral convergence of round k = sqrt(sum_t resid[k, t] / sum A^2), left to the caller.
 * A sample, a frame and a residual depend on their utterance alone and the two large GEMMs run on one fixed f32 tile whatever the row
 * count, so a ragged batch is bit-identical to its utterances alone.  Both GEMMs stay on the f32 MFMA tiles (their bases are not in
 * the weight store and have no fp16 planes): exp(M) beyond the fp16 range is an ordinary number and mt2_x3h_guard is not involved.
 * Refused (error, nothing launched, outputs untouched): B < 1; n_iter < 0; momentum outside [0, 1); a T_b outside
 * [N / (2 h) + 2, T_max] (the reflect padding needs L_b > N / 2); L_max < (max T_b - 1) h; taps < 2; the rank-deficient filterbank.
 * Frames at or beyond T_b are never read, NaN included.  `m` may be a bare handle; the constants of a configuration are built on the
 * first call that needs them (a synchronous copy) and kept in the handle; scratch comes from the handle's arena. */
/* wav f32 [B, L_max] (device), lens host -> spec f32 [B, T_max, S] (device): frame t = [re(0..F-1) | im(0..F-1) | zero pad], T_b =
 * 1 + L_b / h, zeros in frames at or beyond T_b.  The same launches and refusals as mt2_mel_spectrogram up to its magnitude. */
int mt2_stft(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* wav, const int32_t* lens /*host*/, int L_max, int B,
             float* spec, int T_max);
/* spec f32 [B, T_max, S] in mt2_stft's layout (pad columns are not read), frame_lens host int32 [B] -> wav f32 [B, L_max]:
 * (T_b - 1) h samples, zeros beyond.  Refusals as mt2_griffin_lim's for the lengths.  The call only enqueues. */
int mt2_istft(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* spec, const int32_t* frame_lens /*host*/, int T_max,
              int B, float* wav, int L_max);
/* mel f32 [B, T_max, n_mels] -> mag f32 [B, T_max, Fp] = A, zeros in columns F .. Fp - 1 and in frames at or beyond mel_lens[b]
 * (1 <= mel_lens[b] <= T_max). */
int mt2_mel_to_linear(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* mel, const int32_t* mel_lens /*host*/, int T_max,
                      int B, float* mag);
/* Arena bytes and output length of one mt2_griffin_lim call; host only, no HIP call (outputs may be NULL; mel_lens NULL: every T_b =
 * T_max).  It refuses what mt2_griffin_lim refuses, the rank-deficient filterbank included.  With r(n) = n rounded up to 256, q(n) = n rounded up
 * to 4, Fr = sum_b T_b, Rb = sum_b (T_b - 1 + taps):
 *   r(4 (2 q(Rb) + 4 q(Fr) + 2 q(B) + (want_resid ? q(2 B) + Fr : 2 B)))   the call's one upload of row maps, lengths and seeds
 *   + r(4 Fr n_mels) + r(4 Fr Fp) + 3 r(4 Fr S) + r(4 Fr N) + r(4 Rb h)     exp(M), A, S / R / Rprev, the frames, the block buffer
 * L_out = (max_b T_b - 1) h. */
int mt2_griffin_lim_query(const mt2_audio_config* ac, const int32_t* mel_lens /*host or NULL*/, int T_max, int B, int n_iter,
                          double momentum, int want_resid, long long* workspace_bytes, long long* L_out);
/* mel f32 [B, T_max, n_mels] (device), mel_lens host int32 [B], seeds host uint64 [B] -> wav f32 [B, L_max] (device): (T_b - 1) h
 * samples, zeros beyond.  resid (device f32 [B, n_iter + 1, T_max] or NULL): the residual rows, zeros at or beyond T_b.  Stage
 * events (mt2_set_profiling): gl_setup, gl_iterations, gl_final.  The call only enqueues, it does not synchronise. */
int mt2_griffin_lim(mt2_model* m, void* stream, const mt2_audio_config* ac, const float* mel, const int32_t* mel_lens /*host*/, int T_max,
                    int B, int n_iter, double momentum, const uint64_t* seeds /*host*/, float* wav, int L_max, float* resid /*or NULL*/);

/* ---- Stationary-noise suppression for prompt audio (csrc/denoise.hip): a per-bin quantile noise floor and a spectral gate between
 * mt2_stft and mt2_istft - hiss, room tone or mains hum under a prompt is otherwise copied into the generated speech.  No counterpart in
 * the reference.  Parity with any outside denoiser (noisereduce, RNNoise, Audacity) is unpinned, and so is audible quality on real
 * speech: the test signals are analytic and the weights synthetic.  The rule is our own, held to tests/denoise_ref.py.  Out of scope:
 * non-stationary noise tracking, a streaming form, multichannel; de-reverberation is a stage of its own, mt2_dereverb below, and runs in
 * front of this one.  THE RULE, for one utterance x[0 .. L) with the audio
 * configuration's N = n_fft, h = hop, F = N / 2 + 1, Fp and S as above, T = 1 + L / h frames, and the parameters of mt2_denoise_config:
 *  1 Spectrum.  S = mt2_stft(x), exactly that call on this utterance alone: in a batch the STFT GEMM is launched per utterance, so that
 *    its tile is the one the utterance's own row count chooses.
 *  2 Power.  P[t, f] = fmaf(im, im, re re) in f32, f < F.
 *  3 Noise floor (quantile-based noise estimation, Stahl, Fischer and Bippus 2000: a bin is speech-free in at least `percentile` % of
 *    the frames).  k = ((T - 1) percentile + 50) / 100 in integers (the rank rule of mt2_loudness_ebu);  q[f] = the value of rank k
 *    (0-based, ascending) among P[0 .. T, f], selected exactly - P >= 0, so the f32 bit pattern orders as an unsigned integer, and a
 *    radix select is order-free: no sum;  c = (float)(1 / -ln(1 - percentile / 100)), in double, rounded once;  Nf[f] = q[f] c, one f32
 *    product.  c turns the quantile of an exponentially distributed periodogram bin into its mean: for white Gaussian noise of variance
 *    s^2 the expectation is Nf[f] = s^2 sum w^2 for 0 < f < N / 2.
 *  4 Gain.  g0[t, f] = P > 0 ? max(g_min, (P - beta Nf[f]) / P) : g_min - one f32 product, one subtraction, one true f32 division, one
 *    max (a NaN quotient takes g_min).
 *  5 Smoothing against musical noise, f32 sums in ascending order divided by the count of existing cells:  g1[t, f] = mean of g0[t, f']
 *    over f' in [f - bf, f + bf] and [0, F);  g[t, f] = mean of g1[t', f] over t' in [t - bt, t + bt] and [0, T).  Pad columns F .. Fp-1
 *    and frames at or beyond T never enter a mean and are never read.
 *  6 Apply.  S'[t, f] = g S[t, f], real and imaginary part each one f32 product, pad columns as mt2_stft wrote them;  y = mt2_istft(S'),
 *    exactly that call:  (T - 1) h = h (L / h) samples, zeros beyond - up to h - 1 tail samples are dropped, the Griffin-Lim convention.
 *  7 Figures, a row of MT2_DENOISE_FIELDS = 8 doubles:  0 noise power 10 log10(sum_f Nf) in dB   1 estimated SNR
 *    10 log10(max(sum P / T - sum Nf, DBL_MIN) / sum Nf)   2 the share of cells with g0 == g_min   3 the reduction
 *    10 log10(sum g^2 P / sum P)   4 T   5 k   6 sum P / T   7 sum_f Nf.  Sums in double: a tile of 16 frames by 64 bins is summed by
 *    256 threads, each its own cells in ascending order, then a fixed tree;  the tiles likewise - an order that depends on the cell's
 *    index in its utterance alone.
 * A sample and a figure depend on their utterance alone: a ragged batch is bit-identical to its utterances alone.  Non-finite input
 * does not fault and promises nothing more.
 * TWO CONSEQUENCES.  A STEADY tone is stationary and is removed like hum: the estimator cannot tell it from noise.  Speech present in a
 * bin for more than 100 - percentile % of the frames raises that bin's floor (at percentile 50 a tone gated on half the time is
 * attenuated, not cleaned).
 * Refused, on the host, with nothing launched and every output as it was:  a parameter outside its range or not finite;  B outside
 * [1, 65535];  for mt2_denoise a T_b outside what mt2_istft accepts (N / (2 h) + 2 <= T_b), for the other two a frame count outside
 * [1, T_max];  a T_max over MT2_DENOISE_MAX_FRAMES;  Lout_max < (max T_b - 1) h;  `out` overlapping `wav`, any output overlapping an
 * input (mt2_spectral_gain's spec_out may BE spec).  `m` may be a bare handle;  scratch comes from its arena;  every call only enqueues. */
#define MT2_DENOISE_FIELDS 8
#define MT2_DENOISE_MAX_FRAMES 16384
typedef struct mt2_denoise_config {
    int32_t percentile;        /* [1, 99];  20 */
    float over_subtraction;    /* beta > 0, finite;  3.0 */
    float floor_gain;          /* g_min in (0, 1];  0.1 = -20 dB */
    int32_t smooth_bins;       /* bf in [0, 8];  1 */
    int32_t smooth_frames;     /* bt in [0, 8];  1 */
    int32_t reserved;          /* 0 */
} mt2_denoise_config;
/* Arena bytes of one mt2_denoise call (exactly its high water), its output length, and k and c for the longest utterance;  host only, no
 * HIP call;  outputs may be NULL;  lens NULL: every L_b = L_max.  It refuses what mt2_denoise refuses for these arguments.  With r(n) =
 * max(256, n rounded up to 256), q(n) = n rounded up to 4, taps = N / h, T_b = 1 + L_b / h, Fr = sum_b T_b, Rb = sum_b (T_b - 1 + taps),
 * tiles = ceil(max T_b / 16) ceil(F / 64):
 *   r(4 (2 q(Rb) + q(B) + 2 q(Fr) + q(B) + B))  the call's one upload of block and row maps and lengths
 *   + r(4 Rb h) + r(4 Fr S) + r(4 Fr Fp) + r(4 B Fp) + r(24 B tiles) + r(4 Fr N)   blocks, spectrum, P, Nf, tile sums, frames
 * L_out = (max_b T_b - 1) h. */
int mt2_denoise_query(const mt2_audio_config* ac, const mt2_denoise_config* dc, const int32_t* lens /*host or NULL*/, int L_max, int B,
                      long long* workspace_bytes, long long* L_out, int* rank, float* factor);
/* Rules 2-3 on a spectrum the caller supplies:  spec f32 [B, T_max, S] in mt2_stft's layout (device; pad columns and frames at or beyond
 * frame_lens[b] are never read), frame_lens host int32 [B] -> floor f32 [B, Fp] (device), zeros in the columns F .. Fp-1.  On a
 * noise-only clip this is a noise profile that mt2_denoise and mt2_spectral_gain take instead of their own rule 3. */
int mt2_noise_floor(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_denoise_config* dc, const float* spec,
                    const int32_t* frame_lens /*host*/, int T_max, int B, float* floor /*[B, Fp]*/);
/* Rules 2 and 4-6 on a spectrum and a floor the caller supplies -> gain f32 [B, T_max, Fp] (device or NULL;  zeros in the pad columns and
 * in the frames at or beyond frame_lens[b]) and / or the gated spectrum spec_out f32 [B, T_max, S] (device or NULL;  it may be `spec`
 * itself: then pad columns and frames at or beyond frame_lens[b] stay as they were, else they are zero).  At least one output. */
int mt2_spectral_gain(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_denoise_config* dc, const float* spec,
                      const int32_t* frame_lens /*host*/, int T_max, int B, const float* floor /*[B, Fp]*/, float* gain /*or NULL*/,
                      float* spec_out /*or NULL*/);
/* The whole rule:  wav f32 [B, L_max] (device; samples at or beyond lens[b] are never read), lens host int32 [B] -> out f32
 * [B, Lout_max] (device):  (T_b - 1) h samples, zeros beyond.  floor_in (device f32 [B, Fp] or NULL): the caller's floor instead of
 * rule 3.  floor_out (device f32 [B, Fp] or NULL): the floor that was used.  figures (device f64 [B, 8] or NULL).  Stage events
 * (mt2_set_profiling): dn_stft, dn_floor, dn_gain, dn_istft. */
int mt2_denoise(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_denoise_config* dc, const float* wav,
                const int32_t* lens /*host*/, int L_max, int B, const float* floor_in /*or NULL*/, float* floor_out /*or NULL*/,
                double* figures /*or NULL*/, float* out, int Lout_max);

/* ---- De-reverberation of prompt audio by weighted prediction error (csrc/wpe.hip): single-channel WPE (Nakatani et al. 2010; Yoshioka
 * and Nakatani 2012) between mt2_stft and mt2_istft - the room of a phone or laptop recording is otherwise copied into the generated
 * voice as hiss was.  It needs no weights.  No counterpart in the reference.  Parity with nara_wpe or any other implementation is
 * unpinned, because none is on hand, and so is audible quality on real speech: the test signals are analytic.  The rule is our own, held
 * to tests/wpe_ref.py.  Out of scope: multichannel WPE, a streaming (RLS) form, joint WPE and denoising, neural variance estimators.
 * THE RULE, for one utterance and one bin f < F;  Y[t], t < T, is the bin's complex STFT column, read from the f32 spectrum and widened
 * to double;  D, K, I, c, eps, load are the parameters of mt2_wpe_config;  all arithmetic is in double.
 *  1 x_k[t] = Y[t - D - k] for k < K, 0 where the index is negative.  Set E = Y (E is the de-reverberated column).
 *  2 Repeat I times:
 *    2.1 P[t] = the mean of |E[t']|^2 over t' in [t - c, t + c] and [0, T), summed in ascending order and divided by the count.
 *    2.2 lambda[t] = max(P[t], eps max_t P[t]) (fmax: a NaN never wins);  w[t] = 1 / lambda[t], one division.  If max P is 0 or not
 *        finite the bin PASSES THROUGH (E = Y) and the loop ends.
 *    2.3 R[j][k] = sum_t (x_j[t] w[t]) conj(x_k[t]),  p[j] = sum_t (x_j[t] w[t]) conj(Y[t]).  Order: lane l of 64 adds its frames l,
 *        l + 64, ... in ascending order, then the 64 partial sums meet in the butterfly of strides 32, 16 .. 1 - an order that depends
 *        on t and T alone.  No atomics.
 *    2.4 R[j][j] += load tr(R) / K, tr(R) summed in ascending j.
 *    2.5 Cholesky R = L L^H without pivoting, a column at a time, each entry R[i][j] minus its products in ascending order.  If a pivot
 *        is <= 0 or not finite the bin passes through (E = Y) and the loop ends.
 *    2.6 g = R^-1 p by the two triangular solves, then E[t] = Y[t] - sum_k conj(g[k]) x_k[t], k ascending.
 *  3 Each part of E is rounded to f32 once.  A bin that passed through comes back bit for bit.
 * mt2_dereverb is mt2_stft on each utterance alone (rule 1 of mt2_denoise, word for word), steps 1-3 per bin, then mt2_istft:  (T - 1) h
 * samples, zeros beyond - up to h - 1 tail samples are dropped, as mt2_denoise does.  A clip too short to estimate K taps passes through
 * unfiltered there:  T_b < D + 4 K gives E = Y for every bin (a 10-tap filter fitted on 4 - 14 frames damages clean audio by 4 - 10 dB).
 * mt2_wpe_spectrum applies steps 1-3 at any T >= 1 (at T <= D every regressor is zero, the first pivot is 0 and every bin passes through).
 * Figures, a row of MT2_WPE_FIELDS = 8 doubles:  0 sum |Y|^2   1 sum |E|^2 (of the f32 output)   2 10 log10([1] / [0])   3 T   4 bins
 * filtered   5 bins passed through   6 max over f, k of |g|   7 the iterations completed by the bin that ran longest.  Sums: a bin's
 * frames by 512 threads, each its own in ascending order, then a fixed tree;  the bins likewise by 256 threads (mt2_denoise's order).
 * A sample, a filter and a figure depend on their utterance alone: a ragged batch is bit-identical to its utterances alone.  Non-finite
 * input neither faults nor hangs - every loop has a fixed trip count - and promises nothing more.
 * CONSEQUENCES.  Diffuse tails are helped only modestly (white noise under an exponential decay: late / early ratio -6.5 -> -9.6 dB at
 * T60 0.6 s, -12.8 -> -13.8 dB at 0.3 s); discrete reflections are removed well.  A STEADY tone is predictable from its own past and is
 * removed like a reflection.  Clean gated noise comes out slightly distorted (about -28 dB from itself).  Real speech is unpinned.
 * Refused, on the host, with nothing launched and every output as it was:  a parameter outside its range or not finite;  B outside
 * [1, 65535];  for mt2_dereverb a T_b outside what mt2_istft accepts (N / (2 h) + 2 <= T_b), for mt2_wpe_spectrum a frame count outside
 * [1, T_max];  a T_max over MT2_WPE_MAX_FRAMES;  Lout_max < (max T_b - 1) h;  an output overlapping an input or another output
 * (mt2_wpe_spectrum's spec_out may BE spec);  spectra not on 16 bytes.  `m` may be a bare handle;  scratch comes from its arena;  every
 * call only enqueues. */
#define MT2_WPE_FIELDS 8
#define MT2_WPE_MAX_FRAMES MT2_DENOISE_MAX_FRAMES
typedef struct mt2_wpe_config {
    int32_t delay;             /* D in [1, 8];  3: frames skipped before the prediction - the direct sound and the window overlap */
    int32_t taps;              /* K in [1, 16];  10 */
    int32_t iterations;        /* I in [1, 8];  3 */
    int32_t context;           /* c in [0, 4];  1: the variance is averaged over +-c frames */
    double variance_floor;     /* eps in (0, 1];  1e-2, relative to the bin's largest variance */
    double loading;            /* load in [0, 1e-2];  1e-8 */
    int32_t reserved;          /* 0 */
} mt2_wpe_config;
/* Arena bytes of one mt2_dereverb call (exactly its high water) and its output length;  host only, no HIP call;  outputs may be NULL;
 * lens NULL: every L_b = L_max.  It refuses what mt2_dereverb refuses for these arguments.  With r, q, taps, T_b, Fr, Rb as for
 * mt2_denoise_query and C = sum_b F q(T_b) complex cells:
 *   r(4 (2 q(Rb) + q(B) + 2 q(Fr) + 3 q(B) + B))  the call's one upload of block, row and column maps, lengths and pass-through flags
 *   + r(4 Rb h) + r(4 Fr S) + 2 r(8 C) + r(40 B F) + r(4 Fr N)   blocks, spectrum, the columns of Y and of E, the bins' sums, frames
 * L_out = (max_b T_b - 1) h. */
int mt2_dereverb_query(const mt2_audio_config* ac, const mt2_wpe_config* wc, const int32_t* lens /*host or NULL*/, int L_max, int B,
                       long long* workspace_bytes, long long* L_out);
/* Steps 1-3 on a spectrum the caller supplies:  spec f32 [B, T_max, S] in mt2_stft's layout (device, on 16 bytes;  frames at or beyond
 * frame_lens[b] are never read, pad columns never enter a result), frame_lens host int32 [B] -> spec_out f32 [B, T_max, S] (device;  it
 * may be `spec` itself: then pad columns and frames at or beyond frame_lens[b] stay as they were, else they are zero).  filters (device
 * f64 [B, Fp, K, 2] or NULL): g of every bin, re and im;  zeros for a bin that passed through and in the rows F .. Fp-1.  figures
 * (device f64 [B, 8] or NULL).  Its arena: r(4 (3 q(B) + B)) + 2 r(8 C) + r(40 B F). */
int mt2_wpe_spectrum(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_wpe_config* wc, const float* spec,
                     const int32_t* frame_lens /*host*/, int T_max, int B, float* spec_out /*may be spec*/, double* filters /*or NULL*/,
                     double* figures /*or NULL*/);
/* The whole rule:  wav f32 [B, L_max] (device; samples at or beyond lens[b] are never read), lens host int32 [B] -> out f32
 * [B, Lout_max] (device):  (T_b - 1) h samples, zeros beyond.  figures (device f64 [B, 8] or NULL).  Stage events (mt2_set_profiling):
 * dr_stft, dr_wpe, dr_istft. */
int mt2_dereverb(mt2_model* m, void* stream, const mt2_audio_config* ac, const mt2_wpe_config* wc, const float* wav,
                 const int32_t* lens /*host*/, int L_max, int B, double* figures /*or NULL*/, float* out, int Lout_max);

/* ---- Declipping of prompt audio by sparsity (csrc/declip.hip): A-SPADE (Kitic, Bertin and Gribonval 2015; the analysis variant in the
 * declipping survey of Zaviska, Rajmic, Ozerov and Rencker 2021) - a prompt recorded too hot has flat tops, the mel front end sees their
 * harmonic distortion and the timbre encoder reproduces it.  It needs no weights.  No counterpart in the reference.  Parity with any
 * outside declipper is unpinned, because none is on hand, and so is audible quality on real speech: the test signals are analytic.  The
 * rule is our own, held to tests/declip_ref.py.  It runs at the audio's OWN sample rate, in front of any resampling or normalisation:
 * both turn flat tops into ripple that nothing can recognise as clipping.  Out of scope: redundant (zero-padded) frames, S-SPADE,
 * social-sparsity shrinkage, soft-clip models, a streaming form, multichannel.
 * THE RULE, for one utterance y[0 .. len) (f32) and the parameters of mt2_declip_config;  N = frame, hop = N / 4, K = N / 2 + 1.
 *  1 Detection, every comparison in f32, the counts integers.  hi = max y, lo = min y (fmax / fmin: a NaN never wins);  with `level`
 *    set hi = (f32)level, lo = -hi.  n_hi = #{y >= hi - tol |hi|} if hi > 0, else 0;  n_lo = #{y <= lo + tol |lo|} if lo < 0, else 0
 *    (the product and the sum each rounded to f32, never fused).  A side is CLIPPED iff its count >= max(min_count, ceil(min_share len))
 *    (the ceiling in double).  A sample is H (at or over the high threshold of a clipped high side), L (likewise low) or reliable.  An
 *    utterance with no clipped side, or with a sample that is not finite, PASSES THROUGH bit for bit.
 *  2 Frames.  The utterance is zero-padded by N - hop in front and up to a multiple of hop plus N - hop behind:  T = ceil(len / hop) + 3
 *    frames, frame t holding the samples t hop - 3 hop + n, n < N, so that every sample lies in exactly four frames;  pad samples are
 *    reliable zeros.  w[n] = sqrt(0.5 - 0.5 cos(2 pi n / N)) is the analysis and the synthesis window;  F = (double)y w.
 *  3 Per frame, in double;  A is the N-point real DFT scaled by 1 / sqrt(N), on the half spectrum of K bins (inner bins count twice in
 *    norms).  If |F| = 0, or the frame has no H or L sample, or NONE of the utterance's own samples in it is reliable (pads anchor
 *    nothing: a stretch that is clipped throughout, a square wave, comes back as it is), x = F and the frame does not iterate.
 *    Otherwise x = F, u = 0, k = step, and for i = 1 .. max_iter (0: every ceil(K / step)):
 *      v = A x + u;  zb keeps every bin whose |v|^2 >= the min(k, K)-th largest |v|^2 of the half spectrum, exactly - ties at the
 *      threshold are all kept, so the rule has no order dependence;  x = proj(A^H (zb - u)), where proj sets reliable samples to F and
 *      takes max(., F) on H and min(., F) on L;  d = A x - zb;  stop if |d| <= eps |F|;  otherwise u += d, and if i mod every = 0 then
 *      k += step.
 *    The transform is the library's own real FFT (an N / 2 point complex radix-2 in LDS; tests/declip_ref.py restates its order);  |v|^2
 *    is fma(re, re, im im);  norms are summed by 256 threads, each its bins t, t + 256, .. in ascending order, then a fixed tree.
 *  4 Synthesis.  s = sum_t x_t w / sum_t w^2 over the sample's four frames in ascending order (the sum of w^2 is 2 in exact arithmetic;
 *    the actual sum divides), rounded to f32 once.  A reliable sample is written as the INPUT'S OWN BITS, an H sample as max(s, y), an L
 *    sample as min(s, y): consistency with the clipped recording is exact in f32.  The output can exceed the input's peak - that is the
 *    point - and the caller normalises after.
 * Figures, a row of MT2_DECLIP_FIELDS = 8 doubles:  0 clipped (0 / 1)   1 hi   2 lo   3 the share of samples that are H or L   4 frames
 * iterated   5 mean iterations over those frames   6 the largest iteration count   7 10 log10(sum out^2 / sum y^2).  mt2_clip_detect
 * fills 0-3 and leaves 4-7 zero;  so does mt2_declip for an utterance that passes through.  A non-finite utterance reads 0, NaN, NaN, 0 ...
 * A sample, a frame and a figure depend on their utterance alone: a ragged batch is bit-identical to its utterances alone.  Every loop
 * has a trip count fixed by N, len and max_iter: non-finite values can neither fault nor hang.
 * CONSEQUENCES.  A STEADY full-scale tone has several per cent of its samples within tol of its peak and reads as clipped;  the true
 * tone satisfies the constraints, but the result need not equal it.  SOFT clipping, and clipping followed by lossy coding or a
 * resampler, has no flat tops and is not detected.  The restoration is a sparse guess, not the original: on the test signal it gains 1
 * to 29 dB of SDR.  Real speech is unpinned.
 * Refused, on the host, with nothing launched and every output as it was:  a parameter outside its range or not finite where a finite
 * one is required;  B outside [1, 65535];  a length outside [1, L_max];  an utterance of more than MT2_DECLIP_MAX_FRAMES frames;
 * Lout_max under the longest length;  iters with T_max under the most frames;  an output overlapping an input or another output - in
 * place is NOT offered, the overlap kernel reads the input's bits.  `m` may be a bare handle;  scratch comes from its arena;  every call
 * only enqueues (the first call of a frame length on a handle uploads its table of twiddles and window, in double, made on the host). */
#define MT2_DECLIP_FIELDS 8
#define MT2_DECLIP_MAX_FRAMES 16384      /* frames of one utterance: 256 MiB of frame scratch at N = 2048;  69 s at 16 kHz and N = 256 */
typedef struct mt2_declip_config {
    int32_t frame;             /* N in {256, 512, 1024, 2048};  1024 */
    int32_t min_count;         /* >= 1;  4 */
    int32_t step;              /* s in [1, N / 2 + 1];  1 */
    int32_t every;             /* r in [1, 64];  1 */
    int32_t max_iter;          /* 0 = r ceil((N / 2 + 1) / s), or >= 1 */
    int32_t reserved;          /* 0 */
    double tol;                /* in [0, 0.1];  1e-3, relative to the level */
    double min_share;          /* in [0, 1];  1e-4 of the utterance's samples */
    double level;              /* NaN = detect, or the clipping level, positive and finite */
    double eps;                /* in (0, 1);  0.02 */
} mt2_declip_config;
/* Arena bytes of one mt2_declip call and of one mt2_clip_detect call (exactly their high water) and the frames of the longest utterance;
 * host only, no HIP call;  outputs may be NULL;  lens NULL: every len_b = L_max.  It refuses what the calls refuse for these arguments.
 * With r(x) = x rounded up to 256 bytes and R = sum_b T_b:  detection r(4 * 2 B) + r(32 B);  the whole call r(4 * 3 B) + r(32 B) + r(4 R)
 * + r(8 R N) - the one upload of lengths, needs and first rows, the detection words, the iteration counts, the frames in double. */
int mt2_declip_query(const mt2_declip_config* dc, const int32_t* lens /*host or NULL*/, int L_max, int B, long long* workspace_bytes,
                     long long* detect_bytes, long long* T_max);
/* Step 1 alone:  wav f32 [B, L_max] (device; samples at or beyond lens[b] are never read), lens host int32 [B] -> figures (device f64
 * [B, 8]).  Nothing is restored. */
int mt2_clip_detect(mt2_model* m, void* stream, const mt2_declip_config* dc, const float* wav, const int32_t* lens /*host*/, int L_max, int B,
                    double* figures);
/* The whole rule:  -> out f32 [B, Lout_max] (device; the samples j < lens[b] are written, the rest are left untouched).  figures (device
 * f64 [B, 8] or NULL).  iters (device int32 [B, T_max] or NULL): the iterations of every frame, zero for a frame that did not iterate
 * and beyond T_b.  Stage events (mt2_set_profiling): dc_detect, dc_frames, dc_overlap, dc_figures. */
int mt2_declip(mt2_model* m, void* stream, const mt2_declip_config* dc, const float* wav, const int32_t* lens /*host*/, int L_max, int B,
               float* out, int Lout_max, double* figures /*or NULL*/, int32_t* iters /*or NULL*/, int T_max);

/* ---- speech segments of prompt audio by frame energy, and the cut that takes the pauses out (csrc/segments.hip).  mt2_trim_silence
 * cuts the two ENDS; silence inside a prompt - the pause between two sentences, room tone, the gap between joined takes - still
 * reaches the mel context and the prosody codes as if it were speech.  The reference relies on pre-cut data (prepare_ds.py).  The rule
 * is our own, held to its restatement (tests/segments_ref.py); parity with librosa.effects.split, webrtcvad or any model-based VAD is
 * unpinned, and so is quality on real speech.
 *
 * THE RULE.  The frames are the trim's, unchanged: s[j], F = 1 + L / 512, e[f] = ((s[f-2] + s[f-1]) + s[f]) + s[f+1], E = max_f e[f],
 * c = (float)pow(10.0, -top_db / 10.0).  (The staged call takes any contour e[f] >= 0; there E = max(0, max_f e[f]).)
 *  1 raw    a[f] = e[f] > E * c, one f32 product;  E < FLT_MIN: every frame is active (the trim's convention)
 *  2 close  an inactive run that lies BETWEEN two active frames and is shorter than min_pause frames becomes active -> b.  Leading and
 *           trailing inactive runs never do.
 *  3 open   a run of b shorter than min_speech frames becomes inactive -> c
 *  4 pad    d[f] = some g in [0, F) with |g - f| <= pad has c[g]
 *  5        c empty ("nothing found"): d is all true - the utterance stays whole as one segment, and figure 3 says so by its sign
 * Segment k is the k-th maximal run [f0, f1] of d: frames [f0, f1 + 1), samples [512 f0, min(L, 512 (f1 + 1))).  Because min_pause >
 * 2 pad the runs of d are the runs of c widened by pad and clamped, one for one, with at least min_pause - 2 pad frames between two of
 * them: no merge step exists.  An utterance has at most max(1,(F + min_pause) / (min_speech + min_pause)) segments (64-bit), which
 * mt2_segments_query reports; a caller's S_max below it is refused, so nothing can overflow.  With min_pause >= F, pad = 0 and
 * min_speech = 2 the one segment is mt2_trim_silence's (start, end) whenever the trim keeps at least two frames.
 *
 * THE CUT.  The kept frames - d with keep = 0 (speech), !d with keep = 1 (pauses: a noise-only clip) - are copied in ascending order,
 * frame f to the offset 512 * (kept frames before f), every copy exact.  No cross-fade: a join lies in frames under the threshold and
 * on a multiple of 512 samples, so on a mel-frame boundary (hop 256).  The output has 512 * (kept frames) samples, minus what the last
 * frame lacks of 512 if it is kept (it owns [512 (F - 1), L)); with keep = 1 that may be 0.  Zeros follow up to Lout_max.
 *
 * Figures, a row of MT2_SEGMENTS_FIELDS = 8 doubles:  0 F   1 raw active frames   2 kept frames   3 segments, NEGATIVE (-1) when
 * nothing was found and the utterance stayed whole   4 kept samples (the staged call: 512 * kept frames)   5 the longest pause between
 * two segments in frames (0 with one segment)   6 mean e over the kept frames   7 mean e over the dropped ones (0 where there are
 * none).  The sums of 6 and 7 are taken in double in a fixed order.
 *
 * A flag, a segment and a figure depend on their utterance alone: a ragged batch is bit-identical to its utterances alone.  Input
 * must be finite; a non-finite sample cannot fault and gives segments inside [0, L], nothing more.
 * Refused on the host, before the first HIP call, outputs untouched: top_db not finite or <= 0; min_speech < 2 (so every segment owns
 * at least 512 samples, even when L % 512 == 0 and the last frame owns none); pad < 0; min_pause <= 2 pad; keep not 0 or 1; B outside
 * [1, 65535]; a length outside [1, L_max]; max length > INT_MAX - 4 * 512; S_max below the bound; F_max or Lout_max too small; an
 * output overlapping an input or another output.
 * Limits: the threshold is relative to the LOUDEST frame - room tone above -top_db of the peak reads as speech and nothing is cut; a
 * breath is speech or pause by its level alone; a weak consonant at a segment's edge is protected only by pad; mel frames that
 * straddle a join see both sides.  Out of scope: a maximum segment length, a streaming form, multichannel, model-based VAD. */
#define MT2_SEGMENTS_FIELDS 8
#define MT2_SEGMENTS_CHUNK 256      /* frames the smoothing kernel takes at a time (tests put runs and gaps across its multiples) */
typedef struct mt2_segments_config {
    float top_db;              /* > 0, finite;  40 */
    int32_t min_pause;         /* frames, > 2 pad;  10 = 320 ms at 16 kHz */
    int32_t min_speech;        /* frames, >= 2;  3 = 96 ms */
    int32_t pad;               /* frames, >= 0;  2 = 64 ms */
    int32_t keep;              /* 0 speech, 1 pauses */
} mt2_segments_config;
/* Host only, no HIP call; outputs may be NULL; lens (samples) NULL: every len_b = L_max.  frames = 1 + max_b len_b / 512, factor = c,
 * max_segments = the bound at `frames`, workspace_bytes = the arena high water of mt2_speech_segments and of mt2_cut_pauses exactly,
 * whatever optional outputs they are given.  With r(x) = x rounded up to 256 bytes, W = frames, NB = ceil(max len / 512):
 *   r(4 * 2 B) + r(4 W B) + r(4 W B) + 3 r(W B) + r(32 B)   [+ r(4 NB B) + r(4 B) + r(4 W B) in front of the energies of the audio calls]
 * mt2_segment_frames takes the unbracketed part with r(4 B) for the plan and W = max_b frame_lens[b].  It refuses what the calls
 * refuse for these arguments. */
int mt2_segments_query(const mt2_segments_config* cfg, const int32_t* lens /*host or NULL*/, int L_max, int B, int* frames, float* factor,
                       long long* max_segments, long long* workspace_bytes);
/* The staged form, steps 1-5 on any energy contour (from mt2_frame_energy, for one): energy f32 [B, F_max] (device; entries at or
 * beyond frame_lens[b] are never read), frame_lens host int32 [B] in [1, F_max], F_max <= INT_MAX / 512 -> flags (device u8 [B, F_max]
 * or NULL: d; bytes at or beyond frame_lens[b] are left alone), segments (device int32 [B, S_max, 2] or NULL: FRAMES [f0, f1 + 1), -1
 * behind counts[b]), counts (device int32 [B] or NULL), figures (device f64 [B, 8] or NULL).  The call only enqueues. */
int mt2_segment_frames(mt2_model* m, void* stream, const mt2_segments_config* cfg, const float* energy /*[B, F_max]*/,
                       const int32_t* frame_lens /*host*/, int F_max, int B, uint8_t* flags, int32_t* segments, int S_max, int32_t* counts,
                       double* figures);
/* wav f32 [B, L_max] (device; samples at or beyond lens[b] are never read) -> segments (device int32 [B, S_max, 2] or NULL: SAMPLES
 * [start, end), -1 behind counts[b]), counts, figures as above; energy (device f32 [B, F_max] or NULL): e[f], zeros in [F_b, F_max).
 * The call only enqueues. */
int mt2_speech_segments(mt2_model* m, void* stream, const mt2_segments_config* cfg, const float* wav, const int32_t* lens /*host*/, int L_max,
                        int B, int32_t* segments, int S_max, int32_t* counts, double* figures, float* energy, int F_max);
/* The cut: -> out f32 [B, Lout_max] (device), Lout_max >= max_b lens[b] (the cut is not known before the call).  out_lens (host int32
 * [B] or NULL): as with the trim's `bounds`, only a caller that asks for it pays for one copy to the host and ONE stream synchronise;
 * otherwise the call only enqueues, and the copy kernel reads its offsets on the device.  segments (samples of the INPUT, whichever
 * `keep`), counts, figures: as above, or NULL. */
int mt2_cut_pauses(mt2_model* m, void* stream, const mt2_segments_config* cfg, const float* wav, const int32_t* lens /*host*/, int L_max, int B,
                   float* out, int Lout_max, int32_t* out_lens /*host or NULL*/, int32_t* segments, int S_max, int32_t* counts, double* figures);

/* ---- F0 tracking by YIN (de Cheveigne & Kawahara 2002, steps 2-5; csrc/f0.hip) and the pitch moments of a track.  No reference
 * counterpart: the reference tree has no pitch tracker (it would take one from librosa or pyworld).  Parity with librosa.yin / pyin
 * is unpinned - neither is on hand - and quality on real speech is unpinned as well; the rule is our own statement and the tests
 * hold the kernel to it.  Frames are the mel front-end's at the same hop, so f0[t] belongs to mel frame t.  For one utterance
 * x[0 .. L), L >= 1, with W = MT2_F0_WINDOW:
 *   T = 1 + L / hop frames;  frame t reads x over [hop t - 512, hop t + 512), a sample outside [0, L) being a zero by its index,
 *   never a read;  s = hop t - 512
 *   tau_min = ceil(sample_rate / fmax), tau_max = floor(sample_rate / fmin); refused, not clamped, unless
 *   2 <= tau_min < tau_max <= MT2_F0_MAX_LAG
 *   d[tau] = sum_{j = 0}^{W - 1} (x[s + j] - x[s + j + tau])^2, tau = 0 .. 256 (all 257, whatever tau_max): in f32 ONE chain over j
 *   ascending, e = a - b rounded, acc = fma(e, e, acc) from 0;  d[0] is exactly 0
 *   c[0] = 0, c[tau] = c[tau - 1] + d[tau] (one f32 add each, tau ascending);  d'[0] = 1,  d'[tau] = (d[tau] * (float)tau) / c[tau]
 *   (one f32 product, one true f32 division), 1 where c[tau] is not > 0
 *   tau0 = the smallest tau in [tau_min, tau_max] with d'[tau] < threshold;  from tau0 up while tau + 1 <= tau_max and
 *   d'[tau + 1] < d'[tau]: the end of the walk is tau*.  No such tau0: tau* = the smallest tau in [tau_min, tau_max] attaining the
 *   minimum of d' (a NaN never wins; all NaN: tau_min).  cmnd = d'[tau*];  the frame is voiced iff d'[tau*] < threshold
 *   voiced frames with tau* - 1 >= 1 and tau* + 1 <= tau_max:  a, b, c = d'[tau* - 1], d'[tau*], d'[tau* + 1];  den = (a - 2 b) + c;
 *   delta = (a - c) / (2 den) if den > 0, else 0 (also 0 without both neighbours);  f0 = (float)sample_rate / ((float)tau* + delta),
 *   every operation rounded on its own;  unvoiced frames: f0 = 0
 * The order of every sum depends on the sample's index in its utterance alone: a ragged batch is bit-identical to its utterances
 * alone.  Non-finite samples cannot fault, cannot write outside the outputs and do not change a frame whose window does not hold
 * one; nothing more is promised.  Frames in [T_b, T_max) are written as unvoiced: f0 0, cmnd 1, lag 0, d 0.
 * Refused (error, nothing launched, every output as it was): B < 1 or > 65535; lens[b] < 1 or > L_max; hop outside [1, 1024];
 * fmin / fmax not finite or <= 0; the lag condition; threshold outside (0, 1]; T_max < 1 + max_b lens[b] / hop; an output
 * overlapping wav.
 * Moments of f0 [B, T_max] over the voiced frames (f0 > 0) of utterance b among its first frame_lens[b], all sums in double, two
 * passes, in an order that depends on the frame index alone (not on the batch slot or T_max):  n;  mu = sum f / n;
 * m_k = sum (f - mu)^k / n, k = 2, 3, 4;  stats[b] = n, n / T_b, mu, sqrt(m2), m3 / m2^1.5, m4 / m2^2 - 3;  n = 0: all zeros;
 * m2 = 0: sigma = skew = kurt = 0. */
#define MT2_F0_FRAME 1024
#define MT2_F0_WINDOW 768
#define MT2_F0_MAX_LAG 256
/* T = 1 + L / hop, the lag range and the arena bytes of one mt2_f0_yin call (of any batch: the lengths alone); host only, no HIP
 * call (outputs may be NULL).  Refuses what mt2_f0_yin refuses of these arguments, and L outside [1, 2^31). */
int mt2_f0_query(int sample_rate, int hop, float fmin, float fmax, long long L, int* frames, int* lag_min, int* lag_max,
                 long long* workspace_bytes);
/* wav f32 [B, L_max] (device), lens host int32 [B] -> f0 f32 [B, T_max] (device; Hz, 0 = unvoiced).  Optional (NULL to skip), device:
 * cmnd f32 [B, T_max] = d'[tau*], lag int32 [B, T_max] = tau*, diff f32 [B, T_max, 257] = d - written to memory only for a caller that
 * passes it.  ONE launch for the batch; the call only enqueues, it does not synchronise.  `m` may be a bare handle. */
int mt2_f0_yin(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
               int sample_rate, int hop, float fmin, float fmax, float threshold, float* f0 /*[B, T_max]*/, float* cmnd /*or NULL*/,
               int32_t* lag /*or NULL*/, int T_max, float* diff /*or NULL*/);
/* ---- A second tracker beside YIN, off by default: a Viterbi pass over YIN's lag costs (csrc/f0.hip), the usual cure (pYIN, RAPT)
 * for YIN's octave errors - where the even harmonics dominate, d'[tau0 / 2] already dips under the threshold and "the first dip"
 * answers an octave high.  One lag per frame is chosen by the frame's whole d' curve plus a cost for jumping between frames.  The
 * rule is our own; parity with librosa.pyin is unpinned, as for YIN.  Per utterance: the frames, d, c and d' are exactly those above
 * (the same device code), tau_min and tau_max too.  n = tau_max - tau_min + 1 (at most 255) states, state k the lag tau_min + k.
 * Every operation is one f32 operation rounded on its own, no fma:
 *   lg[k]    = (float) log2((double)(tau_min + k))   (built in double on the host, rounded once)
 *   bias[k]  = octave_cost * (lg[k] - lg[0])
 *   o[t, k]  = q + bias[k],  q = d'[t, tau_min + k] if that is finite, else 1: every cost is finite by construction
 *   tr(j, k) = jump_cost * |lg[k] - lg[j]|: the jump in octaves times a weight, over all n x n pairs, no band
 *   delta[0, k] = o[0, k];  for t >= 1:  best = min_j (delta[t - 1, j] + tr(j, k)), j ascending with a strict <, so the smallest j
 *   wins a tie;  psi[t, k] = that j;  delta'[k] = o[t, k] + best;  m = min_k delta'[k];  delta[t, k] = delta'[k] - m (the per-frame
 *   renormalisation keeps f32 resolution on long clips)
 *   k*[T - 1] = the smallest k attaining min delta[T - 1, .];  k*[t - 1] = psi[t, k*[t]];  T = 1: the arg-min alone
 *   tau* = tau_min + k*[t];  cmnd = d'[t, tau*];  the frame is voiced iff cmnd < threshold - YIN's own criterion at the tracked lag:
 *   there is no unvoiced state and octave_cost never enters the voicing decision;  f0 by the parabola above, 0 when unvoiced
 * octave_cost (default 0.02) and jump_cost (default 0.5) must be finite and >= 0; jump_cost = 0 makes the frames independent.
 * Nothing depends on the batch slot, L_max or T_max: a ragged batch is bit-identical to its utterances alone.  A non-finite sample
 * cannot fault, cannot write outside the outputs and cannot move tau* outside [tau_min, tau_max]; UNLIKE YIN it may change frames
 * anywhere in its utterance, because the path is global.  Frames in [T_b, T_max) are written as mt2_f0_yin writes them.
 *
 * mt2_f0_track_query: host only, no HIP call (outputs may be NULL) - T = 1 + L / hop, the lag range, n and the arena bytes of one
 * mt2_f0_track call with B utterances and T_max = T:  r(4 (4 ceil(B / 4) + 256)) for the lengths and lg + r(4 B T 257) for d' +
 * r(256 B T) for psi, r(x) = x rounded up to a multiple of 256.  Refuses what mt2_f0_track refuses of these arguments, and L
 * outside [1, 2^31). */
int mt2_f0_track_query(int sample_rate, int hop, float fmin, float fmax, float octave_cost, float jump_cost, long long L, int B,
                       int* frames, int* lag_min, int* lag_max, int* states, long long* workspace_bytes);
/* Arguments and outputs as mt2_f0_yin (diff is d, the same bits as mt2_f0_yin's).  Two launches for the batch: d' of every frame to
 * arena scratch, then one workgroup per utterance for the recurrence, the backtrack and the refinement (stage events, with
 * mt2_set_profiling: f0_cmnd, f0_viterbi).  The call only enqueues.  Refused (error, nothing launched, every output as it was):
 * everything mt2_f0_yin refuses, and a negative or non-finite octave_cost or jump_cost. */
int mt2_f0_track(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                 int sample_rate, int hop, float fmin, float fmax, float threshold, float octave_cost, float jump_cost,
                 float* f0 /*[B, T_max]*/, float* cmnd /*or NULL*/, int32_t* lag /*or NULL*/, int T_max, float* diff /*or NULL*/);
/* f0 f32 [B, T_max] (device), frame_lens host int32 [B] in [1, T_max] -> stats f64 [B, 6] (device).  One launch, a workgroup per
 * utterance; the call only enqueues.  Refused: B < 1 or > 65535, a frame count outside [1, T_max], stats overlapping f0. */
int mt2_f0_stats(mt2_model* m, void* stream, const float* f0 /*[B, T_max]*/, const int32_t* frame_lens /*host*/, int T_max, int B,
                 double* stats /*[B, 6]*/);

/* ---- Per-phone prosody (csrc/prosody.hip): an energy contour on the mel's frames, the segment reduction of an F0 track over phone
 * durations, and the voiced frames of a track compacted to a semitone contour, which turns mt2_dtw_align with D = 1 into a pitch-
 * contour distance.  No reference counterpart (it would take pitch and energy from librosa or pyworld): the rules are our own,
 * parity with any outside library and quality on real speech are unpinned, and the tests hold the kernels to the rules.  For all
 * three: every sum is taken in an order that depends on the sample / frame / phone index within its utterance alone, so a ragged
 * batch is bit-identical to its utterances alone, whatever the slot, L_max, T_max or Np_max;  a non-finite input cannot fault,
 * cannot write outside the outputs and cannot change an output whose inputs do not hold it;  `m` may be a bare handle;  the
 * lengths travel in the call's one upload and the call only enqueues;  every refusal is decided on the host before the first HIP
 * call (error, nothing launched, every output as it was).
 *
 * mt2_frame_energy.  wav f32 [B, L_max] (device), lens host int32 [B], hop in [1, 1024] -> energy f32 [B, T_max] (device).  For one
 * utterance x[0 .. L):  T = 1 + L / hop;  frame t reads [hop t - 512, hop t + 512) - MT2_F0_FRAME samples, exactly the F0 frames, so
 * energy[t], f0[t] and mel frame t coincide;  a sample outside [0, L) is a zero by its index and is never read.  energy[t] = the
 * mean square of the 1024 samples in f32 by one wave:  lane l runs ONE chain acc = fma(x, x, acc) from 0 over the in-frame offsets
 * 256 i + 4 l + r, i = 0 .. 3 outer, r = 0 .. 3 inner;  the 64 partial sums meet in the xor butterfly 32, 16, 8, 4, 2, 1;  one
 * product by 2^-10 (exact).  Frames in [T_b, T_max) are written 0.  Refused: what mt2_f0_yin refuses of B, lens, hop and T_max, and
 * energy overlapping wav. */
int mt2_frame_energy(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B, int hop,
                     float* energy /*[B, T_max]*/, int T_max);
/* mt2_phone_prosody.  f0 f32 [B, T_max], energy f32 [B, T_max] or NULL, dur int32 [B, Np_max] (all device - dur as the ADM leaves
 * it), phone_lens and frame_lens host int32 [B] -> out f64 [B, Np_max, 8] (device, 16-byte aligned), optionally dur_sum int64 [B]
 * (device).  For utterance b with Np phones and T frames:  start[p] = sum_{q < p} max(dur[q], 0) in int64;  phone p owns the frames
 * [min(start, T), min(start + max(dur[p], 0), T)), taken in ascending order;  a frame is voiced iff f0 > 0 (a NaN is not).  The
 * fields of out[b, p], all in double:
 *   0 start (clipped)   1 frames owned   2 voiced frames among them   3 mean f0 in Hz over the voiced frames
 *   4 mean of 12 log2((double)f0 / 55) over the voiced frames (semitones above A1)   5 min f0   6 max f0 over the voiced frames
 *   7 mean of energy over all owned frames (0 when energy is NULL)
 * 3 - 6 are 0 without a voiced frame, 7 is 0 without a frame;  rows p >= phone_lens[b] are all zeros;  dur beyond phone_lens[b] and
 * frames beyond frame_lens[b] are never read.  dur_sum[b] = the unclipped sum of max(dur, 0): the caller compares it with T_b, the
 * kernel decides nothing.  One launch, a workgroup per utterance.  Refused: B < 1 or > 65535; a phone count outside [1, Np_max]; a
 * frame count outside [1, T_max]; overlapping buffers. */
#define MT2_PROSODY_FIELDS 8
int mt2_phone_prosody(mt2_model* m, void* stream, const float* f0 /*[B, T_max]*/, const float* energy /*or NULL*/,
                      const int32_t* dur /*device [B, Np_max]*/, const int32_t* phone_lens /*host*/, int Np_max,
                      const int32_t* frame_lens /*host*/, int T_max, int B, double* out /*[B, Np_max, 8]*/, long long* dur_sum /*or NULL*/);
/* mt2_pitch_contour.  f0 f32 [B, T_max] (device), frame_lens host int32 [B], center 0 / 1 -> st f32 [B, T_max], n_voiced int32 [B],
 * optionally index int32 [B, T_max] (all device).  The voiced frames (f0 > 0) among the first T_b are kept in order - a stable
 * compaction by the exclusive count of voiced flags in front of each frame.  s = 12 log2((double)f0);  with center, mu = sum s / n in
 * double in the order of the pitch moments (thread i sums the frames i, i + 256, ... ascending, the 256 partial sums meet in a fixed
 * tree) and st[k] = (float)(s - mu), rounded once;  without, st[k] = (float)s.  index[k] = the frame entry k came from.  Entries in
 * [n, T_max) are written 0 / -1;  n = 0: the whole row is 0 / -1 and n_voiced 0.  One launch, a workgroup per utterance.
 * mt2_dtw_align with D = 1 on two such contours gives `total` and `steps`: sqrt(total / steps) is the distance in semitones along the
 * path - centring removes the speaker's register, the warp the speaking rate, compaction keeps unvoiced gaps from counting as pitch.
 * Refused: B < 1 or > 65535; a frame count outside [1, T_max]; center not 0 or 1; overlapping buffers. */
int mt2_pitch_contour(mt2_model* m, void* stream, const float* f0 /*[B, T_max]*/, const int32_t* frame_lens /*host*/, int T_max, int B,
                      int center, float* st /*[B, T_max]*/, int32_t* n_voiced /*[B]*/, int32_t* index /*or NULL*/);

/* ---- Formant candidates by linear prediction (csrc/formants.hip; Markel & Gray 1976) and the formant figures of an utterance: the
 * resonances of an all-pole fit of every frame, their means, the formant dispersion (Fitch 1997) and a vocal-tract length (the uniform
 * tube closed at one end; Wakita 1977, Reby & McComb 2003) - a timbre measure that, unlike mt2_mel_cepstral_distortion, needs no
 * recording of the same sentence.  No reference counterpart.  The fit is the AUTOCORRELATION method; parity with Praat (Burg's method,
 * Gaussian window) is unpinned, and so is quality on real speech; the rule is our own statement, restated in tests/formant_ref.py,
 * and the tests hold the kernel to it and to the poles of known all-pole filters.  Candidates are per frame: candidate q of one frame
 * need not be candidate q of the next - mt2_formant_track (below) connects them.
 * THE RULE, for one utterance x f32 [L] at sample_rate, a hop, an even window W in [64, 1024] and an even order P in [2, 32], P < W:
 *  1 frames  T = 1 + L / hop.  Frame t covers the samples i = s + j, s = hop t - W / 2, j = 0 .. W - 1.  A sample outside [0, L) is a
 *            zero by its index and is never read.  At hop = the mel's and the mel's rate, frame t is centred like mel frame t.
 *  2 pre-emphasis in double:  y[i] = x[i] - alpha * x[i - 1] (one product, one difference, each rounded), x[-1] = 0,
 *            alpha = exp(-2 pi preemphasis_hz / sample_rate) made in double on the host.  preemphasis_hz = 0 is alpha = 0: off, y[i] =
 *            x[i] and x[i - 1] is not read.  With alpha > 0 frame t reads x over [s - 1, s + W) within [0, L).
 *  3 window  v[j] = y[s + j] * w[j], one product; 0 for a sample outside [0, L).  MT2_FORMANT_HANN: w[j] = 0.5 - 0.5 cos(2 pi (j + 0.5)
 *            / W);  MT2_FORMANT_RECT: w[j] = 1.  The table is built in double on the host (mt2_formant_window) and kept in the handle
 *            per (W, kind) as the resampler keeps its filters: the first call with a new pair uploads it, every later one only enqueues.
 *  4 autocorrelation in double:  r[k] = sum_j v[j] v[j + k], k = 0 .. P, in this order: lane l of 64 runs ONE chain acc = fma(v[j],
 *            v[j + k], acc) from 0 over j = l, l + 64, l + 128, ... while j + k < W;  the 64 partial sums meet in the xor butterfly
 *            32, 16, 8, 4, 2, 1 (lane l adds lane l ^ o's value to its own).  Then r[0] = r[0] * (1 + 1e-9), one product.  The frame is
 *            EMPTY unless r[0] > 1e-300 and r[0] is finite.
 *  5 Levinson-Durbin in double, every operation rounded on its own, no fma:
 *              e = r[0];  a[0] = 1
 *              for m = 1 .. P:
 *                acc = r[m];  for i = 1 .. m - 1 ascending:  acc = acc + (a[i] * r[m - i])
 *                k = (-acc) / e;  the frame is empty unless |k| < 1
 *                for i = 1 .. m - 1:  a'[i] = a[i] + (k * a[m - i]) (from the a of before this m);  a'[m] = k;  a = a'
 *                e = e * (1 - (k * k));  the frame is empty unless e > 0 and e is finite
 *            and empty if an a[i] is not finite.  lpc = a[0 .. P], err = the last e.
 *  6 roots   of z^P + a[1] z^(P-1) + ... + a[P] by Aberth-Ehrlich iteration in double complex, not pinned to the bit.  Starts z_k =
 *            0.9 exp(i (2 pi k / P + 0.4)), k = 0 .. P - 1.  One iteration, for every k from the z of before it:  p and p' at z_k by
 *            Horner, q = p / p';  S = sum over j != k, j ascending, of 1 / (z_k - z_j);  w_k = q / (1 - q S);  z_k = z_k - w_k.  It stops
 *            after the iteration whose max_k |w_k|^2 < 1e-26 (max_k |w_k| < 1e-13); iters = the iterations run.  The frame is empty
 *            if a w_k is not finite or MT2_FORMANT_MAX_ITERS = 64 iterations do not get there.
 *  7 candidates  of the roots with Im z > 0:  f = atan2(Im z, Re z) sample_rate / (2 pi),  bw = -(1/2) ln(|z|^2) sample_rate / pi.
 *            Kept:  fmin_hz < f < sample_rate / 2 - fmin_hz  and  bw < max_bandwidth_hz.  Sorted ascending by f, a tie going to the
 *            smaller root index.  count = min(kept, MT2_FORMANT_MAX = 5);  freq[t][q], bw[t][q] = candidate q rounded to f32 for q <
 *            count, zeros behind.
 * An EMPTY frame has count 0, freq and bw zeros, iters -1; of the optional outputs it keeps what its stages reached - autocorr always,
 * lpc and err if step 5 went through - and has zeros in the others.  A frame in [T_b, T_max) has zeros everywhere, iters 0 as well.
 * Nothing depends on the batch slot, L_max or T_max: a ragged batch is bit-identical to its utterances alone.  A non-finite sample
 * cannot fault and cannot write outside the outputs; it empties the frames that read it (step 2) and changes no other frame's bits.
 * Refused on the host (error, nothing launched, every output as it was): B < 1 or > 65535; lens[b] < 1 or > L_max; sample_rate < 1;
 * hop outside [1, 1024]; window outside [64, 1024] or odd; order outside [2, 32] or odd; order >= window (which the two ranges as they stand already exclude: a guard); kind not one of the two;
 * reserved not 0; a non-finite or negative preemphasis_hz, fmin_hz or max_bandwidth_hz; fmin_hz >= sample_rate / 4; T_max < 1 + max_b
 * lens[b] / hop; a NULL or misaligned buffer; an output overlapping wav or another output.
 * Limits: LPC on a voiced frame fits the harmonics as well as the envelope - a formant near a strong harmonic is drawn to it (F1 of a
 * 700 Hz resonance under 110 Hz pulses reads about 764 Hz, by the 7th harmonic): a property of linear prediction, not of the kernel.
 * Out of scope: Burg's method; LPC-cepstral distortion; line spectral frequencies;
 * nasal / anti-formant models; a streaming form; multichannel.
 *
 * THE FIGURES, mt2_formant_stats: over the frames t < frame_lens[b] with count[t] >= 4, and f0[t] > 0 where an F0 track is given, all
 * in double, two passes, sums in the order of mt2_f0_stats (thread i of 256 sums the frames i, i + 256, ... ascending, the partial sums
 * meet in a fixed tree):  n;  mu_k = sum freq[t][k - 1] / n and sigma_k = sqrt(sum (freq[t][k - 1] - mu_k)^2 / n) for k = 1 .. 4.  A row
 * of MT2_FORMANT_STAT_FIELDS = 12 doubles:  0 n   1 n / T_b   2-5 mu_1 .. mu_4   6-9 sigma_1 .. sigma_4   10 the formant dispersion
 * (mu_4 - mu_1) / 3   11 the vocal-tract length in cm, (35000 / 4) (1 / 4) sum_k (2 k - 1) / mu_k, evaluated as
 * 2187.5 * (((1 / mu_1 + 3 / mu_2) + 5 / mu_3) + 7 / mu_4): 17.5 cm for 500 / 1500 / 2500 / 3500 Hz.  n = 0: all zeros. */
#define MT2_FORMANT_MAX 5
#define MT2_FORMANT_MAX_WINDOW 1024
#define MT2_FORMANT_MAX_ORDER 32
#define MT2_FORMANT_MAX_ITERS 64
#define MT2_FORMANT_STAT_FIELDS 12
#define MT2_FORMANT_HANN 0
#define MT2_FORMANT_RECT 1
typedef struct mt2_formant_config {
    int32_t window;            /* W, samples: even, in [64, 1024];  550 = 50 ms at 11 kHz */
    int32_t order;             /* P: even, in [2, 32], < window;  10 */
    int32_t kind;              /* MT2_FORMANT_HANN or MT2_FORMANT_RECT */
    int32_t reserved;          /* 0 */
    double preemphasis_hz;     /* >= 0, finite; 0 = off;  50 */
    double fmin_hz;            /* >= 0, finite, < sample_rate / 4;  50 */
    double max_bandwidth_hz;   /* >= 0, finite;  500 */
} mt2_formant_config;
/* Host only, no HIP call; outputs may be NULL.  frames = 1 + L / hop;  workspace_bytes = the arena high water of one mt2_lpc_formants
 * call exactly, whatever B and whatever optional outputs: 4 * 65535 rounded up to 256 - the lengths, in the room of the largest batch.
 * Refuses what mt2_lpc_formants refuses of these arguments, and L outside [1, 2^31). */
int mt2_formant_query(int sample_rate, int hop, int window, int order, long long L, int* frames, long long* workspace_bytes);
/* Host only: the window of step 3, table[0 .. window) in double.  Refuses a window outside [64, 1024] or odd and an unknown kind. */
int mt2_formant_window(int window, int kind, double* table /*host [window]*/);
/* wav f32 [B, L_max] (device; samples at or beyond lens[b] are never read), lens host int32 [B] -> freq, bw f32 [B, T_max, 5] and count
 * int32 [B, T_max] (device).  Optional (NULL to skip), device, 8-byte aligned where f64: lpc f64 [B, T_max, P + 1], err f64 [B, T_max],
 * autocorr f64 [B, T_max, P + 1] (r[0] as scaled), roots f64 [B, T_max, P, 2] (re, im; in root-index order), iters int32 [B, T_max].
 * ONE launch for the batch, a wave per frame; the call only enqueues.  `m` may be a bare handle. */
int mt2_lpc_formants(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                     int sample_rate, int hop, const mt2_formant_config* cfg, float* freq /*[B, T_max, 5]*/, float* bw /*[B, T_max, 5]*/,
                     int32_t* count /*[B, T_max]*/, int T_max, double* lpc /*or NULL*/, double* err /*or NULL*/, double* autocorr /*or NULL*/,
                     double* roots /*or NULL*/, int32_t* iters /*or NULL*/);
/* freq f32 [B, T_max, 5], count int32 [B, T_max], f0 f32 [B, T_max] or NULL (all device), frame_lens host int32 [B] in [1, T_max] ->
 * stats f64 [B, 12] (device).  One launch, a workgroup per utterance; the call only enqueues.  Refused: B < 1 or > 65535; a frame count
 * outside [1, T_max]; a NULL or misaligned buffer; stats overlapping an input. */
int mt2_formant_stats(mt2_model* m, void* stream, const float* freq /*[B, T_max, 5]*/, const int32_t* count /*[B, T_max]*/,
                      const float* f0 /*or NULL*/, const int32_t* frame_lens /*host*/, int T_max, int B, double* stats /*[B, 12]*/);

/* ---- Formant tracks across frames (csrc/formant_track.hip): of the candidates of mt2_lpc_formants, the K per frame that form the cheapest
 * smooth path through the utterance, by a Viterbi pass in the manner of Praat's "Formant: Track" (Xia & Espy-Wilson 2000) with a rule of
 * our own.  No reference counterpart.  The outputs have the candidates' own layout, so mt2_formant_stats reads them unchanged: one spurious
 * root no longer shifts every formant above it by one slot.  Parity with Praat's tracker is unpinned, and so is quality on real speech; the
 * rule is restated in tests/formant_track_ref.py, and the tests hold the kernel to it to the bit and to the truth of a synthetic scene.
 * THE RULE, for one utterance freq, bw f32 [T, 5], count int32 [T], K = tracks in [1, 5], ref_hz[0 .. K), freq_cost, bw_cost, jump_cost:
 * everything in DOUBLE, every operation rounded on its own, no fma; the f32 inputs convert exactly; there is no transcendental function, so
 * a numpy restatement reproduces every cost, and hence every decision, to the bit.
 *  states    the C(5, K) strictly increasing K-tuples of candidate indices from {0 .. 4} in lexicographic order, at most
 *            MT2_FORMANT_TRACK_STATES = 10.  State s assigns candidate st[s][q] to track q.  The table does not depend on the frame.
 *  gap       n = min(count[t], 5).  Frame t is a GAP if n < K, or if among its first n candidates a freq is not finite or <= 0 or a bw is
 *            not finite or < 0.  State s is valid in a non-gap frame iff st[s][K - 1] < n; state 0 always is.
 *  local     of a valid state:  term_q = (freq_cost * (|f - ref_q| / 1000)) + (bw_cost * (b / f)) with f, b the candidate of track q;
 *            o[t, s] = term_0 + term_1 + ..., q ascending, left to right.  An invalid state has o = +inf.
 *  jump      between non-gap frames t - 1 and t:  u_q = (2 * |f' - f|) / (f' + f), f the candidate of track q under state j at t - 1
 *            and f' under state k at t;  tr(j, k) = jump_cost * (u_0 + u_1 + ...), q ascending.
 *  forward   t = 0 or frame t - 1 a gap:  delta[t, k] = o[t, k], psi[t, k] = 0.  Otherwise best = min_j (delta[t - 1, j] + tr(j, k)) over
 *            the j with finite delta[t - 1, j], j ascending with a strict < from +inf (the smallest j wins a tie), psi[t, k] that j,
 *            delta[t, k] = o[t, k] + best; an invalid k has delta = +inf, psi = 0.  Costs are not renormalised: in double the sums stay
 *            exact enough for any clip the call accepts.  In a gap frame delta[t, k] = 0 for every k and psi[t, k] is the smallest j
 *            attaining min delta[t - 1, .] (0 at t = 0): a gap cuts the utterance into segments that are tracked independently.
 *  backward  k*[T - 1] = the smallest k attaining min delta[T - 1, .];  k*[t - 1] = psi[t, k*[t]].
 *  outputs   a non-gap frame:  sel[t][q] = st[k*[t]][q] for q < K and -1 behind;  track_freq[t][q], track_bw[t][q] = the selected
 *            candidate's freq and bw, copied bit for bit, zeros behind;  track_count[t] = K.  A gap frame, and a frame in [T_b, T_max):
 *            sel all -1, track_freq and track_bw zeros, track_count 0.
 * jump_cost = 0 makes the frames independent: each picks its own arg-min of o.  Nothing depends on the batch slot or T_max: a ragged
 * batch is bit-identical to its utterances alone.  A non-finite input cannot fault and cannot write outside the outputs; it turns its frame
 * into a gap, which may change the path elsewhere in the same utterance, as in mt2_f0_track.
 * Refused on the host (error, nothing launched, every output as it was): B < 1 or > 65535; a frame_lens[b] outside [1, T_max]; tracks
 * outside [1, 5]; reserved not 0; a non-finite or non-positive ref_hz among the first K; a non-finite or negative cost; a NULL or
 * misaligned buffer (sel may be NULL); an output overlapping an input or another output.
 * Out of scope: a track that may be absent in some frames (every non-gap frame carries all K); an unvoiced state; a streaming form. */
#define MT2_FORMANT_TRACK_STATES 10
typedef struct mt2_formant_track_config {   /* 72 bytes, no padding */
    int32_t tracks;      /* K in [1, 5];  4 */
    int32_t reserved;    /* 0 */
    double ref_hz[5];    /* finite, > 0, the first K used;  550 1650 2750 3850 4950 */
    double freq_cost, bw_cost, jump_cost;   /* finite, >= 0;  1 1 1 */
} mt2_formant_track_config;
/* Host only, no HIP call; outputs may be NULL.  states = C(5, tracks);  workspace_bytes = the arena high water of one mt2_formant_track
 * call exactly: r(4 * 65535) + r(16 * B * T_max), r rounding up to 256 - the lengths in the room of the largest batch, then psi, 16 bytes
 * a frame.  Refuses tracks outside [1, 5], B outside [1, 65535] and T_max outside [1, 2^31). */
int mt2_formant_track_query(int tracks, long long T_max, int B, int* states, long long* workspace_bytes);
/* freq, bw f32 [B, T_max, 5], count int32 [B, T_max] (device, as mt2_lpc_formants wrote them; frames at or beyond frame_lens[b] are never
 * read), frame_lens host int32 [B] -> track_freq, track_bw f32 [B, T_max, 5], track_count int32 [B, T_max] and, unless NULL, sel int32
 * [B, T_max, 5] (device).  ONE launch for the batch, a workgroup per utterance; the call only enqueues.  `m` may be a bare handle. */
int mt2_formant_track(mt2_model* m, void* stream, const float* freq, const float* bw, const int32_t* count,
                      const int32_t* frame_lens /*host*/, int T_max, int B, const mt2_formant_track_config* cfg,
                      float* track_freq /*[B,T_max,5]*/, float* track_bw /*[B,T_max,5]*/, int32_t* track_count /*[B,T_max]*/,
                      int32_t* sel /*[B,T_max,5] or NULL*/);

/* ---- Integrated loudness and loudness normalisation (csrc/loudness.hip): ITU-R BS.1770-4 gated loudness, which EBU R 128 builds on, of
 * a ragged batch of mono utterances, and each utterance brought to a target loudness by one gain.  No reference counterpart (the
 * reference peak-normalises its prompts, models/megatts2.py:336, and leaves the output level alone).  Parity with pyloudnorm /
 * libebur128 is unpinned - neither is on hand; the kernels are held to the standard's own figures (a full-scale 997 Hz sine at 48 kHz
 * reads -3.01 LKFS), to the analytic steady-state reading of a sine, and to the float64 restatement tests/loudness_ref.py.  True peak
 * (oversampled) and loudness range (EBU Tech 3342) are measured by the calls of the next section, which leave these as they are.
 * THE RULE, for one utterance x f32 [L] at sample_rate:
 *  1 sample_rate is a multiple of 10 in [8000, 192000], never rounded.  h = sample_rate / 10 (the 100 ms sub-block);  ns = L / h
 *    complete sub-blocks;  nb = max(0, ns - 3) blocks of 400 ms with 75 % overlap - only blocks wholly inside the signal count.
 *  2 K-weighting coefficients in double from the analogue prototypes (at 48 kHz they reproduce the standard's table to 1e-13):
 *    shelf      f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196;  K = tan(pi f0 / sr), Vh = 10^(G / 20),
 *               Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2;  b = (Vh + Vb K / Q + K^2) / a0, 2 (K^2 - Vh) / a0,
 *               (Vh - Vb K / Q + K^2) / a0;  a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0
 *    high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773, K and a0 as above;  b = 1, -2, 1;  a1, a2 as above
 *  3 The shelf, then the high-pass, each in transposed direct form II in double:  y = b0 v + s1;  s1 = b1 v - a1 y + s2;
 *    s2 = b2 v - a2 y.  Zero state in front of sample 0;  the input is (double)x[i];  a sample at or beyond L is never read.  (The
 *    high-pass has a double pole at radius 0.985 at 16 kHz, 0.995 at 48 kHz: a direct form in f32 loses the low band.)  The device
 *    runs the recurrence in chunks of h samples - from zero state, the states carried by M = A^h, then again from the true entry
 *    state - which is exact up to rounding (1e-13 relative in the sub-block sums).
 *  4 S[j] = sum of y[i]^2 over sub-block j;  z[k] = (((S[k] + S[k+1]) + S[k+2]) + S[k+3]) / (4 h);  l[k] = -0.691 + 10 log10 z[k]
 *    (-inf for z = 0).  Gamma = -0.691 + 10 log10(mean of z over l > -70) - 10;  I = -0.691 + 10 log10(mean of z over l > -70 and
 *    l > Gamma);  no block over the absolute gate (nb = 0, silence): I = Gamma = -inf.  A block is over a gate unless l <= gate, so
 *    a NaN block counts.  Means are taken in a fixed order of the block index: partial sums over k = i, i + 256, ... ascending for
 *    i < 256, then a halving tree.
 *  5 stats f64 [8] per utterance:  0 I   1 nb   2 blocks over the absolute gate   3 blocks over both gates   4 Gamma
 *    5 sample peak max |x[i]| over i < L (a NaN sample is passed over)   6 max_k l[k] (-inf for nb = 0)   7 the linear gain of 6
 *    (1 for the measuring call).  momentary f64 [NB_max]: l[k], -inf for k >= nb.
 *  6 Normalisation:  g = 10^((target_lufs - I) / 20) in double;  with peak_ceiling > 0, g = min(g, peak_ceiling / peak);  g is rounded
 *    once to f32;  where the ceiling binds, g then moves by whole ulps (at most 4 each way) to the largest f32 whose f32 product
 *    with the peak is at or under the ceiling - the output's peak is <= the ceiling and within 2 ulp of it;
 *    out[i] = x[i] g, one f32 product;  zeros in [L, L_max).  g = 1 exactly, the utterance copied unchanged, when I is not finite
 *    (too short, silent, a non-finite sample) or g does not fit f32 - the peak normaliser's convention for silence.  The gain is
 *    formed and read on the device: the normalising call only enqueues.
 *  7 A non-finite sample cannot fault or write outside the outputs;  it makes its own utterance's loudness NaN from the sub-block
 *    that holds it on (the recurrence carries it to the end) and changes no bit of another utterance.  Every arithmetic order depends
 *    on the sample's, sub-block's or block's index in its utterance alone, so a ragged batch is bit-identical to its utterances
 *    alone, whatever the slot, L_max or B.
 * Refused, on the host before the first HIP call, every output as it was:  B < 1 or > 65535;  a length outside [1, L_max] or beyond
 * 2^31 - 153600;  the rate;  a non-finite target_lufs or peak_ceiling;  NB_max < 1 or smaller than the blocks of the longest
 * utterance while `momentary` is given;  `out` overlapping `wav` other than out == wav;  stats / momentary overlapping anything.
 * `m` may be a bare handle;  scratch comes from its arena. */
#define MT2_LOUDNESS_FIELDS 8
/* h, nb, the ten coefficients (b0 b1 b2 a1 a2 of the shelf, then of the high-pass) and the arena bytes of a call with ONE utterance of L
 * samples;  host only, no HIP call (outputs may be NULL).  A call with B utterances, the longest with ns sub-blocks, takes
 * r(4 (4 ceil(B / 4) + 32)) + r(32 B ns) + r(8 B ns) + r(8 B) bytes, r(x) = max(256, x rounded up to 256). */
int mt2_loudness_query(int sample_rate, long long L, int* sub_block, int* blocks, double* coeffs /*[10]*/, long long* workspace_bytes);
/* wav f32 [B, L_max] (device), lens host int32 [B] -> stats f64 [B, 8] (device), optionally momentary f64 [B, NB_max] (device).  Four
 * launches; the call only enqueues. */
int mt2_loudness(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                 int sample_rate, double* stats /*[B, 8]*/, double* momentary /*[B, NB_max] or NULL*/, int NB_max);
/* -> out f32 [B, L_max] (device; may be wav itself), optionally stats f64 [B, 8] (device) of the INPUT, the gain in field 7.  Five
 * launches; no copy to the host and no wait. */
int mt2_loudness_normalize(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                           int sample_rate, double target_lufs, double peak_ceiling /*<= 0: none*/, float* out /*[B, L_max]*/,
                           double* stats /*[B, 8] or NULL*/);

/* ---- EBU-mode metering (csrc/ebu.hip): what EBU R 128 / Tech 3341 asks of a meter beside integrated and momentary loudness - true
 * peak, short-term loudness and loudness range - and normalisation under a true-peak ceiling.  No reference counterpart.  Parity with
 * libebur128 / pyloudnorm is unpinned - neither is on hand; Tech 3341 cases 20-23 and Tech 3342 cases 5-6 need the EBU's recorded
 * files, which are not on hand either.  The kernels are held to analytic truths (the true peak of a band-limited tone is its amplitude
 * whatever the sampling phase; the loudness range of a two-level tone is the difference of the levels, Tech 3342 cases 1-4) and to the
 * float64 restatement tests/ebu_ref.py.  THE RULE, for one utterance x f32 [L] at sample_rate; h, ns and S[j] as in the loudness rule:
 *  1 True peak (ITU-R BS.1770-4 Annex 2, with a filter of this library's own).  o = ceil(192000 / sample_rate) phases: 12 at 16 kHz, 9 at
 *    22.05 kHz, 4 at 48 kHz, 1 at 192 kHz, at most 24.  Phase 0 is the sample itself, unfiltered, so true peak >= sample peak holds
 *    exactly.  Phases p = 1 .. o - 1 are a Kaiser-windowed sinc with its cutoff at Nyquist: Z = 12 zero crossings a side (24 taps per
 *    phase), beta = 8;  h[p][k] = sinc(t) I0(beta sqrt(1 - (t / Z)^2)) / I0(beta), t = (k - Z + 1) - p / o, k = 0 .. 2 Z - 1, sinc(t) =
 *    sin(pi t) / (pi t), built in double and rounded once to f32.  y[i o + p] = sum_k h[p][k] x[i - Z + 1 + k], one f32 fma chain from
 *    0 with k ascending;  x = 0 outside [0, L);  i runs over [-Z, L), so the ringing in front of and behind the signal counts.
 *    TP = max |y|, taken with v > m from m = 0: a NaN never wins, an Inf does (the sample peak's convention).  dBTP = 20 log10 TP.
 *    With these constants tones of amplitude A at fs/4 (0 and 45 degrees), fs/6 (60) and fs/8 (67.5) under a 10 ms raised-cosine
 *    fade read within +0.003 / -0.108 dB of A at 8, 16, 22.05, 44.1 and 48 kHz (Tech 3341 allows +0.2 / -0.4);  an abrupt onset
 *    overshoots by up to 0.7 dB, which is a property of the truncated signal.
 *  2 Short-term loudness.  nst = max(0, ns - 29) blocks of 3 s every 100 ms, only blocks wholly inside the signal.  z3[k] = (S[k] +
 *    ... + S[k + 29]) / (30 h), summed ascending from S[k];  s[k] = -0.691 + 10 log10 z3[k] (-inf for z3 = 0).
 *  3 Loudness range (EBU Tech 3342).  Gamma_r = -0.691 + 10 log10(mean of z3 over s > -70) - 20, the mean in the fixed order of the
 *    loudness rule (partial sums over k = i, i + 256, ... ascending for i < 256, then a halving tree);  -inf with no block over -70.
 *    A block is over a gate unless s <= gate, so a NaN block counts.  Over the n blocks over both gates, sorted ascending g[0 .. n)
 *    with a NaN last:  P10 = g[((n - 1) 10 + 50) / 100], P95 = g[((n - 1) 95 + 50) / 100] in integer division (Tech 3342's
 *    round((n - 1) p / 100 + 1) in 0-based integers);  LRA = P95 - P10;  n = 0 (under 3 s, or silent): LRA, P10 and P95 are NaN.  The
 *    two are elements of the set, selected exactly.  A non-finite sample makes every later block of its utterance NaN, hence its LRA
 *    NaN unless it sits in the last 5 % of the blocks, and changes nothing of another utterance.
 *  4 stats f64 [18] per utterance:  0-7 the row of mt2_loudness, bit for bit (7 the gain of 5 below; 1 for the measuring call)
 *    8 TP (linear)   9 o   10 LRA   11 nst   12 short-term blocks over the absolute gate   13 over both gates   14 Gamma_r   15 P10
 *    16 P95   17 max_k s[k] (-inf for nst = 0).  short_term f64 [NST_max]: s[k], -inf for k >= nst.
 *  5 Normalisation under a true-peak ceiling:  g = 10^((target_lufs - I) / 20) in double;  where TP > 0 and c = 10^(ceiling_dbtp / 20) /
 *    TP is smaller, g = c;  g is rounded once to f32 - toward zero where the cap binds, to nearest otherwise;  out[i] = x[i] g, one f32
 *    product;  zeros in [L, L_max).  g = 1 exactly and the utterance copied unchanged when I is not finite or g does not fit f32.  A
 *    binding ceiling lowers the loudness reached (one gain, no limiter).  The gain is formed and read on the device: the call only
 *    enqueues.
 *  6 The max and the selection are order-free and every sum's order depends on the block's index in its utterance alone, so a ragged
 *    batch is bit-identical to its utterances alone, whatever the slot, L_max or B.  A sample at or beyond L is never read.
 * Refused, on the host before the first HIP call, every output as it was:  all that mt2_loudness refuses;  a non-finite ceiling_dbtp;
 * NST_max < 1 or smaller than the short-term blocks of the longest utterance while `short_term` is given;  overlapping buffers.
 * `m` may be a bare handle;  scratch comes from its arena. */
#define MT2_EBU_FIELDS 18
#define MT2_TP_ZERO_CROSSINGS 12
#define MT2_TP_TAPS 24
#define MT2_TP_TILE 1024 /* positions i of one workgroup of the true-peak kernel: tile t holds i in [1024 t - 12, 1024 (t + 1) - 12) */
/* o, the taps per phase, the tile of the true-peak kernel, nst and the arena bytes of a call with ONE utterance of L samples;  host
 * only, no HIP call (outputs may be NULL).  A call with B utterances, the longest with ns sub-blocks and nst short-term blocks, takes
 * r(4 (4 ceil(B / 4) + 32 + 24 o)) + r(32 B ns) + r(8 B ns) + r(12 B) + r(64 B) + r(8 B nst) bytes, r(x) = max(256, x rounded up to
 * 256): lengths, carry matrix and filter table; chunk states; S; the peak, gain and true-peak words; the loudness rows; z3 / keys. */
int mt2_ebu_query(int sample_rate, long long L, int* oversample, int* taps, int* tile, int* short_term_blocks, long long* workspace_bytes);
/* the interpolation table f32 [o][24] of rule 1 (row 0 is the unit sample);  host only, no HIP call */
int mt2_true_peak_table(int sample_rate, float* table /*[o][24]*/);
/* wav f32 [B, L_max] (device), lens host int32 [B] -> stats f64 [B, 18] (device), optionally momentary f64 [B, NB_max] as mt2_loudness
 * writes it and short_term f64 [B, NST_max] (device).  Six launches; the call only enqueues. */
int mt2_loudness_ebu(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                     int sample_rate, double* stats /*[B, 18]*/, double* momentary /*[B, NB_max] or NULL*/, int NB_max,
                     double* short_term /*[B, NST_max] or NULL*/, int NST_max);
/* -> out f32 [B, L_max] (device; may be wav itself), optionally stats f64 [B, 18] (device) of the INPUT, the gain in field 7.  Seven
 * launches; no copy to the host and no wait. */
int mt2_loudness_normalize_tp(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                              int sample_rate, double target_lufs, double ceiling_dbtp, float* out /*[B, L_max]*/,
                              double* stats /*[B, 18] or NULL*/);

/* ---- True-peak look-ahead limiter (csrc/limiter.hip): a gain s[i] <= 1 per sample under which G x holds a true-peak ceiling, so that
 * normalisation under a ceiling reaches its target loudness where the one gain of rule 5 above gives way.  Offline and symmetric (it
 * looks as far ahead as behind);  no reference counterpart.  Parity with any outside limiter and audible quality on real speech are
 * unpinned;  the kernels are held to the rule's own properties and to the float64 restatement tests/limiter_ref.py.  THE RULE, for one
 * utterance x f32 [L] at sample_rate;  o, Z, h[p][k] and y are those of the true-peak rule:
 *  1 Window.  H = floor(sample_rate window_ms / 1000 + 0.5), in double;  W = 2 H + 1.  w[k] = 0.5 - 0.5 cos(2 pi (k + 1) / (2 H + 2)),
 *    k = 0 .. 2 H, in double, divided by their sum (added ascending) and rounded once to f32.  Default 5 ms: H = 80 at 16 kHz.
 *  2 Envelope, once per call, from x itself.  e[i] = max over p of |y[i o + p]| for i in [-1, L) - the f32 fma chains of the true-peak
 *    rule, the max taken with v > m from 0, so a NaN never wins and an Inf does.  E[i] = max(e[i - 1], e[i]) for i in [0, L): every
 *    oversampled position in (i - 1, i + 1).  The ringing in front of i = -1 and behind L - 1 is left to step 6.
 *  3 Need, per pass with pre-gain G (f32).  a = G E[i], one f32 product;  need[i] = c / a (one f32 division) if a > c, else 1;
 *    c = (f32) 10^(ceiling_dbtp / 20);  need = 1 outside [0, L).
 *  4 Hold.  m[i] = min of need over [i - H, i + H].
 *  5 Smooth and clamp.  d[i] = sum_k w[k] (1 - m[i - H + k]), 1 - m one f32 subtraction, one f32 fma chain from 0 with k ascending;
 *    s[i] = min(need[i], 1 - d[i]).  Hence s <= need always, and s = 1 exactly wherever need is 1 over [i - 2 H, i + 2 H].
 *    out[i] = (x[i] G) s[i], two f32 products;  zeros in [L, L_max).
 *  6 Trim.  s varies inside the interpolator's window, so the true peak TP' of out, measured by the true-peak rule, can differ from c
 *    by a little.  t = 1 where TP' <= c, else (double) c / TP' rounded toward zero to f32;  out is scaled by t in place (one f32
 *    product, none where t = 1).
 *  7 Normalising form, P passes (1 .. 4, default 2).  G_1 = 10^((target_lufs - I(x)) / 20) rounded to f32.  Pass k runs 3-6 on x with
 *    G_k and measures I_k of its output by the loudness rule;  for k < P, G_(k+1) = G_k 10^((target_lufs - I_k) / 20), formed in double
 *    on the device and rounded once to f32 (G_k is kept where I_k or the product is not finite).  The output is pass P's.  An
 *    utterance whose I(x) is not finite, or whose G_1 does not fit f32, is copied unchanged (G = s = t = 1), as in the loudness
 *    rule.  Everything is enqueued: no copy to the host and no wait.
 *  8 stats f64 [24] per utterance:  0-17 mt2_loudness_ebu's row of the INPUT, bit for bit, with field 7 the final G   18 H
 *    19 min s (1 where no sample was limited)   20 samples with s < 1   21 TP' before the trim   22 t   23 I of the final output.
 *    19-22 are the last pass's.
 *  9 Optional device outputs:  gain f32 [B, L_max], s of the last pass, 1 in [L, L_max);  need f32 [B, L_max] likewise.
 * 10 The max, the min and the count are order-free and every chain's order depends on the sample's index in its utterance alone, so a
 *    ragged batch is bit-identical to its utterances alone, whatever the slot, L_max or B.  A sample at or beyond L is never read.
 *    A non-finite sample changes its own utterance only.
 * Refused, on the host before the first HIP call, every output as it was:  all that mt2_loudness_normalize_tp refuses;  a non-finite
 * window_ms or pre_gain_db, H outside [1, 1024], a pre-gain that is not a positive finite f32, passes outside [1, 4];  gain, need or stats
 * misaligned or overlapping anything (out may be wav itself).  `m` may be a bare handle;  scratch comes from its arena. */
#define MT2_LIMITER_FIELDS 24
#define MT2_LIMITER_TILE 1024 /* samples of one workgroup of both limiter kernels: tile t holds i in [1024 t, 1024 (t + 1)) */
#define MT2_LIMITER_MAX_HALF_WINDOW 1024
#define MT2_LIMITER_MAX_PASSES 4
/* H, the tile of the limiter kernels and the arena bytes of a call with ONE utterance of L samples, whatever the passes;  host only, no
 * HIP call (outputs may be NULL).  A call with B utterances, the longest of L samples, takes what mt2_ebu_query states and
 * r(4 Wp) + 2 r(4 B Lp) + r(64 B) + r(12 B) + r(144 B) + r(64 B) bytes, Wp = W rounded up to 4, Lp = L rounded up to 4: the weights;  E
 * and the output of a pass that is not the last;  the min, count, true-peak and peak words of four passes;  G, the copy flag and t;
 * the meter's row;  a pass's loudness row. */
int mt2_limiter_query(int sample_rate, long long L, double window_ms, int* half_window, int* tile, long long* workspace_bytes);
/* the weights f32 [2 H + 1] of rule 1;  host only, no HIP call */
int mt2_limiter_window(int sample_rate, double window_ms, float* w /*[2 H + 1]*/);
/* One pass with a host-given gain G = (f32) 10^(pre_gain_db / 20):  wav f32 [B, L_max] (device), lens host int32 [B] -> out f32
 * [B, L_max] (device; may be wav itself), optionally gain and need f32 [B, L_max] and stats f64 [B, 24] (device; fields 0-17 are the
 * input's meter row, 23 is measured only with stats).  The call only enqueues. */
int mt2_limit_true_peak(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max, int B,
                        int sample_rate, double pre_gain_db, double ceiling_dbtp, double window_ms, float* out /*[B, L_max]*/,
                        float* gain /*[B, L_max] or NULL*/, float* need /*[B, L_max] or NULL*/, double* stats /*[B, 24] or NULL*/);
/* Rule 7:  each utterance brought to target_lufs under the true-peak ceiling by `passes` passes of the limiter.  No copy to the host
 * and no wait. */
int mt2_loudness_normalize_limited(mt2_model* m, void* stream, const float* wav /*[B, L_max]*/, const int32_t* lens /*host*/, int L_max,
                                   int B, int sample_rate, double target_lufs, double ceiling_dbtp, double window_ms, int passes,
                                   float* out /*[B, L_max]*/, float* gain /*[B, L_max] or NULL*/, float* need /*[B, L_max] or NULL*/,
                                   double* stats /*[B, 24] or NULL*/);

/* ---- the whole of Megatts.forward's no_grad block (models/megatts2.py:353-368 [+370]) for a batch,
 * activations staying in the packed internal layout between stages.
 *   forced_dur   (host, optional) int32 [B, Np_max]: replaces the ADM's integer durations AFTER the ADM
 *                has run (benchmarks on synthetic weights).  NULL: the ADM's own
 *                durations are copied to the host (one stream synchronisation, as in the reference).
 *   forced_codes (device, optional) int64 [B, Tq_cap]: replaces the PLM (config C2).
 *   flags: bit0 run the PLM (ignored when forced_codes given), bit1 run the vocoder, bit2 skip the ADM.
 * Outputs: mel f32 [B, Tm_cap, mel_bins] (time-major), mel_lens (host) int32 [B], optional
 * dur_out int32 [B, Np_max] (device), codes_out int64 [B, Tq_cap] (device),
 * wav f32 [B, hop*(Tm_cap + 2*hg_inference_padding)].
 * Tm_cap / Tq_cap are capacities; an utterance longer than Tm_cap is an error.
 * Phone ids and forced codes (the whole zero-padded [B, Tq_cap] tensor) are range-checked on the device before
 * use - one stream synchronisation at the start of the call; an id outside its table is an error (the reference
 * raises IndexError from nn.Embedding), never an out-of-bounds read. */
#define MT2_RUN_PLM 1
#define MT2_RUN_VOCODER 2
#define MT2_SKIP_ADM 4
#define MT2_PROMPT_VQPE 8   /* also run VQProsodyEncoder.forward (modules/vqpe.py:50-62) on the PROMPT mel, on an internal
                             * stream beside the ADM: prompt_codes int64 [B, ceil(Tp_max / vq_stride)] (device) receives
                             * its prosody codes (what a prompt-conditioned PLM or stage-2 extraction consume) */
int mt2_synthesize_batch(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens /*host*/,
                         int Np_max, const float* prompt_mel, const int32_t* prompt_lens /*host*/, int Tp_max,
                         int B, const int32_t* forced_dur /*host*/, const int64_t* forced_codes, int Tq_cap,
                         int flags, float* mel, int Tm_cap, int32_t* mel_lens /*host*/, int32_t* dur_out,
                         int64_t* codes_out, float* wav, int64_t* prompt_codes);

/* ---- prompt-conditioned synthesis as ONE call: the layout the PLM is trained on
 * (modules/datamodule.py:161-177,196-212) at inference.  `prompt_phone` int64 [B, Npp_max] (device) / `prompt_phone_lens` (host) /
 * `prompt_dur` int32 [B, Npp_max] (HOST) are the prompt utterance's own phones and alignment (sum over an utterance = its
 * prompt frames; every prompt pools to the same ceil(frames / vq_stride) = P).  The prompt's tc_latents (its phones against
 * the prompt mel, length-regulated by its alignment, max-pooled by vq_stride) stand in front of the target's as the PLM's
 * conditioning, the prompt's VQ-PE codes (computed here, returned in prompt_codes int64 [B, ceil(Tp_max / vq_stride)], the first P
 * of each row valid) behind the BOS; the PLM decodes the target's codes greedily from there (models/megatts2.py:165-181 on
 * that layout), then :361-368 [+370] as in mt2_synthesize_batch.  One MRTE mel-encoder pass per call; flags: MT2_RUN_VOCODER.
 * forced_dur (host, optional) replaces the ADM's durations after the ADM has run.  Other arguments as mt2_synthesize_batch. */
int mt2_synthesize_prompt_conditioned(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens /*host*/,
                                      int Np_max, const float* prompt_mel, const int32_t* prompt_lens /*host*/, int Tp_max, int B,
                                      const int64_t* prompt_phone, const int32_t* prompt_phone_lens /*host*/, int Npp_max,
                                      const int32_t* prompt_dur /*host*/, const int32_t* forced_dur /*host*/, int Tq_cap, int flags,
                                      float* mel, int Tm_cap, int32_t* mel_lens /*host*/, int32_t* dur_out, int64_t* codes_out,
                                      float* wav, int64_t* prompt_codes);
/* the two synthesis calls with the PLM's codes sampled (mt2_sampling; seeds[b] for utterance b).  NULL: greedy, identical to
 * the call without the suffix.  mt2_workspace_query bounds the arena of these calls too. */
int mt2_synthesize_batch_sampled(mt2_model* m, void* stream, const int64_t* phone, const int32_t* phone_lens /*host*/,
                                 int Np_max, const float* prompt_mel, const int32_t* prompt_lens /*host*/, int Tp_max,
                                 int B, const int32_t* forced_dur /*host*/, const int64_t* forced_codes, int Tq_cap,
                                 int flags, float* mel, int Tm_cap, int32_t* mel_lens /*host*/, int32_t* dur_out,
                                 int64_t* codes_out, float* wav, int64_t* prompt_codes, const mt2_sampling* sampling);
int mt2_synthesize_prompt_conditioned_sampled(mt2_model* m, void* stream, const int64_t* phone,
                                              const int32_t* phone_lens /*host*/, int Np_max, const float* prompt_mel,
                                              const int32_t* prompt_lens /*host*/, int Tp_max, int B,
                                              const int64_t* prompt_phone, const int32_t* prompt_phone_lens /*host*/,
                                              int Npp_max, const int32_t* prompt_dur /*host*/,
                                              const int32_t* forced_dur /*host*/, int Tq_cap, int flags, float* mel,
                                              int Tm_cap, int32_t* mel_lens /*host*/, int32_t* dur_out, int64_t* codes_out,
                                              float* wav, int64_t* prompt_codes, const mt2_sampling* sampling);

/* ---- tuning.  Every switch lives in the handle (no process-global state): two handles do not see each other's settings.  None
 * changes results beyond f32 summation order.  The 31 names (default in parentheses; the options the A/B records closed
 * were retired with their code and are unknown names now):
 *   stream groups   "ar_groups" (2; 1..8: the sequences of an autoregressive run are dealt into that many independent kernel chains
 *                   on internal HIP streams that fork from and join back into `stream`), "adm_groups" / "plm_groups" (0: per-stage
 *                   override), "voc_streams" (3: the three ResBlocks of a HiFi-GAN MRF side by side);
 *   arithmetic      "x3h" (15: bit mask of the fp16-pipe three-product forms - 1 loader-wave GEMM tiles, 2 K-split tiles of the AR
 *                   steps, 4 window convolutions, 8 long-sequence attention; 0 = the bf16 six-product forms, what the range guard's
 *                   repeat runs), "x6_conv" (1), "x6_gemm" (1), "x6_ks" (4), "win_conv" (1), "splitk" (1: K slices reduced by the next
 *                   LayerNorm), "skinny_tm" (1: launches of at most "skinny_rows" = 64 rows on the tile-major weight-streaming
 *                   kernel incl. its LayerNorm prologue), "skinny_nw" (16), "skinny_pairs" (1), "ln_pairs_adm" (2: LayerNorm
 *                   statistics handed from GEMM to GEMM in the ADM's layers), "ln_pairs_maxm" (1280), "ldr_prio" (3: s_setprio of the
 *                   loader waves), "a_planes" (3: bit mask of the producers that hand an activation to an x3h GEMM as fp16 planes -
 *                   1 LayerNorm kernels, 2 ff.0's epilogue -> ff.3, 4 attention -> out-projection), "up_fuse" (3: bit mask 1 | 2 = the MRF mean in front of the 64- | 128-channel
 *                   stride-2 upsampler fused into it), "pair_fuse" (3: bit mask
 *                   of the HiFi-GAN stages whose resblock conv pairs x + conv2(lrelu(conv1(lrelu(x)))) run as ONE launch, bit-identical
 *                   to the two launches - 1 the 32-channel stage, 2 the 64-channel stage, 4 the 128-channel stage), "ks_epi4" (1: the
 *                   fp16-pipe K-split tiles finish with 16-byte loads and stores where the layout allows, bit-identical to 0);
 *   thresholds      "t_x3h_128" (72), "t_x6_256" (160), "t_x6_128" (72), "t_ks4" (256), "t_ks2" (640), "t32" (64), "t32x32" (160)
 *                   (tile counts at which the tile choice changes), "attn_x6_min" (192), "attn_lds_min" (640) (queries per sequence);
 *   measurement     "force_gemm_config" (-1), "stage_markers" (0), "ldr64" (0).
 * Unknown names are an error. */
int mt2_set_option(mt2_model* m, const char* name, int value);
int mt2_get_option(mt2_model* m, const char* name, int* value);
int mt2_set_ar_groups(mt2_model* m, int groups);

/* ---- measurement support: time (ms, HIP events on `stream`) spent in each stage of the last
 * mt2_synthesize_batch when profiling was enabled with mt2_set_profiling(m, 1).
 * names: "mrte", "adm", "regulate", "plm", "decoder", "vocoder".  Returns the number of stages. */
int mt2_set_profiling(mt2_model* m, int enable);
int mt2_last_stage_ms(mt2_model* m, const char** names, float* ms, int cap);

/* ---- kernel-level entry points (parity tests and micro-benchmarks call the engine directly)
 * C[M,N] = act(conv/linear(X) + bias) * scale + R, see megatts2_amd/csrc/mt2_kernels.h GemmP. */
int mt2_op_gemm(void* stream, const float* X, int ldx, int Rx, const int32_t* rowbase, int a_mul, int shift0,
                int taps, int dil, int Cin, const float* W, int ldw, const float* bias, const float* R, int ldr,
                const int32_t* valid, float* C, int ldc, int M, int N, int pro_act, float pro_slope, int epi_act,
                float out_scale, int force_cfg);
/* Window convolution with the weights additionally given as three bf16 planes W3 [3][N][K] (device uint16; truncation
 * split: W = W3[0] + W3[1] + W3[2] exactly): the kernel may then run on the bf16 matrix pipe in the f32-equivalent
 * 6-product form (conv_win_x6_kernel; force_cfg 34 / 58 / 59 = 32 / 64 / 128 channels, or -1 for the automatic choice; a retired
 * configuration index answers hipErrorNotSupported). */
int mt2_op_gemm_x6(void* stream, const float* X, int ldx, int Rx, int shift0, int taps, int dil, int Cin, const float* W,
                   const void* W3, const float* bias, const float* R, int ldr, const int32_t* valid, float* C, int ldc,
                   int M, int N, int pro_act, float pro_slope, int epi_act, int force_cfg);
/* The same launch with the weights ALSO as two fp16 planes (hi, lo * 2^11) of the row-scaled matrix - Wh: chunk-interleaved,
 * [N][ceil32(K) / 32] blocks of 128 bytes = 32 hi then 32 lo values of one row and 32-k chunk, 128-byte aligned - and the inverse
 * power-of-two row scales wh_inv [N] (mt2_x3h_split): the Linear / Conv1d of modules/transformer.py:35-57,88-102 and
 * modules/convnet.py:23-31 on the fp16 matrix pipe in the f32-equivalent THREE-product form (csrc/gemm_x3h.hip; force_cfg 103 = the
 * 128x128 loader tile, 95 / 96 / 97 = the K-split tiles, 98 / 99 / 100 = window convolutions of 32 / 64 / 128 channels, or -1).  Test
 * conventions of this entry point: force_cfg + 1000 = the loaders' 64-bit address form, + 2000 = X holds fp16 planes written by a
 * producer kernel (mt2_op_layernorm with act + 100, or this entry with + 4000), + 4000 = C is stored as such planes (loader tile only).
 * range_flag (device int32, may be NULL): |= 1 when an activation with |a| >= 65504 was converted (fp16 range). */
int mt2_op_gemm_x3h(void* stream, const float* X, int ldx, int Rx, int shift0, int taps, int dil, int Cin, const float* W,
                    const void* W3, const void* Wh, const float* wh_inv, const float* bias, const float* R, int ldr,
                    const int32_t* valid, float* C, int ldc, int M, int N, int pro_act, float pro_slope, int epi_act, int force_cfg,
                    int32_t* range_flag);
/* host helper: the fp16-pipe operand format of a row-major f32 matrix W [rows][row_len] (host memory): planes
 * [rows][2 * ceil32(row_len)] uint16 (fp16 bit patterns; per row and 32-k chunk 32 hi values, then 32 lo values; K zero-padded to a
 * multiple of 32), inv [rows] */
int mt2_x3h_split(const float* W, long long rows, long long row_len, uint16_t* planes, float* inv);
/* host helper (no device): how a launch with `groups` groups, weight pointer `w_off` elements into a buffer that was split as
 * [rows][row_len] (mt2_x3h_split), row stride ldw and group stride strideW walks that buffer's fp16 planes - the rule the model
 * applies to every launch (csrc/x3h_planes.h, x3h_group_planes).  *form = 0: the launch cannot use the planes (the other outputs are
 * 0); 1 "whole": the groups step through whole matrices, rows and scales move together; 2 "slices": the groups are K slices of the
 * same rows and share their scales.  *wh_off: byte offset of Wh in the plane buffer, *wh_ldb: bytes per plane row, *wh_gstride:
 * bytes between groups, *inv_off: element offset of wh_inv, *wh_inv_stride: scales between groups. */
int mt2_x3h_group_planes(long long row_len, long long w_off, long long ldw, long long strideW, long long groups, int32_t* form,
                         long long* wh_off, long long* wh_ldb, long long* wh_gstride, long long* inv_off, long long* wh_inv_stride);
/* Kernel tests of GROUPED launches (grid.z = groups; tests/test_gpu_gemm_groups.py): one launch of the engine with every operand,
 * stride and leading dimension of its parameter block (csrc/mt2_kernels.h, GemmP) given explicitly - nothing is defaulted and
 * force_cfg carries no offsets.  K = taps * Cin.  Group g reads X + g * strideX, W + g * strideW (W3 likewise, in bf16 elements, its
 * three planes w3_plane elements apart), Wh + g * wh_gstride BYTES, wh_inv + g * wh_inv_stride, bias + g * strideB, R + g * strideR
 * and writes C + g * strideC; a stride of 0 shares the operand.  One group of a grouped launch is the same descriptor with
 * groups = 1 and the pointers moved by the strides.  W3 / Wh / wh_inv / rowbase / bias / R / valid / range_flag may be NULL;
 * a_planes = 1: X holds fp16 planes.  range_flag: device int32, |= 1 when an fp16-pipe launch converted an activation with
 * |a| >= 65504.  cfg_out (host, may be NULL): the configuration index the routing chose (-1: rejected before a choice).
 * ks_epi4: the option of that name for this launch (0: the x3h K-split tiles keep their dword finish); epi4_out (host, may be NULL):
 * 1 when the launch finished its tiles with 16-byte loads and stores.
 * struct_bytes = sizeof(mt2_gemm_desc) as the caller sees it: a mirror of the struct laid out differently is an error, not a launch. */
typedef struct mt2_gemm_desc {
    int32_t struct_bytes;
    const float* X; long long strideX; int32_t ldx, Rx;
    const int32_t* rowbase; int32_t a_mul, shift0, taps, dil, Cin;
    const float* W; long long strideW; int32_t ldw;
    const void* W3; long long w3_plane;
    const void* Wh; const float* wh_inv; long long wh_ldb, wh_gstride, wh_inv_stride;
    int32_t a_planes;
    const float* bias; long long strideB;
    const float* R; long long strideR; int32_t ldr;
    const int32_t* valid;
    float* C; long long strideC; int32_t ldc;
    int32_t M, N, groups;
    int32_t pro_act; float pro_slope; int32_t epi_act; float out_scale;
    int32_t force_cfg;
    int32_t* range_flag;
    int32_t* cfg_out;
    int32_t ks_epi4;
    int32_t* epi4_out;
} mt2_gemm_desc;
int mt2_op_gemm_grouped(void* stream, const mt2_gemm_desc* d);
/* Range guard of the fp16-pipe kernels inside a model handle (option "x3h", default 15): waits for the handle's last call, then
 * *tripped = 1 (and the guard is re-armed) when that call converted an activation outside the fp16 range - its outputs are then
 * to be discarded and the call repeated with mt2_set_option(m, "x3h", 0) (the bf16 six-product form has f32's exponent range). */
int mt2_x3h_guard(mt2_model* m, int* tripped);
/* LayerNorm statistics handed from GEMM to GEMM (round 5; the AR layers of models/megatts2.py:172-179,264-273 =
 * TransformerEncoderLayer.forward, modules/transformer.py:88-102: `x = x + out_proj(...)` followed by `norm2(x)`, `x = x + ff(...)`
 * followed by the next layer's `norm1(x)`).  ONE linear launch C = epi(X @ W^T + bias) + R on a bf16-pipe (x6) tile with
 *   stat_out != NULL: the epilogue also writes, per row and per wave tile of *stat_w columns, the pair (mean, M2) of the final C
 *     values: stat_out[M][*stat_nt][2] (*stat_nt = 0: the chosen tile has no such epilogue, nothing was written);
 *   ln_stat  != NULL: C = LayerNorm(X) @ Wo^T + b in its algebraic form on those pairs - W / W3 = gamma-folded weights
 *     W'[n,k] = gamma[k] Wo[n,k], bias = c[n] = sum_k beta[k] Wo[n,k] + b[n], ln_s[n] = sum_k W'[n,k]; mean / rstd of source row r
 *     merged (Chan, fixed order) from ln_stat[r][ln_nt][2] with ln_w columns per pair: rstd * (X W'^T - mean * s) + c. */
int mt2_op_gemm_x6_ln(void* stream, const float* X, int ldx, int Rx, int a_mul, int shift0, const float* W, const void* W3,
                      const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N, int K, int epi_act,
                      int force_cfg, float* stat_out, int32_t* stat_nt, int32_t* stat_w, const float* ln_stat, int ln_nt,
                      int ln_w, const float* ln_s, float ln_eps);
/* Linear layers of at most 64 rows on a TILE-MAJOR copy of the weights (round 4; gemm_skinny_tm_kernel - what the AR steps of one
 * utterance and the last-row launches of every batched AR step run on: F.linear at models/megatts2.py:172-179,264-273 with a
 * handful of rows).  mt2_op_tile_major turns a row-major [N, K] matrix (N a multiple of 16, K of 64) into blocks of 16 columns x 64 k,
 * block (nb, kb) at (nb * K/64 + kb) * 1024 floats, inside a block [j][lane][i] = W[nb*16 + lane%16][kb*64 + j*16 + (lane/16)*4 + i].
 * mt2_op_gemm_tm: C[g][M,N] = epi(pro(X[g] rows m*a_mul + shift0) @ Wsub[g]^T + bias) with Wsub[g] = rows [n0, n0 + N), columns
 * [k0, k0 + K) of the whole [*, Kw] matrix, moved by g * w_gstride row-major elements per group (split-K slabs: w_gstride = K).
 * ln_gamma != NULL: LayerNorm(X rows; gamma, beta, eps) as the prologue (K <= 1024, groups = 1) instead of pro_act.
 * pro_act + 0x100: the eight-wave form of the kernel (default: sixteen / twelve waves split K at M <= 32, round 5). */
int mt2_op_tile_major(void* stream, const float* W, int N, int K, float* out);
int mt2_op_gemm_tm(void* stream, const float* X, long long x_gstride, int ldx, int Rx, int a_mul, int shift0, const float* Wtm,
                   int Kw, int n0, int k0, long long w_gstride, int groups, const float* bias, const float* R, int ldr,
                   const int32_t* valid, float* C, long long c_gstride, int ldc, int M, int N, int K, int pro_act, float pro_slope,
                   int epi_act, const float* ln_gamma, const float* ln_beta, float ln_eps);
/* The same hand-off at a handful of rows (tile-major weight-streaming kernel, M <= 64): stat_out != NULL - the epilogue also writes
 * (mean, M2) of every final row per 16-column block, stat_out[M][N / 16][2]; ln_stat != NULL (with ln_gamma / ln_beta) - the LayerNorm
 * prologue takes mean / rstd of source row r from ln_stat[r][ln_nt = K / 16][2] instead of reading the rows. */
int mt2_op_gemm_tm_pairs(void* stream, const float* X, int ldx, int Rx, int a_mul, int shift0, const float* Wtm, int Kw,
                         const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N, int K, int epi_act,
                         const float* ln_gamma, const float* ln_beta, float ln_eps, float* stat_out, const float* ln_stat, int ln_nt);
int mt2_op_layernorm(void* stream, const float* x, int ldx, const float* gamma, const float* beta, const float* R1,
                     int ldr1, const int32_t* valid, float* out, int ldo, int M, int C, float eps, int act);
/* Test-only entries into the row kernels (csrc/rowops.hip; tests/test_gpu_rowops.py).  Every pointer is device memory.
 * mt2_op_layernorm_ex: one LayerNorm launch with every field of its parameter block -
 *   out[m] = mask * (act(LN(x[m]) * gamma[g] + beta[g]) + R1[m % r1_rows] + R2[m]),  g = m / rows_per_group, mask = valid[m % valid_rows]
 *   (rows_per_group / r1_rows / valid_rows = 0: one gamma / beta, R1 row m, valid[m]; R1, R2, valid, x3h_flag may be NULL);
 *   out_planes = 1 stores fp16 planes as mt2_op_layernorm's act + 100 does. */
int mt2_op_layernorm_ex(void* stream, const float* x, int ldx, const float* gamma, const float* beta, int rows_per_group,
                        const float* R1, int ldr1, int r1_rows, const float* R2, int ldr2, const int32_t* valid, int valid_rows,
                        float* out, int ldo, int M, int C, float eps, int act, int out_planes, int32_t* x3h_flag);
/* mt2_op_ln_reduce: the split-K consumer, xout = ((sum_{g < S} parts[g * pstride + m * C ..], g ascending) + bias) + R (bias, R and
 *   xout may be NULL; xout may alias R), hout = LN(xout) * gamma + beta (fp16 planes when h_planes = 1: M <= 4096 only).  The launcher
 *   picks one workgroup per row up to M = 4096 and one wave per row beyond. */
int mt2_op_ln_reduce(void* stream, const float* parts, long long pstride, int S, const float* bias, const float* R, int ldr,
                     const float* gamma, const float* beta, float* xout, int ldx, float* hout, int ldh, int M, int C, float eps,
                     int h_planes, int32_t* x3h_flag);
/* mt2_op_row: one row utility by name (embed_pe, gather_rows, pool_max, sum_groups, avg3, conv_post, fill_reflect, pack_rows,
 *   unpack_rows, adm_step_input, plm_step_input, adm_predict, adm_finalize, plm_finalize, adm_init_hist, plm_init_hist, check_ids,
 *   copy_2d, scatter_i64, expand_mask, unpack_wav, argmax_rows, vq_argmin, row_sqnorm, codebook_rows, reflect_pad_blocks, magnitude).
 *   The arguments are those of launch_<op> (csrc/mt2_kernels.h) in its order, split by kind: pointers -> ptrs, integers -> ints,
 *   floats -> flts.  An unknown name or a wrong count of any kind is an error (mt2_last_error) and launches nothing. */
int mt2_op_row(void* stream, const char* op, void* const* ptrs, int nptrs, const long long* ints, int nints, const float* flts,
               int nflts);
/* The PLM's sampling draw on A rows of N <= 1024 logits (row stride ld): out[j] (int64, device) = the code of row j under the
 * rule of mt2_sampling with Philox key seeds_dev[j] (uint64, device) and counter positions_dev[j] (int32, device).
 * s->seeds is not read here (may be NULL); the other fields are checked as for the _sampled calls. */
int mt2_op_sample_rows(void* stream, const float* logits, int ld, int N, int A, const mt2_sampling* s, const uint64_t* seeds_dev,
                       const int32_t* positions_dev, int64_t* out);
/* The interpolated draw on A PAIRS of rows (pair j = rows 2j, 2j + 1 of logits: context A, context B) with gamma_dev[j] (f32,
 * device): out (int64 [2 A], device) receives the code of pair j at 2j AND 2j + 1, as both histories do.  s NULL = greedy on the
 * mixture (seeds_dev / positions_dev are then not read). */
int mt2_op_sample_mix_rows(void* stream, const float* logits, int ld, int N, int A, const mt2_sampling* s,
                           const uint64_t* seeds_dev, const int32_t* positions_dev, const float* gamma_dev, int64_t* out);
int mt2_op_attention(void* stream, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                     float* O, int ldo, const int32_t* q_start, const int32_t* q_len, const int32_t* kv_start,
                     const int32_t* kv_len, int B, int H, int D, int max_qlen, float scale);
/* ... with the kernel choice exposed: lds_min_qlen = first query count served by the LDS-tiled kernel (0 never, < 0 default),
 * lds_waves = its query tiles per workgroup (8, otherwise 4); x6_min_qlen = first query count served by the bf16-pipe
 * kernel (f32-equivalent six-product form, head dims 64 / 96; 0 never, < 0 default); lds_waves + 32: the register kernel instead of the
 * head-dim-split kernel that serves D = 64 / 96 with at most 128 keys; lds_waves + 64: O receives fp16 planes (the operand format the
 * out-projection's x3h GEMM takes as it is: per 32 columns 32 hi | 32 lo fp16, same bytes per row; ldo % 32 == 0, O on 128 bytes);
 * lds_waves + 128: the bf16-pipe kernel in its fp16-pipe form (two fp16 planes per operand, three products; Q / K / V beyond the fp16
 * range are not reported through this entry point - the model's calls raise the handle's range guard);
 * max_kvlen: longest key range of the launch (0 = unknown). */
int mt2_op_attention_tuned(void* stream, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                           float* O, int ldo, const int32_t* q_start, const int32_t* q_len, const int32_t* kv_start,
                           const int32_t* kv_len, int B, int H, int D, int max_qlen, float scale, int lds_min_qlen,
                           int lds_waves, int x6_min_qlen, int max_kvlen);
/* The long-sequence kernel in its fp16-pipe form (two fp16 planes per operand, three products; head dims 64 / 96) with the range guard
 * exposed: range_flag (device int32) |= 1 when a Q / K / V value at or beyond 65504 was converted.  What mt2_synthesize_batch runs for
 * sequences of attn_x6_min queries or more under option x3h & 8 (reference modules/transformer.py:52-57, F.scaled_dot_product_attention). */
int mt2_op_attention_x3h(void* stream, const float* Q, int ldq, const float* K, int ldk, const float* V, int ldv,
                         float* O, int ldo, const int32_t* q_start, const int32_t* q_len, const int32_t* kv_start,
                         const int32_t* kv_len, int B, int H, int D, int max_qlen, float scale, int lds_waves, int max_kvlen,
                         int32_t* range_flag);
/* Kernel tests of the attention launches' GEOMETRY (tests/test_gpu_attention_geometry.py): one launch with every field of its
 * parameter block (csrc/mt2_kernels.h, AttnP) given explicitly - nothing is defaulted, no flag rides on another argument.
 * Ragged geometry: q_start / q_len / kv_start / kv_len (device int32 [B], all four or none) give the row range of sequence b in Q and
 * in K / V; its output rows start at o_start[b] (device int32 [B], may be NULL: q_start[b]).  Uniform geometry (the four arrays
 * NULL): sequence b starts at row b * u_qstride (queries) and b * u_kvstride (keys), has u_qlen / u_kvlen rows, and writes output rows
 * b * u_ostride + i (u_ostride = 0: u_qstride; o_start, when given, takes precedence here as well).  max_qlen sizes the grid;
 * max_kvlen: longest key range of a ragged launch (0 = unknown).  lds_min_qlen / x6_min_qlen: first query count served by the
 * LDS-tiled / matrix-pipe kernels (0: never); lds_waves: 0, 4 or 8 query tiles per workgroup of those; ds_short: 1 lets D = 64 / 96 with
 * at most 128 keys run on the head-dim-split kernel; x3h: 1 = the matrix-pipe kernel in its fp16-pipe form; o_planes: 1 = O receives fp16
 * planes (ldo % 32 == 0, O on 128 bytes).  range_flag (device int32, may be NULL): |= 1 when a value at or beyond 65504 was converted
 * to fp16.  kernel_out (host, may be NULL): the kernel the routing chose (MT2_ATTN_*; MT2_ATTN_NONE: nothing to launch, or rejected).
 * struct_bytes = sizeof(mt2_attn_desc) as the caller sees it: a mirror of the struct laid out differently is an error, not a launch.
 * Nothing about the buffers' sizes is known here: the caller answers for every row the geometry names. */
enum { MT2_ATTN_NONE = 0, MT2_ATTN_GENERIC = 1, MT2_ATTN_REG = 2, MT2_ATTN_DS = 3, MT2_ATTN_LDS = 4, MT2_ATTN_X6 = 5, MT2_ATTN_X3H = 6 };
typedef struct mt2_attn_desc {
    int32_t struct_bytes;
    const float* Q; int32_t ldq;
    const float* K; int32_t ldk;
    const float* V; int32_t ldv;
    float* O; int32_t ldo;
    const int32_t* q_start; const int32_t* q_len; const int32_t* kv_start; const int32_t* kv_len; const int32_t* o_start;
    int32_t u_qstride, u_qlen, u_kvstride, u_kvlen, u_ostride;
    int32_t B, H, D, max_qlen, max_kvlen; float scale;
    int32_t lds_min_qlen, x6_min_qlen, lds_waves, ds_short, x3h, o_planes;
    int32_t* range_flag;
    int32_t* kernel_out;
} mt2_attn_desc;
int mt2_op_attention_desc(void* stream, const mt2_attn_desc* d);
/* test hook, no device needed: what launch_attention (csrc/attention.hip, attn_route) would do with the launch `d` describes - no
 * pointer of `d` is dereferenced (Q / K / V / O may be NULL; O's alignment and whether q_start is NULL are looked at).  err: the
 * hipError_t it would return before launching (0: it launches, or there is nothing to launch); kernel: MT2_ATTN_*; tmpl[4]: the template
 * arguments that matter - head dim D (generic kernel: DT, 32-column tiles per wave), query tiles per workgroup, key tiles per workgroup
 * (head-dim-split kernel), split-KV waves (register kernel; generic kernel: waves across the head dim); launch[4]: grid x, y, z and
 * block size; lds: dynamic LDS bytes.  Returns 0, or -1 for a NULL or mis-sized descriptor. */
int mt2_attention_route(const mt2_attn_desc* d, int32_t* err, int32_t* kernel, int32_t* tmpl, int32_t* launch, long long* lds);
/* Launch trace of the GEMM/conv engine (measurement only): between begin and end every launch is
 * bracketed by HIP events on its own stream.  end() reports, per tile configuration, the number of
 * launches, the executed FLOPs (2*M*N*K*groups) and the summed kernel time in ms, plus a last entry named
 * "union" = length of the union of all launch intervals (launches on different internal streams overlap);
 * returns the number of entries written (<= cap). */
int mt2_gemm_trace_begin(mt2_model* m);
int mt2_gemm_trace_end(mt2_model* m, int cap, const char** names, int64_t* launches, double* flops, double* ms);
/* text table "config M N K groups launches ms tflops" of the traced launches grouped by shape, slowest first;
 * call BEFORE mt2_gemm_trace_end (which frees the records); returns the bytes written or -1 */
int mt2_gemm_trace_shapes(mt2_model* m, char* buf, int cap, int top);
/* Form log of the autoregressive step wiring and of the vocoder wiring (tests).  Between begin and end every decision the step layers
 * of the ADM / PLM (csrc/model_stages.hip, ar_step_layers) and the HiFi-GAN generator (hifigan_rows) take is recorded as one text line,
 * in call order:
 *     <kind> <point> <form> key=value ...
 *   kind   the layer that issued it: first-fill, first-incr, mid, last-skinny, last-split, last-fused
 *   ln_linear   skinny-ln | skinny-ln-pairs | pair-fed | plain | plain+planes      M= N= tile= nw=
 *   residual    split (S > 1 K slices) | stat (un-split, row statistics handed on) | nostat      S= stat_nt= stat_w= a_planes= M= K= tile= nw=
 *               (tile: the configuration name of the GEMM; nw: the waves that split K if it ran on the tile-major weight-streaming kernel, else 0)
 *   ln_pending  reduce (S > 0 slabs summed) | plain      S= h_planes= M=
 *   attention   generic | reg | ds | lds | x6 | x3h      o_planes= B= qlen= kvlen= D=  (ragged launches: kvlen is the longest key range)
 *   tail        fpl | nofpl (ff.0 stores fp16 planes for ff.3 or not)      S1= S2= M= att_planes=
 * and of the vocoder (ch: channels, R: rows of the stage, tile: the configuration name of the launch):
 *   kind   voc-pre, voc-stage<i> (upsampler i and its three resblocks), voc-post
 *   pre         gemm (conv_pre)      ch= R= tile=
 *   upsample    halves (one entry per GEMM half: half=) | fused (MRF mean + upsampler as one launch)      ch= R= tile=
 *   mean        avg3 | in-upsample | in-post: where the mean of the stage's three resblocks is formed      ch= R=
 *   pair        fused | two (tile / tile2: the first and second convolution)      j= n= ch= k= dil= R= tile= [tile2=]
 *   halo        fill (reflect edge mode: one entry per halo fill)      width= G=
 *   streams     1 | 3: the streams the stage's three resblock chains run on      ch= R=
 *   post        fused (mean + conv_post + tanh as one launch) | gemm      ch= k= R= tile=
 * and of the parallel stages in front of and behind the AR steps (tile: the configuration name of the launch; M: rows with their gaps):
 *   kind   mel-encoder (MRTE mel encoder), phone-encoder, cross (the cross attention of MRTE.tc_latent), vqpe, decoder
 *   conv        first | block (a ConvBlock of a residual stack) | mid (the strided middle convolution) | last | ff (conv-FF)
 *               tile= M= N= taps= groups= shared= (the groups read one input) wshared= (one weight) relued= (input stored ReLU'd) a_planes=
 *   linear      qkv | out | ff | q | kv | vq (the VQ distance GEMM)      tile= M= N= K= nw=
 *   ln          block (ReLU folded into the store) | residual (a stack's last, with the residual add) | plain      out_planes= act= M= groups=
 *   attention   as above
 * The log is per handle and off by default; it observes only - nothing is timed, no HIP call is made for it, and the launches and
 * their arguments are the same with it on or off.  end() turns it off, writes the lines ('\n'-separated, NUL-terminated) into buf
 * and returns the bytes written, or -1 (NULL arguments, or the text does not fit cap); the records are dropped either way. */
int mt2_form_log_begin(mt2_model* m);
int mt2_form_log_end(mt2_model* m, char* buf, int cap);
int mt2_gemm_config_count(void);
const char* mt2_gemm_config_name(int idx);
/* test hook, no device needed: what the GEMM front door (gemm_dispatch.hip) would do with the dense launch M x N x K (taps, dilation,
 * groups, prologue pro_act) - err: the hipError_t it would return before launching (0: it launches), cfg: the configuration index (-1:
 * none chosen), variant: the kernel variant of that tile, lds: dynamic LDS bytes, planes: bit 0 the launch could take its A operand as
 * fp16 planes, bit 1 it could write C as planes.  operands: which optional operands exist - 1 W3, 2 Wh + wh_inv, 4 Wtm, 8 stat_out,
 * 16 ln_stat, 32 R, 64 rowbase, 128 a_planes, 256 c_planes; all on 128 bytes except those named in `misaligned` (same bits; 512 X,
 * 1024 C).  force_cfg / x3h: the options of the same names.  Returns 0. */
int mt2_gemm_route(int M, int N, int K, int taps, int dil, int groups, int pro_act, int operands, int misaligned, int force_cfg,
                   int x3h, int* err, int* cfg, int* variant, long long* lds, int* planes);
/* ... the same launch with the rows of C and R ld_pad floats further apart (ldc = ldr = N + ld_pad) and the option ks_epi4 as given;
 * epi4 (may be NULL): 1 when an x3h K-split tile would finish the launch row-major with 16-byte loads and stores - N, ldc, ldr and, in
 * grouped launches, the group strides multiples of 4, C / R / bias / wh_inv on 16 bytes - 0 for its dword finish or any other kernel. */
int mt2_gemm_route_ex(int M, int N, int K, int taps, int dil, int groups, int pro_act, int operands, int misaligned, int force_cfg,
                      int x3h, int ld_pad, int ks_epi4, int* err, int* cfg, int* variant, long long* lds, int* planes, int* epi4);
/* test hook, no device needed: what launch_conv_pair (csrc/gemm_x3h.hip, conv_pair_route) would do with the resblock conv pair of C
 * channels, `taps` taps, first dilation `dil` over R rows - err: 0 it launches (or R <= 0: nothing to launch, grid 0), hipErrorNotSupported
 * (801) the two-launch form keeps the pair, hipErrorInvalidValue (1) bad arguments; lds: dynamic LDS bytes; grid / block: the launch;
 * bm / bmo: rows per pass / output rows per workgroup.  flags: 1 reflect padding, 2 no fp16 planes, 4 an operand of 2 GiB or more,
 * 8 an operand off its alignment.  pair_fuse / x3h: the options of the same names.  Returns 0. */
int mt2_conv_pair_route(int R, int C, int taps, int dil, int flags, int pair_fuse, int x3h, int* err, long long* lds, int* grid,
                        int* block, int* bm, int* bmo);
/* test entry: Y [R, ldy] = X + conv2(lrelu(conv1(lrelu(X)))) on the fused pair kernel - X [R, ldx] f32 (C channels), both weight
 * matrices [C][taps * C] as fp16 planes (mt2_x3h_split) with their inverse row scales, conv1 dilation `dil`, conv2 dilation 1, rows
 * with valid[m] == 0 written as zeros; pair_fuse: the option's mask (a clear bit answers hipErrorNotSupported as an error); range_flag
 * as mt2_op_gemm_x3h. */
int mt2_op_conv_pair(void* stream, const float* X, int ldx, int R, int C, int taps, int dil, float slope, const void* Wh1,
                     const float* inv1, const float* bias1, const void* Wh2, const float* inv2, const float* bias2,
                     const int32_t* valid, float* Y, int ldy, int pair_fuse, int32_t* range_flag);
/* test hook, no device needed: what launch_up_mrf (csrc/gemm_x3h.hip, up_mrf_route) would do with the fused MRF mean + stride-`stride`
 * transposed convolution of `ch` input channels over R rows - err / lds / grid / block as mt2_conv_pair_route; bm: rows per workgroup.
 * flags: 1 no fp16 planes, 2 an operand of 2 GiB or more, 4 the output off its alignment, 8 the planes off theirs, 16 a row stride that
 * is no multiple of 4, 32 a null input, 64 an output row stride below the width, 128 the bias off its alignment.  up_fuse / x3h: the
 * options of the same names; off: 1 win_conv off, 2 x6_conv off, 4 a forced configuration, 8 ldr64.  Returns 0. */
int mt2_up_mrf_route(int R, int ch, int stride, int flags, int up_fuse, int x3h, int off, int* err, long long* lds, int* grid, int* block,
                     int* bm);
/* test entry: Y [R, ldy] (= [2 R, ch / 2] time-major) = ConvTranspose1d(stride 2) of lrelu(((X0 + X1) + X2) * scale) on the fused kernel -
 * X0 / X1 / X2 [R, ldx] f32 (ch channels), Wh / inv: the [ch][2 ch] matrix [wlo rows | whi rows] as fp16 planes (mt2_x3h_split) with its
 * inverse row scales, bias [ch / 2], rows with valid[q] == 0 written as zeros; up_fuse: the option's mask (a clear bit answers
 * hipErrorNotSupported as an error); range_flag as mt2_op_gemm_x3h. */
int mt2_op_up_mrf(void* stream, const float* X0, const float* X1, const float* X2, int ldx, int R, int ch, float scale, float slope,
                  const void* Wh, const float* inv, const float* bias, const int32_t* valid, float* Y, int ldy, int up_fuse,
                  int32_t* range_flag);
/* time `iters` back-to-back launches of one GEMM / conv (taps, dilation) with HIP events on `stream`, cycling
 * through `w_copies` copies of the weight matrix (> 1: weights are not L2-resident from the previous launch);
 * flags bit0: leaky-ReLU prologue, bit1: bias + residual + row-mask epilogue, bit2: clock probe - one wave of the
 * loader-wave x6 kernel reads s_memtime and s_memrealtime around its K loop; `sustained_ghz` (nullable) receives the
 * shader clock that launch ran at (0 when the configuration has no probe), bit3: no stderr report, bit4: loader waves at the default
 * issue priority, bit5: no fp16-pipe forms, bit6: the x3h K-split tiles' dword finish (option ks_epi4 = 0); average ms */
int mt2_op_gemm_x3h_ln(void* stream, const float* X, int ldx, int Rx, int a_mul, int shift0, const float* W, const void* W3,
                       const void* Wh, const float* wh_inv, const float* bias, const float* R, int ldr, float* C, int ldc, int M, int N,
                       int K, int epi_act, int force_cfg, float* stat_out, int32_t* stat_nt, int32_t* stat_w, const float* ln_stat,
                       int ln_nt, int ln_w, const float* ln_s, float ln_eps);   /* mt2_op_gemm_x6_ln with the fp16 planes as well */
int mt2_bench_gemm(void* stream, int M, int N, int K, int taps, int dil, int flags, int force_cfg, int iters,
                   int w_copies, float* avg_ms, char* cfg_name, int cfg_name_cap, double* sustained_ghz);

#ifdef __cplusplus
}
#endif
#endif /* MEGATTS2_HIP_H */
