/*
 * evhip.h -- C ABI of libevhip.so: the MI355X-native (gfx950) EmotiVoice inference hot path.
 *
 * The reference has no FFI/plugin interface for this path; its boundary is the Python object
 * protocol of JETSGenerator (reference models/prompt_tts_modified/jets.py:26-71).  Each entry
 * point below replaces one piece of that protocol:
 *
 *   ev_create            <- JETSGenerator.__init__(config) + .to(device)      (jets.py:27-47,
 *                           inference_am_vocoder_joint.py:70)
 *   ev_load_weights[_device] <- .load_state_dict(ckpt['generator'])           (inference_am_vocoder_joint.py:72-73)
 *   ev_synthesize        <- JETSGenerator.forward, inference branch           (jets.py:50-71 ->
 *                           model_open_source.py:102-163 -> models/hifigan/models.py:115-131)
 *   ev_synthesize_prosody <- the same, with per-utterance speed / pitch / energy controls and per-token prosody overrides
 *                           fed through the embeddings and the length regulator exactly where the teacher-forced branch
 *                           feeds ps / es / ds (model_open_source.py:113-139); an extension, not part of the reference call
 *   ev_vocoder           <- HiFiGANGenerator.forward on pre-computed mels     (models/hifigan/models.py:115-131)
 *   ev_align             <- the teacher-forced branch's alignment: AlignmentModule + viterbi_decode + average_by_duration
 *                           (model_open_source.py:113-119, modules/alignment.py:27-162), batched on the device
 *   ev_get_stage         <- register_forward_hook taps used by the parity tests
 *   ev_last_error        <- Python exceptions (no exceptions cross the ABI)
 *
 * Conventions: 0 = OK, negative = error (message via ev_last_error).  A handle owns one device,
 * one HIP stream and one workspace arena; it is NOT thread-safe (the reference is single-threaded
 * per process as well).  Inputs are borrowed for the duration of a call.  Outputs are owned by
 * the handle and stay valid until the next ev_synthesize / ev_vocoder / ev_destroy on it.
 * No torch types appear anywhere in this interface: plain pointers and sizes only.
 */
#ifndef EVHIP_H_
#define EVHIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EV_ABI_VERSION 7      /* 2: ev_config engine switches (mx_residual, decoder_attention, fused_pairs), ev_abi_info;
                                 3: ev_config.mx_mrf / decoder_ln_planes, partial plane sets in ev_conv_gemm_desc (acc_h ..., mxo_partial);
                                 4: ev_config.token_splitk, ev_conv_gemm_desc.ksplit (same struct sizes);
                                 5: ev_default_config() sets decoder_precision = vocoder_precision = EV_PREC_MX, the mode that meets the 1e-3 contract
                                    (same struct sizes; until 4 the default was EV_PREC_F16 = 2.4e-3 on zero-mean audio);
                                 6: ev_config.mx_act_format (was reserved[0], same struct size): the fused C = 32 pairs of the MX generator default to
                                    E5M2 activation operands in the cross terms -- the results of the default mode change in their last bits;
                                 7: ev_config.mx_group appended (sizeof(ev_config) + 4): grouped launches of a stage's same-level ResBlock convs -- same bits */

typedef struct ev_handle ev_handle;

/* Mirrors reference config/joint/config.yaml:36-94 (+ n_vocab/n_speaker patched in by the
 * callers, inference_am_vocoder_joint.py:57-58).  Use ev_default_config() and override. */
typedef struct ev_config {
    int32_t abi_version;        /* EV_ABI_VERSION */
    int32_t n_vocab;            /* 502   */
    int32_t n_speaker;          /* 2014  */
    int32_t n_mels;             /* 80    */
    int32_t hidden;             /* 384 (encoder/decoder/variance hidden) */
    int32_t heads;              /* 8     */
    int32_t enc_layers;         /* 4     */
    int32_t dec_layers;         /* 4     */
    int32_t ffn_kernel;         /* 3     */
    int32_t bert_dim;           /* 768   */
    int32_t dur_layers;         /* 2     */
    int32_t pitch_layers;       /* 3     */
    int32_t energy_layers;      /* 2     */
    int32_t var_kernel;         /* 3     */
    int32_t var_embed_kernel;   /* 9     */
    int32_t n_up;               /* 4     */
    int32_t up_rates[8];        /* 8,8,2,2 */
    int32_t up_kernels[8];      /* 16,16,4,4 */
    int32_t up_init_ch;         /* 512   */
    int32_t n_rb;               /* 3     */
    int32_t rb_kernels[8];      /* 3,7,11 */
    int32_t rb_dils[8][4];      /* {1,3,5} x3 */
    int32_t n_rb_dils;          /* 3     */
    int32_t sample_rate;        /* 16000 */
    /* engine options (not in the reference) */
    int32_t decoder_precision;  /* EV_PREC_MX (default since ABI 5: split precision with the conv-FFN / projections in the MX arithmetic, see
                                   vocoder_precision), EV_PREC_X3 (split precision), EV_PREC_F32 (exact fp32 MFMA) or EV_PREC_F16 (opt-in, out of
                                   the 1e-3 contract on zero-mean audio) */
    int32_t keep_stages;        /* !=0: keep every Appendix-C stage tap retrievable by ev_get_stage */
    int32_t token_rate_split;   /* 1 (default): fp32 token-rate GEMMs as 3 fp16 MFMAs on hi/lo splits (fp32-level accuracy,
                                   ~4x faster); 0: exact fp32 MFMA (v_mfma_f32_16x16x4_f32) */
    int32_t vocoder_chunk_mb;   /* accepted and without effect in every precision (the field keeps the layout).  It selected row chunks sized for the
                                   Infinity Cache for the fp16 generator's ResBlocks: bit-identical, but 1-4 % slower than whole tensors in the full
                                   forward at every size measured, so that schedule was removed */
    int32_t vocoder_streams;    /* 0 (default): the three ResBlocks of a generator stage run concurrently (two internal streams beside
                                   the handle's); 1: everything on the handle's stream.  The pitch / energy predictors use the same two streams beside the
                                   duration predictor. */
    int32_t vocoder_precision;  /* EV_PREC_MX (default since ABI 5): the X3 data flow, but a product is ONE fp16 MFMA (hi x hi) + two block-scaled
                                   fp4 MFMAs for the cross terms (v_mfma_scale_f32_16x16x128_f8f6f4) on operand planes written by the producing
                                   layer: waveform within ~5e-4 of the reference on every fixture, zero-mean audio included (contract: 1e-3);
                                   EV_PREC_X3: fp32 activations, every product as three fp16 MFMAs on hi/lo splits (fp32-class accuracy);
                                   EV_PREC_F16 (opt-in): fp16 operands / fp16 activations in HBM, fp32 accumulate -- 1.6x faster, but 2.4e-3
                                   on zero-mean audio, i.e. OUTSIDE the 1e-3 contract */
    /* engine switches that used to be environment variables (read per layer per forward); all default to 0 */
    int32_t mx_residual;        /* EV_PREC_MX generator: 0 (default) = the residual stream of a ResBlock travels ONLY as the plane set its
                                   conv1 reads (fp16 hi plane + fp4 remainder codes; conv2's epilogue rebuilds x from it: 8.7 instead of
                                   14.1 bytes per element and conv2 launch, worst fixture 5.3e-4 instead of 4.4e-4); 1 = a separate fp32
                                   residual tensor beside the planes (round 3's flow) */
    int32_t decoder_attention;  /* decoder self-attention in the X3 / MX modes: 0 (default) = split precision (three fp16 MFMAs per
                                   product, K / V tiles staged through LDS); 1 = exact fp32 MFMA kernel (the token-rate encoder's) */
    int32_t fused_pairs;        /* 0 (default) = fused ResBlock-pair kernels where they exist (C = 32 every k, C = 64 / k = 3 in fp16); 1 = every
                                   conv as its own launch (A/B switch, bit-identical in the fp16 mode) */
    int32_t mx_mrf;             /* EV_PREC_MX generator, stages with >= 128 channels: 0 (default) = the running MRF sum of a stage's three ResBlocks travels
                                   as a partial plane set (fp16 hi plane + fp4 remainder codes + block scales: 2.53 instead of 4 bytes per element and
                                   transfer, re-quantised once per ResBlock; emulated cost 5e-6 of waveform error); 1 = an fp32 running sum */
    int32_t decoder_ln_planes;  /* EV_PREC_MX decoder: 0 (default) = the LayerNorms in front of the QKV projection and the conv-FFN write the plane sets those
                                   layers read (no fp32 copy, no separate quantisation pass; the same bits); 1 = fp32 output + a planes pass */
    int32_t token_splitk;       /* token-rate stack with split hi/lo GEMMs: 0 (default) = the phoneme encoder's second conv-FFN conv (N = hidden, K x taps = 4608:
                                   144 sequential (K-chunk, tap) steps per tile) runs split-K -- 4 ranges, partial sums reduced in range order by a second
                                   kernel -- because that chain is what a single utterance waits for (B = 1, 64 phonemes: 4.25 -> 3.95 ms; +0.08 ms per
                                   32 x 256-token batch).  Chosen by layer shape only: an utterance alone and in a batch gets the same bits.
                                   1 = every GEMM in one pass (the summation order of rounds 1-3) */
    int32_t mx_act_format;      /* EV_PREC_MX generator, format of the ACTIVATION operand in the two cross-term MFMAs where a kernel offers the choice (the fused
                                   ResBlock pairs at 32 channels): 0 (default) = OCP E5M2 without block maxima -- Q(xh) = the top byte of the fp16 hi part,
                                   Q(xl) = E5M2 of the remainder at the constant block scale 2^-11; per-element exponents, ~3x fewer quantiser instructions,
                                   emulated waveform error 2 % LOWER than fp4's; 1 = block-scaled fp4 (e2m1) as in ABI <= 5.  Weights are fp4 planes either way. */
    int32_t mx_group;           /* EV_PREC_MX generator, stages with >= 128 channels, large batches (ABI 7): 0 (default) = the same-level convs of a stage's three
                                   ResBlocks (k = 3 / 7 / 11: independent until the MRF sum) are issued as ONE grouped launch per level -- a launch of its own
                                   costs each conv 30-50 us of ramp and tail at B = 32 x 1024 frames -- with one set of intermediates per ResBlock
                                   (+ ~5 GB of workspace at that size); 1 = one launch per conv, ResBlock after ResBlock.  The same bits either way. */
} ev_config;

/* Precision of the frame-rate path (ev_default_config: MX for both components).  F16: fp16 MFMA operands (what BASELINE.json's bf16 / fp16 configs name).
 * F32: exact fp32 MFMA (decoder only; v_mfma_f32_16x16x4_f32, 1/16 of the fp16 rate).
 * X3:  fp32 activations in HBM, weights and activations split into fp16 hi + lo parts, x*w = hi*hi + hi*lo + lo*hi as three
 *      fp16 MFMAs with fp32 accumulation (2^-22 relative truncation: the fp32 rounding class at 1/3 of the fp16 rate).
 *      With decoder_precision = vocoder_precision = EV_PREC_X3 ("strict") the waveform matches the fp32 reference to ~1e-5
 *      relative L2 also on DC-free audio, where fp16 operands measure ~2e-3. */
enum { EV_PREC_F16 = 0, EV_PREC_F32 = 1, EV_PREC_X3 = 2, EV_PREC_MX = 3 };

/* flags for ev_synthesize / ev_vocoder */
enum {
    EV_FLAG_DEVICE_INPUTS = 1,  /* all input pointers are device pointers (zero-copy from a torch-ROCm tensor) */
    EV_FLAG_NO_VOCODER = 2,     /* acoustic model only (mel out) */
    EV_FLAG_WANT_INT16 = 4,     /* also produce the caller epilogue wav*32768 -> int16 (inference_am_vocoder_joint.py:130-131) */
    EV_FLAG_FORCED_DURATIONS = 8, /* teacher-forced durations (test mode): use result-independent durations passed via ev_set_forced_durations */
    EV_FLAG_DEVICE_MEL = 16      /* ev_align only: mel, pitch_frames and energy_frames are device pointers, the other inputs stay host pointers
                                    (an ev_features_result goes straight into ev_align) */
};

/* Result of one call.  All pointers are DEVICE pointers owned by the handle.
 * Packed layouts: utterance b occupies [mel_offsets[b], mel_offsets[b]+mel_lens[b]) rows of mel and
 * 256x that range of wav; tokens are packed exactly like the `ling` input (cu_seqlens). */
typedef struct ev_result {
    int32_t batch;
    int32_t total_tokens;
    int64_t total_frames;           /* sum of mel_lens */
    int64_t total_samples;          /* total_frames * prod(up_rates) */
    const float*   wav;             /* (total_samples,) fp32 in [-1,1]        = wav_predictions   */
    const int16_t* wav_i16;         /* (total_samples,) or NULL                                   */
    const float*   mel;             /* (total_frames, n_mels) fp32 row-major  = dec_outputs       */
    const int64_t* durations;       /* (total_tokens,)  int64                 = log_duration_predictions (inference) */
    const float*   log_durations;   /* (total_tokens,)  fp32, pre-round (test tap)                */
    const float*   pitch;           /* (total_tokens,)  fp32                  = pitch_predictions  */
    const float*   energy;          /* (total_tokens,)  fp32                  = energy_predictions */
    const int32_t* mel_lens;        /* (batch,) HOST pointer                                      */
    const int64_t* mel_offsets;     /* (batch+1,) HOST pointer: exclusive prefix sum of mel_lens  */
} ev_result;

void ev_default_config(ev_config* cfg);

/* What the loaded library was built as: EV_ABI_VERSION and the sizes of the structs a binding mirrors (ev_config, ev_result, and the two
 * descriptors of include/evhip_ops.h), so that a stale binding or a stale libevhip.so is an error at load time instead of a mis-parsed struct.
 * sizes: 4 entries {sizeof(ev_config), sizeof(ev_result), sizeof(ev_conv_gemm_desc), sizeof(ev_res_pair_desc)}; returns EV_ABI_VERSION. */
int ev_abi_info(size_t sizes[4]);

int ev_create(int device_id, const ev_config* cfg, ev_handle** out);
void ev_destroy(ev_handle* h);
const char* ev_last_error(ev_handle* h);   /* h may be NULL: returns the last creation error */

/* Use an externally owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream) instead of the
 * handle's own stream.  Pass NULL to go back to the internal stream. */
int ev_set_stream(ev_handle* h, void* hip_stream);

/* Packed weight blob produced by emotivoice_amd/packer.py (self-describing; manifest_json is an
 * optional human-readable copy of the table and may be NULL).  Host pointer: copied to the device.
 * Device pointer variant (after an RCCL broadcast): borrowed, must outlive the handle. */
int ev_load_weights(ev_handle* h, const void* blob, size_t nbytes, const char* manifest_json);
int ev_load_weights_device(ev_handle* h, const void* dptr, size_t nbytes, const char* manifest_json);

/* JETSGenerator.forward (inference): B utterances, tokens packed back to back.
 *   ling      (cu_seqlens[B],) int64 phoneme ids            = inputs_ling (unpadded)
 *   cu_seqlens(B+1,) int32 HOST pointer, cu_seqlens[0] = 0   = input_lengths as prefix sums
 *   speaker   (B,) int64                                     = inputs_speaker
 *   style     (B, bert_dim) fp32                             = inputs_style_embedding
 *   content   (B, bert_dim) fp32                             = inputs_content_embedding
 *   alpha     duration scale as GaussianUpsampling.forward applies it (alignment.py:183).  NB: the reference's inference branch
 *             never forwards JETSGenerator.forward's alpha to the length regulator (model_open_source.py:142), so the drop-in
 *             Python mirror always passes 1.0; values != 1 are an extension (speed control)
 * Every utterance is evaluated with the reference's B = 1 semantics (zero halo at sequence edges,
 * attention restricted to its own tokens / frames). */
int ev_synthesize(ev_handle* h, int B, const int64_t* ling, const int32_t* cu_seqlens,
                  const int64_t* speaker, const float* style, const float* content,
                  float alpha, uint32_t flags, ev_result* out);

/* Per-utterance prosody control (ev_synthesize_prosody).  For utterance b and its token j (packed index cu_seqlens[b] + j):
 *   p_src[j] = pitch[j] if pitch is given and pitch[j] is not NaN, else the predicted pitch;  e_src[j] likewise from energy;
 *   d_src[j] = durations[j] if durations is given and durations[j] >= 0, else the predicted clamp(round(exp(logd) - 1), 0);
 *   p[j] = pitch_scale[b] * p_src[j] + pitch_shift[b],  e[j] = energy_scale[b] * e_src[j] + energy_shift[b]
 *          (one fmaf; an utterance whose scale is 1 and shift 0 gets p_src unchanged, -0.0 included) -- p / e go into pitch_embed /
 *          energy_embed where the predictions go in ev_synthesize.  Units are the predictor's own: the checkpoint's normalised tracks;
 *   d_src is scaled by alpha[b] in the Gaussian upsampling exactly as ev_synthesize's alpha scales every utterance (float scale,
 *          mel_len = int(sum), all-zero guard); alpha == NULL: the call's alpha for every utterance.
 * ev_result.pitch / .energy / .durations / .log_durations keep returning the PREDICTIONS, so that a caller can edit them and send them back.
 * Identity controls (every pointer NULL, or scale 1, shift 0, all-NaN pitch / energy, all -1 durations, alpha[b] == alpha) give the
 * bits of ev_synthesize.  What was used can be read back with ev_get_stage: "dur_eff" (int64, every call) and, with keep_stages,
 * "pitch_eff" / "energy_eff" (the tracks the embeddings read).
 * Ordering of device per-token arrays: like ling, they are read in the order of the handle's stream (ev_set_stream), which the internal
 * stream gives no ordering against any other stream, the null stream included.  The caller makes sure they are written before the call:
 * produce them on the stream set with ev_set_stream, or synchronise the producing stream first (emotivoice_amd.prosody.pack_prosody does).
 * The device arrays of an ev_align_result qualify as they are: ev_align has completed them before it returns, and they stay valid across
 * this call (they live in ev_align's own workspace until the next ev_align), so a re-voicing passes them straight back here.
 * The per-utterance arrays are always HOST memory and are validated: alpha[b] > 0 and finite, scales / shifts finite.  The per-token arrays
 * follow EV_FLAG_DEVICE_INPUTS like ling.  Host per-token values are validated too: pitch / energy must not be +-inf, durations must lie
 * in [-1, EV_PROSODY_MAX_DURATION].  Device per-token values cannot be checked without a sync; the kernels treat a non-finite pitch /
 * energy as "predicted", a negative duration as "predicted" and clamp durations at EV_PROSODY_MAX_DURATION. */
#define EV_PROSODY_MAX_DURATION 1024      /* frames per token (~16 s at 16 kHz / 256) */
typedef struct ev_prosody {
    uint32_t struct_size;            /* sizeof(ev_prosody): lets the struct grow later without a new entry point (a version that appends
                                        fields keeps accepting this size; today any other size is rejected) */
    uint32_t reserved0;              /* 0 */
    const float*   alpha;            /* (B,) HOST, duration scale per utterance (> 0, finite) or NULL = the call's alpha */
    const float*   pitch_scale;      /* (B,) HOST or NULL = 1 */
    const float*   pitch_shift;      /* (B,) HOST or NULL = 0 */
    const float*   energy_scale;     /* (B,) HOST or NULL = 1 */
    const float*   energy_shift;     /* (B,) HOST or NULL = 0 */
    const float*   pitch;            /* (total_tokens,) packed like ling, NaN = predicted; NULL = all predicted */
    const float*   energy;           /* same */
    const int64_t* durations;        /* (total_tokens,) >= 0 forced, -1 predicted; NULL = all predicted */
} ev_prosody;

/* ev_synthesize with prosody controls (semantics above).  prosody == NULL is exactly ev_synthesize.  Rejected (negative return, message
 * naming the field, nothing launched): struct_size != sizeof(ev_prosody), reserved0 != 0, an invalid control value, and prosody combined
 * with EV_FLAG_FORCED_DURATIONS.  Costs one small token-rate launch (prosody_tracks) more than ev_synthesize, and the durations kernel
 * runs its prosody instantiation (durations_prosody). */
int ev_synthesize_prosody(ev_handle* h, int B, const int64_t* ling, const int32_t* cu_seqlens, const int64_t* speaker,
                          const float* style, const float* content, float alpha, const ev_prosody* prosody,
                          uint32_t flags, ev_result* out);

/* Forced alignment (ev_align): the teacher-forced branch's AlignmentModule + monotonic alignment search + per-token averages
 * (reference model_open_source.py:113-119, modules/alignment.py:27-162), batched on the device.  For utterance b with N tokens and
 * T = mel_lens[b] frames, with the reference's B = 1 semantics (zero conv halo at the utterance's own edges):
 *   1. text:  x = embed_projection1 output (the "x_proj" tap of ev_synthesize, same inputs, same bits);  t = t_conv2(relu(t_conv1(x)))
 *   2. mel:   f = f_conv3(relu(f_conv2(relu(f_conv1(mel)))))           (kernels 3 / 3 / 1, and 3 / 1 on the text side)
 *   3. score: log_p[t, n] = log_softmax_n(-||f_t - x_n||_2) + (float)log betabinom.pmf(n; N, t + 1, T - t)     ("log_p_attn")
 *   4. MAS:   Q in fp64: Q[0, j] = sum_{j' <= j} log_p[j', 0] summed SEQUENTIALLY in fp64 -- the one deliberate deviation: the reference
 *             sums that row in float32 (numpy's pairwise order unjitted, numba's when jitted); Q[i, j] = max(Q[i-1, j-1], Q[i, j-1]) + log_p[j, i];
 *             backtrack from A[T-1] = N-1, taking i-1 on a tie (>=);  durations = bincount(A)   (>= 1 each, summing to T)
 *   5. pitch[n] / energy[n] = mean of pitch_frames / energy_frames over token n's frames (fp64 sum, one rounding to fp32)
 *   6. score[b] = mean_t log_p[t, A[t]]  (= -bin_loss of the utterance; fp64 sum)
 * The distance is evaluated in direct form on fp32 (never as |f|^2 + |x|^2 - 2 f.x), the convs are split-precision (fp32-class) GEMMs
 * whatever decoder_precision / vocoder_precision say: the results are the same bits on every precision mode and for an utterance
 * alone or in any batch.
 * Inputs: ling / cu_seqlens / speaker / style / content exactly as ev_synthesize; mel packed as ev_vocoder takes it (per utterance
 * (n_mels, mel_lens[b]) row-major, fp32 or fp16); mel_lens HOST; pitch_frames / energy_frames (total_frames,) packed like mel's frames, in
 * the checkpoint's normalised units, or NULL (then the result's pitch / energy are NULL).  EV_FLAG_DEVICE_INPUTS covers every input pointer
 * except cu_seqlens and mel_lens; EV_FLAG_DEVICE_MEL covers mel, pitch_frames and energy_frames only (the arrays of an ev_features_result: they
 * are complete when ev_features returns and live in its own workspace).
 * Rejected before anything is launched (message naming the utterance or field): struct_size != sizeof(ev_align_result), mel_lens[b] <
 * N_b (no monotonic path gives every token a frame), N_b > EV_ALIGN_MAX_TOKENS or mel_lens[b] > EV_ALIGN_MAX_FRAMES, bad ids (as
 * ev_synthesize), a weight blob without the aligner ("aln.*": packed only from state dicts that carry am.alignment_module.*).
 * Lifetime: the result and its device arrays live in a workspace of their own.  They stay valid across ev_synthesize[_prosody] and
 * ev_vocoder calls on the same handle, until the next ev_align or ev_destroy -- so durations / pitch / energy can be passed straight
 * back as ev_prosody.durations / .pitch / .energy with EV_FLAG_DEVICE_INPUTS (they are complete when ev_align returns: it synchronises).
 * ev_align itself may invalidate an earlier ev_result, like any call.  After ev_align, ev_get_stage serves "log_p_attn" (the (T_b, N_b)
 * fp32 blocks of the utterances, concatenated) and, with keep_stages, "aln_text" (t_conv2 out, token rows) and "aln_feats" (f_conv3
 * out, frame rows); "dur" / "dur_eff" have no data until the next synthesis. */
#define EV_ALIGN_MAX_TOKENS 2048      /* tokens per utterance */
#define EV_ALIGN_MAX_FRAMES 16384     /* mel frames per utterance (~262 s at 16 kHz / 256) */
typedef struct ev_align_result {
    uint32_t struct_size;          /* sizeof(ev_align_result), set by the caller; any other value is rejected (room to grow, as ev_prosody) */
    int32_t  batch;
    int32_t  total_tokens;
    int32_t  reserved0;
    int64_t  total_frames;
    const int64_t* durations;      /* (total_tokens,) DEVICE, packed like ling: frames per token; >= 1 each, sum over utterance b = mel_lens[b] */
    const float*   pitch;          /* (total_tokens,) DEVICE: per-token mean of pitch_frames over the token's frames, or NULL */
    const float*   energy;         /* same for energy_frames, or NULL */
    const float*   score;          /* (batch,) DEVICE: mean over the utterance's frames of log_p_attn along the path (= -bin_loss of that utterance) */
    const int32_t* mel_lens;       /* (batch,) HOST */
    const int64_t* mel_offsets;    /* (batch+1,) HOST */
} ev_align_result;

int ev_align(ev_handle* h, int B, const int64_t* ling, const int32_t* cu_seqlens, const int64_t* speaker,
             const float* style, const float* content, const void* mel, int mel_is_f16, const int32_t* mel_lens,
             const float* pitch_frames, const float* energy_frames, uint32_t flags, ev_align_result* out);

/* Acoustic features (ev_features): wav -> the log-mel spectrogram ev_align / ev_vocoder take and the per-frame energy, on the device.  The reference
 * computes them in its training stack (prompt_dataset.get_mel -> TacotronSTFT.mel_spectrogram, models/prompt_tts_modified/tacotron_stft.py:71-80,
 * stft.py:48-76, with config/joint/config.py's filter length = window length 1024, hop 256, 80 mels, 16 kHz, 0-8000 Hz).  For an utterance of L
 * samples in [-1, 1] (int16 input: x / 32768):
 *   1. reflect-pad n_fft / 2 samples on each side (L >= n_fft / 2 + 1);  2. frames t = 0 .. L / hop, T = L / hop + 1, frame t = padded[hop t, hop t + n_fft);
 *   3. re / im[k, t] = frame . basis, k = 0 .. n_fft / 2, basis = float32(cos / -sin(2 pi k n / n_fft)) * float32(window[n]), a float32 product;
 *   4. mag = sqrt(re^2 + im^2);  5. mel = log(max(mel_basis @ mag, mel_clip));  6. energy[t] = sqrt(max(sum_k mag[k, t]^2, energy_floor)),
 *      returned standardised as (e - energy_mean) / energy_std.
 * Arithmetic: step 3 runs on the matrix cores in the split-precision (fp32-class) arithmetic of EV_PREC_X3 -- samples and basis as fp16 hi + lo parts,
 * three fp16 MFMAs per product, fp32 accumulation -- whatever decoder_precision / vocoder_precision say; step 5's matrix product is fp32, its log and
 * step 6's sum fp64 rounded once.  No atomics and no split of a frame's sums over blocks: an utterance gives the same bits alone, anywhere in a
 * batch, as int16 or as the equal floats, and on every precision mode.  The pitch track is a call of its own: ev_pitch, below. */
#define EV_FEATURES_MAX_NFFT 2048      /* n_fft: a multiple of 128 up to this */
#define EV_FEATURES_MAX_MELS 128       /* n_mels */
#define EV_FEATURES_MAX_RUN  24576     /* 63 hop + n_fft: the samples of a 64-frame tile, which stay in LDS */
typedef struct ev_features_config {
    uint32_t struct_size;          /* sizeof(ev_features_config); any other value is rejected */
    int32_t  n_fft;                /* 1024: filter length = window length; a multiple of 128, at most 2048 */
    int32_t  hop;                  /* 256: a multiple of 8, at most n_fft, 63 hop + n_fft <= 24576 */
    int32_t  n_mels;               /* 80: at most 128 */
    float    mel_clip;             /* 1e-5 */
    float    energy_floor;         /* 1e-10 */
    const float* mel_basis;        /* HOST (n_mels, n_fft / 2 + 1) row-major, required (emotivoice_amd/features.py: mel_filterbank) */
    const float* window;           /* HOST (n_fft,) or NULL = periodic hann */
} ev_features_config;
void ev_default_features_config(ev_features_config* cfg);      /* the reference's values; mel_basis is left NULL */
/* Builds the basis planes and keeps them on the device (copies mel_basis / window; may be called again).  Independent of ev_load_weights. */
int ev_features_setup(ev_handle* h, const ev_features_config* cfg);

typedef struct ev_features_result {
    uint32_t struct_size;          /* sizeof(ev_features_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total_frames;
    const float*   mel;            /* DEVICE, packed per utterance as (n_mels, T_b) row-major: exactly what ev_align / ev_vocoder take */
    const float*   energy;         /* DEVICE (total_frames,): (e - energy_mean) / energy_std */
    const int32_t* mel_lens;       /* (batch,) HOST */
    const int64_t* mel_offsets;    /* (batch+1,) HOST */
} ev_features_result;
/* wav: the B utterances back to back, fp32 or int16 (wav_is_i16), a device pointer with EV_FLAG_DEVICE_INPUTS; wav_lens HOST.  Rejected before
 * anything is launched (message naming the field or utterance): a wrong struct_size, no ev_features_setup, wav_lens[b] < n_fft / 2 + 1,
 * T_b > EV_ALIGN_MAX_FRAMES, a non-finite or non-positive energy_std (or a non-finite energy_mean).  The result lives in a workspace of its own and is
 * complete when the call returns; it stays valid across ev_align / ev_synthesize[_prosody] / ev_vocoder until the next ev_features or ev_destroy.
 * On a handle created with keep_stages, ev_get_stage("feat_mag") returns the (total_frames, n_fft / 2 + 1) magnitudes of the last ev_features. */
int ev_features(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* wav_lens, float energy_mean, float energy_std,
                uint32_t flags, ev_features_result* out);

/* Pitch extraction (ev_pitch): wav -> per-frame F0 on ev_features' frame grid, in the units ev_align takes as pitch_frames.  The reference gets
 * its training pitch from pyworld (feats.Pitch: dio + stonemask at a frame period of 1000 hop / sr ms, a "continuous pitch" fill of the unvoiced
 * frames, then (f0 - pitch_stats[0]) / pitch_stats[1]).  This is not DIO + StoneMask: the estimator here is YIN (a cumulative-mean-normalised
 * difference function), specified below; only the frame grid, the fill (step 6) and the standardisation (step 7) restate the reference.  Agreement
 * with pyworld's track has not been measured.  Lags: tau_min = floor(sample_rate / f_max), tau_max = ceil(sample_rate / f_min), both evaluated in
 * fp64 on the float fields.  For an utterance of L >= 1 samples in [-1, 1] (int16 input: x / 32768), W = win:
 *   1. frames t = 0 .. L / hop, T = L / hop + 1 (ev_features' grid and count, dio's time axis).  Frame t reads the S = W + tau_max + 1 samples
 *      s[0 .. S) that start at t hop - S / 2 (integer division); samples outside [0, L) are zero (no reflection).  a = s[0 .. W).
 *   2. d[tau] = sum_{j < W} (a[j] - s[j + tau])^2, tau = 0 .. tau_max + 1: the direct form in fp32 (never E0 + E_tau - 2 r), summed in an order fixed
 *      by (W, tau) alone -- four interleaved partial sums over j mod 4, j ascending, combined as (s0 + s1) + (s2 + s3).
 *   3. cs[tau] = sum_{k = 1 .. tau} d[k], a running fp64 sum;  d'[0] = 1, d'[tau] = (float)(d[tau] * tau / cs[tau]) where cs[tau] > 0, else 1.
 *   4. the frame is unvoiced if E0 = sum_j a[j]^2 < W silence_rms^2.  Otherwise tau = the first lag in [tau_min, tau_max] with d'[tau] < threshold,
 *      walked on while tau + 1 <= tau_max and d'[tau + 1] < d'[tau]; no such lag: unvoiced.
 *   5. y0, y1, y2 = d'[tau - 1], d'[tau], d'[tau + 1];  off = 0.5 (y0 - y2) / (y0 - 2 y1 + y2) clamped to [-0.5, 0.5], 0 unless the denominator is
 *      > 0 (fp64);  f0 = sample_rate / (tau + off), aperiodicity = y1.  Unvoiced frames: f0 = 0, aperiodicity = 1.
 *   6. continuous track (the reference's Pitch._convert_to_continuous_pitch): no voiced frame: all zero.  Otherwise frames before the first voiced
 *      frame take its value, frames after the last voiced one take its value, and an unvoiced frame t between voiced neighbours a < t < b gets
 *      f0[a] + ((f0[b] - f0[a]) / (b - a)) (t - a), evaluated in fp64 and rounded once.
 *   7. pitch[t] = (cont[t] - pitch_mean) / pitch_std; an all-unvoiced utterance gives (0 - pitch_mean) / pitch_std, as the reference would.
 * No atomics and no split of a frame's sums over blocks: an utterance gives the same bits alone, anywhere in a batch, as int16 or as the equal
 * floats, from host or device memory, and on every precision mode.  Needs neither weights nor ev_features_setup. */
#define EV_PITCH_TILE_FRAMES 8         /* frames per block of the kernel */
#define EV_PITCH_MAX_WIN 2048          /* win */
#define EV_PITCH_MAX_LDS 65536         /* bytes of a tile: 4 (7 hop + win + tau_max + 1) + 96 (tau_max + 2 rounded up to even) + 32 */
typedef struct ev_pitch_config {
    uint32_t struct_size;          /* sizeof(ev_pitch_config); any other value is rejected */
    int32_t  sample_rate;          /* 16000 */
    int32_t  hop;                  /* 256: 1 .. win */
    int32_t  win;                  /* 1024: the integration window W; tau_max + 1 <= win <= EV_PITCH_MAX_WIN and the tile within EV_PITCH_MAX_LDS */
    float    f_min;                /* 80 */
    float    f_max;                /* 400: 0 < f_min < f_max <= sample_rate / 4 */
    float    threshold;            /* 0.15: in (0, 1] */
    float    silence_rms;          /* 1e-3: >= 0 */
} ev_pitch_config;
void ev_default_pitch_config(ev_pitch_config* cfg);

typedef struct ev_pitch_result {
    uint32_t struct_size;          /* sizeof(ev_pitch_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total_frames;
    const float*   pitch;          /* DEVICE (total_frames,): step 7, what ev_align takes as pitch_frames */
    const float*   f0_hz;          /* DEVICE (total_frames,): step 5, 0 = unvoiced */
    const float*   aperiodicity;   /* DEVICE (total_frames,) */
    const int32_t* mel_lens;       /* (batch,) HOST */
    const int64_t* mel_offsets;    /* (batch+1,) HOST */
} ev_pitch_result;
/* wav / wav_is_i16 / wav_lens / EV_FLAG_DEVICE_INPUTS as ev_features; cfg NULL = ev_default_pitch_config.  Rejected before anything is launched
 * (message naming the field or utterance): a wrong struct_size (config or result), wav_lens[b] < 1, T_b > EV_ALIGN_MAX_FRAMES, hop < 1 or hop > win,
 * win above EV_PITCH_MAX_WIN or a tile above EV_PITCH_MAX_LDS, f_min / f_max not finite or not 0 < f_min < f_max <= sample_rate / 4, tau_max + 1 > win,
 * threshold outside (0, 1], a negative or non-finite silence_rms, a non-finite pitch_mean, a non-finite or non-positive pitch_std.  The result lives
 * in a workspace of its own and is complete when the call returns; it stays valid across ev_features / ev_align / ev_synthesize[_prosody] /
 * ev_vocoder until the next ev_pitch or ev_destroy, so `pitch` goes into ev_align beside an ev_features_result under EV_FLAG_DEVICE_MEL. */
int ev_pitch(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* wav_lens, const ev_pitch_config* cfg,
             float pitch_mean, float pitch_std, uint32_t flags, ev_pitch_result* out);

/* Sample-rate conversion and trimming (ev_resample): a recording at sr_in -> the waveform at sr_out (the model's 16 kHz), optionally trimmed and
 * padded, on the device -- the step the reference runs before it computes a mel: librosa.resample(y, orig_sr, 16000) when it prepares a corpus,
 * then prompt_dataset.get_mel's trim (cut what lies below 0.5 % of the peak, pad 50 ms of zeros on each side).  The resampler is NOT librosa's
 * (soxr): it is the polyphase windowed-sinc filter specified here, and agreement with soxr has not been measured.  The trim restates the reference.
 * Deliberate difference: the reference writes a PCM-16 file between the two steps; here nothing is re-quantised between them.
 *   Rates and lengths: g = gcd(sr_in, sr_out), up = sr_out / g, down = sr_in / g, q = max(up, down).  An utterance of L >= 1 samples gives
 *     n = ceil(L up / down) outputs (int64 arithmetic).
 *   Prototype filter (designed in fp64, rounded once to fp32): half = zeros q, i = -half .. half,
 *     g[i] = sinc(rolloff i / q) I0(beta sqrt(1 - (i / half)^2)) / I0(beta),  h[i] = (float)(up g[i] / sum g),  sinc(x) = sin(pi x) / (pi x);
 *     the default design has zeros = 16, rolloff = 0.945, beta = 9.0.  A caller's own taps h[-half_len .. half_len] replace it.
 *   Output sample: y[m] = sum_k x[k] h[m down - k up], k from k_lo = ceil((m down - half) / up) to k_hi = floor((m down + half) / up), ascending,
 *     x[k] = +0.0 outside [0, L) (zero padding, no reflection); m down in int64.  fp32 fmaf into four interleaved partial sums over (k - k_lo) mod 4,
 *     combined as (s0 + s1) + (s2 + s3) -- the order rule of ev_pitch step 2, so the bits of y[m] depend on (utterance, m) alone.
 *     int16 input is x / 32768.  sr_in == sr_out is a copy (int16 -> float) with no filter.
 *   Trim (only with trim_frac > 0, on the fp32 y): peak = max |y|, thr = (float)peak * (float)trim_frac (one fp32 product); start = the first index
 *     with |y| > thr, end = the LAST such index; the output is trim_pad zeros, y[start .. end), trim_pad zeros -- the slice excludes `end`, so the
 *     last sample above the threshold is dropped, as the reference does.  No sample above the threshold (an all-zero utterance): start = end = 0 and
 *     the output is 2 trim_pad zeros (the reference raises there; the caller sees it in trim_start / trim_end).  The reference's values are
 *     trim_frac = 0.005 and trim_pad = sr_out / 20.
 * No atomics and no floating sum split over threads: an utterance gives the same bits alone or anywhere in a batch, as int16 or as the equal floats,
 * from host or device memory, and on every precision mode; the max and first / last index reductions are exact in any order.  Needs no weights. */
#define EV_RESAMPLE_MAX_RATIO 1024    /* up and down after the gcd */
#define EV_RESAMPLE_MAX_TAPS  32769   /* 2 half + 1 */
#define EV_RESAMPLE_TILE      256     /* outputs per block of the kernel */
typedef struct ev_resample_config {
    uint32_t struct_size;          /* sizeof(ev_resample_config); any other value is rejected */
    int32_t  sr_in, sr_out;        /* >= 1; up and down <= EV_RESAMPLE_MAX_RATIO */
    int32_t  half_len;             /* with taps: (len - 1) / 2 >= 1; ignored without */
    const float* taps;             /* HOST (2 half_len + 1) or NULL = the default design; copied */
    float    trim_frac;            /* 0 = no trim; in [0, 1) */
    int32_t  trim_pad;             /* zeros on each side after the trim; >= 0 */
} ev_resample_config;
void ev_default_resample_config(ev_resample_config* cfg);      /* 16000 -> 16000, taps NULL, trim off */
/* Host only, no device touched: writes the design's 2 half + 1 taps (half = zeros max(up, down)) and returns half, or, with cap < 2 half + 1 (taps may
 * then be NULL), the negative needed capacity -(2 half + 1).  0 for arguments outside the design's domain: a rate < 1, up or down above
 * EV_RESAMPLE_MAX_RATIO, zeros outside [1, 4096], rolloff not in (0, 1], beta negative or non-finite. */
int ev_resample_design(int sr_in, int sr_out, int zeros, double rolloff, double beta, float* taps, int cap);
/* Copies the taps (or designs the default ones) and builds the device table.  Rejected (message naming the field): a wrong struct_size, sr_in or
 * sr_out < 1, up or down > EV_RESAMPLE_MAX_RATIO, taps with half_len < 1, more than EV_RESAMPLE_MAX_TAPS taps, a non-finite tap, trim_frac outside
 * [0, 1) or non-finite, trim_pad < 0.  A rejected setup leaves the previous one in place. */
int ev_resample_setup(ev_handle* h, const ev_resample_config* cfg);

typedef struct ev_resample_result {
    uint32_t struct_size;          /* sizeof(ev_resample_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total_samples;
    const float*   wav;            /* DEVICE, utterances back to back: what ev_features / ev_pitch take with EV_FLAG_DEVICE_INPUTS */
    const int64_t* wav_lens;       /* (batch,)   HOST */
    const int64_t* wav_offsets;    /* (batch+1,) HOST */
    const int64_t* trim_start;     /* (batch,) HOST, indices into the untrimmed resampled utterance; 0 / n_b without trim */
    const int64_t* trim_end;       /* (batch,) HOST */
} ev_resample_result;
/* wav / wav_is_i16 / wav_lens / EV_FLAG_DEVICE_INPUTS as ev_features.  Rejected before anything is launched (message naming the field or utterance):
 * a wrong struct_size, no ev_resample_setup, B outside [1, 65535], wav_lens[b] < 1, an utterance whose output (with its padding) exceeds
 * EV_ALIGN_MAX_FRAMES * 256 samples.  The result lives in a workspace of its own and is complete when the call returns; it stays valid across
 * ev_features / ev_pitch / ev_align / ev_synthesize[_prosody] / ev_vocoder until the next ev_resample or ev_destroy -- the contract of
 * ev_features_result.  ev_get_stage("resample_taps") returns the phase-major table in use: (up, R) floats, R = (2 half / up + 1) | 1, row
 * p = (m down) mod up holding h[i], i = p (mod up), from the largest i <= half downwards, zero-filled; with keep_stages, "resample_raw" returns the
 * untrimmed y of the last call, packed at ceil(L_b up / down) each. */
int ev_resample(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* wav_lens, uint32_t flags, ev_resample_result* out);

/* Long-form stitching (ev_stitch): the waveforms of one synthesis batch -> finished documents on the device: every segment (sentence) cut at its
 * edge silence, laid out with a pause or a cross-fade to its neighbour, ramped at its free ends, and written as fp32 and, when asked, as int16.
 * The reference has no such stage ("Support longer text" is the open item of its roadmap); the arithmetic is the one specified here.
 *   Inputs: S segments wav + seg_offsets[s] of seg_lens[s] >= 1 fp32 samples; seg_doc[s] non-decreasing from 0 in steps of at most 1 (the segments
 *     of one document are consecutive); pause_after[s] in samples, ignored for the last segment of a document.
 *   Cut: peak_s = max |x|, thr_s = max((float)peak_s * trim_frac as one fp32 product, trim_abs); first / last = the first and the LAST index with
 *     |x| > thr_s; a_s = max(0, first - keep), b_s = min(L_s, last + 1 + keep), n_s = b_s - a_s.  The last sample above the threshold is KEPT: this
 *     differs from ev_resample's trim, which restates the reference's slice y[start .. end) and drops it.  No sample above the threshold:
 *     a_s = b_s = 0, an empty segment.  trim_frac == 0 && trim_abs == 0: no scan is launched, a_s = 0, b_s = L_s and seg_peak is 0.
 *   Plan (host, int64; ev_stitch_plan).  For consecutive segments s, s + 1 of one document: ov_s = 0 if pause_after[s] >= 0 or either segment is
 *     empty, else ov_s = min(-pause_after[s], F, n_s / 2, n_{s+1} / 2) (integer division); gap_s = max(pause_after[s], 0) when ov_s = 0, else 0.
 *     pos_first = lead, pos_{s+1} = pos_s + n_s + gap_s - ov_s, doc_len = pos_last + n_last + tail.  Fade lengths per side: at a joint with
 *     ov_s > 0, FR_s = FL_{s+1} = ov_s; elsewhere (the document's ends included) FL_s = FR_s = min(F, n_s / 2).  At most two segments cover any
 *     output sample: pos_{s+2} = pos_s + n_s + (gap_s + gap_{s+1}) + (n_{s+1} - ov_s - ov_{s+1}) >= pos_s + n_s, since ov_s and ov_{s+1} are each
 *     at most n_{s+1} / 2 rounded down.
 *   Ramp table (ev_stitch_ramp): tab[i] = (float)(0.5 - 0.5 cos(pi (i + 0.5) / F)), i < F, in fp64, rounded once.  r(i, L) = tab[((2 i + 1) F) / (2 L)]
 *     for i < L (int64 index), 1.0f for i >= L or L = 0.  With L = F the index is i, and tab[i] + tab[F - 1 - i] = 1 in exact arithmetic.
 *   Output sample p of a document: every covering segment contributes c = x[a_s + i] * (r(i, FL_s) * r(n_s - 1 - i, FR_s)), i = p - pos_s, two
 *     rounded fp32 products; out = c where one segment covers p, c_earlier + c_later (one rounded fp32 sum, no fma) where two do, +0.0 where none
 *     does.  Where both ramps are 1 the source bits pass through.
 *   int16 (want_i16): (int)(out * 32768.0f) truncated toward zero, then clamped to [-32768, 32767] -- a deliberate difference from
 *     EV_FLAG_WANT_INT16's wrapping cast, because a cross-fade can exceed 1.
 * No atomics and no floating sum split over threads: a document's bits are the same alone or anywhere in a batch and from host or device memory;
 * the max and first / last index reductions are exact in any order.  Needs no weights. */
#define EV_STITCH_MAX_FADE  4096            /* samples */
#define EV_STITCH_MAX_PAUSE (1 << 24)       /* samples */
#define EV_STITCH_MAX_DOC   (1 << 30)       /* samples per document */
typedef struct ev_stitch_config {
    uint32_t struct_size;          /* sizeof(ev_stitch_config); any other value is rejected */
    float    trim_frac;            /* in [0, 1) */
    float    trim_abs;             /* >= 0, finite; both zero = no cut */
    int32_t  keep;                 /* samples kept on each side of the cut; >= 0 */
    int32_t  fade;                 /* F, in [0, EV_STITCH_MAX_FADE] */
    int32_t  lead, tail;           /* zeros before the first / after the last segment of every document; >= 0 */
    int32_t  want_i16;             /* != 0: also the int16 documents */
} ev_stitch_config;
void ev_default_stitch_config(ev_stitch_config* cfg);      /* no trim, keep 0, fade 0, lead = tail = 0, fp32 only: plain concatenation */
/* Host only, no device touched.  ev_stitch_ramp writes tab[0 .. F) and returns F, or -1 for F outside [0, EV_STITCH_MAX_FADE].  ev_stitch_plan
 * takes the cut lengths n[s] >= 0 and writes pos, fl, fr (S each) and doc_lens (one per document); it returns the number of documents, or -1 with
 * a message naming the field or segment (ev_last_error(NULL)) for what ev_stitch rejects in cfg, seg_doc, pause_after, S, a negative n[s] or a
 * document longer than EV_STITCH_MAX_DOC.  ev_stitch plans with this function. */
int ev_stitch_ramp(int F, float* tab);
int ev_stitch_plan(int S, const int64_t* n, const int32_t* seg_doc, const int32_t* pause_after, const ev_stitch_config* cfg, int64_t* pos, int32_t* fl,
                   int32_t* fr, int64_t* doc_lens);

typedef struct ev_stitch_result {
    uint32_t struct_size;          /* sizeof(ev_stitch_result), set by the caller; any other value is rejected */
    int32_t  batch_docs;
    int32_t  batch_segs;
    int32_t  reserved;
    int64_t  total_samples;
    const float*   wav;            /* DEVICE, the documents back to back */
    const int16_t* wav_i16;        /* DEVICE, the same layout, or NULL without want_i16 */
    const int64_t* doc_lens;       /* (batch_docs,)     HOST */
    const int64_t* doc_offsets;    /* (batch_docs + 1,) HOST */
    const int64_t* seg_pos;        /* (batch_segs,) HOST: the cut segment's first sample inside its document */
    const int64_t* seg_start;      /* (batch_segs,) HOST: a_s, an index into the segment */
    const int64_t* seg_end;        /* (batch_segs,) HOST: b_s */
    const float*   seg_peak;       /* (batch_segs,) HOST: max |x| of the whole segment; 0 when no scan was launched */
} ev_stitch_result;
/* wav: a device pointer with EV_FLAG_DEVICE_INPUTS (the other flags are ignored); seg_offsets, seg_lens, seg_doc and pause_after are always HOST
 * arrays, so an ev_result.wav with seg_offsets = mel_offsets * 256 goes straight in.  cfg NULL = ev_default_stitch_config.  Rejected before anything
 * is launched (message naming the field or segment; the previous result stays valid): a wrong struct_size of cfg or out, S outside [1, 65535],
 * seg_offsets[s] < 0, seg_lens[s] < 1, a seg_doc that does not start at 0, decreases or skips, fade outside [0, EV_STITCH_MAX_FADE], a negative
 * keep / lead / tail, pause_after[s] outside [-EV_STITCH_MAX_FADE, EV_STITCH_MAX_PAUSE], a non-finite or negative trim_frac / trim_abs, trim_frac
 * >= 1, and a document longer than EV_STITCH_MAX_DOC samples -- judged before the cut, as lead + tail + its segments + its positive pauses.  The
 * cuts come back to the host between the scan and the mix (one synchronisation, as ev_resample's trim).  The result lives in a workspace of its
 * own and is complete when the call returns; it stays valid across ev_synthesize[_prosody] / ev_vocoder / ev_align / ev_features / ev_pitch /
 * ev_resample until the next ev_stitch or ev_destroy -- the contract of ev_features_result.  ev_get_stage("stitch_ramp") returns the F floats of
 * the ramp table of the last ev_stitch. */
int ev_stitch(ev_handle* h, int S, const float* wav, const int64_t* seg_offsets, const int64_t* seg_lens, const int32_t* seg_doc,
              const int32_t* pause_after, const ev_stitch_config* cfg, uint32_t flags, ev_stitch_result* out);

/* Signal comparison (ev_compare): how far a signal a (under test) lies from a signal b (the yardstick), per segment, on the device -- the
 * measurement behind "waveform within 1e-3 of the reference" (the tests' rel_l2 / rel_l2_ac), without a device -> host copy of either signal.
 * Nothing is waveform-specific: a mel is compared with lens = mel_lens * n_mels.  The reference has no such stage; the arithmetic is the one
 * specified here, in fp64 with a fixed order, so that a float64 restatement reproduces every output bit.
 *   Inputs: a and b, B segments each, packed back to back with the same lens[b] >= 1 fp32 elements; segment b starts at element
 *     off_b = lens[0] + .. + lens[b - 1] of both.  n_b = lens[b].
 *   Per element i of a segment: x = (double)a[i], y = (double)b[i].  Where a[i] or b[i] is not finite (NaN, +-inf) the element counts once in
 *     nonfinite[b] and enters everything else as d = 0, y = 0.  Otherwise d = x - y (one fp64 rounding).  The element's terms are d, d * d, y and
 *     y * y, each product one fp64 rounding; no product is fused with a sum.
 *   Sums (sum_d, sum_d2, sum_y, sum_y2; each on its own, the same rule): the segment is cut into chunks of EV_COMPARE_CHUNK elements, chunk c =
 *     elements [c * EV_COMPARE_CHUNK, min((c + 1) * EV_COMPARE_CHUNK, n_b)).  Inside a chunk, t = 0 .. 255: s[t] = +0.0, then the terms of the
 *     chunk's elements t, t + 256, t + 512, ... (those that exist) are added to s[t] in ascending order.  Then the halving tree: for o = 128, 64,
 *     .., 1: s[t] = s[t] + s[t + o] for every t < o.  s[0] is the chunk's sum (chunk_d2 / chunk_y2 hold it for d * d and y * y).  The segment's
 *     sum starts at +0.0 and adds its chunks' sums in ascending chunk order.  Every addition is one fp64 rounding.
 *   Maxima: max_abs_d[b] = (float)max_i |d| (the fp64 maximum, rounded once to fp32, so +inf where it exceeds FLT_MAX); argmax_d[b] = the
 *     smallest i with |d| equal to that maximum (0 where every d is 0); peak_y[b] = max_i |b[i]| over the elements that count (exact in fp32).
 *   Ratios (host, C double, from the sums; sqrt, max, *, / and - one correctly rounded operation each, in the order written):
 *     rel_l2[b]    = sqrt(sum_d2) / sqrt(max(sum_y2, EV_COMPARE_FLOOR))
 *     rel_l2_ac[b] = sqrt(sum_d2) / sqrt(max(sum_y2 - (sum_y * sum_y) / (double)n_b, EV_COMPARE_FLOOR))
 *     rel_l2_ac removes the yardstick's mean in one pass: sum (y - mean)^2 = sum_y2 - sum_y^2 / n.  The subtraction cancels where the mean
 *     dominates: with |mean| = k * rms_ac the relative error of the denominator's square is about (1 + k^2) * 2^-52 times a small factor, so the
 *     ratio is good to 1e-9 for k up to a few hundred (the synthetic-weight fixtures have k = 3).  n_b includes the elements counted in nonfinite.
 * No atomics; the order of every sum is fixed by (segment, index) alone and the maxima are exact in any order, so a segment gives the same bits
 * alone or anywhere in a batch, and from host or device memory.  Needs no weights. */
#define EV_COMPARE_CHUNK 4096
#define EV_COMPARE_FLOOR 1e-60      /* the square of the 1e-30 the tests' rel_l2 clamps a norm with */
typedef struct ev_compare_result {
    uint32_t struct_size;          /* sizeof(ev_compare_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total;                /* elements per signal */
    const double*  sum_d;          /* every array: HOST, (batch,) unless stated */
    const double*  sum_d2;
    const double*  sum_y;
    const double*  sum_y2;
    const double*  rel_l2;
    const double*  rel_l2_ac;
    const float*   max_abs_d;
    const int64_t* argmax_d;       /* index inside the segment */
    const float*   peak_y;
    const int64_t* nonfinite;
    const double*  chunk_d2;       /* (chunk_offsets[batch],): the chunks' sums of d * d, segment after segment: where in a segment the error sits */
    const double*  chunk_y2;       /* (chunk_offsets[batch],): the same for y * y */
    const int64_t* chunk_offsets;  /* (batch + 1,): segment b owns chunks chunk_offsets[b] .. chunk_offsets[b + 1], ceil(n_b / EV_COMPARE_CHUNK) of them */
} ev_compare_result;
/* a, b: host pointers, or with EV_FLAG_DEVICE_INPUTS (the other flags are ignored) device pointers on the handle's device -- both of one kind.
 * Device signals may belong to other handles: the ev_result.wav of a strict engine and of an mx engine go straight in (a result is complete when
 * its call returns, so no ordering between the handles' streams is needed).  lens is always a HOST array.  Rejected before anything is
 * launched (message naming the field or segment; the previous result stays valid): a NULL h, a, b, lens or out, a wrong struct_size, B outside
 * [1, 65535], lens[b] < 1.  The call synchronises (as ev_resample's trim): every array of the result is HOST memory in a workspace of its own,
 * complete when the call returns, and stays valid across every other entry point until the next ev_compare or ev_destroy. */
int ev_compare(ev_handle* h, int B, const float* a, const float* b, const int64_t* lens, uint32_t flags, ev_compare_result* out);

/* FLAC encoding (ev_flac): packed 16-bit PCM, or the fp32 that converts to it, -> one FLAC stream per segment, on the device: what a `flac`
 * response carries.  The reference has no such stage (its compressed formats go through pydub / ffmpeg); FLAC is lossless, so a decoder returns
 * every input sample.  Everything below is integer arithmetic with fixed tie rules: a restatement reproduces every output byte.
 *   Input: B segments packed back to back, lens[b] >= 1 samples each, int16 (pcm_is_i16 != 0) or fp32.  An fp32 sample x converts as
 *     t = x * 32768.0f (one fp32 product); NaN -> 0; otherwise t truncated toward zero and saturated to int32.  convert = EV_FLAC_WRAP keeps
 *     the low 16 bits (two's complement): the bits of EV_FLAG_WANT_INT16, so a flac response decodes to what a pcm response carries.
 *     convert = EV_FLAC_CLAMP clamps to [-32768, 32767]: ev_stitch's int16 rule.  convert is ignored for int16 input.
 *   Stream of a segment of n samples: "fLaC"; the metadata block header 0x80 0x00 0x00 0x22 (last block, STREAMINFO, 34 bytes); STREAMINFO;
 *     the frames; nothing else.  STREAMINFO, big-endian bit fields in order: min block size = max block size = N (16 bits each); min and
 *     max frame size in bytes over this stream's frames (24 bits each); sample rate (20); channels - 1 = 0 (3); bits per sample - 1 = 15 (5);
 *     n (36); MD5 = 16 zero bytes ("not known", which the format allows; ev_flac_lpc below can write it).
 *   Blocks: N = block_size; ceil(n / N) frames; every frame holds N samples but the last, which holds the rest (1 .. N).
 *   Frame header: 0xFF 0xF8 (sync, fixed block size); a byte of block-size code << 4 | sample-rate code; a byte 0x08 (channel code 0, sample-size
 *     code 4 = 16 bits, a reserved 0 bit); the frame's index in its stream in the format's UTF-8-like coding (1 byte below 2^7, then 2 .. 6 bytes
 *     carrying 11, 16, 21, 26, 31 bits); then, for a last frame shorter than N, its size - 1 in 8 bits (size <= 256, block-size code 6) or 16
 *     bits (code 7); CRC-8 (polynomial 0x07, initial value 0, not reflected, no final xor) of the header bytes before it.  A frame of N samples
 *     carries the table code 8 + log2(N / 256).  Sample-rate codes: 8000: 4, 16000: 5, 22050: 6, 24000: 7, 32000: 8, 44100: 9, 48000: 10.
 *   Subframe: a byte type << 1 (a 0 bit, the 6-bit type, a 0 bit: no wasted bits); types CONSTANT 0, VERBATIM 1, FIXED order o = 8 + o (LPC: ev_flac_lpc below).
 *   Choice, for a block of m samples:
 *     1. All samples equal: CONSTANT, the sample in 16 bits (8 + 16 bits).
 *     2. Otherwise for every order o = 0 .. min(max_fixed_order, m - 1): the residual r_i, i = o .. m - 1, is the o-th finite difference
 *        (x_i; x_i - x_{i-1}; x_i - 2 x_{i-1} + x_{i-2}; x_i - 3 x_{i-1} + 3 x_{i-2} - x_{i-3}; x_i - 4 x_{i-1} + 6 x_{i-2} - 4 x_{i-3} + x_{i-4});
 *        u_i = r_i >= 0 ? 2 r_i : -2 r_i - 1.  A partition order p is valid when p <= max_partition_order, m % 2^p == 0 and (m >> p) > o
 *        (p = 0 always is); partition j = 0 .. 2^p - 1 holds the residuals of samples [j (m >> p), (j + 1)(m >> p)), without the o warm-up
 *        samples in partition 0.  A partition of c residuals costs, with Rice parameter k = 0 .. 14, (k + 1) c + sum (u >> k) bits; it takes the
 *        smallest cost, the smaller k on a tie.  Order p costs 4 + sum_j (4 + cost_j); the smallest wins, the smaller p on a tie.
 *        bits_o = 8 + 16 o + 2 + that cost; the smallest wins, the smaller o on a tie.
 *     3. If that minimum is >= 8 + 16 m: VERBATIM, the samples in 16 bits each.
 *   FIXED subframe: the o warm-up samples in 16 bits each; 2 bits 00 (coding method 0: 4-bit parameters); p in 4 bits; per partition k in 4 bits
 *     (the escape code 15 is never written), then per residual u >> k zero bits, a one bit, and the low k bits of u, most significant first.
 *   Frame end: zero bits to the next byte boundary, then CRC-16 (polynomial 0x8005, initial value 0, not reflected, no final xor) of every byte
 *     of the frame before it, high byte first.
 * No atomics across blocks and nothing depends on the order of execution: a segment's bytes are the same alone or anywhere in a batch, from host or
 * device memory, from int16 or from the fp32 that converts to it.  Needs no weights. */
#define EV_FLAC_WRAP  0
#define EV_FLAC_CLAMP 1
#define EV_FLAC_MAX_SAMPLES (1 << 30)       /* per segment */
typedef struct ev_flac_config {
    uint32_t struct_size;          /* sizeof(ev_flac_config); any other value is rejected */
    int32_t  sample_rate;          /* one of 8000, 16000, 22050, 24000, 32000, 44100, 48000 */
    int32_t  block_size;           /* N: 256, 512, 1024, 2048 or 4096 */
    int32_t  max_fixed_order;      /* in [0, 4] */
    int32_t  max_partition_order;  /* in [0, 6] */
    int32_t  convert;              /* EV_FLAC_WRAP or EV_FLAC_CLAMP; fp32 input only */
} ev_flac_config;
void ev_default_flac_config(ev_flac_config* cfg);      /* 16000, 4096, 4, 5, EV_FLAC_WRAP */
/* Host only: an upper bound of the stream of a segment of n samples: 42 + (2 N + 15) per full frame + 2 r + 15 for a last frame of r < N samples
 * (12 header bytes at most, one subframe byte, 16 bits a sample, two CRC bytes; VERBATIM is the largest subframe the choice can take).  -1 for n
 * outside [1, EV_FLAC_MAX_SAMPLES] or a block_size outside the set. */
int64_t ev_flac_bound(int64_t n, int block_size);

typedef struct ev_flac_result {
    uint32_t struct_size;          /* sizeof(ev_flac_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total_bytes;
    int64_t  total_frames;
    const uint8_t* bytes;          /* DEVICE, (total_bytes,): the streams back to back */
    const int64_t* stream_offsets; /* (batch + 1,) HOST: stream b is bytes[stream_offsets[b] .. stream_offsets[b + 1]) */
    const int64_t* stream_frames;  /* (batch,) HOST */
    const int64_t* frame_offsets;  /* (total_frames + 1,) HOST: byte offsets of the frames in bytes, stream after stream; the last entry is total_bytes */
    const uint8_t* frame_kind;     /* (total_frames,) HOST: 0 constant, 1 verbatim, 8 + o fixed, 32 + (o - 1) LPC (ev_flac_lpc only) */
    const uint8_t* frame_porder;   /* (total_frames,) HOST: the partition order of a fixed subframe, else 0 */
} ev_flac_result;
/* pcm: a host pointer, or with EV_FLAG_DEVICE_INPUTS (the other flags are ignored) a device pointer on the handle's device; lens is always a HOST
 * array, so an ev_result.wav with lens = mel_lens * 256, an ev_result.wav_i16 or an ev_stitch_result.wav_i16 goes straight in.  cfg NULL =
 * ev_default_flac_config.  Rejected before anything is launched (message naming the field or segment; the previous result stays valid): a NULL
 * h, pcm, lens or out, a wrong struct_size of cfg or out, B outside [1, 65535], lens[b] < 1 or > EV_FLAC_MAX_SAMPLES, a sample_rate outside the
 * table, a block_size outside the set, max_fixed_order outside [0, 4], max_partition_order outside [0, 6], convert outside {0, 1}.  The frame
 * sizes come back to the host between the encode and the gather (one synchronisation, as ev_stitch's cut).  The result lives in a workspace of
 * its own and is complete when the call returns; it stays valid across every other entry point until the next ev_flac or ev_destroy -- the
 * contract of ev_features_result. */
int ev_flac(ev_handle* h, int B, const void* pcm, int pcm_is_i16, const int64_t* lens, const ev_flac_config* cfg, uint32_t flags, ev_flac_result* out);

/* FLAC with LPC subframes and the MD5 signature (ev_flac_lpc): ev_flac with the extension ext.  ext NULL, or max_lpc_order = 0 and md5 = 0, gives
 * the bytes of ev_flac.  Everything above holds; the Choice continues, for a block of m samples x_i that is not CONSTANT, with max_lpc_order > 0:
 *     4. Window (Welch, integers, from m alone): w_i = (32767 * 4 * i * (m - 1 - i)) / (m - 1)^2, integer division, i = 0 .. m - 1 (m >= 2);
 *        y_i = (x_i * w_i) >> 15, an arithmetic shift, so |y_i| < 2^15.
 *     5. Autocorrelation: R[l] = sum_{i = l}^{m - 1} y_i y_{i - l}, l = 0 .. L, L = min(max_lpc_order, m - 1): exact in int64 (< 2^42), so any
 *        order of summation gives the same value.  R[0] = 0: no LPC candidate.
 *     6. Levinson-Durbin in fp64, one IEEE operation (round to nearest even) per rounding, no contraction: err = (double)R[0]; for it = 0 ..
 *        L - 1: acc = (double)R[it + 1]; for j = 0 .. it - 1 in that order acc = acc - a_j * (double)R[it - j]; k = acc / err;
 *        a'_j = a_j - k * a_{it - 1 - j} for j < it, a'_it = k; a = a'; err = err * (1 - k * k).  The recursion stops when err is not finite or
 *        err <= 0; otherwise a are the coefficients of order o = it + 1.
 *     7. Quantisation, per order, q = qlp_precision: c_max = max |a_j|; an order with c_max = 0 (or not finite) is skipped.  c_max = f 2^e with f
 *        in [0.5, 1); shift = q - 1 - e; shift < 0: that order is no candidate; shift > 15 is taken as 15.
 *        c_j = clamp(rint(a_j * 2^shift), -2^(q - 1), 2^(q - 1) - 1), rint to nearest even (the product by a power of two is one IEEE product).
 *     8. Residual of order o: r_i = x_i - ((sum_{j = 0}^{o - 1} c_j x_{i - 1 - j}) >> shift), the sum in 64 bits, an arithmetic shift, i = o ..
 *        m - 1.  An order with some |r_i| >= 2^31 is no candidate.
 *     9. Cost: the partition / Rice search of rule 2 with o warm-up samples; bits_o = 8 + 16 o + 4 + 5 + q o + 2 + that cost.  The candidates
 *        are FIXED 0 .. min(max_fixed_order, m - 1), then LPC 1 .. L; the smallest wins; on a tie FIXED wins over LPC and the smaller order wins.
 *        Rule 3 (VERBATIM) applies to that minimum unchanged, so ev_flac_bound still holds.
 *   LPC subframe, type 32 + (o - 1): the o warm-up samples in 16 bits each; q - 1 in 4 bits; shift in 5 bits; c_0 .. c_{o - 1} in q bits each, two's
 *     complement (c_0 multiplies x_{i - 1}); then the residual exactly as in a FIXED subframe.  frame_kind reports 32 + (o - 1).
 *   MD5: with md5 = 1 the last 16 bytes of STREAMINFO are the MD5 (RFC 1321) of the segment's samples as little-endian 16-bit values (for fp32
 *     input: of the converted samples), one wave per segment, before the synchronisation that brings the frame sizes back; with md5 = 0 they are
 *     zero.
 * The streams have been held to a numpy restatement of these rules and to an independent decoder written from the format (tests/), not to
 * libFLAC or ffmpeg. */
typedef struct ev_flac_ext {
    uint32_t struct_size;     /* sizeof(ev_flac_ext); any other value is rejected */
    int32_t  max_lpc_order;   /* 0 (no LPC) .. 12 */
    int32_t  qlp_precision;   /* 5 .. 15; default 12 */
    int32_t  md5;             /* 0 / 1 */
    int32_t  reserved[4];     /* 0 */
} ev_flac_ext;
void ev_default_flac_ext(ev_flac_ext* ext);      /* 8, 12, 1 */
/* As ev_flac (arguments, rejections, the one synchronisation, the result's lifetime: the result shares ev_flac's workspace, so it stays valid until
 * the next ev_flac or ev_flac_lpc); additionally rejected, with a message naming the field: a wrong ext->struct_size, max_lpc_order outside
 * [0, 12], qlp_precision outside [5, 15], md5 outside {0, 1}, a non-zero reserved word. */
int ev_flac_lpc(ev_handle* h, int B, const void* pcm, int pcm_is_i16, const int64_t* lens, const ev_flac_config* cfg, const ev_flac_ext* ext, uint32_t flags,
                ev_flac_result* out);

/* Loudness normalisation (ev_loudness): packed segments -> their programme loudness after ITU-R BS.1770 / EBU R 128 (K-weighted, gated, in LUFS),
 * their sample peak, one gain per segment that brings it to a target within two limits, and the scaled waveform, on the device: it sits between
 * the vocoder (or ev_stitch) and ev_flac.  The reference has no such stage; the arithmetic is the one specified here.
 *   Filter design (ev_loudness_design, fp64): two biquads from the analogue prototypes that reproduce the standard's 48 kHz table.  With
 *     K = tan(pi f0 / fs) and a0 = 1 + K / Q + K^2:
 *     shelf: f0 = 1681.974450955533, G = 3.999843853973347 dB, Q = 0.7071752369554196, Vh = 10^(G / 20), Vb = Vh^0.4996667741545416;
 *       b = [Vh + Vb K / Q + K^2, 2 (K^2 - Vh), Vh - Vb K / Q + K^2] / a0, a = [1, 2 (K^2 - 1) / a0, (1 - K / Q + K^2) / a0];
 *     high-pass: f0 = 38.13547087602444, Q = 0.5003270373238773; b = [1, -2, 1] (not normalised, as in the standard), a as above with this K, Q.
 *     coef = shelf b0 b1 b2 a1 a2, then high-pass b0 b1 b2 a1 a2.  At 48000 Hz these are the standard's printed coefficients.
 *   Measurement, all of it fp64.  An int16 sample is s / 32768, an fp32 sample is widened.  A non-finite sample (NaN, +-inf) counts once in
 *     nonfinite[b] and enters the measurement as 0.  Each segment is filtered from a zero state, shelf then high-pass, giving y.
 *     step = fs / 10, block = 4 step.  n >= block: nblk = (n - block) / step + 1 blocks, block j covers [j step, j step + block), z_j = the mean
 *     of y^2 over it; samples after the last whole block are not measured.  n < block: one block of all n samples, so that a short word still
 *     has a level.  l_j = -0.691 + 10 log10(z_j).  Absolute gate: keep l_j > -70.  Relative gate: Gamma = -0.691 + 10 log10(mean z over the
 *     blocks the absolute gate kept) - 10; keep the blocks that also have l_j > Gamma.  loudness[b] = -0.691 + 10 log10(mean z over the blocks
 *     both gates kept); no block past the absolute gate: loudness[b] = rel_threshold[b] = -inf.
 *     peak[b] = max |x| over the finite samples: the SAMPLE peak, exact in fp32 (int16: |s| / 32768).  It is not the true (inter-sample) peak of
 *     BS.1770 annex 2: a ceiling of -1 dBFS on it leaves the usual margin for that, it does not measure it.
 *   Sums.  y^2 is summed per step [m step, (m + 1) step).  The device forms the sum of a step inside each tile of EV_LOUDNESS_TILE samples
 *     (counted from the segment's start) that it reaches into, in an order fixed by the sample's index in its segment; the host adds a step's
 *     tile sums in ascending tile order, a block's four steps in ascending order, then divides by the block's samples.  A float64 restatement
 *     that filters sequentially therefore agrees to rounding (block_ms to about 1e-12 relative), not to the bit.
 *   Gain (host, C double, operations in the order written).  target_lufs NaN = measure only: gain[b] = 1, no output.  Otherwise
 *     1. g = 1 if loudness[b] is -inf (flag EV_LOUDNESS_UNDEFINED, which a measure-only call sets as well), 2. else g = 10^((target - L) / 20);
 *     3. g = min(g, 10^(max_gain_db / 20)) (flag EV_LOUDNESS_BOOST_LIMITED when that lowers g); 4. if peak[b] > 0: g = min(g, (double)peak_ceiling /
 *     (double)peak[b]) (flag EV_LOUDNESS_PEAK_LIMITED when that lowers g); 5. gain[b] = (float)g.
 *   Output (skipped for measure only: wav and wav_i16 are NULL then): out = x * gain[b], one rounded fp32 product of the fp32 sample or of
 *     (float)s / 32768.0f; where gain[b] == 1.0f the source bits pass through.  want_i16: ev_stitch's rule, (int)(out * 32768.0f) truncated toward
 *     zero, then clamped to [-32768, 32767]; it never wraps; NaN -> 0.
 * No atomics; every reduction's order is fixed by (segment, index) alone: a segment gives the same bits, doubles included, alone or anywhere in a
 * batch, from host or device memory, as int16 or as the equal floats.  Needs no weights. */
#define EV_LOUDNESS_MAX_SAMPLES (1 << 30)   /* per segment */
#define EV_LOUDNESS_TILE 4096               /* samples */
#define EV_LOUDNESS_UNDEFINED     1         /* flags[b]: no block passed the absolute gate; the gain is 1 before the peak limit */
#define EV_LOUDNESS_BOOST_LIMITED 2         /* max_gain_db lowered the gain */
#define EV_LOUDNESS_PEAK_LIMITED  4         /* peak_ceiling lowered the gain */
typedef struct ev_loudness_config {
    uint32_t struct_size;          /* sizeof(ev_loudness_config); any other value is rejected */
    int32_t  sample_rate;          /* one of 8000, 16000, 22050, 24000, 32000, 44100, 48000 (ev_flac's table; all divisible by 10) */
    double   target_lufs;          /* finite in [-70, 0], or NaN: measure only */
    double   max_gain_db;          /* finite, >= 0: the largest boost */
    float    peak_ceiling;         /* linear, in (0, 1]: the sample peak of the output stays at or below it (to fp32 rounding) */
    int32_t  want_i16;             /* != 0: also the int16 output */
} ev_loudness_config;
void ev_default_loudness_config(ev_loudness_config* cfg);      /* 16000, NaN (measure only), 20.0, (float)10^(-1/20) = -1 dBFS, 0 */
/* Host only: the ten coefficients above.  0, or -1 for a sample_rate outside the table. */
int ev_loudness_design(int sample_rate, double coef[10]);

typedef struct ev_loudness_result {
    uint32_t struct_size;          /* sizeof(ev_loudness_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total;                /* samples: the sum of lens */
    const float*   wav;            /* DEVICE, (total,), packed as the input; NULL for measure only */
    const int16_t* wav_i16;        /* DEVICE, the same layout; NULL without want_i16 or for measure only */
    const double*  loudness;       /* (batch,) HOST, LUFS; -inf when no block passed the absolute gate */
    const double*  rel_threshold;  /* (batch,) HOST: Gamma, or -inf */
    const float*   gain;           /* (batch,) HOST, linear */
    const float*   peak;           /* (batch,) HOST: the sample peak of the input */
    const uint8_t* flags;          /* (batch,) HOST: EV_LOUDNESS_* */
    const int64_t* nonfinite;      /* (batch,) HOST */
    const int64_t* block_offsets;  /* (batch + 1,) HOST: the blocks of segment b are [block_offsets[b], block_offsets[b + 1]) */
    const double*  block_ms;       /* (block_offsets[batch],) HOST: z_j, segment after segment */
    const uint8_t* block_state;    /* likewise: 0 dropped by the absolute gate, 1 dropped by the relative gate, 2 counted */
} ev_loudness_result;
/* wav: a host pointer, or with EV_FLAG_DEVICE_INPUTS (the other flags are ignored) a device pointer on the handle's device, which must not be the
 * wav of the previous ev_loudness_result; lens is always a HOST array, so an ev_result.wav with lens = mel_lens * 256 or an ev_stitch_result.wav
 * goes straight in, and the result's wav_i16 goes straight into ev_flac.  cfg NULL = ev_default_loudness_config.  Rejected before anything is
 * launched (message naming the field or segment; the previous result stays valid): a NULL h, wav, lens or out, a wrong struct_size of cfg or out,
 * B outside [1, 65535], lens[b] < 1 or > EV_LOUDNESS_MAX_SAMPLES, a sample_rate outside the table, a target_lufs that is neither NaN nor in
 * [-70, 0], a negative or non-finite max_gain_db, a peak_ceiling outside (0, 1].  The tile sums and peaks come back to the host between the
 * measurement and the gain pass: the call's one synchronisation in the middle of its work, as ev_stitch's cut; no waveform is copied to the host.
 * The result lives in a workspace of its own and is complete when the call returns; it stays valid across every other entry point until the next
 * ev_loudness or ev_destroy -- the contract of ev_features_result. */
int ev_loudness(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const ev_loudness_config* cfg, uint32_t flags,
                ev_loudness_result* out);

/* True-peak metering and look-ahead limiting (ev_limit): packed segments -> their sample peak and true (inter-sample) peak, a gain per SAMPLE that
 * holds the true peak at a ceiling, and the limited waveform, on the device: it sits between ev_loudness and ev_flac, so that one plosive no
 * longer lowers the gain of its whole utterance (ev_loudness's step 4).  The reference has no such stage; the arithmetic is the one specified
 * here.  The defaults (-1 dBTP, 80 samples of look-ahead and 800 of hold: 5 ms and 50 ms at 16 kHz) are starting values; none has been measured
 * on a released checkpoint.
 *   Pre-gain: u[n] = x[n] * gains[b], one rounded fp32 product of the fp32 sample or of (float)s / 32768.0f; where gains[b] == 1.0f (or gains is
 *     NULL) the source bits pass through.  A non-finite u (NaN, +-inf) counts once in nonfinite[b] and enters the meter as 0.
 *   Interpolator: h[-64 .. 64] = ev_resample_design(1, 4, 16, 0.945, 9.0): the 4x windowed sinc of ev_resample, 129 fp32 taps.
 *   Oversampled signal: v[4 n + q] = sum_k u[k] h[4 n + q - 4 k], q = 0 .. 3, k ascending over the taps' support, u = +0 outside [0, len): an fp64
 *     accumulation from +0.0 of the exact fp32 x fp32 products in that order, rounded once to fp32.  (An fp64 fma of an exact product equals
 *     multiply-then-add, so contraction cannot change the bits.)
 *   Peaks: p[n] = max(|u[n]|, |v[4 n]|, |v[4 n + 1]|, |v[4 n + 2]|, |v[4 n + 3]|); true_peak_in[b] = max_n p[n], sample_peak_in[b] = max_n |u[n]|.
 *     Known limitation: this is the project's own 4x windowed sinc, not the table printed in BS.1770 annex 2, and it under-reads near Nyquist: a
 *     sine at 0.4 fs reads about 3 % low, one at 0.45 fs about 23 % low (INTEGRATION.md has the table).
 *   Required gain: r[n] = 1.0f if p[n] <= ceiling, else (float)((double)ceiling / (double)p[n]); r = 1 for every index outside [0, len).
 *   Erosion: m[k] = min(r[k - Hd .. k + L]) for EVERY integer k, the indices before 0 and past len - 1 included: m[k] for k in [-L, 0) can be
 *     below 1 (it is not padded with ones; that would break s <= r at a segment's first and last samples).  L = lookahead, Hd = hold.
 *   Window (ev_limit_design, host, fp64): w[j] = 1 - cos(2 pi (j + 1) / (L + 2)), j = 0 .. L, divided by its sum (added in ascending j) and rounded
 *     to fp32; then, while the fp64 sum of the fp32 taps in ascending j exceeds 1, the first largest tap is lowered by one ulp toward 0.
 *   Gain: s[n] = 1.0f exactly when m[n - j] == 1.0f for all j = 0 .. L; otherwise s[n] = (float)(sum_j (double)w[j] * (double)m[n - j]), fp64,
 *     j ascending from +0.0.  Every m[n - j] covers sample n, the taps sum to at most 1 and rounding is monotone, so s[n] <= r[n] bitwise.  The
 *     gain starts to fall L samples before a peak, is at the required value at the peak, holds for Hd samples and is back at 1 after L more.
 *     L = 0 does not smooth: the sample peak holds, the true peak of the output can exceed the ceiling by a few percent.
 *   Output: y[n] = u[n] * s[n], one rounded fp32 product; where s[n] == 1.0f the bits of u pass through.  want_i16: ev_stitch's rule,
 *     (int)(y * 32768.0f) truncated toward zero, then clamped to [-32768, 32767]; it never wraps; NaN -> 0.
 *   true_peak_out / sample_peak_out: the same meter over y (a non-finite y enters as 0).  min_gain[b] = min_n s[n]; limited[b] = the count of
 *     s[n] < 1.
 * No atomics, no recursion, nothing carried from tile to tile: every value depends on (segment, index) alone, and the maxima, the minimum and the
 * counts are exact in any order.  A segment gives the same bits alone or anywhere in a batch, from host or device memory, as int16 or as the
 * equal floats.  Needs no weights.
 *   The second kernel keeps, per tile of EV_LIMIT_TILE samples, r on [t0 - L - Hd, t0 + EV_LIMIT_TILE + L) twice (the erosion doubles its window
 *     from one copy into the other) and the window as fp64 in LDS: EV_LIMIT_LDS_BYTES(L, Hd), within EV_LIMIT_MAX_LDS at the largest L and Hd. */
#define EV_LIMIT_MAX_SAMPLES   (1 << 30)    /* per segment */
#define EV_LIMIT_MAX_LOOKAHEAD 1024         /* samples */
#define EV_LIMIT_MAX_HOLD      8192         /* samples */
#define EV_LIMIT_TILE          4096         /* samples */
#define EV_LIMIT_MAX_LDS       (160 * 1024)
#define EV_LIMIT_REACH(L, Hd)     (EV_LIMIT_TILE + 2 * (L) + (Hd))                      /* samples of r a tile looks at */
#define EV_LIMIT_LDS_BYTES(L, Hd) (2 * 4 * EV_LIMIT_REACH(L, Hd) + 8 * ((L) + 1))
#ifdef __cplusplus
static_assert(EV_LIMIT_LDS_BYTES(EV_LIMIT_MAX_LOOKAHEAD, EV_LIMIT_MAX_HOLD) <= EV_LIMIT_MAX_LDS, "ev_limit's largest tile must fit the LDS of a CU");
static_assert(EV_LIMIT_LDS_BYTES(EV_LIMIT_MAX_LOOKAHEAD, EV_LIMIT_MAX_HOLD) == 122888, "2 * 4 * (4096 + 2048 + 8192) + 8 * 1025");
#endif
typedef struct ev_limit_config {
    uint32_t struct_size;          /* sizeof(ev_limit_config); any other value is rejected */
    int32_t  sample_rate;          /* one of 8000, 16000, 22050, 24000, 32000, 44100, 48000 (ev_flac's table) */
    float    ceiling;              /* linear, in (0, 1]: the true peak of the output aims at it */
    int32_t  lookahead;            /* L, samples, in [0, EV_LIMIT_MAX_LOOKAHEAD] */
    int32_t  hold;                 /* Hd, samples, in [0, EV_LIMIT_MAX_HOLD] */
    int32_t  want_i16;             /* != 0: also the int16 output */
} ev_limit_config;
void ev_default_limit_config(ev_limit_config* cfg);      /* 16000, (float)10^(-1/20) = -1 dBTP, 80, 800, 0 */
/* Host only: the L + 1 taps of the smoothing window above.  Returns L + 1, or -1 for L outside [0, EV_LIMIT_MAX_LOOKAHEAD] or a NULL w. */
int ev_limit_design(int L, float* w);

typedef struct ev_limit_result {
    uint32_t struct_size;          /* sizeof(ev_limit_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total;                /* samples: the sum of lens */
    const float*   wav;            /* DEVICE, (total,), packed as the input: y */
    const int16_t* wav_i16;        /* DEVICE, the same layout; NULL without want_i16 */
    const float*   true_peak_in;   /* every array below: (batch,) HOST */
    const float*   sample_peak_in;
    const float*   true_peak_out;
    const float*   sample_peak_out;
    const float*   min_gain;       /* min s */
    const int64_t* limited;        /* samples with s < 1 */
    const int64_t* nonfinite;      /* non-finite u */
} ev_limit_result;
/* wav: a host pointer, or with EV_FLAG_DEVICE_INPUTS (the other flags are ignored) a device pointer on the handle's device, which must not be the
 * wav of the previous ev_limit_result; lens is always a HOST array, so an ev_result.wav with lens = mel_lens * 256, an ev_stitch_result.wav or an
 * ev_loudness_result.wav goes straight in, and the result's wav_i16 goes straight into ev_flac.  gains: a HOST array (B,) of pre-gains, or NULL =
 * all 1: with ev_loudness's measurement and its gain rule without step 4, one pass scales and limits.  cfg NULL = ev_default_limit_config.
 * Rejected before anything is launched (message naming the field or segment; the previous result stays valid): a NULL h, wav, lens or out, a
 * wrong struct_size of cfg or out, a sample_rate outside the table, a ceiling outside (0, 1] or not finite, lookahead outside
 * [0, EV_LIMIT_MAX_LOOKAHEAD], hold outside [0, EV_LIMIT_MAX_HOLD], B outside [1, 65535], lens[b] < 1 or > EV_LIMIT_MAX_SAMPLES, a gains[b] that
 * is negative, NaN or infinite.  The per-tile records come back to the host once, at the end of the call; no waveform is copied to the host.
 * The result lives in a workspace of its own and is complete when the call returns; it stays valid across every other entry point until the next
 * ev_limit or ev_destroy -- the contract of ev_features_result. */
int ev_limit(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const float* gains, const ev_limit_config* cfg, uint32_t flags,
             ev_limit_result* out);

/* Response delivery (ev_deliver): packed utterances at sr_in (the model's 16 kHz) -> the bytes a client asked for: the waveform at sr_out as fp32,
 * as int16 (optionally TPDF-dithered), or as G.711 mu-law / A-law, on the device -- the last stage after ev_limit, so that an 8 kHz mu-law response
 * leaves the device as 1/8 of the bytes of the fp32 waveform and no fp32 intermediate reaches memory unless fp32 is the encoding.  The reference has
 * no such stage.  The filter is ev_resample's own windowed sinc (not soxr, not ffmpeg); G.711 is held to CPython's audioop and to the restatement
 * below (no telephony endpoint was exercised); the dither generator is the integer hash specified here, checked for mean and variance only.
 * Upsampling after the limiter can overshoot its ceiling: peak and clipped report it, the stage does not limit again.
 *   Filter: y[m], m < n = ceil(L up / down), is EXACTLY ev_resample's output sample: the same prototype design (ev_resample_design's default for
 *     the rate pair, or the caller's taps), the same phase-major table, the same k range, the same four interleaved fmaf partial sums combined as
 *     (s0 + s1) + (s2 + s3), the same zero padding and x / 32768 for int16 input; sr_in == sr_out passes the sample through with no filter.  With
 *     EV_DELIVER_F32 the bytes of an utterance therefore equal ev_resample's for the same taps.
 *   EV_DELIVER_S16 without dither: t = y * 32768.0f (one fp32 product); s = (int)t truncated toward zero, clamped to [-32768, 32767]; NaN -> 0
 *     (ev_stitch's rule).
 *   EV_DELIVER_S16 with TPDF dither: on uint32 with wraparound, h(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16.
 *     For a uint64 counter c, mix(seed, c) = h(h((uint32)c + h(seed ^ (uint32)(c >> 32))) ^ seed).  ua = mix(s_b, 2 m) >> 8, ub = mix(s_b, 2 m + 1)
 *     >> 8, d = (float)((int)ua - (int)ub) * 2^-24 (exact in fp32, |d| < 1); s = rintf(t + d): one fp32 add, ties to even, clamped, NaN -> 0.
 *     s_b = seeds[b] when the host array seeds is given, else cfg.seed: the bits of a sample depend on (utterance, its seed, m) alone.
 *     Known answers: mix(0, 0) = 0x00000000, mix(1, 5) = 0x820138b2, mix(12345, 2^32 + 7) = 0xe07a7e79.
 *   EV_DELIVER_ULAW, from s (dithered or not): v = s >> 2 (arithmetic); v < 0: v = -v, mask = 0x7F, else mask = 0xFF; v = min(v, 8159) + 33; seg =
 *     the index of the first end in {0x3F, 0x7F, 0xFF, 0x1FF, 0x3FF, 0x7FF, 0xFFF, 0x1FFF} with v <= end; byte = ((seg << 4) | ((v >> (seg + 1)) &
 *     0xF)) ^ mask; no such end (v = 8192, the clipped magnitude): byte = 0x7F ^ mask, as audioop answers.
 *   EV_DELIVER_ALAW, from s: v = s >> 3; v >= 0: mask = 0xD5, else mask = 0x55 and v = -v - 1; seg over the ends {0x1F, 0x3F, 0x7F, 0xFF, 0x1FF,
 *     0x3FF, 0x7FF, 0xFFF}; nibble = (v >> 1) & 0xF for seg < 2, else (v >> seg) & 0xF; byte = ((seg << 4) | nibble) ^ mask.
 *   peak[b] = max |y| over the finite samples (before any conversion).  clipped[b] = the count of samples whose t (with dither: t + d) is below
 *     -32768 or above 32767 (a NaN is not counted); 0 for EV_DELIVER_F32.
 *   Layout: utterance b occupies data[byte_offsets[b] .. byte_offsets[b + 1]); its n_samples[b] * (4, 2, 1, 1) bytes come first, zeros fill the
 *     rest; every byte_offsets[b] is a multiple of 16.
 * The kernel writes EV_DELIVER_TILE consecutive outputs of one utterance per block, four consecutive outputs per thread as one store of 16 / 8 /
 * 4 bytes.  No atomics and no floating sum split over threads: an utterance gives the same bytes alone or anywhere in a batch, as int16 or as
 * the equal floats, from host or device memory; the max and the count are exact in any order.  Needs no weights. */
#define EV_DELIVER_F32  0
#define EV_DELIVER_S16  1
#define EV_DELIVER_ULAW 2
#define EV_DELIVER_ALAW 3
#define EV_DELIVER_TILE 1024      /* outputs per block of the kernel */
typedef struct ev_deliver_config {
    uint32_t struct_size;          /* sizeof(ev_deliver_config); any other value is rejected */
    int32_t  sr_in, sr_out;        /* >= 1; up and down <= EV_RESAMPLE_MAX_RATIO */
    int32_t  encoding;             /* EV_DELIVER_* */
    int32_t  dither;               /* 0 = none, 1 = TPDF; not with EV_DELIVER_F32 */
    uint32_t seed;                 /* the dither's seed where ev_deliver is given no seeds */
    int32_t  half_len;             /* with taps: (len - 1) / 2 >= 1; ignored without */
    const float* taps;             /* HOST (2 half_len + 1) or NULL = ev_resample_design's default for the rate pair; copied */
} ev_deliver_config;
void ev_default_deliver_config(ev_deliver_config* cfg);      /* 16000 -> 16000, EV_DELIVER_S16, no dither, seed 0, taps NULL */
/* Copies the taps (or designs the default ones) and builds the device table, in a workspace of its own: it does not disturb ev_resample_setup's
 * state, nor the reverse.  Rejected (message naming the field): a wrong struct_size, sr_in or sr_out < 1, up or down > EV_RESAMPLE_MAX_RATIO, an
 * unknown encoding or dither, dither with EV_DELIVER_F32, taps with half_len < 1, more than EV_RESAMPLE_MAX_TAPS taps, a non-finite tap.  A
 * rejected setup leaves the previous one in place. */
int ev_deliver_setup(ev_handle* h, const ev_deliver_config* cfg);

typedef struct ev_deliver_result {
    uint32_t struct_size;          /* sizeof(ev_deliver_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total_bytes;          /* byte_offsets[batch] */
    const uint8_t* data;           /* DEVICE, (total_bytes,); an EV_DELIVER_S16 utterance at data + byte_offsets[b] goes straight into ev_flac as int16 */
    const int64_t* byte_offsets;   /* (batch+1,) HOST, multiples of 16 */
    const int64_t* n_samples;      /* (batch,) HOST: ceil(lens[b] up / down) */
    const float*   peak;           /* (batch,) HOST */
    const int64_t* clipped;        /* (batch,) HOST */
} ev_deliver_result;
/* wav / wav_is_i16 / lens / EV_FLAG_DEVICE_INPUTS as ev_limit (an ev_limit_result.wav, an ev_loudness_result.wav, an ev_stitch_result.wav or an
 * ev_result.wav goes straight in).  seeds: a HOST array (B,) of uint32, or NULL = cfg.seed for every utterance; read only with dither.  Rejected
 * before anything is launched (message naming the field or utterance; the previous result stays valid): a NULL h, wav, lens or out, a wrong
 * struct_size, no ev_deliver_setup, B outside [1, 65535], lens[b] < 1, an utterance with more than EV_ALIGN_MAX_FRAMES * 256 output samples
 * (ev_resample's limit).  The per-utterance figures come back to the host once, at the end of the call; no waveform is copied to the host.  The
 * result lives in a workspace of its own and is complete when the call returns; it stays valid across every other entry point until the next
 * ev_deliver or ev_destroy -- the contract of ev_limit_result. */
int ev_deliver(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const uint32_t* seeds, uint32_t flags, ev_deliver_result* out);

/* Vocoder bias removal (ev_denoise): the stationary tone and hiss a GAN vocoder emits even for an all-zero mel, subtracted from the magnitude
 * spectrum of every utterance on the device -- the `Denoiser` of the Tacotron 2 / WaveGlow / FastPitch recipes.  It runs first in the output
 * chain, on the vocoder's (or ev_stitch's) waveform, before ev_loudness, ev_limit and ev_deliver.  The arithmetic is that of the reference's
 * STFT class (models/prompt_tts_modified/stft.py: transform, clamp(mag - s bias, 0), inverse with window-sum normalisation), against which it is
 * tested; NVIDIA's Denoiser code itself was not available.  The default strength 0.01 is FastPitch's published value for HiFi-GAN, an UNMEASURED
 * starting value here: nobody has listened to a released checkpoint with it, and no audible improvement is claimed.
 *   1 Input.  x[i], i < L: the fp32 sample, or s / 32768 for int16.  padded[i] = x reflected by n_fft / 2 at both ends (numpy's "reflect": the edge
 *     sample is not repeated), which needs L >= n_fft / 2 + 1.  T = L / hop + 1 frames (integer division); frame t is padded[hop t .. hop t + n_fft).
 *   2 Basis.  Exactly ev_features' (step 2 there): float32(cos / -sin(2 pi k n / n_fft)) * float32 window[n], k = 0 .. n_fft / 2; window NULL =
 *     periodic hann evaluated in float64 and rounded to float32.  Re[t][k], Im[t][k] = frame t times the two rows of bin k, operands split as
 *     x = hi + 2^-11 lo in fp16 (lo x lo dropped), products accumulated in fp32 by the matrix cores.
 *   3 Gain.  mag = sqrtf(Re^2 + Im^2); g = mag > 0 ? max(mag - s_b * bias[k], 0) / mag : 0, in fp32, s_b = strengths[b] or cfg.strength; mag == 0
 *     (and a NaN) gives a zero cell.  The cell becomes g Re, g Im, again split into fp16 hi / lo planes in a scratch in device memory
 *     ([frame][k_pad], k_pad = 2 (n_fft / 2 + 1) rounded up to 32): |g Re| and |g Im| must stay below 65504, which holds for |x| <= 100.
 *   4 Inverse.  The untrimmed signal u[i], i < n_fft + hop (T - 1): u[i] = sum over the frames t with 0 <= i - hop t < n_fft, t ascending, of
 *     sum_k c_k (g Re[t][k] cos(2 pi k m / n_fft) - g Im[t][k] sin(2 pi k m / n_fft)) * window[m], m = i - hop t, c_k = 1 for k = 0 and n_fft / 2,
 *     else 2 (the weights of the real inverse DFT; the reference's pinv basis equals this wherever Im[0] = Im[n_fft / 2] = 0, which a gain on a real
 *     signal's spectrum preserves).  The table entries are float32(c_k cos / -c_k sin) * float32 window[m]; one GEMM row per chunk of hop samples
 *     over the R = n_fft / hop frames that reach it, so the overlap-add is the GEMM's own fp32 accumulation in one fixed order.
 *   5 Envelope.  env[i] = the reference's window_sumsquare: a float32 accumulator from 0, += (double)window[m]^2 over the same frames, t ascending
 *     (window NULL: the square of the float64 hann before its rounding to float32, as the reference squares scipy's float64 window).
 *     y = u * (1.0f / n_fft) (one fp32 product; the reference's pinv scale hop / n_fft and its final n_fft / hop cancel), then y = y / env[i]
 *     where env[i] > FLT_MIN (the reference's tiny), else y unchanged.
 *   6 Trim.  out[i] = y[i + n_fft / 2], i < hop (L / hop): the output length is L rounded down to a multiple of hop (the reference's), so a
 *     waveform of whole frames -- every ev_result.wav -- keeps its length.
 *   7 int16 (want_i16): ev_loudness' rule -- t = out * 32768.0f (one fp32 product), clamped to [-32768, 32767], truncated toward zero; NaN -> 0.
 * Strength 0 is the identity up to the float32 round trip (about 1e-7 of the peak).  No atomics and nothing carried between blocks: an
 * utterance gives the same bits alone, anywhere in a batch and in any batch, as int16 or as the equal floats, from host or device memory.
 * Shapes: n_fft a multiple of 128 up to EV_FEATURES_MAX_NFFT, hop a multiple of 8 dividing n_fft with n_fft / hop <= EV_DENOISE_MAX_R, and
 * ev_features' limit EV_FEATURES_MAX_RUN on 63 hop + n_fft.  The scratch takes 4 k_pad bytes per frame (about 130 MB at 32 x 16 s). */
#define EV_DENOISE_MAX_R 8             /* n_fft / hop */
#define EV_DENOISE_BIAS_FRAMES 88      /* the zero mel ev_denoise_setup vocodes to measure the bias (the Denoiser's choice) */
typedef struct ev_denoise_config {
    uint32_t struct_size;          /* sizeof(ev_denoise_config); any other value is rejected */
    int32_t  n_fft, hop;
    int32_t  want_i16;             /* also write the clamped int16 waveform */
    float    strength;             /* >= 0 and finite: s_b where ev_denoise is given no strengths */
    const float* window;           /* HOST (n_fft,) or NULL = periodic hann; copied */
} ev_denoise_config;
void ev_default_denoise_config(ev_denoise_config* cfg);      /* 1024, 256, no int16, strength 0.01, window NULL */
/* Builds the tables in a workspace of its own (it leaves ev_features_setup alone) and takes the bias: `bias` is a HOST array (n_fft / 2 + 1,) of
 * finite values >= 0, or NULL -- then the engine measures its own: it runs ev_vocoder on an all-zero mel of EV_DENOISE_BIAS_FRAMES frames (which
 * needs weights and replaces the last ev_result) and keeps the magnitudes (step 3's mag) of frame 0 of that waveform on the device.  Rejected
 * (message naming the field): a wrong struct_size, a shape outside the limits above, a negative or non-finite strength or bias value.  A
 * rejected setup leaves the previous one in place. */
int ev_denoise_setup(ev_handle* h, const ev_denoise_config* cfg, const float* bias);
/* Copies the bias in use to out, HOST (n_fft / 2 + 1,): what to store beside a checkpoint and pass back to ev_denoise_setup, bit for bit. */
int ev_denoise_bias(ev_handle* h, float* out);

typedef struct ev_denoise_result {
    uint32_t struct_size;          /* sizeof(ev_denoise_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total;                /* offsets[batch] */
    const float*   wav;            /* DEVICE, (total,) utterances back to back: what ev_loudness / ev_limit / ev_deliver / ev_flac take */
    const int16_t* wav_i16;        /* DEVICE, the same layout; NULL without want_i16 */
    const int64_t* lens_out;       /* (batch,) HOST: hop * (lens[b] / hop) */
    const int64_t* offsets;        /* (batch+1,) HOST */
} ev_denoise_result;
/* wav / wav_is_i16 / lens / EV_FLAG_DEVICE_INPUTS as ev_limit (an ev_result.wav with lens = mel_lens * 256 or an ev_stitch_result.wav goes straight
 * in).  strengths: a HOST array (B,) of finite values >= 0, or NULL = cfg.strength for every utterance.  Rejected before anything is launched
 * (message naming the field or utterance; the previous result stays valid): a NULL h, wav, lens or out, a wrong struct_size, no ev_denoise_setup,
 * B outside [1, 65535], lens[b] < n_fft / 2 + 1, an utterance of more than EV_ALIGN_MAX_FRAMES frames, a bad strength.  The result lives in a
 * workspace of its own and is complete when the call returns; it stays valid across every other entry point until the next ev_denoise or
 * ev_destroy -- the contract of ev_limit_result. */
int ev_denoise(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const float* strengths, uint32_t flags, ev_denoise_result* out);

/* Time-scale modification (ev_stretch): a finished waveform at another length and the same pitch, per segment, on the device -- the waveform
 * meaning of the reference's `speed` (openaiapi.py: pyrb.time_stretch) and the last few per cent of "this sentence in exactly 2.50 s".  It runs
 * second in the output chain, after ev_denoise and before ev_loudness, so that the later stages measure and shape what is delivered.
 * This is WSOLA (waveform-similarity overlap-add) with a squared-difference search on 12-bit samples.  It is NOT Rubber Band, which is a phase
 * vocoder with transient handling; nobody has listened to it and it was compared to no other stretcher; N, H and the lag range are UNMEASURED
 * starting values chosen for 16 kHz speech, in samples, and used as they are at any other rate.  Everything is integer except the last sum.
 *   1 Lengths (host, ev_stretch_plan).  From a speed s: L_out = max(1, rint(L_in / s)) in fp64, ties to even; a target in samples is used as it
 *     is.  Needed: L_in >= 1, L_out >= 1, both <= EV_STRETCH_MAX_SAMPLES, and L_in <= 2 L_out and L_out <= 2 L_in unless min(L_in, L_out) <
 *     EV_STRETCH_FRAME (at a few samples the ratio means nothing).
 *   2 Decision samples.  x[i]: the fp32 sample, or s / 32768 for int16; zero outside [0, L_in).  q[i] = clamp(rint(x[i] * 2048), -2047, 2047) as an
 *     integer, ties to even; a non-finite sample gives 0 and counts in nonfinite.
 *   3 Frames.  N = EV_STRETCH_FRAME, H = EV_STRETCH_HOP, K = ceil(L_out / H).  a_k = floor((2 k H L_in + L_out) / (2 L_out)) in int64, the nominal
 *     read position.  p_(-1) = -H, delta_0 = 0.  For k >= 1 the template starts at t_k = p_(k-1) + H, the natural continuation of the previous frame;
 *     D_k(d) = sum_(n < N) (q[t_k + n] - q[a_k + d + n])^2 for the lags d in [-EV_STRETCH_LAGS / 2, EV_STRETCH_LAGS / 2 - 1], an exact integer
 *     (it reaches 8.6e9); delta_k = the lag of the smallest D_k, ties to the smallest |d|, then to the negative one.  p_k = a_k + delta_k.
 *   4 Window (ev_stretch_window, host, fp64): w[j] = rint(2^23 (0.5 - 0.5 cos(2 pi j / N))) / 2^23, j < H, the rising half; the falling half is
 *     1 - w[j].  Both are exact in fp32 and they sum to exactly 1.
 *   5 Output.  For m < L_out, k = m / H, j = m % H: y[m] = (float)((double)w[j] (double)x[p_k + j] + (double)(1 - w[j]) (double)x[p_(k-1) + H + j]):
 *     two products that are exact in fp64, one fp64 sum, one rounding to fp32.  A non-finite x reaches y by IEEE rules (0 * Inf = NaN).
 *   6 int16 (want_int16): ev_loudness' rule -- t = y * 32768.0f (one fp32 product), clamped to [-32768, 32767], truncated toward zero; NaN -> 0.
 *   7 Figures per segment: frames = K; edge_frames = the count of k >= 1 whose lag sits on either end of the range; sum_dist = the sum over
 *     k >= 1 of D_k(delta_k); nonfinite; deltas, the track itself (delta_0 = 0 included).
 * What follows from the rules: L_out == L_in returns a finite input bit for bit (distance 0 at lag 0 wins every tie; w x + (1 - w) x is exact);
 * a segment gives the same bits alone or anywhere in a batch, as int16 or as the equal floats, from host or device memory; an input of integer
 * period P <= EV_STRETCH_LAGS / 2 comes out as y[m] = x[m % P] away from its end.  A segment's last 896 / r + 256 output samples (r = L_in /
 * L_out) read the zero extension: the search there is against silence.  The search of one segment is a serial chain of K steps on one compute
 * unit; a batch runs its segments side by side.  No atomics.  Needs no setup call and no weights. */
#define EV_STRETCH_FRAME 512                 /* N, samples */
#define EV_STRETCH_HOP   256                 /* H, samples */
#define EV_STRETCH_LAGS  256                 /* lags -128 .. 127 */
#define EV_STRETCH_MAX_SAMPLES (1 << 30)     /* per segment, in and out */
typedef struct ev_stretch_config {
    uint32_t struct_size;          /* sizeof(ev_stretch_config); any other value is rejected */
    int32_t  want_int16;           /* also write the clamped int16 waveform */
} ev_stretch_config;
void ev_default_stretch_config(ev_stretch_config* cfg);      /* no int16 */
/* Host only: the EV_STRETCH_HOP values of the rising half of the window (step 4).  Returns EV_STRETCH_HOP, or -1 for a NULL w. */
int ev_stretch_window(float* w);
/* Host only: step 1 for B segments.  lens: (B,) L_in.  Segment b takes targets[b] samples where targets is given and targets[b] != 0, else the
 * length that speeds[b] gives (speeds NULL: 1.0).  Writes lens_out (B,) and returns 0; or returns -1 with the message, which names the segment
 * and the rule, in ev_last_error(NULL): a NULL lens or lens_out, B outside [1, 65535], a speed that is not finite and > 0, a broken rule of step 1. */
int ev_stretch_plan(int B, const int64_t* lens, const double* speeds, const int64_t* targets, int64_t* lens_out);

typedef struct ev_stretch_result {
    uint32_t struct_size;          /* sizeof(ev_stretch_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total;                /* offsets[batch] */
    const float*   wav;            /* DEVICE, (total,) segments back to back: what ev_loudness / ev_limit / ev_deliver / ev_flac take */
    const int16_t* wav_i16;        /* DEVICE, the same layout; NULL without want_int16 */
    const int64_t* lens_out;       /* (batch,) HOST: the call's lens_out */
    const int64_t* offsets;        /* (batch+1,) HOST */
    const int32_t* frames;         /* (batch,) HOST: K */
    const int64_t* frame_offsets;  /* (batch+1,) HOST: segment b's lags are deltas[frame_offsets[b] .. frame_offsets[b+1]) */
    const int16_t* deltas;         /* DEVICE, (frame_offsets[batch],) */
    const int32_t* edge_frames;    /* (batch,) HOST */
    const uint64_t* sum_dist;      /* (batch,) HOST */
    const int64_t* nonfinite;      /* (batch,) HOST */
} ev_stretch_result;
/* wav / wav_is_i16 / lens / EV_FLAG_DEVICE_INPUTS as ev_limit (an ev_result.wav with lens = mel_lens * 256, an ev_denoise_result.wav or an
 * ev_stitch_result.wav goes straight in).  lens_out: a HOST array (B,), what ev_stretch_plan wrote or the caller's own targets.  cfg NULL =
 * ev_default_stretch_config.  Rejected before anything is launched (message naming the field or segment; the previous result stays valid): a NULL
 * h, wav, lens, lens_out or out, a wrong struct_size, B outside [1, 65535], a pair (lens[b], lens_out[b]) that breaks a rule of step 1, more than
 * INT_MAX output tiles in one call.  The result lives in a workspace of its own and is complete when the call returns; it stays valid across
 * every other entry point until the next ev_stretch or ev_destroy -- the contract of ev_limit_result. */
int ev_stretch(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const int64_t* lens_out, const ev_stretch_config* cfg,
               uint32_t flags, ev_stretch_result* out);

/* Audio watermark (ev_watermark, ev_watermark_detect): a keyed, machine-detectable mark in a finished waveform, so that the operator of the
 * engine can answer "did this audio come from us?".  The embed runs third in the output chain, after ev_stretch (which would move the tiles) and
 * before ev_loudness and ev_limit (a gain does not change the detector's signs).  It is a spread-spectrum mark on the STFT magnitude: every cell
 * of a band is raised or lowered by a fraction of a dB according to a pseudo-random chip, and the detector correlates the sign of the local
 * contrast of the log band energies with the chips.  Every constant below is an UNMEASURED starting value for 16 kHz speech.  Not verified:
 * nobody has listened to it and no imperceptibility is claimed; it was compared with no other watermark (AudioSeal, WavMark: none installed); it
 * was not tested against mp3, Opus or acoustic re-recording; the hash is not a proven source of independent bits and nothing here is a defence
 * against someone who wants the mark gone -- no security claim.
 * Shapes: n_fft = EV_WATERMARK_NFFT, hop = EV_WATERMARK_HOP, periodic hann: ev_denoise's frames, padding, limits and frame count at those values.
 *   Pattern (host, ev_watermark_pattern).  Chip i = 48 u + v, tile u < EV_WATERMARK_PERIOD, band v < EV_WATERMARK_BANDS.  h = mix(key, i) with
 *     hash(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32 and mix(key, c) = hash(hash((uint32)c +
 *     hash(key ^ (uint32)(c >> 32))) ^ key) -- ev_deliver's dither hash.  sign = (h & 1) ? +1 : -1; role = (h >> 1) mod (2 nbits).  A role <
 *     nbits carries that payload bit: its sign is flipped where the bit is 1.  Every other role is a pilot; with nbits = 0 every chip is.
 *   Embed.
 *   1, 2 ev_denoise's steps 1 and 2, word for word: input, reflect padding, T = L / hop + 1 frames, basis, split-precision GEMM.
 *   3 Gain.  Band v holds the bins EV_WATERMARK_BAND0 + 4 v .. + 3.  mag = sqrtf(Re^2 + Im^2); for a cell (t, k) of band v, u = (t / 8) mod 16 and
 *     g = a where chip 48 u + v has sign +1, float32(1 / a) (one fp32 division) where it has -1; g = 1 outside the bands; mag == 0 (and a NaN)
 *     gives a zero cell.  a = float32(10^(strength_db / 20)), formed on the host in fp64.  The cell becomes g Re, g Im in ev_denoise's scratch.
 *   4 .. 7 ev_denoise's steps 4 to 7, word for word: inverse GEMM, envelope, trim to hop (L / hop) samples, int16 rule.
 *   Consequences: strength_db = 0 gives ev_denoise's output at strength 0 bit for bit; no atomics and nothing carried between blocks, so a segment
 *   gives the same bits alone and in any batch.
 *   Detect.
 *   D1 Steps 1 and 2 again.  m2[t][k] = (Re Re) + (Im Im): two rounded fp32 products and one rounded sum, never fused.
 *   D2 Band energy E[t][v] = (m2[k0] + m2[k0 + 1]) + (m2[k0 + 2] + m2[k0 + 3]), k0 = EV_WATERMARK_BAND0 + 4 v, rounded fp32 sums in that order.
 *   D3 Floor.  M[t] = the largest m2[t][k] over ALL n_fft / 2 + 1 bins (carried through the GEMM's bin tiles before any band is written);
 *     E = max(E, M * 2^-24).
 *   D4 q[t][v] = bits(E) >> 17 as an integer: the float's exponent and its top six mantissa bits, a monotone piecewise-linear log2 in steps of
 *     1 / 64 octave and an exact function of E.
 *   D5 For every offset s in 0 .. EV_WATERMARK_OFFSETS - 1: tiles start at the frames f >= 0 with (f - s) mod 8 == 0 and f + 8 <= T (whole
 *     tiles only); tile j (f = s mod 8 + 8 j) carries the chips of u = (j - s / 8) mod 16.  D[j][v] = the sum of q over the tile's 8 frames.
 *     X = 2 D[j] - D[j - 1] - D[j + 1] for the interior tiles.  C(s) = the sum over the pilot chips of sign(chip) sign(X), n(s) = the count of
 *     pilot chips with X != 0.
 *   D6 The reported offset maximises C / sqrt(n) over the offsets with C > 0, compared exactly in int64 as C_a^2 n_b against C_b^2 n_a; a tie goes
 *     to the smaller offset; without any C > 0 the offset is 0.  At that offset C_j, n_j are the same sums over the chips of payload bit j, with
 *     the signs of payload 0.
 *   D7 The device returns integers only.  The host forms z = C / sqrt(n) in fp64 (0 for n = 0), present = z >= threshold, bit j = C_j < 0.
 *   Given q everything is integer: exact in any summation order.
 *   Threshold: derived, not measured.  For fixed audio and independent +-1 chips Hoeffding gives P(z >= t) <= exp(-t^2 / 2); over 128 offsets
 *   t = 6.25 bounds the false-alarm rate per segment and key at 128 exp(-19.5) < 5e-7 -- if the hash's bits were independent, which is not proven. */
#define EV_WATERMARK_NFFT    1024
#define EV_WATERMARK_HOP     256
#define EV_WATERMARK_BAND0   20        /* first bin of band 0: 312.5 Hz at 16 kHz */
#define EV_WATERMARK_BANDS   48        /* of 4 bins each: up to 3.3125 kHz, inside the telephone band */
#define EV_WATERMARK_TILE    8         /* frames per time tile */
#define EV_WATERMARK_PERIOD  16        /* tiles per pattern period: 128 frames, 2.048 s */
#define EV_WATERMARK_CHIPS   768       /* PERIOD * BANDS */
#define EV_WATERMARK_OFFSETS 128       /* TILE * PERIOD */
#define EV_WATERMARK_MAX_BITS 16
#define EV_WATERMARK_MAX_DB  6.0f      /* strength_db in [0, 6]: the scratch's fp16 range then holds for |x| <= 50 */
#define EV_WATERMARK_THRESHOLD 6.25
typedef struct ev_watermark_config {
    uint32_t struct_size;          /* sizeof(ev_watermark_config); any other value is rejected */
    uint32_t key;                  /* per call */
    int32_t  want_i16;             /* also write the clamped int16 waveform */
    int32_t  nbits;                /* 0 .. EV_WATERMARK_MAX_BITS: the payload length where ev_watermark is given no nbits */
    uint32_t payload;              /* < 2^nbits: likewise */
    float    strength_db;          /* in [0, EV_WATERMARK_MAX_DB]: likewise */
} ev_watermark_config;
void ev_default_watermark_config(ev_watermark_config* cfg);      /* key 0, no int16, nbits 0, payload 0, 1.0 dB */
/* Host only: the EV_WATERMARK_CHIPS signs (+1 / -1) of the pattern, payload flips applied.  0, or -1 for a NULL signs, nbits outside
 * [0, EV_WATERMARK_MAX_BITS] or payload >= 2^nbits. */
int ev_watermark_pattern(uint32_t key, int nbits, uint32_t payload, int8_t* signs);

typedef struct ev_watermark_result {
    uint32_t struct_size;          /* sizeof(ev_watermark_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int64_t  total;                /* offsets[batch] */
    const float*   wav;            /* DEVICE, (total,) segments back to back: what ev_loudness / ev_limit / ev_deliver / ev_flac take */
    const int16_t* wav_i16;        /* DEVICE, the same layout; NULL without want_i16 */
    const int64_t* lens_out;       /* (batch,) HOST: hop * (lens[b] / hop) */
    const int64_t* offsets;        /* (batch+1,) HOST */
} ev_watermark_result;
/* wav / wav_is_i16 / lens / EV_FLAG_DEVICE_INPUTS as ev_denoise.  cfg NULL = ev_default_watermark_config.  payloads (uint32), nbits (int32) and
 * strengths_db (float): HOST arrays (B,), or NULL = the config's value for every segment.  Needs no setup call and no weights (the tables are
 * built on the first call).  Rejected before anything is launched (message naming the field or segment; the previous result stays valid): a
 * NULL h, wav, lens or out, a wrong struct_size, B outside [1, 65535], lens[b] < n_fft / 2 + 1, a segment of more than EV_ALIGN_MAX_FRAMES
 * frames, nbits outside [0, EV_WATERMARK_MAX_BITS], a payload >= 2^nbits, a strength outside [0, EV_WATERMARK_MAX_DB] or not finite.  The
 * result lives in a workspace of its own and stays valid until the next ev_watermark or ev_destroy -- the contract of ev_limit_result. */
int ev_watermark(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const ev_watermark_config* cfg, const uint32_t* payloads,
                 const int32_t* nbits, const float* strengths_db, uint32_t flags, ev_watermark_result* out);

typedef struct ev_watermark_detect_result {
    uint32_t struct_size;          /* sizeof(ev_watermark_detect_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int32_t  nbits;                /* the call's */
    int32_t  reserved;
    const int32_t* offset;         /* (batch,) HOST: D6 */
    const int32_t* C;              /* (batch,) HOST */
    const int32_t* n;              /* (batch,) HOST */
    const int32_t* bit_C;          /* (batch, EV_WATERMARK_MAX_BITS) HOST; zero from nbits on */
    const int32_t* bit_n;          /* (batch, EV_WATERMARK_MAX_BITS) HOST */
    const int32_t* frames;         /* (batch,) HOST: T */
    const int64_t* frame_offsets;  /* (batch+1,) HOST: segment b's rows of q */
    const int32_t* q;              /* DEVICE, (frame_offsets[batch], EV_WATERMARK_BANDS): D4 */
} ev_watermark_detect_result;
/* Inputs as ev_watermark; key and nbits are per call.  Rejected as ev_watermark rejects.  The result stays valid until the next
 * ev_watermark_detect or ev_destroy. */
int ev_watermark_detect(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, uint32_t key, int nbits, uint32_t flags,
                        ev_watermark_detect_result* out);

/* Objective scoring (ev_score): how close a signal a (under test: a synthesised utterance) is to a signal b (the yardstick: a recording of the
 * same sentence) when the two differ in length and timing -- mel-cepstral distortion, F0 error in cents and the voiced / unvoiced error rate
 * along a dynamic-time-warping path, on the device.  ev_compare is the measure for signals of equal length; with EV_SCORE_LINEAR the same scores
 * are taken without a warp (an mx against a strict rendering with forced durations).  The reference has no such stage.  The scores are specified on
 * integers, so that a restatement in numpy and Python integers reproduces every decision and every sum; nothing depends on how a square root or a
 * cosine is rounded.  This is an MFCC-style MCD on the engine's own log-mel (ev_features), NOT SPTK's warped mel-cepstrum: the figures compare
 * among themselves only, and nobody has set them against a published MCD.
 * The calls are two-step because an ev_features_result is valid only until the next ev_features: ev_score_load copies what scoring needs of one
 * side (the integer cepstra, the F0 track) into a workspace of ev_score's own, ev_score scores the two loaded sides pair by pair.
 *   1 Basis.  basis[d-1][m] = (float)(sqrt(2.0 / M) * cos(pi * d * (m + 0.5) / M)), d = 1 .. D = n_ceps, m = 0 .. M-1 = n_mels - 1, evaluated in fp64
 *     (the cosine's argument as ((pi * d) * (m + 0.5)) / M) and rounded once: rows 1 .. D of the orthonormal DCT-II; c0 is left out.
 *     ev_score_design writes the table, ev_score_load uses the same one.
 *   2 Integer cepstra.  mel is packed as ev_features_result.mel: per signal (n_mels, T) row-major, fp32 natural-log mel.  For frame t and
 *     coefficient d: x = sum_m (double)mel[m][t] * (double)basis[d-1][m], m ascending from x = +0.0; each product is exact in fp64, each addition
 *     one fp64 rounding, no product fused with a sum.  cq[t][d-1] = clamp(llrint(x * 65536.0), -2^27, 2^27), ties to even; a non-finite x gives
 *     cq = 0.  A frame that holds a non-finite mel value counts once in nonfinite_a[b] / nonfinite_b[b].
 *   3 Local distance.  For frame i of a and frame j of b: s = sum_d (int64)(cqa[i][d] - cqb[j][d])^2 (differences below 2^28, so s < 2^61 for
 *     D <= 32: exact); dist(i, j) = the largest integer r with r * r <= s.
 *   4 DTW.  A[0][0] = dist(0, 0); A[i][j] = dist(i, j) + min(A[i-1][j-1], A[i-1][j], A[i][j-1]), cells outside the grid infinite.  Values stay
 *     below 2^44.  The predecessor of (i, j): the diagonal (i-1, j-1) if A[i-1][j-1] <= A[i-1][j] and A[i-1][j-1] <= A[i][j-1]; otherwise
 *     (i-1, j), an "a-step", if A[i-1][j] <= A[i][j-1]; otherwise (i, j-1), a "b-step".  The path runs from (Ta-1, Tb-1) back to (0, 0) and is
 *     reported ascending, K cells.  With EV_SCORE_LINEAR there is no DP: K = min(Ta, Tb), the cells are (k, k).
 *   5 Sums along the path.  sum_dist (int64) = the sum of dist over the path's cells; without EV_SCORE_LINEAR that is A[Ta-1][Tb-1].  n_diag, n_a,
 *     n_b: the step counts, K = 1 + n_diag + n_a + n_b.  With f0_hz loaded on both sides a frame is voiced iff its f0 is finite and > 0; n_vv,
 *     n_vu, n_uv, n_uu (a's state first) sum to K; over the vv cells c = 1200 * log2((double)fa / (double)fb), and sum_c, sum_c2 (of c * c) are
 *     fp64 sums from +0.0 in ascending path order.  The counts are exact; log2 is not specified bit for bit, so the two sums are specified to
 *     1e-9 relative (sum_c: 1e-9 * sum |c|).  With f0_hz NULL on either side the four counts are 0 and the sums +0.0.
 *   6 Ratios (host, C double, in the order written):
 *     mcd_db = (10 / ln 10) * sqrt(2) * ((double)sum_dist / 65536) / K
 *     f0_rmse_cents = sqrt(sum_c2 / n_vv), f0_bias_cents = sum_c / n_vv; both NaN when n_vv = 0
 *     vuv_error = (n_vu + n_uv) / K;  warp = (n_a + n_b) / K
 * No atomics, no synchronisation between blocks; every loop runs over a length the host has validated.  The distance and decision workspaces
 * together stay within EV_SCORE_WORKSPACE bytes: a batch that needs more runs in passes of whole pairs.  Every decision is an integer one, so a
 * pair gives the same bits alone or anywhere in a batch, from host or device memory, on every precision mode.  Needs no weights and no
 * ev_features_setup. */
#define EV_SCORE_MAX_FRAMES 4096     /* frames per signal (65 s at 16 kHz / 256) */
#define EV_SCORE_MAX_CEPS   32
#define EV_SCORE_Q          65536    /* cepstra are held as integers in units of 1 / 65536 nat */
#define EV_SCORE_CLAMP      (1 << 27)
#define EV_SCORE_LINEAR     0x1u     /* flag of ev_score: no warp, path (k, k), k < min(Ta, Tb) */
#define EV_SCORE_WORKSPACE  (1ll << 30)
typedef struct ev_score_result {
    uint32_t struct_size;          /* sizeof(ev_score_result), set by the caller; any other value is rejected */
    int32_t  batch;
    int32_t  n_ceps;
    int32_t  linear;               /* 1: scored with EV_SCORE_LINEAR */
    int64_t  total_frames_a;       /* lens_a[0] + .. + lens_a[batch - 1] */
    int64_t  total_frames_b;
    const int64_t* sum_dist;       /* every array: HOST, (batch,) unless stated */
    const int32_t* path_len;       /* K */
    const int32_t* n_diag;
    const int32_t* n_a;
    const int32_t* n_b;
    const int32_t* n_vv;
    const int32_t* n_vu;
    const int32_t* n_uv;
    const int32_t* n_uu;
    const double*  sum_c;
    const double*  sum_c2;
    const double*  mcd_db;
    const double*  f0_rmse_cents;
    const double*  f0_bias_cents;
    const double*  vuv_error;
    const double*  warp;
    const int32_t* lens_a;
    const int32_t* lens_b;
    const int32_t* nonfinite_a;
    const int32_t* nonfinite_b;
    const int64_t* path_offsets;   /* (batch+1,) HOST: pair b owns path entries path_offsets[b] .. path_offsets[b + 1], path_len[b] of them */
    const int32_t* path_a;         /* DEVICE, (path_offsets[batch],): the path's frames of a, ascending */
    const int32_t* path_b;         /* DEVICE, likewise for b */
    const int32_t* cq_a;           /* DEVICE, (total_frames_a, n_ceps): step 2 of side a, signal after signal */
    const int32_t* cq_b;           /* DEVICE, (total_frames_b, n_ceps) */
} ev_score_result;
/* HOST, needs no handle: basis (n_ceps, n_mels) row-major, step 1.  0, or -1 for a NULL basis, n_mels outside [1, EV_FEATURES_MAX_MELS] or n_ceps
 * outside [1, min(n_mels - 1, EV_SCORE_MAX_CEPS)]. */
int ev_score_design(int n_mels, int n_ceps, float* basis);
/* Loads side 0 (a, under test) or 1 (b, the yardstick): steps 1 and 2 of B signals and a copy of their F0 tracks.  mel as step 2 states; lens[b] frames
 * per signal, always a HOST array; f0_hz: (lens[0] + .. + lens[B - 1],) Hz as ev_pitch_result.f0_hz, or NULL.  EV_FLAG_DEVICE_INPUTS covers mel and
 * f0_hz (an ev_features_result.mel and an ev_pitch_result.f0_hz of the same batch go straight in); the other flags are ignored.  Rejected before
 * anything is launched (message naming the field or signal; the side stays as it was): a NULL h, mel or lens, side not 0 or 1, B outside [1, 65535],
 * lens[b] outside [1, EV_SCORE_MAX_FRAMES], n_mels outside [1, EV_FEATURES_MAX_MELS], n_ceps outside [1, min(n_mels - 1, EV_SCORE_MAX_CEPS)].  The
 * call synchronises; a loaded side stays loaded, across every other entry point, until it is replaced or ev_destroy. */
int ev_score_load(ev_handle* h, int side /* 0 = a (under test), 1 = b (yardstick) */, int B, int n_mels, int n_ceps,
                  const float* mel, const int32_t* lens, const float* f0_hz /* or NULL */, uint32_t flags);
/* Scores pair b = (signal b of side 0, signal b of side 1), steps 3 to 6.  flags: EV_SCORE_LINEAR or 0.  Rejected before anything is launched
 * (message naming the field or side; the previous result stays valid): a NULL h or out, a wrong struct_size, a side that is not loaded, sides that
 * differ in B, n_mels or n_ceps.  The call synchronises (as ev_compare): the HOST arrays are complete when it returns; the result, cq_a and cq_b
 * included, lives in a workspace of its own and stays valid across every other entry point, ev_score_load included, until the next ev_score or
 * ev_destroy.  A call that fails after its launches began (a HIP error) has rewritten that workspace: no result is valid after it. */
int ev_score(ev_handle* h, uint32_t flags, ev_score_result* out);
/* HOST, needs no handle: how ev_score lays a batch of pairs (lens_a[b] x lens_b[b] frames) out in passes.  A pair's distances take
 * (lens_b + 63) * rm * 64 * 4 bytes and its decisions (lens_b + 63) * max(rm / 16, 1) * 64 * 4, rm the power of two from 1 with rm * 64 >= lens_a;
 * consecutive pairs share a pass while their sum stays within EV_SCORE_WORKSPACE.  pass_of: (B,) out, the pass of every pair; pass_bytes: (B,) out,
 * its first n entries the bytes of every pass -- ev_score's workspace for distances and decisions is ONE buffer of their maximum.  Returns the
 * number of passes n, or -1 (a NULL argument, B outside [1, 65535], a length outside [1, EV_SCORE_MAX_FRAMES]). */
int ev_score_plan(int B, const int32_t* lens_a, const int32_t* lens_b, int32_t* pass_of, int64_t* pass_bytes);

/* Durations for EV_FLAG_FORCED_DURATIONS: (total_tokens,) int64 HOST pointer, copied. */
int ev_set_forced_durations(ev_handle* h, const int64_t* durations, int64_t n);

/* HiFi-GAN generator only.  mel: B tensors packed back to back, each (n_mels, mel_lens[b]) row-major
 * (the reference's (B,80,T) layout per utterance), fp32 or fp16 (mel_is_f16). mel_lens: HOST pointer. */
int ev_vocoder(ev_handle* h, int B, const void* mel, int mel_is_f16, const int32_t* mel_lens,
               uint32_t flags, ev_result* out);

/* SimBERT prompt / content encoder on the device (reference models/prompt_tts_modified/simbert.py:48-72, called twice per utterance
 * at inference_am_vocoder_joint.py:25-38,106-107 and predict.py:142-158 -- on the CPU there): BERT-base forward, the result is
 * outputs["pooled_output"] = tanh(W_pool h[CLS] + b_pool), which the callers pass as inputs_style_embedding /
 * inputs_content_embedding.  The weights are a second packed blob (emotivoice_amd/packer.py: pack_bert_state_dict, from the
 * StyleEncoder state dict); fp32-class arithmetic (split-precision GEMMs, exact-fp32 MFMA attention). */
typedef struct ev_bert_config {
    int32_t vocab_size;        /* 13685 (WangZeJun/simbert-base-chinese) */
    int32_t hidden;            /* 768  */
    int32_t layers;            /* 12   */
    int32_t heads;             /* 12 (64-wide heads) */
    int32_t intermediate;      /* 3072 */
    int32_t max_position;      /* 512  */
    int32_t type_vocab;        /* 2    */
    float   ln_eps;            /* 1e-12 */
    int32_t reserved[8];
} ev_bert_config;
void ev_default_bert_config(ev_bert_config* cfg);
int ev_style_load_weights(ev_handle* h, const ev_bert_config* cfg, const void* blob, size_t nbytes);   /* host pointer, copied */
/* B texts, token ids packed back to back (what the tokenizer returns per text: [CLS] ... [SEP]).
 *   input_ids      (cu_seqlens[B],) int64          = tokenizer(...)["input_ids"]
 *   token_type_ids (cu_seqlens[B],) int64 or NULL  = tokenizer(...)["token_type_ids"] (NULL: all 0)
 *   cu_seqlens     (B+1,) int32 HOST pointer       (attention_mask is all ones per text: each text attends to its own tokens)
 *   out            (B, hidden) fp32: host pointer, or a device pointer with EV_FLAG_DEVICE_INPUTS (then ids are device pointers too) */
int ev_style_embed(ev_handle* h, int B, const int64_t* input_ids, const int64_t* token_type_ids, const int32_t* cu_seqlens,
                   uint32_t flags, float* out);

/* Copy a named stage tap (SURVEY.md Appendix C names) of the LAST call to host memory as fp32
 * (integer taps as int64), in the packed utterance-major layout (rows x channels, valid rows only).
 * Returns the number of bytes written, or a negative error (e.g. cap too small, unknown name,
 * keep_stages disabled).  With host_dst == NULL returns the required size.  "dur" / "dur_eff" (int64, always available): the durations
 * ev_result.durations holds / the durations the length regulator used (they differ only where ev_synthesize_prosody overrides them). */
int64_t ev_get_stage(ev_handle* h, const char* name, void* host_dst, size_t cap);

/* Convenience for callers without a HIP runtime binding (numpy/ctypes): synchronous device -> host copy
 * of one of the result pointers. */
int ev_memcpy_d2h(ev_handle* h, void* host_dst, const void* dev_src, size_t nbytes);

/* Timing of the last call, measured with hipEvents on the handle's stream (ms).  Names: "total",
 * "am", "encoder", "variance", "decoder", "vocoder".  Enabled by ev_set_profiling(h, 1). */
int ev_set_profiling(ev_handle* h, int enable);
int ev_get_timing(ev_handle* h, const char* name, float* ms);

/* Per-kernel-family accounting of the last call (profiling enabled): number of launches, summed
 * hipEvent duration and algorithmic FLOPs / bytes.  idx in [0, ev_kernel_stat_count). */
typedef struct ev_kernel_stat {
    char name[48];
    int32_t launches;
    float ms;
    double flops;
    double bytes;
} ev_kernel_stat;
int ev_kernel_stat_count(ev_handle* h);
int ev_get_kernel_stat(ev_handle* h, int idx, ev_kernel_stat* out);

/* Per-LAUNCH records of the last profiled call, in launch order: kernel family, the GEMM / conv shape (M rows, N output channels,
 * K input channels, taps, dilation; 0 for non-GEMM kernels), hipEvent duration and algorithmic FLOPs / bytes.  Lets a reader
 * recompute TF/s and TB/s per layer (profiles/ r2_*_launches.json). */
typedef struct ev_launch_record {
    char name[48];
    int32_t M, N, K, taps, dil;
    float ms;
    double flops;
    double bytes;
} ev_launch_record;
int ev_launch_record_count(ev_handle* h);
int ev_get_launch_record(ev_handle* h, int idx, ev_launch_record* out);

#ifdef __cplusplus
}
#endif
#endif /* EVHIP_H_ */
