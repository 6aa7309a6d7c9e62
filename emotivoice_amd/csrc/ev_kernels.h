// Internal launcher interface between the host code (ev_engine.cpp, ev_audio.cpp, ev_ops.cpp) and the gfx950 kernels.
// Not part of the public ABI (that is include/evhip.h); the ev_op_* C wrappers in
// include/evhip_ops.h expose these launchers to the per-kernel parity tests.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

#include <vector>

namespace ev {

// A/B switches of the kernel launchers (EV_GEMM_TILE, EV_ATTN_X3_NW, ...: tools/bench_*.py) exist only in tuning builds
// (`build.py --variant tune EV_TUNING`, loaded through EVHIP_LIB): the product library reads no environment variable; what an
// integrator may choose is an ev_config field.
#ifdef EV_TUNING
inline const char* tuning_env(const char* name) { return getenv(name); }
#else
inline const char* tuning_env(const char*) { return nullptr; }
#endif

enum Act { ACT_NONE = 0, ACT_RELU = 1, ACT_GELU = 2, ACT_LRELU = 3, ACT_TANH = 4 };
enum DType { DT_F16 = 0, DT_F32 = 1, DT_F32S = 2, DT_MX = 3 };   // F32S: fp32 activations, fp16 hi/lo split weights (ConvGemmParams::W / W_lo)
                                                                  // MX: fp32 activations; hi.hi as one fp16 MFMA + the two cross terms as block-scaled fp4 MFMAs (W, W_lo, W_mx)

// out[m, n] = post( scale * ( act( sum_{tap,k} pro(A[m + (tap-center)*dil, k]) * W[n][tap][k] + bias[n] )
//                              + seq_bias[row_seq[m]][n] + res[m, n] ) + acc32[m, n] + add16_a[m, n] + add16_b[m, n] )
// rows with row_valid[m >> valid_shift] == 0 are written as exact zeros.
// Channels-last activations ([rows][channels]); the conv over time is an implicit GEMM whose
// M dimension is time.  Reference ops covered: nn.Linear, Conv1d (any k / dilation, "same" pad),
// ConvTranspose1d(k = 2*stride, pad = stride/2) as a 3-tap conv with N = stride*C_out.
struct ConvGemmParams {
    int dtype;              // DT_F16: A/W fp16, MFMA f32_16x16x32_f16; DT_F32: A/W fp32, MFMA f32_16x16x4_f32 (exact fp32)
    const void* A; int lda; // activations, row pitch in elements; rows [-64, M+64) must be readable
    const void* W;          // [N][taps][K], K contiguous (DT_F32S: fp16 "hi" part)
    const void* W_lo;       // DT_F32S only: fp16((w - hi) * 2048), same layout
    const float* bias;      // [N] or null
    int M, N, K, taps, dil, center;
    const uint8_t* row_valid; int valid_shift;   // null -> all rows valid
    const int32_t* row_seq; const float* seq_bias; int ld_seq_bias;   // per-utterance additive vector, or null
    int act; float act_slope;
    int pro_lrelu; float pro_slope;              // leaky-relu applied to A while staging
    const void* res; int res_dtype; int ldres;   // residual (fp16 or fp32) or null
    float out_scale;
    const float* acc32; int ldacc;               // fp32 accumulate-in (after scaling) or null
    int post_lrelu; float post_slope;
    void* out16; float* out32; int ldo;          // either / both outputs
    int out32_before_post;                       // out32 receives the value BEFORE post_lrelu (stage taps)
    int reserved0;                               // (was: ablation switches used while tuning)
    const void* add16_a; const void* add16_b; int ldadd;   // two fp16 tensors added after scaling (the MRF sum of three ResBlocks
                                                 // with the first two branches kept in fp16: half the traffic of acc32), or null
    int ksplit;                                  // DT_F32S, N % 64 == 0, no add16: > 1 = split-K.  The K / 32 chunks are cut into `ksplit` equal ranges (K / 32 must be a
                                                 // multiple), each (tile, range) is a block of the 128 x 64-tile kernel writing fp32 partial sums to mx_scratch
                                                 // (>= ksplit * M * N * 4 bytes), and a second kernel adds them in range order and applies the epilogue.  Shortens the
                                                 // sequential step chain of the token-rate GEMMs (few tiles, K * taps up to 4608).  The summation order differs from
                                                 // ksplit <= 1, so a caller that promises batch invariance picks it by layer shape, never by M.
    // DT_MX only.  W_mx: the weight's fp4 planes (emotivoice_amd/mxfp4.py: pack_weight_planes), null -> the call runs as DT_F32S.
    // Activations, either (a) A = fp32 [M][K] + mx_scratch (>= mx_scratch_bytes(M, K) bytes): the launcher first runs mx_planes_kernel
    // (leaky-relu of pro_lrelu, then the planes) into the scratch, or (b) a plane set written by the producer's epilogue (mxo below):
    // A = the fp16 hi plane (lda == K), mx_x4 / mx_xs / mx_xs_stride = its code and scale planes; pro_lrelu must be 0.
    // polyphase_cout > 0 (DT_MX, taps == 3, conv_gemm_mx_kernel launches): the call is a ConvTranspose1d(k = 2 s, stride s, pad s / 2) run as a 3-tap conv with
    // N = s * polyphase_cout (packer._convT_to_gemm): output phase n / polyphase_cout < s / 2 has an all-zero tap 2, the other phases an all-zero tap 0, and the kernel
    // skips that tap's matrix instructions (a third of the launch's).  0: every tap is multiplied.  The weights' zero tap must really be zero.
    const void* W_mx; void* mx_scratch; size_t mx_scratch_size;
    const void* mx_x4[2]; const void* mx_xs[2]; unsigned mx_xs_stride; int polyphase_cout;
    // Plane-set OUTPUT (any dtype whose launch takes an EPI_MXP epilogue: DT_MX kernels): besides / instead of out32 the epilogue writes
    // the planes of a = lrelu(result, mxo_slope) (slope 1 = none) viewed as [rows][C], C = 2^mxo_logC, or C = N when mxo_logC == 0
    // (ldo == N; a transposed conv's [M][s * C] output is the [M * s][C] tensor): mxo_h fp16(a); mxo_q4[0] / [1] fp4 codes of fp16(a) and of a - fp16(a), C / 2 bytes
    // per row; mxo_qs[0] / [1] their E8M0 block scales, one byte per 32 channels, chunk-major [C / 128][mxo_qs_stride / 4 rows][4].
    // Invalid rows give all-zero planes.  Every plane needs 64 readable slack rows on both sides for its consumer.
    void* mxo_h; void* mxo_q4[2]; void* mxo_qs[2]; unsigned mxo_qs_stride; int mxo_logC; float mxo_slope; int reserved3;
    // Residual from a plane set (res_dtype == DT_MX; DT_MX launches only): the residual x of the launch's [M][N] output is not an fp32 tensor but the
    // plane set of a = lrelu(x, 1 / res_inv_slope) that conv1 of the pair read as its operand: res = its fp16 hi plane ([M][N], ldres == N), res_x4 = the
    // fp4 codes of the remainder a - fp16(a) ([M][N / 2]), res_xs their E8M0 scales (chunk-major [N / 128][res_xs_stride / 4 rows][4], as mx_xs);
    // the epilogue rebuilds x = a' >= 0 ? a' : a' * res_inv_slope, a' = hi + code * scale.  tools/precision_study_mx.py: the generator's waveform error
    // goes from 3.4e-4 to 4.4e-4 on the zero-mean recipe, and a conv2 launch moves 8.7 instead of 14.1 bytes per element.
    const void* res_x4; const void* res_xs; unsigned res_xs_stride; float res_inv_slope;
    // Accumulate-in from a PARTIAL plane set (conv_gemm_mx_kernel launches with a plane-set residual; excludes acc32): the addend is acc_h (fp16 hi plane,
    // [M][N], ldacc == N) + acc_x4 (fp4 codes of the remainder, [M][N / 2]) * acc_xs (their E8M0 scales, chunk-major [N / 128][acc_xs_stride / 4 rows][4]) --
    // a plane set without the hi-code plane and without an activation: 2.53 bytes per element instead of acc32's 4.  mxo_partial != 0: the OUTPUT plane set is
    // such a partial one (mxo_h, mxo_q4[1], mxo_qs[1]; mxo_q4[0] / mxo_qs[0] unused; mxo_slope must be 1); it may alias the acc_* planes (same rows, same
    // columns: each element is read before it is rewritten by the same lane).  The MRF running sum of a generator stage travels like this.
    const void* acc_h; const void* acc_x4; const void* acc_xs; unsigned acc_xs_stride; int mxo_partial;
};
// bytes of activation-plane scratch a DT_MX call with an [M][K] input needs
size_t mx_scratch_bytes(int M, int K);
// 0 if the plane-set fields of a call are consistent with its dtype, shape and epilogue (launch_conv_gemm would run it)
int mx_check(const ConvGemmParams& p);
// 0 if ConvGemmParams::ksplit is consistent with the rest of the call (<= 1, or a DT_F32S call whose shape and scratch allow the split)
int splitk_check(const ConvGemmParams& p);
void launch_conv_gemm(const ConvGemmParams& p, hipStream_t s);
// Three independent DT_MX convs of the conv_gemm_mx_kernel family (same M, N, K and epilogue form, taps {3, 7, 11}, plane sets in) as ONE grid -- the same-level
// convs of a generator stage's three ResBlocks; 0 = launched (check_only: would be), -1 = not such a triple (launch them one by one: the results are the same bits)
int launch_conv_gemm_group3(const ConvGemmParams* ps, hipStream_t s, bool check_only = false);
// which kernel launch_conv_gemm runs a DT_MX call on: 0 = the split-precision fallback (three fp16 MFMAs per product), 1 = conv_gemm_mx_kernel,
// 2 = conv_c64_mx_kernel (profiling records name the launch by this, not by what the caller hoped for)
int mx_launch_kind(const ConvGemmParams& p);
// per-device setup of the kernels in ev_gemm.hip (large-LDS opt-in, CU count of the persistent kernels); 0 = OK
int init_device_kernels(int device);

// Fused HiFi-GAN ResBlock1 pair for C = 32 (reference models/hifigan/models.py:50-57, one iteration of the zip loop):
//     xt = leaky_relu(c1(leaky_relu(x, .1)) + b1, .1);   out = epilogue(c2(xt) + b2 + x)
// c1 = Conv1d(C, C, k, dilation d), c2 = Conv1d(C, C, k, dilation 1).  Persistent blocks, both weight sets stationary in LDS,
// the intermediate xt never leaves LDS.  `epi` carries the c2 epilogue in ConvGemmParams form (bias = b2, res = x,
// out_scale / acc32 / post_lrelu / out16 / out32 / row_valid as for launch_conv_gemm); its GEMM fields are ignored.
struct ResPairParams {
    const void* x; int ldx;             // [rows][32] fp16 residual stream; rows [-64, M+64) readable
    const void* w1; const float* b1;    // [32][k][32] fp16
    const void* w2;
    int M, k, dil;
    int gmin, gmax;                     // rows g of x (relative to the x pointer) that exist in the tensor: gmin <= g < gmax.  {0, M} for a
                                        // whole tensor; a launch on a row sub-range (chunked execution) passes the tensor's real bounds so
                                        // that only true sequence edges are zero-padded.  gmax == 0 means {0, M}.
    const void* w1_mx; const void* w2_mx;   // launch_resblock_pair_c32_mx only: the convs' fp4 planes (mxfp4.py: pack_pair_weight_planes)
    ConvGemmParams epi;
};
void launch_resblock_pair_c32(const ResPairParams& p, hipStream_t s);
// the same pair in the MX arithmetic (ev_pair_mx.h): x / epi.res fp32 [rows][32], w1 / w2 the fp16 hi parts, w1_mx / w2_mx the fp4 planes;
// epilogue: bias, fp32 residual (= x), out_scale, optional acc32, row mask, out32 only.  Returns 0, or -1 for an unsupported call.
int launch_resblock_pair_c32_mx(const ResPairParams& p, hipStream_t s);
// the pair at C = 64, k = 3 in the MX arithmetic, plane sets in / out (ev_pair64_mx.h): x = the fp16 hi plane of the input plane set (ldx == 64), epi.mx_x4 /
// mx_xs its code / scale planes, w1 / w2 fp16 hi parts, w1_mx / w2_mx = mxfp4.pack_c64_weight_planes; the residual is rebuilt from the input plane set
// (epi.res_inv_slope); outputs epi.out32 and / or the plane set epi.mxo_*.  Returns 0, or -1 for an unsupported call.
int launch_resblock_pair_c64_mx(const ResPairParams& p, hipStream_t s);
// same pair at C = 64 (stage 2), k = 3 only: both weight sets (48 KB) stationary in LDS, x as two 64-byte K-chunk planes
// dil <= PAIR64_MAX_DIL: the slab of a tile has 272 rows, conv1's 256 output rows read rows up to 255 + 2 dil (callers check: nothing is launched beyond it)
constexpr int PAIR64_MAX_DIL = 8;
void launch_resblock_pair_c64(const ResPairParams& p, hipStream_t s);

// LayerNorm over the channel dim (eps 1e-12, reference modules/encoder.py:112-127), fp32 in.
// out16/out32 optional; if dot_w != null additionally dot_out[r] = <LN(x[r]), dot_w> + dot_b.
struct LayerNormParams {
    const float* x; int ldx; int rows; int C;
    const float* gamma; const float* beta; float eps;
    const uint8_t* row_valid;
    void* out16; float* out32; int ldo;
    const float* dot_w; float dot_b; float* dot_out;
    // optional (C <= 512): the MX plane set of the output as a DT_MX consumer reads it (ConvGemmParams::mx_x4 ...): fp16 hi plane [rows][C], fp4 code
    // planes of the hi / lo parts [rows][C / 2], their E8M0 scale planes [C / 128][mxo_qs_stride / 4 rows][4]; mxo_h == null: none
    void* mxo_h; void* mxo_q4[2]; void* mxo_qs[2]; unsigned mxo_qs_stride;
};
// where a DT_MX call with an fp32 [M][K] input lays that input's plane set inside its mx_scratch (what launch_conv_gemm's own mx_planes_kernel pass fills):
// a producer that writes these planes itself passes them as ConvGemmParams::A (= h, lda = K) / mx_x4 / mx_xs / mx_xs_stride instead of the fp32 tensor
struct MxScratchPlanes { void* h; void* q4[2]; void* qs[2]; unsigned qs_stride; };
MxScratchPlanes mx_scratch_planes(void* scratch, int M, int K);
void launch_layernorm(const LayerNormParams& p, hipStream_t s);

// token embedding gather + alpha * PE[pos] (reference model_open_source.py:107, encoder.py:257-261)
void launch_embed_pe(const int64_t* ling_packed, const int32_t* cu_seqlens_dev, const int32_t* row_seq /* -1 = gap */,
                     const int32_t* row_pos, const float* emb, int n_vocab, const float* pe, float alpha, float* out, float* tap_out,
                     int rows, int C, hipStream_t s);

// Self-attention, one (utterance, head, 64-query tile) per wave; fp32 math, online softmax.
// qkv: [rows][3*C] (fp16 or fp32) with q | k | v column blocks; out: [rows][C].
struct AttnParams {
    const void* qkv; int dtype; int ld; int C; int heads;
    const int32_t* seq_off; const int32_t* seq_len; int B; int max_len;
    void* out; int ldo;     // same dtype as qkv
};
void launch_attention(const AttnParams& p, hipStream_t s);

// SimBERT (BERT-base) embeddings: out[row] = word[ids] + type[type_ids] + pos[position] (transformers BertEmbeddings; the LayerNorm that
// follows is launch_layernorm); pooler: out[b] = tanh(W x[first row of text b] + bias) (BertPooler).  reference
// models/prompt_tts_modified/simbert.py:37,49-55.
void launch_bert_embed(const int64_t* ids, const int64_t* type_ids /* or null = 0 */, const int32_t* cu_seqlens_dev, const int32_t* row_seq,
                       const int32_t* row_pos, const float* word, const float* pos_emb, const float* type_emb, int vocab, int max_pos,
                       int n_types, float* out, int rows, int C, hipStream_t s);
void launch_bert_pooler(const float* x, int ldx, const int32_t* seq_off, const float* W, const float* bias, float* out, int B, int C,
                        hipStream_t s);

// u[b, :] = bias + Wspk . spk_emb[speaker[b]] + Wsty . style[b] + Wcon . content[b]
// (columns 384..2303 of embed_projection1, reference model_open_source.py:110-111)
void launch_cond_vector(const int64_t* speaker, const float* style, const float* content, const float* spk_emb, int n_speaker,
                        const float* Wcond /* [C][C + 2*bert] */, const float* bias, float* u, int B, int C, int bert,
                        hipStream_t s);

// x_var = x_proj + pitch_embed(pitch) + energy_embed(energy)   (Conv1d 1->C, k taps, zero pad; :131-134)
void launch_var_embed_add(const float* x, const float* pitch, const float* energy, const float* wp, const float* bp,
                          const float* we, const float* be, const uint8_t* row_valid, float* out, int rows, int C, int k,
                          hipStream_t s);

// durations: d = max(rint(exp(log_d) - 1), 0) (variance.py:47-51); all-zero guard, cumsum, centres
// (alignment.py:183-202).  One block per utterance, wavefront prefix sum.
void launch_durations(const float* log_d /* token rows */, const int32_t* tok_off, const int32_t* tok_len, int B,
                      float alpha, const int64_t* forced /* packed or null */, const int32_t* cu_seqlens_dev,
                      int64_t* dur_packed, float* logd_packed, float* centre_rows, int32_t* mel_len, hipStream_t s);
// ev_synthesize_prosody: the same, with per-utterance duration scales alpha_b (B,) (NULL = alpha) and per-token overrides partial
// (packed, >= 0 forced and clamped to dur_cap, negative = predicted; NULL = all predicted).  dur_packed keeps the predictions, dur_eff
// receives the durations that are scanned.
void launch_durations_prosody(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const float* alpha_b,
                              const int64_t* partial, int64_t dur_cap, const int32_t* cu_seqlens_dev, int64_t* dur_packed, int64_t* dur_eff,
                              float* logd_packed, float* centre_rows, int32_t* mel_len, hipStream_t s);

// ev_synthesize_prosody: effective pitch / energy token rows = per-utterance affine transform of (override if finite, else prediction);
// ctrl is SoA [5][B] (alpha, pitch_scale, pitch_shift, energy_scale, energy_shift); gap rows = 0.
void launch_prosody_tracks(const float* pitch, const float* energy, const int32_t* row_seq, const int32_t* row_pos, const int32_t* cu_seqlens_dev,
                           const float* pitch_ovr /* packed or null */, const float* energy_ovr /* packed or null */, const float* ctrl, int B,
                           float* pitch_out, float* energy_out, int rows, hipStream_t s);

// Gaussian upsampling (alignment.py:204-210) + decoder positional encoding (encoder.py:257-261).
void launch_gauss_upsample(const float* xvar, const float* centre_rows, const int32_t* tok_off, const int32_t* tok_len,
                           const int32_t* frm_row_seq, const int32_t* frm_row_pos, const float* pe, float pe_alpha,
                           float delta, float* out, float* tap_out, int rows, int C, hipStream_t s);

// mel (B x (n_mels, T_b), fp32/fp16) -> channels-last fp16 [rows][ldo] with zero gaps and zero pad channels
void launch_mel_to_rows(const void* mel, int is_f16, const int64_t* mel_elem_off, const int32_t* frm_row_seq,
                        const int32_t* frm_row_pos, const int32_t* mel_len, void* out, int out_f32, int rows, int n_mels, int ldo,
                        hipStream_t s);

// conv_post: input [rows][C] -> Conv1d(C->1, k) -> tanh -> wav fp32.  fp16 input: already leaky-relu'd by its producer;
// fp32 input (split-precision mode): raw MRF mean, leaky_relu(pre_slope) applied while reading (pre_slope in [0, 1])
void launch_conv_post(const void* x, int is_f32, int ldx, const float* w /* [k][C] */, float bias, int k, float pre_slope,
                      const uint8_t* row_valid, int valid_shift, float* wav_rows, int rows, int C, hipStream_t s);

// gather valid rows of a [rows][ld] buffer (fp16 or fp32) into a packed fp32 [n_valid][C] host-visible buffer
void launch_pack_rows(const void* src, int dtype, int ld, int C, const int64_t* seq_row_off /* per utterance first row */,
                      const int64_t* seq_out_off /* per utterance packed offset (rows) */, const int32_t* seq_rows, int B,
                      int64_t max_rows, float* dst, hipStream_t s);

// rows [row0, row1) of the sinusoid table: pe[t][2i] = sin(t * div[i]), pe[t][2i+1] = cos(t * div[i]) (encoder.py:216-237,
// which auto-extends its table the same way for inputs longer than max_len)
void launch_pe_extend(float* pe, const float* div, int row0, int row1, int C, hipStream_t s);
void launch_wav_to_i16(const float* wav, int16_t* out, int64_t n, hipStream_t s);
// gap-layout row maps on the device: seq[r] = utterance of row r (-1 in gaps), pos[r] = position inside it, valid[r]
void launch_row_maps(const int32_t* off, const int32_t* len, int B, int32_t* seq, int32_t* pos, uint8_t* valid, int rows, hipStream_t s);
void launch_fill_zero(void* p, size_t bytes, hipStream_t s);

// ev_align (ev_align.hip).  Per utterance: its rows in the token / frame layouts, its sizes and its offsets into the packed outputs.
#define EV_ALIGN_MAX_TOKENS 2048
#define EV_ALIGN_MAX_FRAMES 16384
struct AlignSeq {
    int32_t tok_row, tokens, frm_row, frames;   // first row in the token / frame layout, N, T
    int64_t lp_off;                             // element offset of the (T, N) log_p block
    int64_t tok_packed, frm_packed;             // packed token / frame offsets (cu_seqlens[b], mel_offsets[b])
    int64_t bits_off;                           // word offset of the (T, 64) decision words
};
// log_p[t, n] = log_softmax_n(-||feats[t] - text[n]||_2) + log betabinom.pmf(n; N, t + 1, T - t): text / feats are the aligner's fp32 row
// layouts ([rows][C]); one block per (64 frames, utterance)
void launch_align_score(const float* text, const float* feats, int C, const AlignSeq* seqs, int B, int max_frames, float* log_p, hipStream_t s);
// monotonic alignment search + durations, per-token means of the optional frame tracks and the mean log_p along the path; one wave per
// utterance.  bits: sum_b frames_b * 64 words of scratch
void launch_align_mas(const float* log_p, const AlignSeq* seqs, int B, int max_tokens, uint32_t* bits, const float* pitch_frames,
                      const float* energy_frames, int64_t* dur, float* pitch_tok, float* energy_tok, float* score, hipStream_t s);

// ev_features (ev_features.hip): wav -> log-mel and frame energy.  Limits of the kernel: n_fft a multiple of 128 up to STFT_MAX_NFFT, hop a multiple
// of 8 up to n_fft, n_mels <= STFT_MAX_MELS, and the 63 hop + n_fft samples of a 64-frame tile within STFT_MAX_RUN (they stay in LDS).
constexpr int STFT_MAX_NFFT = 2048, STFT_MAX_MELS = 128, STFT_MAX_RUN = 24576;
struct StftSeq { int64_t wav_off, len, frm_off; int32_t frames, reserved; };   // sample offset / length of the utterance, its packed frame offset, T
struct StftTile { int32_t seq, t0; };                                           // one block: utterance and first frame
// Layout facts of the windowed-DFT kernels, each stated once for host and device.  A block multiplies STFT_TF frames by basis tiles of STFT_TB bins
// (64 GEMM columns: re and im of the same bins); the frames are ONE run of samples, kept in LDS as two fp16 planes.
constexpr int STFT_TF = 64, STFT_TB = 32;
// LDS index of sample i of the block's run: 8 halfs of padding after every 256 samples, so that the 16 frames of an A fragment (hop apart:
// 512 bytes at hop 256) start 16 bytes apart modulo the bank width.  A fragment's 8 samples start at a multiple of 8 and never straddle a pad.
constexpr int stft_spad(int i) { return i + 8 * (i >> 8); }
constexpr int stft_run_samples(int n_fft, int hop) { return (STFT_TF - 1) * hop + n_fft; }                  // the samples a block stages
constexpr int stft_plane_halfs(int n_fft, int hop) { return stft_spad(stft_run_samples(n_fft, hop)) + 8; }   // one plane
constexpr int stft_bin_tiles(int n_fft) { return (n_fft / 2 + 1 + STFT_TB - 1) / STFT_TB; }
constexpr int stft_mels_per_group(int n_mels) { return (n_mels + 3) / 4; }
constexpr int denoise_k_pad(int n_fft) { return (2 * (n_fft / 2 + 1) + 31) / 32 * 32; }                      // the width of a scratch row (ev_denoise, below)

// What every forward kernel takes, the first member of its parameters.  n_fft and n_btiles reach the kernels as RUNTIME values, at the watermark's
// fixed shape too: with constants the compiler unrolls the GEMM's k loop whole and spills.
struct StftFront {
    const void* wav; int wav_is_i16;                  // utterances back to back, fp32 or int16 (x / 32768)
    const StftSeq* seqs; const StftTile* tiles; int n_tiles;
    const void* basis;                                // stft_pack_basis, on the device
    int n_fft, hop, n_btiles;                         // n_btiles = stft_bin_tiles
};
struct StftParams {
    StftFront f;
    const float* melT;                                // stft_pack_mel, on the device
    int n_mels;
    float mel_clip, energy_floor, energy_mean, energy_std;
    float* mel;                                       // per utterance (n_mels, T) row-major at frm_off * n_mels: log(max(mel_basis @ mag, mel_clip))
    float* energy;                                    // (total_frames,): (sqrt(max(sum_k mag^2, energy_floor)) - energy_mean) / energy_std
    float* mag;                                       // (total_frames, n_bins) or null
};
int stft_shape_ok(int n_fft, int hop, int n_mels);
size_t stft_basis_halfs(int n_fft);
size_t stft_melT_floats(int n_fft);
// the window of the three packers in float64: window (host, n_fft), or the periodic hann for null.  The bases multiply by its float32 rounding, the
// envelope squares it as it is.
std::vector<double> host_window(int n_fft, const float* window);
void stft_pack_basis(int n_fft, const float* window /* host (n_fft,) or null = periodic hann */, uint16_t* out /* host, stft_basis_halfs */);
void stft_pack_mel(int n_fft, int n_mels, const float* mel_basis /* host (n_mels, n_bins) */, float* out /* host, stft_melT_floats */);
int launch_stft_mel(const StftParams& p, hipStream_t s);      // 0, or -1 for a shape the kernel does not build

// ev_denoise (ev_denoise.hip): wav -> STFT -> gain per cell -> inverse STFT.  The two kernels meet in a scratch of fp16 hi / lo planes
// (x = hi + 2^-11 lo), [total_frames][k_pad]: column 2 k is g Re, 2 k + 1 is g Im of bin k, k_pad = denoise_k_pad = 2 n_bins rounded up to 32 with
// zero padding columns.  Utterances and forward tiles are the StftSeq / StftTile of ev_features.  Limits: stft_shape_ok, n_fft % hop == 0 and
// R = n_fft / hop <= DN_MAX_R.
constexpr int DN_MAX_R = 8, DN_TJ = 64, DN_TN = 128;      // chunks (of hop output samples) and output columns per block of the inverse
struct StftGainParams {
    StftFront f;
    const float* bias;                                // (n_bins,) device
    const float* strengths;                           // (B,) device
    uint16_t *spec_hi, *spec_lo;                      // the scratch planes; frame t of an utterance is row frm_off + t
    float* mag; int mag_frames;                       // not null: the other mode -- fp32 magnitudes (row frm_off + t, n_bins columns) of frames t < mag_frames
};
struct IstftSeq { int64_t frm_off, out_off, out_len; int32_t frames, reserved; };      // first scratch row, first output sample, hop (frames - 1), T
struct IstftParams {
    const uint16_t *spec_hi, *spec_lo;
    const IstftSeq* seqs; const StftTile* tiles; int n_tiles;      // a tile: utterance and first chunk j0 (chunk j = untrimmed samples hop j .. hop j + hop)
    const void* ibasis;                               // istft_pack_basis, on the device
    const float* env;                                 // istft_pack_envelope, on the device
    int n_fft, hop, R, k_pad;
    float* out; int16_t* out_i16;                     // packed at out_off; out_i16 may be null
};
int denoise_shape_ok(int n_fft, int hop);
size_t istft_basis_halfs(int n_fft, int hop);
size_t istft_envelope_floats(int n_fft, int hop);
// Inverse basis planes.  Row q k_pad + 2 k + part (q = 0 .. R - 1: the frame j - R + 1 + q of chunk j), column n: float32(c_k cos / -c_k sin(2 pi k m / n_fft))
// * window[m] at m = (R - 1 - q) hop + n, c_k = 1 for k = 0 and n_fft / 2, else 2; zero in the padding rows and columns.
// Order: [16-column tile][k step of 32][hi, lo][lane][8]: lane l holds rows 32 step + 8 (l >> 4) + j of column (l & 15).
void istft_pack_basis(int n_fft, int hop, const float* window /* host (n_fft,) or null = periodic hann */, uint16_t* out /* host, istft_basis_halfs */);
// env[(qa R + qb) hop + n]: the float32 window-sum envelope at phase n of a chunk that the frames q = qa .. qb reach, summed in ascending q as the
// reference's window_sumsquare sums it (float32 accumulator, float64 squares); 0 for qa > qb
void istft_pack_envelope(int n_fft, int hop, const float* window, float* out /* host, istft_envelope_floats */);
int launch_stft_gain(const StftGainParams& p, hipStream_t s);      // 0, or -1 for a shape the kernel does not build
int launch_istft_ola(const IstftParams& p, hipStream_t s);

// ev_watermark / ev_watermark_detect (ev_watermark.hip), on ev_denoise's shapes at n_fft = WM_NFFT, hop = WM_HOP.  Embed: ev_denoise's forward
// GEMM with the gain of a chip's sign, into the same scratch planes, then launch_istft_ola unchanged.  Detect: the forward GEMM again with a band
// epilogue -- q[frame][WM_BANDS] int32, the quantised log2 of the floored band energies -- then wm_correlate_kernel, one block per segment.
constexpr int WM_NFFT = 1024, WM_HOP = 256, WM_BAND0 = 20, WM_BAND_BINS = 4, WM_BANDS = 48, WM_TILE = 8, WM_PERIOD = 16, WM_CHIPS = WM_PERIOD * WM_BANDS,
              WM_MAX_BITS = 16, WM_OFFSETS = WM_TILE * WM_PERIOD, WM_PILOT = 255;
struct WmEmbedParams {
    StftFront f;                                      // at n_fft = WM_NFFT, hop = WM_HOP
    const int8_t* signs;                              // (B, WM_CHIPS) device: watermark_pattern of the segment's key, payload and length
    const float* gains;                               // (B, 2) device: a and float32(1 / a) of the segment
    uint16_t *spec_hi, *spec_lo;                      // ev_denoise's scratch planes
};
struct WmBandParams {
    StftFront f;                                      // as WmEmbedParams has it
    int32_t* q;                                       // (total frames, WM_BANDS) device; frame t of a segment is row frm_off + t
};
struct WmFig { int32_t offset, C, n, pad; int32_t bit_C[WM_MAX_BITS], bit_n[WM_MAX_BITS]; };
// chip i = WM_BANDS u + v: h = dl_mix(key, i), sign (h & 1) ? +1 : -1, role (h >> 1) % (2 nbits); a role < nbits is that payload bit (the sign is
// flipped where the bit of `payload` is 1), every other role -- and every chip at nbits == 0 -- is WM_PILOT.  roles may be null.
void watermark_pattern(uint32_t key, int nbits, uint32_t payload, int8_t* signs /* host, WM_CHIPS */, uint8_t* roles /* host, WM_CHIPS, or null */);
int launch_wm_embed(const WmEmbedParams& p, hipStream_t s);      // 0, or -1 for an empty grid
int launch_wm_bands(const WmBandParams& p, hipStream_t s);
// q as wm_bands wrote it; win: device scratch (total frames, WM_BANDS) int32; tabs: device 3 x WM_CHIPS bytes -- the pilot chips (sign, or 0 for a
// payload chip), every chip's sign with payload 0, every chip's role; figs: device (B,)
int launch_wm_correlate(const int32_t* q, int32_t* win, const StftSeq* seqs, int B, const int8_t* tabs, WmFig* figs, hipStream_t s);

// ev_pitch (ev_pitch.hip): wav -> per-frame F0 (YIN), then the continuous fill and the standardisation.  The utterance and tile tables are the
// StftSeq / StftTile of ev_features, with tiles of PITCH_TF frames.  Limits of the kernel: win <= PITCH_MAX_WIN, 1 <= hop <= win, 4 <= tau_min <
// tau_max, tau_max + 1 <= win, and the tile's LDS (pitch_lds_bytes: its run of samples and three numbers per (frame, lag)) within PITCH_MAX_LDS.
constexpr int PITCH_TF = 8, PITCH_MAX_WIN = 2048, PITCH_MAX_LDS = 65536;
struct PitchParams {
    const void* wav; int wav_is_i16;                  // utterances back to back, fp32 or int16 (x / 32768)
    const StftSeq* seqs; const StftTile* tiles; int n_tiles;
    int sample_rate, hop, win, tau_min, tau_max;
    float threshold; double e0_floor;                 // win * silence_rms^2
    float* f0;                                        // (total_frames,): Hz, 0 = unvoiced
    float* ap;                                        // (total_frames,): d' at the chosen lag, 1 = unvoiced
    int32_t* tau;                                     // (total_frames,) or null: the chosen lag, -1 = unvoiced
};
int pitch_run_samples(int hop, int win, int tau_max);
size_t pitch_lds_bytes(int hop, int win, int tau_max);
int pitch_shape_ok(int hop, int win, int tau_min, int tau_max);
int launch_pitch_yin(const PitchParams& p, hipStream_t s);      // 0, or -1 for a shape the kernel does not build
// out[t] = (cont[t] - mean) / stdv, cont = f0 with unvoiced frames held at the edges and interpolated between voiced neighbours; out != f0
void launch_pitch_fill(const float* f0, const StftSeq* seqs, int B, float mean, float stdv, float* out, hipStream_t s);

// ev_resample (ev_resample.hip): polyphase sample-rate conversion, then the silence trim.  A tile is RS_TM consecutive outputs of one utterance.  The
// taps go in as a phase-major table (resample_pack_table): row p = (m down) mod up holds h[i], i = p (mod up), from the largest i <= half downwards,
// zero-filled to resample_row_len (odd).  A tile's run of inputs stays in LDS up to POLY_MAX_RUN_BYTES, the table beside it up to POLY_MAX_LDS in all
// (polyphase_lds: ev_deliver's kernel takes the same decision with its own tile).
constexpr int RS_TM = 256, POLY_MAX_RUN_BYTES = 49152, POLY_MAX_LDS = 65536;
struct ResampleSeq { int64_t in_off, len, out_off, n; };      // input offset / length, output offset / length n = ceil(len up / down)
struct ResampleTile { int32_t seq, m0; };                     // one block: utterance and first output
struct TrimSeq { int64_t src_off, dst_off, cut; };            // the cut y[src_off .. src_off + cut) goes to out[dst_off + pad ..)
struct ResampleParams {
    const void* wav; int wav_is_i16;                  // utterances back to back, fp32 or int16 (x / 32768)
    const ResampleSeq* seqs; const ResampleTile* tiles; int n_tiles;
    int up, down, half, row;                          // row = resample_row_len(up, half)
    const float* tab;                                 // (up, row) on the device
    float* out;                                       // packed at out_off
    int run_cap;                                      // set by the launcher: floats of LDS for the run, 0 = read through L1
};
int resample_row_len(int up, int half);
size_t resample_table_floats(int up, int half);
void resample_pack_table(int up, int half, const float* taps /* host (2 half + 1,) */, float* out /* host, resample_table_floats */);
int64_t polyphase_run_max(int tile, int up, int down, int half);      // an upper bound of the run of input samples under a tile of `tile` outputs
// Where a tile's run and the table go.  padded: the run keeps one unused float after every 32 (ev_deliver at down >= 2 up).
struct PolyphaseLds { bool run_lds, tab_lds; int run_cap; size_t bytes; };      // run_cap: floats of LDS for the run, 0 = read through L1; bytes: dynamic LDS
PolyphaseLds polyphase_lds(int tile, int up, int down, int half, bool padded);
int launch_resample_poly(const ResampleParams& p, hipStream_t s);      // 0, or -1 for bad parameters
void launch_resample_copy(const void* wav, int wav_is_i16, int64_t total, float* out, hipStream_t s);      // sr_in == sr_out
void launch_trim_scan(const float* y, const ResampleSeq* seqs, int B, float frac, int64_t* cuts /* (2 B,): first, last */, hipStream_t s);
void launch_trim_gather(const float* y, const TrimSeq* seqs, int B, int64_t max_len, int pad, float* out, hipStream_t s);

// ev_deliver (ev_deliver.hip): ev_resample's output sample, converted in registers to the response's encoding.  A tile is DL_TILE consecutive outputs
// of one utterance, four consecutive outputs per thread, stored as one quad (4 / 8 / 16 bytes); the table is ev_resample's (resample_pack_table).  A
// tile's run of inputs stays in LDS and the table beside it by ev_resample's rule (polyphase_lds).  Every tile leaves a DeliverPart; the fold
// kernel reduces the parts of an utterance, tile0 .. tile0 + ceil(n / DL_TILE), in ascending order (a max and an integer sum: exact in any order).
constexpr int DL_TILE = 1024;
enum { DL_F32 = 0, DL_S16 = 1, DL_ULAW = 2, DL_ALAW = 3 };
struct DeliverSeq { int64_t in_off, len, n, byte_off, slot; uint32_t seed; int32_t tile0; };      // slot = the utterance's bytes rounded up to 16
struct DeliverTile { int32_t seq, m0; };
struct DeliverPart { float peak; int32_t clipped; };
struct DeliverOut { float peak; int32_t pad; int64_t clipped; };
struct DeliverParams {
    const void* wav; int wav_is_i16;                  // utterances back to back, fp32 or int16 (x / 32768)
    const DeliverSeq* seqs; const DeliverTile* tiles; int n_tiles;
    int up, down, half, row;                          // row = resample_row_len(up, half); up == down == 1: no filter, tab unused
    const float* tab;                                 // (up, row) on the device
    int encoding, dither;                             // DL_*; dither: 0 none, 1 TPDF
    uint8_t* out;                                     // utterance b at byte_off, slot bytes
    DeliverPart* parts;                               // (n_tiles,)
    int run_cap;                                      // set by the launcher: floats of LDS for the run, 0 = read through L1
};
int launch_deliver(const DeliverParams& p, hipStream_t s);      // 0, or -1 for bad parameters
void launch_deliver_fold(const DeliverPart* parts, const DeliverSeq* seqs, int B, DeliverOut* outs, hipStream_t s);

// ev_stitch (ev_stitch.hip): segments -> documents.  The scan spreads a segment's peak over blocks of ST_PEAK_CHUNK samples and finds its edges in
// chunks of ST_EDGE_CHUNK; the mix writes one tile of ST_TILE output samples per block with the ramp table (F <= ST_MAX_FADE floats) in LDS.
constexpr int ST_PEAK_CHUNK = 4096, ST_EDGE_CHUNK = 1024, ST_TILE = 1024, ST_MAX_FADE = 4096;
struct StitchSeg { int64_t off, len, part_off; };                  // first sample, length, index of the first of its ceil(len / ST_PEAK_CHUNK) partial peaks
struct StitchMixSeg { int64_t src, pos; int32_t n, fl, fr, pad; }; // the cut wav[src .. src + n) starts at sample pos of its document; fade lengths left / right
struct StitchDoc { int64_t out_off, len; int32_t seg0, nseg; };    // output offset / length, its run of segments
struct StitchTile { int32_t doc, tile; };                          // one block: document and tile
void launch_stitch_peak(const float* wav, const StitchSeg* segs, int S, int64_t max_len, float* part, hipStream_t s);
void launch_stitch_edges(const float* wav, const StitchSeg* segs, int S, const float* part, float frac, float abs_thr, float* peak /* (S,) */,
                         int64_t* cuts /* (2 S,): first, last, or -1, -1 */, hipStream_t s);
// In one document pos and pos + n are non-decreasing, pos[s + 2] >= pos[s] + n[s], fl, fr <= min(F, n) and pos + n <= len (ev_stitch_plan gives that).
int launch_stitch_mix(const float* wav, const StitchMixSeg* segs, const StitchDoc* docs, const StitchTile* tiles, int64_t n_tiles, const float* tab, int F,
                      float* out, int16_t* out_i16 /* or NULL */, hipStream_t s);      // 0, or -1 for bad parameters

// ev_compare (ev_compare.hip): two packed signals -> per-segment fp64 sums and maxima.  One block per chunk of CMP_CHUNK elements of one segment;
// the chunk results land in per-chunk arrays (`sums`: four planes of n_chunks -- d, d^2, y, y^2) and a second kernel folds a segment's chunks in order.
constexpr int CMP_CHUNK = 4096;
struct CompareChunk { int64_t off; int32_t n, pad; };              // first element in the packed signals, its 1 .. CMP_CHUNK elements
struct CompareSeg { double sum[4]; double max_d; int64_t arg, nonfinite; float peak_y; int32_t pad; };
int launch_compare_chunks(const float* a, const float* b, const CompareChunk* chunks, int64_t n_chunks, double* sums, double* maxd, int32_t* argd,
                          float* peak, int32_t* nonf, hipStream_t s);      // 0, or -1 for a grid that does not exist
void launch_compare_finish(int B, const int64_t* chunk_offs /* (B + 1,) */, const double* sums, int64_t n_chunks, const double* maxd, const int32_t* argd,
                           const float* peak, const int32_t* nonf, CompareSeg* out /* (B,) */, hipStream_t s);

// ev_flac (ev_flac.hip): packed PCM -> FLAC streams.  One block per frame encodes it into a slot of `stride` bytes (a multiple of 4, at least
// 2 block_size + 24) of a scratch buffer and reports its size and decision; the host lays the frames out; the gather copies every frame to its byte
// offset and, with a stream's first frame, the stream's FLAC_STREAM_HEADER bytes from a table with FLAC_HEADER_STRIDE bytes per segment.
constexpr int FLAC_MAX_BLOCK = 4096, FLAC_STREAM_HEADER = 42, FLAC_HEADER_STRIDE = 48;
struct FlacFrame { int64_t src; int32_t n, index, seg, pad; };     // first sample in the packed input, 1 .. block_size samples, frame number in its segment, the segment
struct FlacParams {
    const void* pcm; int pcm_is_i16, convert;         // int16, or fp32 converted with wrap (0) or clamp (1)
    int block_size, bs_code, sr_code;                 // N and the frame header's codes for N and the sample rate
    int max_fixed_order, max_partition_order;
    const FlacFrame* frames;
    uint8_t* scratch; int stride;
    int32_t* sizes;                                   // (n_frames,): the frame's bytes
    uint32_t* desc;                                   // (n_frames,): kind | partition order << 8
};
int launch_flac_encode(const FlacParams& p, int64_t n_frames, hipStream_t s);      // 0, or -1 for bad parameters
// ev_flac_lpc: the same encoder with the LPC candidates of orders 1 .. max_order (0 .. 12) at `precision` bits (5 .. 15); the analysis alone, per
// frame R (13 int64), shift (12, -1 = no candidate) and coef (12 x 12, [order - 1][j]); and the MD5 of every segment's 16-bit samples, one wave
// per segment (of p only pcm, pcm_is_i16 and convert are read), four little-endian words per segment.
constexpr int FLAC_LPC_MAX_ORDER = 12;
struct FlacLpc { int max_order, precision; };
struct FlacMd5Seg { int64_t src, n; };      // first sample in the packed input, samples
int launch_flac_encode_lpc(const FlacParams& p, const FlacLpc& q, int64_t n_frames, hipStream_t s);
int launch_flac_lpc_analysis(const FlacParams& p, const FlacLpc& q, int64_t n_frames, int64_t* R, int32_t* shift, int32_t* coef, hipStream_t s);
void launch_flac_md5(const FlacParams& p, const FlacMd5Seg* segs, int B, uint32_t* digests, hipStream_t s);
void launch_flac_gather(const uint8_t* scratch, int stride, const FlacFrame* frames, int64_t n_frames, const int32_t* sizes, const int64_t* frame_offs,
                        const uint8_t* headers, uint8_t* out, hipStream_t s);

// ev_loudness (ev_loudness.hip): packed segments -> per tile of LOUD_TILE samples (counted from its segment's start) the K-weighted sums of y^2 over
// the 100 ms steps it reaches into, its sample peak and its count of non-finite samples; then, with one gain per segment, the scaled waveform.
constexpr int LOUD_TILE = 4096, LOUD_RUN = 16, LOUD_SLOTS = 8;
struct LoudTile { int64_t src, pos; int32_t n, seg; };      // first sample in the packed input, the same counted in its segment, 1 .. LOUD_TILE samples, the segment
struct LoudSeg { int64_t tile0, ntiles; };                  // the segment's tiles are [tile0, tile0 + ntiles)
struct LoudCoef {
    double b[2][3], a[2][2];      // shelf, high-pass: b0 b1 b2, a1 a2
    double P[9][16];              // P[d] = A^(LOUD_RUN 2^d), row-major, A the 4 x 4 transition matrix of the cascade; P[8] = A^LOUD_TILE
};
struct LoudTileOut { double sum[LOUD_SLOTS]; float peak; int32_t nonfinite; };      // sum[k]: step pos / step + k of the segment; unused slots are 0
// ends and init are (n_tiles, 4) scratch; step is sample_rate / 10.  0, or -1 for a shape the kernels do not build.
int launch_loudness_measure(const void* wav, int is16, const LoudTile* tiles, int64_t n_tiles, const LoudSeg* segs, int B, const LoudCoef* coef, int step,
                            double* ends, double* init, LoudTileOut* outs, hipStream_t s);
// offs: (B + 1,) device; out must be 16-byte aligned; out_i16 may be NULL
int launch_loudness_gain(const void* wav, int is16, const int64_t* offs, int B, const float* gain, int64_t total, float* out, int16_t* out_i16,
                         hipStream_t s);

// ev_limit (ev_limit.hip): packed segments -> per sample the gain r that the 4x true-peak meter requires, per tile of LIMIT_TILE samples (counted
// from its segment's start) the sample peak, the true peak and the count of non-finite samples; then, per tile, the eroded and smoothed gain s, the
// limited waveform, the smallest s and the count of s < 1.  The taps go in as limit_pack_taps lays them out; the window as L + 1 doubles.
constexpr int LIMIT_TILE = 4096, LIMIT_HALO = 16, LIMIT_TAPS = 129, LIMIT_TAB = 4 * (2 * LIMIT_HALO + 1);
constexpr int LIMIT_MAX_LOOKAHEAD = 1024, LIMIT_MAX_HOLD = 8192, LIMIT_MAX_LDS = 160 * 1024;
struct LimitTile { int64_t src, pos, len; int32_t n, seg; };      // first sample in the packed input, the same counted in its segment, the segment's length, 1 .. LIMIT_TILE samples, the segment
struct LimitPeakOut { float sample_peak, true_peak; int32_t nonfinite, pad; };
struct LimitApplyOut { float min_gain; int32_t limited; };
// r reach twice (the erosion's two copies) and the window in fp64: EV_LIMIT_LDS_BYTES of include/evhip.h
constexpr size_t limit_apply_lds_bytes(int L, int Hd) { return 2 * sizeof(float) * (size_t)(LIMIT_TILE + 2 * L + Hd) + sizeof(double) * (size_t)(L + 1); }
// tab[(d + LIMIT_HALO) * 4 + q] = (double)h[q - 4 d], d = -LIMIT_HALO .. LIMIT_HALO, 0 outside the taps' support: host, LIMIT_TAB doubles
void limit_pack_taps(const float* h /* host (LIMIT_TAPS,), h[-64 .. 64] */, double* tab);
// gains: device (B,) or null = 1; r: device, packed as the input, or null = measure only.  0, or -1 for a grid that does not exist.
int launch_limit_peak(const void* wav, int is16, const float* gains, const LimitTile* tiles, int64_t n_tiles, const double* tab, float ceiling, float* r,
                      LimitPeakOut* outs, hipStream_t s);
// win: device (L + 1,) doubles; out_i16 and s_out (the gain per sample) may be null.  0, or -1 for bad parameters.
int launch_limit_apply(const void* wav, int is16, const float* gains, const LimitTile* tiles, int64_t n_tiles, const float* r, const double* win, int L,
                       int Hd, float* out, int16_t* out_i16, float* s_out, LimitApplyOut* outs, hipStream_t s);

// ev_stretch (ev_stretch.hip): packed segments -> per segment the lag track of WSOLA (one block per segment, the frame loop inside), then, per
// tile of STRETCH_OLA_FRAMES output frames, the two-term overlap-add.  Segment b has `frames` = ceil(len_out / STRETCH_HOP) lags at frame_off.
constexpr int STRETCH_FRAME = 512, STRETCH_HOP = 256, STRETCH_LAGS = 256, STRETCH_OLA_FRAMES = 4;
struct StretchSeg { int64_t in_off, len_in, out_off, len_out, frame_off; int32_t frames, pad; };
struct StretchTile { int32_t seg, k0; };      // the segment, the tile's first frame
struct StretchFig { uint64_t sum_dist; int64_t nonfinite; int32_t edge_frames, pad; };
// the nominal read position of frame k: floor(k H L_in / L_out + 1/2); k H <= len_out + H and both lengths <= 2^30 keep it inside int64
__host__ __device__ inline int64_t stretch_a(int64_t k, int64_t len_in, int64_t len_out) { return (2 * k * STRETCH_HOP * len_in + len_out) / (2 * len_out); }
// deltas: device (total frames,) int16; figs: device (B,).  0, or -1 for a grid that does not exist.
int launch_wsola_search(const void* wav, int is16, const StretchSeg* segs, int B, int16_t* deltas, StretchFig* figs, hipStream_t s);
// win: device (STRETCH_HOP,) the rising half of the window; out_i16 may be null
int launch_wsola_ola(const void* wav, int is16, const StretchSeg* segs, const StretchTile* tiles, int64_t n_tiles, const int16_t* deltas, const float* win,
                     float* out, int16_t* out_i16, hipStream_t s);

// ev_score (ev_score.hip): log-mel -> integer cepstra (one side at a time), then per pair the local distances, the time warp and the sums along
// its path.  The distances and the 2-bit decisions are stored in the order the warp's wavefront visits them: lane l of the wave owns rows
// [l * rm, (l + 1) * rm) of a and works on column s - l at step s, so cell (i, j) lives at step s = j + i / rm, run index r = i % rm, lane l = i / rm:
// dist[(s * rm + r) * 64 + l] and bit pair r % 16 of dec[(s * W + r / 16) * 64 + l], W = score_dec_words(rm).  rm is the pair's own (score_run).
constexpr int SCORE_MAX_FRAMES = 4096, SCORE_MAX_CEPS = 32, SCORE_MAX_MELS = 128, SCORE_TF = 64, SCORE_CLAMP = 1 << 27;
constexpr int score_run(int Ta) { int rm = 1; while (rm * 64 < Ta) rm *= 2; return rm; }      // 1 .. 64 for Ta <= SCORE_MAX_FRAMES
constexpr int score_dec_words(int rm) { return rm > 16 ? rm / 16 : 1; }
struct ScoreTile { int64_t mel_off, frm_off; int32_t T, t0, sig, pad; };      // the signal's first mel element / packed frame, its frames, the tile's first frame, the signal
struct ScoreSig { int64_t frm_off; int32_t T, pad; };
struct ScorePair {
    int64_t fa_off, fb_off;         // first packed frame of the pair's signals
    int64_t dist_off, dec_off;      // into this pass' workspace (uint32 elements): the pass' distances, then its decisions
    int64_t rev_off;                // the backtrack's path, written from the end of Ta + Tb - 1 slots
    int64_t path_off;               // the finished path (score_sums)
    int32_t Ta, Tb, rm, K;          // K: known for a linear score, read back from ScoreWarp otherwise
};
struct ScoreWarp { int64_t sum_dist; int32_t K, pad; };
struct ScoreSums { int64_t sum_dist; double sum_c, sum_c2; int32_t n_diag, n_a, n_b, n_vv, n_vu, n_uv, n_uu, pad; };
// basis: device (D, M) fp32; bad: (total_frames,) 0 / 1, a frame with a non-finite mel value; cq: (total_frames, D)
int launch_score_cepstra(const float* mel, const ScoreTile* tiles, int64_t n_tiles, const float* basis, int M, int D, int32_t* cq, int32_t* bad, hipStream_t s);
void launch_score_count(const int32_t* bad, const ScoreSig* sigs, int B, int32_t* nonfinite /* (B,) */, hipStream_t s);
// sel: device (n,) indices of the pairs of one pass whose run is rm; max_steps over them (steps = Tb + 63).  dist and dec are one workspace:
// a pair's dist_off and dec_off are both counted from its start
int launch_score_dist(const int32_t* cqa, const int32_t* cqb, int D, const ScorePair* pairs, const int32_t* sel, int n, int rm, int max_steps, uint32_t* dist,
                      hipStream_t s);
// sel: device (n,) indices of the pairs whose run is rm
int launch_score_dtw(int rm, const ScorePair* pairs, const int32_t* sel, int n, const uint32_t* dist, uint32_t* dec, int32_t* rev, ScoreWarp* warp, hipStream_t s);
// f0a / f0b: packed as the frames, both or neither; linear: the path is (k, k), k < K, and the distances are computed here; otherwise the path is
// read from rev and sum_dist from warp
void launch_score_sums(const ScorePair* pairs, int B, int linear, const int32_t* cqa, const int32_t* cqb, int D, const int32_t* rev, const ScoreWarp* warp,
                       const float* f0a, const float* f0b, int32_t* path_a, int32_t* path_b, ScoreSums* out, hipStream_t s);

}  // namespace ev
