/*
 * evhip_ops.h -- per-kernel entry points of libevhip.so used by the parity tests (tests/test_gpu_ops.py, test_gpu_pair_long.py,
 * test_gpu_group3.py).  They launch one gfx950 kernel on caller-provided DEVICE pointers and are not needed by an integrator;
 * the drop-in boundary is include/evhip.h.  Each op cites the reference op it is checked against.
 */
#ifndef EVHIP_OPS_H_
#define EVHIP_OPS_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Implicit-GEMM conv / linear (emotivoice_amd/csrc/ev_gemm.hip).  Checked against torch.nn.functional
 * linear / conv1d / conv_transpose1d, i.e. the ops behind reference modules/encoder.py:50-52,72-109,
 * modules/variance.py:41-46 and models/hifigan/models.py:50-57,116-128.
 *   out[m,n] = post( scale * ( act( sum_{tap,k} pro(A[m+(tap-center)*dil,k]) * W[n][tap][k] + bias[n] )
 *                               + seq_bias[row_seq[m]][n] + res[m,n] ) + acc32[m,n] + add16_a[m,n] + add16_b[m,n] ), invalid rows -> 0
 * Field order and types mirror ev::ConvGemmParams exactly. */
typedef struct ev_conv_gemm_desc {
    int dtype;                 /* 0: fp16 operands (MFMA 16x16x32 f16), 1: fp32 operands (MFMA 16x16x4 f32),
                                  2: fp32 activations x fp16 hi/lo split weights, 3 fp16 MFMAs per product (fp32-level accuracy),
                                  3: fp32 activations; hi x hi as one fp16 MFMA + the two cross terms as block-scaled fp4 MFMAs
                                     (v_mfma_scale_f32_16x16x128_f8f6f4): needs W, W_lo, W_mx, mx_scratch */
    const void* A; int lda;
    const void* W;
    const void* W_lo;          /* dtype 2 only */
    const float* bias;
    int M, N, K, taps, dil, center;
    const uint8_t* row_valid; int valid_shift;
    const int32_t* row_seq; const float* seq_bias; int ld_seq_bias;
    int act; float act_slope;  /* 0 none, 1 relu, 2 gelu(erf), 3 leaky_relu, 4 tanh */
    int pro_lrelu; float pro_slope;
    const void* res; int res_dtype; int ldres;
    float out_scale;
    const float* acc32; int ldacc;
    int post_lrelu; float post_slope;
    void* out16; float* out32; int ldo;
    int out32_before_post;
    int reserved0;
    const void* add16_a; const void* add16_b; int ldadd;   /* two fp16 [M][N] tensors added after scaling (both or neither), or NULL */
    int ksplit;                                  // DT_F32S, N % 64 == 0, no add16: > 1 = split-K.  The K / 32 chunks are cut into `ksplit` equal ranges (K / 32 must be a
                                                 // multiple), each (tile, range) is a block of the 128 x 64-tile kernel writing fp32 partial sums to mx_scratch
                                                 // (>= ksplit * M * N * 4 bytes), and a second kernel adds them in range order and applies the epilogue.  Shortens the
                                                 // sequential step chain of the token-rate GEMMs (few tiles, K * taps up to 4608).  The summation order differs from
                                                 // ksplit <= 1, so a caller that promises batch invariance picks it by layer shape, never by M.
    const void* W_mx;          /* dtype 3: emotivoice_amd/mxfp4.py pack_weight_planes(W) on the device (NULL: the call runs as dtype 2) */
    void* mx_scratch; size_t mx_scratch_size;   /* dtype 3 with fp32 A: device scratch, >= ev_op_mx_scratch_bytes(M, K) */
    const void* mx_x4[2]; const void* mx_xs[2]; unsigned mx_xs_stride; int polyphase_cout;   /* dtype 3 with a plane-set input: A = its fp16 hi
                                  plane, these = its fp4 code planes (hi, lo), E8M0 scale planes and the chunk stride of those; else zero.
                                  polyphase_cout > 0 (dtype 3, taps 3): the call is a ConvTranspose1d(k = 2 s, stride s, pad s / 2) as a 3-tap conv with
                                  N = s * polyphase_cout (packer._convT_to_gemm): phases below s / 2 have an all-zero tap 2, the others an all-zero tap 0,
                                  and the MX conv-GEMM skips that tap's matrix instructions; 0 = every tap is multiplied */
    /* plane-set output (dtype 3): planes of lrelu(result, mxo_slope) as [rows][2^mxo_logC]: fp16 hi plane, fp4 code planes of the hi / lo
       parts, their scale planes [C/128][mxo_qs_stride/4][4]; all NULL = none.  emotivoice_amd/mxfp4.py states the contents. */
    void* mxo_h; void* mxo_q4[2]; void* mxo_qs[2]; unsigned mxo_qs_stride; int mxo_logC; float mxo_slope; int reserved3;
    /* res_dtype 3 (dtype 3 only): the residual is the plane set of lrelu(x, 1 / res_inv_slope): res = its fp16 hi plane [M][N] (ldres == N),
       res_x4 = the fp4 codes of the remainder [M][N / 2], res_xs their E8M0 scales [N / 128][res_xs_stride / 4][4]; x = hi + code * scale,
       negative values times res_inv_slope */
    const void* res_x4; const void* res_xs; unsigned res_xs_stride; float res_inv_slope;
    /* accumulate-in from a partial plane set (dtype 3 with res_dtype 3; instead of acc32): acc_h fp16 hi plane [M][N] (ldacc == N), acc_x4 fp4 codes of the
       remainder [M][N / 2], acc_xs their E8M0 scales [N / 128][acc_xs_stride / 4][4]; the addend is hi + code * scale.  mxo_partial != 0: the output plane
       set is partial as well (mxo_h, mxo_q4[1], mxo_qs[1] only; mxo_slope = 1), and may alias the acc_* planes */
    const void* acc_h; const void* acc_x4; const void* acc_xs; unsigned acc_xs_stride; int mxo_partial;
} ev_conv_gemm_desc;

int ev_op_conv_gemm(const ev_conv_gemm_desc* d, void* hip_stream);
/* Three independent dtype-3 convs as ONE grid (conv_gemm_mx_group3_kernel, emotivoice_amd/csrc/ev_gemm_mx.h): what the engine issues for the same-level convs of
 * a stage's three ResBlocks.  d3 = three descriptors with taps {3, 7, 11} in any order, plane sets in, the same M / N / K (M % 256 == 0, N % 128 == 0,
 * K % 128 == 0) and the same epilogue form, one of two: planes only (conv1 of a pair), or residual from a plane set + planes only (conv2 inside a ResBlock);
 * no acc32, no out32, reserved0 == 0.  Returns -2 if a member fails the descriptor checks of the single launch, -1 if the three are not such a triple (nothing is
 * launched: the caller issues them one by one) or the launch failed, 0 otherwise; check_only != 0 answers without launching.  Checked against the three single
 * launches of the same descriptors, bit for bit (tests/test_gpu_group3.py). */
int ev_op_conv_gemm_group3(const ev_conv_gemm_desc* d3, int check_only, void* hip_stream);
/* scratch bytes a dtype-3 call with an [M][K] activation needs (fp16 hi plane, two fp4 code planes, two E8M0 scale planes) */
size_t ev_op_mx_scratch_bytes(int M, int K);
/* where a dtype-3 call with an fp32 [M][K] activation lays that activation's plane set inside its mx_scratch (what its mx_planes_kernel pass fills), row 0 of
 * each plane: out[0] the fp16 hi plane [M][K], out[1] / out[2] the fp4 code planes of the hi / lo parts [M][K / 2], out[3] / out[4] their E8M0 scale planes
 * (chunk-major [K / 128][out[5] / 4 rows][4], as mx_xs), all as addresses, out[5] = the scale planes' chunk stride in bytes.  Host only: nothing is launched.
 * Returns 0, or -2 for a null argument or a shape the scratch layout does not cover (M <= 0, K % 128). */
int ev_op_mx_scratch_planes(void* scratch, int M, int K, unsigned long long out[6]);

/* Fused HiFi-GAN ResBlock1 pair for C = 32: xt = lrelu(c1(lrelu(x)) + b1); out = epi(c2(xt) + b2 + x)
 * (reference models/hifigan/models.py:50-57).  `epi` uses the ev_conv_gemm_desc fields bias (= b2), res (= x), res_dtype,
 * ldres, row_valid, valid_shift, out_scale, acc32, ldacc, add16_a, add16_b, ldadd (acc32 and add16 are mutually exclusive here),
 * post_lrelu, post_slope (in [0, 1]), out16, out32, ldo, out32_before_post.
 * Kernel variant: a k = 3 call with ntiles = ceil(M / 254) >= 4 x the device's CU count takes the two-blocks-per-CU kernel (grid 2 x CUs), every other call the
 * one-block kernel (grid min(ntiles, CUs)); epi.reserved0 bit 2 (4) selects the one-block kernel for every call.  Both give the same bits. */
typedef struct ev_res_pair_desc {
    const void* x; int ldx;
    const void* w1; const float* b1;
    const void* w2;
    int M, k, dil;
    int gmin, gmax;    /* rows of x that exist (relative to x): gmin <= g < gmax; leave both 0 for the whole tensor {0, M} */
    const void* w1_mx; const void* w2_mx;   /* ev_op_resblock_pair_c32_mx only: mxfp4.pack_pair_weight_planes(w) of the two convs */
    ev_conv_gemm_desc epi;
} ev_res_pair_desc;
int ev_op_resblock_pair_c32(const ev_res_pair_desc* d, void* hip_stream);
/* The same pair in the MX arithmetic (one fp16 MFMA + two block-scaled fp4 MFMAs per product): x and out32 fp32 [rows][32], w1 / w2 the
 * fp16 hi parts of the weights, w1_mx / w2_mx their fp4 planes; epi: bias, res (= x, fp32), row_valid, out_scale, acc32 (optional, may
 * alias out32), out32, ldo.
 * Kernel variant, by epi.reserved0: 0 = the rule on the layer's shape (the E5M2-operand kernel at k = 3, the fp4 kernel at k = 7 / 11); bit 5 (32) = the E5M2 kernel
 * at every k; bit 4 (16) = the fp4 kernel at every k (it wins over bit 5); bit 2 (4), fp4 only = the lock-step kernel (256-row tiles) instead of the two-group one
 * (128-row tiles, taken from two tiles on) -- the two fp4 kernels give the same bits, the E5M2 kernel different ones. */
int ev_op_resblock_pair_c32_mx(const ev_res_pair_desc* d, void* hip_stream);
/* The pair at C = 64, k = 3 in the MX arithmetic with plane sets in and out: x = the fp16 hi plane [rows][64] of the plane set of leaky_relu(x, 1 / res_inv_slope),
 * epi.mx_x4 / mx_xs / mx_xs_stride its code / scale planes; w1 / w2 fp16 hi parts [64][3][64], w1_mx / w2_mx = mxfp4.pack_c64_weight_planes; epi: bias (= b2),
 * res_inv_slope, out_scale, acc32 (optional), row_valid, out32 and / or the output plane set mxo_* (mxo_logC = 6).  Bit-identical to the two layer-wise
 * ev_op_conv_gemm launches it replaces. */
int ev_op_resblock_pair_c64_mx(const ev_res_pair_desc* d, void* hip_stream);
/* the same pair at C = 64 (HiFi-GAN stage 2), k = 3 only (both weight sets stay in LDS), dil <= 8 (the tile's slab); -2 otherwise */
int ev_op_resblock_pair_c64(const ev_res_pair_desc* d, void* hip_stream);

/* LayerNorm(eps) over channels, optional fused Linear(C,1) head (reference modules/encoder.py:112-127,
 * modules/variance.py:29-33,46).  One wave per row: C % 128 == 0, 128 <= C <= 1024 (-2 otherwise); rows > 0; out16 / out32 / dot_out optional. */
int ev_op_layernorm(const float* x, int rows, int C, const float* gamma, const float* beta, float eps,
                    const uint8_t* row_valid, void* out16, float* out32, const float* dot_w, float dot_b,
                    float* dot_out, void* hip_stream);

/* The same LayerNorm writing the MX plane set of its output (emotivoice_amd/mxfp4.py) instead of fp32 rows: h fp16 hi plane [rows][C], q4h / q4l the fp4
 * codes of the hi / lo parts [rows][C / 2], qsh / qsl their E8M0 block scales [C / 128][qs_stride / 4 rows][4]; C <= 512, C % 128 == 0.  What the mel
 * decoder's QKV projection / conv-FFN read in the mx mode (reference modules/encoder.py:154-200: the norm in front of each sub-layer). */
int ev_op_layernorm_planes(const float* x, int rows, int C, const float* gamma, const float* beta, float eps,
                           const uint8_t* row_valid, void* h, void* q4h, void* q4l, void* qsh, void* qsl,
                           unsigned qs_stride, void* hip_stream);

/* Multi-head self-attention restricted to each utterance's rows (reference modules/encoder.py:72-109).
 * is_f16: 1 = fp16 rows (fp16 MFMA flash kernel), 0 = fp32 rows, exact fp32 MFMA products, 2 = fp32 rows, split-precision products
 * (three fp16 MFMAs each: the mel decoder in the strict / mx modes).  d_k = C / heads must be 48 (is_f16 == 0: 48 or 64), max_len >= every
 * seq_len (it sizes the grid and, for is_f16 == 2, picks the 4 / 8 / 16-wave kernel at 64 / 128); only rows [seq_off, seq_off + seq_len) are read. */
int ev_op_attention(const void* qkv, int is_f16, int C, int heads, const int32_t* seq_off, const int32_t* seq_len,
                    int B, int max_len, void* out, void* hip_stream);

/* ---- the non-GEMM kernels (emotivoice_amd/csrc/ev_misc.hip, ev_align.hip; tests/test_gpu_misc_ops.py).  Each entry point launches exactly the launcher the
 * engine uses, on caller-provided device pointers, and returns -2 without launching for a shape its kernel would silently mishandle.  "rows" follow the
 * gap layout: row_seq[r] = utterance of row r or -1 (gap), row_pos[r] = position inside it, cu_seqlens[b] = packed offset of utterance b. */

/* out[r] = emb[clamp(ling[cu[b] + pos], 0, n_vocab - 1)] + alpha * pe[pos]; tap_out[r] (optional) = the embedding row; gap rows = 0
 * (reference model_open_source.py:107, modules/encoder.py:257-261).  C even; pe needs max(pos) + 1 rows. */
int ev_op_embed_pe(const int64_t* ling, const int32_t* cu_seqlens, const int32_t* row_seq, const int32_t* row_pos, const float* emb, int n_vocab,
                   const float* pe, float alpha, float* out, float* tap_out, int rows, int C, void* hip_stream);
/* out[r] = (word[clamp(id)] + type[clamp(type_id)]) + pos_emb[min(pos, max_pos - 1)] (transformers BertEmbeddings.forward; reference
 * models/prompt_tts_modified/simbert.py:37); type_ids NULL = type 0; gap rows = 0.  C even. */
int ev_op_bert_embed(const int64_t* ids, const int64_t* type_ids, const int32_t* cu_seqlens, const int32_t* row_seq, const int32_t* row_pos,
                     const float* word, const float* pos_emb, const float* type_emb, int vocab, int max_pos, int n_types, float* out, int rows,
                     int C, void* hip_stream);
/* out[b] = tanh(W x[seq_off[b]] + bias) (transformers BertPooler; simbert.py:49-55).  W [C][C]; B <= 65535; ldx >= C. */
int ev_op_bert_pooler(const float* x, int ldx, const int32_t* seq_off, const float* W, const float* bias, float* out, int B, int C, void* hip_stream);
/* u[b] = bias + Wcond[:, :C] spk_emb[clamp(speaker[b])] + Wcond[:, C:C+bert] style[b] + Wcond[:, C+bert:] content[b]
 * (reference model_open_source.py:109-111).  Wcond [C][C + 2 bert]; B <= 65535. */
int ev_op_cond_vector(const int64_t* speaker, const float* style, const float* content, const float* spk_emb, int n_speaker, const float* Wcond,
                      const float* bias, float* u, int B, int C, int bert, void* hip_stream);
/* out[r] = x[r] + (bp + sum_t wp[t] pitch[r + t - (k-1)/2]) + (be + sum_t we[t] energy[r + t - (k-1)/2]) on valid rows, 0 elsewhere
 * (Conv1d(1 -> C, k, pad (k-1)/2), reference model_open_source.py:131-134).  wp / we [k][C]; k odd, C even; row_valid required.  Halo: pitch / energy are
 * read at [r - (k-1)/2, r + (k-1)/2] for every valid row r, so (k-1)/2 readable (zero) scalars on both sides of each utterance. */
int ev_op_var_embed_add(const float* x, const float* pitch, const float* energy, const float* wp, const float* bp, const float* we, const float* be,
                        const uint8_t* row_valid, float* out, int rows, int C, int k, void* hip_stream);
/* ev_synthesize_prosody's effective tracks: src = override[cu[b] + pos] if given and finite else the prediction; out = scale * src + shift per utterance
 * (one fma), an identity transform copies src bit for bit; ctrl SoA [5][B] = alpha, pitch_scale, pitch_shift, energy_scale, energy_shift; gap rows = +0. */
int ev_op_prosody_tracks(const float* pitch, const float* energy, const int32_t* row_seq, const int32_t* row_pos, const int32_t* cu_seqlens,
                         const float* pitch_ovr, const float* energy_ovr, const float* ctrl, int B, float* pitch_out, float* energy_out, int rows,
                         void* hip_stream);
/* d = max(rint(exp(log_d) - 1), 0) or forced[]; all-zero guard (every d := 1); centre = cumsum(d alpha) - d alpha / 2; mel_len = int(sum d alpha)
 * (reference modules/variance.py:47-51, modules/alignment.py:183-202).  One block per utterance; alpha == 1: exact integer scan, else a sequential fp32
 * running sum.  alpha > 0.  log_d / centre_rows are token rows (tok_off), dur_packed / logd_packed / forced packed (cu_seqlens). */
int ev_op_durations(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const int64_t* forced,
                    const int32_t* cu_seqlens, int64_t* dur_packed, float* logd_packed, float* centre_rows, int32_t* mel_len, void* hip_stream);
/* the same with per-utterance scales alpha_b (NULL = alpha) and per-token overrides partial (packed; >= 0 forced and clamped to dur_cap, negative =
 * predicted; NULL = none): dur_packed keeps the predictions, dur_eff (required) receives what is scanned.  0 <= dur_cap <= 2^20. */
int ev_op_durations_prosody(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const float* alpha_b,
                            const int64_t* partial, int64_t dur_cap, const int32_t* cu_seqlens, int64_t* dur_packed, int64_t* dur_eff,
                            float* logd_packed, float* centre_rows, int32_t* mel_len, void* hip_stream);
/* tap[t] = sum_j softmax_j(-delta (t - c_j)^2) x[j]; out[t] = tap[t] + pe_alpha * pe[t]; gap rows = 0 (reference modules/alignment.py:204-210,
 * modules/encoder.py:257-261).  C even, C <= 512 (four float2 accumulators per lane); delta > 0; tap_out optional. */
int ev_op_gauss_upsample(const float* xvar, const float* centre_rows, const int32_t* tok_off, const int32_t* tok_len, const int32_t* frm_row_seq,
                         const int32_t* frm_row_pos, const float* pe, float pe_alpha, float delta, float* out, float* tap_out, int rows, int C,
                         void* hip_stream);
/* mel of utterance b = (n_mels, mel_len[b]) at element mel_elem_off[b] (fp32, or fp16 if is_f16) -> channels-last rows [rows][ldo] (fp16, or fp32 if
 * out_f32) with zero gap rows and zero pad channels n_mels..ldo-1.  ldo >= n_mels. */
int ev_op_mel_to_rows(const void* mel, int is_f16, const int64_t* mel_elem_off, const int32_t* frm_row_seq, const int32_t* frm_row_pos,
                      const int32_t* mel_len, void* out, int out_f32, int rows, int n_mels, int ldo, void* hip_stream);
/* wav[r] = tanh(bias + sum_{t, c} w[t][c] a[r + t - (k-1)/2][c]) on rows with row_valid[r >> valid_shift] != 0, else 0 (reference
 * models/hifigan/models.py:127-129).  fp16 x: a = x; fp32 x: a = max(x, pre_slope x), pre_slope in [0, 1].  C == 32, k odd <= 15, ldx >= 32 and a multiple
 * of 16 bytes, row_valid required.  Halo: every 256-row block stages rows [256 i - (k-1)/2, 256 i + 256 + (k-1)/2), so rows
 * [-(k-1)/2, 256 ceil(rows / 256) + (k-1)/2) of x must be readable, and zero outside the utterances. */
int ev_op_conv_post(const void* x, int is_f32, int ldx, const float* w, float bias, int k, float pre_slope, const uint8_t* row_valid, int valid_shift,
                    float* wav_rows, int rows, int C, void* hip_stream);
/* seq[r] = the utterance b with off[b] <= r < off[b] + len[b] or -1, pos[r] = r - off[b] or 0, valid[r] = 1 or 0.  off ascending. */
int ev_op_row_maps(const int32_t* off, const int32_t* len, int B, int32_t* seq, int32_t* pos, uint8_t* valid, int rows, void* hip_stream);
/* dst[(seq_out_off[b] + r) * C + c] = (float)src[(seq_row_off[b] + r) * ld + c], r < seq_rows[b] (src fp16 if is_f16, else fp32).  max_rows = max_b
 * seq_rows[b] sizes the grid (grid-stride above 4096 blocks); B <= 65535; ld >= C. */
int ev_op_pack_rows(const void* src, int is_f16, int ld, int C, const int64_t* seq_row_off, const int64_t* seq_out_off, const int32_t* seq_rows, int B,
                    int64_t max_rows, float* dst, void* hip_stream);
/* out[i] = (int16)(int32)(wav[i] * 32768.0f): truncation toward zero, wrap-around (reference inference_am_vocoder_joint.py:130-131). */
int ev_op_wav_to_i16(const float* wav, int16_t* out, int64_t n, void* hip_stream);
/* rows [row0, row1) of the sinusoid table: pe[t][2i] = sin((float)t * div[i]), pe[t][2i+1] = cos(.) (reference modules/encoder.py:216-237).  C even. */
int ev_op_pe_extend(float* pe, const float* div, int row0, int row1, int C, void* hip_stream);
/* log_p[lp_off[b] + t N + n] = log_softmax_n(-||feats[frm_row[b] + t] - text[tok_row[b] + n]||_2) + log betabinom.pmf(n; N, t + 1, T - t)
 * (reference modules/alignment.py:27-55).  The per-utterance arrays are HOST arrays of B entries; the call waits for the stream.  C % 32 == 0,
 * 1 <= tokens <= 2048, 1 <= frames <= 16384 (-2 otherwise). */
int ev_op_align_score(const float* text, const float* feats, int C, int B, const int32_t* tok_row, const int32_t* tokens, const int32_t* frm_row,
                      const int32_t* frames, const int64_t* lp_off, float* log_p, void* hip_stream);
/* Monotonic alignment search on log_p (T, N) per utterance with Q in fp64 (reference modules/alignment.py:93-122, 145-162): dur[tok_packed[b] + n],
 * the per-token fp64 means of the optional frame tracks (pitch_frames / energy_frames at frm_packed[b] + t; both NULL-able), score[b] = the mean
 * log_p along the path.  bits: scratch, 64 words per frame at bits_off[b].  HOST per-utterance arrays; the call waits for the stream.  One wave per
 * utterance, RM = 1, 2, .. 32 tokens per lane chosen by the batch's longest utterance.  1 <= tokens <= 2048, tokens <= frames <= 16384 (-2 otherwise). */
int ev_op_align_mas(const float* log_p, int B, const int32_t* tokens, const int32_t* frames, const int64_t* lp_off, const int64_t* tok_packed,
                    const int64_t* frm_packed, const int64_t* bits_off, uint32_t* bits, const float* pitch_frames, const float* energy_frames,
                    int64_t* dur, float* pitch_tok, float* energy_tok, float* score, void* hip_stream);

/* ev_features' kernel on caller-provided DEVICE buffers: wav (B utterances back to back, fp32 or int16) -> mel (per utterance (n_mels, T_b) row-major,
 * T_b = wav_lens[b] / hop + 1, packed in utterance order), energy (sum_b T_b,) and, unless NULL, mag (sum_b T_b, n_fft / 2 + 1); semantics as ev_features
 * (include/evhip.h).  wav_lens, mel_basis (n_mels, n_fft / 2 + 1) and window (n_fft,) or NULL are HOST arrays: the call packs the basis planes, waits for
 * the stream and frees them.  -2 for what the kernel would mishandle: n_fft not a multiple of 128 or above 2048, hop not a multiple of 8 or above n_fft,
 * 63 hop + n_fft > 24576, n_mels outside [1, 128], wav_lens[b] < n_fft / 2 + 1, T_b > 16384, B outside [1, 65535].
 * Held on the device (tests/test_gpu_stft_shapes.py) at 128 / 8, 128 / 128, 384 / 48, 640 / 320, 2048 / 352 (n_mels 128 and 80) and 2048 / 256 besides the
 * default 1024 / 256, with the hann window and an asymmetric one, to 4 x the error of a plain float32 evaluation (floor 2^-22); a non-finite sample
 * stays inside its utterance (no rule is stated for the utterance itself). */
int ev_op_stft_mel(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, const float* mel_basis, const float* window, int n_fft, int hop,
                   int n_mels, float mel_clip, float energy_floor, float energy_mean, float energy_std, float* mel, float* energy, float* mag,
                   void* hip_stream);

/* ev_denoise's two kernels on caller-provided DEVICE buffers (semantics: include/evhip.h, ev_denoise).  ev_op_stft_gain: steps 1-3, wav (B utterances
 * back to back, fp32 or int16), bias (n_fft / 2 + 1,) and strengths (B,) -> the scratch planes spec_hi / spec_lo, fp16 (sum_b T_b, k_pad) each, T_b =
 * wav_lens[b] / hop + 1, k_pad = 2 (n_fft / 2 + 1) rounded up to 32: column 2 k holds g Re, 2 k + 1 g Im of bin k, value = hi + lo / 2048, padding columns
 * zero.  With mag not NULL it writes the fp32 magnitudes (sum_b T_b, n_fft / 2 + 1) instead and reads neither bias nor strengths nor the planes.
 * ev_op_istft: steps 4-7, the planes of T_b = frames[b] frames per utterance -> out (sum_b hop (T_b - 1),) fp32 and, unless NULL, out_i16.  wav_lens,
 * frames and window (n_fft,) or NULL are HOST arrays: the calls pack their tables, wait for the stream and free them.  -2 for what a kernel would
 * mishandle: a shape outside ev_denoise's limits, wav_lens[b] < n_fft / 2 + 1, T_b outside [1, 16384], B outside [1, 65535].
 * Held on the device (tests/test_gpu_stft_shapes.py): both modes of ev_op_stft_gain and ev_op_istft at R = n_fft / hop = 1 (128 / 128), 2 (640 / 320), 4 and
 * 8 (384 / 48, 2048 / 256), T_b < R and a second chunk tile included, with the hann window, an asymmetric window and one with a run of zeros; the
 * rejections of 128 / 8 (R = 16) and 2048 / 352 (-2, nothing written); peaks of 2^-12 and 8.0 and +-2 LSB of int16 at the same relative bars; a
 * NaN or an infinity in an utterance gives zero cells in the frames that hold it (step 3) and leaves every other frame and utterance alone. */
int ev_op_stft_gain(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, const float* window, int n_fft, int hop, const float* bias,
                    const float* strengths, void* spec_hi, void* spec_lo, float* mag, void* hip_stream);
int ev_op_istft(const void* spec_hi, const void* spec_lo, int B, const int32_t* frames, const float* window, int n_fft, int hop, float* out,
                int16_t* out_i16, void* hip_stream);

/* ev_pitch's two kernels on caller-provided DEVICE buffers (semantics: include/evhip.h, ev_pitch).  ev_op_pitch_yin: steps 1-5, wav (B utterances back
 * to back, fp32 or int16) -> f0_hz and aperiodicity (sum_b T_b,), T_b = wav_lens[b] / hop + 1, and, unless NULL, the chosen lag tau (-1 = unvoiced).
 * ev_op_pitch_fill: steps 6-7, f0_hz (sum_b frames[b],) -> pitch of the same shape; pitch must not be f0_hz.  wav_lens / frames are HOST arrays; the
 * calls wait for the stream.  -2 for what ev_pitch rejects, B outside [1, 65535], or frames[b] outside [1, 16384]. */
int ev_op_pitch_yin(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, int sample_rate, int hop, int win, float f_min, float f_max,
                    float threshold, float silence_rms, float* f0_hz, float* aperiodicity, int32_t* tau, void* hip_stream);
int ev_op_pitch_fill(const float* f0_hz, int B, const int32_t* frames, float pitch_mean, float pitch_std, float* pitch, void* hip_stream);

/* ev_resample's kernels on caller-provided DEVICE buffers (semantics: include/evhip.h, ev_resample).  ev_op_resample: wav (B utterances back to back,
 * fp32 or int16) -> y (sum_b n_b,), n_b = ceil(wav_lens[b] up / down), packed in utterance order; taps HOST (2 half_len + 1) or NULL = the default
 * design (half_len ignored); sr_in == sr_out copies.  ev_op_trim: y (B utterances of lens[b] samples back to back) -> out, the padded cuts back to
 * back (at most sum_b lens[b] + 2 B trim_pad floats), and the HOST arrays out_lens, trim_start, trim_end (B each); out must not overlap y.  wav_lens /
 * lens are HOST arrays; the calls wait for the stream.  -2 for what ev_resample_setup / ev_resample reject, B outside [1, 65535], and for
 * ev_op_trim a trim_frac outside (0, 1). */
int ev_op_resample(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, int sr_in, int sr_out, const float* taps, int half_len, float* y,
                   void* hip_stream);
int ev_op_trim(const float* y, int B, const int64_t* lens, float trim_frac, int trim_pad, float* out, int64_t* out_lens, int64_t* trim_start,
               int64_t* trim_end, void* hip_stream);

/* ev_stitch's kernels on caller-provided DEVICE buffers (semantics: include/evhip.h, ev_stitch).  ev_op_stitch_scan: the two scan kernels on the S
 * segments wav + seg_offsets[s] of seg_lens[s] samples -> the HOST arrays peak, first, last (S each): max |x|, and the first / last index with
 * |x| > max(peak * trim_frac, trim_abs), or -1, -1 where no sample is.  ev_op_stitch_mix: the mix kernel on segments that are already cut and
 * planned: segment s is wav[src[s] .. src[s] + n[s]) at sample pos[s] of document seg_doc[s] with fade lengths fl[s] / fr[s]; tab = the F ramp
 * values; the D documents of doc_lens samples go to out (and out_i16 unless NULL) back to back.  Every array but wav / out / out_i16 is a HOST
 * array; the calls wait for the stream.  -2 for what ev_stitch rejects and, for ev_op_stitch_mix, a layout the kernel would mishandle: n[s]
 * outside [0, 2^30], fl / fr outside [0, min(F, n[s])], pos or pos + n decreasing inside a document, pos[s + 2] < pos[s] + n[s], a segment that
 * leaves its document, D not seg_doc's count of documents. */
int ev_op_stitch_scan(const float* wav, int S, const int64_t* seg_offsets, const int64_t* seg_lens, float trim_frac, float trim_abs, float* peak,
                      int64_t* first, int64_t* last, void* hip_stream);
int ev_op_stitch_mix(const float* wav, int S, const int64_t* src, const int64_t* n, const int32_t* seg_doc, const int64_t* pos, const int32_t* fl,
                     const int32_t* fr, const float* tab, int F, int D, const int64_t* doc_lens, float* out, int16_t* out_i16, void* hip_stream);

/* ev_flac's encode kernel on caller-provided DEVICE buffers (semantics: include/evhip.h, ev_flac): the frames of B segments of pcm (int16 or
 * fp32, packed back to back, lens[b] samples each) -> slots: frame f, counted segment after segment, starts at slots + f * (2 N + 24), N =
 * cfg->block_size, and the kernel writes its sizes[f] bytes rounded up to a multiple of four there and nothing else.  sizes, kind and porder are
 * HOST arrays of sum_b ceil(lens[b] / N) entries (kind: 0 constant, 1 verbatim, 8 + o fixed); lens is a HOST array; cfg NULL = the default.
 * slots must be 4-byte aligned.  The call waits for the stream.  -2 for what ev_flac rejects. */
int ev_op_flac_encode(const void* pcm, int pcm_is_i16, int B, const int64_t* lens, const ev_flac_config* cfg, uint8_t* slots, int32_t* sizes,
                      uint8_t* kind, uint8_t* porder, void* hip_stream);
/* ev_flac_lpc's analysis alone (rules 4 .. 7 of include/evhip.h) on the frames of the same input: per frame f, R[13 f + l] (l = 0 .. 12, zero
 * beyond L), and per order o = 1 .. 12 shift[12 f + o - 1] (-1: no candidate) and coef[144 f + 12 (o - 1) + j]; a frame of one sample gives zeros
 * and -1.  CONSTANT frames are analysed like any other.  R, shift and coef are HOST arrays.  -2 for what ev_flac_lpc rejects. */
int ev_op_flac_lpc(const void* pcm, int pcm_is_i16, int B, const int64_t* lens, const ev_flac_config* cfg, int max_lpc_order, int qlp_precision, int64_t* R,
                   int32_t* shift, int32_t* coef, void* hip_stream);

/* ev_limit's kernels on caller-provided DEVICE buffers (semantics: include/evhip.h, ev_limit).  ev_op_limit_peak: the meter on B segments of wav
 * (int16 or fp32, packed back to back, lens[b] samples each) with the pre-gains -> r (the required gain per sample, packed as the input; NULL =
 * measure only) and the HOST arrays sample_peak, true_peak, nonfinite (B each).  ev_op_limit_apply: r -> the gain per sample s (unless NULL), out =
 * u * s, out_i16 (unless NULL), and the HOST arrays min_gain and limited (B each).  lens and gains (or NULL = all 1) are HOST arrays.  The calls
 * wait for the stream.  -2 for what ev_limit rejects. */
int ev_op_limit_peak(const void* wav, int wav_is_i16, int B, const int64_t* lens, const float* gains, float ceiling, float* r, float* sample_peak,
                     float* true_peak, int64_t* nonfinite, void* hip_stream);
int ev_op_limit_apply(const void* wav, int wav_is_i16, int B, const int64_t* lens, const float* gains, const float* r, int lookahead, int hold, float* out,
                      int16_t* out_i16, float* s, float* min_gain, int64_t* limited, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* EVHIP_OPS_H_ */
