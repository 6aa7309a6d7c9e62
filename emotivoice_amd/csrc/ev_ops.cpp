// libevhip.so host side: the per-kernel test entry points (include/evhip_ops.h) of the model's kernels.  Each checks what its launcher assumes
// (-2), launches on the caller's stream and reports a launch error (-1); none needs a handle.
#include "ev_host.h"

using namespace ev;
using namespace evh;

extern "C" {

// ------------------------------------------------------------------- per-kernel test entry points (include/evhip_ops.h)
// what ev_op_conv_gemm and ev_op_conv_gemm_group3 refuse (-2) before any launcher sees the descriptor
static bool op_conv_gemm_desc_ok(const ConvGemmParams& p) {
    const int es = p.dtype == DT_F16 ? 2 : 4;
    if (p.M % ROW_ALIGN || p.N % 32 || (p.K * es) % 64 || (p.taps - 1) * p.dil > 64) return false;
    if (p.dtype == DT_F32S && (p.K % 32 || !p.W_lo)) return false;
    if (p.dtype == DT_MX && (p.K % 32 || !p.W)) return false;
    if (mx_check(p) || splitk_check(p)) return false;
    if (!p.out16 && !p.out32 && !p.mxo_h) return false;
    if (p.pro_lrelu && !(p.pro_slope >= 0.f && p.pro_slope <= 1.f)) return false;
    return true;
}
int ev_op_conv_gemm(const ev_conv_gemm_desc* d, void* stream) {
    static_assert(sizeof(ev_conv_gemm_desc) == sizeof(ConvGemmParams), "descriptor layout must match ConvGemmParams");
    ConvGemmParams p;
    memcpy(&p, d, sizeof p);
    if (!op_conv_gemm_desc_ok(p)) return -2;
    launch_conv_gemm(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// three descriptors as ONE grouped grid (launch_conv_gemm_group3): 0 = launched (check_only: would be), -1 = not a triple the grouped kernel takes (nothing launched)
int ev_op_conv_gemm_group3(const ev_conv_gemm_desc* d3, int check_only, void* stream) {
    ConvGemmParams ps[3];
    memcpy(ps, d3, sizeof ps);
    for (int i = 0; i < 3; ++i)
        if (!op_conv_gemm_desc_ok(ps[i])) return -2;
    if (launch_conv_gemm_group3(ps, (hipStream_t)stream, check_only != 0)) return -1;
    if (check_only) return 0;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
size_t ev_op_mx_scratch_bytes(int M, int K) { return mx_scratch_bytes(M, K); }
int ev_op_mx_scratch_planes(void* scratch, int M, int K, unsigned long long out[6]) {
    if (!scratch || !out || M <= 0 || K <= 0 || K % 128) return -2;
    const MxScratchPlanes sp = mx_scratch_planes(scratch, M, K);
    out[0] = (unsigned long long)(uintptr_t)sp.h;
    for (int i = 0; i < 2; ++i) { out[1 + i] = (unsigned long long)(uintptr_t)sp.q4[i]; out[3 + i] = (unsigned long long)(uintptr_t)sp.qs[i]; }
    out[5] = sp.qs_stride;
    return 0;
}
int ev_op_resblock_pair_c32(const ev_res_pair_desc* d, void* stream) {
    static_assert(sizeof(ev_res_pair_desc) == sizeof(ResPairParams), "descriptor layout must match ResPairParams");
    ResPairParams p;
    memcpy(&p, d, sizeof p);
    if (p.k != 3 && p.k != 7 && p.k != 11) return -2;
    if (p.epi.post_lrelu && !(p.epi.post_slope >= 0.f && p.epi.post_slope <= 1.f)) return -2;   // max(v, s v) form of leaky-relu
    launch_resblock_pair_c32(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_resblock_pair_c32_mx(const ev_res_pair_desc* d, void* stream) {
    static_assert(sizeof(ev_res_pair_desc) == sizeof(ResPairParams), "descriptor layout must match ResPairParams");
    ResPairParams p;
    memcpy(&p, d, sizeof p);
    if (p.M <= 0 || p.dil < 1 || (p.k - 1) * p.dil > 64) return -2;
    if (launch_resblock_pair_c32_mx(p, (hipStream_t)stream)) return -2;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_resblock_pair_c64_mx(const ev_res_pair_desc* d, void* stream) {
    ResPairParams p;
    memcpy(&p, d, sizeof p);
    if (launch_resblock_pair_c64_mx(p, (hipStream_t)stream)) return -2;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_resblock_pair_c64(const ev_res_pair_desc* d, void* stream) {
    ResPairParams p;
    memcpy(&p, d, sizeof p);
    if (p.k != 3 || p.dil < 1 || p.dil > PAIR64_MAX_DIL) return -2;
    if (p.epi.post_lrelu && !(p.epi.post_slope >= 0.f && p.epi.post_slope <= 1.f)) return -2;
    launch_resblock_pair_c64(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_layernorm(const float* x, int rows, int C, const float* gamma, const float* beta, float eps, const uint8_t* row_valid,
                    void* out16, float* out32, const float* dot_w, float dot_b, float* dot_out, void* stream) {
    if (rows <= 0 || C < 128 || C > 1024 || C % 128 || (dot_w && !dot_out)) return -2;      // one wave per row, NV float2 chunks of 128 channels per lane
    LayerNormParams p{};
    p.x = x; p.ldx = C; p.rows = rows; p.C = C; p.gamma = gamma; p.beta = beta; p.eps = eps; p.row_valid = row_valid; p.out16 = out16;
    p.out32 = out32; p.ldo = C; p.dot_w = dot_w; p.dot_b = dot_b; p.dot_out = dot_out;
    launch_layernorm(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_layernorm_planes(const float* x, int rows, int C, const float* gamma, const float* beta, float eps, const uint8_t* row_valid,
                           void* h, void* q4h, void* q4l, void* qsh, void* qsl, unsigned qs_stride, void* stream) {
    if (rows <= 0 || C < 128 || C > 512 || C % 128 || !h || !q4h || !q4l || !qsh || !qsl) return -2;
    LayerNormParams p{};
    p.x = x; p.ldx = C; p.rows = rows; p.C = C; p.gamma = gamma; p.beta = beta; p.eps = eps; p.row_valid = row_valid; p.ldo = C;
    p.mxo_h = h; p.mxo_q4[0] = q4h; p.mxo_q4[1] = q4l; p.mxo_qs[0] = qsh; p.mxo_qs[1] = qsl; p.mxo_qs_stride = qs_stride;
    launch_layernorm(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_attention(const void* qkv, int is_f16, int C, int heads, const int32_t* seq_off, const int32_t* seq_len, int B, int max_len,
                    void* out, void* stream) {
    const int dk = heads > 0 && C % heads == 0 ? C / heads : 0;
    if (is_f16 < 0 || is_f16 > 2 || B <= 0 || max_len <= 0) return -2;
    if (is_f16 == 0 ? (dk != 48 && dk != 64) : dk != 48) return -2;          // the MFMA kernels are built for d_k = 48 (fp32: also 64)
    AttnParams p{};
    // is_f16 == 2: fp32 rows, split-precision products
    p.qkv = qkv; p.dtype = is_f16 == 1 ? DT_F16 : (is_f16 == 2 ? DT_F32S : DT_F32); p.ld = 3 * C; p.C = C; p.heads = heads; p.seq_off = seq_off; p.seq_len = seq_len;
    p.B = B; p.max_len = max_len; p.out = out; p.ldo = C;
    launch_attention(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The non-GEMM launchers (ev_misc.hip, ev_align.hip).  Each wrapper refuses (-2) what its kernel silently assumes; include/evhip_ops.h states the limits.
int ev_op_embed_pe(const int64_t* ling, const int32_t* cu_seqlens, const int32_t* row_seq, const int32_t* row_pos, const float* emb, int n_vocab,
                   const float* pe, float alpha, float* out, float* tap_out, int rows, int C, void* stream) {
    if (rows <= 0 || C <= 0 || C % 2 || n_vocab < 1 || !out) return -2;
    launch_embed_pe(ling, cu_seqlens, row_seq, row_pos, emb, n_vocab, pe, alpha, out, tap_out, rows, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_bert_embed(const int64_t* ids, const int64_t* type_ids, const int32_t* cu_seqlens, const int32_t* row_seq, const int32_t* row_pos,
                     const float* word, const float* pos_emb, const float* type_emb, int vocab, int max_pos, int n_types, float* out, int rows,
                     int C, void* stream) {
    if (rows <= 0 || C <= 0 || C % 2 || vocab < 1 || max_pos < 1 || n_types < 1 || !out) return -2;
    launch_bert_embed(ids, type_ids, cu_seqlens, row_seq, row_pos, word, pos_emb, type_emb, vocab, max_pos, n_types, out, rows, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_bert_pooler(const float* x, int ldx, const int32_t* seq_off, const float* W, const float* bias, float* out, int B, int C, void* stream) {
    if (B <= 0 || B > 65535 || C <= 0 || ldx < C) return -2;
    launch_bert_pooler(x, ldx, seq_off, W, bias, out, B, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_cond_vector(const int64_t* speaker, const float* style, const float* content, const float* spk_emb, int n_speaker, const float* Wcond,
                      const float* bias, float* u, int B, int C, int bert, void* stream) {
    if (B <= 0 || B > 65535 || C <= 0 || bert < 0 || n_speaker < 1) return -2;
    launch_cond_vector(speaker, style, content, spk_emb, n_speaker, Wcond, bias, u, B, C, bert, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_var_embed_add(const float* x, const float* pitch, const float* energy, const float* wp, const float* bp, const float* we, const float* be,
                        const uint8_t* row_valid, float* out, int rows, int C, int k, void* stream) {
    if (rows <= 0 || C <= 0 || C % 2 || k < 1 || k % 2 == 0 || !row_valid) return -2;
    launch_var_embed_add(x, pitch, energy, wp, bp, we, be, row_valid, out, rows, C, k, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_prosody_tracks(const float* pitch, const float* energy, const int32_t* row_seq, const int32_t* row_pos, const int32_t* cu_seqlens,
                         const float* pitch_ovr, const float* energy_ovr, const float* ctrl, int B, float* pitch_out, float* energy_out, int rows,
                         void* stream) {
    if (rows <= 0 || B <= 0 || !ctrl) return -2;
    launch_prosody_tracks(pitch, energy, row_seq, row_pos, cu_seqlens, pitch_ovr, energy_ovr, ctrl, B, pitch_out, energy_out, rows, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_durations(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const int64_t* forced,
                    const int32_t* cu_seqlens, int64_t* dur_packed, float* logd_packed, float* centre_rows, int32_t* mel_len, void* stream) {
    if (B <= 0 || !(alpha > 0.f)) return -2;
    launch_durations(log_d, tok_off, tok_len, B, alpha, forced, cu_seqlens, dur_packed, logd_packed, centre_rows, mel_len, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_durations_prosody(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const float* alpha_b,
                            const int64_t* partial, int64_t dur_cap, const int32_t* cu_seqlens, int64_t* dur_packed, int64_t* dur_eff,
                            float* logd_packed, float* centre_rows, int32_t* mel_len, void* stream) {
    if (B <= 0 || !(alpha > 0.f) || dur_cap < 0 || dur_cap > (int64_t)1 << 20 || !dur_eff) return -2;
    launch_durations_prosody(log_d, tok_off, tok_len, B, alpha, alpha_b, partial, dur_cap, cu_seqlens, dur_packed, dur_eff, logd_packed, centre_rows,
                             mel_len, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_gauss_upsample(const float* xvar, const float* centre_rows, const int32_t* tok_off, const int32_t* tok_len, const int32_t* frm_row_seq,
                         const int32_t* frm_row_pos, const float* pe, float pe_alpha, float delta, float* out, float* tap_out, int rows, int C,
                         void* stream) {
    if (rows <= 0 || C <= 0 || C > 512 || C % 2 || !(delta > 0.f)) return -2;      // acc[4]: four float2 chunks of 128 channels per lane
    launch_gauss_upsample(xvar, centre_rows, tok_off, tok_len, frm_row_seq, frm_row_pos, pe, pe_alpha, delta, out, tap_out, rows, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_mel_to_rows(const void* mel, int is_f16, const int64_t* mel_elem_off, const int32_t* frm_row_seq, const int32_t* frm_row_pos,
                      const int32_t* mel_len, void* out, int out_f32, int rows, int n_mels, int ldo, void* stream) {
    if (rows <= 0 || n_mels <= 0 || ldo < n_mels) return -2;
    launch_mel_to_rows(mel, is_f16, mel_elem_off, frm_row_seq, frm_row_pos, mel_len, out, out_f32, rows, n_mels, ldo, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_conv_post(const void* x, int is_f32, int ldx, const float* w, float bias, int k, float pre_slope, const uint8_t* row_valid, int valid_shift,
                    float* wav_rows, int rows, int C, void* stream) {
    if (rows <= 0 || C != 32 || k < 1 || k > 15 || k % 2 == 0 || ldx < C || ldx % (is_f32 ? 4 : 8)) return -2;      // 16 taps of weights and 256 + 16 rows fit the LDS
    if (!row_valid || valid_shift < 0 || valid_shift > 30 || !(pre_slope >= 0.f && pre_slope <= 1.f)) return -2;  // max(v, s v) form of leaky-relu
    launch_conv_post(x, is_f32, ldx, w, bias, k, pre_slope, row_valid, valid_shift, wav_rows, rows, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_row_maps(const int32_t* off, const int32_t* len, int B, int32_t* seq, int32_t* pos, uint8_t* valid, int rows, void* stream) {
    if (rows <= 0 || B <= 0) return -2;
    launch_row_maps(off, len, B, seq, pos, valid, rows, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_pack_rows(const void* src, int is_f16, int ld, int C, const int64_t* seq_row_off, const int64_t* seq_out_off, const int32_t* seq_rows, int B,
                    int64_t max_rows, float* dst, void* stream) {
    if (B <= 0 || B > 65535 || C <= 0 || ld < C || max_rows < 0) return -2;
    launch_pack_rows(src, is_f16 ? DT_F16 : DT_F32, ld, C, seq_row_off, seq_out_off, seq_rows, B, max_rows, dst, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_wav_to_i16(const float* wav, int16_t* out, int64_t n, void* stream) {
    if (n <= 0) return -2;
    launch_wav_to_i16(wav, out, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_pe_extend(float* pe, const float* div, int row0, int row1, int C, void* stream) {
    if (row0 < 0 || row1 <= row0 || C <= 0 || C % 2) return -2;
    launch_pe_extend(pe, div, row0, row1, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}}  // extern "C"
