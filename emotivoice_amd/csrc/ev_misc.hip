// Non-GEMM kernels of the EmotiVoice hot path for gfx950 (wave = 64 lanes).
// All activations are channels-last [rows][channels]; "rows" follow the gap layout described in
// DESIGN.md (utterances separated by >= 4 zero rows; invalid rows are always written as zeros).
#include <hip/hip_fp16.h>
#include <stdlib.h>

#include "ev_kernels.h"
#include "ev_mxq.h"

namespace ev {

// maximum over lanes l, l ^ 16, l ^ 32, l ^ 48 (the four 16-lane rows of a wave) without the LDS pipe: v_permlane32_swap / v_permlane16_swap
// on two copies of the value leave {lower half, lower half} and {upper half, upper half}; their maximum is the xor reduction on every lane.
// (__shfl_xor is ds_bpermute_b32: two dependent LDS round trips per key tile of the attention kernels.  Inline asm: hipcc's builtin folded the
// second result away.)
__device__ __forceinline__ float rows_max(float v) {
    float a = v, b = v;
    asm("s_nop 1\n\tv_permlane32_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    a = fmaxf(a, b); b = a;
    asm("s_nop 1\n\tv_permlane16_swap_b32 %0, %1" : "+v"(a), "+v"(b));
    return fmaxf(a, b);
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_min_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = min(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ int wave_max_i(int v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = max(v, __shfl_xor(v, o));
    return v;
}

// ------------------------------------------------------------------ LayerNorm (+ optional dot head)
// reference modules/encoder.py:112-127 (eps = 1e-12); variance.py:29-33 (channel LN in predictors);
// variance.py:46,119 (Linear(C,1) head fused as dot_w/dot_b).  One wave per row, C % 128 == 0; NV = float2 chunks per lane
// (4: C <= 512, the acoustic model; 8: C <= 1024, the SimBERT encoder's 768).
// PLANES: the output is (also) written as the MX plane set its DT_MX consumer reads (LayerNormParams::mxo_*: the mel decoder's QKV projection and conv-FFN
// in the mx mode) -- bit for bit what mx_planes_kernel makes of the fp32 output, without that tensor pass: a lane's two channels are one byte of each code
// plane (the four lanes of a quad gather theirs into one dword), a 32-channel block is one 16-lane DPP row (block maxima by quad / row-mirror permutes).
__device__ __forceinline__ int dpp_quad_xor1(int v) { return __builtin_amdgcn_mov_dpp(v, 0xB1, 0xF, 0xF, true); }
__device__ __forceinline__ int dpp_quad_xor2(int v) { return __builtin_amdgcn_mov_dpp(v, 0x4E, 0xF, 0xF, true); }
__device__ __forceinline__ float row16_max(float v) {          // maximum over the 16 lanes of a DPP row (v >= 0)
    v = fmaxf(v, __int_as_float(dpp_quad_xor1(__float_as_int(v))));
    v = fmaxf(v, __int_as_float(dpp_quad_xor2(__float_as_int(v))));
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x141, 0xF, 0xF, true)));      // row_half_mirror: quads 0 <-> 1, 2 <-> 3
    v = fmaxf(v, __int_as_float(__builtin_amdgcn_mov_dpp(__float_as_int(v), 0x140, 0xF, 0xF, true)));      // row_mirror: the two halves
    return v;
}
template <int NV, bool PLANES>
__global__ __launch_bounds__(256) void layernorm_kernel(const LayerNormParams p) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= p.rows) return;
    const int nv = p.C >> 7;   // float2 chunks per lane
    const bool valid = p.row_valid ? p.row_valid[row] != 0 : true;
    float2 v[NV], gv[NV], bv[NV];
    float s = 0.f;
    const float* xr = p.x + (long)row * p.ldx;
    // (round 6) gamma / beta requested WITH the row, not behind the two wave reductions: one exposed memory round trip per wave instead of two (same values,
    // same arithmetic: bit-identical output)
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i < nv) {
            v[i] = *reinterpret_cast<const float2*>(xr + i * 128 + lane * 2);
            gv[i] = *reinterpret_cast<const float2*>(p.gamma + i * 128 + lane * 2);
            bv[i] = *reinterpret_cast<const float2*>(p.beta + i * 128 + lane * 2);
        }
    }
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i < nv) s += v[i].x + v[i].y;
    }
    const float mean = wave_sum(s) / (float)p.C;
    float q = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i < nv) {
            const float a = v[i].x - mean, b = v[i].y - mean;
            q += a * a + b * b;
        }
    }
    const float var = wave_sum(q) / (float)p.C;
    const float rstd = 1.0f / sqrtf(var + p.eps);
    float dot = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        if (i < nv) {
            const int c = i * 128 + lane * 2;
            const float2 g = gv[i], b = bv[i];
            float y0 = (v[i].x - mean) * rstd * g.x + b.x;
            float y1 = (v[i].y - mean) * rstd * g.y + b.y;
            if (!valid) { y0 = 0.f; y1 = 0.f; }
            if (p.dot_w) {
                const float2 w = *reinterpret_cast<const float2*>(p.dot_w + c);
                dot += y0 * w.x + y1 * w.y;
            }
            if (p.out32) *reinterpret_cast<float2*>(p.out32 + (long)row * p.ldo + c) = make_float2(y0, y1);
            if (p.out16) *reinterpret_cast<__half2*>(reinterpret_cast<__half*>(p.out16) + (long)row * p.ldo + c) = __floats2half2_rn(y0, y1);
            if constexpr (PLANES) {
                const _Float16 h0 = (_Float16)y0, h1 = (_Float16)y1;
                const float hf0 = (float)h0, hf1 = (float)h1, lf0 = y0 - hf0, lf1 = y1 - hf1;
                const float mh = row16_max(fmaxf(fabsf(hf0), fabsf(hf1))), ml = row16_max(fmaxf(fabsf(lf0), fabsf(lf1)));
                const unsigned bh = mx_scale_byte(mh), bl = mx_scale_byte(ml);
                const float ih = __uint_as_float((254u - bh) << 23), il = __uint_as_float((254u - bl) << 23);
                unsigned wh = (mx_fp4_code(hf0 * ih) | (mx_fp4_code(hf1 * ih) << 4)) << (8 * (lane & 3));
                unsigned wl = (mx_fp4_code(lf0 * il) | (mx_fp4_code(lf1 * il) << 4)) << (8 * (lane & 3));
                wh |= (unsigned)dpp_quad_xor1((int)wh); wh |= (unsigned)dpp_quad_xor2((int)wh);
                wl |= (unsigned)dpp_quad_xor1((int)wl); wl |= (unsigned)dpp_quad_xor2((int)wl);
                typedef _Float16 h2v __attribute__((ext_vector_type(2)));
                *reinterpret_cast<h2v*>(reinterpret_cast<_Float16*>(p.mxo_h) + (long)row * p.C + c) = h2v{h0, h1};
                if ((lane & 3) == 0) {
                    *reinterpret_cast<unsigned*>(reinterpret_cast<char*>(p.mxo_q4[0]) + (long)row * (p.C >> 1) + i * 64 + lane) = wh;
                    *reinterpret_cast<unsigned*>(reinterpret_cast<char*>(p.mxo_q4[1]) + (long)row * (p.C >> 1) + i * 64 + lane) = wl;
                }
                if ((lane & 15) == 0) {
                    const long so = (long)i * p.mxo_qs_stride + (long)row * 4 + (lane >> 4);
                    reinterpret_cast<uint8_t*>(p.mxo_qs[0])[so] = (uint8_t)bh;
                    reinterpret_cast<uint8_t*>(p.mxo_qs[1])[so] = (uint8_t)bl;
                }
            }
        }
    }
    if (p.dot_w) {
        dot = wave_sum(dot);
        if (lane == 0) p.dot_out[row] = valid ? dot + p.dot_b : 0.f;
    }
}
void launch_layernorm(const LayerNormParams& p, hipStream_t s) {
    if (p.mxo_h && p.C <= 512) hipLaunchKernelGGL((layernorm_kernel<4, true>), dim3((p.rows + 3) / 4), dim3(256), 0, s, p);
    else if (p.C <= 512) hipLaunchKernelGGL((layernorm_kernel<4, false>), dim3((p.rows + 3) / 4), dim3(256), 0, s, p);
    else hipLaunchKernelGGL((layernorm_kernel<8, false>), dim3((p.rows + 3) / 4), dim3(256), 0, s, p);
}

// ------------------------------------------------------------------ SimBERT embeddings + pooler
// reference models/prompt_tts_modified/simbert.py:37,49-55 -> transformers BertEmbeddings: word + position + token-type
// embeddings, summed (the LayerNorm that follows is launch_layernorm with eps from the BERT config).
__global__ __launch_bounds__(256) void bert_embed_kernel(const int64_t* ids, const int64_t* type_ids, const int32_t* cu, const int32_t* row_seq,
                                                         const int32_t* row_pos, const float* word, const float* pos_emb, const float* type_emb,
                                                         int vocab, int max_pos, int n_types, float* out, int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int b = row_seq[row];
    float* o = out + (long)row * C;
    if (b < 0) {
        for (int c = lane * 2; c < C; c += 128) *reinterpret_cast<float2*>(o + c) = make_float2(0.f, 0.f);
        return;
    }
    const int pos = row_pos[row];
    const long tok = min(max(ids[cu[b] + pos], 0L), (long)vocab - 1);
    const long tt = type_ids ? min(max(type_ids[cu[b] + pos], 0L), (long)n_types - 1) : 0L;
    const float* w = word + tok * C;
    const float* pe = pos_emb + (long)min(pos, max_pos - 1) * C;
    const float* te = type_emb + tt * C;
    for (int c = lane * 2; c < C; c += 128) {
        const float2 a = *reinterpret_cast<const float2*>(w + c), p2 = *reinterpret_cast<const float2*>(pe + c), t2 = *reinterpret_cast<const float2*>(te + c);
        // summation order of BertEmbeddings.forward: (inputs_embeds + token_type_embeddings) + position_embeddings
        *reinterpret_cast<float2*>(o + c) = make_float2((a.x + t2.x) + p2.x, (a.y + t2.y) + p2.y);
    }
}
void launch_bert_embed(const int64_t* ids, const int64_t* type_ids, const int32_t* cu, const int32_t* row_seq, const int32_t* row_pos,
                       const float* word, const float* pos_emb, const float* type_emb, int vocab, int max_pos, int n_types, float* out,
                       int rows, int C, hipStream_t s) {
    hipLaunchKernelGGL(bert_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, ids, type_ids, cu, row_seq, row_pos, word, pos_emb, type_emb,
                       vocab, max_pos, n_types, out, rows, C);
}

// BertPooler: pooled[b] = tanh(W h[first token of text b] + bias); one wave per (output channel, text)
__global__ __launch_bounds__(256) void bert_pooler_kernel(const float* x, int ldx, const int32_t* seq_off, const float* W, const float* bias,
                                                          float* out, int C) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= C) return;
    const float* h = x + (long)seq_off[b] * ldx;
    const float* w = W + (long)c * C;
    float a = 0.f;
    for (int i = lane; i < C; i += 64) a = fmaf(w[i], h[i], a);
    a = wave_sum(a);
    if (lane == 0) out[(long)b * C + c] = tanhf(a + bias[c]);
}
void launch_bert_pooler(const float* x, int ldx, const int32_t* seq_off, const float* W, const float* bias, float* out, int B, int C,
                        hipStream_t s) {
    hipLaunchKernelGGL(bert_pooler_kernel, dim3((C + 3) / 4, B), dim3(256), 0, s, x, ldx, seq_off, W, bias, out, C);
}

// ------------------------------------------------------------------ embedding + positional encoding
// reference model_open_source.py:107 (src_word_emb) and modules/encoder.py:257-261 (x + alpha * pe[t])
__global__ __launch_bounds__(256) void embed_pe_kernel(const int64_t* ling, const int32_t* cu, const int32_t* row_seq,
                                                       const int32_t* row_pos, const float* emb, int n_vocab, const float* pe, float alpha,
                                                       float* out, float* tap, int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int b = row_seq[row];
    float* o = out + (long)row * C;
    if (b < 0) {
        for (int c = lane * 2; c < C; c += 128) {
            *reinterpret_cast<float2*>(o + c) = make_float2(0.f, 0.f);
            if (tap) *reinterpret_cast<float2*>(tap + (long)row * C + c) = make_float2(0.f, 0.f);
        }
        return;
    }
    const int pos = row_pos[row];
    // host inputs are range-checked by ev_synthesize (nn.Embedding's IndexError); device inputs cannot be without a sync, so an
    // out-of-range id is clamped instead of reading outside the table
    const long tok = min(max(ling[cu[b] + pos], 0L), (long)n_vocab - 1);
    const float* e = emb + tok * C;
    const float* pr = pe + (long)pos * C;
    for (int c = lane * 2; c < C; c += 128) {
        const float2 ev = *reinterpret_cast<const float2*>(e + c);
        const float2 pv = *reinterpret_cast<const float2*>(pr + c);
        if (tap) *reinterpret_cast<float2*>(tap + (long)row * C + c) = ev;
        *reinterpret_cast<float2*>(o + c) = make_float2(ev.x + alpha * pv.x, ev.y + alpha * pv.y);
    }
}
void launch_embed_pe(const int64_t* ling, const int32_t* cu, const int32_t* row_seq, const int32_t* row_pos, const float* emb,
                     int n_vocab, const float* pe, float alpha, float* out, float* tap_out, int rows, int C, hipStream_t s) {
    hipLaunchKernelGGL(embed_pe_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, ling, cu, row_seq, row_pos, emb, n_vocab, pe, alpha, out,
                       tap_out, rows, C);
}

// ------------------------------------------------------------------ self-attention (fp32 math)
// reference modules/encoder.py:72-109: softmax(q k^T / sqrt(dk)) v, restricted to the utterance's own
// rows (B = 1 semantics; decoder runs with mask=None over its own frames, model_open_source.py:145-146).
// One wave = 64 consecutive queries of one (utterance, head); keys/values are streamed through LDS
// in tiles of 64 with an online softmax (chunks of 8 keys per rescale).
template <typename T, int DK>
__global__ __launch_bounds__(64) void attention_kernel(const AttnParams p) {
    constexpr int KP = DK + 4;   // padded LDS row (floats)
    __shared__ __attribute__((aligned(16))) float Ks[64 * KP];
    __shared__ __attribute__((aligned(16))) float Vs[64 * KP];
    const int b = blockIdx.z, h = blockIdx.y, qt = blockIdx.x;
    const int len = p.seq_len[b];
    if (qt * 64 >= len) return;
    const int lane = threadIdx.x;
    const long row0 = p.seq_off[b];
    const int qi = qt * 64 + lane;
    const bool qvalid = qi < len;
    const T* base = reinterpret_cast<const T*>(p.qkv);
    const float scale = 1.0f / sqrtf((float)DK);

    float q[DK], o[DK];
#pragma unroll
    for (int d = 0; d < DK; ++d) { q[d] = 0.f; o[d] = 0.f; }
    if (qvalid) {
        const T* qp = base + (row0 + qi) * p.ld + h * DK;
#pragma unroll
        for (int d = 0; d < DK; ++d) q[d] = (float)qp[d];
    }
    float m = -INFINITY, l = 0.f;

    for (int k0 = 0; k0 < len; k0 += 64) {
        const int cnt = min(64, len - k0);
        __syncthreads();
        if (lane < cnt) {
            const T* kp = base + (row0 + k0 + lane) * p.ld + p.C + h * DK;
            const T* vp = kp + p.C;
#pragma unroll
            for (int d = 0; d < DK; ++d) {
                Ks[lane * KP + d] = (float)kp[d];
                Vs[lane * KP + d] = (float)vp[d];
            }
        }
        __syncthreads();
        for (int j0 = 0; j0 < cnt; j0 += 8) {
            float sc[8];
            float cm = -INFINITY;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int j = j0 + jj;
                float a = 0.f;
                if (j < cnt) {
                    const float4* kr = reinterpret_cast<const float4*>(Ks + j * KP);
#pragma unroll
                    for (int d4 = 0; d4 < DK / 4; ++d4) {
                        const float4 kv = kr[d4];
                        a = fmaf(q[4 * d4 + 0], kv.x, a);
                        a = fmaf(q[4 * d4 + 1], kv.y, a);
                        a = fmaf(q[4 * d4 + 2], kv.z, a);
                        a = fmaf(q[4 * d4 + 3], kv.w, a);
                    }
                    a *= scale;
                } else {
                    a = -INFINITY;
                }
                sc[jj] = a;
                cm = fmaxf(cm, a);
            }
            const float mn = fmaxf(m, cm);
            const float alpha = expf(m - mn);   // m = -inf on the first chunk -> 0
            l *= alpha;
#pragma unroll
            for (int d = 0; d < DK; ++d) o[d] *= alpha;
            m = mn;
#pragma unroll
            for (int jj = 0; jj < 8; ++jj) {
                const int j = j0 + jj;
                if (j < cnt) {
                    const float pj = expf(sc[jj] - m);
                    l += pj;
                    const float4* vr = reinterpret_cast<const float4*>(Vs + j * KP);
#pragma unroll
                    for (int d4 = 0; d4 < DK / 4; ++d4) {
                        const float4 vv = vr[d4];
                        o[4 * d4 + 0] = fmaf(pj, vv.x, o[4 * d4 + 0]);
                        o[4 * d4 + 1] = fmaf(pj, vv.y, o[4 * d4 + 1]);
                        o[4 * d4 + 2] = fmaf(pj, vv.z, o[4 * d4 + 2]);
                        o[4 * d4 + 3] = fmaf(pj, vv.w, o[4 * d4 + 3]);
                    }
                }
            }
        }
    }
    if (qvalid) {
        const float inv = 1.0f / l;
        T* op = reinterpret_cast<T*>(p.out) + (row0 + qi) * p.ldo + h * DK;
#pragma unroll
        for (int d = 0; d < DK; ++d) op[d] = (T)(o[d] * inv);
    }
}
// ---- fp16 MFMA flash attention (decoder): 128 queries per block (4 waves x 2 tiles of 16), keys/values streamed in
// tiles of 64 through double-buffered LDS, online softmax in registers.
// Both products are computed TRANSPOSED so that probabilities never leave registers:
//   S^T[key][query] = K . Q^T   (A = K tile rows, B = Q fragment held in registers for the whole kernel;
//                                d_k = 48 = one 16x16x32 MFMA + one 16x16x16 MFMA)
//   O^T[d][query]  += V^T . P^T (A = V^T from LDS, B = P packed straight from the S^T accumulators)
// The MFMA C layout gives lane (query j, group g) the keys {16*kt + 4g + r}; the k-slot order of the P.V MFMA is
// permuted to exactly that set (slots 0-3: keys 32*kb + 4g + r, slots 4-7: keys 32*kb + 16 + 4g + r), which only
// requires V^T to be read with the same permutation (two 8-byte LDS reads) -- any k permutation applied to both
// operands leaves the product unchanged.  The softmax max/sum of a query lives in the 4 lanes (j, g=0..3): two
// shuffles per tile.  reference: modules/encoder.py:72-109 (mask = None / all-valid for B = 1).
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef float f4 __attribute__((ext_vector_type(4)));

__global__ __launch_bounds__(256) void attention_mfma_kernel(const AttnParams p) {
    constexpr int DK = 48, KP = 112, VP = 144;         // LDS pitches (bytes): K rows 96 B + 16, V^T rows 128 B + 16
    constexpr int KBYTES = 64 * KP, VBYTES = DK * VP;
    __shared__ __attribute__((aligned(16))) char lds[2 * (KBYTES + VBYTES)];
    const int b = blockIdx.z, h = blockIdx.y, qblk = blockIdx.x;
    const int len = p.seq_len[b];
    if (qblk * 128 >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fg = lane >> 4;
    const long row0 = p.seq_off[b];
    const _Float16* base = reinterpret_cast<const _Float16*>(p.qkv);

    h8 q32[2];
    h4 q16[2];
    int qrow[2];
#pragma unroll
    for (int nq = 0; nq < 2; ++nq) {
        qrow[nq] = qblk * 128 + wave * 32 + nq * 16 + fr;
        const int qc = min(qrow[nq], len - 1);
        const _Float16* qp = base + (row0 + qc) * p.ld + h * DK;
        q32[nq] = *reinterpret_cast<const h8*>(qp + 8 * fg);
        q16[nq] = *reinterpret_cast<const h4*>(qp + 32 + 4 * fg);
    }
    const h4 zero4 = h4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    const h8 q16w[2] = {__builtin_shufflevector(q16[0], zero4, 0, 1, 2, 3, 4, 5, 6, 7), __builtin_shufflevector(q16[1], zero4, 0, 1, 2, 3, 4, 5, 6, 7)};
    const float scale2 = 1.4426950408889634f / sqrtf((float)DK);    // log2(e) / sqrt(d_k): softmax in base 2

    // staging: 64 keys x 96 B = 384 16-byte chunks for K and for V; 256 threads -> chunk tid and (tid < 128) chunk tid + 256
    const int ntiles = (len + 63) >> 6;
    // (scalar staging registers + macros: uint4 arrays captured by lambdas end up in scratch with hipcc)
    uint4 kr0, kr1 = make_uint4(0, 0, 0, 0), vr0, vr1 = make_uint4(0, 0, 0, 0);
    const int c1 = tid + 256;                       // second chunk, valid for tid < 128
    const int key_a = tid / 6, part_a = tid % 6, key_b = c1 / 6, part_b = c1 % 6;
    const long col_a = p.C + h * DK + part_a * 8, col_b = p.C + h * DK + part_b * 8;
#define EV_AT_GLOAD(T)                                                                                   \
    {                                                                                                    \
        const _Float16* kp_ = base + (row0 + min((T) * 64 + key_a, len - 1)) * p.ld + col_a;             \
        kr0 = *reinterpret_cast<const uint4*>(kp_);                                                      \
        vr0 = *reinterpret_cast<const uint4*>(kp_ + p.C);                                                \
        if (tid < 128) {                                                                                 \
            const _Float16* kq_ = base + (row0 + min((T) * 64 + key_b, len - 1)) * p.ld + col_b;         \
            kr1 = *reinterpret_cast<const uint4*>(kq_);                                                  \
            vr1 = *reinterpret_cast<const uint4*>(kq_ + p.C);                                            \
        }                                                                                                \
    }
#define EV_AT_SSTORE1(KR, VR, KEY, PART, KB_, VB_)                                                       \
    {                                                                                                    \
        *reinterpret_cast<uint4*>((KB_) + (KEY) * KP + (PART) * 16) = KR;                                \
        const h8 hv_ = *reinterpret_cast<const h8*>(&VR);                                                \
        /* V^T rows 8 apart are 1152 bytes = 288 dwords = 0 mod 32 banks apart: the six parts of one key hit ONE bank (the 61 % */ \
        /* SQ_LDS_BANK_CONFLICT / SQ_LDS_IDX_ACTIVE of profiles/r2_d).  The key index is XOR-ed with 4 * (row >> 3): banks 0, 2, ... 10; */ \
        /* the 4-key groups the P.V fragment reads stay contiguous (the reads apply the same XOR). */ \
        _Pragma("unroll") for (int e = 0; e < 8; ++e)                                                    \
            *reinterpret_cast<_Float16*>((VB_) + ((PART) * 8 + e) * VP + (((KEY) ^ ((PART) << 2)) * 2)) = hv_[e]; \
    }
#define EV_AT_SSTORE(BUF)                                                                                \
    {                                                                                                    \
        char* Kb_ = lds + (BUF) * (KBYTES + VBYTES);                                                     \
        char* Vb_ = Kb_ + KBYTES;                                                                        \
        EV_AT_SSTORE1(kr0, vr0, key_a, part_a, Kb_, Vb_)                                                 \
        if (tid < 128) EV_AT_SSTORE1(kr1, vr1, key_b, part_b, Kb_, Vb_)                                  \
    }

    float m[2] = {-INFINITY, -INFINITY}, l[2] = {0.f, 0.f};
    f4 o[2][3];
#pragma unroll
    for (int nq = 0; nq < 2; ++nq)
#pragma unroll
        for (int dt = 0; dt < 3; ++dt) o[nq][dt] = f4{0.f, 0.f, 0.f, 0.f};

    EV_AT_GLOAD(0)
    EV_AT_SSTORE(0)
    __syncthreads();
    for (int t = 0; t < ntiles; ++t) {
        const bool more = t + 1 < ntiles;
        if (more) EV_AT_GLOAD(t + 1)
        const char* Kb = lds + (t & 1) * (KBYTES + VBYTES);
        const char* Vb = Kb + KBYTES;
        f4 s[2][4];
#pragma unroll
        for (int kt = 0; kt < 4; ++kt) {
            const h8 ka32 = *reinterpret_cast<const h8*>(Kb + (kt * 16 + fr) * KP + 16 * fg);
            const h4 ka16 = *reinterpret_cast<const h4*>(Kb + (kt * 16 + fr) * KP + 64 + 8 * fg);
            const h8 ka16w = __builtin_shufflevector(ka16, zero4, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
            for (int nq = 0; nq < 2; ++nq) {
                // d_k = 48 = one full K = 32 MFMA + one with a zero half.  NOT a K = 32 followed by the legacy 16x16x16 form on the same accumulator: that
                // chain loses products on the MI355X unless >= 5 wait states separate the two (tools/mfma_chain_check.hip, profiles/r5_a_mfma_chain_check.txt:
                // wrong with 0 and 4 states, exact from 5), and hipcc pads its own builtins with none (tests/test_isa_hazards.py keeps such a chain out of the library)
                f4 z = f4{0.f, 0.f, 0.f, 0.f};
                z = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka32, q32[nq], z, 0, 0, 0);
                s[nq][kt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ka16w, q16w[nq], z, 0, 0, 0);
            }
        }
        h8 pb[2][2];
        const int key0 = t * 64 + 4 * fg;
#pragma unroll
        for (int nq = 0; nq < 2; ++nq) {
            float mx = -INFINITY;
            if (more) {                       // only the last key tile can reach past the utterance: no per-element compare elsewhere
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const float v = s[nq][kt][r] * scale2;
                        s[nq][kt][r] = v;
                        mx = fmaxf(mx, v);
                    }
            } else {
#pragma unroll
                for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        float v = s[nq][kt][r] * scale2;
                        if (key0 + kt * 16 + r >= len) v = -INFINITY;
                        s[nq][kt][r] = v;
                        mx = fmaxf(mx, v);
                    }
            }
            mx = rows_max(mx);
            const float mn = fmaxf(m[nq], mx);
            const float alpha = __builtin_amdgcn_exp2f(m[nq] - mn);
            m[nq] = mn;
            float ps = 0.f;
#pragma unroll
            for (int kt = 0; kt < 4; ++kt)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float pv = __builtin_amdgcn_exp2f(s[nq][kt][r] - mn);
                    s[nq][kt][r] = pv;
                    ps += pv;
                }
            l[nq] = l[nq] * alpha + ps;
#pragma unroll
            for (int dt = 0; dt < 3; ++dt) o[nq][dt] *= alpha;
#pragma unroll
            for (int kb = 0; kb < 2; ++kb) {
                h8 pk;
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    pk[r] = (_Float16)s[nq][2 * kb][r];
                    pk[4 + r] = (_Float16)s[nq][2 * kb + 1][r];
                }
                pb[nq][kb] = pk;
            }
        }
#pragma unroll
        for (int kb = 0; kb < 2; ++kb)
#pragma unroll
            for (int dt = 0; dt < 3; ++dt) {
                const int vrow = dt * 16 + fr, vx = (vrow >> 3) << 2;          // the staging XOR (see EV_AT_SSTORE1)
                const char* vp = Vb + vrow * VP;
                const h4 lo = *reinterpret_cast<const h4*>(vp + (((kb * 32 + 4 * fg) ^ vx) * 2));
                const h4 hi = *reinterpret_cast<const h4*>(vp + (((kb * 32 + 16 + 4 * fg) ^ vx) * 2));
                const h8 va = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
#pragma unroll
                for (int nq = 0; nq < 2; ++nq) o[nq][dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(va, pb[nq][kb], o[nq][dt], 0, 0, 0);
            }
        if (more) EV_AT_SSTORE((t + 1) & 1)
        __syncthreads();
    }
#undef EV_AT_GLOAD
#undef EV_AT_SSTORE
#undef EV_AT_SSTORE1
#pragma unroll
    for (int nq = 0; nq < 2; ++nq) {
        float lt = l[nq];
        lt += __shfl_xor(lt, 16);
        lt += __shfl_xor(lt, 32);
        const float inv = 1.0f / lt;
        if (qrow[nq] < len) {
            _Float16* op = reinterpret_cast<_Float16*>(p.out) + (row0 + qrow[nq]) * p.ldo + h * DK + 4 * fg;
#pragma unroll
            for (int dt = 0; dt < 3; ++dt) {
                h4 ov;
#pragma unroll
                for (int r = 0; r < 4; ++r) ov[r] = (_Float16)(o[nq][dt][r] * inv);
                *reinterpret_cast<h4*>(op + dt * 16) = ov;
            }
        }
    }
}

// ---- fp32 MFMA flash attention (text encoder, strict-fp32 decoder): exact fp32 products on v_mfma_f32_16x16x4_f32.
// The VALU kernel above keeps one query per lane and walks the keys serially (142 us per encoder layer at 32 x 256 tokens,
// a pure latency chain); here one wave owns 16 queries and a 16-key tile is two small GEMMs:
//     S^T[key][query] = K_tile . Q^T        (12 MFMAs: d_k = 48 = 12 x 4)
//     O^T[d][query]  += V_tile^T . P^T      (3 d-tiles x 4 MFMAs)
// computed transposed so that the probabilities never leave the registers: the C layout of S^T gives lane (query = lane % 16,
// g = lane / 16) the keys 4 g + i, and the B operand of the second product wants, at reduction step i, exactly
// "key 4 g + i of query lane % 16" when the step's four reduction slots are mapped to keys {i, 4 + i, 8 + i, 12 + i}.  The
// reduction index of the first product is permuted the same way (slot g of step j = dim 12 g + j), which makes the Q / K
// operands three contiguous float4 loads per lane.  Online softmax per query: 2 cross-lane shuffles per tile.
template <int DK>
__global__ __launch_bounds__(256) void attention_mfma_f32_kernel(const AttnParams p) {
    static_assert(DK % 16 == 0, "d_k = 48 (acoustic model): 12 reduction steps of 4, 3 output tiles of 16; d_k = 64 (SimBERT): 16 / 4");
    constexpr int NJ = DK / 4, ND = DK / 16, NC = NJ / 4;      // reduction steps, output tiles, float4 loads per lane
    const int b = blockIdx.z, h = blockIdx.y;
    const int len = p.seq_len[b];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.x * 64 + wave * 16;
    if (q0 >= len) return;
    const int fr = lane & 15, g = lane >> 4;
    const long row0 = p.seq_off[b];
    const float* base = reinterpret_cast<const float*>(p.qkv);
    const float scale = 1.0f / sqrtf((float)DK);

    float qv[NJ];
    {
        const int qi = min(q0 + fr, len - 1);
        const float4* qp = reinterpret_cast<const float4*>(base + (row0 + qi) * p.ld + h * DK + g * NJ);
#pragma unroll
        for (int c = 0; c < NC; ++c) { const float4 t = qp[c]; qv[4 * c] = t.x * scale; qv[4 * c + 1] = t.y * scale; qv[4 * c + 2] = t.z * scale; qv[4 * c + 3] = t.w * scale; }
    }
    f4 o[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) o[dt] = f4{0.f, 0.f, 0.f, 0.f};
    float m = -INFINITY, l = 0.f;

    float kv[NJ], vv[ND][4];
    const int ntile = (len + 15) >> 4;
#define EV_ATT_LOAD(KT)                                                                                        \
    {                                                                                                          \
        const int kr_ = min((KT) * 16 + fr, len - 1);                                                          \
        const float4* kp_ = reinterpret_cast<const float4*>(base + (row0 + kr_) * p.ld + p.C + h * DK + g * NJ); \
        _Pragma("unroll") for (int c = 0; c < NC; ++c) { const float4 t = kp_[c]; kv[4 * c] = t.x; kv[4 * c + 1] = t.y; kv[4 * c + 2] = t.z; kv[4 * c + 3] = t.w; } \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                        \
            const float* vp_ = base + (row0 + min((KT) * 16 + 4 * g + i, len - 1)) * p.ld + 2 * p.C + h * DK + fr; \
            _Pragma("unroll") for (int dt = 0; dt < ND; ++dt) vv[dt][i] = vp_[dt * 16];                          \
        }                                                                                                      \
    }
    EV_ATT_LOAD(0)
    for (int kt = 0; kt < ntile; ++kt) {
        // S^T tile
        f4 st = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int j = 0; j < NJ; ++j) st = __builtin_amdgcn_mfma_f32_16x16x4f32(kv[j], qv[j], st, 0, 0, 0);
        float vcur[ND][4];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
#pragma unroll
            for (int i = 0; i < 4; ++i) vcur[dt][i] = vv[dt][i];
        if (kt + 1 < ntile) EV_ATT_LOAD(kt + 1)          // next tile's K / V rows arrive under this tile's softmax and PV
        // mask keys beyond the utterance, online softmax over the 16 keys of this tile (4 per lane x 4 lane groups)
        float sc[4];
        float cm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sc[i] = (kt * 16 + 4 * g + i < len) ? st[i] : -INFINITY;
            cm = fmaxf(cm, sc[i]);
        }
        cm = rows_max(cm);
        const float mn = fmaxf(m, cm);
        const float alpha = expf(m - mn);            // m = -inf on the first tile -> 0
        m = mn;
        float pr[4];
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { pr[i] = expf(sc[i] - mn); ps += pr[i]; }
        l = l * alpha + ps;                          // per-lane partial row sum; the 4 lane groups are added at the end
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            o[dt] *= alpha;
#pragma unroll
            for (int i = 0; i < 4; ++i) o[dt] = __builtin_amdgcn_mfma_f32_16x16x4f32(vcur[dt][i], pr[i], o[dt], 0, 0, 0);
        }
    }
#undef EV_ATT_LOAD
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (q0 + fr < len) {
        const float inv = 1.0f / l;
        float* op = reinterpret_cast<float*>(p.out) + (row0 + q0 + fr) * p.ldo + h * DK + 4 * g;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt)
            *reinterpret_cast<float4*>(op + dt * 16) = make_float4(o[dt][0] * inv, o[dt][1] * inv, o[dt][2] * inv, o[dt][3] * inv);
    }
}

// ---- split-precision MFMA flash attention (mel decoder in the strict / mx modes; round 3).  Same structure, operand permutation and online
// softmax as attention_mfma_f32_kernel, but every product runs on the fp16 pipe as three MFMAs on hi / lo halves
//     x = xh + 2^-11 xl,  xh = fp16(x),  xl = fp16((x - xh) 2^11):      a.b = ah.bh + 2^-11 (ah.bl + al.bh) + O(2^-22)
// (the arithmetic of conv_gemm_split_kernel): v_mfma_f32_16x16x16_f16 holds FOUR consecutive reduction slots per lane, which are exactly the
// four registers the fp32 kernel feeds to four 16x16x4 steps (qv[4 s .. 4 s + 3] / the keys 4 g + i of the P.V product), so the operands are
// plain register packs.  Per 16-key tile: 9 + 9 fp16 MFMAs at the 16x rate instead of 12 + 12 fp32 ones; the exact-fp32 kernel stays for the
// token-rate encoder (its output decides the bit-exact durations) and SimBERT.
typedef _Float16 h4 __attribute__((ext_vector_type(4)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
__device__ __forceinline__ void split4(const float* x, h4& hi, h4& lo) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const _Float16 h = (_Float16)x[i];
        hi[i] = h;
        lo[i] = (_Float16)((x[i] - (float)h) * 2048.0f);
    }
}
template <int DK>
__global__ __launch_bounds__(256) void attention_mfma_x3_kernel(const AttnParams p) {
    static_assert(DK % 16 == 0, "d_k = 48: 3 reduction steps of 16, 3 output tiles of 16");
    constexpr int NJ = DK / 4, ND = DK / 16, NC = NJ / 4, NS = DK / 16;
    const int b = blockIdx.z, h = blockIdx.y;
    const int len = p.seq_len[b];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int q0 = blockIdx.x * 64 + wave * 16;
    if (q0 >= len) return;
    const int fr = lane & 15, g = lane >> 4;
    const long row0 = p.seq_off[b];
    const float* base = reinterpret_cast<const float*>(p.qkv);
    const float scale = 1.0f / sqrtf((float)DK);
    constexpr float LO = 1.0f / 2048.0f;

    h4 qh[NS], ql[NS];
    {
        const int qi = min(q0 + fr, len - 1);
        const float4* qp = reinterpret_cast<const float4*>(base + (row0 + qi) * p.ld + h * DK + g * NJ);
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            const float4 t = qp[c];
            const float x[4] = {t.x * scale, t.y * scale, t.z * scale, t.w * scale};
            split4(x, qh[c], ql[c]);
        }
    }
    f4 oh[ND], ox[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) { oh[dt] = f4{0.f, 0.f, 0.f, 0.f}; ox[dt] = f4{0.f, 0.f, 0.f, 0.f}; }
    float m = -INFINITY, l = 0.f;
    float kv[NJ], vv[ND][4];
    const int ntile = (len + 15) >> 4;
#define EV_ATX_LOAD(KT)                                                                                        \
    {                                                                                                          \
        const int kr_ = min((KT) * 16 + fr, len - 1);                                                          \
        const float4* kp_ = reinterpret_cast<const float4*>(base + (row0 + kr_) * p.ld + p.C + h * DK + g * NJ); \
        _Pragma("unroll") for (int c = 0; c < NC; ++c) { const float4 t = kp_[c]; kv[4 * c] = t.x; kv[4 * c + 1] = t.y; kv[4 * c + 2] = t.z; kv[4 * c + 3] = t.w; } \
        _Pragma("unroll") for (int i = 0; i < 4; ++i) {                                                        \
            const float* vp_ = base + (row0 + min((KT) * 16 + 4 * g + i, len - 1)) * p.ld + 2 * p.C + h * DK + fr; \
            _Pragma("unroll") for (int dt = 0; dt < ND; ++dt) vv[dt][i] = vp_[dt * 16];                          \
        }                                                                                                      \
    }
    EV_ATX_LOAD(0)
    for (int kt = 0; kt < ntile; ++kt) {
        f4 sh = f4{0.f, 0.f, 0.f, 0.f}, sx = f4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            h4 kh, kl;
            split4(kv + 4 * c, kh, kl);
            sh = __builtin_amdgcn_mfma_f32_16x16x16f16(kh, qh[c], sh, 0, 0, 0);
            sx = __builtin_amdgcn_mfma_f32_16x16x16f16(kh, ql[c], sx, 0, 0, 0);
            sx = __builtin_amdgcn_mfma_f32_16x16x16f16(kl, qh[c], sx, 0, 0, 0);
        }
        h4 vh[ND], vl[ND];
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) split4(vv[dt], vh[dt], vl[dt]);
        if (kt + 1 < ntile) EV_ATX_LOAD(kt + 1)          // next tile's K / V rows arrive under this tile's softmax and PV
        float sc[4];
        float cm = -INFINITY;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            sc[i] = (kt * 16 + 4 * g + i < len) ? sh[i] + sx[i] * LO : -INFINITY;
            cm = fmaxf(cm, sc[i]);
        }
        cm = rows_max(cm);
        const float mn = fmaxf(m, cm);
        const float alpha = expf(m - mn);            // m = -inf on the first tile -> 0
        m = mn;
        float pr[4];
        float ps = 0.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { pr[i] = expf(sc[i] - mn); ps += pr[i]; }
        l = l * alpha + ps;
        h4 ph, pl;
        split4(pr, ph, pl);
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            oh[dt] *= alpha; ox[dt] *= alpha;
            oh[dt] = __builtin_amdgcn_mfma_f32_16x16x16f16(vh[dt], ph, oh[dt], 0, 0, 0);
            ox[dt] = __builtin_amdgcn_mfma_f32_16x16x16f16(vh[dt], pl, ox[dt], 0, 0, 0);
            ox[dt] = __builtin_amdgcn_mfma_f32_16x16x16f16(vl[dt], ph, ox[dt], 0, 0, 0);
        }
    }
#undef EV_ATX_LOAD
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (q0 + fr < len) {
        const float inv = 1.0f / l;
        float* op = reinterpret_cast<float*>(p.out) + (row0 + q0 + fr) * p.ldo + h * DK + 4 * g;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            const f4 o = oh[dt] + ox[dt] * LO;
            *reinterpret_cast<float4*>(op + dt * 16) = make_float4(o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv);
        }
    }
}

// ---- the same arithmetic with the K / V tiles shared through LDS.  In the kernel above every wave fetches its own copy of each 16-key tile
// (V as twelve strided dword loads per lane) and splits it itself: 2.6 ms for the four decoder layers at B = 32 x 1024 frames, memory-instruction
// bound (the MFMAs are 5 % of it).  Here a block of four waves (64 queries) stages 32 keys at a time: 768 float4 loads, split ONCE into fp16
// hi / lo planes in the operand layouts -- K row-major [key][48] (pitch 104 B: conflict-free 8-byte fragment reads), V transposed [d][key]
// (pitch 72 B) --, double-buffered, one barrier per stage; a wave's fragments are twelve ds_read_b64 per 16 keys.
// NW waves per block = 16 NW queries per staged K / V tile: 8 waves halve the staging (global loads, hi / lo splits, LDS stores, barriers) per query
template <int DK, int NW>
__global__ __launch_bounds__(64 * NW) void attention_mfma_x3_lds_kernel(const AttnParams p) {
    static_assert(DK == 48, "d_k = 48: 12 float4 per row, 3 reduction steps of 16, 3 output tiles of 16");
    constexpr int NS = DK / 16, ND = DK / 16, KT = 32, KP = 104, VP = 72, NT = 64 * NW, NJ = (768 + NT - 1) / NT;
    constexpr int KB = KT * KP, VB = DK * VP, STAGE = 2 * KB + 2 * VB;       // K hi, K lo, Vt hi, Vt lo
    __shared__ __attribute__((aligned(16))) char lds[2 * STAGE];
    const int b = blockIdx.z, h = blockIdx.y;
    const int len = p.seq_len[b];
    if ((int)blockIdx.x * 16 * NW >= len) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int q0 = blockIdx.x * 16 * NW + wave * 16;
    const int fr = lane & 15, g = lane >> 4;
    const long row0 = p.seq_off[b];
    const float* base = reinterpret_cast<const float*>(p.qkv);
    // scores are kept in log2 units (log2 e folded into the query scale): the softmax is two v_exp_f32 chains shorter per element than with expf
    const float scale = 1.4426950408889634f / sqrtf((float)DK);
    constexpr float LO = 1.0f / 2048.0f;

    h4 qh[NS], ql[NS];
    {
        const int qi = min(q0 + fr, len - 1);
        const float4* qp = reinterpret_cast<const float4*>(base + (row0 + qi) * p.ld + h * DK + g * 12);
#pragma unroll
        for (int c = 0; c < NS; ++c) {
            const float4 t = qp[c];
            const float x[4] = {t.x * scale, t.y * scale, t.z * scale, t.w * scale};
            split4(x, qh[c], ql[c]);
        }
    }
    // d_k = 48 as TWO K = 32 MFMAs per product term, the second one half zeros (the lane's slots 8..11 + four zeros).  Not a 16x16x32 + a legacy 16x16x16
    // on the same accumulator: that mix measured 5e-5 ... 4e-4 and run-to-run differences on the MI355X (a dependent chain across the two opcodes
    // loses cross terms; the legacy form issues at the K = 32 form's 16 cycles anyway, so the zero half costs nothing).
    const h4 z4 = h4{(_Float16)0.f, (_Float16)0.f, (_Float16)0.f, (_Float16)0.f};
    const h8 qh8 = __builtin_shufflevector(qh[0], qh[1], 0, 1, 2, 3, 4, 5, 6, 7), ql8 = __builtin_shufflevector(ql[0], ql[1], 0, 1, 2, 3, 4, 5, 6, 7);
    const h8 qh8b = __builtin_shufflevector(qh[2], z4, 0, 1, 2, 3, 4, 5, 6, 7), ql8b = __builtin_shufflevector(ql[2], z4, 0, 1, 2, 3, 4, 5, 6, 7);
    // staging roles: unit u = tid + NT j (768 units per stage); u < 384: K unit (key u / 12, float4 u % 12), else V unit u - 384
    int ukey[NJ], uc4[NJ];
    bool uv[NJ], uon[NJ];
#pragma unroll
    for (int j = 0; j < NJ; ++j) {
        int u = tid + NT * j;
        uon[j] = u < 768;                      // (wave-uniform: 768 is a multiple of 64)
        u = min(u, 767);
        uv[j] = u >= 384; if (uv[j]) u -= 384; ukey[j] = u / 12; uc4[j] = u % 12;
    }
    float4 st[NJ];
    const int nstage = (len + KT - 1) / KT;
#define EV_ATL_LOAD(S)                                                                                                   \
    _Pragma("unroll") for (int j = 0; j < NJ; ++j) {                                                                     \
        const int kr_ = min((S) * KT + ukey[j], len - 1);                                                                \
        st[j] = *reinterpret_cast<const float4*>(base + (row0 + kr_) * p.ld + (uv[j] ? 2 : 1) * p.C + h * DK + uc4[j] * 4); \
    }
#define EV_ATL_STORE(BUF)                                                                                                \
    _Pragma("unroll") for (int j = 0; j < NJ; ++j) if (uon[j]) {                                                         \
        const float x_[4] = {st[j].x, st[j].y, st[j].z, st[j].w};                                                        \
        h4 hi_, lo_;                                                                                                     \
        split4(x_, hi_, lo_);                                                                                            \
        char* sb_ = lds + (BUF) * STAGE;                                                                                 \
        if (!uv[j]) {                                                                                                    \
            *reinterpret_cast<h4*>(sb_ + ukey[j] * KP + uc4[j] * 8) = hi_;                                               \
            *reinterpret_cast<h4*>(sb_ + KB + ukey[j] * KP + uc4[j] * 8) = lo_;                                          \
        } else {                                                                                                         \
            _Pragma("unroll") for (int e = 0; e < 4; ++e) {                                                              \
                *reinterpret_cast<_Float16*>(sb_ + 2 * KB + (uc4[j] * 4 + e) * VP + ukey[j] * 2) = hi_[e];               \
                *reinterpret_cast<_Float16*>(sb_ + 2 * KB + VB + (uc4[j] * 4 + e) * VP + ukey[j] * 2) = lo_[e];          \
            }                                                                                                            \
        }                                                                                                                \
    }
    f4 oh[ND], ox[ND];
#pragma unroll
    for (int dt = 0; dt < ND; ++dt) { oh[dt] = f4{0.f, 0.f, 0.f, 0.f}; ox[dt] = f4{0.f, 0.f, 0.f, 0.f}; }
    float m = -INFINITY, l = 0.f;
    EV_ATL_LOAD(0)
    EV_ATL_STORE(0)
    __syncthreads();
    for (int sg = 0; sg < nstage; ++sg) {
        if (sg + 1 < nstage) EV_ATL_LOAD(sg + 1)
        const char* sb = lds + (sg & 1) * STAGE;
        // Round 4: the stage's 32 keys as ONE softmax step on the double-K MFMAs.  d_k = 48 is two v_mfma_f32_16x16x32_f16 (slots 0..7 of the lane's 12, then
        // slots 8..11 + zeros) per product term instead of three 16x16x16 -- the legacy K = 16 form issues at the K = 32 form's 16 cycles on gfx950 --,
        // and P.V reduces over all 32 keys in one K = 32 MFMA per (output tile, term): k-slot j of lane group g is key 4 g + j of the first 16-key tile
        // (j < 4) or of the second (j >= 4), which is how the two S^T tiles leave their accumulators, so P still never moves.  36 -> 21 MFMAs per 32 keys
        // and one running-max / rescale pass instead of two.  Keys beyond the utterance (second half of the last stage) get score -inf -> weight 0; their
        // K / V rows are clamped copies of the last key (finite).
        {
            const int kbase = sg * KT;
            f4 sh[2], sx[2];
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf) {
                const char* kp = sb + (hlf * 16 + fr) * KP + g * 24;
                const h4 k0h = *reinterpret_cast<const h4*>(kp), k1h = *reinterpret_cast<const h4*>(kp + 8), k2h = *reinterpret_cast<const h4*>(kp + 16);
                const h4 k0l = *reinterpret_cast<const h4*>(kp + KB), k1l = *reinterpret_cast<const h4*>(kp + KB + 8), k2l = *reinterpret_cast<const h4*>(kp + KB + 16);
                const h8 kh8 = __builtin_shufflevector(k0h, k1h, 0, 1, 2, 3, 4, 5, 6, 7), kl8 = __builtin_shufflevector(k0l, k1l, 0, 1, 2, 3, 4, 5, 6, 7);
                const h8 kh8b = __builtin_shufflevector(k2h, z4, 0, 1, 2, 3, 4, 5, 6, 7), kl8b = __builtin_shufflevector(k2l, z4, 0, 1, 2, 3, 4, 5, 6, 7);
                f4 a = f4{0.f, 0.f, 0.f, 0.f}, x = f4{0.f, 0.f, 0.f, 0.f};
                a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh8, qh8, a, 0, 0, 0);
                a = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh8b, qh8b, a, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh8, ql8, x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_16x16x32_f16(kh8b, ql8b, x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl8, qh8, x, 0, 0, 0);
                x = __builtin_amdgcn_mfma_f32_16x16x32_f16(kl8b, qh8b, x, 0, 0, 0);
                sh[hlf] = a; sx[hlf] = x;
            }
            float sc[8];
            float cm = -INFINITY;
#pragma unroll
            for (int hlf = 0; hlf < 2; ++hlf)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    sc[hlf * 4 + i] = (kbase + hlf * 16 + 4 * g + i < len) ? sh[hlf][i] + sx[hlf][i] * LO : -INFINITY;
                    cm = fmaxf(cm, sc[hlf * 4 + i]);
                }
            cm = rows_max(cm);
            const float mn = fmaxf(m, cm);
            const float alpha = __builtin_amdgcn_exp2f(m - mn);            // (m = -inf on the first stage -> 0)
            m = mn;
            float pr[8];
            float ps = 0.f;
#pragma unroll
            for (int i = 0; i < 8; ++i) { pr[i] = __builtin_amdgcn_exp2f(sc[i] - mn); ps += pr[i]; }
            l = l * alpha + ps;
            h4 p0h, p0l, p1h, p1l;
            split4(pr, p0h, p0l);
            split4(pr + 4, p1h, p1l);
            const h8 ph8 = __builtin_shufflevector(p0h, p1h, 0, 1, 2, 3, 4, 5, 6, 7), pl8 = __builtin_shufflevector(p0l, p1l, 0, 1, 2, 3, 4, 5, 6, 7);
            const char* vp = sb + 2 * KB + fr * VP + (4 * g) * 2;
#pragma unroll
            for (int dt = 0; dt < ND; ++dt) {
                const h4 v0h = *reinterpret_cast<const h4*>(vp + dt * 16 * VP), v1h = *reinterpret_cast<const h4*>(vp + dt * 16 * VP + 32);
                const h4 v0l = *reinterpret_cast<const h4*>(vp + VB + dt * 16 * VP), v1l = *reinterpret_cast<const h4*>(vp + VB + dt * 16 * VP + 32);
                const h8 vh8 = __builtin_shufflevector(v0h, v1h, 0, 1, 2, 3, 4, 5, 6, 7), vl8 = __builtin_shufflevector(v0l, v1l, 0, 1, 2, 3, 4, 5, 6, 7);
                oh[dt] *= alpha; ox[dt] *= alpha;
                oh[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh8, ph8, oh[dt], 0, 0, 0);
                ox[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vh8, pl8, ox[dt], 0, 0, 0);
                ox[dt] = __builtin_amdgcn_mfma_f32_16x16x32_f16(vl8, ph8, ox[dt], 0, 0, 0);
            }
        }
        if (sg + 1 < nstage) EV_ATL_STORE((sg + 1) & 1)        // (the other buffer: its last readers finished before the previous barrier)
        __syncthreads();
    }
#undef EV_ATL_LOAD
#undef EV_ATL_STORE
    l += __shfl_xor(l, 16);
    l += __shfl_xor(l, 32);
    if (q0 + fr < len) {
        const float inv = 1.0f / l;
        float* op = reinterpret_cast<float*>(p.out) + (row0 + q0 + fr) * p.ldo + h * DK + 4 * g;
#pragma unroll
        for (int dt = 0; dt < ND; ++dt) {
            const f4 o = oh[dt] + ox[dt] * LO;
            *reinterpret_cast<float4*>(op + dt * 16) = make_float4(o[0] * inv, o[1] * inv, o[2] * inv, o[3] * inv);
        }
    }
}

void launch_attention(const AttnParams& p, hipStream_t s) {
    if (p.dtype == DT_F32S && p.C / p.heads == 48) {          // fp32 rows, split-precision products (decoder, strict / mx modes)
        static const bool no_lds = tuning_env("EV_ATTN_X3_NOLDS") != nullptr;     // A/B switch: every wave fetches and splits its own tiles
        static const char* nw_env = tuning_env("EV_ATTN_X3_NW");                   // A/B switch: "4" = 64 queries per block
        if (no_lds) hipLaunchKernelGGL((attention_mfma_x3_kernel<48>), dim3((p.max_len + 63) / 64, p.heads, p.B), dim3(256), 0, s, p);
        else if ((nw_env && nw_env[0] == '4') || p.max_len <= 64)
            hipLaunchKernelGGL((attention_mfma_x3_lds_kernel<48, 4>), dim3((p.max_len + 63) / 64, p.heads, p.B), dim3(256), 0, s, p);
        else if ((nw_env && nw_env[0] == '8') || p.max_len <= 128)
            hipLaunchKernelGGL((attention_mfma_x3_lds_kernel<48, 8>), dim3((p.max_len + 127) / 128, p.heads, p.B), dim3(512), 0, s, p);
        else hipLaunchKernelGGL((attention_mfma_x3_lds_kernel<48, 16>), dim3((p.max_len + 255) / 256, p.heads, p.B), dim3(1024), 0, s, p);
        return;
    }
    if (p.dtype == DT_F16) {
        static const bool valu = tuning_env("EV_ATTN_VALU") != nullptr;     // A/B switch: fp32-math VALU kernel on fp16 inputs
        if (!valu) {
            hipLaunchKernelGGL(attention_mfma_kernel, dim3((p.max_len + 127) / 128, p.heads, p.B), dim3(256), 0, s, p);
            return;
        }
        hipLaunchKernelGGL((attention_kernel<_Float16, 48>), dim3((p.max_len + 63) / 64, p.heads, p.B), dim3(64), 0, s, p);
    } else {
        static const bool valu32 = tuning_env("EV_ATTN_VALU") != nullptr;   // A/B switch: the one-query-per-lane VALU kernel
        if (!valu32 && p.C / p.heads == 48) {
            hipLaunchKernelGGL((attention_mfma_f32_kernel<48>), dim3((p.max_len + 63) / 64, p.heads, p.B), dim3(256), 0, s, p);
            return;
        }
        if (p.C / p.heads == 64) {       // SimBERT encoder (12 heads x 64)
            hipLaunchKernelGGL((attention_mfma_f32_kernel<64>), dim3((p.max_len + 63) / 64, p.heads, p.B), dim3(256), 0, s, p);
            return;
        }
        hipLaunchKernelGGL((attention_kernel<float, 48>), dim3((p.max_len + 63) / 64, p.heads, p.B), dim3(64), 0, s, p);
    }
}

// ------------------------------------------------------------------ conditioning vector
// reference model_open_source.py:109-111: the speaker/style/content part of embed_projection1's input is
// constant over time, so its contribution (plus the bias) is one vector per utterance.
__global__ __launch_bounds__(256) void cond_vector_kernel(const int64_t* speaker, const float* style, const float* content,
                                                          const float* spk_emb, int n_speaker, const float* Wcond, const float* bias, float* u,
                                                          int C, int bert) {
    const int b = blockIdx.y;
    const int c = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (c >= C) return;
    const int ncond = C + 2 * bert;
    const float* w = Wcond + (long)c * ncond;
    const float* se = spk_emb + min(max(speaker[b], 0L), (long)n_speaker - 1) * C;      // clamped like the token ids (embed_pe_kernel)
    float a = 0.f;
    for (int i = lane; i < C; i += 64) a = fmaf(w[i], se[i], a);
    for (int i = lane; i < bert; i += 64) a = fmaf(w[C + i], style[(long)b * bert + i], a);
    for (int i = lane; i < bert; i += 64) a = fmaf(w[C + bert + i], content[(long)b * bert + i], a);
    a = wave_sum(a);
    if (lane == 0) u[(long)b * C + c] = a + bias[c];
}
void launch_cond_vector(const int64_t* speaker, const float* style, const float* content, const float* spk_emb, int n_speaker,
                        const float* Wcond, const float* bias, float* u, int B, int C, int bert, hipStream_t s) {
    hipLaunchKernelGGL(cond_vector_kernel, dim3((C + 3) / 4, B), dim3(256), 0, s, speaker, style, content, spk_emb, n_speaker, Wcond,
                       bias, u, C, bert);
}

// ------------------------------------------------------------------ pitch / energy embedding add
// reference model_open_source.py:131-134: Conv1d(1 -> C, k, pad (k-1)/2) on the predicted scalar tracks.
// wp / we are packed [k][C].
__global__ __launch_bounds__(256) void var_embed_add_kernel(const float* x, const float* pitch, const float* energy, const float* wp,
                                                            const float* bp, const float* we, const float* be,
                                                            const uint8_t* row_valid, float* out, int rows, int C, int k) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const bool valid = row_valid[row] != 0;
    const int half = (k - 1) / 2;
    for (int c = lane * 2; c < C; c += 128) {
        float2 r = make_float2(0.f, 0.f);
        if (valid) {
            const float2 xv = *reinterpret_cast<const float2*>(x + (long)row * C + c);
            const float2 b0 = *reinterpret_cast<const float2*>(bp + c);
            const float2 b1 = *reinterpret_cast<const float2*>(be + c);
            float2 ap = b0, ae = b1;
            for (int t = 0; t < k; ++t) {
                const float pv = pitch[row + t - half], evv = energy[row + t - half];
                const float2 w0 = *reinterpret_cast<const float2*>(wp + (long)t * C + c);
                const float2 w1 = *reinterpret_cast<const float2*>(we + (long)t * C + c);
                ap.x = fmaf(w0.x, pv, ap.x); ap.y = fmaf(w0.y, pv, ap.y);
                ae.x = fmaf(w1.x, evv, ae.x); ae.y = fmaf(w1.y, evv, ae.y);
            }
            r.x = xv.x + ap.x + ae.x;
            r.y = xv.y + ap.y + ae.y;
        }
        *reinterpret_cast<float2*>(out + (long)row * C + c) = r;
    }
}
void launch_var_embed_add(const float* x, const float* pitch, const float* energy, const float* wp, const float* bp, const float* we,
                          const float* be, const uint8_t* row_valid, float* out, int rows, int C, int k, hipStream_t s) {
    hipLaunchKernelGGL(var_embed_add_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, x, pitch, energy, wp, bp, we, be, row_valid, out,
                       rows, C, k);
}

// ------------------------------------------------------------------ prosody: effective pitch / energy tracks (ev_synthesize_prosody)
// One thread per token row.  src = the caller's override where one is given and finite (NaN = "predicted"; device inputs: any
// non-finite value), else the prediction (the last predictor LayerNorm's Linear(C, 1) head); then scale * src + shift per utterance
// (ctrl: SoA [5][B] = alpha, pitch_scale, pitch_shift, energy_scale, energy_shift).  An identity transform copies src through
// untouched (fmaf(1, -0, 0) would turn -0 into +0).  Gap rows are written as exact zeros: they are the k = 9 embedding conv's halo.
__global__ __launch_bounds__(256) void prosody_tracks_kernel(const float* pitch, const float* energy, const int32_t* row_seq,
                                                             const int32_t* row_pos, const int32_t* cu, const float* pitch_ovr,
                                                             const float* energy_ovr, const float* ctrl, int B, float* pitch_out,
                                                             float* energy_out, int rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    const int b = row_seq[r];
    if (b < 0) { pitch_out[r] = 0.f; energy_out[r] = 0.f; return; }
    const int j = cu[b] + row_pos[r];
    float p = pitch[r], e = energy[r];
    if (pitch_ovr) { const float v = pitch_ovr[j]; if (isfinite(v)) p = v; }
    if (energy_ovr) { const float v = energy_ovr[j]; if (isfinite(v)) e = v; }
    const float ps = ctrl[B + b], psh = ctrl[2 * B + b], es = ctrl[3 * B + b], esh = ctrl[4 * B + b];
    if (!(ps == 1.0f && psh == 0.0f)) p = fmaf(ps, p, psh);
    if (!(es == 1.0f && esh == 0.0f)) e = fmaf(es, e, esh);
    pitch_out[r] = p;
    energy_out[r] = e;
}
void launch_prosody_tracks(const float* pitch, const float* energy, const int32_t* row_seq, const int32_t* row_pos, const int32_t* cu,
                           const float* pitch_ovr, const float* energy_ovr, const float* ctrl, int B, float* pitch_out, float* energy_out,
                           int rows, hipStream_t s) {
    hipLaunchKernelGGL(prosody_tracks_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, pitch, energy, row_seq, row_pos, cu, pitch_ovr,
                       energy_ovr, ctrl, B, pitch_out, energy_out, rows);
}

// ------------------------------------------------------------------ durations + prefix sum
// reference modules/variance.py:47-51: d = clamp(round(exp(x) - 1), 0) (round-half-even);
// modules/alignment.py:183-202: ds*alpha, all-zero guard, mel_len = int(sum), c = cumsum(ds) - ds/2.
// One 256-thread block per utterance; inclusive scan = wave shuffle scan + cross-wave carry in LDS.
// PROS (ev_synthesize_prosody only; the plain call runs the <false> instantiation, i.e. the code above this extension): alpha_b = the
// per-utterance duration scales (each block takes the integer-scan or the float path by ITS OWN alpha, so that an utterance gets the
// same bits alone and in a mixed batch), partial = per-token overrides (>= 0 forced, clamped to dur_cap; negative = predicted).
// dur_packed keeps the predictions; the durations the length regulator uses go to dur_eff, which the scan below reads.
template <bool PROS>
__global__ __launch_bounds__(256) void durations_kernel(const float* log_d, const int32_t* tok_off, const int32_t* tok_len,
                                                        float alpha, const int64_t* forced, const int32_t* cu, int64_t* dur_packed,
                                                        float* logd_packed, float* centre_rows, int32_t* mel_len,
                                                        const float* alpha_b, const int64_t* partial, int64_t dur_cap, int64_t* dur_eff) {
    __shared__ int wsum[4];
    __shared__ int carry_s;
    __shared__ int total_s;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int off = tok_off[b], n = tok_len[b], c0 = cu[b];
    if (PROS && alpha_b) alpha = alpha_b[b];
    int64_t* const dur_scan = PROS ? dur_eff : dur_packed;
    // pass 1: integer durations + total
    int local = 0;
    for (int j = tid; j < n; j += 256) {
        const float ld = log_d[off + j];
        long d;
        if (forced) d = forced[c0 + j];
        else d = (long)fmaxf(rintf(expf(ld) - 1.0f), 0.0f);
        dur_packed[c0 + j] = d;
        logd_packed[c0 + j] = ld;
        if (PROS) {
            if (partial && partial[c0 + j] >= 0) d = min((long)partial[c0 + j], (long)dur_cap);
            dur_eff[c0 + j] = d;
        }
        local += (int)d;
    }
    int ws = local;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) ws += __shfl_xor(ws, o);
    if (lane == 0) wsum[w] = ws;
    __syncthreads();
    if (tid == 0) { total_s = wsum[0] + wsum[1] + wsum[2] + wsum[3]; carry_s = 0; }
    __syncthreads();
    const bool all_zero = (total_s == 0);   // alignment.py:187-191 (per utterance == B=1 semantics)
    if (alpha == 1.0f) {
        // integer inclusive scan, chunk of 256 tokens at a time (exact; fp32 cumsum of integers is exact too)
        for (int base = 0; base < n; base += 256) {
            const int j = base + tid;
            int d = 0;
            if (j < n) d = all_zero ? 1 : (int)dur_scan[c0 + j];
            int x = d;
#pragma unroll
            for (int o = 1; o < 64; o <<= 1) {
                const int y = __shfl_up(x, o);
                if (lane >= o) x += y;
            }
            if (lane == 63) wsum[w] = x;
            __syncthreads();
            int pre = carry_s;
            for (int i = 0; i < w; ++i) pre += wsum[i];
            const int incl = pre + x;
            if (j < n) centre_rows[off + j] = (float)incl - (float)d / 2.0f;
            __syncthreads();
            if (tid == 255) carry_s = incl;
            __syncthreads();
        }
        if (tid == 0) mel_len[b] = all_zero ? n : total_s;
    } else {
        // general alpha (an extension: the reference's inference branch never scales, model_open_source.py:142): the fp32 products
        // ds * alpha are summed in double and the centre is rounded once (a sequential fp32 running sum was 6e-7 off at 255 tokens,
        // six times the reference's own cumsum: tests/test_gpu_misc_ops.py); the length follows alignment.py:194
        // torch.sum(ds * alpha).int() evaluated in double, so that it does not depend on the order of a float reduction (the CPU
        // oracle does the same)
        if (tid == 0) {
            double tot = 0.0;
            for (int j = 0; j < n; ++j) {
                const float d = all_zero ? 1.0f : (float)dur_scan[c0 + j] * alpha;
                tot += (double)d;
                centre_rows[off + j] = (float)(tot - (double)d * 0.5);
            }
            mel_len[b] = (int)tot;
        }
    }
}
void launch_durations(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const int64_t* forced,
                      const int32_t* cu, int64_t* dur_packed, float* logd_packed, float* centre_rows, int32_t* mel_len,
                      hipStream_t s) {
    hipLaunchKernelGGL(durations_kernel<false>, dim3(B), dim3(256), 0, s, log_d, tok_off, tok_len, alpha, forced, cu, dur_packed,
                       logd_packed, centre_rows, mel_len, nullptr, nullptr, (int64_t)0, nullptr);
}
void launch_durations_prosody(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const float* alpha_b,
                              const int64_t* partial, int64_t dur_cap, const int32_t* cu, int64_t* dur_packed, int64_t* dur_eff,
                              float* logd_packed, float* centre_rows, int32_t* mel_len, hipStream_t s) {
    hipLaunchKernelGGL(durations_kernel<true>, dim3(B), dim3(256), 0, s, log_d, tok_off, tok_len, alpha, (const int64_t*)nullptr, cu,
                       dur_packed, logd_packed, centre_rows, mel_len, alpha_b, partial, dur_cap, dur_eff);
}

// ------------------------------------------------------------------ Gaussian upsampling
// reference modules/alignment.py:204-210: p = softmax_j(-delta (t - c_j)^2); out[t] = sum_j p_j x[j]
// followed by the decoder's x + alpha * pe[t] (modules/encoder.py:257-261).  One wave per frame.
__global__ __launch_bounds__(256) void gauss_upsample_kernel(const float* xvar, const float* centre, const int32_t* tok_off,
                                                             const int32_t* tok_len, const int32_t* row_seq, const int32_t* row_pos,
                                                             const float* pe, float pe_alpha, float delta, float* out, float* tap,
                                                             int rows, int C) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (row >= rows) return;
    const int b = row_seq[row];
    float* o = out + (long)row * C;
    if (b < 0) {
        for (int c = lane * 2; c < C; c += 128) {
            *reinterpret_cast<float2*>(o + c) = make_float2(0.f, 0.f);
            if (tap) *reinterpret_cast<float2*>(tap + (long)row * C + c) = make_float2(0.f, 0.f);
        }
        return;
    }
    const int t = row_pos[row];
    const int off = tok_off[b], n = tok_len[b];
    const float tf = (float)t;
    float mx = -INFINITY;
    for (int j = lane; j < n; j += 64) {
        const float dd = tf - centre[off + j];
        mx = fmaxf(mx, -1.0f * delta * (dd * dd));
    }
    mx = wave_max(mx);
    float sum = 0.f;
    int jlo = n, jhi = -1;
    for (int j = lane; j < n; j += 64) {
        const float dd = tf - centre[off + j];
        const float e = expf(-1.0f * delta * (dd * dd) - mx);
        sum += e;
        if (e > 0.f) { jlo = min(jlo, j); jhi = max(jhi, j); }
    }
    sum = wave_sum(sum);
    jlo = wave_min_i(jlo);
    jhi = wave_max_i(jhi);
    float2 acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = make_float2(0.f, 0.f);
    // (round 6) four token rows requested per round trip instead of one (the loop was load -> wait -> fma per token: 9-40 serial L2 round trips per frame);
    // the products are added in the same token order: bit-identical output
    for (int j = jlo; j <= jhi; j += 4) {
        float pj[4];
        float2 xv[4][4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const int jj = min(j + u, jhi);                 // (wave-uniform; a clamped row is loaded and not used)
            const float dd = tf - centre[off + jj];
            pj[u] = expf(-1.0f * delta * (dd * dd) - mx) / sum;
            const float* xr = xvar + (long)(off + jj) * C;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = i * 128 + lane * 2;
                if (c < C) xv[u][i] = *reinterpret_cast<const float2*>(xr + c);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            if (j + u <= jhi) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = i * 128 + lane * 2;
                    if (c < C) {
                        acc[i].x = fmaf(pj[u], xv[u][i].x, acc[i].x);
                        acc[i].y = fmaf(pj[u], xv[u][i].y, acc[i].y);
                    }
                }
            }
        }
    }
    const float* pr = pe + (long)t * C;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = i * 128 + lane * 2;
        if (c < C) {
            if (tap) *reinterpret_cast<float2*>(tap + (long)row * C + c) = acc[i];
            const float2 pv = *reinterpret_cast<const float2*>(pr + c);
            *reinterpret_cast<float2*>(o + c) = make_float2(acc[i].x + pe_alpha * pv.x, acc[i].y + pe_alpha * pv.y);
        }
    }
}
void launch_gauss_upsample(const float* xvar, const float* centre_rows, const int32_t* tok_off, const int32_t* tok_len,
                           const int32_t* frm_row_seq, const int32_t* frm_row_pos, const float* pe, float pe_alpha, float delta,
                           float* out, float* tap_out, int rows, int C, hipStream_t s) {
    hipLaunchKernelGGL(gauss_upsample_kernel, dim3((rows + 3) / 4), dim3(256), 0, s, xvar, centre_rows, tok_off, tok_len, frm_row_seq,
                       frm_row_pos, pe, pe_alpha, delta, out, tap_out, rows, C);
}

// ------------------------------------------------------------------ mel (B x (n_mels, T)) -> channels-last rows
template <typename TO>
__global__ __launch_bounds__(256) void mel_to_rows_kernel(const void* mel, int is_f16, const int64_t* mel_elem_off,
                                                          const int32_t* row_seq, const int32_t* row_pos, const int32_t* mel_len,
                                                          TO* out, int rows, int n_mels, int ldo) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= (long)rows * ldo) return;
    const int row = (int)(idx / ldo), c = (int)(idx % ldo);
    const int b = row_seq[row];
    float v = 0.f;
    if (b >= 0 && c < n_mels) {
        const long e = mel_elem_off[b] + (long)c * mel_len[b] + row_pos[row];
        v = is_f16 ? __half2float(reinterpret_cast<const __half*>(mel)[e]) : reinterpret_cast<const float*>(mel)[e];
    }
    out[idx] = (TO)v;
}
void launch_mel_to_rows(const void* mel, int is_f16, const int64_t* mel_elem_off, const int32_t* frm_row_seq,
                        const int32_t* frm_row_pos, const int32_t* mel_len, void* out, int out_f32, int rows, int n_mels, int ldo,
                        hipStream_t s) {
    const long n = (long)rows * ldo;
    if (out_f32)
        hipLaunchKernelGGL((mel_to_rows_kernel<float>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mel, is_f16, mel_elem_off,
                           frm_row_seq, frm_row_pos, mel_len, reinterpret_cast<float*>(out), rows, n_mels, ldo);
    else
        hipLaunchKernelGGL((mel_to_rows_kernel<_Float16>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, mel, is_f16, mel_elem_off,
                           frm_row_seq, frm_row_pos, mel_len, reinterpret_cast<_Float16*>(out), rows, n_mels, ldo);
}

// ------------------------------------------------------------------ conv_post + tanh
// reference models/hifigan/models.py:127-129: leaky_relu(0.01) [fused into the producer] -> Conv1d(C->1,k7,p3) -> tanh.
// Block = 256 output samples; the (256 + k - 1) x C fp16 input rows are staged in LDS (80-B pitch).
template <int C, typename T>
__global__ __launch_bounds__(256) void conv_post_kernel(const T* x, int ldx, const float* w, float bias, int k, float pre_slope,
                                                        const uint8_t* row_valid, int valid_shift, float* wav_rows, int rows) {
    constexpr int ES = sizeof(T);
    constexpr int PITCH = C * ES + 16;
    __shared__ __attribute__((aligned(16))) char xs[(256 + 16) * PITCH];
    __shared__ float ws[16 * C];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * 256;
    const int half = (k - 1) / 2;
    const int nrows = 256 + k - 1;
    constexpr int CPR = C * ES / 16;   // 16-B chunks per row
    for (int c = tid; c < nrows * CPR; c += 256) {
        const int r = c / CPR, part = c % CPR;
        *reinterpret_cast<uint4*>(xs + r * PITCH + part * 16) =
            *reinterpret_cast<const uint4*>(reinterpret_cast<const char*>(x) + ((r0 + r - half) * ldx) * ES + part * 16);
    }
    for (int i = tid; i < k * C; i += 256) ws[i] = w[i];
    __syncthreads();
    const long row = r0 + tid;
    if (row >= rows) return;
    float a = bias;
    for (int t = 0; t < k; ++t) {
        const char* xr = xs + (tid + t) * PITCH;
#pragma unroll
        for (int part = 0; part < CPR; ++part) {
            const uint4 v = *reinterpret_cast<const uint4*>(xr + part * 16);
            if constexpr (ES == 2) {
                const __half2* h = reinterpret_cast<const __half2*>(&v);
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float2 f = __half22float2(h[e]);
                    a = fmaf(f.x, ws[t * C + part * 8 + e * 2], a);
                    a = fmaf(f.y, ws[t * C + part * 8 + e * 2 + 1], a);
                }
            } else {
                const float* f = reinterpret_cast<const float*>(&v);
#pragma unroll
                for (int e = 0; e < 4; ++e) a = fmaf(fmaxf(f[e], f[e] * pre_slope), ws[t * C + part * 4 + e], a);   // leaky_relu of models.py:127
            }
        }
    }
    const bool valid = row_valid[row >> valid_shift] != 0;
    wav_rows[row] = valid ? tanhf(a) : 0.f;
}
// fp32 input, K taps known at compile time (the reference's 7): the generic kernel above spent its time on one LDS read per weight and a
// leaky-relu per (tap, element) -- ~900 VALU + 280 LDS instructions per output sample, 0.40 ms for 8.4 M samples against an HBM floor of 0.2.
// Here the leaky-relu is applied ONCE per element while staging, and the weights are compile-time offsets from a uniform pointer (scalar loads,
// SGPR operands of the FMAs).  Same summation order as the generic kernel: bit-identical output.
template <int C, int K>
__global__ __launch_bounds__(256) void conv_post_f32_kernel(const float* __restrict__ x, int ldx, const float* __restrict__ w, float bias, float pre_slope,
                                                            const uint8_t* __restrict__ row_valid, int valid_shift, float* __restrict__ wav_rows, int rows) {
    constexpr int PITCH = C * 4 + 16, CPR = C / 4, NROWS = 256 + K - 1, HALF = (K - 1) / 2;
    __shared__ __attribute__((aligned(16))) char xs[NROWS * PITCH];
    const int tid = threadIdx.x;
    const long r0 = (long)blockIdx.x * 256;
    // (round 6) ALL of a thread's requests first, then the stores: as a rolled loop (load, s_waitcnt vmcnt(0), ds_write, branch -- what hipcc made of it) a block
    // paid nine HBM round trips one after the other, 0.28 ms for 1.08 GB; the validity byte of the thread's output row travels with them.  Same values, same
    // summation order: bit-identical output.
    constexpr int NIT = (NROWS * CPR + 255) / 256;
    float4 ld[NIT];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int c = min(tid + i * 256, NROWS * CPR - 1), r = c / CPR, part = c % CPR;          // (the last, partial round re-reads the slab's last chunk)
        ld[i] = *reinterpret_cast<const float4*>(x + (r0 + r - HALF) * ldx + part * 4);
    }
    const long row = r0 + tid;
    const uint8_t vbyte = row_valid[min(row, (long)rows - 1) >> valid_shift];
#pragma unroll
    for (int i = 0; i < NIT; ++i) {
        const int c = tid + i * 256, r = c / CPR, part = c % CPR;
        float4 u = ld[i];
        u.x = fmaxf(u.x, u.x * pre_slope); u.y = fmaxf(u.y, u.y * pre_slope); u.z = fmaxf(u.z, u.z * pre_slope); u.w = fmaxf(u.w, u.w * pre_slope);   // leaky_relu of models.py:127
        if (c < NROWS * CPR) *reinterpret_cast<float4*>(xs + r * PITCH + part * 16) = u;
    }
    __syncthreads();
    if (row >= rows) return;
    float a = bias;
#pragma unroll
    for (int t = 0; t < K; ++t) {
        const char* xr = xs + (tid + t) * PITCH;
#pragma unroll
        for (int part = 0; part < CPR; ++part) {
            const float4 v = *reinterpret_cast<const float4*>(xr + part * 16);
            a = fmaf(v.x, w[t * C + part * 4 + 0], a);
            a = fmaf(v.y, w[t * C + part * 4 + 1], a);
            a = fmaf(v.z, w[t * C + part * 4 + 2], a);
            a = fmaf(v.w, w[t * C + part * 4 + 3], a);
        }
    }
    wav_rows[row] = vbyte != 0 ? tanhf(a) : 0.f;
}
void launch_conv_post(const void* x, int is_f32, int ldx, const float* w, float bias, int k, float pre_slope, const uint8_t* row_valid,
                      int valid_shift, float* wav_rows, int rows, int C, hipStream_t s) {
    const int grid = (rows + 255) / 256;
    if (C != 32) return;      // ev_create rejects configurations whose last stage is not 32 channels wide
    if (is_f32 && k == 7)
        hipLaunchKernelGGL((conv_post_f32_kernel<32, 7>), dim3(grid), dim3(256), 0, s, reinterpret_cast<const float*>(x), ldx, w, bias, pre_slope, row_valid,
                           valid_shift, wav_rows, rows);
    else if (is_f32)
        hipLaunchKernelGGL((conv_post_kernel<32, float>), dim3(grid), dim3(256), 0, s, reinterpret_cast<const float*>(x), ldx, w, bias, k,
                           pre_slope, row_valid, valid_shift, wav_rows, rows);
    else
        hipLaunchKernelGGL((conv_post_kernel<32, __half>), dim3(grid), dim3(256), 0, s, reinterpret_cast<const __half*>(x), ldx, w, bias, k,
                           pre_slope, row_valid, valid_shift, wav_rows, rows);
}

// ------------------------------------------------------------------ row maps of the gap layout
// rows -> (utterance, position, valid) from the per-utterance first row / length: one thread per row, binary search over the
// utterance offsets.  Replaces O(rows) host loops + three H2D copies + a stream synchronisation per call.
__global__ __launch_bounds__(256) void row_maps_kernel(const int32_t* off, const int32_t* len, int B, int32_t* seq, int32_t* pos,
                                                       uint8_t* valid, int rows) {
    const int r = blockIdx.x * 256 + threadIdx.x;
    if (r >= rows) return;
    int lo = 0, hi = B - 1, b = -1;
    while (lo <= hi) {              // last utterance whose first row is <= r
        const int mid = (lo + hi) >> 1;
        if (off[mid] <= r) { b = mid; lo = mid + 1; } else hi = mid - 1;
    }
    const bool in = b >= 0 && r < off[b] + len[b];
    seq[r] = in ? b : -1;
    pos[r] = in ? r - off[b] : 0;
    valid[r] = in ? 1 : 0;
}
void launch_row_maps(const int32_t* off, const int32_t* len, int B, int32_t* seq, int32_t* pos, uint8_t* valid, int rows, hipStream_t s) {
    hipLaunchKernelGGL(row_maps_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, off, len, B, seq, pos, valid, rows);
}

// ------------------------------------------------------------------ packing helpers
__global__ __launch_bounds__(256) void pack_rows_kernel(const void* src, int dtype, int ld, int C, const int64_t* seq_row_off,
                                                        const int64_t* seq_out_off, const int32_t* seq_rows, float* dst) {
    const int b = blockIdx.y;
    const long n = (long)seq_rows[b] * C;
    const long src0 = seq_row_off[b], dst0 = seq_out_off[b] * C;
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256) {
        const long r = i / C, c = i % C;
        float v;
        if (dtype == DT_F16) v = __half2float(reinterpret_cast<const __half*>(src)[(src0 + r) * ld + c]);
        else v = reinterpret_cast<const float*>(src)[(src0 + r) * ld + c];
        dst[dst0 + i] = v;
    }
}
void launch_pack_rows(const void* src, int dtype, int ld, int C, const int64_t* seq_row_off, const int64_t* seq_out_off,
                      const int32_t* seq_rows, int B, int64_t max_rows, float* dst, hipStream_t s) {
    long blocks = (max_rows * C + 255) / 256;
    if (blocks > 4096) blocks = 4096;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(pack_rows_kernel, dim3((unsigned)blocks, B), dim3(256), 0, s, src, dtype, ld, C, seq_row_off, seq_out_off,
                       seq_rows, dst);
}

// reference inference_am_vocoder_joint.py:130-131: (wav * 32768.0).astype('int16') -> C cast (truncate, wrap)
__global__ __launch_bounds__(256) void wav_to_i16_kernel(const float* wav, int16_t* out, long n) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < n; i += (long)gridDim.x * 256)
        out[i] = (int16_t)(int32_t)(wav[i] * 32768.0f);
}
void launch_wav_to_i16(const float* wav, int16_t* out, int64_t n, hipStream_t s) {
    long blocks = (n + 255) / 256;
    if (blocks > 8192) blocks = 8192;
    if (blocks < 1) blocks = 1;
    hipLaunchKernelGGL(wav_to_i16_kernel, dim3((unsigned)blocks), dim3(256), 0, s, wav, out, (long)n);
}

__global__ __launch_bounds__(256) void pe_extend_kernel(float* pe, const float* div, int row0, int rows, int C) {
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    const int half = C / 2;
    if (idx >= (long)rows * half) return;
    const int t = row0 + (int)(idx / half), i = (int)(idx % half);
    const float ang = (float)t * div[i];
    pe[(long)t * C + 2 * i] = sinf(ang);
    pe[(long)t * C + 2 * i + 1] = cosf(ang);
}
void launch_pe_extend(float* pe, const float* div, int row0, int row1, int C, hipStream_t s) {
    const long n = (long)(row1 - row0) * (C / 2);
    if (n <= 0) return;
    hipLaunchKernelGGL(pe_extend_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, pe, div, row0, row1 - row0, C);
}

void launch_fill_zero(void* p, size_t bytes, hipStream_t s) { (void)hipMemsetAsync(p, 0, bytes, s); }

}  // namespace ev
