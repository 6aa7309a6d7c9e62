// Response delivery (ev_deliver): wav at sr_in -> the response's bytes at sr_out, as fp32, int16 (optionally TPDF-dithered), G.711 mu-law or A-law.
// include/evhip.h states the specification.
//
// deliver: one block = DL_TILE consecutive outputs of one utterance, 256 threads, four CONSECUTIVE outputs per thread.  Output m is ev_resample's
// sample, term for term: the same phase-major table (resample_pack_table), the same k range (polyphase_taps) and the same sum (polyphase_sum,
// ev_audio_dev.h); only the distribution of the outputs over threads differs.  The tile's run of inputs is kept in LDS as fp32 (zero outside the
// utterance) when it fits, the table beside it when both fit (16 -> 44.1 kHz: 57 KB + 1.6 KB); what does not fit is read through L1 with the same
// bounds (polyphase_lds decides, as for ev_resample).  up == down == 1 is the same kernel without the filter.
// The four samples are converted in registers and leave as one store: a dword of four law bytes, 8 bytes of four int16, 16 bytes of four fp32 -- every utterance starts on a 16-byte boundary and a tile on a multiple of
// DL_TILE outputs, so the stores are aligned; the quad that holds the utterance's last sample writes zeros behind it and up to the end of the slot.
// Each block leaves its max |y| over finite samples and its count of clipped samples; deliver_fold reduces an utterance's tiles (a max and an integer
// sum: exact in any order).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

namespace {

// y -> the int16 value s (as int) and whether t (with dither: t + d) fell outside [-32768, 32767]
__device__ inline int dl_s16(float y, int dither, uint32_t seed, int64_t m, int* clipped) {
    float t = __fmul_rn(y, 32768.0f);
    if (dither) {
        const int ua = (int)(dl_mix(seed, 2 * (uint64_t)m) >> 8), ub = (int)(dl_mix(seed, 2 * (uint64_t)m + 1) >> 8);
        t = __fadd_rn(t, __fmul_rn((float)(ua - ub), 0x1p-24f));
    }
    *clipped = (t < -32768.0f || t > 32767.0f) ? 1 : 0;
    if (t != t) return 0;
    const float v = fminf(fmaxf(t, -32768.0f), 32767.0f);
    return dither ? (int)rintf(v) : (int)v;      // ties to even / truncation toward zero; the bounds are integers, so clamping first changes nothing
}

__device__ inline uint32_t dl_ulaw(int s) {
    int v = s >> 2, mask = 0xFF;
    if (v < 0) { v = -v; mask = 0x7F; }
    v = min(v, 8159) + 33;
    int seg = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) seg += v > ((0x40 << i) - 1) ? 1 : 0;
    if (seg >= 8) return (uint32_t)(0x7F ^ mask);      // v = 8192 only: audioop's answer for the clipped magnitude
    return (uint32_t)((((seg << 4) | ((v >> (seg + 1)) & 0xF)) ^ mask) & 0xFF);
}

__device__ inline uint32_t dl_alaw(int s) {
    int v = s >> 3, mask = 0xD5;
    if (v < 0) { mask = 0x55; v = -v - 1; }
    int seg = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) seg += v > ((0x20 << i) - 1) ? 1 : 0;      // v <= 4095: seg <= 7
    const int nib = seg < 2 ? (v >> 1) & 0xF : (v >> seg) & 0xF;
    return (uint32_t)((((seg << 4) | nib) ^ mask) & 0xFF);
}

}  // namespace

// PAD (only with RUN_LDS): the run is kept with one unused float after every 32.  Neighbouring lanes are four outputs = 4 down / up inputs apart;
// at down >= 2 up that is 8 floats or more, which would put a wave's reads on a quarter of the banks or fewer.
template <bool FILTER, bool RUN_LDS, bool TAB_LDS, bool PAD>
__global__ __launch_bounds__(256) void deliver_kernel(const DeliverParams p) {
    auto at = [](int i) -> int { return PAD ? i + (i >> 5) : i; };
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float s_pk[4];
    __shared__ int s_cl[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const DeliverTile tl = p.tiles[blockIdx.x];
    const DeliverSeq sq = p.seqs[tl.seq];
    const int64_t L = sq.len, up = p.up, down = p.down, half = p.half;
    const int m0 = tl.m0, m1 = (int)min((int64_t)m0 + DL_TILE, sq.n) - 1;      // the tile's outputs m0 .. m1
    float* run = reinterpret_cast<float*>(smem);
    float* ltab = run + (RUN_LDS ? p.run_cap : 0);
    int64_t k_first = 0;
    if (FILTER) {
        k_first = ceil_div((int64_t)m0 * down - half, up);
        const int64_t k_last = floor_div((int64_t)m1 * down + half, up);
        if (RUN_LDS)      // k_last - k_first + 1 < polyphase_run_max, and at() of the last one < run_cap
            stage_run<256>([&](int i) -> float& { return run[at(i)]; }, p.wav, p.wav_is_i16, sq.in_off, L, k_first, (int)(k_last - k_first + 1));
        if (TAB_LDS) {
            const int NT = p.up * p.row;
            for (int i = tid; i < NT; i += 256) ltab[i] = p.tab[i];
        }
        if (RUN_LDS || TAB_LDS) __syncthreads();
    }
    const int mq = m0 + 4 * tid;      // this thread's quad: outputs mq .. mq + 3
    float y[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int m = mq + r;
        y[r] = 0.f;
        if (m > m1) continue;
        if (!FILTER) {
            y[r] = load_sample(p.wav, p.wav_is_i16, sq.in_off + m);
            continue;
        }
        int64_t k_lo;
        int nk, ph;
        polyphase_taps(m, up, down, half, &k_lo, &nk, &ph);
        const float* h = (TAB_LDS ? ltab : p.tab) + (size_t)ph * p.row;
        const int x0 = (int)(k_lo - k_first);
        y[r] = RUN_LDS ? polyphase_sum([&](int j) { return run[at(x0 + j)]; }, h, nk)
                       : polyphase_sum([&](int j) { return sample_or_zero(p.wav, p.wav_is_i16, sq.in_off, L, k_lo + j); }, h, nk);
    }
    // the conversion, in registers; lanes past m1 carry zeros (the slot's padding)
    float pk = 0.f;
    int cl = 0;
    int q[4] = {0, 0, 0, 0};
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        if (mq + r > m1) continue;
        const float a = fabsf(y[r]);
        if (a <= 3.402823466e38f) pk = fmaxf(pk, a);      // finite samples only
        if (p.encoding != DL_F32) {
            int c = 0;
            const int s = dl_s16(y[r], p.dither, sq.seed, (int64_t)(mq + r), &c);
            cl += c;
            q[r] = p.encoding == DL_S16 ? s : (int)(p.encoding == DL_ULAW ? dl_ulaw(s) : dl_alaw(s));
        }
    }
    if (mq <= m1) {
        const int es = p.encoding == DL_F32 ? 4 : p.encoding == DL_S16 ? 2 : 1;
        uint8_t* base = p.out + sq.byte_off;
        const int64_t at = (int64_t)mq * es;      // a multiple of 4 es
        if (es == 4) {
            *reinterpret_cast<float4*>(base + at) = make_float4(y[0], y[1], y[2], y[3]);
        } else if (es == 2) {
            *reinterpret_cast<uint2*>(base + at) = make_uint2(((uint32_t)q[0] & 0xFFFFu) | ((uint32_t)q[1] << 16), ((uint32_t)q[2] & 0xFFFFu) | ((uint32_t)q[3] << 16));
        } else {
            *reinterpret_cast<uint32_t*>(base + at) = (uint32_t)q[0] | ((uint32_t)q[1] << 8) | ((uint32_t)q[2] << 16) | ((uint32_t)q[3] << 24);
        }
        if (mq + 3 >= sq.n - 1) {      // the utterance's last quad: zeros up to the end of its slot (a multiple of 16, so of the quad's 4 es bytes)
            for (int64_t o = at + 4 * es; o < sq.slot; o += 4 * es) {
                if (es == 4) *reinterpret_cast<float4*>(base + o) = make_float4(0.f, 0.f, 0.f, 0.f);
                else if (es == 2) *reinterpret_cast<uint2*>(base + o) = make_uint2(0u, 0u);
                else *reinterpret_cast<uint32_t*>(base + o) = 0u;
            }
        }
    }
    pk = wave_max_f32(pk);
    cl = wave_sum_i32(cl);
    if (lane == 0) { s_pk[w] = pk; s_cl[w] = cl; }
    __syncthreads();
    if (tid == 0) p.parts[blockIdx.x] = DeliverPart{fmaxf(fmaxf(s_pk[0], s_pk[1]), fmaxf(s_pk[2], s_pk[3])), (s_cl[0] + s_cl[1]) + (s_cl[2] + s_cl[3])};
}

// one wave per utterance over its tiles' parts
__global__ __launch_bounds__(64) void deliver_fold_kernel(const DeliverPart* __restrict__ parts, const DeliverSeq* __restrict__ seqs, DeliverOut* __restrict__ outs) {
    const DeliverSeq sq = seqs[blockIdx.x];
    const int nt = (int)((sq.n + DL_TILE - 1) / DL_TILE);
    float pk = 0.f;
    int64_t cl = 0;
    for (int i = threadIdx.x; i < nt; i += 64) { const DeliverPart t = parts[sq.tile0 + i]; pk = fmaxf(pk, t.peak); cl += t.clipped; }
    pk = wave_max_f32(pk);
    cl = wave_sum_i64(cl);
    if (threadIdx.x == 0) outs[blockIdx.x] = DeliverOut{pk, 0, cl};
}

int launch_deliver(const DeliverParams& p, hipStream_t s) {
    if (p.n_tiles <= 0 || p.up < 1 || p.down < 1 || p.encoding < DL_F32 || p.encoding > DL_ALAW || (p.dither != 0 && p.dither != 1)) return -1;
    const dim3 g((unsigned)p.n_tiles), b(256);
    DeliverParams q = p;
    q.run_cap = 0;
    if (p.up == 1 && p.down == 1) {
        hipLaunchKernelGGL((deliver_kernel<false, false, false, false>), g, b, 0, s, q);
        return 0;
    }
    if (p.half < 1 || p.row != resample_row_len(p.up, p.half) || !p.tab) return -1;
    const bool pad = p.down >= 2 * p.up;
    const PolyphaseLds l = polyphase_lds(DL_TILE, p.up, p.down, p.half, pad);
    q.run_cap = l.run_cap;
    void (*fn)(const DeliverParams) = l.run_lds ? (l.tab_lds ? (pad ? deliver_kernel<true, true, true, true> : deliver_kernel<true, true, true, false>)
                                                             : (pad ? deliver_kernel<true, true, false, true> : deliver_kernel<true, true, false, false>))
                                                : (l.tab_lds ? deliver_kernel<true, false, true, false> : deliver_kernel<true, false, false, false>);
    if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes) != hipSuccess) return -1;
    hipLaunchKernelGGL(fn, g, b, l.bytes, s, q);
    return 0;
}

void launch_deliver_fold(const DeliverPart* parts, const DeliverSeq* seqs, int B, DeliverOut* outs, hipStream_t s) {
    hipLaunchKernelGGL(deliver_fold_kernel, dim3((unsigned)B), dim3(64), 0, s, parts, seqs, outs);
}

}  // namespace ev
