// True-peak metering and look-ahead limiting (ev_limit): packed segments -> the gain every sample requires under a 4x oversampling true-peak meter,
// the peaks per tile, and, from that gain eroded over look-ahead + hold and smoothed by a raised-cosine window, the limited waveform.
// include/evhip.h states the specification.
//
// A tile is LIMIT_TILE samples counted from the segment's start; one block of 256 per tile, lane l owns the samples l, l + 256, l + 512, ...: both
// kernels read LDS at consecutive addresses across a wave (unit stride, every lane its own bank) and the taps / the window at one address per
// wave (a broadcast), so neither the halo nor the reversed window walk meets a bank conflict.
// limit_peak<MEASURE>: the tile's u = x * gain with LIMIT_HALO samples on each side (zeros outside the segment and for non-finite values) and the
//   phase table go to LDS.  Four samples per lane at a time, so that one read of the four phases' taps feeds sixteen fp64 fmas: d = -16 .. 16
//   ascending is k = n + d ascending, the order of the specification; the table holds 0 where 4 d - q leaves the taps' support, which adds +-0 to a
//   sum that started at +0.0 and changes no bit.  The products are exact in fp64, so the fma is the multiply-then-add of the specification.
//   MEASURE = false also writes r.  Maxima and the non-finite count: an xor butterfly inside a wave, then waves 0 .. 3 in order.
// limit_apply: r on [t0 - L - Hd, t0 + LIMIT_TILE + L) goes to LDS (1 outside the segment).  A tile whose reach is all ones copies through: s = 1
//   there by the specification's rule.  Otherwise the erosion by window doubling between two copies, a_(j+1)[i] = min(a_j[i], a_j[i + 2^j]), and
//   m[i] = min(a_p[i], a_p[i + W - 2^p]) for W = L + Hd + 1 >= 2^p; then the (L + 1)-tap fp64 sum, four samples per lane at a time.  min is exact in any
//   order.  fp64 runs at a fraction of the fp32 rate, but 81 fmas a sample at the default L is far below what the 10 bytes a sample of traffic cost.
// No return sits before a __syncthreads(): every branch around one is uniform over the block.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

namespace {

// u of the specification: the source bits where the gain is one
__device__ inline float limit_load(const void* wav, int is16, int64_t i, float g) {
    const float x = load_sample(wav, is16, i);
    return g == 1.0f ? x : mul_rn(x, g);
}

constexpr int LIMIT_GROUP = 4 * 256;      // samples a block handles at a time: four per lane

}  // namespace

template <bool MEASURE>
__global__ __launch_bounds__(256) void limit_peak_kernel(const void* __restrict__ wav, int is16, const float* __restrict__ gains,
                                                          const LimitTile* __restrict__ tiles, const double* __restrict__ tab, float ceiling,
                                                          float* __restrict__ r, LimitPeakOut* __restrict__ outs) {
    __shared__ float s_u[LIMIT_TILE + 2 * LIMIT_HALO];      // u[pos - LIMIT_HALO + i]
    __shared__ __attribute__((aligned(16))) double s_h[LIMIT_TAB];
    __shared__ float s_sp[4], s_tp[4];
    __shared__ int s_nf[4];
    const LimitTile tl = tiles[blockIdx.x];
    const float g = gains ? gains[tl.seg] : 1.0f;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t seg0 = tl.src - tl.pos;      // the segment's first sample in the packed input
    if (tid < LIMIT_TAB) s_h[tid] = tab[tid];
    float sp = 0.f, tp = 0.f;
    int nf = 0;
    for (int i = tid; i < LIMIT_TILE + 2 * LIMIT_HALO; i += 256) {
        const int64_t k = tl.pos - LIMIT_HALO + i;
        const bool own = i >= LIMIT_HALO && i < LIMIT_HALO + tl.n;
        float v = 0.f;
        if (k >= 0 && k < tl.len && i < tl.n + 2 * LIMIT_HALO) {
            v = limit_load(wav, is16, seg0 + k, g);
            if (!finite_f32(v)) { v = 0.f; nf += own ? 1 : 0; }
        }
        if (own) sp = fmaxf(sp, fabsf(v));
        s_u[i] = v;
    }
    __syncthreads();
    for (int base = 0; base < tl.n; base += LIMIT_GROUP) {
        double acc[4][4];
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int q = 0; q < 4; ++q) acc[e][q] = 0.0;
        for (int d = 0; d <= 2 * LIMIT_HALO; ++d) {
            const double h0 = s_h[d * 4], h1 = s_h[d * 4 + 1], h2 = s_h[d * 4 + 2], h3 = s_h[d * 4 + 3];
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const double u = (double)s_u[base + e * 256 + tid + d];
                acc[e][0] = fma(u, h0, acc[e][0]); acc[e][1] = fma(u, h1, acc[e][1]);
                acc[e][2] = fma(u, h2, acc[e][2]); acc[e][3] = fma(u, h3, acc[e][3]);
            }
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = base + e * 256 + tid;
            if (n < tl.n) {
                float p = fabsf(s_u[n + LIMIT_HALO]);
#pragma unroll
                for (int q = 0; q < 4; ++q) p = fmaxf(p, fabsf((float)acc[e][q]));
                tp = fmaxf(tp, p);
                if (!MEASURE) r[tl.src + n] = p <= ceiling ? 1.0f : (float)((double)ceiling / (double)p);
            }
        }
    }
    sp = wave_max_f32(sp);
    tp = wave_max_f32(tp);
    nf = wave_sum_i32(nf);
    if (lane == 0) { s_sp[w] = sp; s_tp[w] = tp; s_nf[w] = nf; }
    __syncthreads();
    if (tid == 0) {
        LimitPeakOut o;
        o.sample_peak = fmaxf(fmaxf(s_sp[0], s_sp[1]), fmaxf(s_sp[2], s_sp[3]));
        o.true_peak = fmaxf(fmaxf(s_tp[0], s_tp[1]), fmaxf(s_tp[2], s_tp[3]));
        o.nonfinite = s_nf[0] + s_nf[1] + s_nf[2] + s_nf[3];
        o.pad = 0;
        outs[blockIdx.x] = o;
    }
}

__global__ __launch_bounds__(256) void limit_apply_kernel(const void* __restrict__ wav, int is16, const float* __restrict__ gains,
                                                           const LimitTile* __restrict__ tiles, const float* __restrict__ r,
                                                           const double* __restrict__ win, int L, int Hd, float* __restrict__ out,
                                                           int16_t* __restrict__ out_i16, float* __restrict__ s_out, LimitApplyOut* __restrict__ outs) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    __shared__ float s_mn[4];
    __shared__ int s_ct[4];
    const int R = LIMIT_TILE + 2 * L + Hd, W = L + Hd + 1;
    double* s_w = reinterpret_cast<double*>(smem);
    float* cur = reinterpret_cast<float*>(smem + sizeof(double) * (size_t)(L + 1));
    float* nxt = cur + R;
    const LimitTile tl = tiles[blockIdx.x];
    const float g = gains ? gains[tl.seg] : 1.0f;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t seg0 = tl.src - tl.pos, k0 = tl.pos - L - Hd;      // cur[i] = r[k0 + i] of the segment
    int below = 0;
    for (int i = tid; i < R; i += 256) {
        const int64_t k = k0 + i;
        const float v = k >= 0 && k < tl.len ? r[seg0 + k] : 1.0f;
        cur[i] = v;
        below |= v != 1.0f ? 1 : 0;
    }
    for (int j = tid; j <= L; j += 256) s_w[j] = win[j];
    below = __syncthreads_or(below);      // uniform over the block from here on
    if (below) {
        int span = 1;
        while (2 * span <= W) {      // cur[i] = min r over [i, i + span) wherever that lies inside the reach
            for (int i = tid; i < R; i += 256) nxt[i] = i + span < R ? fminf(cur[i], cur[i + span]) : cur[i];
            __syncthreads();
            float* t = cur; cur = nxt; nxt = t;
            span *= 2;
        }
        // m[pos - L + i] = min r[pos - L + i - Hd .. pos + i] = min cur[i .. i + W): two windows of span <= W < 2 span samples
        for (int i = tid; i < LIMIT_TILE + L; i += 256) nxt[i] = fminf(cur[i], cur[i + W - span]);
        __syncthreads();
    }
    const float* m = nxt;      // m[i] is the erosion at the segment's index pos - L + i; read only under `below`
    float mn = 1.0f;
    int ct = 0;
    for (int base = 0; base < tl.n; base += LIMIT_GROUP) {
        float sv[4] = {1.0f, 1.0f, 1.0f, 1.0f};
        if (below) {
            double acc[4] = {0.0, 0.0, 0.0, 0.0};
            float lo[4] = {1.0f, 1.0f, 1.0f, 1.0f};
            for (int j = 0; j <= L; ++j) {
                const double wj = s_w[j];
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float v = m[base + e * 256 + tid + L - j];      // m[n - j]
                    lo[e] = fminf(lo[e], v);
                    acc[e] = fma(wj, (double)v, acc[e]);
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) sv[e] = lo[e] == 1.0f ? 1.0f : (float)acc[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int n = base + e * 256 + tid;
            if (n < tl.n) {
                const float u = limit_load(wav, is16, tl.src + n, g), s = sv[e];
                const float y = s == 1.0f ? u : mul_rn(u, s);
                out[tl.src + n] = y;
                if (out_i16) out_i16[tl.src + n] = y != y ? (int16_t)0 : s16_trunc(y);      // NaN -> 0
                if (s_out) s_out[tl.src + n] = s;
                mn = fminf(mn, s);
                ct += s < 1.0f ? 1 : 0;
            }
        }
    }
    mn = wave_min_f32(mn);
    ct = wave_sum_i32(ct);
    if (lane == 0) { s_mn[w] = mn; s_ct[w] = ct; }
    __syncthreads();
    if (tid == 0) {
        LimitApplyOut o;
        o.min_gain = fminf(fminf(s_mn[0], s_mn[1]), fminf(s_mn[2], s_mn[3]));
        o.limited = s_ct[0] + s_ct[1] + s_ct[2] + s_ct[3];
        outs[blockIdx.x] = o;
    }
}

void limit_pack_taps(const float* h, double* tab) {
    const int half = (LIMIT_TAPS - 1) / 2;
    for (int d = -LIMIT_HALO; d <= LIMIT_HALO; ++d)
        for (int q = 0; q < 4; ++q) {
            const int i = q - 4 * d;
            tab[(d + LIMIT_HALO) * 4 + q] = i >= -half && i <= half ? (double)h[i + half] : 0.0;
        }
}

int launch_limit_peak(const void* wav, int is16, const float* gains, const LimitTile* tiles, int64_t n_tiles, const double* tab, float ceiling, float* r,
                      LimitPeakOut* outs, hipStream_t s) {
    if (n_tiles < 1 || n_tiles > INT_MAX) return -1;
    if (r) hipLaunchKernelGGL(limit_peak_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0, s, wav, is16, gains, tiles, tab, ceiling, r, outs);
    else hipLaunchKernelGGL(limit_peak_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0, s, wav, is16, gains, tiles, tab, ceiling, r, outs);
    return 0;
}

int launch_limit_apply(const void* wav, int is16, const float* gains, const LimitTile* tiles, int64_t n_tiles, const float* r, const double* win, int L,
                       int Hd, float* out, int16_t* out_i16, float* s_out, LimitApplyOut* outs, hipStream_t s) {
    if (n_tiles < 1 || n_tiles > INT_MAX || L < 0 || L > LIMIT_MAX_LOOKAHEAD || Hd < 0 || Hd > LIMIT_MAX_HOLD) return -1;
    const size_t lds = limit_apply_lds_bytes(L, Hd);
    if (lds > (size_t)LIMIT_MAX_LDS) return -1;
    if (hipFuncSetAttribute((const void*)limit_apply_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(limit_apply_kernel, dim3((unsigned)n_tiles), dim3(256), lds, s, wav, is16, gains, tiles, r, win, L, Hd, out, out_i16, s_out, outs);
    return 0;
}

}  // namespace ev
