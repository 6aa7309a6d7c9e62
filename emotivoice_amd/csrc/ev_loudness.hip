// Loudness normalisation (ev_loudness): packed segments -> the K-weighted 100 ms step sums of ITU-R BS.1770, the sample peak and the count of
// non-finite samples per tile, and, once the host has gated the blocks and fixed one gain per segment, the scaled waveform.  include/evhip.h states
// the specification.
//
// The two biquads (shelf, then high-pass) in transposed direct form II are one linear system with four states, s' = A s + B x, y = C s + D x.  A tile
// is LOUD_TILE samples counted from the segment's start; lane l of a block of 256 owns the LOUD_RUN = 16 consecutive samples [16 l, 16 l + 16).
// loud_tile<false>: every lane runs its samples from a zero state; an inclusive scan over the lanes, m_l += A^(16 2^d) m_(l - 2^d) for d = 0 .. 7,
//   turns the end states into the tile's zero-state end state e_t (samples past the segment's end enter as zeros).
// loud_carry: one thread per segment walks its tiles, s_(t+1) = A^4096 s_t + e_t, and leaves every tile's true initial state.
// loud_tile<true>: the same run and scan with lane 0 started from the tile's initial state, so the scan gives every lane's true start state; a second
//   run from it yields y.  A lane's y^2 go, in sample order, into the sum of the step its first sample lies in and, past the step's end, into the
//   next one (step >= 800 > 16: a run meets one boundary at most); per step of the tile the lanes' sums are added by an xor butterfly inside a
//   wave and wave 0 .. 3 in order.  Everything is fp64, nothing is atomic, and no order depends on anything but the sample's index in its segment.
// loud_gain: four packed samples per thread; the segment of the first comes from a binary search of the offsets.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

namespace {

// one sample through both biquads; returns y
__device__ inline double loud_step(const LoudCoef& c, double x, double s[4]) {
    const double y1 = c.b[0][0] * x + s[0];
    s[0] = c.b[0][1] * x - c.a[0][0] * y1 + s[1];
    s[1] = c.b[0][2] * x - c.a[0][1] * y1;
    const double y = c.b[1][0] * y1 + s[2];
    s[2] = c.b[1][1] * y1 - c.a[1][0] * y + s[3];
    s[3] = c.b[1][2] * y1 - c.a[1][1] * y;
    return y;
}

}  // namespace

template <bool FINAL>
__global__ __launch_bounds__(256) void loud_tile_kernel(const void* __restrict__ wav, int is16, const LoudTile* __restrict__ tiles,
                                                         const LoudCoef* __restrict__ cf, const double* __restrict__ init, double* __restrict__ ends,
                                                         int step, LoudTileOut* __restrict__ outs) {
    __shared__ float s_x[256 * (LOUD_RUN + 1)];      // lane l's run at 17 l: consecutive lanes on consecutive banks
    __shared__ double s_st[4][256];
    __shared__ double s_red[4];
    __shared__ float s_pk[4];
    __shared__ int s_nf[4];
    const LoudTile tl = tiles[blockIdx.x];
    const LoudCoef c = *cf;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
#pragma unroll
    for (int r = 0; r < LOUD_TILE / 256; ++r) {
        const int i = r * 256 + tid;
        float v = 0.f;
        // not load_sample: through the helper the compiler forms these sixteen addresses per lane in 64 bits, and the kernel measured 1 % slower
        if (i < tl.n) v = is16 ? (float)reinterpret_cast<const int16_t*>(wav)[tl.src + i] / 32768.0f : reinterpret_cast<const float*>(wav)[tl.src + i];
        s_x[(i >> 4) * (LOUD_RUN + 1) + (i & 15)] = v;
    }
    __syncthreads();
    double x[LOUD_RUN];
    float pk = 0.f;
    int nf = 0;
#pragma unroll
    for (int i = 0; i < LOUD_RUN; ++i) {
        const float v = s_x[tid * (LOUD_RUN + 1) + i];
        if (finite_f32(v)) { pk = fmaxf(pk, fabsf(v)); x[i] = (double)v; } else { ++nf; x[i] = 0.0; }
    }
    double s0[4] = {0.0, 0.0, 0.0, 0.0};
    if (FINAL && tid == 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s0[k] = init[(int64_t)blockIdx.x * 4 + k];
    }
    double m[4] = {s0[0], s0[1], s0[2], s0[3]};
#pragma unroll
    for (int i = 0; i < LOUD_RUN; ++i) (void)loud_step(c, x[i], m);
#pragma unroll
    for (int d = 0; d < 8; ++d) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s_st[k][tid] = m[k];
        __syncthreads();
        if (tid >= (1 << d)) {
            double o[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) o[k] = s_st[k][tid - (1 << d)];
#pragma unroll
            for (int j = 0; j < 4; ++j)
                m[j] += ((c.P[d][j * 4 + 0] * o[0] + c.P[d][j * 4 + 1] * o[1]) + c.P[d][j * 4 + 2] * o[2]) + c.P[d][j * 4 + 3] * o[3];
        }
        __syncthreads();
    }
    if (!FINAL) {
        if (tid == 255) {
#pragma unroll
            for (int k = 0; k < 4; ++k) ends[(int64_t)blockIdx.x * 4 + k] = m[k];
        }
        return;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) s_st[k][tid] = m[k];
    __syncthreads();
    if (tid > 0) {
#pragma unroll
        for (int k = 0; k < 4; ++k) s0[k] = s_st[k][tid - 1];
    }
    // the lane's samples [i0, i0 + cnt) of the segment; `edge` of them lie in step bin0, the rest in bin0 + 1
    const int64_t i0 = tl.pos + (int64_t)tid * LOUD_RUN, bin0 = i0 / step, tb0 = tl.pos / step;
    const int cnt = min(max(tl.n - tid * LOUD_RUN, 0), LOUD_RUN);
    const int64_t edge = (bin0 + 1) * (int64_t)step - i0;
    const int klo = (int)(bin0 - tb0), nslots = (int)((tl.pos + tl.n - 1) / step - tb0) + 1;
    double lo = 0.0, hi = 0.0;
#pragma unroll
    for (int i = 0; i < LOUD_RUN; ++i) {
        const double y = loud_step(c, x[i], s0);
        if (i < cnt) {
            if (i < edge) lo += y * y; else hi += y * y;
        }
    }
    for (int k = 0; k < LOUD_SLOTS; ++k) {
        double v = 0.0;
        if (k < nslots) {
            v = wave_sum_f64((k == klo ? lo : 0.0) + (k == klo + 1 ? hi : 0.0));
            if (lane == 0) s_red[w] = v;
            __syncthreads();
            v = ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
            __syncthreads();
        }
        if (tid == 0) outs[blockIdx.x].sum[k] = v;
    }
    pk = wave_max_f32(pk);
    nf = wave_sum_i32(nf);
    if (lane == 0) { s_pk[w] = pk; s_nf[w] = nf; }
    __syncthreads();
    if (tid == 0) {
        outs[blockIdx.x].peak = fmaxf(fmaxf(s_pk[0], s_pk[1]), fmaxf(s_pk[2], s_pk[3]));
        outs[blockIdx.x].nonfinite = s_nf[0] + s_nf[1] + s_nf[2] + s_nf[3];
    }
}

__global__ __launch_bounds__(64) void loud_carry_kernel(const LoudSeg* __restrict__ segs, int B, const LoudCoef* __restrict__ cf,
                                                         const double* __restrict__ ends, double* __restrict__ init) {
    const int b = blockIdx.x * 64 + threadIdx.x;
    if (b >= B) return;
    const LoudSeg sg = segs[b];
    const double* P = cf->P[8];
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t t = sg.tile0; t < sg.tile0 + sg.ntiles; ++t) {
        double e[4], n[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) { init[t * 4 + k] = s[k]; e[k] = ends[t * 4 + k]; }
#pragma unroll
        for (int j = 0; j < 4; ++j) n[j] = (((P[j * 4 + 0] * s[0] + P[j * 4 + 1] * s[1]) + P[j * 4 + 2] * s[2]) + P[j * 4 + 3] * s[3]) + e[j];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = n[k];
    }
}

__global__ __launch_bounds__(256) void loud_gain_kernel(const void* __restrict__ wav, int is16, const int64_t* __restrict__ offs, int B,
                                                         const float* __restrict__ gain, int64_t total, float* __restrict__ out,
                                                         int16_t* __restrict__ out_i16) {
    const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i0 >= total) return;
    int lo = 0, hi = B;      // the last segment whose offset is <= i0
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (offs[mid] <= i0) lo = mid; else hi = mid;
    }
    int seg = lo;
    float g = gain[seg];
    int64_t end = offs[seg + 1];
    const int cnt = (int)min((int64_t)4, total - i0);
    float o[4] = {0.f, 0.f, 0.f, 0.f};
    for (int r = 0; r < cnt; ++r) {
        const int64_t i = i0 + r;
        while (i >= end) { ++seg; g = gain[seg]; end = offs[seg + 1]; }      // lens >= 1 and i < total = offs[B]: seg stays below B
        const float x = load_sample(wav, is16, i);
        o[r] = g == 1.0f ? x : mul_rn(x, g);      // the source bits where the gain is one, else one rounded fp32 product
    }
    if (cnt == 4) {
        *reinterpret_cast<float4*>(out + i0) = make_float4(o[0], o[1], o[2], o[3]);      // out is 256-byte aligned and i0 a multiple of 4
    } else {
        for (int r = 0; r < cnt; ++r) out[i0 + r] = o[r];
    }
    if (out_i16) {
        for (int r = 0; r < cnt; ++r) out_i16[i0 + r] = o[r] != o[r] ? (int16_t)0 : s16_trunc(o[r]);      // NaN -> 0
    }
}

int launch_loudness_measure(const void* wav, int is16, const LoudTile* tiles, int64_t n_tiles, const LoudSeg* segs, int B, const LoudCoef* coef, int step,
                            double* ends, double* init, LoudTileOut* outs, hipStream_t s) {
    // a tile of LOUD_TILE samples must not reach into more than LOUD_SLOTS steps, and a lane's run must meet one step boundary at most
    if (n_tiles < 1 || n_tiles > INT_MAX || B < 1 || step <= LOUD_RUN || (LOUD_TILE - 1) / step + 2 > LOUD_SLOTS) return -1;
    hipLaunchKernelGGL(loud_tile_kernel<false>, dim3((unsigned)n_tiles), dim3(256), 0, s, wav, is16, tiles, coef, (const double*)nullptr, ends, step,
                       (LoudTileOut*)nullptr);
    hipLaunchKernelGGL(loud_carry_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0, s, segs, B, coef, (const double*)ends, init);
    hipLaunchKernelGGL(loud_tile_kernel<true>, dim3((unsigned)n_tiles), dim3(256), 0, s, wav, is16, tiles, coef, (const double*)init, (double*)nullptr, step,
                       outs);
    return 0;
}

int launch_loudness_gain(const void* wav, int is16, const int64_t* offs, int B, const float* gain, int64_t total, float* out, int16_t* out_i16,
                         hipStream_t s) {
    const int64_t blocks = (total + 1023) / 1024;
    if (total < 1 || blocks > INT_MAX || B < 1) return -1;
    hipLaunchKernelGGL(loud_gain_kernel, dim3((unsigned)blocks), dim3(256), 0, s, wav, is16, offs, B, gain, total, out, out_i16);
    return 0;
}

}  // namespace ev
