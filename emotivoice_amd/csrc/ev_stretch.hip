// Time-scale modification (ev_stretch): packed segments -> the same audio at another length and the same pitch, by WSOLA (waveform-similarity
// overlap-add).  include/evhip.h states the specification; every decision is an integer one and the only floating arithmetic is the two-term
// weighted sum of the output.
//
// wsola_search_kernel: one block of 256 per segment, thread l owns the lag l - 128, the frame loop inside.  The chain delta_(k-1) -> delta_k is
//   serial, but what frame k reads is known before delta_(k-1) is: its candidates lie in q[a_k - 128, a_k + 127 + N) and the template of frame
//   k + 1 in q[a_k + H - 128, a_k + H + 127 + N), so ONE run R_k = q[a_k - 128, a_k - 128 + 1023) serves both.  Three runs rotate through LDS as
//   int16: while frame k reads R_k (candidates) and R_(k-1) (template), the samples of R_(k+1) are on their way from memory in registers; they are
//   quantised and written to the third run after the sums, before the barrier that publishes the frame's minimum.
//   The distance is formed as D(d) = eT + e(d) - 2 c(d): c(d) = sum T[n] C[d + n] stays inside int32 (512 * 2047^2 < 2^31) and takes
//   v_dot2c_i32_i16 on pairs of samples; e(d) and eT, sums of 512 squares, are differences of a prefix sum of squares that is laid down with
//   each run (uint32, relative to the 256-sample quarter, and the four quarter totals), so no lane squares a candidate twice.
//   LDS layout of the c loop: thread l = 8 g + r reads the ALIGNED groups of eight candidates 8 (g + i), i = 0 .. 64 (one ds_read_b128: eight
//   lanes share an address, a wave covers eight neighbouring 16-byte slots), against the template shifted by its own r: row r of s_ts holds
//   T[u - r] at u, zero where u - r leaves [0, N), rebuilt once delta_(k-1) is known.  The rows are 1040 bytes apart, 4 banks modulo 64, so the
//   eight rows a wave reads sit in eight different 16-byte slots: neither read meets a bank conflict, and none is off its natural alignment.
//   The argmin is one wave_min_i64 over the key D << 9 | |delta| << 1 | (delta > 0), then four keys through LDS.
//   The block also counts the segment's non-finite samples, in a pass of its own before the frames.
// wsola_ola_kernel: one block per STRETCH_OLA_FRAMES output frames, thread j owns the window position j.  Each output has exactly two terms; the
//   products w x are exact in fp64 (24 x 24 bits), so whether the compiler fuses the second product into the sum changes no bit.
// No atomics; no return sits before a __syncthreads(): every branch around one is uniform over the block.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

namespace {

constexpr int ST_N = STRETCH_FRAME, ST_H = STRETCH_HOP, ST_HALF = STRETCH_LAGS / 2;
constexpr int ST_RUN = 1024;                 // samples of a staged run: four per lane; 2 * ST_HALF - 1 + ST_N + ST_H = 1023 of them are read
constexpr int ST_GROUPS = ST_N / 8 + 1;      // aligned groups of eight that a window of N samples starting at r < 8 touches
constexpr int ST_TS_PITCH = 8 * ST_GROUPS;   // samples of a shifted template row: 520, 1040 bytes
static_assert(ST_N == 512 && ST_H == 256 && STRETCH_LAGS == 256, "the search block is one lag per thread and four staged samples per thread");
static_assert(2 * ST_HALF - 1 + ST_N + ST_H <= ST_RUN, "a run holds a frame's candidates and the next frame's template");
static_assert(512ll * 2047 * 2047 < (1ll << 31), "a dot product of N decision samples stays inside int32");
static_assert((long long)ST_RUN * 2047 * 2047 < (1ll << 32), "the prefix sum of a run's squares stays inside uint32");
static_assert((ST_TS_PITCH * 2) % 16 == 0 && (ST_TS_PITCH / 2) % 64 == 4, "the template rows are 16-byte aligned and 4 banks apart");

typedef short short2v __attribute__((ext_vector_type(2)));

// the decision sample: 12 bits, 0 for a non-finite value
__device__ inline int stretch_q(float x) { return finite_f32(x) ? (int)fminf(fmaxf(rintf(x * 2048.0f), -2047.0f), 2047.0f) : 0; }

__device__ inline int dot2(int a, int b, int c) { return __builtin_amdgcn_sdot2(__builtin_bit_cast(short2v, a), __builtin_bit_cast(short2v, b), c, false); }

// One staged run in LDS: the samples, the sum of the squares before each sample inside its quarter of 256, and the quarters' totals.
struct StretchRun {
    __attribute__((aligned(16))) int16_t q[ST_RUN];
    __attribute__((aligned(16))) uint32_t sq[ST_RUN];
    uint32_t quarter[4];
};

// the samples 4 tid .. 4 tid + 3 of the run that starts at the segment's sample `first`
__device__ inline void run_load(float v[4], const void* wav, int is16, const StretchSeg& sg, int64_t first) {
#pragma unroll
    for (int e = 0; e < 4; ++e) v[e] = sample_or_zero(wav, is16, sg.in_off, sg.len_in, first + 4 * (int)threadIdx.x + e);
}

// quantises them and lays the run down; wave w holds the quarter w
__device__ inline void run_store(StretchRun& run, const float v[4]) {
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int q[4];
    uint32_t before[4], sum = 0;
#pragma unroll
    for (int e = 0; e < 4; ++e) { q[e] = stretch_q(v[e]); before[e] = sum; sum += (uint32_t)(q[e] * q[e]); }
    const uint32_t incl = wave_scan_u32(sum), excl = incl - sum;
    *reinterpret_cast<uint2*>(run.q + 4 * tid) = make_uint2((uint32_t)(q[0] & 0xffff) | ((uint32_t)q[1] << 16), (uint32_t)(q[2] & 0xffff) | ((uint32_t)q[3] << 16));
    *reinterpret_cast<uint4*>(run.sq + 4 * tid) = make_uint4(excl + before[0], excl + before[1], excl + before[2], excl + before[3]);
    if (lane == 63) run.quarter[w] = incl;
}

// the sum of the squares of the run's samples before u, u <= ST_RUN - 1
__device__ inline uint32_t run_prefix(const StretchRun& run, int u) {
    const int j = u >> 8;
    return run.sq[u] + (j > 0 ? run.quarter[0] : 0u) + (j > 1 ? run.quarter[1] : 0u) + (j > 2 ? run.quarter[2] : 0u);
}

}  // namespace

__global__ __launch_bounds__(256) void wsola_search_kernel(const void* __restrict__ wav, int is16, const StretchSeg* __restrict__ segs,
                                                            int16_t* __restrict__ deltas, StretchFig* __restrict__ figs) {
    __shared__ StretchRun s_run[3];
    __shared__ __attribute__((aligned(16))) int16_t s_ts[8][ST_TS_PITCH];
    __shared__ int64_t s_min[4];
    __shared__ int64_t s_nf[4];
    const StretchSeg sg = segs[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    int64_t nf = 0;
    if (!is16)
        for (int64_t i = tid; i < sg.len_in; i += 256) nf += finite_f32(load_sample(wav, 0, sg.in_off + i)) ? 0 : 1;
    nf = wave_sum_i64(nf);
    if (lane == 0) s_nf[w] = nf;
    const int K = sg.frames;
    uint64_t sum = 0;
    int edges = 0;
    if (tid == 0) deltas[sg.frame_off] = 0;
    if (K > 1) {      // uniform over the block
        float v[4];
        run_load(v, wav, is16, sg, -(int64_t)ST_HALF);      // a_0 = 0
        run_store(s_run[0], v);
        run_load(v, wav, is16, sg, stretch_a(1, sg.len_in, sg.len_out) - ST_HALF);
        run_store(s_run[1], v);
        __syncthreads();
        const int r = tid & 7, g = tid >> 3;
        int prev = 0, tpl = 0, cnd = 1, nxt = 2;      // delta_(k-1); the runs R_(k-1), R_k, R_(k+1)
        for (int k = 1; k < K; ++k) {
            const bool more = k + 1 < K;
            if (more) run_load(v, wav, is16, sg, stretch_a(k + 1, sg.len_in, sg.len_out) - ST_HALF);
            // the template q[p_(k-1) + H + n] = R_(k-1)[base + n], shifted by every r
            const int base = ST_H + ST_HALF + prev;
            const int16_t* T = s_run[tpl].q + base;
            // Thread tid fills the columns u = tid, tid + 256 (and tid + 512 < ST_TS_PITCH) of every row: row rr takes T[u - rr].  Every read goes
            // out before the first write (at a clamped index, then the select), so the block pays one LDS latency, not one per element.
            int16_t tv[3][8];
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                if (it == 2 && w != 0) break;      // uniform over the wave
#pragma unroll
                for (int rr = 0; rr < 8; ++rr) {
                    const int n = tid + 256 * it - rr;
                    const int16_t t = T[min(max(n, 0), ST_N - 1)];
                    tv[it][rr] = (n >= 0 && n < ST_N) ? t : (int16_t)0;
                }
            }
#pragma unroll
            for (int it = 0; it < 3; ++it) {
                const int u = tid + 256 * it;
                if (it == 2 && w != 0) break;
#pragma unroll
                for (int rr = 0; rr < 8; ++rr)
                    if (u < ST_TS_PITCH) s_ts[rr][u] = tv[it][rr];
            }
            __syncthreads();
            const int4* tp = reinterpret_cast<const int4*>(s_ts[r]);
            const int4* cp = reinterpret_cast<const int4*>(s_run[cnd].q) + g;
            int c0 = 0, c1 = 0;
#pragma unroll 13
            for (int i = 0; i < ST_GROUPS; ++i) {      // 65 groups: five rounds of 26 reads in flight (one wave per SIMD: the latency is not hidden otherwise)
                const int4 t = tp[i], x = cp[i];
                c0 = dot2(t.x, x.x, c0); c1 = dot2(t.y, x.y, c1); c0 = dot2(t.z, x.z, c0); c1 = dot2(t.w, x.w, c1);
            }
            const uint32_t e = run_prefix(s_run[cnd], tid + ST_N) - run_prefix(s_run[cnd], tid);
            const uint32_t eT = run_prefix(s_run[tpl], base + ST_N) - run_prefix(s_run[tpl], base);
            const int64_t D = (int64_t)eT + (int64_t)e - 2 * ((int64_t)c0 + (int64_t)c1);
            const int dl = tid - ST_HALF;
            int64_t key = (D << 9) | (int64_t)((dl < 0 ? -dl : dl) << 1) | (int64_t)(dl > 0 ? 1 : 0);
            key = wave_min_i64(key);
            if (lane == 0) s_min[w] = key;
            if (more) run_store(s_run[nxt], v);
            __syncthreads();
            key = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
            const int mag = (int)(key & 511) >> 1;
            prev = (key & 1) ? mag : -mag;
            if (tid == 0) {
                deltas[sg.frame_off + k] = (int16_t)prev;
                sum += (uint64_t)key >> 9;
                edges += (prev == -ST_HALF || prev == ST_HALF - 1) ? 1 : 0;
            }
            const int t = tpl; tpl = cnd; cnd = nxt; nxt = t;
        }
    }
    __syncthreads();
    if (tid == 0) {
        StretchFig f;
        f.sum_dist = sum;
        f.nonfinite = s_nf[0] + s_nf[1] + s_nf[2] + s_nf[3];
        f.edge_frames = edges;
        f.pad = 0;
        figs[blockIdx.x] = f;
    }
}

__global__ __launch_bounds__(256) void wsola_ola_kernel(const void* __restrict__ wav, int is16, const StretchSeg* __restrict__ segs,
                                                         const StretchTile* __restrict__ tiles, const int16_t* __restrict__ deltas,
                                                         const float* __restrict__ win, float* __restrict__ out, int16_t* __restrict__ out_i16) {
    const StretchTile tl = tiles[blockIdx.x];
    const StretchSeg sg = segs[tl.seg];
    const int j = threadIdx.x;
    const float w1 = win[j], w0 = 1.0f - w1;      // both exact in fp32
    for (int f = 0; f < STRETCH_OLA_FRAMES; ++f) {
        const int k = tl.k0 + f;
        if (k >= sg.frames) break;
        const int64_t m = (int64_t)k * ST_H + j;
        const int64_t pk = stretch_a(k, sg.len_in, sg.len_out) + deltas[sg.frame_off + k];
        const int64_t pp = k > 0 ? stretch_a(k - 1, sg.len_in, sg.len_out) + deltas[sg.frame_off + k - 1] : -(int64_t)ST_H;
        if (m < sg.len_out) {
            const float x1 = sample_or_zero(wav, is16, sg.in_off, sg.len_in, pk + j);
            const float x0 = sample_or_zero(wav, is16, sg.in_off, sg.len_in, pp + ST_H + j);
            const float y = (float)((double)w1 * (double)x1 + (double)w0 * (double)x0);
            out[sg.out_off + m] = y;
            if (out_i16) out_i16[sg.out_off + m] = y != y ? (int16_t)0 : s16_trunc(y);      // NaN -> 0
        }
    }
}

int launch_wsola_search(const void* wav, int is16, const StretchSeg* segs, int B, int16_t* deltas, StretchFig* figs, hipStream_t s) {
    if (B < 1) return -1;
    hipLaunchKernelGGL(wsola_search_kernel, dim3((unsigned)B), dim3(256), 0, s, wav, is16, segs, deltas, figs);
    return 0;
}

int launch_wsola_ola(const void* wav, int is16, const StretchSeg* segs, const StretchTile* tiles, int64_t n_tiles, const int16_t* deltas, const float* win,
                     float* out, int16_t* out_i16, hipStream_t s) {
    if (n_tiles < 1 || n_tiles > INT_MAX) return -1;
    hipLaunchKernelGGL(wsola_ola_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, wav, is16, segs, tiles, deltas, win, out, out_i16);
    return 0;
}

}  // namespace ev
