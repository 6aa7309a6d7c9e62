// Long-form stitching (ev_stitch): the S segments of one synthesis batch -> finished documents: each segment cut at its edge silence, laid out with
// pauses or cross-fades between neighbours, ramped at its free ends, and written as fp32 and, when asked, as clamped int16.  include/evhip.h states
// the specification.
//
// stitch_peak: grid (ST_PEAK_CHUNK-sample chunks, segment), one partial max |x| per block -- a long segment spreads over many blocks.
// stitch_edges: one block per segment: the peak from the partials, the threshold, then ST_EDGE_CHUNK-sample chunks from the front until one holds a
//   sample above the threshold (block-wide min of indices) and the same from the back (max): it reads the silence it removes, not the segment.
//   Max, min-index and max-index reductions are exact in any order.
// stitch_mix: one block per ST_TILE output samples of one document, 256 threads x 4 samples.  The ramp table sits in LDS.  The block finds the first
//   segment that reaches into its tile by a binary search (the segments' ends pos + n are non-decreasing in a document, as are their starts) and
//   walks forward while segments start inside the tile; a sample's contributions are formed in segment order, at most two (ev_stitch_plan's clamps).
//   The specification's products and its sum are rounded one by one: mul_rn / add_rn (ev_audio_dev.h).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

namespace {

// r(i, L) of the specification: i < L <= F <= ST_MAX_FADE, so (2 i + 1) F < 2^26 and the 32-bit quotient is the int64 one
__device__ inline float ramp(int64_t i, int L, int F, const float* tab) {
    if (L == 0 || i >= L) return 1.0f;
    return tab[((2u * (unsigned)i + 1u) * (unsigned)F) / (2u * (unsigned)L)];
}

}  // namespace

__global__ __launch_bounds__(256) void stitch_peak_kernel(const float* __restrict__ wav, const StitchSeg* __restrict__ segs, float* __restrict__ part) {
    __shared__ float s_pk[4];
    const StitchSeg sg = segs[blockIdx.y];
    const int64_t base = (int64_t)blockIdx.x * ST_PEAK_CHUNK;
    if (base >= sg.len) return;
    const float* v = wav + sg.off;
    const int tid = threadIdx.x;
    float pk = 0.f;
#pragma unroll
    for (int r = 0; r < ST_PEAK_CHUNK / 256; ++r) {
        const int64_t i = base + r * 256 + tid;
        if (i < sg.len) pk = fmaxf(pk, fabsf(v[i]));
    }
    pk = wave_max_f32(pk);
    if ((tid & 63) == 0) s_pk[tid >> 6] = pk;
    __syncthreads();
    if (tid == 0) part[sg.part_off + blockIdx.x] = fmaxf(fmaxf(s_pk[0], s_pk[1]), fmaxf(s_pk[2], s_pk[3]));
}

// peak[s] = max |x|; cuts[2 s] = the first index with |x| > thr, cuts[2 s + 1] = the last one, thr = max(peak * frac, abs_thr); no such index: -1, -1
__global__ __launch_bounds__(256) void stitch_edges_kernel(const float* __restrict__ wav, const StitchSeg* __restrict__ segs, const float* __restrict__ part,
                                                            float frac, float abs_thr, float* __restrict__ peak, int64_t* __restrict__ cuts) {
    __shared__ float s_pk[4];
    __shared__ int64_t s_ix[4];
    const StitchSeg sg = segs[blockIdx.x];
    const float* v = wav + sg.off;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int64_t n_part = (sg.len + ST_PEAK_CHUNK - 1) / ST_PEAK_CHUNK;
    float pk = 0.f;
    for (int64_t i = tid; i < n_part; i += 256) pk = fmaxf(pk, part[sg.part_off + i]);
    pk = wave_max_f32(pk);
    if (lane == 0) s_pk[w] = pk;
    __syncthreads();
    pk = fmaxf(fmaxf(s_pk[0], s_pk[1]), fmaxf(s_pk[2], s_pk[3]));
    const float thr = fmaxf(mul_rn(pk, frac), abs_thr);
    int64_t first = -1, last = -1;
    for (int64_t c0 = 0; c0 < sg.len; c0 += ST_EDGE_CHUNK) {
        int64_t lo = INT64_MAX;
#pragma unroll
        for (int r = ST_EDGE_CHUNK / 256 - 1; r >= 0; --r) {      // descending: the thread's smallest hit stays
            const int64_t i = c0 + r * 256 + tid;
            if (i < sg.len && fabsf(v[i]) > thr) lo = i;
        }
        lo = wave_min_i64(lo);
        __syncthreads();      // the reads of the round before
        if (lane == 0) s_ix[w] = lo;
        __syncthreads();
        lo = min(min(s_ix[0], s_ix[1]), min(s_ix[2], s_ix[3]));
        if (lo != INT64_MAX) { first = lo; break; }      // the same value in every thread
    }
    if (first >= 0) {      // then the walk from the back ends at a hit as well
        for (int64_t c1 = sg.len; c1 > 0; c1 -= ST_EDGE_CHUNK) {
            const int64_t c0 = max(c1 - (int64_t)ST_EDGE_CHUNK, (int64_t)0);
            int64_t hi = -1;
#pragma unroll
            for (int r = 0; r < ST_EDGE_CHUNK / 256; ++r) {
                const int64_t i = c0 + r * 256 + tid;
                if (i < c1 && fabsf(v[i]) > thr) hi = i;
            }
            hi = wave_max_i64(hi);
            __syncthreads();
            if (lane == 0) s_ix[w] = hi;
            __syncthreads();
            hi = max(max(s_ix[0], s_ix[1]), max(s_ix[2], s_ix[3]));
            if (hi >= 0) { last = hi; break; }
        }
    }
    if (tid == 0) { peak[blockIdx.x] = pk; cuts[2 * blockIdx.x] = first; cuts[2 * blockIdx.x + 1] = last; }
}

__global__ __launch_bounds__(256) void stitch_mix_kernel(const float* __restrict__ wav, const StitchMixSeg* __restrict__ segs, const StitchDoc* __restrict__ docs,
                                                          const StitchTile* __restrict__ tiles, const float* __restrict__ tab, int F,
                                                          float* __restrict__ out, int16_t* __restrict__ out_i16) {
    extern __shared__ __attribute__((aligned(16))) float s_tab[];
    const int tid = threadIdx.x;
    const StitchTile tl = tiles[blockIdx.x];
    const StitchDoc dc = docs[tl.doc];
    for (int i = tid; i < F; i += 256) s_tab[i] = tab[i];
    __syncthreads();
    const int64_t t0 = (int64_t)tl.tile * ST_TILE, t1 = min(t0 + ST_TILE, dc.len);
    const StitchMixSeg* sg = segs + dc.seg0;
    int lo = 0, hi = dc.nseg;      // the first segment whose end lies beyond t0
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (sg[mid].pos + sg[mid].n > t0) hi = mid; else lo = mid + 1;
    }
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    unsigned hit = 0;
    for (int s = lo; s < dc.nseg; ++s) {
        const StitchMixSeg q = sg[s];
        if (q.pos >= t1) break;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int64_t i = t0 + r * 256 + tid - q.pos;
            if (i >= 0 && i < q.n) {
                const float g = mul_rn(ramp(i, q.fl, F, s_tab), ramp(q.n - 1 - i, q.fr, F, s_tab));
                const float c = mul_rn(wav[q.src + i], g);
                acc[r] = (hit >> r & 1u) ? add_rn(acc[r], c) : c;
                hit |= 1u << r;
            }
        }
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t p = t0 + r * 256 + tid;
        if (p < t1) {
            out[dc.out_off + p] = acc[r];
            if (out_i16) out_i16[dc.out_off + p] = s16_trunc(acc[r]);
        }
    }
}

void launch_stitch_peak(const float* wav, const StitchSeg* segs, int S, int64_t max_len, float* part, hipStream_t s) {
    hipLaunchKernelGGL(stitch_peak_kernel, dim3((unsigned)((max_len + ST_PEAK_CHUNK - 1) / ST_PEAK_CHUNK), (unsigned)S), dim3(256), 0, s, wav, segs, part);
}

void launch_stitch_edges(const float* wav, const StitchSeg* segs, int S, const float* part, float frac, float abs_thr, float* peak, int64_t* cuts,
                         hipStream_t s) {
    hipLaunchKernelGGL(stitch_edges_kernel, dim3((unsigned)S), dim3(256), 0, s, wav, segs, part, frac, abs_thr, peak, cuts);
}

int launch_stitch_mix(const float* wav, const StitchMixSeg* segs, const StitchDoc* docs, const StitchTile* tiles, int64_t n_tiles, const float* tab, int F,
                      float* out, int16_t* out_i16, hipStream_t s) {
    if (n_tiles < 1) return 0;      // every document empty
    if (F < 0 || F > ST_MAX_FADE || n_tiles > INT_MAX) return -1;
    hipLaunchKernelGGL(stitch_mix_kernel, dim3((unsigned)n_tiles), dim3(256), (size_t)F * sizeof(float), s, wav, segs, docs, tiles, tab, F, out, out_i16);
    return 0;
}

}  // namespace ev
