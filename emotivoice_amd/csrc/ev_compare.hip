// Signal comparison (ev_compare): two packed batches of fp32 segments -> per-segment fp64 sums of d, d^2, y, y^2 (d = a - b, y = b), max |d| with
// its first index, max |y| and the count of non-finite elements.  include/evhip.h states the specification, the summation order included.
//
// compare_chunks: one block per CMP_CHUNK-element chunk of one segment (a host-built table: segments have ragged lengths).  Thread t owns the
//   chunk's elements t, t + 256, ... and adds them in ascending order; the 256 thread sums meet in the halving tree s[t] += s[t + 128], + 64, ..., + 1.
//   A full chunk whose first element is 16-byte aligned in both signals is fetched as float4 (four per thread and signal) and handed to the owning
//   threads through LDS; any other chunk is read element by element at stride 256, which a wave still fetches as whole lines.  Both paths feed
//   the same accumulation, so the load width does not reach the bits.  Measured at 1 GB per signal pair: 5.3 TB/s staged, 2.7 TB/s element-wise
//   (profiles/compare_cost.json).
// compare_finish: five waves per segment; four add one of the four sums over the segment's chunks in ascending order, the fifth folds the maxima,
//   the first index and the non-finite count.  No atomics anywhere: block arrival order does not reach the result.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

// every term and every sum of the specification is rounded on its own: no d * d + s as one fma
#pragma clang fp contract(off)

namespace ev {

namespace {

struct Acc { double d, d2, y, y2, md; float py; int ix, nf; };

// one element into its owner's accumulators; i = the element's index inside the chunk (ascending per thread, so `>` keeps the first maximum)
__device__ inline void take(Acc& c, float xa, float xb, int i) {
    const double x = (double)xa, y0 = (double)xb;
    const bool ok = isfinite(xa) && isfinite(xb);
    const double d = ok ? x - y0 : 0.0, y = ok ? y0 : 0.0;
    c.nf += ok ? 0 : 1;
    c.d += d; c.d2 += d * d; c.y += y; c.y2 += y * y;
    const double ad = fabs(d);
    if (ad > c.md) { c.md = ad; c.ix = i; }
    c.py = fmaxf(c.py, ok ? fabsf(xb) : 0.f);
}

}  // namespace

__global__ __launch_bounds__(256) void compare_chunks_kernel(const float* __restrict__ a, const float* __restrict__ b, const CompareChunk* __restrict__ chunks,
                                                              double* __restrict__ sums /* 4 planes of n_chunks */, int64_t n_chunks,
                                                              double* __restrict__ maxd, int32_t* __restrict__ argd, float* __restrict__ peak,
                                                              int32_t* __restrict__ nonf) {
    // the staged chunk (a, then b) and, once every thread has taken its elements out of it, the reduction tree in the same bytes
    __shared__ __attribute__((aligned(16))) float s_raw[2 * CMP_CHUNK];
    float* s_a = s_raw;
    float* s_b = s_raw + CMP_CHUNK;
    double (*s_sum)[256] = reinterpret_cast<double (*)[256]>(s_raw);      // 4 x 256 doubles
    double* s_md = reinterpret_cast<double*>(s_raw) + 4 * 256;
    float* s_py = reinterpret_cast<float*>(s_md + 256);
    int* s_ix = reinterpret_cast<int*>(s_py + 256);
    int* s_nf = s_ix + 256;
    const int tid = threadIdx.x;
    const CompareChunk ck = chunks[blockIdx.x];
    const float* pa = a + ck.off;
    const float* pb = b + ck.off;
    Acc c{0.0, 0.0, 0.0, 0.0, 0.0, 0.f, 0, 0};
    const bool wide = ck.n == CMP_CHUNK && (((uintptr_t)pa | (uintptr_t)pb) & 15u) == 0;      // the same in every thread of the block
    if (wide) {
#pragma unroll
        for (int r = 0; r < CMP_CHUNK / 1024; ++r) {
            const int q = r * 256 + tid;
            reinterpret_cast<float4*>(s_a)[q] = reinterpret_cast<const float4*>(pa)[q];
            reinterpret_cast<float4*>(s_b)[q] = reinterpret_cast<const float4*>(pb)[q];
        }
        __syncthreads();
#pragma unroll
        for (int r = 0; r < CMP_CHUNK / 256; ++r) take(c, s_a[r * 256 + tid], s_b[r * 256 + tid], r * 256 + tid);
    } else {
#pragma unroll 4
        for (int r = 0; r < CMP_CHUNK / 256; ++r) {
            const int i = r * 256 + tid;
            if (i < ck.n) take(c, pa[i], pb[i], i);
        }
    }
    __syncthreads();      // the staged chunk has been read
    s_sum[0][tid] = c.d; s_sum[1][tid] = c.d2; s_sum[2][tid] = c.y; s_sum[3][tid] = c.y2;
    s_md[tid] = c.md; s_ix[tid] = c.ix; s_py[tid] = c.py; s_nf[tid] = c.nf;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) {
#pragma unroll
            for (int k = 0; k < 4; ++k) s_sum[k][tid] += s_sum[k][tid + o];
            const double m = s_md[tid + o];
            const int ix = s_ix[tid + o];
            if (m > s_md[tid] || (m == s_md[tid] && ix < s_ix[tid])) { s_md[tid] = m; s_ix[tid] = ix; }
            s_py[tid] = fmaxf(s_py[tid], s_py[tid + o]);
            s_nf[tid] += s_nf[tid + o];
        }
        __syncthreads();
    }
    if (tid < 4) sums[(int64_t)tid * n_chunks + blockIdx.x] = s_sum[tid][0];
    if (tid == 4) { maxd[blockIdx.x] = s_md[0]; argd[blockIdx.x] = s_ix[0]; peak[blockIdx.x] = s_py[0]; nonf[blockIdx.x] = s_nf[0]; }
}

// grid (segment, 5), one wave each.  y = 0 .. 3: sum plane y over the segment's chunks, one after the other.  The chain of additions is serial by
// specification, the loads are not: the wave fetches 64 chunk sums at a time (and the next 64 while it adds), then every lane adds them in chunk
// order out of lane 0, 1, ..., 63.  Chunks past the segment's end enter as +0.0, which changes no bit of a sum that started at +0.0.
// y = 4: the maxima, the first index and the non-finite count, which are exact in any order: a strided pass and a wave butterfly.
__global__ __launch_bounds__(64) void compare_finish_kernel(const int64_t* __restrict__ chunk_offs /* (B + 1,) */, const double* __restrict__ sums,
                                                             int64_t n_chunks, const double* __restrict__ maxd, const int32_t* __restrict__ argd,
                                                             const float* __restrict__ peak, const int32_t* __restrict__ nonf, CompareSeg* __restrict__ out) {
    const int seg = blockIdx.x, q = blockIdx.y, lane = threadIdx.x;
    const int64_t c0 = chunk_offs[seg], c1 = chunk_offs[seg + 1];
    if (q < 4) {
        const double* p = sums + (int64_t)q * n_chunks;
        double s = 0.0;
        double cur = c0 + lane < c1 ? p[c0 + lane] : 0.0;
        for (int64_t base = c0; base < c1; base += 64) {
            const double nxt = base + 64 + lane < c1 ? p[base + 64 + lane] : 0.0;
#pragma unroll
            for (int j = 0; j < 64; ++j) s += lane_value(cur, j);
            cur = nxt;
        }
        if (lane == 0) out[seg].sum[q] = s;
        return;
    }
    double md = 0.0; int64_t ix = 0, nf = 0; float py = 0.f;
    for (int64_t c = c0 + lane; c < c1; c += 64) {      // ascending per lane, so `>` keeps the lane's first chunk that attains its maximum
        if (maxd[c] > md) { md = maxd[c]; ix = (c - c0) * CMP_CHUNK + argd[c]; }
        py = fmaxf(py, peak[c]);
        nf += nonf[c];
    }
    // (max, first index) has a tie-break of its own.  py and nf stay inside its butterfly: folded after it by wave_max_f32 / wave_sum_i64, the
    // kernel measured 0.6 % slower.
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        const double m2 = __shfl_xor(md, o, 64);
        const int64_t i2 = (int64_t)__shfl_xor((long long)ix, o, 64);
        if (m2 > md || (m2 == md && i2 < ix)) { md = m2; ix = i2; }
        py = fmaxf(py, __shfl_xor(py, o, 64));
        nf += (int64_t)__shfl_xor((long long)nf, o, 64);
    }
    if (lane == 0) { out[seg].max_d = md; out[seg].arg = ix; out[seg].nonfinite = nf; out[seg].peak_y = py; out[seg].pad = 0; }
}

int launch_compare_chunks(const float* a, const float* b, const CompareChunk* chunks, int64_t n_chunks, double* sums, double* maxd, int32_t* argd,
                          float* peak, int32_t* nonf, hipStream_t s) {
    if (n_chunks < 1 || n_chunks > INT_MAX) return -1;
    hipLaunchKernelGGL(compare_chunks_kernel, dim3((unsigned)n_chunks), dim3(256), 0, s, a, b, chunks, sums, n_chunks, maxd, argd, peak, nonf);
    return 0;
}

void launch_compare_finish(int B, const int64_t* chunk_offs, const double* sums, int64_t n_chunks, const double* maxd, const int32_t* argd,
                           const float* peak, const int32_t* nonf, CompareSeg* out, hipStream_t s) {
    hipLaunchKernelGGL(compare_finish_kernel, dim3((unsigned)B, 5), dim3(64), 0, s, chunk_offs, sums, n_chunks, maxd, argd, peak, nonf, out);
}

}  // namespace ev
