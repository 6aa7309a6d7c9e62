// Sample-rate conversion and trimming (ev_resample): wav at sr_in -> wav at sr_out by a polyphase windowed-sinc filter, then the reference's silence
// trim (prompt_dataset.get_mel: cut what lies below a fraction of the peak, pad zeros on each side).  include/evhip.h states the specification.
//
// resample_poly: one block = RS_TM consecutive outputs of one utterance, one output per thread.  The tile's run of input samples is kept in LDS as
// fp32 (zero outside the utterance) when it fits; a run that does not fit (a large down / up, or a long custom filter) is read through L1 with the
// same bounds.  The taps live in a phase-major table: row p = (m down) mod up lists h[i], i = p (mod up), from the largest i <= half downwards, which
// is the order k ascends in; rows are padded to an odd length so that lanes on different phases fall on different LDS banks.  The table is copied
// into LDS when it fits beside the run (44.1 -> 16 kHz: 57 KB), else read through L1 (it stays L2-resident).  Whichever way, output m sums its
// products in four interleaved partial sums over (k - k_lo) mod 4, k ascending, combined as (s0 + s1) + (s2 + s3): its bits depend on (utterance, m).
// trim_scan: one block per utterance, the peak first, then the first and the last index above peak * frac (max and min reductions: exact in any order).
// trim_gather: the padded cuts at their final offsets.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_kernels.h"

namespace ev {

namespace {

__host__ __device__ inline int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && (a < 0)) ? q - 1 : q; }      // b > 0
__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

}  // namespace

int resample_row_len(int up, int half) { return ((2 * half) / up + 1) | 1; }
size_t resample_table_floats(int up, int half) { return (size_t)up * (size_t)resample_row_len(up, half); }
void resample_pack_table(int up, int half, const float* taps, float* out) {
    const int row = resample_row_len(up, half);
    for (int p = 0; p < up; ++p) {
        const int i0 = half - (int)(((int64_t)half - p) % up + up) % up;      // the largest i <= half with i = p (mod up)
        for (int j = 0; j < row; ++j) {
            const int64_t i = (int64_t)i0 - (int64_t)j * up;
            out[(size_t)p * row + j] = i >= -half ? taps[half + i] : 0.f;
        }
    }
}
int64_t resample_run_max(int up, int down, int half) { return ((int64_t)(RS_TM - 1) * down + 2 * (int64_t)half) / up + 2; }

template <bool RUN_LDS, bool TAB_LDS>
__global__ __launch_bounds__(RS_TM) void resample_poly_kernel(const ResampleParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x;
    const ResampleTile tl = p.tiles[blockIdx.x];
    const ResampleSeq sq = p.seqs[tl.seq];
    const int64_t L = sq.len, up = p.up, down = p.down, half = p.half;
    const int m0 = tl.m0, m1 = (int)min((int64_t)m0 + RS_TM, sq.n) - 1;      // the tile's outputs m0 .. m1
    const int64_t k_first = ceil_div((int64_t)m0 * down - half, up), k_last = floor_div((int64_t)m1 * down + half, up);
    float* run = reinterpret_cast<float*>(smem);
    float* ltab = run + (RUN_LDS ? p.run_cap : 0);
    const float* wf = reinterpret_cast<const float*>(p.wav) + sq.in_off;
    const int16_t* wi = reinterpret_cast<const int16_t*>(p.wav) + sq.in_off;
    if (RUN_LDS) {
        const int NS = (int)(k_last - k_first + 1);      // <= run_cap (resample_run_max)
        for (int i = tid; i < NS; i += RS_TM) {
            const int64_t s = k_first + i;
            float v = 0.f;
            if (s >= 0 && s < L) v = p.wav_is_i16 ? (float)wi[s] * (1.0f / 32768.0f) : wf[s];
            run[i] = v;
        }
    }
    if (TAB_LDS) {
        const int NT = p.up * p.row;
        for (int i = tid; i < NT; i += RS_TM) ltab[i] = p.tab[i];
    }
    if (RUN_LDS || TAB_LDS) __syncthreads();
    const int m = m0 + tid;
    if (m > m1) return;
    const int64_t md = (int64_t)m * down;
    const int64_t k_lo = ceil_div(md - half, up), k_hi = floor_div(md + half, up);
    const int nk = (int)(k_hi - k_lo + 1);
    const int ph = (int)(md % up);
    const float* h = (TAB_LDS ? ltab : p.tab) + (size_t)ph * p.row;
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    if (RUN_LDS) {
        const float* x = run + (k_lo - k_first);
        int j = 0;
        for (; j + 4 <= nk; j += 4) {
            s0 = fmaf(x[j], h[j], s0); s1 = fmaf(x[j + 1], h[j + 1], s1); s2 = fmaf(x[j + 2], h[j + 2], s2); s3 = fmaf(x[j + 3], h[j + 3], s3);
        }
        if (j < nk) { s0 = fmaf(x[j], h[j], s0); ++j; }
        if (j < nk) { s1 = fmaf(x[j], h[j], s1); ++j; }
        if (j < nk) { s2 = fmaf(x[j], h[j], s2); }
    } else {
        auto x = [&](int j) -> float {
            const int64_t k = k_lo + j;
            if (k < 0 || k >= L) return 0.f;
            return p.wav_is_i16 ? (float)wi[k] * (1.0f / 32768.0f) : wf[k];
        };
        int j = 0;
        for (; j + 4 <= nk; j += 4) {
            s0 = fmaf(x(j), h[j], s0); s1 = fmaf(x(j + 1), h[j + 1], s1); s2 = fmaf(x(j + 2), h[j + 2], s2); s3 = fmaf(x(j + 3), h[j + 3], s3);
        }
        if (j < nk) { s0 = fmaf(x(j), h[j], s0); ++j; }
        if (j < nk) { s1 = fmaf(x(j), h[j], s1); ++j; }
        if (j < nk) { s2 = fmaf(x(j), h[j], s2); }
    }
    p.out[sq.out_off + m] = (s0 + s1) + (s2 + s3);
}

// sr_in == sr_out: the packed input and the packed output have one layout
__global__ __launch_bounds__(256) void resample_copy_kernel(const void* __restrict__ wav, int wav_is_i16, int64_t total, float* __restrict__ out) {
    const float* wf = reinterpret_cast<const float*>(wav);
    const int16_t* wi = reinterpret_cast<const int16_t*>(wav);
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256)
        out[i] = wav_is_i16 ? (float)wi[i] * (1.0f / 32768.0f) : wf[i];
}

// cuts[2 b] = first index with |y| > peak * frac, cuts[2 b + 1] = the last one; no such index: 0, 0
__global__ __launch_bounds__(256) void trim_scan_kernel(const float* __restrict__ y, const ResampleSeq* __restrict__ seqs, float frac,
                                                         int64_t* __restrict__ cuts) {
    __shared__ float s_peak[4];
    __shared__ int64_t s_lo[4], s_hi[4];
    const ResampleSeq sq = seqs[blockIdx.x];
    const float* v = y + sq.out_off;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    float pk = 0.f;
    for (int64_t i = tid; i < sq.n; i += 256) pk = fmaxf(pk, fabsf(v[i]));
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) pk = fmaxf(pk, __shfl_xor(pk, o, 64));
    if (lane == 0) s_peak[w] = pk;
    __syncthreads();
    pk = fmaxf(fmaxf(s_peak[0], s_peak[1]), fmaxf(s_peak[2], s_peak[3]));
    const float thr = __fmul_rn(pk, frac);
    int64_t lo = INT64_MAX, hi = -1;
    for (int64_t i = tid; i < sq.n; i += 256)
        if (fabsf(v[i]) > thr) { lo = min(lo, i); hi = i; }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
        lo = min(lo, (int64_t)__shfl_xor((long long)lo, o, 64));
        hi = max(hi, (int64_t)__shfl_xor((long long)hi, o, 64));
    }
    if (lane == 0) { s_lo[w] = lo; s_hi[w] = hi; }
    __syncthreads();
    if (tid == 0) {
        lo = min(min(s_lo[0], s_lo[1]), min(s_lo[2], s_lo[3]));
        hi = max(max(s_hi[0], s_hi[1]), max(s_hi[2], s_hi[3]));
        cuts[2 * blockIdx.x] = hi < 0 ? 0 : lo;
        cuts[2 * blockIdx.x + 1] = hi < 0 ? 0 : hi;
    }
}

// out[dst_off + i], i < pad + cut + pad: zeros, y[src_off .. src_off + cut), zeros.  blockIdx.y = utterance, blockIdx.x = a run of 1024 outputs.
__global__ __launch_bounds__(256) void trim_gather_kernel(const float* __restrict__ y, const TrimSeq* __restrict__ seqs, int pad, float* __restrict__ out) {
    const TrimSeq sq = seqs[blockIdx.y];
    const int64_t n = sq.cut + 2 * (int64_t)pad;
    const int64_t base = (int64_t)blockIdx.x * 1024;
    if (base >= n) return;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int64_t i = base + r * 256 + threadIdx.x;
        if (i < n) {
            const int64_t c = i - pad;
            out[sq.dst_off + i] = (c >= 0 && c < sq.cut) ? y[sq.src_off + c] : 0.f;
        }
    }
}

int launch_resample_poly(const ResampleParams& p, hipStream_t s) {
    if (p.n_tiles <= 0 || p.up < 1 || p.down < 1 || p.half < 1 || p.row != resample_row_len(p.up, p.half)) return -1;
    const int64_t run_max = resample_run_max(p.up, p.down, p.half);
    const size_t tab_bytes = resample_table_floats(p.up, p.half) * sizeof(float);
    const bool run_lds = (size_t)run_max * sizeof(float) <= (size_t)RS_MAX_RUN_BYTES;
    const size_t run_bytes = run_lds ? (size_t)run_max * sizeof(float) : 0;
    const bool tab_lds = run_bytes + tab_bytes <= (size_t)RS_MAX_LDS;
    const size_t lds = run_bytes + (tab_lds ? tab_bytes : 0);
    ResampleParams q = p;
    q.run_cap = run_lds ? (int)run_max : 0;
    const void* fn = run_lds ? (tab_lds ? (const void*)resample_poly_kernel<true, true> : (const void*)resample_poly_kernel<true, false>)
                             : (tab_lds ? (const void*)resample_poly_kernel<false, true> : (const void*)resample_poly_kernel<false, false>);
    if (hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    const dim3 g((unsigned)p.n_tiles), b(RS_TM);
    if (run_lds && tab_lds) hipLaunchKernelGGL((resample_poly_kernel<true, true>), g, b, lds, s, q);
    else if (run_lds) hipLaunchKernelGGL((resample_poly_kernel<true, false>), g, b, lds, s, q);
    else if (tab_lds) hipLaunchKernelGGL((resample_poly_kernel<false, true>), g, b, lds, s, q);
    else hipLaunchKernelGGL((resample_poly_kernel<false, false>), g, b, lds, s, q);
    return 0;
}

void launch_resample_copy(const void* wav, int wav_is_i16, int64_t total, float* out, hipStream_t s) {
    const int64_t blocks = (total + 1023) / 1024;
    hipLaunchKernelGGL(resample_copy_kernel, dim3((unsigned)(blocks < 1 ? 1 : (blocks > 65536 ? 65536 : blocks))), dim3(256), 0, s, wav, wav_is_i16, total, out);
}

void launch_trim_scan(const float* y, const ResampleSeq* seqs, int B, float frac, int64_t* cuts, hipStream_t s) {
    hipLaunchKernelGGL(trim_scan_kernel, dim3((unsigned)B), dim3(256), 0, s, y, seqs, frac, cuts);
}

void launch_trim_gather(const float* y, const TrimSeq* seqs, int B, int64_t max_len, int pad, float* out, hipStream_t s) {
    if (max_len < 1) return;
    hipLaunchKernelGGL(trim_gather_kernel, dim3((unsigned)((max_len + 1023) / 1024), (unsigned)B), dim3(256), 0, s, y, seqs, pad, out);
}

}  // namespace ev
