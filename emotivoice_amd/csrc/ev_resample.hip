// Sample-rate conversion and trimming (ev_resample): wav at sr_in -> wav at sr_out by a polyphase windowed-sinc filter, then the reference's silence
// trim (prompt_dataset.get_mel: cut what lies below a fraction of the peak, pad zeros on each side).  include/evhip.h states the specification.
//
// resample_poly: one block = RS_TM consecutive outputs of one utterance, one output per thread.  The tile's run of input samples is kept in LDS as
// fp32 (zero outside the utterance) when it fits; a run that does not fit (a large down / up, or a long custom filter) is read through L1 with the
// same bounds.  The taps live in a phase-major table: row p = (m down) mod up lists h[i], i = p (mod up), from the largest i <= half downwards, which
// is the order k ascends in; rows are padded to an odd length so that lanes on different phases fall on different LDS banks.  The table is copied
// into LDS when it fits beside the run (44.1 -> 16 kHz: 57 KB), else read through L1 (it stays L2-resident); polyphase_lds decides both.  Whichever
// way, output m is polyphase_sum (ev_audio_dev.h, where the order of the sum is stated): its bits depend on (utterance, m).
// trim_scan: one block per utterance, the peak first, then the first and the last index above peak * frac (max and min reductions: exact in any order).
// trim_gather: the padded cuts at their final offsets.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

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
int64_t polyphase_run_max(int tile, int up, int down, int half) { return ((int64_t)(tile - 1) * down + 2 * (int64_t)half) / up + 2; }
PolyphaseLds polyphase_lds(int tile, int up, int down, int half, bool padded) {
    const int64_t run = polyphase_run_max(tile, up, down, half), cap = padded ? run + run / 32 + 1 : run;      // floats of LDS, the unused ones included
    const size_t run_bytes = (size_t)cap * sizeof(float), tab_bytes = resample_table_floats(up, half) * sizeof(float);
    PolyphaseLds r;
    r.run_lds = run_bytes <= (size_t)POLY_MAX_RUN_BYTES;
    r.tab_lds = (r.run_lds ? run_bytes : 0) + tab_bytes <= (size_t)POLY_MAX_LDS;
    r.run_cap = r.run_lds ? (int)cap : 0;
    r.bytes = (r.run_lds ? run_bytes : 0) + (r.tab_lds ? tab_bytes : 0);
    return r;
}

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
    if (RUN_LDS)      // k_last - k_first + 1 <= run_cap (polyphase_run_max)
        stage_run<RS_TM>([&](int i) -> float& { return run[i]; }, p.wav, p.wav_is_i16, sq.in_off, L, k_first, (int)(k_last - k_first + 1));
    if (TAB_LDS) {
        const int NT = p.up * p.row;
        for (int i = tid; i < NT; i += RS_TM) ltab[i] = p.tab[i];
    }
    if (RUN_LDS || TAB_LDS) __syncthreads();
    const int m = m0 + tid;
    if (m > m1) return;
    int64_t k_lo;
    int nk, ph;
    polyphase_taps(m, up, down, half, &k_lo, &nk, &ph);
    const float* h = (TAB_LDS ? ltab : p.tab) + (size_t)ph * p.row;
    const float* x = run + (k_lo - k_first);
    p.out[sq.out_off + m] = RUN_LDS ? polyphase_sum([&](int j) { return x[j]; }, h, nk)
                                    : polyphase_sum([&](int j) { return sample_or_zero(p.wav, p.wav_is_i16, sq.in_off, L, k_lo + j); }, h, nk);
}

// sr_in == sr_out: the packed input and the packed output have one layout
__global__ __launch_bounds__(256) void resample_copy_kernel(const void* __restrict__ wav, int wav_is_i16, int64_t total, float* __restrict__ out) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < total; i += (int64_t)gridDim.x * 256) out[i] = load_sample(wav, wav_is_i16, i);
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
    pk = wave_max_f32(pk);
    if (lane == 0) s_peak[w] = pk;
    __syncthreads();
    pk = fmaxf(fmaxf(s_peak[0], s_peak[1]), fmaxf(s_peak[2], s_peak[3]));
    const float thr = __fmul_rn(pk, frac);
    int64_t lo = INT64_MAX, hi = -1;
    for (int64_t i = tid; i < sq.n; i += 256)
        if (fabsf(v[i]) > thr) { lo = min(lo, i); hi = i; }
    lo = wave_min_i64(lo);
    hi = wave_max_i64(hi);
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
    const PolyphaseLds l = polyphase_lds(RS_TM, p.up, p.down, p.half, false);
    ResampleParams q = p;
    q.run_cap = l.run_cap;
    void (*fn)(const ResampleParams) = l.run_lds ? (l.tab_lds ? resample_poly_kernel<true, true> : resample_poly_kernel<true, false>)
                                                 : (l.tab_lds ? resample_poly_kernel<false, true> : resample_poly_kernel<false, false>);
    if (hipFuncSetAttribute((const void*)fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)l.bytes) != hipSuccess) return -1;
    hipLaunchKernelGGL(fn, dim3((unsigned)p.n_tiles), dim3(RS_TM), l.bytes, s, q);
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
