// Device parts shared by the audio kernels (ev_pitch, ev_resample, ev_stitch, ev_compare, ev_loudness, ev_limit, ev_deliver, ev_score): wave
// reductions, the element rules that decide a bit, and the polyphase filter of ev_resample and ev_deliver.  Everything is inline with internal
// linkage: the library exports nothing from here.  Include it before a file-wide `#pragma clang fp contract`: it leaves contraction at the default
// (fast), as a file without pragmas has it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ev {

namespace {

// ---- wave reductions: the xor butterfly over 64 lanes, offset 32 down to 1; every lane ends with the result.  For the two floating sums the order
// is part of the specification (pitch's E0, loudness's step sums); max, min and the integer sums are exact in any order.
__device__ inline float wave_max_f32(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline float wave_min_f32(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = fminf(v, __shfl_xor(v, o, 64));
    return v;
}
__device__ inline float wave_sum_f32(float v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline double wave_sum_f64(double v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline int wave_sum_i32(int v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ inline int64_t wave_sum_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v += (int64_t)__shfl_xor((long long)v, o, 64);
    return v;
}
__device__ inline int64_t wave_min_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = min(v, (int64_t)__shfl_xor((long long)v, o, 64));
    return v;
}
__device__ inline int64_t wave_max_i64(int64_t v) {
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) v = max(v, (int64_t)__shfl_xor((long long)v, o, 64));
    return v;
}

// lane j's value in every lane (j the same in all of them)
__device__ inline double lane_value(double v, int j) {
    union { double d; int i[2]; } u;
    u.d = v;
    u.i[0] = __builtin_amdgcn_readlane(u.i[0], j);
    u.i[1] = __builtin_amdgcn_readlane(u.i[1], j);
    return u.d;
}

// ---- element rules
__device__ inline bool finite_f32(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }

// One rounded fp32 product / sum, never fused with anything.  __fmul_rn / __fadd_rn are plain operators compiled with contraction allowed, so a
// product followed by a sum would still fuse into an fma after inlining; these two carry no such licence.
#pragma clang fp contract(off)
__device__ inline float mul_rn(float a, float b) { return a * b; }
__device__ inline float add_rn(float a, float b) { return a + b; }
#pragma clang fp contract(fast)

// sample i of a packed fp32-or-int16 input: s / 32768 is exact
__device__ inline float load_sample(const void* wav, int is16, int64_t i) {
    return is16 ? (float)reinterpret_cast<const int16_t*>(wav)[i] * (1.0f / 32768.0f) : reinterpret_cast<const float*>(wav)[i];
}

// y -> int16: one rounded product, the clamp, truncation toward zero (the same integers as truncating first).  What a NaN becomes is the caller's rule.
__device__ inline int16_t s16_trunc(float y) { return (int16_t)(int)fminf(fmaxf(mul_rn(y, 32768.0f), -32768.0f), 32767.0f); }

__host__ __device__ inline int64_t floor_div(int64_t a, int64_t b) { const int64_t q = a / b; return (a % b != 0 && (a < 0)) ? q - 1 : q; }      // b > 0
__host__ __device__ inline int64_t ceil_div(int64_t a, int64_t b) { return -floor_div(-a, b); }

// ---- the polyphase filter.  Output m of an utterance is sum_k x[k] h[m down - k up] over the k with |m down - k up| <= half.  The taps come as
// the phase-major table of resample_pack_table: row `phase` lists them in the order k ascends in.
__device__ inline void polyphase_taps(int64_t m, int64_t up, int64_t down, int64_t half, int64_t* k_lo, int* nk, int* phase) {
    const int64_t md = m * down;
    *k_lo = ceil_div(md - half, up);
    *nk = (int)(floor_div(md + half, up) - *k_lo + 1);
    *phase = (int)(md % up);
}

// THE sum of ev_resample and ev_deliver: x(j) = input k_lo + j, h = the phase's row.  Four interleaved fmaf partial sums over j mod 4, j ascending,
// combined as (s0 + s1) + (s2 + s3).  Where x and h live (LDS, padded LDS, global memory) is the caller's functor and pointer, and reaches no bit.
template <class X>
__device__ inline float polyphase_sum(X x, const float* h, int nk) {
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int j = 0;
    for (; j + 4 <= nk; j += 4) {
        s0 = fmaf(x(j), h[j], s0); s1 = fmaf(x(j + 1), h[j + 1], s1); s2 = fmaf(x(j + 2), h[j + 2], s2); s3 = fmaf(x(j + 3), h[j + 3], s3);
    }
    if (j < nk) { s0 = fmaf(x(j), h[j], s0); ++j; }
    if (j < nk) { s1 = fmaf(x(j), h[j], s1); ++j; }
    if (j < nk) { s2 = fmaf(x(j), h[j], s2); }
    return (s0 + s1) + (s2 + s3);
}

// sample s of the utterance wav[in_off .. in_off + L), zero outside it
__device__ inline float sample_or_zero(const void* wav, int is16, int64_t in_off, int64_t L, int64_t s) {
    return (s >= 0 && s < L) ? load_sample(wav, is16, in_off + s) : 0.f;
}

// a block of THREADS stages the utterance's samples first .. first + NS - 1 as fp32: dst(i) is where sample first + i goes
template <int THREADS, class D>
__device__ inline void stage_run(D dst, const void* wav, int is16, int64_t in_off, int64_t L, int64_t first, int NS) {
    for (int i = threadIdx.x; i < NS; i += THREADS) dst(i) = sample_or_zero(wav, is16, in_off, L, first + i);
}

}  // namespace

}  // namespace ev
