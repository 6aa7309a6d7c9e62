// Device parts shared by the audio kernels (ev_features, ev_pitch, ev_resample, ev_stitch, ev_compare, ev_loudness, ev_limit, ev_deliver, ev_score,
// ev_denoise, ev_stretch, ev_watermark): wave reductions, the element rules that decide a bit, the polyphase filter of ev_resample and ev_deliver, and the windowed DFT of
// ev_features, ev_denoise and ev_watermark.  Everything is inline with internal
// linkage: the library exports nothing from here.  Include it before a file-wide `#pragma clang fp contract`: it leaves contraction at the default
// (fast), as a file without pragmas has it.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ev_kernels.h"

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
// the inclusive prefix sum over the wave: lane l ends with the sum of lanes 0 .. l (modulo 2^32, exact in any order)
__device__ inline uint32_t wave_scan_u32(uint32_t v) {
    const int lane = (int)(threadIdx.x & 63);
#pragma unroll
    for (int o = 1; o <= 32; o <<= 1) {
        const uint32_t below = (uint32_t)__shfl_up((int)v, o, 64);
        if (lane >= o) v += below;
    }
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

// the keyed integer hash of ev_deliver's dither and ev_watermark's pattern (include/evhip.h states it): dl_mix(seed, c) is the value of counter c
__host__ __device__ inline uint32_t dl_hash(uint32_t x) {
    x ^= x >> 16; x *= 0x7feb352du; x ^= x >> 15; x *= 0x846ca68bu; x ^= x >> 16;
    return x;
}
__host__ __device__ inline uint32_t dl_mix(uint32_t seed, uint64_t c) { return dl_hash(dl_hash((uint32_t)c + dl_hash(seed ^ (uint32_t)(c >> 32))) ^ seed); }

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

// ---- the windowed DFT of ev_features and ev_denoise: a GEMM with overlapping rows.  Row t of the A operand is padded[hop t .. hop t + n_fft), so a
// tile of STFT_TF frames is ONE run of (STFT_TF - 1) hop + n_fft samples, kept in LDS as fp16 hi / lo planes (x = hi + 2^-11 lo); ev_kernels.h states
// the layout (stft_spad, stft_plane_halfs).  A forward kernel is stft_begin, its own staging, __syncthreads(), then stft_tile_loop with its epilogue.
typedef _Float16 half8 __attribute__((ext_vector_type(8)));
typedef _Float16 half2v __attribute__((ext_vector_type(2)));
typedef float f4 __attribute__((ext_vector_type(4)));

// a block of 256 threads stages samples first .. first + NS - 1 of the utterance wav[wav_off .. wav_off + L) as the two planes: reflected at
// both ends, int16 converted (x / 32768), zero where the reflection still falls outside (frames of the tile that are never written)
__device__ inline void stft_stage_planes(_Float16* sh, _Float16* sl, const void* wav, int is16, int64_t wav_off, int64_t L, int64_t first, int NS) {
    const float* wf = reinterpret_cast<const float*>(wav) + wav_off;
    const int16_t* wi = reinterpret_cast<const int16_t*>(wav) + wav_off;
    for (int i = threadIdx.x; i < NS; i += 256) {
        int64_t s = first + i;
        if (s < 0) s = -s;
        if (s >= L) s = 2 * (L - 1) - s;
        float v = 0.f;
        if (s >= 0 && s < L) v = is16 ? (float)wi[s] * (1.0f / 32768.0f) : wf[s];
        const _Float16 h = (_Float16)v;
        sh[stft_spad(i)] = h;
        sl[stft_spad(i)] = (_Float16)((v - (float)h) * 2048.0f);
    }
}

// one gained cell (g Re, g Im) into the scratch planes of ev_denoise and ev_watermark: `at` = row k_pad + 2 bin, each value split as hi + 2^-11 lo
__device__ inline void stft_store_cell(uint16_t* spec_hi, uint16_t* spec_lo, size_t at, float vr, float vi) {
    const _Float16 hr = (_Float16)vr, hi = (_Float16)vi;
    *reinterpret_cast<half2v*>(reinterpret_cast<_Float16*>(spec_hi) + at) = half2v{hr, hi};
    *reinterpret_cast<half2v*>(reinterpret_cast<_Float16*>(spec_lo) + at) =
        half2v{(_Float16)((vr - (float)hr) * 2048.0f), (_Float16)((vi - (float)hi) * 2048.0f)};
}

// One wave's share of one basis tile: its 32 frames (two 16-row tiles, A fragments at aoff[a] + 32 step) times the re and im columns of its 16
// bins.  bp: the wave's packed basis (stft_pack_basis) at its lane; per 32-sample step 2 A fragments (hi, lo) from LDS, 4 B fragments (prefetched
// one step ahead) and 12 MFMAs.  acc[a][c] takes hi x hi, accl[a][c] the two cross terms (in units of 2^-11); c = 0 re, 1 im.
__device__ inline void stft_tile_gemm(const _Float16* sh, const _Float16* sl, const half8* bp, int KS, const int aoff[2], f4 acc[2][2], f4 accl[2][2]) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 2; ++c) { acc[a][c] = f4{0.f, 0.f, 0.f, 0.f}; accl[a][c] = f4{0.f, 0.f, 0.f, 0.f}; }
    half8 bn[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) bn[q] = bp[q * 64];
    for (int ks = 0; ks < KS; ++ks) {
        half8 b[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) b[q] = bn[q];
        if (ks + 1 < KS) {
#pragma unroll
            for (int q = 0; q < 4; ++q) bn[q] = bp[(size_t)(ks + 1) * 256 + q * 64];
        }
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int at = stft_spad(aoff[a] + ks * 32);
            const half8 ah = *reinterpret_cast<const half8*>(sh + at);
            const half8 al = *reinterpret_cast<const half8*>(sl + at);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, b[2 * c], acc[a][c], 0, 0, 0);
                accl[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(ah, b[2 * c + 1], accl[a][c], 0, 0, 0);
                accl[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(al, b[2 * c], accl[a][c], 0, 0, 0);
            }
        }
    }
}

// A thread's place in a forward block of 4 waves: wave (nb, mh) multiplies frames 32 mh .. + 31 of the tile (two 16-row tiles a) into the re and im
// columns of bins 16 nb .. + 15 of each basis tile, and lane (fr, g) ends with bin fr of the frames 4 g + r.
struct StftLane {
    StftSeq sq; int seq, t0;      // the utterance, its index, the tile's first frame
    int fr, g, nb, mh;
    const _Float16 *sh, *sl;      // the staged planes
    __device__ int frame(int a, int r) const { return mh * 32 + a * 16 + g * 4 + r; }      // the frame of the tile that re[a][r], im[a][r] belong to
};

// The start of a forward block of 256 threads: looks its tile up, carves the two planes from the dynamic LDS at `smem` and stages them.  *tail is
// what follows the planes, 16-byte aligned; the planes may be read after the kernel's next __syncthreads().
__device__ inline StftLane stft_begin(const StftFront& f, char* smem, char** tail) {
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const StftTile tl = f.tiles[blockIdx.x];
    const int NSP = stft_plane_halfs(f.n_fft, f.hop);
    _Float16* sh = reinterpret_cast<_Float16*>(smem);
    _Float16* sl = sh + NSP;
    *tail = reinterpret_cast<char*>(sl + NSP);
    const StftLane L{f.seqs[tl.seq], tl.seq, tl.t0, lane & 15, lane >> 4, w & 1, w >> 1, sh, sl};
    stft_stage_planes(sh, sl, f.wav, f.wav_is_i16, L.sq.wav_off, L.sq.len, (int64_t)L.t0 * f.hop - f.n_fft / 2, stft_run_samples(f.n_fft, f.hop));
    return L;
}

// The loop over the basis tiles: the wave's share of tile nt (stft_tile_gemm), hi and cross terms recombined, then cell(nt, bin, re, im) with
// re[a][r], im[a][r] of the lane's bin = 32 nt + 16 nb + fr at frame L.frame(a, r).  Every thread calls `cell` for every tile: it may hold barriers.
template <class Cell>
__device__ inline void stft_tile_loop(const StftFront& f, const StftLane& L, Cell cell) {
    const int KS = f.n_fft / 32;
    int aoff[2];
#pragma unroll
    for (int a = 0; a < 2; ++a) aoff[a] = (L.mh * 32 + a * 16 + L.fr) * f.hop + 8 * L.g;
    const half8* basis = reinterpret_cast<const half8*>(f.basis) + (threadIdx.x & 63);
    for (int nt = 0; nt < f.n_btiles; ++nt) {
        f4 acc[2][2], accl[2][2];
        stft_tile_gemm(L.sh, L.sl, basis + (size_t)(nt * 2 + L.nb) * KS * 256, KS, aoff, acc, accl);
        float re[2][4], im[2][4];
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                re[a][r] = acc[a][0][r] + accl[a][0][r] * (1.0f / 2048.0f);
                im[a][r] = acc[a][1][r] + accl[a][1][r] * (1.0f / 2048.0f);
            }
        cell(nt, nt * STFT_TB + L.nb * 16 + L.fr, re, im);
    }
}

// |re + i im| as every forward kernel has rounded it: im * im, then one fma.  Spelled as the fma, not left to contraction: with re * re + im * im the
// vectoriser packed the two squares of some cells of stft_mel_kernel and left them unfused, an ulp away from stft_gain_kernel's.
__device__ inline float stft_mag(float re, float im) { return sqrtf(fmaf(re, re, im * im)); }

// Launches a forward kernel over the front's tiles, 256 threads each, with the two planes and `tail_bytes` of its own as dynamic LDS: 0, or -1 for
// a shape the kernels do not build
template <class P>
inline int stft_launch(void (*kernel)(P), const P& p, size_t tail_bytes, hipStream_t s) {
    const StftFront& f = p.f;
    if (!stft_shape_ok(f.n_fft, f.hop, 1) || f.n_tiles <= 0 || f.n_btiles != stft_bin_tiles(f.n_fft)) return -1;
    const size_t lds = (size_t)stft_plane_halfs(f.n_fft, f.hop) * 2 * sizeof(_Float16) + tail_bytes;
    if (hipFuncSetAttribute((const void*)kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(kernel, dim3((unsigned)f.n_tiles), dim3(256), lds, s, p);
    return 0;
}


}  // namespace

}  // namespace ev
