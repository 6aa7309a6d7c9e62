// Vocoder bias removal (ev_denoise): the Tacotron 2 / WaveGlow `Denoiser` on the reference's STFT class (reference
// models/prompt_tts_modified/stft.py: transform, inverse; audio_processing.py: window_sumsquare) -- STFT, a gain per cell, inverse STFT.
//
// stft_gain_kernel is the forward GEMM of ev_features (the shared parts of ev_audio_dev.h, the basis of stft_pack_basis) with another epilogue:
// re and im of a bin land in the same lane, so the magnitude and the gain g = max(mag - s bias, 0) / mag are formed in registers and g re, g im
// go to a scratch in device memory as fp16 hi / lo planes, [frame][k_pad], re and im of a bin side by side.
//
// istft_ola_kernel is a GEMM over overlapping rows again.  Chunk j -- the hop samples hop j .. hop j + hop of the untrimmed signal -- is the
// sum over the R = n_fft / hop frames j - R + 1 .. j that reach it, and those frames are R consecutive rows of the scratch: ONE contiguous run
// of R k_pad values, which is row j of the A operand; row j + 1 starts k_pad further.  The B operand [R k_pad][hop] holds every frame's part of
// the windowed inverse DFT basis (istft_pack_basis).  The overlap-add is the GEMM's own accumulation: no atomics, nothing carried between
// blocks, one fixed order, so the bits of an utterance depend on that utterance alone.  Frames before 0 and after T - 1 are zero fragments by
// bounds; nothing outside the utterance's rows is read.
#include <hip/hip_runtime.h>
#include <float.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

int denoise_shape_ok(int n_fft, int hop) {
    return stft_shape_ok(n_fft, hop, 1) && n_fft % hop == 0 && n_fft / hop <= DN_MAX_R;
}
static int istft_col_tiles(int hop) { return (hop + 15) / 16; }
size_t istft_basis_halfs(int n_fft, int hop) { return (size_t)istft_col_tiles(hop) * ((size_t)(n_fft / hop) * denoise_k_pad(n_fft) / 32) * 2 * 64 * 8; }
size_t istft_envelope_floats(int n_fft, int hop) { const size_t R = n_fft / hop; return R * R * hop; }

void istft_pack_basis(int n_fft, int hop, const float* window, uint16_t* out) {
    const int n_bins = n_fft / 2 + 1, R = n_fft / hop, KP = denoise_k_pad(n_fft), KS = R * KP / 32, NT = istft_col_tiles(hop);
    const std::vector<double> win = host_window(n_fft, window);
    _Float16* o = reinterpret_cast<_Float16*>(out);
    for (int nt = 0; nt < NT; ++nt)
        for (int ks = 0; ks < KS; ++ks)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int row = ks * 32 + 8 * (lane >> 4) + j, n = nt * 16 + (lane & 15);
                    const int q = row / KP, c = row % KP, bin = c >> 1, part = c & 1;
                    float v = 0.f;
                    if (bin < n_bins && n < hop) {
                        const int m = (R - 1 - q) * hop + n;
                        const double ang = 2.0 * M_PI * (double)(((int64_t)bin * m) % n_fft) / (double)n_fft;
                        const double ck = (bin == 0 || bin == n_fft / 2) ? 1.0 : 2.0;
                        v = (float)(part ? -ck * sin(ang) : ck * cos(ang)) * (float)win[m];
                    }
                    const _Float16 hi = (_Float16)v;
                    const size_t at = ((((size_t)nt * KS + ks) * 2) * 64 + lane) * 8 + j;
                    o[at] = hi;
                    o[at + 64 * 8] = (_Float16)((v - (float)hi) * 2048.0f);
                }
}

void istft_pack_envelope(int n_fft, int hop, const float* window, float* out) {
    const int R = n_fft / hop;
    std::vector<double> w2 = host_window(n_fft, window);      // the squares in float64: of the float64 hann for window == null, as the reference squares scipy's
    for (double& w : w2) w = w * w;
    for (int qa = 0; qa < R; ++qa)
        for (int qb = 0; qb < R; ++qb)
            for (int n = 0; n < hop; ++n) {
                float x = 0.f;
                for (int q = qa; q <= qb; ++q) x = (float)((double)x + w2[(R - 1 - q) * hop + n]);      // ascending frames, as window_sumsquare adds them: float32 += float64
                out[((size_t)qa * R + qb) * hop + n] = x;
            }
}

// The forward GEMM of ev_features (stft_begin, stft_tile_loop) with the gain epilogue: one block = 64 frames of one utterance, and lane (fr, g)
// holds re and im of bin fr of the frames 4 g + r (StftLane).
__global__ __launch_bounds__(256) void stft_gain_kernel(const StftGainParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* tail;
    const StftLane L = stft_begin(p.f, smem, &tail);
    __syncthreads();
    const int T = p.mag ? min(L.sq.frames, p.mag_frames) : L.sq.frames, n_bins = p.f.n_fft / 2 + 1, k_pad = denoise_k_pad(p.f.n_fft);
    const float s = p.mag ? 0.f : p.strengths[L.seq];
    stft_tile_loop(p.f, L, [&](int, int bin, const float (&re)[2][4], const float (&im)[2][4]) {
        const float sb = (!p.mag && bin < n_bins) ? s * p.bias[bin] : 0.f;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float m = stft_mag(re[a][r], im[a][r]);
                const int t = L.t0 + L.frame(a, r);
                if (t >= T) continue;
                const int64_t row = L.sq.frm_off + t;
                if (p.mag) {
                    if (bin < n_bins) p.mag[row * n_bins + bin] = m;
                    continue;
                }
                if (2 * bin >= k_pad) continue;
                const bool live = m > 0.f;      // mag == 0 (and a NaN): the cell is zero -- selected, since 0 * NaN is NaN
                const float gn = live ? fmaxf(m - sb, 0.f) / m : 0.f;
                const float vr = live ? gn * re[a][r] : 0.f, vi = live ? gn * im[a][r] : 0.f;
                stft_store_cell(p.spec_hi, p.spec_lo, (size_t)row * k_pad + 2 * bin, vr, vi);
            }
    });
}

int launch_stft_gain(const StftGainParams& p, hipStream_t s) {
    if (!denoise_shape_ok(p.f.n_fft, p.f.hop)) return -1;
    if (p.mag ? p.mag_frames < 1 : (!p.spec_hi || !p.spec_lo || !p.bias || !p.strengths)) return -1;
    return stft_launch(stft_gain_kernel, p, 0, s);
}

// One block = DN_TJ chunks of one utterance times DN_TN output columns, 4 waves: wave w multiplies chunks 32 (w >> 1) .. + 31 (two 16-row tiles)
// into columns 64 (w & 1) .. + 63 (four 16-column tiles).  Per 32-row step of the basis: 2 A fragments (hi, lo) straight from the scratch --
// lane (fr, g) reads the 8 values at 32 step + 8 g of the run of chunk fr, 16 bytes, a zero fragment where the step's frame is outside
// [0, T) -- 4 B fragments (hi, lo) from the packed basis, one coalesced 16-byte load per lane each, both prefetched one step ahead, and 24 MFMAs.
__global__ __launch_bounds__(256) void istft_ola_kernel(const IstftParams p) {
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const StftTile tl = p.tiles[blockIdx.x];
    const IstftSeq sq = p.seqs[tl.seq];
    const int T = sq.frames, hop = p.hop, R = p.R, KP = p.k_pad, KPS = KP / 32, KS = R * KPS;
    const int fr = lane & 15, g = lane >> 4, nh = w & 1, mh = w >> 1;
    const int NT = (hop + 15) / 16;
    const half8 zero = half8{0, 0, 0, 0, 0, 0, 0, 0};
    int jrow[2];                 // the first frame (q = 0) of the lane's chunk in each row tile
    int64_t aat[2];              // where the lane's run starts in the planes; before the utterance's rows for frames < 0, which are never read
#pragma unroll
    for (int a = 0; a < 2; ++a) {
        jrow[a] = tl.t0 + mh * 32 + a * 16 + fr - (R - 1);
        aat[a] = (sq.frm_off + jrow[a]) * (int64_t)KP + 8 * g;
    }
    const int64_t safe = sq.frm_off * (int64_t)KP + 8 * g;      // frame 0 of the utterance: what a lane reads (and drops) for a frame outside [0, T)
    const _Float16* ph = reinterpret_cast<const _Float16*>(p.spec_hi);
    const _Float16* pl = reinterpret_cast<const _Float16*>(p.spec_lo);
    const half8* bp[4];
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int nt = min((int)blockIdx.y * (DN_TN / 16) + nh * 4 + c, NT - 1);      // a tile past the last one: its columns are never stored
        bp[c] = reinterpret_cast<const half8*>(p.ibasis) + (size_t)nt * KS * 128 + lane;
    }
    f4 acc[2][4], accl[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c) { acc[a][c] = f4{0.f, 0.f, 0.f, 0.f}; accl[a][c] = f4{0.f, 0.f, 0.f, 0.f}; }
    half8 ahn[2] = {zero, zero}, aln[2] = {zero, zero}, bhn[4] = {zero, zero, zero, zero}, bln[4] = {zero, zero, zero, zero};
    int q = 0, kk = 0;           // the step being loaded is q KPS + kk
    for (int ks = -1; ks < KS; ++ks) {
        half8 Ah[2], Al[2], Bh[4], Bl[4];
#pragma unroll
        for (int a = 0; a < 2; ++a) { Ah[a] = ahn[a]; Al[a] = aln[a]; }
#pragma unroll
        for (int c = 0; c < 4; ++c) { Bh[c] = bhn[c]; Bl[c] = bln[c]; }
        const int kn = min(ks + 1, KS - 1);      // the last pass loads its own step again and drops it
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int t = jrow[a] + q;
            const bool ok = t >= 0 && t < T && q < R;
            const int64_t at = ok ? aat[a] + kn * 32 : safe;
            const half8 vh = *reinterpret_cast<const half8*>(ph + at), vl = *reinterpret_cast<const half8*>(pl + at);
            ahn[a] = ok ? vh : zero;
            aln[a] = ok ? vl : zero;
        }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
            bhn[c] = bp[c][(size_t)kn * 128];
            bln[c] = bp[c][(size_t)kn * 128 + 64];
        }
        if (kn == ks + 1 && ++kk == KPS) { kk = 0; ++q; }
        if (ks < 0) continue;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int c = 0; c < 4; ++c) {
                acc[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[a], Bh[c], acc[a][c], 0, 0, 0);
                accl[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Ah[a], Bl[c], accl[a][c], 0, 0, 0);
                accl[a][c] = __builtin_amdgcn_mfma_f32_16x16x32_f16(Al[a], Bh[c], accl[a][c], 0, 0, 0);
            }
    }
    // epilogue: lane (fr, g) holds column fr of chunks 4 g + r of each tile
    const float inv_n = 1.0f / (float)p.n_fft;
    const int half_n = p.n_fft / 2;
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int c = 0; c < 4; ++c)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int j = tl.t0 + mh * 32 + a * 16 + g * 4 + r;
                const int n = ((int)blockIdx.y * (DN_TN / 16) + nh * 4 + c) * 16 + fr;
                const int64_t i = (int64_t)j * hop + n - half_n;
                if (n >= hop || i < 0 || i >= sq.out_len) continue;
                const int qa = max(0, R - 1 - j), qb = min(R - 1, T + R - 2 - j);
                const float e = p.env[((size_t)qa * R + qb) * hop + n];
                float y = mul_rn(acc[a][c][r] + accl[a][c][r] * (1.0f / 2048.0f), inv_n);
                if (e > FLT_MIN) y = y / e;
                p.out[sq.out_off + i] = y;
                if (p.out_i16) p.out_i16[sq.out_off + i] = y != y ? (int16_t)0 : s16_trunc(y);      // NaN -> 0
            }
}

int launch_istft_ola(const IstftParams& p, hipStream_t s) {
    if (!denoise_shape_ok(p.n_fft, p.hop) || p.n_tiles <= 0 || p.R != p.n_fft / p.hop || p.k_pad != denoise_k_pad(p.n_fft) || !p.out) return -1;
    hipLaunchKernelGGL(istft_ola_kernel, dim3((unsigned)p.n_tiles, (unsigned)((p.hop + DN_TN - 1) / DN_TN)), dim3(256), 0, s, p);
    return 0;
}

}  // namespace ev
