// Acoustic features (ev_features): wav -> log-mel spectrogram and frame energy, the reference's TacotronSTFT.mel_spectrogram
// (reference models/prompt_tts_modified/tacotron_stft.py:71-80, stft.py:48-76) and the energy of the same magnitudes.
//
// The windowed DFT is a GEMM with overlapping rows: M = frames, K = n_fft, N = 2 x (n_fft / 2 + 1).  Row t of the A operand is
// padded[hop t .. hop t + n_fft), so a tile of 64 frames is ONE run of 63 hop + n_fft samples, kept in LDS for the block's life as fp16
// hi / lo planes (x = hi + 2^-11 lo, the split of conv_gemm_split_kernel); reflect padding and the int16 conversion happen on load.
// The basis is packed on the host (stft_pack_basis) in MFMA operand order: a wave's B fragment is one coalesced 16-byte load per lane.
// The staging of the run and a wave's share of one basis tile (stft_stage_planes, stft_tile_gemm) are in ev_audio_dev.h: ev_denoise's forward
// kernel runs the same code.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include <vector>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

namespace {

constexpr int FT_TF = STFT_TF, FT_TB = STFT_TB;      // frames per block, bins per basis tile (ev_kernels.h)
constexpr int FT_MAGP = FT_TF + 1;                   // pitch of the [bin][frame] magnitude tile

}  // namespace

int stft_shape_ok(int n_fft, int hop, int n_mels) {
    return n_fft >= 128 && n_fft % 128 == 0 && n_fft <= STFT_MAX_NFFT && hop >= 8 && hop % 8 == 0 && hop <= n_fft && n_mels >= 1 &&
           n_mels <= STFT_MAX_MELS && stft_run_samples(n_fft, hop) <= STFT_MAX_RUN;
}
size_t stft_basis_halfs(int n_fft) { return (size_t)stft_bin_tiles(n_fft) * 2 * (n_fft / 32) * 4 * 64 * 8; }
size_t stft_melT_floats(int n_fft) { return (size_t)stft_bin_tiles(n_fft) * FT_TB * STFT_MAX_MELS; }

// Basis planes.  Entry (bin, k) is float32(cos / -sin(2 pi bin k / n_fft)) * window[k] in float32 (the reference multiplies its float32 Fourier
// basis by its float32 window), the angle reduced exactly in integers.  window == null: periodic hann in float64, rounded to float32.
// Order: [bin tile][16-bin half][k step of 32][re hi, re lo, im hi, im lo][lane][8]: lane l holds k = 32 step + 8 (l >> 4) + j of bin (l & 15).
std::vector<double> host_window(int n_fft, const float* window) {
    std::vector<double> win((size_t)n_fft);
    for (int n = 0; n < n_fft; ++n) win[n] = window ? (double)window[n] : 0.5 - 0.5 * cos(2.0 * M_PI * (double)n / (double)n_fft);
    return win;
}
void stft_pack_basis(int n_fft, const float* window, uint16_t* out) {
    const int n_bins = n_fft / 2 + 1, nbt = stft_bin_tiles(n_fft), KS = n_fft / 32;
    const std::vector<double> win = host_window(n_fft, window);
    _Float16* o = reinterpret_cast<_Float16*>(out);
    for (int nt = 0; nt < nbt; ++nt)
        for (int nb = 0; nb < 2; ++nb)
            for (int ks = 0; ks < KS; ++ks)
                for (int part = 0; part < 2; ++part)
                    for (int lane = 0; lane < 64; ++lane)
                        for (int j = 0; j < 8; ++j) {
                            const int bin = nt * FT_TB + nb * 16 + (lane & 15), k = ks * 32 + 8 * (lane >> 4) + j;
                            float v = 0.f;
                            if (bin < n_bins) {
                                const double ang = 2.0 * M_PI * (double)(((int64_t)bin * k) % n_fft) / (double)n_fft;
                                v = (float)(part ? -sin(ang) : cos(ang)) * (float)win[k];
                            }
                            const _Float16 hi = (_Float16)v;
                            const size_t at = ((((size_t)(nt * 2 + nb) * KS + ks) * 4 + part * 2) * 64 + lane) * 8 + j;
                            o[at] = hi;
                            o[at + 64 * 8] = (_Float16)((v - (float)hi) * 2048.0f);
                        }
}

// mel_basis (n_mels, n_bins) -> [bin][4 groups][32]: group g holds mels g nmi .. g nmi + nmi - 1 (nmi = ceil(n_mels / 4)), zero elsewhere
void stft_pack_mel(int n_fft, int n_mels, const float* mel_basis, float* out) {
    const int n_bins = n_fft / 2 + 1, nmi = stft_mels_per_group(n_mels);
    const size_t n = stft_melT_floats(n_fft);
    for (size_t i = 0; i < n; ++i) out[i] = 0.f;
    for (int m = 0; m < n_mels; ++m)
        for (int k = 0; k < n_bins; ++k) out[(size_t)k * STFT_MAX_MELS + (m / nmi) * 32 + m % nmi] = mel_basis[(size_t)m * n_bins + k];
}

// One block = 64 frames of one utterance, 4 waves, laid out as StftLane says (ev_audio_dev.h).  re and im of a bin land in the same lane and
// register, so the magnitude is formed in registers.  It goes to an LDS tile [bin][frame]; then thread (frame = lane, group = wave) adds the
// tile's 32 bins into its mel rows in fp32, bins in ascending order, and wave 0 adds mag^2 into the frame's energy in fp64.  No atomics, no split
// over bins: the bits of a frame depend on its utterance alone.
template <int NMI>
__global__ __launch_bounds__(256) void stft_mel_kernel(const StftParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int lane = threadIdx.x & 63, w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    char* tail;
    const StftLane L = stft_begin(p.f, smem, &tail);
    float* magT = reinterpret_cast<float*>(tail);
    __syncthreads();
    const int T = L.sq.frames, n_bins = p.f.n_fft / 2 + 1, nmi = stft_mels_per_group(p.n_mels);
    float macc[NMI];
#pragma unroll
    for (int i = 0; i < NMI; ++i) macc[i] = 0.f;
    double e64 = 0.0;
    stft_tile_loop(p.f, L, [&](int nt, int bin, const float (&re)[2][4], const float (&im)[2][4]) {
        __syncthreads();          // the previous tile's magnitudes have been read
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float m = stft_mag(re[a][r], im[a][r]);
                const int f = L.frame(a, r);
                magT[(L.nb * 16 + L.fr) * FT_MAGP + f] = m;
                if (p.mag && L.t0 + f < T && bin < n_bins) p.mag[(L.sq.frm_off + L.t0 + f) * n_bins + bin] = m;
            }
        __syncthreads();
        const float* wrow = p.melT + (size_t)nt * FT_TB * STFT_MAX_MELS + w * 32;
        // by 2 at 20 mels, rolled at 32, as the compiler chose while the loop stood in the kernel's own body; inside the callable it would unroll the
        // loop whole (macc is still in memory when it decides): 224 VGPRs, a wave less
#pragma unroll NMI <= 20 ? 2 : 1
        for (int j = 0; j < FT_TB; ++j) {
            const float mv = magT[j * FT_MAGP + lane];
#pragma unroll
            for (int i = 0; i < NMI; ++i) macc[i] = fmaf(wrow[j * STFT_MAX_MELS + i], mv, macc[i]);
            if (w == 0) e64 += (double)mv * (double)mv;
        }
    });
    const int t = L.t0 + lane;
    if (t >= T) return;
    float* mo = p.mel + L.sq.frm_off * p.n_mels + t;
#pragma unroll
    for (int i = 0; i < NMI; ++i) {
        const int m = w * nmi + i;
        if (i < nmi && m < p.n_mels) mo[(int64_t)m * T] = (float)log((double)fmaxf(macc[i], p.mel_clip));
    }
    if (w == 0) {
        const float e = (float)sqrt(fmax(e64, (double)p.energy_floor));
        p.energy[L.sq.frm_off + t] = (e - p.energy_mean) / p.energy_std;
    }
}

int launch_stft_mel(const StftParams& p, hipStream_t s) {
    if (!stft_shape_ok(p.f.n_fft, p.f.hop, p.n_mels)) return -1;
    const size_t tail = (size_t)FT_TB * FT_MAGP * sizeof(float);      // the magnitude tile
    return stft_mels_per_group(p.n_mels) <= 20 ? stft_launch(stft_mel_kernel<20>, p, tail, s) : stft_launch(stft_mel_kernel<32>, p, tail, s);
}

}  // namespace ev
