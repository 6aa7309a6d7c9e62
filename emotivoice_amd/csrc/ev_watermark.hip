// Audio watermark (ev_watermark, ev_watermark_detect): a keyed pattern of small gains on the STFT magnitude, and the detector that finds it again.
// include/evhip.h states the scheme.
//
// wm_embed_kernel is stft_gain_kernel (ev_denoise.hip) with another gain: the same begin and tile loop (ev_audio_dev.h), the same cell
// store into the same scratch planes, from which launch_istft_ola rebuilds the waveform unchanged.  The gain of cell (t, k) in band v is a or
// float32(1 / a) by the sign of chip 48 ((t / 8) mod 16) + v, read from the segment's 768 signs in LDS; 1 outside the bands.
//
// wm_bands_kernel is the forward GEMM once more with a band epilogue.  Bin fr of a wave's 16 lives in lane fr, so the four mag^2 of a band are four
// neighbouring lanes: E = (m0 + m1) + (m2 + m3) by two xor shuffles.  The floor needs the frame's largest mag^2 over ALL bins: it is a max carried
// through the bin-tile loop in registers while the unfloored band energies wait in LDS (64 frames x 48 bands), reduced over the 16 lanes of a
// frame by shuffles and over the two waves that share the frame through LDS; only then are the bands floored, quantised and written, 48 int32
// per frame.
//
// wm_correlate_kernel: one block of 8 waves per segment.  The sums of q over every window of 8 frames go to a scratch first (each an independent
// sum of 8 loads: the same integers as differences of a prefix sum, without its serial chain).  The tiles of offset s start at frames = s mod 8,
// so wave p owns phase p: a lane forms sign(X) of a (tile, band) once and adds it into the 16 offsets 8 k + p, whose chips differ only by the
// tile shift k.  One wave then takes the argmax of C / sqrt(n) over the 128 offsets by exact int64 cross-multiplication, and the block sums the
// payload bits' chips at that offset.  Integer sums throughout: exact in any order.  No atomics, vector stores only.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

void watermark_pattern(uint32_t key, int nbits, uint32_t payload, int8_t* signs, uint8_t* roles) {
    for (int i = 0; i < WM_CHIPS; ++i) {
        const uint32_t h = dl_mix(key, (uint64_t)i);
        int c = (h & 1u) ? 1 : -1, role = WM_PILOT;
        if (nbits > 0) {
            const int r = (int)((h >> 1) % (uint32_t)(2 * nbits));
            if (r < nbits) {
                role = r;
                if ((payload >> r) & 1u) c = -c;
            }
        }
        signs[i] = (int8_t)c;
        if (roles) roles[i] = (uint8_t)role;
    }
}

namespace {

constexpr int WM_BINS = WM_NFFT / 2 + 1, WM_KPAD = denoise_k_pad(WM_NFFT);
constexpr int WM_WAVES = WM_TILE;      // wm_correlate_kernel: one wave per phase of the tile grid
static_assert(WM_BAND0 % WM_BAND_BINS == 0, "a band is four neighbouring lanes that start at a multiple of four");

// the checks the two forward launchers share: the one shape the kernels' constants describe
bool wm_front_ok(const StftFront& f) { return f.n_fft == WM_NFFT && f.hop == WM_HOP; }

}  // namespace

// One block = 64 frames of one segment, 4 waves, laid out as stft_gain_kernel: lane (fr, g) of wave (nb, mh) holds re and im of bin
// 32 nt + 16 nb + fr of frames t0 + 32 mh + 16 a + 4 g + r.  t0 is a multiple of 64, so the tile of those four frames is one value per (a, g).
__global__ __launch_bounds__(256) void wm_embed_kernel(const WmEmbedParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* tail;
    const StftLane L = stft_begin(p.f, smem, &tail);
    int8_t* sg = reinterpret_cast<int8_t*>(tail);
    for (int i = threadIdx.x; i < WM_CHIPS; i += 256) sg[i] = p.signs[(size_t)L.seq * WM_CHIPS + i];
    __syncthreads();
    const int T = L.sq.frames;
    const float ga = p.gains[2 * L.seq], gi = p.gains[2 * L.seq + 1];
    stft_tile_loop(p.f, L, [&](int, int bin, const float (&re)[2][4], const float (&im)[2][4]) {
        const bool banded = bin >= WM_BAND0 && bin < WM_BAND0 + WM_BAND_BINS * WM_BANDS;
        const int v = banded ? (bin - WM_BAND0) / WM_BAND_BINS : 0;
#pragma unroll
        for (int a = 0; a < 2; ++a) {
            const int u = ((L.t0 + L.frame(a, 0)) / WM_TILE) & (WM_PERIOD - 1);
            const float gw = banded ? (sg[WM_BANDS * u + v] > 0 ? ga : gi) : 1.0f;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float m = stft_mag(re[a][r], im[a][r]);
                const int t = L.t0 + L.frame(a, r);
                if (t >= T || 2 * bin >= WM_KPAD) continue;
                const bool live = m > 0.f;      // mag == 0 (and a NaN): the cell is zero, selected as ev_denoise selects it (0 * NaN is NaN)
                stft_store_cell(p.spec_hi, p.spec_lo, (size_t)(L.sq.frm_off + t) * WM_KPAD + 2 * bin, live ? gw * re[a][r] : 0.f, live ? gw * im[a][r] : 0.f);
            }
        }
    });
}

int launch_wm_embed(const WmEmbedParams& p, hipStream_t s) {
    if (!wm_front_ok(p.f) || !p.signs || !p.gains || !p.spec_hi || !p.spec_lo) return -1;
    return stft_launch(wm_embed_kernel, p, WM_CHIPS, s);      // the tail: the segment's signs
}

__global__ __launch_bounds__(256) void wm_bands_kernel(const WmBandParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    char* tail;
    const StftLane L = stft_begin(p.f, smem, &tail);
    float* eb = reinterpret_cast<float*>(tail);      // [frame of the tile][band]: the unfloored band energies
    float* fm = eb + STFT_TF * WM_BANDS;             // [nb][frame of the tile]: the largest mag^2 of each half of the bins
    __syncthreads();
    const int T = L.sq.frames;
    float mx[2][4];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) mx[a][r] = 0.f;
    stft_tile_loop(p.f, L, [&](int, int bin, const float (&re)[2][4], const float (&im)[2][4]) {
        const bool owner = (L.fr & (WM_BAND_BINS - 1)) == 0 && bin >= WM_BAND0 && bin < WM_BAND0 + WM_BAND_BINS * WM_BANDS;
        const int v = (bin - WM_BAND0) / WM_BAND_BINS;
#pragma unroll
        for (int a = 0; a < 2; ++a)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const float m2 = bin < WM_BINS ? add_rn(mul_rn(re[a][r], re[a][r]), mul_rn(im[a][r], im[a][r])) : 0.f;
                mx[a][r] = fmaxf(mx[a][r], m2);
                float e = add_rn(m2, __shfl_xor(m2, 1, 64));      // (m0 + m1) and (m2 + m3) ...
                e = add_rn(e, __shfl_xor(e, 2, 64));               // ... and their sum: the same value in all four lanes of the band
                if (owner) eb[L.frame(a, r) * WM_BANDS + v] = e;
            }
    });
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            float m = mx[a][r];
#pragma unroll
            for (int o = 1; o <= 8; o <<= 1) m = fmaxf(m, __shfl_xor(m, o, 64));      // over the 16 lanes (bins) of the frame
            if (L.fr == 0) fm[L.nb * STFT_TF + L.frame(a, r)] = m;
        }
    __syncthreads();
    for (int i = threadIdx.x; i < STFT_TF * WM_BANDS; i += 256) {
        const int f = i / WM_BANDS, t = L.t0 + f;
        if (t >= T) continue;
        const float peak = fmaxf(fm[f], fm[STFT_TF + f]);
        const float e = fmaxf(eb[i], mul_rn(peak, 0x1p-24f));
        p.q[(size_t)(L.sq.frm_off + t) * WM_BANDS + (i - f * WM_BANDS)] = (int32_t)(__float_as_uint(e) >> 17);
    }
}

int launch_wm_bands(const WmBandParams& p, hipStream_t s) {
    if (!wm_front_ok(p.f) || !p.q) return -1;
    return stft_launch(wm_bands_kernel, p, (size_t)(STFT_TF * WM_BANDS + 2 * STFT_TF) * sizeof(float), s);      // the tail: eb and fm
}

namespace {

// is offset a (C, n, s) a better answer than offset b?  C / sqrt(n) over C > 0, compared exactly; a tie, and any two offsets without a positive C,
// go to the smaller offset.  C^2 n < 2^63: n <= 48 tiles <= 48 * EV_ALIGN_MAX_FRAMES / 8 < 2^17 and |C| <= n.
__device__ inline bool wm_better(int Ca, int na, int sa, int Cb, int nb, int sb) {
    if ((Ca > 0) != (Cb > 0)) return Ca > 0;
    if (Ca > 0) {
        const int64_t l = (int64_t)Ca * Ca * nb, r = (int64_t)Cb * Cb * na;
        if (l != r) return l > r;
    }
    return sa < sb;
}

// sign(X) of tile j (whose first frame is f) and band v from the window sums
__device__ inline int wm_sign_x(const int32_t* win, int f, int v) {
    const int X = 2 * win[(size_t)f * WM_BANDS + v] - win[(size_t)(f - WM_TILE) * WM_BANDS + v] - win[(size_t)(f + WM_TILE) * WM_BANDS + v];
    return (X > 0) - (X < 0);
}

}  // namespace

__global__ __launch_bounds__(64 * WM_WAVES) void wm_correlate_kernel(const int32_t* q, int32_t* win, const StftSeq* seqs, const int8_t* tabs, WmFig* figs) {
    __shared__ int8_t pil[WM_CHIPS], chip[WM_CHIPS];
    __shared__ uint8_t role[WM_CHIPS];
    __shared__ int sC[WM_OFFSETS], sN[WM_OFFSETS], sB[WM_WAVES][2 * WM_MAX_BITS], best[3];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const StftSeq sq = seqs[blockIdx.x];
    const int T = sq.frames;
    const int32_t* qs = q + (size_t)sq.frm_off * WM_BANDS;
    int32_t* ws = win + (size_t)sq.frm_off * WM_BANDS;
    for (int i = tid; i < WM_CHIPS; i += 512) {
        pil[i] = tabs[i]; chip[i] = tabs[WM_CHIPS + i]; role[i] = (uint8_t)tabs[2 * WM_CHIPS + i];
    }
    // ws[f][v] = q[f][v] + .. + q[f + 7][v] for every f with f + 8 <= T
    const int n_win = max(T - (WM_TILE - 1), 0) * WM_BANDS;
    for (int i = tid; i < n_win; i += 512) {
        int s = 0;
#pragma unroll
        for (int k = 0; k < WM_TILE; ++k) s += qs[i + k * WM_BANDS];
        ws[i] = s;
    }
    __syncthreads();
    {      // wave p: the tiles that start at frames p + 8 j; whole tiles j < nts, interior ones 1 .. nts - 2
        const int p = w, nts = T >= p ? (T - p) / WM_TILE : 0, items = max(nts - 2, 0) * WM_BANDS;
        int C[WM_PERIOD], N[WM_PERIOD];
#pragma unroll
        for (int k = 0; k < WM_PERIOD; ++k) { C[k] = 0; N[k] = 0; }
        for (int idx = lane; idx < items; idx += 64) {
            const int j = 1 + idx / WM_BANDS, v = idx % WM_BANDS;
            const int sg = wm_sign_x(ws, p + WM_TILE * j, v);
#pragma unroll
            for (int k = 0; k < WM_PERIOD; ++k) {      // offset s = 8 k + p: tile j carries the chips of u = (j - k) mod 16
                const int c = pil[WM_BANDS * ((j - k) & (WM_PERIOD - 1)) + v] * sg;
                C[k] += c;
                N[k] += c != 0;
            }
        }
#pragma unroll
        for (int k = 0; k < WM_PERIOD; ++k) {
            const int c = wave_sum_i32(C[k]), n = wave_sum_i32(N[k]);
            if (lane == 0) { sC[WM_TILE * k + p] = c; sN[WM_TILE * k + p] = n; }
        }
    }
    __syncthreads();
    if (w == 0) {
        int s = lane, c = sC[lane], n = sN[lane];
        if (wm_better(sC[lane + 64], sN[lane + 64], lane + 64, c, n, s)) { s = lane + 64; c = sC[s]; n = sN[s]; }
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const int s2 = __shfl_xor(s, o, 64), c2 = __shfl_xor(c, o, 64), n2 = __shfl_xor(n, o, 64);
            if (wm_better(c2, n2, s2, c, n, s)) { s = s2; c = c2; n = n2; }
        }
        if (lane == 0) { best[0] = s; best[1] = c; best[2] = n; }
    }
    __syncthreads();
    {      // the payload bits at the reported offset: every chip of role b, with the sign it has at payload 0
        const int s = best[0], p = s & (WM_TILE - 1), k = s >> 3, nts = T >= p ? (T - p) / WM_TILE : 0, items = max(nts - 2, 0) * WM_BANDS;
        int bc[WM_MAX_BITS], bn[WM_MAX_BITS];
#pragma unroll
        for (int b = 0; b < WM_MAX_BITS; ++b) { bc[b] = 0; bn[b] = 0; }
        for (int idx = tid; idx < items; idx += 512) {
            const int j = 1 + idx / WM_BANDS, v = idx % WM_BANDS;
            const int sg = wm_sign_x(ws, p + WM_TILE * j, v);
            const int i = WM_BANDS * ((j - k) & (WM_PERIOD - 1)) + v, r = role[i], c = chip[i] * sg;
#pragma unroll
            for (int b = 0; b < WM_MAX_BITS; ++b) {
                bc[b] += r == b ? c : 0;
                bn[b] += (r == b && c != 0) ? 1 : 0;
            }
        }
#pragma unroll
        for (int b = 0; b < WM_MAX_BITS; ++b) {
            const int c = wave_sum_i32(bc[b]), n = wave_sum_i32(bn[b]);
            if (lane == 0) { sB[w][b] = c; sB[w][WM_MAX_BITS + b] = n; }
        }
    }
    __syncthreads();
    WmFig* out = figs + blockIdx.x;
    if (tid < 2 * WM_MAX_BITS) {
        int v = 0;
#pragma unroll
        for (int i = 0; i < WM_WAVES; ++i) v += sB[i][tid];
        if (tid < WM_MAX_BITS) out->bit_C[tid] = v; else out->bit_n[tid - WM_MAX_BITS] = v;
    }
    if (tid == 0) { out->offset = best[0]; out->C = best[1]; out->n = best[2]; out->pad = 0; }
}

int launch_wm_correlate(const int32_t* q, int32_t* win, const StftSeq* seqs, int B, const int8_t* tabs, WmFig* figs, hipStream_t s) {
    if (B <= 0 || !q || !win || !seqs || !tabs || !figs) return -1;
    hipLaunchKernelGGL(wm_correlate_kernel, dim3((unsigned)B), dim3(512), 0, s, q, win, seqs, tabs, figs);
    return 0;
}

}  // namespace ev
