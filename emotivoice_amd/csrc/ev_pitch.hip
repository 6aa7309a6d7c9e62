// Pitch extraction (ev_pitch): wav -> per-frame F0 by YIN (a cumulative-mean-normalised difference function), then the reference's continuous-pitch
// fill and standardisation (reference feats.Pitch: _convert_to_continuous_pitch and (f0 - mean) / std).  include/evhip.h states the seven steps.
// This is NOT the reference's estimator (pyworld's dio + stonemask): only the frame grid, the fill and the units are its.
//
// pitch_yin: a tile of PITCH_TF frames of one utterance is ONE run of (PITCH_TF - 1) hop + S samples (S = win + tau_max + 1), kept in LDS as fp32; samples
// outside the utterance are zero.  Lags are spread over lanes: lane l of a wave owns lag 64 g + l of one frame, reads a[j] as a broadcast and
// s[j + lag] as consecutive words, and sums its win difference squares alone, so the bits of (frame, lag) depend on the utterance only.
// pitch_fill: one wave per utterance, next / previous voiced frame by a backward min-scan and a forward max-scan over 64-frame chunks.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

namespace ev {

namespace {

inline size_t pt_lags_padded(int tau_max) { return (size_t)((tau_max + 2 + 1) & ~1); }

}  // namespace

int pitch_run_samples(int hop, int win, int tau_max) { return (PITCH_TF - 1) * hop + win + tau_max + 1; }
size_t pitch_lds_bytes(int hop, int win, int tau_max) {
    return PITCH_TF * pt_lags_padded(tau_max) * (sizeof(double) + sizeof(float)) + PITCH_TF * sizeof(float) + (size_t)pitch_run_samples(hop, win, tau_max) * sizeof(float);
}
int pitch_shape_ok(int hop, int win, int tau_min, int tau_max) {
    return win >= 8 && win <= PITCH_MAX_WIN && hop >= 1 && hop <= win && tau_min >= 4 && tau_min < tau_max && tau_max + 1 <= win &&
           pitch_lds_bytes(hop, win, tau_max) <= (size_t)PITCH_MAX_LDS;
}

// One block = PITCH_TF frames of one utterance, 4 waves.  Work item (frame, 64-lag group) -> one wave; lane = lag.  The difference sum of a lag runs
// over j in four interleaved partial sums (j mod 4), ascending, combined as (s0 + s1) + (s2 + s3): an order fixed by (win, lag).  Then, per frame:
// the running fp64 sum of d (one lane, sequential), d' for every lag (all threads), and the dip search and parabolic refinement (one lane).
__global__ __launch_bounds__(256) void pitch_yin_kernel(const PitchParams p) {
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int tid = threadIdx.x, lane = tid & 63, w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const StftTile tl = p.tiles[blockIdx.x];
    const StftSeq sq = p.seqs[tl.seq];
    const int t0 = tl.t0, T = sq.frames, hop = p.hop, W = p.win;
    const int NL = p.tau_max + 2, NLP = (NL + 1) & ~1, S = W + p.tau_max + 1, NS = (PITCH_TF - 1) * hop + S;
    double* cs = reinterpret_cast<double*>(smem);
    float* dsh = reinterpret_cast<float*>(cs + PITCH_TF * NLP);
    float* e0 = dsh + PITCH_TF * NLP;
    float* run = e0 + PITCH_TF;
    stage_run<256>([&](int i) -> float& { return run[i]; }, p.wav, p.wav_is_i16, sq.wav_off, sq.len, (int64_t)t0 * hop - S / 2, NS);
    __syncthreads();
    const int NG = (NL + 63) >> 6;
    for (int it = w; it < PITCH_TF * NG; it += 4) {
        const int f = it / NG, g = it - f * NG;
        if (t0 + f >= T) break;
        const int tau = g * 64 + lane;
        const bool ok = tau < NL;
        const float* a = run + f * hop;
        const float* s = a + (ok ? tau : 0);
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
        int j = 0;
        for (; j + 4 <= W; j += 4) {
            const float u0 = a[j] - s[j], u1 = a[j + 1] - s[j + 1], u2 = a[j + 2] - s[j + 2], u3 = a[j + 3] - s[j + 3];
            s0 = fmaf(u0, u0, s0); s1 = fmaf(u1, u1, s1); s2 = fmaf(u2, u2, s2); s3 = fmaf(u3, u3, s3);
        }
        if (j < W) { const float u = a[j] - s[j]; s0 = fmaf(u, u, s0); ++j; }
        if (j < W) { const float u = a[j] - s[j]; s1 = fmaf(u, u, s1); ++j; }
        if (j < W) { const float u = a[j] - s[j]; s2 = fmaf(u, u, s2); }
        if (ok) dsh[f * NLP + tau] = (s0 + s1) + (s2 + s3);
    }
    // E0 = sum a[j]^2: lane l adds j = l, l + 64, ..; the 64 partial sums meet in a butterfly
    for (int f = w; f < PITCH_TF && t0 + f < T; f += 4) {
        const float* a = run + f * hop;
        float acc = 0.f;
        for (int j = lane; j < W; j += 64) acc = fmaf(a[j], a[j], acc);
        acc = wave_sum_f32(acc);
        if (lane == 0) e0[f] = acc;
    }
    __syncthreads();
    if (tid < PITCH_TF && t0 + tid < T) {
        const float* d = dsh + tid * NLP;
        double* c = cs + tid * NLP;
        double run_sum = 0.0;
        c[0] = 0.0;
        for (int tau = 1; tau < NL; ++tau) { run_sum += (double)d[tau]; c[tau] = run_sum; }
    }
    __syncthreads();
    for (int i = tid; i < PITCH_TF * NL; i += 256) {
        const int f = i / NL, tau = i - f * NL;
        if (t0 + f >= T) break;
        const double c = cs[f * NLP + tau];
        float dp = 1.0f;
        if (tau > 0 && c > 0.0) dp = (float)((double)dsh[f * NLP + tau] * (double)tau / c);
        dsh[f * NLP + tau] = dp;
    }
    __syncthreads();
    if (tid < PITCH_TF && t0 + tid < T) {
        const float* dp = dsh + tid * NLP;
        float f0 = 0.f, ap = 1.0f;
        int tau = -1;
        if ((double)e0[tid] >= p.e0_floor) {
            for (int k = p.tau_min; k <= p.tau_max; ++k)
                if (dp[k] < p.threshold) { tau = k; break; }
            if (tau >= 0) {
                while (tau + 1 <= p.tau_max && dp[tau + 1] < dp[tau]) ++tau;
                const double y0 = dp[tau - 1], y1 = dp[tau], y2 = dp[tau + 1];
                const double den = y0 - 2.0 * y1 + y2;
                double off = den > 0.0 ? 0.5 * (y0 - y2) / den : 0.0;
                off = off < -0.5 ? -0.5 : (off > 0.5 ? 0.5 : off);
                f0 = (float)((double)p.sample_rate / ((double)tau + off));
                ap = (float)y1;
            }
        }
        const int64_t at = sq.frm_off + t0 + tid;
        p.f0[at] = f0;
        p.ap[at] = ap;
        if (p.tau) p.tau[at] = tau;
    }
}

// One wave per utterance.  Pass 1 (chunks of 64 frames, last to first): the next voiced frame >= t, kept in out[t] as an integer; pass 2 (first to
// last): the previous voiced frame <= t, then the edge hold or the fp64 interpolation, rounded once, and the standardisation.  Thread (chunk, lane)
// reads back only what it wrote itself.
__global__ __launch_bounds__(64) void pitch_fill_kernel(const float* __restrict__ f0, const StftSeq* __restrict__ seqs, float mean, float stdv,
                                                        float* __restrict__ out) {
    const StftSeq sq = seqs[blockIdx.x];
    const int T = sq.frames, lane = threadIdx.x, nch = (T + 63) >> 6;
    const float* f = f0 + sq.frm_off;
    int* oi = reinterpret_cast<int*>(out + sq.frm_off);      // every access to the output goes through this one type
    int carry = INT_MAX;
    for (int c = nch - 1; c >= 0; --c) {
        const int t = c * 64 + lane;
        int v = (t < T && f[t] > 0.f) ? t : INT_MAX;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_down(v, d, 64);
            if (lane + d < 64) v = min(v, u);
        }
        v = min(v, carry);
        carry = __shfl(v, 0, 64);
        if (t < T) oi[t] = v;
    }
    carry = -1;
    for (int c = 0; c < nch; ++c) {
        const int t = c * 64 + lane;
        int v = (t < T && f[t] > 0.f) ? t : -1;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int u = __shfl_up(v, d, 64);
            if (lane >= d) v = max(v, u);
        }
        v = max(v, carry);
        carry = __shfl(v, 63, 64);
        if (t < T) {
            const int nx = oi[t];
            float cont;
            if (v < 0 && nx == INT_MAX) cont = 0.f;
            else if (v < 0) cont = f[nx];
            else if (nx == INT_MAX) cont = f[v];
            else if (v == nx) cont = f[t];
            else {
                const double fa = f[v], fb = f[nx];
                cont = (float)(fa + ((fb - fa) / (double)(nx - v)) * (double)(t - v));
            }
            oi[t] = __float_as_int((cont - mean) / stdv);
        }
    }
}

int launch_pitch_yin(const PitchParams& p, hipStream_t s) {
    if (!pitch_shape_ok(p.hop, p.win, p.tau_min, p.tau_max) || p.n_tiles <= 0) return -1;
    const size_t lds = pitch_lds_bytes(p.hop, p.win, p.tau_max);
    if (hipFuncSetAttribute((const void*)pitch_yin_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return -1;
    hipLaunchKernelGGL(pitch_yin_kernel, dim3((unsigned)p.n_tiles), dim3(256), lds, s, p);
    return 0;
}

void launch_pitch_fill(const float* f0, const StftSeq* seqs, int B, float mean, float stdv, float* out, hipStream_t s) {
    hipLaunchKernelGGL(pitch_fill_kernel, dim3((unsigned)B), dim3(64), 0, s, f0, seqs, mean, stdv, out);
}

}  // namespace ev
