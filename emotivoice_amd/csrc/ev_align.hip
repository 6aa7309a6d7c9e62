// Forced alignment (ev_align): the score of the reference's AlignmentModule and its monotonic alignment search
// (reference models/prompt_tts_modified/modules/alignment.py:27-55, 93-122, 125-162).  The aligner's convs are
// split-precision conv-GEMMs launched by the engine; this file holds the two kernels that follow them.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "ev_kernels.h"

namespace ev {

namespace {

constexpr int SC_TF = 64;     // frames per score block
constexpr int SC_TN = 64;     // tokens per score tile
constexpr int SC_KC = 32;     // channels per LDS stage
constexpr int SC_PITCH = SC_KC + 1;

// log betabinom.pmf(k; n, a, b) in fp64, in the order of scipy.stats.betabinom._logpmf:
//   -log(n + 1) - betaln(n - k + 1, k + 1) + betaln(k + a, n - k + b) - betaln(a, b)
__device__ double betaln_d(double x, double y) { return lgamma(x) + lgamma(y) - lgamma(x + y); }
__device__ double log_betabinom(double k, double n, double a, double b) {
    const double combiln = -log(n + 1.0) - betaln_d(n - k + 1.0, k + 1.0);
    return combiln + betaln_d(k + a, n - k + b) - betaln_d(a, b);
}

}  // namespace

// One block = 64 frames of one utterance (blockIdx.y).  Pass 1 walks 64-token tiles: the direct-form squared distance
// sum_c (f[t, c] - x[n, c])^2 in fp32 on the VALU (channel chunks of f and x staged in LDS, channels summed in order), the score
// -sqrt(.) is written to log_p and folded into a per-thread online max / sum-exp.  The 16 threads of a frame combine theirs in a
// fixed order; pass 2 rewrites each thread's own entries as score - lse + (float)prior.  Each thread owns frames ty + 16 i and
// tokens tx + 16 j of a tile (i, j < 4).
__global__ __launch_bounds__(256) void align_score_kernel(const float* __restrict__ text, const float* __restrict__ feats, int C,
                                                          const AlignSeq* __restrict__ seqs, float* __restrict__ log_p) {
    __shared__ float fs[SC_TF * SC_PITCH];
    __shared__ float xs[SC_TN * SC_PITCH];
    __shared__ float red_m[SC_TF][17], red_s[SC_TF][17];
    const AlignSeq sq = seqs[blockIdx.y];
    const int T = sq.frames, N = sq.tokens;
    const int t0 = blockIdx.x * SC_TF;
    if (t0 >= T) return;
    const int tid = threadIdx.x, tx = tid & 15, ty = tid >> 4;
    const float* frow = feats + (int64_t)(sq.frm_row + t0) * C;     // rows past T are gap / pad rows of the layout (readable, ignored)
    const float* xrow = text + (int64_t)sq.tok_row * C;
    float* lp = log_p + sq.lp_off;
    float m[4], s[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) { m[i] = -INFINITY; s[i] = 0.f; }
    for (int n0 = 0; n0 < N; n0 += SC_TN) {
        float d[4][4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) d[i][j] = 0.f;
        for (int c0 = 0; c0 < C; c0 += SC_KC) {
            __syncthreads();
            for (int e = tid; e < SC_TF * SC_KC; e += 256) {
                const int r = e / SC_KC, c = e % SC_KC;
                fs[r * SC_PITCH + c] = (t0 + r < T) ? frow[(int64_t)r * C + c0 + c] : 0.f;
                xs[r * SC_PITCH + c] = (n0 + r < N) ? xrow[(int64_t)(n0 + r) * C + c0 + c] : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int c = 0; c < SC_KC; ++c) {
                float fv[4], xv[4];
#pragma unroll
                for (int i = 0; i < 4; ++i) { fv[i] = fs[(ty + 16 * i) * SC_PITCH + c]; xv[i] = xs[(tx + 16 * i) * SC_PITCH + c]; }
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j) { const float df = fv[i] - xv[j]; d[i][j] = fmaf(df, df, d[i][j]); }
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + ty + 16 * i;
            if (t >= T) continue;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + tx + 16 * j;
                if (n >= N) continue;
                const float v = -sqrtf(d[i][j]);
                lp[(int64_t)t * N + n] = v;
                if (v > m[i]) { s[i] = s[i] * expf(m[i] - v) + 1.f; m[i] = v; }
                else s[i] += expf(v - m[i]);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { red_m[ty + 16 * i][tx] = m[i]; red_s[ty + 16 * i][tx] = s[i]; }
    __syncthreads();
    float lse[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int r = ty + 16 * i;
        float M = -INFINITY;
        for (int k = 0; k < 16; ++k) M = fmaxf(M, red_m[r][k]);
        float S = 0.f;
        for (int k = 0; k < 16; ++k) if (red_s[r][k] > 0.f) S += red_s[r][k] * expf(red_m[r][k] - M);
        lse[i] = M + logf(S);
    }
    // pass 2: this thread's own entries (written above by the same thread)
    const double Nd = (double)N;
    for (int n0 = 0; n0 < N; n0 += SC_TN) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int t = t0 + ty + 16 * i;
            if (t >= T) continue;
            const double a = (double)(t + 1), b = (double)(T - t);        // alpha = 1..T, beta = T - alpha + 1
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int n = n0 + tx + 16 * j;
                if (n >= N) continue;
                float* e = lp + (int64_t)t * N + n;
                *e = (*e - lse[i]) + (float)log_betabinom((double)n, Nd, a, b);
            }
        }
    }
}

// Monotonic alignment search, one wavefront per utterance (blockIdx.x).  Lane l owns tokens [l * RM, (l + 1) * RM) with their Q values
// in fp64 registers; a frame step needs the previous lane's last Q (one __shfl_up) and no barrier.  Per (token, frame) one decision
// bit, Q[i-1, j-1] >= Q[i, j-1] -- the comparison the backtrack makes -- is written as one 32-bit word per lane and frame.  The
// backtrack stages 64 frames of words in LDS at a time (independent, coalesced loads) and walks them; then the lanes derive
// durations (bincount of the path), the mean of log_p along the path and the per-token means of the frame tracks (fp64 sums).
template <int RM>
__global__ __launch_bounds__(64) void mas_kernel(const float* __restrict__ log_p, const AlignSeq* __restrict__ seqs, uint32_t* __restrict__ bits,
                                                 const float* __restrict__ pitch_frames, const float* __restrict__ energy_frames,
                                                 int64_t* __restrict__ dur, float* __restrict__ pitch_tok, float* __restrict__ energy_tok,
                                                 float* __restrict__ score) {
    __shared__ uint32_t sb[64][65];
    __shared__ int32_t start[EV_ALIGN_MAX_TOKENS + 1];
    __shared__ double red[64];
    const AlignSeq sq = seqs[blockIdx.x];
    const int T = sq.frames, N = sq.tokens, lane = threadIdx.x;
    const float* lp = log_p + sq.lp_off;
    uint32_t* bw = bits + sq.bits_off;
    const int i0 = lane * RM;
    double q[RM];
    float nv[RM];
#pragma unroll
    for (int r = 0; r < RM; ++r) q[r] = (i0 + r == 0) ? (double)lp[0] : -INFINITY;
#pragma unroll
    for (int r = 0; r < RM; ++r) nv[r] = (T > 1 && i0 + r < N) ? lp[(int64_t)N + i0 + r] : -INFINITY;
    for (int j = 1; j < T; ++j) {
        float v[RM];
#pragma unroll
        for (int r = 0; r < RM; ++r) v[r] = nv[r];
        if (j + 1 < T) {
#pragma unroll
            for (int r = 0; r < RM; ++r) nv[r] = (i0 + r < N) ? lp[(int64_t)(j + 1) * N + i0 + r] : -INFINITY;
        }
        double prev = __shfl_up(q[RM - 1], 1);
        if (lane == 0) prev = -INFINITY;
        uint32_t word = 0;
#pragma unroll
        for (int r = RM - 1; r >= 0; --r) {
            const double left = r > 0 ? q[r - 1] : prev;          // Q[i-1, j-1]
            const bool up = left >= q[r];
            word |= (uint32_t)up << r;
            q[r] = (i0 + r == 0 ? q[r] : (up ? left : q[r])) + (double)v[r];
        }
        bw[(int64_t)j * 64 + lane] = word;
    }
    __syncthreads();
    // backtrack: A[T-1] = N-1; A[j] = bit(A[j+1], j+1) ? A[j+1] - 1 : A[j+1]  (A[j+1] == 0 stays 0)
    int cur = N - 1;
    for (int i = lane; i <= N; i += 64) start[i] = i == N ? T : -1;
    __syncthreads();
    for (int hi = T - 1; hi > 0; hi -= 64) {
        const int lo = hi - 63 > 1 ? hi - 63 : 1;
        __syncthreads();
        for (int jj = lo; jj <= hi; ++jj) sb[jj - lo][lane] = bw[(int64_t)jj * 64 + lane];
        __syncthreads();
        if (lane == 0) {
            for (int jj = hi; jj >= lo; --jj) {
                const int ib = cur;
                if (ib > 0 && ((sb[jj - lo][ib / RM] >> (ib % RM)) & 1u)) {
                    cur = ib - 1;
                    start[ib] = jj;              // token ib starts at frame jj
                }
            }
        }
    }
    if (lane == 0) {          // a path that did not reach token 0 (only non-finite log_p can do that) still gives in-range token spans
        for (int i = N - 1; i > 0; --i) if (start[i] < 0 || start[i] > start[i + 1]) start[i] = start[i + 1];
        start[0] = 0;
    }
    __syncthreads();
    double acc = 0.0;
    for (int i = lane; i < N; i += 64) {
        const int a = start[i], e = start[i + 1];
        dur[sq.tok_packed + i] = e - a;
        for (int f = a; f < e; ++f) acc += (double)lp[(int64_t)f * N + i];
        if (pitch_frames) {
            double ps = 0.0;
            for (int f = a; f < e; ++f) ps += (double)pitch_frames[sq.frm_packed + f];
            pitch_tok[sq.tok_packed + i] = (float)(ps / (double)(e - a));
        }
        if (energy_frames) {
            double es = 0.0;
            for (int f = a; f < e; ++f) es += (double)energy_frames[sq.frm_packed + f];
            energy_tok[sq.tok_packed + i] = (float)(es / (double)(e - a));
        }
    }
    red[lane] = acc;
    __syncthreads();
    if (lane == 0) {
        double tot = 0.0;
        for (int k = 0; k < 64; ++k) tot += red[k];
        score[blockIdx.x] = (float)(tot / (double)T);
    }
}

void launch_align_score(const float* text, const float* feats, int C, const AlignSeq* seqs, int B, int max_frames, float* log_p, hipStream_t s) {
    hipLaunchKernelGGL(align_score_kernel, dim3((unsigned)((max_frames + SC_TF - 1) / SC_TF), (unsigned)B), dim3(256), 0, s, text, feats, C, seqs,
                       log_p);
}

int align_mas_run(int max_tokens) {
    int rm = 1;
    while (rm * 64 < max_tokens) rm *= 2;
    return rm;
}

void launch_align_mas(const float* log_p, const AlignSeq* seqs, int B, int max_tokens, uint32_t* bits, const float* pitch_frames,
                      const float* energy_frames, int64_t* dur, float* pitch_tok, float* energy_tok, float* score, hipStream_t s) {
#define EV_MAS(RM) hipLaunchKernelGGL(mas_kernel<RM>, dim3((unsigned)B), dim3(64), 0, s, log_p, seqs, bits, pitch_frames, energy_frames, dur, \
                                      pitch_tok, energy_tok, score)
    switch (align_mas_run(max_tokens)) {
        case 1: EV_MAS(1); break;
        case 2: EV_MAS(2); break;
        case 4: EV_MAS(4); break;
        case 8: EV_MAS(8); break;
        case 16: EV_MAS(16); break;
        default: EV_MAS(32); break;
    }
#undef EV_MAS
}

}  // namespace ev
