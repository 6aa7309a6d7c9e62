// Objective scoring (ev_score): log-mel -> integer mel-cepstra, local distances, dynamic time warping and the sums along the warp's path.
// include/evhip.h states the specification; everything that decides a bit is integer arithmetic or an fp64 operation of exact operands.
//
// score_cepstra: one block per SCORE_TF frames of one signal (a host-built tile table: signals have ragged lengths).  The tile's mel values and the
//   basis sit in LDS; a frame lies on a lane, the four waves take the coefficients d = w, w + 4, ...; the sum over m is a chain of fp64 additions of
//   exact products, m ascending.  Loads run along t, the fast axis of (n_mels, T).
// score_count: one wave per signal adds the per-frame non-finite flags (integers: any order).
// score_dist: the local distances of the pairs of one pass that share a run, over the whole chip, written in the order the warp reads them (ev_kernels.h).  A block takes 64 steps
//   x 64 lanes of one run index r: the 64 rows l * rm + r of a and the 127 columns the steps reach, both in LDS at an odd row stride.
// score_dtw: one wavefront per pair.  Lane l owns rm consecutive rows of a with their accumulated costs in fp64 registers (integers below 2^44: exact);
//   at step s it works on column s - l, which makes (i - 1, j) of its first row available: the lane above finished that column one step earlier and
//   column j - 1 two steps earlier, so one __shfl_up per step (and the value received a step ago) delivers both.  No barrier, no atomics.  Each cell
//   emits a 2-bit decision, packed per lane and step.  The backtrack stages decision words in LDS in chunks and lane 0 walks them; the path is
//   written from the end of a scratch of Ta + Tb - 1 slots because its length is known only when (0, 0) is reached.
// score_sums: one wave per pair copies the path to its place, counts the steps and the voiced / unvoiced cells, and adds the F0 terms in path
//   order (the chain of additions is serial, the log2 of 64 cells at a time is not).  For a linear score it also computes dist(k, k).
#include <hip/hip_runtime.h>
#include <limits.h>
#include <math.h>
#include <stdint.h>

#include "ev_audio_dev.h"
#include "ev_kernels.h"

// every product and every sum of the specification is rounded on its own
#pragma clang fp contract(off)

namespace ev {

namespace {

constexpr int CQ_LD = SCORE_MAX_CEPS + 1;      // LDS row stride of a cq row: odd, so 64 rows fall on different banks

// the largest r with r * r <= s (s < 2^61): an fp64 guess, then integer correction in both directions
__device__ inline uint32_t isqrt_u64(uint64_t s) {
    uint64_t r = (uint64_t)sqrt((double)s);
#pragma unroll 1
    for (int k = 0; k < 4 && r * r > s; ++k) --r;
#pragma unroll 1
    for (int k = 0; k < 4 && (r + 1) * (r + 1) <= s; ++k) ++r;
    return (uint32_t)r;
}

__device__ inline uint64_t sq_dist(const int32_t* a, const int32_t* b, int D) {
    uint64_t s = 0;
    for (int d = 0; d < D; ++d) {
        const int32_t e = a[d] - b[d];      // both within +-2^27
        s += (uint64_t)((int64_t)e * (int64_t)e);
    }
    return s;
}

}  // namespace

__global__ __launch_bounds__(256) void score_cepstra_kernel(const float* __restrict__ mel, const ScoreTile* __restrict__ tiles, const float* __restrict__ basis,
                                                             int M, int D, int32_t* __restrict__ cq, int32_t* __restrict__ bad) {
    __shared__ float s_mel[SCORE_MAX_MELS][SCORE_TF];
    __shared__ float s_bas[SCORE_MAX_CEPS * SCORE_MAX_MELS];
    const ScoreTile tl = tiles[blockIdx.x];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int nt = tl.T - tl.t0 < SCORE_TF ? tl.T - tl.t0 : SCORE_TF;
    const float* src = mel + tl.mel_off + tl.t0;
    for (int m = w; m < M; m += 4) s_mel[m][lane] = lane < nt ? src[(int64_t)m * tl.T + lane] : 0.f;
    for (int k = tid; k < D * M; k += 256) s_bas[k] = basis[k];
    __syncthreads();
    if (lane >= nt) return;
    const int64_t f = tl.frm_off + tl.t0 + lane;
    if (w == 0) {
        int nf = 0;
        for (int m = 0; m < M; ++m) nf |= isfinite(s_mel[m][lane]) ? 0 : 1;
        bad[f] = nf;
    }
    for (int d = w; d < D; d += 4) {
        const float* bs = s_bas + d * M;
        double x = 0.0;
        for (int m = 0; m < M; ++m) x += (double)s_mel[m][lane] * (double)bs[m];
        int32_t q = 0;
        if (isfinite(x)) {
            double y = x * 65536.0;
            y = y < -(double)SCORE_CLAMP ? -(double)SCORE_CLAMP : (y > (double)SCORE_CLAMP ? (double)SCORE_CLAMP : y);
            q = (int32_t)rint(y);      // ties to even
        }
        cq[f * D + d] = q;
    }
}

__global__ __launch_bounds__(64) void score_count_kernel(const int32_t* __restrict__ bad, const ScoreSig* __restrict__ sigs, int32_t* __restrict__ nonfinite) {
    const ScoreSig sg = sigs[blockIdx.x];
    int n = 0;
    for (int t = threadIdx.x; t < sg.T; t += 64) n += bad[sg.frm_off + t];
    n = wave_sum_i32(n);
    if (threadIdx.x == 0) nonfinite[blockIdx.x] = n;
}

// grid (step tiles, run indices, the pairs of one pass that share a run: sel); a block whose tile its pair does not have leaves at once
__global__ __launch_bounds__(256) void score_dist_kernel(const int32_t* __restrict__ cqa, const int32_t* __restrict__ cqb, int D,
                                                          const ScorePair* __restrict__ pairs, const int32_t* __restrict__ sel,
                                                          uint32_t* __restrict__ dist) {
    __shared__ int32_t s_a[64 * CQ_LD];
    __shared__ int32_t s_b[128 * CQ_LD];
    const ScorePair p = pairs[sel[blockIdx.z]];
    const int r = blockIdx.y, s0 = blockIdx.x * 64;
    const int L = (p.Ta + p.rm - 1) / p.rm;      // lanes that own a row
    if (r >= p.rm || s0 >= p.Tb + L - 1) return;
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int j0 = s0 - 63;                      // the first column any (step, lane) of the tile reaches
    for (int k = tid; k < 64 * D; k += 256) {
        const int l = k / D, d = k - l * D, i = l * p.rm + r;
        s_a[l * CQ_LD + d] = i < p.Ta ? cqa[(p.fa_off + i) * D + d] : 0;
    }
    for (int k = tid; k < 127 * D; k += 256) {
        const int c = k / D, d = k - c * D, j = j0 + c;
        s_b[c * CQ_LD + d] = j >= 0 && j < p.Tb ? cqb[(p.fb_off + j) * D + d] : 0;
    }
    __syncthreads();
    const int i = lane * p.rm + r;
    if (i >= p.Ta) return;
    uint32_t* out = dist + p.dist_off;
    for (int q = w; q < 64; q += 4) {
        const int s = s0 + q, j = s - lane;
        if (j < 0 || j >= p.Tb) continue;
        out[((int64_t)s * p.rm + r) * 64 + lane] = isqrt_u64(sq_dist(s_a + lane * CQ_LD, s_b + (j - j0) * CQ_LD, D));
    }
}

template <int RM>
__global__ __launch_bounds__(64) void score_dtw_kernel(const ScorePair* __restrict__ pairs, const int32_t* __restrict__ sel, const uint32_t* __restrict__ dist,
                                                       uint32_t* __restrict__ dec, int32_t* __restrict__ rev, ScoreWarp* __restrict__ warp) {
    constexpr int W = score_dec_words(RM), CH = 64 / W;      // decision words per lane and step; steps the backtrack stages at a time
    __shared__ uint32_t sb[CH * W * 64];
    const int pi = sel[blockIdx.x];
    const ScorePair p = pairs[pi];
    const int Ta = p.Ta, Tb = p.Tb, lane = threadIdx.x;
    const uint32_t* dp = dist + p.dist_off;
    uint32_t* dw = dec + p.dec_off;
    const int i0 = lane * RM;
    const int L = (Ta + RM - 1) / RM, nsteps = Tb + L - 1;
    const bool owner = i0 < Ta;
    double q[RM];
    uint32_t nv[RM];
#pragma unroll
    for (int r = 0; r < RM; ++r) q[r] = INFINITY;
#pragma unroll
    for (int r = 0; r < RM; ++r) nv[r] = (lane == 0 && r < Ta) ? dp[(int64_t)r * 64] : 0u;      // step 0: lane 0, column 0
    double up_prev = INFINITY;      // what the lane above held two steps ago: its last row at column j - 1
    double fin = 0.0;
    for (int s = 0; s < nsteps; ++s) {
        uint32_t v[RM];
#pragma unroll
        for (int r = 0; r < RM; ++r) v[r] = nv[r];
        {
            const int jn = s + 1 - lane;
            const bool ld = s + 1 < nsteps && owner && jn >= 0 && jn < Tb;
#pragma unroll
            for (int r = 0; r < RM; ++r) nv[r] = (ld && i0 + r < Ta) ? dp[((int64_t)(s + 1) * RM + r) * 64 + lane] : 0u;
        }
        double up0 = __shfl_up(q[RM - 1], 1);
        if (lane == 0) up0 = INFINITY;
        const int j = s - lane;
        if (owner && j >= 0 && j < Tb) {
            double dg = up_prev, up = up0;
            uint32_t word[W];
#pragma unroll
            for (int k = 0; k < W; ++k) word[k] = 0;
#pragma unroll
            for (int r = 0; r < RM; ++r) {
                const double left = q[r];
                const bool diag = dg <= up && dg <= left;
                const bool astep = up <= left;
                double m = diag ? dg : (astep ? up : left);
                if (r == 0 && lane == 0 && j == 0) m = 0.0;
                const uint32_t code = diag ? 0u : (astep ? 1u : 2u);
                word[r / 16] |= code << (2 * (r % 16));
                const double nq = m + (double)v[r];
                dg = left; up = nq; q[r] = nq;
            }
#pragma unroll
            for (int k = 0; k < W; ++k) dw[((int64_t)s * W + k) * 64 + lane] = word[k];
        }
        up_prev = up0;
    }
#pragma unroll
    for (int r = 0; r < RM; ++r) if (i0 + r == Ta - 1) fin = q[r];
    __syncthreads();
    // backtrack from (Ta - 1, Tb - 1); the step of a cell never grows along it
    const int cap = Ta + Tb - 1;
    int32_t* ra = rev + p.rev_off;
    int32_t* rb = ra + cap;
    int ci = Ta - 1, cj = Tb - 1, pos = cap - 1;
    if (lane == 0) { ra[pos] = ci; rb[pos] = cj; }
    for (int hi = nsteps - 1; hi >= 0; hi -= CH) {
        const int lo = hi - CH + 1 > 0 ? hi - CH + 1 : 0;
        __syncthreads();
        for (int k = lane; k < (hi - lo + 1) * W * 64; k += 64) sb[k] = dw[(int64_t)lo * W * 64 + k];
        __syncthreads();
        if (lane == 0) {
            for (int it = 0; it < cap && (ci > 0 || cj > 0); ++it) {
                const int l = ci / RM, r = ci % RM, s = cj + l;
                if (s < lo) break;
                uint32_t code = (sb[((s - lo) * W + r / 16) * 64 + l] >> (2 * (r % 16))) & 3u;
                if (ci == 0) code = 2u; else if (cj == 0) code = 1u;      // the grid's edges leave one predecessor
                if (code != 2u) --ci;
                if (code != 1u) --cj;
                --pos;
                ra[pos] = ci; rb[pos] = cj;
            }
        }
    }
    const double total = lane_value(fin, (Ta - 1) / RM);
    if (lane == 0) { warp[pi].sum_dist = (int64_t)total; warp[pi].K = cap - pos; warp[pi].pad = 0; }
}

__global__ __launch_bounds__(64) void score_sums_kernel(const ScorePair* __restrict__ pairs, int linear, const int32_t* __restrict__ cqa,
                                                        const int32_t* __restrict__ cqb, int D, const int32_t* __restrict__ rev,
                                                        const ScoreWarp* __restrict__ warp, const float* __restrict__ f0a, const float* __restrict__ f0b,
                                                        int32_t* __restrict__ path_a, int32_t* __restrict__ path_b, ScoreSums* __restrict__ out) {
    const ScorePair p = pairs[blockIdx.x];
    const int lane = threadIdx.x, K = p.K, cap = p.Ta + p.Tb - 1;
    const int32_t* ra = rev + p.rev_off + (cap - K);
    const int32_t* rb = rev + p.rev_off + cap + (cap - K);
    int n_diag = 0, n_a = 0, n_b = 0, n_vv = 0, n_vu = 0, n_uv = 0, n_uu = 0;
    int64_t sd = 0;
    double sc = 0.0, sc2 = 0.0;
    for (int k0 = 0; k0 < K; k0 += 64) {
        const int k = k0 + lane;
        const bool in = k < K;
        int i = 0, j = 0, pi = 0, pj = 0;
        if (in) {
            if (linear) { i = j = k; pi = pj = k - 1; }
            else { i = ra[k]; j = rb[k]; if (k > 0) { pi = ra[k - 1]; pj = rb[k - 1]; } }
            path_a[p.path_off + k] = i; path_b[p.path_off + k] = j;
            if (k > 0) {
                const bool da = i != pi, db = j != pj;
                n_diag += da && db; n_a += da && !db; n_b += !da && db;
            }
            if (linear) sd += (int64_t)isqrt_u64(sq_dist(cqa + (p.fa_off + i) * D, cqb + (p.fb_off + j) * D, D));
        }
        double c = 0.0;
        if (f0a && f0b) {
            const float fa = in ? f0a[p.fa_off + i] : 0.f, fb = in ? f0b[p.fb_off + j] : 0.f;
            const bool va = isfinite(fa) && fa > 0.f, vb = isfinite(fb) && fb > 0.f;
            n_vv += in && va && vb; n_vu += in && va && !vb; n_uv += in && !va && vb; n_uu += in && !va && !vb;
            if (in && va && vb) c = 1200.0 * log2((double)fa / (double)fb);
            const double c2 = c * c;
            // ascending path order; a cell that is not voiced on both sides adds +0.0, which changes no sum
#pragma unroll
            for (int t = 0; t < 64; ++t) { sc += lane_value(c, t); sc2 += lane_value(c2, t); }
        }
    }
    n_diag = wave_sum_i32(n_diag); n_a = wave_sum_i32(n_a); n_b = wave_sum_i32(n_b);
    n_vv = wave_sum_i32(n_vv); n_vu = wave_sum_i32(n_vu); n_uv = wave_sum_i32(n_uv); n_uu = wave_sum_i32(n_uu);
    sd = wave_sum_i64(sd);
    if (lane == 0) {
        ScoreSums r;
        r.sum_dist = linear ? sd : warp[blockIdx.x].sum_dist;
        r.sum_c = sc; r.sum_c2 = sc2;
        r.n_diag = n_diag; r.n_a = n_a; r.n_b = n_b; r.n_vv = n_vv; r.n_vu = n_vu; r.n_uv = n_uv; r.n_uu = n_uu; r.pad = 0;
        out[blockIdx.x] = r;
    }
}

int launch_score_cepstra(const float* mel, const ScoreTile* tiles, int64_t n_tiles, const float* basis, int M, int D, int32_t* cq, int32_t* bad, hipStream_t s) {
    if (n_tiles < 1 || n_tiles > INT_MAX || M < 1 || M > SCORE_MAX_MELS || D < 1 || D > SCORE_MAX_CEPS) return -1;
    hipLaunchKernelGGL(score_cepstra_kernel, dim3((unsigned)n_tiles), dim3(256), 0, s, mel, tiles, basis, M, D, cq, bad);
    return 0;
}

void launch_score_count(const int32_t* bad, const ScoreSig* sigs, int B, int32_t* nonfinite, hipStream_t s) {
    hipLaunchKernelGGL(score_count_kernel, dim3((unsigned)B), dim3(64), 0, s, bad, sigs, nonfinite);
}

int launch_score_dist(const int32_t* cqa, const int32_t* cqb, int D, const ScorePair* pairs, const int32_t* sel, int n, int rm, int max_steps, uint32_t* dist,
                      hipStream_t s) {
    if (n < 1 || n > 65535 || rm < 1 || rm > 64 || max_steps < 1 || D < 1 || D > SCORE_MAX_CEPS) return -1;
    hipLaunchKernelGGL(score_dist_kernel, dim3((unsigned)((max_steps + 63) / 64), (unsigned)rm, (unsigned)n), dim3(256), 0, s, cqa, cqb, D, pairs, sel, dist);
    return 0;
}

int launch_score_dtw(int rm, const ScorePair* pairs, const int32_t* sel, int n, const uint32_t* dist, uint32_t* dec, int32_t* rev, ScoreWarp* warp, hipStream_t s) {
    if (n < 1) return -1;
#define EV_DTW(RM) hipLaunchKernelGGL(score_dtw_kernel<RM>, dim3((unsigned)n), dim3(64), 0, s, pairs, sel, dist, dec, rev, warp)
    switch (rm) {
        case 1: EV_DTW(1); break;
        case 2: EV_DTW(2); break;
        case 4: EV_DTW(4); break;
        case 8: EV_DTW(8); break;
        case 16: EV_DTW(16); break;
        case 32: EV_DTW(32); break;
        case 64: EV_DTW(64); break;
        default: return -1;
    }
#undef EV_DTW
    return 0;
}

void launch_score_sums(const ScorePair* pairs, int B, int linear, const int32_t* cqa, const int32_t* cqb, int D, const int32_t* rev, const ScoreWarp* warp,
                       const float* f0a, const float* f0b, int32_t* path_a, int32_t* path_b, ScoreSums* out, hipStream_t s) {
    hipLaunchKernelGGL(score_sums_kernel, dim3((unsigned)B), dim3(64), 0, s, pairs, linear, cqa, cqb, D, rev, warp, f0a, f0b, path_a, path_b, out);
}

}  // namespace ev
