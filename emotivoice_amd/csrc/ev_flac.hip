// FLAC encoding (ev_flac): packed 16-bit PCM (or the fp32 that converts to it) -> one FLAC stream per segment.  include/evhip.h states the
// specification; everything here is integer arithmetic whose result does not depend on the order of execution.
//
// flac_encode: one 256-thread block per frame (a block of n <= N samples of one segment).
//   1. The samples go into LDS as int32, converted on the way in; a flag records whether any differs from the first (CONSTANT otherwise).
//   2. The block is cut into its finest valid partitions (P = 2^pmax, pmax = min(max_partition_order, ctz(n))); 256 / P consecutive threads share a
//      partition and stride through it.  A thread keeps, for every order o and Rice parameter k, the sum of u >> k over its samples; the sums are
//      folded inside the thread group by wave shuffles and land in s_sum[o][k][partition] by an LDS integer add (at most four adders per cell,
//      one per wave, when a partition spans waves).  A term is clamped at FL_CLAMP = 2^17: a partition that holds such a term costs more than any
//      VERBATIM subframe under every parameter that clamps, so neither its parameter (a parameter that does not clamp is exact and smaller) nor
//      the decision changes, and the 32-bit sums cannot overflow (4096 * 2^17 = 2^29).
//   3. From the finest level upwards: the best parameter and cost of every (order, partition), summed per (order, level); then neighbouring
//      partitions are added in place (a partition's cell is the cell of its first finest partition) for the next coarser level.
//   4. Thread 0 applies the specification's tie rules and writes the frame header with its CRC-8.
//   5. The subframe is assembled in a zeroed LDS buffer.  A block-wide prefix sum over the code lengths, 256 samples a round, gives every sample its
//      bit position; a sample ORs in its stop bit and remainder (at most 15 bits, two words) with LDS atomics, the unary zeros are already there.
//   6. CRC-16: linear with initial value 0.  The frame is right-aligned in 256 runs of R bytes (leading zero bytes do not change a CRC that starts
//      at 0), every thread takes one run, and a halving tree joins neighbours: crc(A || B) = crc(A) x^(8 |B|) + crc(B) mod the polynomial.
//   7. The frame goes to its fixed-stride slot of the scratch buffer, its size and decision to per-frame arrays.
// flac_encode<true> (ev_flac_lpc) adds the LPC candidates of the specification's rules 4 .. 9; flac_encode<false> is the kernel above and nothing else.
//   a. Analysis (lpc_analyse): the windowed block y goes, as int16, into the still unused frame buffer.  Every thread keeps int64 partial sums of
//      the 13 lags over its samples; they are folded by wave shuffles and one LDS 64-bit add per wave and lag (integers: any order gives the same
//      sum).  Thread 0 runs the Levinson recursion in fp64, one IEEE operation per rounding (contraction is off around it), and quantises every
//      order; the coefficients and shifts of all orders stay in LDS.  The frame buffer is zeroed again.
//   b. Search: the candidates are walked in passes of five through the same s_sum / s_cost / s_k: pass 0 the FIXED orders, pass 1 + t the LPC
//      orders 5 t + 1 .. 5 t + 5.  After a pass thread 0 compares its candidates with the best so far (strictly smaller wins, which is the
//      specification's tie rule in this order of visits) and the winner's Rice parameters are copied out of s_k before the next pass reuses it.
//   c. FL_CLAMP for LPC residuals: an order with a residual outside int32 is dropped (s_bad), so u = zigzag(r) is a uint32 and a term u >> k may
//      reach 2^32 >> k, far above a FIXED term.  The argument above does not use the size of the terms: a partition that holds a term >= 2^17
//      under parameter k costs more than 2^17 > 8 + 16 * 4096 bits under k, which is more than VERBATIM; a candidate whose chosen parameters all
//      clamp loses to VERBATIM with its true cost as with its clamped cost, and a candidate that wins has no clamped term under its chosen
//      parameters, so its cost is exact.  The sums stay below 4096 * 2^17 = 2^29 per cell, and s_cost below 2^29 + 64 * (4 + 15 * 4096).
// flac_lpc_analysis: step a alone, one block per frame, for ev_op_flac_lpc.
// flac_md5: one wave per segment.  MD5's 64-byte rounds are one serial chain, so the wave does not split them: its lanes fetch and convert the
//   next 64 rounds' words (16 per lane, the RFC's padding and length included) into registers, every lane runs the current 64 rounds from LDS
//   (the same address in all lanes: a broadcast), then the registers go to the other LDS buffer.
// flac_gather: one block per frame copies the slot to the frame's byte offset in the output (word stores once the destination is aligned); the
//   block of a stream's first frame also copies the stream's 42 header bytes, which the host builds from the frame sizes.
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

#include "ev_kernels.h"

namespace ev {

namespace {

constexpr uint32_t FL_CLAMP = 1u << 17;
constexpr int FL_BUF_WORDS = (2 * FLAC_MAX_BLOCK + 24) / 4 + 2;      // the frame and one word of slack behind it for put_bits' second word
constexpr int FL_LPC = FLAC_LPC_MAX_ORDER;
static_assert(FL_BUF_WORDS * 4 >= FLAC_MAX_BLOCK * 2, "the windowed block borrows the frame buffer");

// the specification's conversion: one fp32 product, NaN -> 0, truncation toward zero saturated to int32, then wrap or clamp
__device__ inline int32_t to_pcm(float x, int clamp) {
    const float t = x * 32768.0f;
    int32_t v;
    if (t != t) v = 0;
    else if (t >= 2147483648.0f) v = INT_MAX;
    else if (t <= -2147483648.0f) v = INT_MIN;
    else v = (int32_t)t;
    return clamp ? min(max(v, -32768), 32767) : (int32_t)(int16_t)(uint16_t)((uint32_t)v & 0xFFFFu);
}

__device__ inline int32_t load_pcm(const FlacParams& P, int64_t i) {
    if (P.pcm_is_i16) return reinterpret_cast<const int16_t*>(P.pcm)[i];
    return to_pcm(reinterpret_cast<const float*>(P.pcm)[i], P.convert);
}

// nbits <= 32 bits of val, most significant first, at bit `pos` of the big-endian bit stream kept in 32-bit words; the buffer starts out zero
__device__ inline void put_bits(uint32_t* buf, uint32_t pos, uint32_t val, int nbits) {
    const uint64_t v = (uint64_t)val << (64 - nbits - (int)(pos & 31u));
    const uint32_t hi = (uint32_t)(v >> 32), lo = (uint32_t)v;
    if (hi) atomicOr(&buf[pos >> 5], hi);
    if (lo) atomicOr(&buf[(pos >> 5) + 1], lo);
}
__device__ inline uint32_t get_byte(const uint32_t* buf, int b) { return (buf[b >> 2] >> (24 - 8 * (b & 3))) & 0xFFu; }

// the o-th finite difference at i >= o; int32 holds it (|r| <= 16 * 32768)
__device__ inline int32_t resid(const int32_t* x, int i, int o) {
    switch (o) {
        case 0: return x[i];
        case 1: return x[i] - x[i - 1];
        case 2: return x[i] - 2 * x[i - 1] + x[i - 2];
        case 3: return x[i] - 3 * x[i - 1] + 3 * x[i - 2] - x[i - 3];
        default: return x[i] - 4 * x[i - 1] + 6 * x[i - 2] - 4 * x[i - 3] + x[i - 4];
    }
}
// the residual of LPC order o at i >= o (rule 8); *bad is raised when it leaves int32
__device__ inline int32_t lpc_resid(const int32_t* x, int i, int o, const int32_t* c, int shift, bool* bad) {
    int64_t pred = 0;
    for (int j = 0; j < o; ++j) pred += (int64_t)c[j] * (int64_t)x[i - 1 - j];
    const int64_t r = (int64_t)x[i] - (pred >> shift);
    if (r >= (int64_t)1 << 31 || r <= -((int64_t)1 << 31)) { *bad = true; return 0; }
    return (int32_t)r;
}

// Rules 4 .. 7 for the block x[0 .. n): R[0 .. 12] (zero beyond L = min(max_order, n - 1)), and per order o = 1 .. 12 shift[o - 1] (-1: no candidate)
// and c[(o - 1) * 12 + j].  y: n int16 of scratch.  Called by all 256 threads; the results are visible after it returns.
__device__ void lpc_analyse(const int32_t* x, int n, int max_order, int q, int16_t* y, unsigned long long* R, int32_t* c, int* shift) {
    const int tid = threadIdx.x, lane = tid & 63;
    if (tid < 13) R[tid] = 0;
    if (tid < FL_LPC) shift[tid] = -1;
    if (tid < FL_LPC * FL_LPC) c[tid] = 0;
    const int L = min(max_order, n - 1);
    if (L >= 1) {
        const int64_t den = (int64_t)(n - 1) * (int64_t)(n - 1);
        for (int i = tid; i < n; i += 256) {
            const int32_t w = (int32_t)(((int64_t)(32767 * 4) * (int64_t)i * (int64_t)(n - 1 - i)) / den);
            y[i] = (int16_t)((x[i] * w) >> 15);
        }
    }
    __syncthreads();
    if (L < 1) return;
    int64_t acc[13];
#pragma unroll
    for (int l = 0; l < 13; ++l) acc[l] = 0;
    for (int i = tid; i < n; i += 256) {
        const int32_t yi = y[i];
#pragma unroll
        for (int l = 0; l < 13; ++l)
            if (l <= L && i >= l) acc[l] += (int64_t)(yi * (int32_t)y[i - l]);
    }
#pragma unroll
    for (int l = 0; l < 13; ++l) {
        if (l > L) continue;
        long long v = acc[l];
        for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
        if (lane == 0) atomicAdd(&R[l], (unsigned long long)v);
    }
    __syncthreads();
    if (tid == 0 && R[0] != 0) {
#pragma clang fp contract(off)
        double a[FL_LPC], t[FL_LPC];
        double err = (double)(long long)R[0];
        for (int it = 0; it < L; ++it) {
            double s = (double)(long long)R[it + 1];
            for (int j = 0; j < it; ++j) s = s - a[j] * (double)(long long)R[it - j];
            const double k = s / err;
            for (int j = 0; j < it; ++j) t[j] = a[j] - k * a[it - 1 - j];
            t[it] = k;
            for (int j = 0; j <= it; ++j) a[j] = t[j];
            err = err * (1.0 - k * k);
            if (!(err > 0.0) || err > 1.7976931348623157e308) break;
            double cmax = 0.0;
            for (int j = 0; j <= it; ++j) cmax = fmax(cmax, fabs(a[j]));
            if (cmax == 0.0) continue;
            const int be = (int)((__double_as_longlong(cmax) >> 52) & 0x7FF);      // cmax = f 2^e, f in [0.5, 1): e = be - 1022; a subnormal's e is smaller still
            if (be == 0x7FF) continue;
            int sh = q - 1 - (be ? be - 1022 : -1022);
            if (sh < 0) continue;
            if (sh > 15) sh = 15;
            const double scale = (double)(1 << sh), lo = -(double)(1 << (q - 1)), hi = (double)((1 << (q - 1)) - 1);
            for (int j = 0; j <= it; ++j) c[it * FL_LPC + j] = (int32_t)fmin(fmax(rint(a[j] * scale), lo), hi);
            shift[it] = sh;
        }
    }
    __syncthreads();
}

__device__ inline uint32_t zigzag(int32_t r) { return ((uint32_t)r << 1) ^ (uint32_t)(r >> 31); }

// a * b mod x^16 + x^15 + x^2 + 1 over GF(2); bit i is the coefficient of x^i
__device__ inline uint32_t gf_mul16(uint32_t a, uint32_t b) {
    uint32_t r = 0;
#pragma unroll
    for (int i = 15; i >= 0; --i) {
        r <<= 1;
        if (r & 0x10000u) r ^= 0x18005u;
        if ((b >> i) & 1u) r ^= a;
    }
    return r;
}

}  // namespace

template <bool LPC>
__global__ __launch_bounds__(256) void flac_encode_kernel(FlacParams P, FlacLpc Q) {
    __shared__ int32_t s_x[FLAC_MAX_BLOCK];
    __shared__ uint32_t s_buf[FL_BUF_WORDS];
    __shared__ uint32_t s_sum[5 * 15 * 64];      // [order][k][finest partition]
    __shared__ uint32_t s_cost[5][8];            // [order][level]: the sum of 4 + cost over the level's partitions
    __shared__ uint8_t s_k[5][128];              // [order][2^level - 1 + partition]: the best parameter
    __shared__ uint32_t s_scan[2][4];
    __shared__ uint32_t s_crc[256];
    __shared__ uint16_t s_tab[256];              // CRC-16 of one byte
    __shared__ int s_diff;
    __shared__ int s_dec[5];                     // kind, order, partition order, the frame header's bits, the subframe's bits
    __shared__ unsigned long long s_R[LPC ? 13 : 1];
    __shared__ int32_t s_c[LPC ? FL_LPC * FL_LPC : 1];      // [order - 1][j]
    __shared__ int s_shift[LPC ? FL_LPC : 1];               // [order - 1]; -1: no candidate
    __shared__ uint8_t s_kb[LPC ? 128 : 1];                 // s_k of the best candidate so far
    __shared__ int s_bad[LPC ? 5 : 1];                      // [slot]: a residual left int32
    __shared__ int s_win;                                   // the slot of a pass's candidate that became the best, or -1

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const FlacFrame fr = P.frames[blockIdx.x];
    const int n = fr.n;

    // 1. samples, tables, zeroed buffers
    const int32_t x0 = load_pcm(P, fr.src);
    if (tid == 0) s_diff = 0;
    for (int i = tid; i < FL_BUF_WORDS; i += 256) s_buf[i] = 0;
    for (int i = tid; i < 5 * 15 * 64; i += 256) s_sum[i] = 0;
    if (tid < 40) s_cost[tid >> 3][tid & 7] = 0;
    {
        uint32_t c = (uint32_t)tid << 8;
#pragma unroll
        for (int b = 0; b < 8; ++b) c = (c & 0x8000u) ? ((c << 1) ^ 0x8005u) & 0xFFFFu : (c << 1) & 0xFFFFu;
        s_tab[tid] = (uint16_t)c;
    }
    __syncthreads();      // s_diff = 0 before anybody raises it
    bool differs = false;
    for (int i = tid; i < n; i += 256) {
        const int32_t v = load_pcm(P, fr.src + i);
        s_x[i] = v;
        differs |= v != x0;
    }
    if (differs) s_diff = 1;
    __syncthreads();

    const int mo = min(P.max_fixed_order, n - 1);
    const int pmax = min(P.max_partition_order, __ffs(n) - 1);
    int L = 0;
    if constexpr (LPC) {
        L = min(Q.max_order, n - 1);
        if (s_diff) {
            lpc_analyse(s_x, n, Q.max_order, Q.precision, reinterpret_cast<int16_t*>(s_buf), s_R, s_c, s_shift);
            for (int i = tid; i < FL_BUF_WORDS; i += 256) s_buf[i] = 0;
            __syncthreads();
        }
    }
    uint32_t best = 0xFFFFFFFFu; int b_kind = 0, b_order = 0, b_porder = 0;      // thread 0's: the best candidate so far
    if (s_diff) {      // the same value in every thread
        const int npass = LPC ? 1 + (L + 4) / 5 : 1;
        for (int pass = 0; pass < npass; ++pass) {
            // slot o of this pass is FIXED order o (pass 0) or LPC order base + o; ns slots
            const bool lp = LPC && pass > 0;
            const int base = lp ? 5 * (pass - 1) + 1 : 0;
            const int ns = lp ? min(5, L - base + 1) : mo + 1;
            if (lp) {
                __syncthreads();      // the last pass's s_k and s_cost have been read
                for (int i = tid; i < 5 * 15 * 64; i += 256) s_sum[i] = 0;
                if (tid < 40) s_cost[tid >> 3][tid & 7] = 0;
                if (tid < 5) s_bad[tid] = 0;
                __syncthreads();
            }
            // 2. sums over the finest partitions
            {
                const int S = n >> pmax, T = 256 >> pmax;      // 2^pmax partitions of S samples, T >= 4 consecutive threads each
                const int j = tid / T, sub = tid & (T - 1);
                uint32_t acc[5][15];
#pragma unroll
                for (int o = 0; o < 5; ++o)
#pragma unroll
                    for (int k = 0; k < 15; ++k) acc[o][k] = 0;
                for (int i = j * S + sub; i < (j + 1) * S; i += T) {
#pragma unroll
                    for (int o = 0; o < 5; ++o) {
                        if (o < ns && i >= base + o) {
                            int32_t r;
                            if (lp) {
                                const int sh = s_shift[base + o - 1];
                                if (sh < 0) continue;
                                bool bad = false;
                                r = lpc_resid(s_x, i, base + o, &s_c[(base + o - 1) * FL_LPC], sh, &bad);
                                if (bad) s_bad[o] = 1;
                            } else r = resid(s_x, i, o);
                            const uint32_t u = zigzag(r);
#pragma unroll
                            for (int k = 0; k < 15; ++k) acc[o][k] += min(u >> k, FL_CLAMP);
                        }
                    }
                }
                const int width = min(T, 64);
#pragma unroll
                for (int o = 0; o < 5; ++o) {
                    if (o >= ns) continue;
#pragma unroll
                    for (int k = 0; k < 15; ++k) {
                        uint32_t v = acc[o][k];
                        for (int d = width >> 1; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
                        if ((lane & (width - 1)) == 0) atomicAdd(&s_sum[(o * 15 + k) * 64 + j], v);
                    }
                }
            }
            __syncthreads();
            // 3. levels pmax .. 0
            for (int p = pmax; p >= 0; --p) {
                const int sh = pmax - p, size = n >> p;
                for (int idx = tid; idx < (ns << p); idx += 256) {
                    const int o = idx >> p, j = idx & ((1 << p) - 1);
                    if (size <= base + o) continue;
                    const uint32_t cnt = (uint32_t)(size - (j == 0 ? base + o : 0));
                    uint32_t bst = 0xFFFFFFFFu; int bk = 0;
                    for (int k = 0; k < 15; ++k) {
                        const uint32_t c = (uint32_t)(k + 1) * cnt + s_sum[(o * 15 + k) * 64 + (j << sh)];
                        if (c < bst) { bst = c; bk = k; }
                    }
                    s_k[o][(1 << p) - 1 + j] = (uint8_t)bk;
                    atomicAdd(&s_cost[o][p], 4u + bst);
                }
                __syncthreads();
                if (p > 0) {
                    const int half = 1 << (p - 1);
                    for (int idx = tid; idx < ns * 15 * half; idx += 256) {
                        const int ok = idx >> (p - 1), j = idx & (half - 1);
                        uint32_t* cell = &s_sum[ok * 64 + ((2 * j) << sh)];
                        cell[0] += cell[1 << sh];
                    }
                    __syncthreads();
                }
            }
            // the pass's candidates against the best so far: strictly smaller wins, so FIXED beats LPC and the smaller order wins on a tie
            if (tid == 0) {
                int win = -1;
                for (int o = 0; o < ns; ++o) {
                    const int ord = base + o;
                    if (lp && (s_shift[ord - 1] < 0 || s_bad[o])) continue;
                    uint32_t bc = 0xFFFFFFFFu; int bp = 0;
                    for (int p = 0; p <= pmax; ++p) {
                        if ((n >> p) <= ord) continue;
                        const uint32_t c = 4u + s_cost[o][p];
                        if (c < bc) { bc = c; bp = p; }
                    }
                    const uint32_t bits = 8u + 16u * (uint32_t)ord + 2u + bc + (lp ? 9u + (uint32_t)(Q.precision * ord) : 0u);
                    if (bits < best) { best = bits; b_order = ord; b_porder = bp; b_kind = lp ? 32 + ord - 1 : 8 + ord; win = o; }
                }
                if (LPC) s_win = win;
            }
            if constexpr (LPC) {
                __syncthreads();
                if (s_win >= 0 && tid < 128) s_kb[tid] = s_k[s_win][tid];
            }
        }
    }

    // 4. the decision and the frame header
    if (tid == 0) {
        int kind = 0, order = 0, porder = 0;
        uint32_t sub_bits = 8 + 16;
        if (s_diff) {
            if (best >= 8u + 16u * (uint32_t)n) { kind = 1; order = 0; porder = 0; sub_bits = 8u + 16u * (uint32_t)n; }
            else { kind = b_kind; order = b_order; porder = b_porder; sub_bits = best; }
        }
        uint32_t hb[16]; int hl = 0;
        const int bs_code = n == P.block_size ? P.bs_code : (n <= 256 ? 6 : 7);
        hb[hl++] = 0xFF; hb[hl++] = 0xF8; hb[hl++] = (uint32_t)(bs_code << 4 | P.sr_code); hb[hl++] = 4u << 1;
        const uint32_t v = (uint32_t)fr.index;
        if (v < 0x80u) hb[hl++] = v;
        else {
            const int nb = v < 0x800u ? 2 : v < 0x10000u ? 3 : v < 0x200000u ? 4 : v < 0x4000000u ? 5 : 6;
            hb[hl++] = ((0xFF00u >> nb) & 0xFFu) | (v >> (6 * (nb - 1)));
            for (int i = nb - 2; i >= 0; --i) hb[hl++] = 0x80u | ((v >> (6 * i)) & 0x3Fu);
        }
        if (bs_code == 6) hb[hl++] = (uint32_t)(n - 1);
        else if (bs_code == 7) { hb[hl++] = (uint32_t)(n - 1) >> 8; hb[hl++] = (uint32_t)(n - 1) & 0xFFu; }
        uint32_t c8 = 0;
        for (int i = 0; i < hl; ++i) {
            c8 ^= hb[i];
            for (int b = 0; b < 8; ++b) c8 = (c8 & 0x80u) ? ((c8 << 1) ^ 0x07u) & 0xFFu : (c8 << 1) & 0xFFu;
        }
        hb[hl++] = c8;
        for (int i = 0; i < hl; ++i) put_bits(s_buf, 8u * (uint32_t)i, hb[i], 8);
        put_bits(s_buf, 8u * (uint32_t)hl, (uint32_t)kind << 1, 8);
        s_dec[0] = kind; s_dec[1] = order; s_dec[2] = porder; s_dec[3] = 8 * hl; s_dec[4] = (int)sub_bits;
    }
    __syncthreads();
    const int kind = s_dec[0], order = s_dec[1], porder = s_dec[2], total_bits = s_dec[3] + s_dec[4];
    const uint32_t warm = (uint32_t)s_dec[3] + 8u;      // the first bit behind the subframe's header byte

    // 5. the subframe's body
    if (kind == 0) {
        if (tid == 0) put_bits(s_buf, warm, (uint32_t)x0 & 0xFFFFu, 16);
    } else if (kind == 1) {
        for (int i = tid; i < n; i += 256) put_bits(s_buf, warm + 16u * (uint32_t)i, (uint32_t)s_x[i] & 0xFFFFu, 16);
    } else {
        if (tid < order) put_bits(s_buf, warm + 16u * (uint32_t)tid, (uint32_t)s_x[tid] & 0xFFFFu, 16);
        uint32_t hb = warm + 16u * (uint32_t)order;
        const bool lpc = LPC && kind >= 32;
        const int q = Q.precision, lsh = lpc ? s_shift[order - 1] : 0;
        const int32_t* lc = &s_c[lpc ? (order - 1) * FL_LPC : 0];
        if (lpc) {      // the precision, the shift, the coefficients
            if (tid == 0) put_bits(s_buf, hb, (uint32_t)(q - 1) << 5 | (uint32_t)lsh, 9);
            if (tid < order) put_bits(s_buf, hb + 9u + (uint32_t)(q * tid), (uint32_t)lc[tid] & ((1u << q) - 1u), q);
            hb += 9u + (uint32_t)(q * order);
        }
        if (tid == 0) put_bits(s_buf, hb, (uint32_t)porder, 6);      // two zero bits (method 0), then the partition order
        const uint32_t rbase = hb + 6u;
        const int size = n >> porder;
        uint32_t running = 0;
        for (int c = 0, round = 0; c < n; c += 256, ++round) {
            const int i = c + tid;
            const bool active = i >= order && i < n;
            uint32_t u = 0, q = 0, len = 0; int k = 0; bool first = false;
            if (active) {
                const int j = i / size;
                k = LPC ? s_kb[(1 << porder) - 1 + j] : s_k[order][(1 << porder) - 1 + j];
                bool bad = false;
                u = zigzag(lpc ? lpc_resid(s_x, i, order, lc, lsh, &bad) : resid(s_x, i, order));
                q = u >> k;
                first = i == max(j * size, order);
                len = q + 1u + (uint32_t)k + (first ? 4u : 0u);
            }
            uint32_t inc = len;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t t = __shfl_up(inc, d, 64);
                if (lane >= d) inc += t;
            }
            if (lane == 63) s_scan[round & 1][wv] = inc;
            __syncthreads();
            uint32_t before = 0, all = 0;
#pragma unroll
            for (int w = 0; w < 4; ++w) { const uint32_t t = s_scan[round & 1][w]; all += t; if (w < wv) before += t; }
            if (active) {
                uint32_t pos = rbase + running + before + inc - len;
                if (pos + len <= (uint32_t)total_bits) {      // always: the decision counted these very bits; the buffer's bound does not rest on that
                    if (first) { put_bits(s_buf, pos, (uint32_t)k, 4); pos += 4u; }
                    put_bits(s_buf, pos + q, (1u << k) | (u & ((1u << k) - 1u)), k + 1);
                }
            }
            running += all;
        }
    }
    __syncthreads();

    // 6. CRC-16 over the frame's bytes
    const int nbytes = (total_bits + 7) >> 3;
    {
        const int R = (nbytes + 255) >> 8, pad = 256 * R - nbytes;
        uint32_t c = 0;
        for (int v = tid * R; v < (tid + 1) * R; ++v) {
            const int b = v - pad;
            if (b >= 0) c = ((c << 8) & 0xFFFFu) ^ s_tab[(c >> 8) ^ get_byte(s_buf, b)];
        }
        s_crc[tid] = c;
        uint32_t M = 1, sq = 0x0100u;      // M = x^(8 R)
        for (int e = R; e; e >>= 1) { if (e & 1) M = gf_mul16(M, sq); sq = gf_mul16(sq, sq); }
        for (int s = 1; s < 256; s <<= 1) {
            __syncthreads();
            if ((tid & (2 * s - 1)) == 0) s_crc[tid] = gf_mul16(s_crc[tid], M) ^ s_crc[tid + s];
            M = gf_mul16(M, M);
        }
        if (tid == 0) {
            put_bits(s_buf, 8u * (uint32_t)nbytes, s_crc[0], 16);
            P.sizes[blockIdx.x] = nbytes + 2;
            P.desc[blockIdx.x] = (uint32_t)kind | ((uint32_t)porder << 8);
        }
    }
    __syncthreads();

    // 7. the frame to its slot, in byte order
    uint32_t* slot = reinterpret_cast<uint32_t*>(P.scratch + (size_t)blockIdx.x * (size_t)P.stride);
    for (int w = tid; w < (nbytes + 2 + 3) >> 2; w += 256) slot[w] = __builtin_bswap32(s_buf[w]);
}

namespace {

// n bytes from the 4-byte aligned src to dst of any alignment
__device__ inline void copy_bytes(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int n, int tid) {
    const int head = min((int)((4u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 3u)) & 3u), n);
    if (tid < head) dst[tid] = src[tid];
    const int words = (n - head) >> 2;
    const uint32_t* s32 = reinterpret_cast<const uint32_t*>(src);
    uint32_t* d32 = reinterpret_cast<uint32_t*>(dst + head);
    if (head == 0) {
        for (int w = tid; w < words; w += 256) d32[w] = s32[w];
    } else {
        const int lo = 8 * head, hi = 32 - lo;
        for (int w = tid; w < words; w += 256) d32[w] = (s32[w] >> lo) | (s32[w + 1] << hi);
    }
    const int done = head + 4 * words;
    if (tid < n - done) dst[done + tid] = src[done + tid];
}

}  // namespace

__global__ __launch_bounds__(256) void flac_gather_kernel(const uint8_t* __restrict__ scratch, int stride, const FlacFrame* __restrict__ frames,
                                                           const int32_t* __restrict__ sizes, const int64_t* __restrict__ frame_offs,
                                                           const uint8_t* __restrict__ headers, uint8_t* __restrict__ out) {
    const int tid = threadIdx.x;
    const FlacFrame fr = frames[blockIdx.x];
    uint8_t* dst = out + frame_offs[blockIdx.x];
    copy_bytes(dst, scratch + (size_t)blockIdx.x * (size_t)stride, sizes[blockIdx.x], tid);
    if (fr.index == 0) copy_bytes(dst - FLAC_STREAM_HEADER, headers + (size_t)fr.seg * FLAC_HEADER_STRIDE, FLAC_STREAM_HEADER, tid);
}

__global__ __launch_bounds__(256) void flac_lpc_analysis_kernel(FlacParams P, FlacLpc Q, int64_t* __restrict__ R, int32_t* __restrict__ shift,
                                                                int32_t* __restrict__ coef) {
    __shared__ int32_t s_x[FLAC_MAX_BLOCK];
    __shared__ int16_t s_y[FLAC_MAX_BLOCK];
    __shared__ unsigned long long s_R[13];
    __shared__ int32_t s_c[FL_LPC * FL_LPC];
    __shared__ int s_shift[FL_LPC];
    const int tid = threadIdx.x;
    const FlacFrame fr = P.frames[blockIdx.x];
    for (int i = tid; i < fr.n; i += 256) s_x[i] = load_pcm(P, fr.src + i);
    __syncthreads();
    lpc_analyse(s_x, fr.n, Q.max_order, Q.precision, s_y, s_R, s_c, s_shift);
    if (tid < 13) R[(size_t)blockIdx.x * 13 + tid] = (int64_t)s_R[tid];
    if (tid < FL_LPC) shift[(size_t)blockIdx.x * FL_LPC + tid] = s_shift[tid];
    if (tid < FL_LPC * FL_LPC) coef[(size_t)blockIdx.x * (FL_LPC * FL_LPC) + tid] = s_c[tid];
}

namespace {

__device__ inline uint32_t rotl32(uint32_t v, int s) { return (v << s) | (v >> (32 - s)); }

// one 64-byte round of RFC 1321 on the words w[0 .. 16)
__device__ inline void md5_round(uint32_t st[4], const uint32_t* w) {
    constexpr uint32_t K[64] = {
        0xd76aa478u, 0xe8c7b756u, 0x242070dbu, 0xc1bdceeeu, 0xf57c0fafu, 0x4787c62au, 0xa8304613u, 0xfd469501u, 0x698098d8u, 0x8b44f7afu, 0xffff5bb1u,
        0x895cd7beu, 0x6b901122u, 0xfd987193u, 0xa679438eu, 0x49b40821u, 0xf61e2562u, 0xc040b340u, 0x265e5a51u, 0xe9b6c7aau, 0xd62f105du, 0x02441453u,
        0xd8a1e681u, 0xe7d3fbc8u, 0x21e1cde6u, 0xc33707d6u, 0xf4d50d87u, 0x455a14edu, 0xa9e3e905u, 0xfcefa3f8u, 0x676f02d9u, 0x8d2a4c8au, 0xfffa3942u,
        0x8771f681u, 0x6d9d6122u, 0xfde5380cu, 0xa4beea44u, 0x4bdecfa9u, 0xf6bb4b60u, 0xbebfbc70u, 0x289b7ec6u, 0xeaa127fau, 0xd4ef3085u, 0x04881d05u,
        0xd9d4d039u, 0xe6db99e5u, 0x1fa27cf8u, 0xc4ac5665u, 0xf4292244u, 0x432aff97u, 0xab9423a7u, 0xfc93a039u, 0x655b59c3u, 0x8f0ccc92u, 0xffeff47du,
        0x85845dd1u, 0x6fa87e4fu, 0xfe2ce6e0u, 0xa3014314u, 0x4e0811a1u, 0xf7537e82u, 0xbd3af235u, 0x2ad7d2bbu, 0xeb86d391u};
    constexpr int S[16] = {7, 12, 17, 22, 5, 9, 14, 20, 4, 11, 16, 23, 6, 10, 15, 21};
    uint32_t a = st[0], b = st[1], c = st[2], d = st[3];
#pragma unroll
    for (int i = 0; i < 64; ++i) {
        uint32_t f; int g;
        if (i < 16) { f = (b & c) | (~b & d); g = i; }
        else if (i < 32) { f = (d & b) | (~d & c); g = (5 * i + 1) & 15; }
        else if (i < 48) { f = b ^ c ^ d; g = (3 * i + 5) & 15; }
        else { f = c ^ (b | ~d); g = (7 * i) & 15; }
        f += a + K[i] + w[g];
        a = d; d = c; c = b;
        b += rotl32(f, S[(i >> 4) * 4 + (i & 3)]);
    }
    st[0] += a; st[1] += b; st[2] += c; st[3] += d;
}

// word W of the padded message of n little-endian 16-bit samples in `blocks` 64-byte rounds: samples, the byte 0x80, zeros, the length in bits
__device__ inline uint32_t md5_word(const FlacParams& P, int64_t src, int64_t n, int64_t blocks, int64_t W) {
    if (W == 16 * blocks - 2) return (uint32_t)((uint64_t)n * 16u);
    if (W == 16 * blocks - 1) return (uint32_t)(((uint64_t)n * 16u) >> 32);
    const int64_t s0 = 2 * W, s1 = 2 * W + 1;
    const uint32_t lo = s0 < n ? (uint32_t)load_pcm(P, src + s0) & 0xFFFFu : s0 == n ? 0x80u : 0u;
    const uint32_t hi = s1 < n ? (uint32_t)load_pcm(P, src + s1) & 0xFFFFu : s1 == n ? 0x80u : 0u;
    return lo | hi << 16;
}

}  // namespace

__global__ __launch_bounds__(64) void flac_md5_kernel(FlacParams P, const FlacMd5Seg* __restrict__ segs, uint32_t* __restrict__ digests) {
    __shared__ uint32_t s_w[2][64 * 16];
    const int lane = threadIdx.x;
    const FlacMd5Seg sg = segs[blockIdx.x];
    const int64_t blocks = (2 * sg.n + 8) / 64 + 1, words = 16 * blocks, chunks = (blocks + 63) / 64;
    uint32_t reg[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        const int64_t W = (int64_t)t * 64 + lane;
        s_w[0][t * 64 + lane] = W < words ? md5_word(P, sg.src, sg.n, blocks, W) : 0u;
    }
    __syncthreads();
    uint32_t st[4] = {0x67452301u, 0xefcdab89u, 0x98badcfeu, 0x10325476u};
    for (int64_t c = 0; c < chunks; ++c) {
        const bool more = c + 1 < chunks;
        if (more) {
#pragma unroll
            for (int t = 0; t < 16; ++t) {
                const int64_t W = (c + 1) * 1024 + (int64_t)t * 64 + lane;
                reg[t] = W < words ? md5_word(P, sg.src, sg.n, blocks, W) : 0u;
            }
        }
        const uint32_t* buf = s_w[c & 1];
        const int nb = (int)min((int64_t)64, blocks - 64 * c);
        for (int b = 0; b < nb; ++b) md5_round(st, buf + 16 * b);
        if (more) {
#pragma unroll
            for (int t = 0; t < 16; ++t) s_w[(c + 1) & 1][t * 64 + lane] = reg[t];
        }
        __syncthreads();
    }
    if (lane < 4) digests[(size_t)blockIdx.x * 4 + lane] = lane == 0 ? st[0] : lane == 1 ? st[1] : lane == 2 ? st[2] : st[3];
}

static bool flac_params_ok(const FlacParams& p, int64_t n_frames) {
    return !(n_frames < 1 || n_frames > INT_MAX || p.block_size > FLAC_MAX_BLOCK || p.stride < 2 * p.block_size + 24 || (p.stride & 3));
}
static bool flac_lpc_ok(const FlacLpc& q) { return q.max_order >= 0 && q.max_order <= FLAC_LPC_MAX_ORDER && q.precision >= 5 && q.precision <= 15; }

int launch_flac_encode(const FlacParams& p, int64_t n_frames, hipStream_t s) {
    if (!flac_params_ok(p, n_frames)) return -1;
    hipLaunchKernelGGL(flac_encode_kernel<false>, dim3((unsigned)n_frames), dim3(256), 0, s, p, FlacLpc{0, 12});
    return 0;
}

int launch_flac_encode_lpc(const FlacParams& p, const FlacLpc& q, int64_t n_frames, hipStream_t s) {
    if (!flac_params_ok(p, n_frames) || !flac_lpc_ok(q)) return -1;
    hipLaunchKernelGGL(flac_encode_kernel<true>, dim3((unsigned)n_frames), dim3(256), 0, s, p, q);
    return 0;
}

int launch_flac_lpc_analysis(const FlacParams& p, const FlacLpc& q, int64_t n_frames, int64_t* R, int32_t* shift, int32_t* coef, hipStream_t s) {
    if (n_frames < 1 || n_frames > INT_MAX || p.block_size > FLAC_MAX_BLOCK || !flac_lpc_ok(q)) return -1;
    hipLaunchKernelGGL(flac_lpc_analysis_kernel, dim3((unsigned)n_frames), dim3(256), 0, s, p, q, R, shift, coef);
    return 0;
}

void launch_flac_md5(const FlacParams& p, const FlacMd5Seg* segs, int B, uint32_t* digests, hipStream_t s) {
    hipLaunchKernelGGL(flac_md5_kernel, dim3((unsigned)B), dim3(64), 0, s, p, segs, digests);
}

void launch_flac_gather(const uint8_t* scratch, int stride, const FlacFrame* frames, int64_t n_frames, const int32_t* sizes, const int64_t* frame_offs,
                        const uint8_t* headers, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(flac_gather_kernel, dim3((unsigned)n_frames), dim3(256), 0, s, scratch, stride, frames, sizes, frame_offs, headers, out);
}

}  // namespace ev
