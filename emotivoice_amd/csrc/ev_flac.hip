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

__global__ __launch_bounds__(256) void flac_encode_kernel(FlacParams P) {
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

    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const FlacFrame fr = P.frames[blockIdx.x];
    const int n = fr.n;

    // 1. samples, tables, zeroed buffers
    int32_t x0;
    if (P.pcm_is_i16) x0 = reinterpret_cast<const int16_t*>(P.pcm)[fr.src];
    else x0 = to_pcm(reinterpret_cast<const float*>(P.pcm)[fr.src], P.convert);
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
        int32_t v;
        if (P.pcm_is_i16) v = reinterpret_cast<const int16_t*>(P.pcm)[fr.src + i];
        else v = to_pcm(reinterpret_cast<const float*>(P.pcm)[fr.src + i], P.convert);
        s_x[i] = v;
        differs |= v != x0;
    }
    if (differs) s_diff = 1;
    __syncthreads();

    const int mo = min(P.max_fixed_order, n - 1);
    const int pmax = min(P.max_partition_order, __ffs(n) - 1);
    if (s_diff) {      // the same value in every thread
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
                    if (o <= mo && i >= o) {
                        const uint32_t u = zigzag(resid(s_x, i, o));
#pragma unroll
                        for (int k = 0; k < 15; ++k) acc[o][k] += min(u >> k, FL_CLAMP);
                    }
                }
            }
            const int width = min(T, 64);
#pragma unroll
            for (int o = 0; o < 5; ++o) {
                if (o > mo) continue;
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
            for (int idx = tid; idx < ((mo + 1) << p); idx += 256) {
                const int o = idx >> p, j = idx & ((1 << p) - 1);
                if (size <= o) continue;
                const uint32_t cnt = (uint32_t)(size - (j == 0 ? o : 0));
                uint32_t best = 0xFFFFFFFFu; int bk = 0;
                for (int k = 0; k < 15; ++k) {
                    const uint32_t c = (uint32_t)(k + 1) * cnt + s_sum[(o * 15 + k) * 64 + (j << sh)];
                    if (c < best) { best = c; bk = k; }
                }
                s_k[o][(1 << p) - 1 + j] = (uint8_t)bk;
                atomicAdd(&s_cost[o][p], 4u + best);
            }
            __syncthreads();
            if (p > 0) {
                const int half = 1 << (p - 1);
                for (int idx = tid; idx < (mo + 1) * 15 * half; idx += 256) {
                    const int ok = idx >> (p - 1), j = idx & (half - 1);
                    uint32_t* cell = &s_sum[ok * 64 + ((2 * j) << sh)];
                    cell[0] += cell[1 << sh];
                }
                __syncthreads();
            }
        }
    }

    // 4. the decision and the frame header
    if (tid == 0) {
        int kind = 0, order = 0, porder = 0;
        uint32_t sub_bits = 8 + 16;
        if (s_diff) {
            uint32_t best = 0xFFFFFFFFu;
            for (int o = 0; o <= mo; ++o) {
                uint32_t bc = 0xFFFFFFFFu; int bp = 0;
                for (int p = 0; p <= pmax; ++p) {
                    if ((n >> p) <= o) continue;
                    const uint32_t c = 4u + s_cost[o][p];
                    if (c < bc) { bc = c; bp = p; }
                }
                const uint32_t bits = 8u + 16u * (uint32_t)o + 2u + bc;
                if (bits < best) { best = bits; order = o; porder = bp; }
            }
            if (best >= 8u + 16u * (uint32_t)n) { kind = 1; order = 0; porder = 0; sub_bits = 8u + 16u * (uint32_t)n; }
            else { kind = 8 + order; sub_bits = best; }
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
        if (tid == 0) put_bits(s_buf, warm + 16u * (uint32_t)order, (uint32_t)porder, 6);      // two zero bits (method 0), then the partition order
        const uint32_t rbase = warm + 16u * (uint32_t)order + 6u;
        const int size = n >> porder;
        uint32_t running = 0;
        for (int c = 0, round = 0; c < n; c += 256, ++round) {
            const int i = c + tid;
            const bool active = i >= order && i < n;
            uint32_t u = 0, q = 0, len = 0; int k = 0; bool first = false;
            if (active) {
                const int j = i / size;
                k = s_k[order][(1 << porder) - 1 + j];
                u = zigzag(resid(s_x, i, order));
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

int launch_flac_encode(const FlacParams& p, int64_t n_frames, hipStream_t s) {
    if (n_frames < 1 || n_frames > INT_MAX || p.block_size > FLAC_MAX_BLOCK || p.stride < 2 * p.block_size + 24 || (p.stride & 3)) return -1;
    hipLaunchKernelGGL(flac_encode_kernel, dim3((unsigned)n_frames), dim3(256), 0, s, p);
    return 0;
}

void launch_flac_gather(const uint8_t* scratch, int stride, const FlacFrame* frames, int64_t n_frames, const int32_t* sizes, const int64_t* frame_offs,
                        const uint8_t* headers, uint8_t* out, hipStream_t s) {
    hipLaunchKernelGGL(flac_gather_kernel, dim3((unsigned)n_frames), dim3(256), 0, s, scratch, stride, frames, sizes, frame_offs, headers, out);
}

}  // namespace ev
