// libevhip.so host side, internal (not installed): the batch layouts of the audio utilities -- per-utterance offsets and the tile tables their kernels
// index by block.  Pure functions of host arrays: no HIP call and no handle, so a plain program can check them (tests/layout_check.cpp).
#pragma once
#include <limits.h>
#include <stdint.h>

#include <algorithm>
#include <vector>

#include "../../include/evhip.h"
#include "ev_kernels.h"

namespace evh __attribute__((visibility("hidden"))) {

// ---------------------------------------------------------------- frames of hop samples, tiles of tile_frames frames (ev_features, ev_pitch)
struct FrameGrid { std::vector<ev::StftSeq> seqs; std::vector<ev::StftTile> tiles; std::vector<int32_t> lens; std::vector<int64_t> offs; };
// frame counts T = len / hop + 1, their offsets (B + 1) and the tile table of a batch; 0 or the index + 1 of the first utterance shorter than min_len
// (-(index + 1): more than EV_ALIGN_MAX_FRAMES frames)
inline int frame_grid_layout(int B, const int64_t* wav_lens, int64_t min_len, int hop, int tile_frames, FrameGrid& g) {
    g.seqs.resize(B); g.lens.resize(B); g.offs.resize((size_t)B + 1); g.tiles.clear();
    int64_t wo = 0, fo = 0;
    for (int b = 0; b < B; ++b) {
        if (wav_lens[b] < min_len) return b + 1;
        const int64_t T = wav_lens[b] / hop + 1;
        if (T > EV_ALIGN_MAX_FRAMES) return -(b + 1);
        g.seqs[b] = ev::StftSeq{wo, wav_lens[b], fo, (int32_t)T, 0};
        g.lens[b] = (int32_t)T; g.offs[b] = fo;
        for (int t0 = 0; t0 < T; t0 += tile_frames) g.tiles.push_back(ev::StftTile{b, t0});
        wo += wav_lens[b]; fo += T;
    }
    g.offs[B] = fo;
    return 0;
}

// ---------------------------------------------------------------- chunks of hop output samples, tiles of DN_TJ chunks (ev_denoise's inverse)
// Utterance b has frames[b] = T frames at consecutive rows of the scratch and hop (T - 1) output samples: the untrimmed samples n_fft / 2 ..
// n_fft / 2 + hop (T - 1), which lie in chunks (n_fft / 2) / hop .. (n_fft / 2 + hop (T - 1) - 1) / hop.  An utterance of one frame has no output
// and no tile.  Returns the total of output samples.
inline int64_t istft_layout(int B, const int32_t* frames, int n_fft, int hop, std::vector<ev::IstftSeq>& seqs, std::vector<ev::StftTile>& tiles) {
    seqs.resize(B); tiles.clear();
    int64_t fo = 0, oo = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = (int64_t)hop * (frames[b] - 1);
        seqs[b] = ev::IstftSeq{fo, oo, n, frames[b], 0};
        if (n > 0)
            for (int64_t j = (n_fft / 2) / hop; j <= (n_fft / 2 + n - 1) / hop; j += ev::DN_TJ) tiles.push_back(ev::StftTile{b, (int32_t)j});
        fo += frames[b]; oo += n;
    }
    return oo;
}

// ---------------------------------------------------------------- outputs n = ceil(len up / down), tiles of RS_TM outputs (ev_resample)
constexpr int64_t RS_MAX_OUT = (int64_t)EV_ALIGN_MAX_FRAMES * 256;
// output lengths, offsets and the tile table of a batch; 0 or the index + 1 of the first empty utterance (-(index + 1): too long with `extra` added)
inline int resample_layout(int B, const int64_t* wav_lens, int up, int down, int64_t extra, std::vector<ev::ResampleSeq>& seqs, std::vector<ev::ResampleTile>& tiles) {
    seqs.resize(B); tiles.clear();
    int64_t io = 0, oo = 0;
    for (int b = 0; b < B; ++b) {
        if (wav_lens[b] < 1) return b + 1;
        if (wav_lens[b] > RS_MAX_OUT * EV_RESAMPLE_MAX_RATIO) return -(b + 1);      // keeps L up inside int64
        const int64_t n = (wav_lens[b] * up + down - 1) / down;
        if (n + extra > RS_MAX_OUT) return -(b + 1);
        seqs[b] = ev::ResampleSeq{io, wav_lens[b], oo, n};
        for (int64_t m0 = 0; m0 < n; m0 += ev::RS_TM) tiles.push_back(ev::ResampleTile{b, (int32_t)m0});
        io += wav_lens[b]; oo += n;
    }
    return 0;
}

// ---------------------------------------------------------------- outputs n = ceil(len up / down) of es bytes, 16-byte slots, tiles of DL_TILE outputs (ev_deliver)
// the utterances' table (slots back to back, each rounded up to 16 bytes), the tile table and the total bytes; 0 or the index + 1 of the first empty
// utterance (-(index + 1): more than RS_MAX_OUT outputs, ev_resample's limit)
inline int deliver_layout(int B, const int64_t* lens, int up, int down, int es, const uint32_t* seeds, uint32_t seed, std::vector<ev::DeliverSeq>& seqs,
                          std::vector<ev::DeliverTile>& tiles, int64_t* total_bytes) {
    seqs.resize(B); tiles.clear();
    int64_t io = 0, bo = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) return b + 1;
        if (lens[b] > RS_MAX_OUT * EV_RESAMPLE_MAX_RATIO) return -(b + 1);      // keeps L up inside int64
        const int64_t n = (lens[b] * up + down - 1) / down;
        if (n > RS_MAX_OUT) return -(b + 1);
        const int64_t slot = (n * es + 15) / 16 * 16;
        seqs[b] = ev::DeliverSeq{io, lens[b], n, bo, slot, seeds ? seeds[b] : seed, (int32_t)tiles.size()};
        for (int64_t m0 = 0; m0 < n; m0 += ev::DL_TILE) tiles.push_back(ev::DeliverTile{b, (int32_t)m0});
        io += lens[b]; bo += slot;
    }
    *total_bytes = bo;
    return 0;
}

// what a table of fixed-size pieces rejects in a length: below 1, above the utility's limit, or more than INT_MAX pieces in the call so far
enum LenBad { LEN_OK = 0, LEN_SHORT, LEN_LONG, LEN_COUNT };

// ---------------------------------------------------------------- frames of block_size samples (ev_flac)
inline int flac_block_code(int block_size) {      // the frame header's code of N, or -1
    for (int i = 0; i < 5; ++i) if (block_size == 256 << i) return 8 + i;
    return -1;
}
inline int flac_rate_code(int sample_rate) {
    const int rates[7] = {8000, 16000, 22050, 24000, 32000, 44100, 48000};
    for (int i = 0; i < 7; ++i) if (sample_rate == rates[i]) return 4 + i;
    return -1;
}
inline int64_t flac_bound(int64_t n, int block_size) {      // the bytes a stream of n samples can take (ev_flac_bound, arguments already judged)
    const int64_t full = n / block_size, rest = n % block_size;
    return ev::FLAC_STREAM_HEADER + full * (2 * (int64_t)block_size + 15) + (rest ? 2 * rest + 15 : 0);
}
// the first field of a config that is out of range, in the order include/evhip.h lists them; gives the frame header's two codes
enum FlacBad { FLAC_OK = 0, FLAC_BAD_RATE, FLAC_BAD_BLOCK, FLAC_BAD_FIXED_ORDER, FLAC_BAD_PARTITION_ORDER, FLAC_BAD_CONVERT };
inline FlacBad flac_check_config(const ev_flac_config& c, int* sr_code, int* bs_code) {
    *sr_code = flac_rate_code(c.sample_rate); *bs_code = flac_block_code(c.block_size);
    if (*sr_code < 0) return FLAC_BAD_RATE;
    if (*bs_code < 0) return FLAC_BAD_BLOCK;
    if (c.max_fixed_order < 0 || c.max_fixed_order > 4) return FLAC_BAD_FIXED_ORDER;
    if (c.max_partition_order < 0 || c.max_partition_order > 6) return FLAC_BAD_PARTITION_ORDER;
    if (c.convert != EV_FLAC_WRAP && c.convert != EV_FLAC_CLAMP) return FLAC_BAD_CONVERT;
    return FLAC_OK;
}
struct FlacPlan { std::vector<ev::FlacFrame> frames; std::vector<int64_t> stream_frames; int64_t total = 0, cap = 0; };      // cap: the streams' bound in bytes
// the frame table of a batch; a rejected length leaves its index in *at (the table's size is judged before it is built)
inline LenBad flac_plan(int B, const int64_t* lens, int N, FlacPlan& p, int* at) {
    int64_t NF = 0;
    p.total = 0; p.cap = 0;
    for (int b = 0; b < B; ++b) {
        *at = b;
        if (lens[b] < 1) return LEN_SHORT;
        if (lens[b] > EV_FLAC_MAX_SAMPLES) return LEN_LONG;
        p.total += lens[b]; NF += (lens[b] + N - 1) / N; p.cap += flac_bound(lens[b], N);
        if (NF > INT_MAX) return LEN_COUNT;
    }
    p.frames.clear(); p.frames.reserve((size_t)NF);
    p.stream_frames.resize((size_t)B);
    for (int64_t b = 0, off = 0; b < B; off += lens[b], ++b) {
        p.stream_frames[(size_t)b] = (lens[b] + N - 1) / N;
        for (int64_t i = 0; i < lens[b]; i += N)
            p.frames.push_back(ev::FlacFrame{off + i, (int32_t)std::min<int64_t>(N, lens[b] - i), (int32_t)(i / N), (int32_t)b, 0});
    }
    return LEN_OK;
}

// ---------------------------------------------------------------- tiles of LOUD_TILE samples, blocks of 4 steps (ev_loudness)
struct LoudPlan { std::vector<ev::LoudTile> tiles; std::vector<ev::LoudSeg> segs; std::vector<int64_t> offs; int64_t total = 0, n_blocks = 0; };
// the tile table of a batch, its segments and offsets (B + 1), and the number of gating blocks (one per `step` once a segment holds 4 steps, else one)
inline LenBad loudness_plan(int B, const int64_t* lens, int64_t step, LoudPlan& p, int* at) {
    const int64_t block = 4 * step;
    int64_t NT = 0;
    p.total = 0; p.n_blocks = 0;
    for (int b = 0; b < B; ++b) {
        *at = b;
        if (lens[b] < 1) return LEN_SHORT;
        if (lens[b] > EV_LOUDNESS_MAX_SAMPLES) return LEN_LONG;
        p.total += lens[b]; NT += (lens[b] + ev::LOUD_TILE - 1) / ev::LOUD_TILE; p.n_blocks += lens[b] >= block ? (lens[b] - block) / step + 1 : 1;
        if (NT > INT_MAX || (p.total + 1023) / 1024 > INT_MAX) return LEN_COUNT;
    }
    p.tiles.clear(); p.tiles.reserve((size_t)NT);
    p.segs = std::vector<ev::LoudSeg>((size_t)B);
    p.offs.assign((size_t)B + 1, 0);
    for (int64_t b = 0, off = 0; b < B; off += lens[b], ++b) {
        p.segs[(size_t)b] = ev::LoudSeg{(int64_t)p.tiles.size(), (lens[b] + ev::LOUD_TILE - 1) / ev::LOUD_TILE};
        p.offs[(size_t)b + 1] = off + lens[b];
        for (int64_t i = 0; i < lens[b]; i += ev::LOUD_TILE)
            p.tiles.push_back(ev::LoudTile{off + i, i, (int32_t)std::min<int64_t>(ev::LOUD_TILE, lens[b] - i), (int32_t)b});
    }
    return LEN_OK;
}

// ---------------------------------------------------------------- tiles of LIMIT_TILE samples (ev_limit)
struct LimitPlan { std::vector<ev::LimitTile> tiles; std::vector<int64_t> tile0; int64_t total = 0; };      // tile0: (B + 1,), the segment's tiles are [tile0[b], tile0[b + 1])
inline LenBad limit_plan(int B, const int64_t* lens, LimitPlan& p, int* at) {
    int64_t NT = 0;
    p.total = 0;
    for (int b = 0; b < B; ++b) {
        *at = b;
        if (lens[b] < 1) return LEN_SHORT;
        if (lens[b] > EV_LIMIT_MAX_SAMPLES) return LEN_LONG;
        p.total += lens[b]; NT += (lens[b] + ev::LIMIT_TILE - 1) / ev::LIMIT_TILE;
        if (NT > INT_MAX) return LEN_COUNT;
    }
    p.tiles.clear(); p.tiles.reserve((size_t)NT);
    p.tile0.assign((size_t)B + 1, 0);
    for (int64_t b = 0, off = 0; b < B; off += lens[b], ++b) {
        for (int64_t i = 0; i < lens[b]; i += ev::LIMIT_TILE)
            p.tiles.push_back(ev::LimitTile{off + i, i, lens[b], (int32_t)std::min<int64_t>(ev::LIMIT_TILE, lens[b] - i), (int32_t)b});
        p.tile0[(size_t)b + 1] = (int64_t)p.tiles.size();
    }
    return LEN_OK;
}

// ---------------------------------------------------------------- frames of STRETCH_HOP outputs, tiles of STRETCH_OLA_FRAMES frames (ev_stretch)
// the first rule of include/evhip.h's step 1 that a pair of lengths breaks
enum StretchBad { STRETCH_OK = 0, STRETCH_IN_SHORT, STRETCH_OUT_SHORT, STRETCH_IN_LONG, STRETCH_OUT_LONG, STRETCH_RATIO, STRETCH_COUNT };
inline StretchBad stretch_check(int64_t len_in, int64_t len_out) {
    if (len_in < 1) return STRETCH_IN_SHORT;
    if (len_out < 1) return STRETCH_OUT_SHORT;
    if (len_in > EV_STRETCH_MAX_SAMPLES) return STRETCH_IN_LONG;
    if (len_out > EV_STRETCH_MAX_SAMPLES) return STRETCH_OUT_LONG;
    if (std::min(len_in, len_out) >= EV_STRETCH_FRAME && (len_in > 2 * len_out || len_out > 2 * len_in)) return STRETCH_RATIO;
    return STRETCH_OK;
}
struct StretchPlan {
    std::vector<ev::StretchSeg> segs; std::vector<ev::StretchTile> tiles; std::vector<int64_t> lens_out, offs, frame_offs; std::vector<int32_t> frames;
    int64_t total_in = 0, total_out = 0, total_frames = 0;
};
// the segment and tile tables of a batch; a rejected pair leaves its index in *at (the tile table's size is judged before it is built)
inline StretchBad stretch_plan(int B, const int64_t* lens, const int64_t* lens_out, StretchPlan& p, int* at) {
    int64_t NT = 0;
    for (int b = 0; b < B; ++b) {
        *at = b;
        const StretchBad bad = stretch_check(lens[b], lens_out[b]);
        if (bad != STRETCH_OK) return bad;
        const int64_t K = (lens_out[b] + ev::STRETCH_HOP - 1) / ev::STRETCH_HOP;
        NT += (K + ev::STRETCH_OLA_FRAMES - 1) / ev::STRETCH_OLA_FRAMES;
        if (NT > INT_MAX) return STRETCH_COUNT;
    }
    p.segs.resize((size_t)B); p.frames.resize((size_t)B); p.lens_out.assign(lens_out, lens_out + B);
    p.offs.assign((size_t)B + 1, 0); p.frame_offs.assign((size_t)B + 1, 0);
    p.tiles.clear(); p.tiles.reserve((size_t)NT);
    int64_t io = 0, oo = 0, fo = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t K = (lens_out[b] + ev::STRETCH_HOP - 1) / ev::STRETCH_HOP;
        p.segs[(size_t)b] = ev::StretchSeg{io, lens[b], oo, lens_out[b], fo, (int32_t)K, 0};
        p.frames[(size_t)b] = (int32_t)K;
        for (int64_t k0 = 0; k0 < K; k0 += ev::STRETCH_OLA_FRAMES) p.tiles.push_back(ev::StretchTile{b, (int32_t)k0});
        io += lens[b]; oo += lens_out[b]; fo += K;
        p.offs[(size_t)b + 1] = oo; p.frame_offs[(size_t)b + 1] = fo;
    }
    p.total_in = io; p.total_out = oo; p.total_frames = fo;
    return STRETCH_OK;
}

}  // namespace evh
