// Stand-alone check of the batch layouts of the audio utilities (emotivoice_amd/csrc/ev_layout.h), built and run by tests/test_layout.py with the
// host sanitizers.  No HIP runtime call, no library: it includes the pure builders and holds them to invariants it works out itself --
// offsets are the prefix sums of the lengths, counts follow the documented formulas, and the pieces of every sequence cover [0, n) exactly once, in
// order.  Exit status 0 and "layout_check: N checks" on success; the first failed check is printed and ends the run with status 1.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "../emotivoice_amd/csrc/ev_layout.h"

using namespace evh;

static long g_checks = 0;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        ++g_checks;                                                                          \
        if (!(cond)) { printf("layout_check: %s:%d: %s\n", __FILE__, __LINE__, #cond); exit(1); } \
    } while (0)

typedef std::vector<int64_t> Lens;

// every batch a case is run on: each of the four lengths alone (B = 1), and the first and the last three together (B = 3)
static std::vector<Lens> batches(const Lens& lens) {
    std::vector<Lens> out;
    for (int64_t n : lens) out.push_back(Lens{n});
    out.push_back(Lens(lens.begin(), lens.begin() + 3));
    out.push_back(Lens(lens.begin() + 1, lens.end()));
    return out;
}

// ---------------------------------------------------------------- frame grids (ev_features: tile 64; ev_pitch: EV_PITCH_TILE_FRAMES)
static void check_frame_grid(const Lens& lens, int64_t min_len, int hop, int tile) {
    const int B = (int)lens.size();
    FrameGrid g;
    CHECK(frame_grid_layout(B, lens.data(), min_len, hop, tile, g) == 0);
    CHECK((int)g.seqs.size() == B && (int)g.lens.size() == B && (int)g.offs.size() == B + 1);
    int64_t wo = 0, fo = 0;
    size_t k = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t T = lens[b] / hop + 1;
        CHECK(g.seqs[b].wav_off == wo && g.seqs[b].len == lens[b] && g.seqs[b].frm_off == fo && g.seqs[b].frames == T && g.seqs[b].reserved == 0);
        CHECK(g.lens[b] == T && g.offs[b] == fo);
        int64_t covered = 0;      // the tiles of utterance b, in order, each starting where the last one ended
        while (k < g.tiles.size() && g.tiles[k].seq == b) {
            CHECK(g.tiles[k].t0 == covered);
            covered += tile;
            ++k;
        }
        CHECK(covered >= T && covered - tile < T);      // the last tile holds frame T - 1 and no tile starts past it
        wo += lens[b]; fo += T;
    }
    CHECK(k == g.tiles.size() && g.offs[B] == fo);
}
static void frame_grid_cases(int64_t min_len, int hop, int tile) {
    const Lens at_tile = {(int64_t)(tile - 2) * hop + hop - 1, (int64_t)(tile - 1) * hop, (int64_t)tile * hop, min_len};      // T = tile - 1, tile, tile + 1; the shortest
    for (const Lens& l : batches(at_tile)) check_frame_grid(l, min_len, hop, tile);
    check_frame_grid(Lens{(int64_t)EV_ALIGN_MAX_FRAMES * hop - 1}, min_len, hop, tile);      // T = EV_ALIGN_MAX_FRAMES: the longest
    FrameGrid g;
    const Lens too_short = {at_tile[0], min_len - 1, at_tile[1]}, too_long = {at_tile[0], at_tile[1], (int64_t)EV_ALIGN_MAX_FRAMES * hop};
    CHECK(frame_grid_layout(3, too_short.data(), min_len, hop, tile, g) == 2);       // index 1, + 1
    CHECK(frame_grid_layout(3, too_long.data(), min_len, hop, tile, g) == -3);       // index 2: -(2 + 1)
    CHECK(frame_grid_layout(1, too_short.data() + 1, min_len, hop, tile, g) == 1);
    CHECK(frame_grid_layout(1, too_long.data() + 2, min_len, hop, tile, g) == -1);
}

// ---------------------------------------------------------------- ev_resample: n = ceil(len up / down) outputs, tiles of EV_RESAMPLE_TILE
static void check_resample(const Lens& lens, int up, int down) {
    const int B = (int)lens.size();
    std::vector<ev::ResampleSeq> seqs; std::vector<ev::ResampleTile> tiles;
    CHECK(resample_layout(B, lens.data(), up, down, 0, seqs, tiles) == 0);
    CHECK((int)seqs.size() == B);
    int64_t io = 0, oo = 0;
    size_t k = 0;
    for (int b = 0; b < B; ++b) {
        int64_t n = lens[b] * up / down;
        if (n * down < lens[b] * up) ++n;      // the ceiling, without the rounding trick of the code under test
        CHECK(seqs[b].in_off == io && seqs[b].len == lens[b] && seqs[b].out_off == oo && seqs[b].n == n);
        int64_t covered = 0;
        while (k < tiles.size() && tiles[k].seq == b) {
            CHECK(tiles[k].m0 == covered);
            covered += EV_RESAMPLE_TILE;
            ++k;
        }
        CHECK(covered >= n && covered - EV_RESAMPLE_TILE < n);
        io += lens[b]; oo += n;
    }
    CHECK(k == tiles.size());
}
static void resample_cases() {
    const int T = EV_RESAMPLE_TILE;
    for (const Lens& l : batches(Lens{T - 1, T, T + 1, 1})) check_resample(l, 1, 1);              // n = len
    for (const Lens& l : batches(Lens{2 * T - 2, 2 * T, 2 * T + 2, 1})) check_resample(l, 1, 2);  // n = T - 1, T, T + 1; and 1
    for (const Lens& l : batches(Lens{170, 171, 341, 1})) check_resample(l, 3, 2);                // n = 255, 257, 512; and 2
    const int64_t max_out = (int64_t)EV_ALIGN_MAX_FRAMES * 256;
    check_resample(Lens{max_out}, 1, 1);                                                          // the longest
    std::vector<ev::ResampleSeq> seqs; std::vector<ev::ResampleTile> tiles;
    const Lens too_short = {5, 0, 5}, too_long = {5, 5, max_out + 1}, with_extra = {max_out - 7};
    CHECK(resample_layout(3, too_short.data(), 1, 1, 0, seqs, tiles) == 2);
    CHECK(resample_layout(3, too_long.data(), 1, 1, 0, seqs, tiles) == -3);
    CHECK(resample_layout(1, with_extra.data(), 1, 1, 7, seqs, tiles) == 0);       // n + extra == the limit
    CHECK(resample_layout(1, with_extra.data(), 1, 1, 8, seqs, tiles) == -1);      // one more
    CHECK(resample_layout(1, with_extra.data(), 2, 1, 0, seqs, tiles) == -1);      // twice as many outputs
}

// ---------------------------------------------------------------- ev_flac: frames of block_size samples
static void check_flac(const Lens& lens, int N) {
    const int B = (int)lens.size();
    FlacPlan p;
    int at = -1;
    CHECK(flac_plan(B, lens.data(), N, p, &at) == LEN_OK);
    CHECK((int)p.stream_frames.size() == B);
    int64_t off = 0, cap = 0;
    size_t k = 0;
    for (int b = 0; b < B; ++b) {
        int64_t covered = 0, count = 0;
        while (k < p.frames.size() && p.frames[k].seg == b) {
            const ev::FlacFrame& f = p.frames[k];
            CHECK(f.src == off + covered && f.index == count && f.n >= 1 && f.n <= N && f.pad == 0);
            CHECK(f.n == N || covered + f.n == lens[b]);      // only a stream's last frame is short
            cap += 2 * (int64_t)f.n + 15;                     // a verbatim frame: 16 bits per sample, and the frame's header and CRC
            covered += f.n; ++count; ++k;
        }
        CHECK(covered == lens[b] && p.stream_frames[b] == count);
        cap += 42;                                            // "fLaC" and the STREAMINFO block
        off += lens[b];
    }
    CHECK(k == p.frames.size() && p.total == off && p.cap == cap);
}
static void flac_cases() {
    const int blocks[2] = {256, 4096};
    for (int N : blocks)
        for (const Lens& l : batches(Lens{N - 1, N, N + 1, 1})) check_flac(l, N);
    check_flac(Lens{EV_FLAC_MAX_SAMPLES}, 4096);                                  // the longest
    FlacPlan p;
    int at = -1;
    const Lens too_short = {5, 0, 5}, too_long = {5, 5, (int64_t)EV_FLAC_MAX_SAMPLES + 1};
    CHECK(flac_plan(3, too_short.data(), 4096, p, &at) == LEN_SHORT && at == 1);
    CHECK(flac_plan(3, too_long.data(), 4096, p, &at) == LEN_LONG && at == 2);
    // the config: the first bad field in the header's order, and the frame header's codes of the FLAC format (16 kHz: 0101, 4096 samples: 1100)
    ev_flac_config c{};
    c.struct_size = sizeof c; c.sample_rate = 16000; c.block_size = 4096; c.max_fixed_order = 4; c.max_partition_order = 5; c.convert = EV_FLAC_WRAP;
    int sr = 0, bs = 0;
    CHECK(flac_check_config(c, &sr, &bs) == FLAC_OK && sr == 5 && bs == 12);
    ev_flac_config bad = c;
    bad.convert = 2; CHECK(flac_check_config(bad, &sr, &bs) == FLAC_BAD_CONVERT);
    bad.max_partition_order = 7; CHECK(flac_check_config(bad, &sr, &bs) == FLAC_BAD_PARTITION_ORDER);
    bad.max_fixed_order = 5; CHECK(flac_check_config(bad, &sr, &bs) == FLAC_BAD_FIXED_ORDER);
    bad.block_size = 4095; CHECK(flac_check_config(bad, &sr, &bs) == FLAC_BAD_BLOCK);
    bad.sample_rate = 16001; CHECK(flac_check_config(bad, &sr, &bs) == FLAC_BAD_RATE);
}

// ---------------------------------------------------------------- ev_loudness: tiles of EV_LOUDNESS_TILE samples, gating blocks of 4 steps
static void check_loudness(const Lens& lens, int64_t step) {
    const int B = (int)lens.size();
    LoudPlan p;
    int at = -1;
    CHECK(loudness_plan(B, lens.data(), step, p, &at) == LEN_OK);
    CHECK((int)p.segs.size() == B && (int)p.offs.size() == B + 1 && p.offs[0] == 0);
    int64_t off = 0, blocks = 0;
    size_t k = 0;
    for (int b = 0; b < B; ++b) {
        CHECK(p.segs[b].tile0 == (int64_t)k);
        int64_t covered = 0;
        while (k < p.tiles.size() && p.tiles[k].seg == b) {
            const ev::LoudTile& t = p.tiles[k];
            CHECK(t.src == off + covered && t.pos == covered && t.n >= 1 && t.n <= EV_LOUDNESS_TILE);
            CHECK(t.n == EV_LOUDNESS_TILE || covered + t.n == lens[b]);
            covered += t.n; ++k;
        }
        CHECK(covered == lens[b] && p.segs[b].ntiles == (int64_t)k - p.segs[b].tile0);
        int64_t fit = 0;      // the 4-step blocks, one per step, that lie inside the segment; a shorter segment is one block
        while ((fit + 4) * step <= lens[b]) ++fit;
        blocks += fit ? fit : 1;
        off += lens[b];
        CHECK(p.offs[b + 1] == off);
    }
    CHECK(k == p.tiles.size() && p.total == off && p.n_blocks == blocks);
}
static void loudness_cases() {
    const int T = EV_LOUDNESS_TILE;
    for (const Lens& l : batches(Lens{T - 1, T, T + 1, 1})) check_loudness(l, 1600);
    for (const Lens& l : batches(Lens{4 * 800 - 1, 4 * 800, 5 * 800, 1})) check_loudness(l, 800);      // below one block, exactly one, two
    check_loudness(Lens{EV_LOUDNESS_MAX_SAMPLES}, 4800);                          // the longest
    LoudPlan p;
    int at = -1;
    const Lens too_short = {5, 0, 5}, too_long = {5, 5, (int64_t)EV_LOUDNESS_MAX_SAMPLES + 1};
    CHECK(loudness_plan(3, too_short.data(), 1600, p, &at) == LEN_SHORT && at == 1);
    CHECK(loudness_plan(3, too_long.data(), 1600, p, &at) == LEN_LONG && at == 2);
}

int main() {
    frame_grid_cases(1024 / 2 + 1, 256, 64);               // ev_features at its default config
    frame_grid_cases(128 / 2 + 1, 8, 64);                  // ... and at its smallest n_fft and hop
    frame_grid_cases(1, 256, EV_PITCH_TILE_FRAMES);        // ev_pitch
    frame_grid_cases(1, 1, EV_PITCH_TILE_FRAMES);
    resample_cases();
    flac_cases();
    loudness_cases();
    printf("layout_check: %ld checks\n", g_checks);
    return 0;
}
