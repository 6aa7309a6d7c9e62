// libevhip.so host side, internal (not installed): the handle and what ev_engine.cpp, ev_audio.cpp and ev_ops.cpp share -- errors, the workspace
// arenas, the profiler and the scaffold of a utility call.  Everything declared here is defined once, in ev_engine.cpp.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>
#include <string.h>

#include <map>
#include <string>
#include <utility>
#include <vector>

#include "../../include/evhip.h"
#include "../../include/evhip_ops.h"
#include "ev_kernels.h"
#include "ev_layout.h"

namespace evh __attribute__((visibility("hidden"))) {      // internal: no name of it leaves the library

constexpr int ROW_ALIGN = 256;    // row counts are padded to the largest GEMM M tile
constexpr int PAD_ROWS = 64;      // readable slack rows before / after every activation buffer
constexpr size_t PIN_MAX_B = 1 << 16;                // utterances per call the pinned staging area is laid out for

// One workspace per phase or utility; a utility's results live in its arena until its next call.
enum Arena {
    ARENA_TOKEN,       // token-rate phase
    ARENA_FRAME,       // frame-rate phase + vocoder
    ARENA_BERT,        // SimBERT
    ARENA_ALIGN,       // ev_align (its results live here until the next ev_align)
    ARENA_FEATURES,    // ev_features (likewise)
    ARENA_PITCH,       // ev_pitch (likewise)
    ARENA_RESAMPLE,    // ev_resample (likewise)
    ARENA_STITCH,      // ev_stitch (likewise)
    ARENA_COMPARE,     // ev_compare (scratch only: its result is host memory)
    ARENA_FLAC,        // ev_flac (like ARENA_ALIGN)
    ARENA_LOUDNESS,    // ev_loudness (likewise)
    ARENA_LIMIT,       // ev_limit (likewise)
    ARENA_DELIVER,     // ev_deliver (likewise)
    ARENA_SCORE_A,     // ev_score_load(0): the side's integer cepstra and F0 track, until the side is replaced
    ARENA_SCORE_B,     // ev_score_load(1) (likewise)
    ARENA_SCORE,       // ev_score (like ARENA_ALIGN; the distance and decision workspaces too)
    ARENA_DENOISE,     // ev_denoise (like ARENA_ALIGN; the spectrum scratch too)
    ARENA_STRETCH,     // ev_stretch (like ARENA_ALIGN)
    ARENA_WATERMARK,   // ev_watermark (like ARENA_DENOISE)
    ARENA_WM_DETECT,   // ev_watermark_detect (like ARENA_ALIGN; q and the window sums)
    ARENA_COUNT
};

// One hipMalloc allocation and its owner: move-only, freed when the owner goes or takes another.  The caller has waited for whatever still reads it.
class DevMem {
    void* p_ = nullptr;
public:
    DevMem() = default;
    DevMem(DevMem&& o) noexcept : p_(o.p_) { o.p_ = nullptr; }
    DevMem& operator=(DevMem&& o) noexcept { if (this != &o) { reset(); p_ = o.p_; o.p_ = nullptr; } return *this; }
    DevMem(const DevMem&) = delete;
    DevMem& operator=(const DevMem&) = delete;
    ~DevMem() { reset(); }
    void reset() { if (p_) (void)hipFree(p_); p_ = nullptr; }
    hipError_t alloc(size_t bytes) {      // replaces what it held; holds nothing after a failure
        reset();
        const hipError_t e = hipMalloc(&p_, bytes);
        if (e != hipSuccess) p_ = nullptr;
        return e;
    }
    void* get() const { return p_; }
    template <typename T> T* as() const { return static_cast<T*>(p_); }
    explicit operator bool() const { return p_ != nullptr; }
};
// host bytes into a fresh allocation, with a synchronous copy; `out` holds nothing after a failure
inline hipError_t dev_upload(DevMem& out, const void* src, size_t bytes) {
    hipError_t e = out.alloc(bytes);
    if (e == hipSuccess && bytes) e = hipMemcpy(out.get(), src, bytes, hipMemcpyHostToDevice);
    if (e != hipSuccess) out.reset();
    return e;
}
template <typename T> hipError_t dev_upload(DevMem& out, const std::vector<T>& v) { return dev_upload(out, v.data(), v.size() * sizeof(T)); }

struct WeightEntry { int dtype; int ndim; uint64_t dims[4]; const char* ptr; uint64_t nbytes; };

struct Buf {              // activation buffer with PAD_ROWS of slack on both sides
    char* base = nullptr; // allocation start
    char* p = nullptr;    // logical row 0
    size_t bytes = 0;
};

struct Tap { const void* ptr; int dtype; int ld; int C; int level; /* 0 token, 1 frame, 2+s vocoder stage s */ int shift; };

struct KStat { std::string name; int launches = 0; float ms = 0; double flops = 0, bytes = 0; };
struct PendingEvt { hipEvent_t a, b; int stat; int rec; };
struct LaunchRec { std::string name; int M = 0, N = 0, K = 0, taps = 0, dil = 0; float ms = 0; double flops = 0, bytes = 0; };

// Per-utility state: the setup a utility keeps on the device, the host halves of its last result (valid until its next call) and what ev_get_stage reads.
struct AlignState {       // ev_align; kept apart from the synthesis' mel_lens / mel_offs.  lp: the "log_p_attn" stage of the last call
    std::vector<int32_t> mel_lens; std::vector<int64_t> mel_offs; std::vector<ev::AlignSeq> seqs;
    const float* lp = nullptr; int64_t lp_elems = 0;
};
struct FeaturesState {       // ev_features.  basis, melT: the basis planes on the device; mag: the "feat_mag" stage of the last call
    ev_features_config cfg{}; bool ready = false; DevMem basis, melT;
    std::vector<int32_t> mel_lens; std::vector<int64_t> mel_offs;
    const float* mag = nullptr; int64_t mag_elems = 0;
};
struct PitchState { std::vector<int32_t> mel_lens; std::vector<int64_t> mel_offs; };       // ev_pitch
struct ResampleState {       // ev_resample.  tab: the phase-major table on the device; raw: the "resample_raw" stage of the last call
    ev_resample_config cfg{}; bool ready = false; int up = 1, down = 1, half = 0; DevMem tab; size_t tab_floats = 0;
    std::vector<int64_t> lens, offs, start, end;
    const float* raw = nullptr; int64_t raw_elems = 0;
};
struct StitchState {       // ev_stitch.  tab: the ramp table of the last call (device, EV_STITCH_MAX_FADE floats once allocated; its host copy feeds the upload)
    DevMem tab; int F = -1; std::vector<float> tab_host;
    std::vector<int64_t> doc_lens, doc_offs, pos, start, end; std::vector<float> peak;
};
struct CompareState {       // ev_compare: its result, all of it host memory
    std::vector<double> d, d2, y, y2, rel, rel_ac, chunk_d2, chunk_y2;
    std::vector<float> max_d, peak_y; std::vector<int64_t> arg, nonf, chunk_offs;
};
struct FlacState { std::vector<int64_t> stream_offs, stream_frames, frame_offs; std::vector<uint8_t> kind, porder; };       // ev_flac
struct LoudnessState {       // ev_loudness
    std::vector<double> loud, rel, ms; std::vector<float> gain, peak; std::vector<uint8_t> flags, state;
    std::vector<int64_t> nonf, boffs;
};
struct DeliverState {       // ev_deliver.  tab: the phase-major table on the device (empty for sr_in == sr_out); its own, never ev_resample's
    ev_deliver_config cfg{}; bool ready = false; int up = 1, down = 1, half = 0; DevMem tab;
    std::vector<int64_t> offs, n, clipped; std::vector<float> peak;
};
struct ScoreSide {       // a side of ev_score as ev_score_load left it: cq (total, D) and f0 (total,) or null live in the side's arena
    bool loaded = false; int B = 0, n_mels = 0, n_ceps = 0; int64_t total = 0;
    const int32_t* cq = nullptr; const float* f0 = nullptr;
    std::vector<int32_t> lens, nonf; std::vector<int64_t> offs;
};
struct ScoreState {       // ev_score: the two sides and the host halves of the last result
    ScoreSide side[2];
    std::vector<int64_t> sum_dist, path_offs; std::vector<int32_t> K, cnt[7], lens_a, lens_b, nonf_a, nonf_b;
    std::vector<double> sum_c, sum_c2, mcd, rmse, bias, vuv, warp;
};
struct StftTables { DevMem basis, ibasis, env; };       // the three tables of an (n_fft, hop, window), one allocation each (denoise_upload_tables)
struct WavOut { std::vector<int64_t> lens, offs; };       // the host half of a result of packed waveforms
struct DenoiseState {       // ev_denoise.  tab, bias: its own tables on the device, never ev_features'
    ev_denoise_config cfg{}; bool ready = false; StftTables tab; DevMem bias; WavOut res;
};
struct LimitState { std::vector<float> tp_in, sp_in, tp_out, sp_out, min_gain; std::vector<int64_t> limited, nonf; };       // ev_limit
struct WatermarkState {       // ev_watermark, ev_watermark_detect.  tab: ev_denoise's tables at the watermark's shape, built by the first call
    bool ready = false; StftTables tab; WavOut res;
    std::vector<int64_t> frame_offs; std::vector<int32_t> offset, C, n, bit_C, bit_n, frames;
};
struct StretchState { std::vector<int64_t> lens_out, offs, frame_offs, nonf; std::vector<int32_t> frames, edges; std::vector<uint64_t> sum_dist; };       // ev_stretch

}  // namespace evh

struct ev_handle {
    ev_config cfg;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t aux[2] = {nullptr, nullptr};         // the first two ResBlocks of a generator stage run beside the third
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    std::string err;
    // weights
    evh::DevMem wblob_own; char* wblob = nullptr; size_t wbytes = 0;      // wblob: the blob in use, wblob_own's (ev_load_weights) or the caller's (ev_load_weights_device)
    std::map<std::string, evh::WeightEntry> wt;
    std::map<std::string, float> scalar_cache;   // host copies of 1-element tensors (biases of the Linear(C,1) heads, PE alphas)
    evh::DevMem pe_dev; int pe_cap = 0;     // positional table, extended on demand beyond the packed length
    // SimBERT style encoder (ev_style_load_weights / ev_style_embed): its own blob, merged into `wt` under the "sb." prefix
    evh::DevMem sblob; size_t sbytes = 0; ev_bert_config bcfg{}; bool style_loaded = false;
    // arenas (evh::Arena)
    evh::DevMem arena[evh::ARENA_COUNT]; size_t arena_bytes[evh::ARENA_COUNT] = {};
    char* tok_ks = nullptr; size_t tok_ks_bytes = 0;          // split-K partial sums of the token-rate conv-FFN (tok_splitk); inside ARENA_TOKEN
    char* pinned = nullptr; size_t pinned_bytes = 0;
    // persistent outputs (host side)
    std::vector<int32_t> mel_lens; std::vector<int64_t> mel_offs;
    std::vector<int64_t> forced_dur;
    std::vector<int64_t> pack_host[8]; std::vector<int32_t> pack_rows[8]; int pack_slot = 0;   // host staging of pack_level (kept alive, no sync)
    // layout of the last call
    int B = 0, total_tokens = 0; int64_t total_frames = 0;
    int Rt = 0, Rf = 0;
    std::vector<int32_t> tok_off, tok_len, frm_off;
    std::map<std::string, evh::Tap> taps;
    const int64_t* last_dur = nullptr; const int32_t* last_mel_len_dev = nullptr;
    const int64_t* last_dur_eff = nullptr;       // the durations the length regulator used (ev_synthesize_prosody: after the overrides)
    // per-utility state (the structs above)
    evh::AlignState aln; evh::FeaturesState feat; evh::PitchState pitch; evh::ResampleState rs;
    evh::StitchState stitch; evh::CompareState cmp; evh::FlacState flac; evh::LoudnessState loud; evh::LimitState lim; evh::DeliverState dlv; evh::ScoreState score; evh::DenoiseState dn; evh::StretchState str; evh::WatermarkState wm;
    // device maps (inside the arena)
    int32_t *d_tok_seq = nullptr, *d_tok_pos = nullptr, *d_tok_off = nullptr, *d_tok_len = nullptr, *d_cu = nullptr;
    uint8_t* d_tok_valid = nullptr;
    int32_t *d_frm_seq = nullptr, *d_frm_pos = nullptr, *d_frm_off = nullptr, *d_mel_len = nullptr, *d_frm_len = nullptr;
    uint8_t* d_frm_valid = nullptr;
    // profiling
    bool profiling = false;
    std::vector<evh::KStat> stats; std::map<std::string, int> stat_idx;
    std::vector<evh::LaunchRec> launches;          // one record per launch of the last profiled call, in launch order
    std::vector<evh::PendingEvt> pending; std::vector<hipEvent_t> evt_pool; size_t evt_next = 0;
    std::map<std::string, float> timings;
    std::map<std::string, std::pair<hipEvent_t, hipEvent_t>> region_evt;
};

namespace evh __attribute__((visibility("hidden"))) {

int fail(ev_handle* h, const char* fmt, ...) __attribute__((format(printf, 2, 3)));      // sets the handle's (h null: the thread's) message; -1

#define HIPCHK(h, expr)                                                                       \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) return evh::fail(h, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// ---------------------------------------------------------------- arenas
int arena_reserve(ev_handle* h, int idx, size_t bytes);
struct ArenaPlan {   // two-pass: the dry pass measures, the second pass hands out pointers
    ev_handle* h; int idx; bool dry; size_t off = 0;
    char* take(size_t bytes) {
        off = align_up(off, 256);
        char* p = dry ? nullptr : h->arena[idx].as<char>() + off;
        off += bytes;
        return p;
    }
    Buf rows(size_t rows, size_t ld, size_t es) {
        Buf b;
        const size_t pad = (size_t)PAD_ROWS * ld * es;
        b.bytes = rows * ld * es;
        b.base = take(pad + b.bytes + pad);
        b.p = dry ? nullptr : b.base + pad;
        return b;
    }
    template <typename T> T* arr(size_t n) { return reinterpret_cast<T*>(take(n * sizeof(T))); }
};
// runs `body(ArenaPlan&)` dry, grows the arena to what it measured, and runs it again for the pointers
template <typename Body> int arena_plan(ev_handle* h, int idx, Body&& body) {
    ArenaPlan dry{h, idx, true};
    body(dry);
    if (arena_reserve(h, idx, dry.off)) return -1;
    ArenaPlan real{h, idx, false};
    body(real);
    return 0;
}
int pinned_reserve(ev_handle* h, size_t bytes);

// ---------------------------------------------------------------- profiling
struct KScope {   // wraps one kernel launch with events when profiling is on
    ev_handle* h; int sid = -1; int rec = -1; hipEvent_t a{}, b{}; hipStream_t st;
    KScope(ev_handle* h_, const char* name, double flops, double bytes, hipStream_t s = nullptr, const ev::ConvGemmParams* g = nullptr);
    ~KScope();
};
void region_begin(ev_handle* h, const char* name);
void region_end(ev_handle* h, const char* name);
void profiling_reset(ev_handle* h);
void profiling_collect(ev_handle* h);

// ---------------------------------------------------------------- the scaffold of a utility call
// a versioned struct's size field against the library's: `field` is how the message names it ("out->struct_size", "cfg->struct_size", ...)
int check_struct_size(ev_handle* h, const char* who, const char* field, uint32_t got, const char* type, size_t want);
// a result struct back to zero, its struct_size kept
template <typename T> void reset_result(T* out) {
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz;
}
// The bracket of a call: call_begin once the arguments are accepted, call_end after the last launch (it closes the "total" region, waits for the
// stream and collects the profile).  An error return in between does neither, and leaves the stream as it is.
int call_begin(ev_handle* h);
int call_end(ev_handle* h);

}  // namespace evh
