// libevhip.so host side: handle, packed-weight table, workspace arena, row layouts, forward
// orchestration and the C ABI declared in include/evhip.h.
//
// Data layout in HBM: every activation is channels-last [rows][channels].
// Rows of a batch are laid out with zero gaps between utterances:
//     [G gap rows][utt 0 rows][G gap rows][utt 1 rows] ... [G gap rows][pad to a multiple of 256]
// G = 4 at token rate and at mel-frame rate; the vocoder's upsampled stages inherit the frame
// layout scaled by the cumulative upsampling factor (gap 32 / 256 / 512 / 1024 rows >= the largest
// conv halo of that stage, 25 rows).  Every kernel writes exact zeros into invalid rows, so a conv
// that reads across an utterance edge sees the zero padding the reference's per-utterance (B = 1)
// Conv1d(padding=...) provides, and no conv ever needs a per-row bounds test.
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdarg.h>
#include <stdlib.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <cmath>
#include <limits>
#include <map>
#include <string>
#include <vector>

#include "../../include/evhip.h"
#include "../../include/evhip_ops.h"
#include "ev_kernels.h"

using namespace ev;

namespace {

constexpr int GAP = 4;            // gap rows between utterances (token and frame rate)
constexpr int ROW_ALIGN = 256;    // row counts are padded to the largest GEMM M tile
constexpr int PAD_ROWS = 64;      // readable slack rows before / after every activation buffer
constexpr int MEL_PAD = 96;       // n_mels padded to a multiple of 32 (MFMA K granularity)
constexpr size_t PIN_MAX_B = 1 << 16;                // utterances per call the pinned staging area is laid out for
constexpr size_t PIN_FRAME = 4 * PIN_MAX_B * 4;      // byte offset of the frame-layout region (after the token-layout region)
constexpr size_t PIN_BYTES = PIN_FRAME + 2 * PIN_MAX_B * 4;
constexpr size_t PIN_PROSODY = PIN_BYTES;                  // ev_synthesize_prosody: its per-utterance controls, 5 floats per utterance
constexpr size_t PIN_BYTES_PROSODY = PIN_PROSODY + 5 * PIN_MAX_B * 4;

thread_local std::string g_create_error;

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

}  // namespace

struct ev_handle {
    ev_config cfg;
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    hipStream_t aux[2] = {nullptr, nullptr};         // the first two ResBlocks of a generator stage run beside the third
    hipEvent_t ev_fork = nullptr, ev_join[2] = {nullptr, nullptr};
    std::string err;
    // weights
    char* wblob = nullptr; bool wblob_owned = false; size_t wbytes = 0;
    std::map<std::string, WeightEntry> wt;
    std::map<std::string, float> scalar_cache;
    float* pe_dev = nullptr; int pe_cap = 0;     // positional table, extended on demand beyond the packed length   // host copies of 1-element tensors (biases of the Linear(C,1) heads, PE alphas)
    // SimBERT style encoder (ev_style_load_weights / ev_style_embed): its own blob, merged into `wt` under the "sb." prefix
    char* sblob = nullptr; size_t sbytes = 0; ev_bert_config bcfg{}; bool style_loaded = false;
    // arena
    char* arena[11] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr}; size_t arena_bytes[11] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // [0] token-rate phase, [1] frame-rate phase + vocoder, [2] SimBERT,
                                                                                                 // [3] ev_align (its results live here until the next ev_align), [4] ev_features, [5] ev_pitch, [6] ev_resample, [7] ev_stitch (likewise), [8] ev_compare (scratch only: its result is host memory), [9] ev_flac (likewise [3]), [10] ev_loudness (likewise)
    char* tok_ks = nullptr; size_t tok_ks_bytes = 0;          // split-K partial sums of the token-rate conv-FFN (tok_splitk); inside arena 0
    char* pinned = nullptr; size_t pinned_bytes = 0;
    // persistent outputs (host side)
    std::vector<int32_t> mel_lens; std::vector<int64_t> mel_offs;
    std::vector<int64_t> forced_dur;
    std::vector<int64_t> pack_host[8]; std::vector<int32_t> pack_rows[8]; int pack_slot = 0;   // host staging of pack_level (kept alive, no sync)
    // layout of the last call
    int B = 0, total_tokens = 0; int64_t total_frames = 0;
    int Rt = 0, Rf = 0;
    std::vector<int32_t> tok_off, tok_len, frm_off;
    std::map<std::string, Tap> taps;
    const int64_t* last_dur = nullptr; const int32_t* last_mel_len_dev = nullptr;
    const int64_t* last_dur_eff = nullptr;       // the durations the length regulator used (ev_synthesize_prosody: after the overrides)
    // ev_align: host halves of its result (kept apart from the synthesis' mel_lens / mel_offs) and the "log_p_attn" stage of the last call
    std::vector<int32_t> aln_mel_lens; std::vector<int64_t> aln_mel_offs; std::vector<AlignSeq> aln_seqs;
    const float* aln_lp = nullptr; int64_t aln_lp_elems = 0;
    // ev_features: its setup (basis planes on the device), the host halves of its result and the "feat_mag" stage of the last call
    ev_features_config fcfg{}; bool feat_ready = false; char* feat_basis = nullptr; float* feat_melT = nullptr;
    std::vector<int32_t> feat_mel_lens; std::vector<int64_t> feat_mel_offs;
    const float* feat_mag = nullptr; int64_t feat_mag_elems = 0;
    // ev_pitch: the host halves of its result
    std::vector<int32_t> pit_mel_lens; std::vector<int64_t> pit_mel_offs;
    // ev_resample: its setup (the phase-major table on the device), the host halves of its result and the "resample_raw" stage of the last call
    ev_resample_config rcfg{}; bool rs_ready = false; int rs_up = 1, rs_down = 1, rs_half = 0; float* rs_tab = nullptr; size_t rs_tab_floats = 0;
    std::vector<int64_t> rs_lens, rs_offs, rs_start, rs_end;
    const float* rs_raw = nullptr; int64_t rs_raw_elems = 0;
    // ev_stitch: the ramp table of the last call (device, EV_STITCH_MAX_FADE floats once allocated; its host copy feeds the upload) and the host halves of its result
    float* st_tab = nullptr; int st_F = -1; std::vector<float> st_tab_host;
    std::vector<int64_t> st_doc_lens, st_doc_offs, st_pos, st_start, st_end; std::vector<float> st_peak;
    // ev_compare: its result, all of it host memory
    std::vector<double> cmp_d, cmp_d2, cmp_y, cmp_y2, cmp_rel, cmp_rel_ac, cmp_chunk_d2, cmp_chunk_y2;
    std::vector<float> cmp_max_d, cmp_peak_y; std::vector<int64_t> cmp_arg, cmp_nonf, cmp_chunk_offs;
    // ev_flac: the host halves of its result
    std::vector<int64_t> fl_stream_offs, fl_stream_frames, fl_frame_offs; std::vector<uint8_t> fl_kind, fl_porder;
    // ev_loudness: the host halves of its result
    std::vector<double> ld_loud, ld_rel, ld_ms; std::vector<float> ld_gain, ld_peak; std::vector<uint8_t> ld_flags, ld_state;
    std::vector<int64_t> ld_nonf, ld_boffs;
    // device maps (inside the arena)
    int32_t *d_tok_seq = nullptr, *d_tok_pos = nullptr, *d_tok_off = nullptr, *d_tok_len = nullptr, *d_cu = nullptr;
    uint8_t* d_tok_valid = nullptr;
    int32_t *d_frm_seq = nullptr, *d_frm_pos = nullptr, *d_frm_off = nullptr, *d_mel_len = nullptr, *d_frm_len = nullptr;
    uint8_t* d_frm_valid = nullptr;
    // profiling
    bool profiling = false;
    std::vector<KStat> stats; std::map<std::string, int> stat_idx;
    std::vector<LaunchRec> launches;          // one record per launch of the last profiled call, in launch order
    std::vector<PendingEvt> pending; std::vector<hipEvent_t> evt_pool; size_t evt_next = 0;
    std::map<std::string, float> timings;
    std::map<std::string, std::pair<hipEvent_t, hipEvent_t>> region_evt;
};

namespace {

int fail(ev_handle* h, const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (h) h->err = buf; else g_create_error = buf;
    return -1;
}

#define HIPCHK(h, expr)                                                                       \
    do {                                                                                      \
        hipError_t _e = (expr);                                                               \
        if (_e != hipSuccess) return fail(h, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
    } while (0)

size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
int ilog2(int v) { int s = 0; while ((1 << s) < v) ++s; return s; }

// ---------------------------------------------------------------- weights
// Blob layout (emotivoice_amd/packer.py): "EVW1\0\0\0\0" | u32 count | u32 reserved |
// count x { char name[64]; u32 dtype(0 f16,1 f32,2 i32,3 i64); u32 ndim; u64 dims[4]; u64 offset; u64 nbytes } | data (256-B aligned)
struct BlobEntry { char name[64]; uint32_t dtype, ndim; uint64_t dims[4]; uint64_t offset, nbytes; };

// `style` selects which of the two blobs is being (re)loaded: the generator's (every name without the "sb." prefix) or the
// SimBERT encoder's ("sb." names); the other one's entries stay in the table.
int parse_blob(ev_handle* h, const char* host_hdr, size_t nbytes, bool style = false) {
    if (nbytes < 16 || memcmp(host_hdr, "EVW1", 4) != 0) return fail(h, "weight blob: bad magic");
    uint32_t count;
    memcpy(&count, host_hdr + 8, 4);
    if (16 + (size_t)count * sizeof(BlobEntry) > nbytes) return fail(h, "weight blob: truncated table");
    for (auto it = h->wt.begin(); it != h->wt.end();) {
        const bool is_style = it->first.compare(0, 3, "sb.") == 0;
        if (is_style == style) it = h->wt.erase(it); else ++it;
    }
    h->scalar_cache.clear();
    if (!style) {
        if (h->pe_dev) { (void)hipFree(h->pe_dev); h->pe_dev = nullptr; }
        h->pe_cap = 0;
    }
    char* base = style ? h->sblob : h->wblob;
    for (uint32_t i = 0; i < count; ++i) {
        BlobEntry e;
        memcpy(&e, host_hdr + 16 + (size_t)i * sizeof(BlobEntry), sizeof e);
        e.name[63] = 0;
        if (e.offset + e.nbytes > nbytes) return fail(h, "weight blob: tensor %s out of range", e.name);
        if ((strncmp(e.name, "sb.", 3) == 0) != style) return fail(h, "weight blob: tensor %s does not belong in the %s blob", e.name, style ? "SimBERT" : "generator");
        WeightEntry w;
        w.dtype = (int)e.dtype; w.ndim = (int)e.ndim; memcpy(w.dims, e.dims, sizeof w.dims);
        w.ptr = base + e.offset; w.nbytes = e.nbytes;
        h->wt[e.name] = w;
    }
    return 0;
}

const WeightEntry* W(ev_handle* h, const std::string& name) {
    auto it = h->wt.find(name);
    if (it == h->wt.end()) { h->err = "missing packed weight: " + name; return nullptr; }
    return &it->second;
}
#define WPTR(var, type, name)                                   \
    const type* var;                                            \
    {                                                           \
        const WeightEntry* _w = W(h, name);                     \
        if (!_w) return -1;                                     \
        var = reinterpret_cast<const type*>(_w->ptr);           \
    }

int get_scalar(ev_handle* h, const std::string& name, float* v) {
    auto it = h->scalar_cache.find(name);
    if (it == h->scalar_cache.end()) {
        const WeightEntry* w = W(h, name);
        if (!w) return -1;
        float x;
        HIPCHK(h, hipMemcpy(&x, w->ptr, 4, hipMemcpyDeviceToHost));
        it = h->scalar_cache.emplace(name, x).first;
    }
    *v = it->second;
    return 0;
}

// positional encoding rows [0, need): the packed (torch-exact) table first, longer utterances computed on the device
int ensure_pe(ev_handle* h, int need) {
    if (need <= h->pe_cap) return 0;
    const WeightEntry* pw = W(h, "pe");
    const WeightEntry* dw = W(h, "pe_div");
    if (!pw || !dw) return -1;
    const int C = h->cfg.hidden, packed = (int)pw->dims[0];
    int cap = std::max(need, std::max(packed, 2 * h->pe_cap));
    cap = (int)align_up((size_t)cap, 1024);
    float* nb = nullptr;
    HIPCHK(h, hipMalloc((void**)&nb, (size_t)cap * C * 4));
    const int have = std::min(packed, cap);
    HIPCHK(h, hipMemcpyAsync(nb, pw->ptr, (size_t)have * C * 4, hipMemcpyDeviceToDevice, h->stream));
    launch_pe_extend(nb, reinterpret_cast<const float*>(dw->ptr), have, cap, C, h->stream);
    HIPCHK(h, hipStreamSynchronize(h->stream));
    if (h->pe_dev) HIPCHK(h, hipFree(h->pe_dev));
    h->pe_dev = nb; h->pe_cap = cap;
    return 0;
}

// ---------------------------------------------------------------- arena
int arena_reserve(ev_handle* h, int idx, size_t bytes) {
    if (bytes <= h->arena_bytes[idx]) return 0;
    if (h->arena[idx]) { HIPCHK(h, hipStreamSynchronize(h->stream)); HIPCHK(h, hipFree(h->arena[idx])); h->arena[idx] = nullptr; h->arena_bytes[idx] = 0; }
    bytes = align_up(bytes + bytes / 8, 1 << 20);
    HIPCHK(h, hipMalloc((void**)&h->arena[idx], bytes));
    HIPCHK(h, hipMemsetAsync(h->arena[idx], 0, bytes, h->stream));
    h->arena_bytes[idx] = bytes;
    return 0;
}
struct ArenaPlan {   // two-pass: the dry pass measures, the second pass hands out pointers
    ev_handle* h; int idx; bool dry; size_t off = 0;
    char* take(size_t bytes) {
        off = align_up(off, 256);
        char* p = dry ? nullptr : h->arena[idx] + off;
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

int pinned_reserve(ev_handle* h, size_t bytes) {
    if (bytes <= h->pinned_bytes) return 0;
    if (h->pinned) { HIPCHK(h, hipStreamSynchronize(h->stream)); HIPCHK(h, hipHostFree(h->pinned)); h->pinned = nullptr; }
    bytes = align_up(bytes * 2, 1 << 16);
    HIPCHK(h, hipHostMalloc((void**)&h->pinned, bytes, hipHostMallocDefault));
    h->pinned_bytes = bytes;
    return 0;
}

// ---------------------------------------------------------------- profiling helpers
int stat_id(ev_handle* h, const char* name) {
    auto it = h->stat_idx.find(name);
    if (it != h->stat_idx.end()) return it->second;
    KStat s; s.name = name;
    h->stats.push_back(s);
    h->stat_idx[name] = (int)h->stats.size() - 1;
    return (int)h->stats.size() - 1;
}
hipEvent_t get_evt(ev_handle* h) {
    if (h->evt_next == h->evt_pool.size()) { hipEvent_t e; (void)hipEventCreate(&e); h->evt_pool.push_back(e); }
    return h->evt_pool[h->evt_next++];
}
struct KScope {   // wraps one kernel launch with events when profiling is on
    ev_handle* h; int sid = -1; int rec = -1; hipEvent_t a{}, b{}; hipStream_t st;
    KScope(ev_handle* h_, const char* name, double flops, double bytes, hipStream_t s = nullptr, const ConvGemmParams* g = nullptr)
        : h(h_), st(s ? s : h_->stream) {
        if (!h->profiling) return;
        sid = stat_id(h, name);
        h->stats[sid].launches++; h->stats[sid].flops += flops; h->stats[sid].bytes += bytes;
        LaunchRec r; r.name = name; r.flops = flops; r.bytes = bytes;
        if (g) { r.M = g->M; r.N = g->N; r.K = g->K; r.taps = g->taps; r.dil = g->dil; }
        h->launches.push_back(r);
        rec = (int)h->launches.size() - 1;
        a = get_evt(h); b = get_evt(h);
        (void)hipEventRecord(a, st);
    }
    ~KScope() {
        if (sid < 0) return;
        (void)hipEventRecord(b, st);
        h->pending.push_back({a, b, sid, rec});
    }
};
void region_begin(ev_handle* h, const char* name) {
    if (!h->profiling) return;
    auto& pr = h->region_evt[name];
    if (!pr.first) { (void)hipEventCreate(&pr.first); (void)hipEventCreate(&pr.second); }
    (void)hipEventRecord(pr.first, h->stream);
}
void region_end(ev_handle* h, const char* name) {
    if (!h->profiling) return;
    (void)hipEventRecord(h->region_evt[name].second, h->stream);
}
void profiling_reset(ev_handle* h) {
    h->stats.clear(); h->stat_idx.clear(); h->pending.clear(); h->evt_next = 0; h->timings.clear(); h->launches.clear();
}
void profiling_collect(ev_handle* h) {
    if (!h->profiling) return;
    for (auto& p : h->pending) {
        float ms = 0;
        (void)hipEventElapsedTime(&ms, p.a, p.b);
        h->stats[p.stat].ms += ms;
        if (p.rec >= 0 && p.rec < (int)h->launches.size()) h->launches[p.rec].ms = ms;
    }
    h->pending.clear();
    for (auto& kv : h->region_evt) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, kv.second.first, kv.second.second) == hipSuccess) h->timings[kv.first] = ms;
    }
}

// ---------------------------------------------------------------- launch wrappers with precondition checks
int check_gemm(ev_handle* h, const ConvGemmParams& p) {
    const int es = p.dtype == DT_F16 ? 2 : 4;
    if (p.M % ROW_ALIGN) return fail(h, "gemm: M=%d not a multiple of %d", p.M, ROW_ALIGN);
    if (p.dtype == DT_F32S && (p.K % 32 || !p.W_lo)) return fail(h, "gemm: bad split-precision call");
    if (p.pro_lrelu && !(p.pro_slope >= 0.f && p.pro_slope <= 1.f)) return fail(h, "gemm: prologue leaky-relu slope %g outside [0, 1]", p.pro_slope);
    if (p.N % 32) return fail(h, "gemm: N=%d not a multiple of 32", p.N);
    if ((p.K * es) % 64) return fail(h, "gemm: K=%d not a multiple of %d", p.K, 64 / es);
    if ((p.taps - 1) * p.dil > 64) return fail(h, "gemm: conv span %d > 64", (p.taps - 1) * p.dil);
    if (p.center * p.dil > PAD_ROWS || (p.taps - 1 - p.center) * p.dil > PAD_ROWS) return fail(h, "gemm: halo exceeds buffer slack");
    if ((p.lda * es) % 16 || ((uintptr_t)p.A & 15) || ((uintptr_t)p.W & 15)) return fail(h, "gemm: unaligned operand");
    if (!p.out16 && !p.out32 && !p.mxo_h) return fail(h, "gemm: no output");
    if (p.dtype == DT_MX && (p.K % 32 || !p.W)) return fail(h, "gemm: bad MX call");
    if (mx_check(p)) return fail(h, "gemm: inconsistent MX plane-set fields (dtype %d, N %d, K %d, taps %d)", p.dtype, p.N, p.K, p.taps);
    if (splitk_check(p)) return fail(h, "gemm: inconsistent split-K call (ksplit %d, dtype %d, N %d, K %d)", p.ksplit, p.dtype, p.N, p.K);
    return 0;
}
// flop_scale: algorithmic / executed FLOPs (2/3 for a ConvTranspose1d run as a 3-tap conv: each output sample has two real taps)
int gemm(ev_handle* h, const char* name, const ConvGemmParams& p, double valid_rows, hipStream_t st = nullptr, double flop_scale = 1.0) {
    if (check_gemm(h, p)) return -1;
    const int es = p.dtype == DT_F16 ? 2 : 4;
    const double flops = 2.0 * valid_rows * p.N * (double)p.K * p.taps * flop_scale;
    double bytes = valid_rows * ((double)p.K * es + (double)p.N * (p.out16 ? 2 : 0) + (double)p.N * (p.out32 ? 4 : 0)) +
                   (double)p.N * p.K * p.taps * es;
    // a DT_MX call that launch_conv_gemm will run as the split-precision kernel (no plane-set input, unsupported shape) is recorded as such
    if (p.dtype == DT_MX && mx_launch_kind(p) == 0) name = strncmp(name, "dec", 3) == 0 ? "dec_f32_gemm" : "voc_conv_gemm_x3";
    KScope ks(h, name, flops, bytes, st, &p);
    launch_conv_gemm(p, st ? st : h->stream);
    return 0;
}
// three independent convs of one level of a stage's ResBlocks as one grid (launch_conv_gemm_group3), or one by one when they are not such a triple
int gemm_group3(ev_handle* h, const char* name, const ConvGemmParams* ps, double valid_rows) {
    double flops = 0, bytes = 0;
    int taps = 0;
    for (int i = 0; i < 3; ++i) {
        if (check_gemm(h, ps[i])) return -1;
        flops += 2.0 * valid_rows * ps[i].N * (double)ps[i].K * ps[i].taps;
        bytes += valid_rows * ((double)ps[i].K * 4 + (double)ps[i].N * (ps[i].out32 ? 4 : 0)) + (double)ps[i].N * ps[i].K * ps[i].taps * 4;
        taps += ps[i].taps;
    }
    if (launch_conv_gemm_group3(ps, h->stream, true) == 0) {
        ConvGemmParams shape = ps[0];
        shape.taps = taps; shape.dil = 0;          // (the record of a grouped launch: the three convs' taps summed, no single dilation)
        KScope ks(h, name, flops, bytes, nullptr, &shape);
        return launch_conv_gemm_group3(ps, h->stream);
    }
    for (int i = 0; i < 3; ++i)          // not a triple the grouped kernel takes: one by one
        if (gemm(h, name, ps[i], valid_rows)) return -1;
    return 0;
}
ConvGemmParams gemm_defaults() {
    ConvGemmParams p;
    memset(&p, 0, sizeof p);
    p.taps = 1; p.dil = 1; p.center = 0; p.out_scale = 1.0f;
    return p;
}

// token-rate (fp32) GEMM operands: exact fp32 MFMA or the hi/lo split pair (cfg.token_rate_split)
int tok_weights(ev_handle* h, const std::string& base /* e.g. "enc.0.qkv.w" */, ConvGemmParams& p) {
    const bool dec = base.compare(0, 4, "dec.") == 0 || base.compare(0, 7, "to_mel.") == 0;
    if (dec ? (h->cfg.decoder_precision == EV_PREC_X3 || h->cfg.decoder_precision == EV_PREC_MX) : h->cfg.token_rate_split != 0) {
        // hi part: fp16(w).  The token-rate stack packs it as "<name>32h"; for the decoder it is the fp16 copy "<name>16"
        const WeightEntry* hi = W(h, base + (h->wt.count(base + "32h") ? "32h" : "16"));
        const WeightEntry* lo = W(h, base + "32l");
        if (!hi || !lo) return -1;
        p.dtype = DT_F32S; p.W = hi->ptr; p.W_lo = lo->ptr;
    } else {
        const WeightEntry* w = W(h, base + "32");
        if (!w) return -1;
        p.dtype = DT_F32; p.W = w->ptr; p.W_lo = nullptr;
    }
    return 0;
}

// raw storage of one MX plane set (ev_gemm_mx.h), sized for the largest [rows][C] it will hold; mx_view() lays a tensor into it
struct PlaneBuf { char* h = nullptr; char* q4[2] = {nullptr, nullptr}; char* qs[2] = {nullptr, nullptr}; };
struct MxView { char* h; char* q4[2]; char* qs[2]; unsigned qs_stride; int logC; };
static constexpr size_t MX_PAD = 64;        // slack rows of every plane, both sides
MxView mx_view(const PlaneBuf& b, size_t rows, int C) {
    MxView v;
    v.h = b.h + MX_PAD * C * 2;
    for (int i = 0; i < 2; ++i) { v.q4[i] = b.q4[i] + MX_PAD * (C / 2); v.qs[i] = b.qs[i] + MX_PAD * 4; }
    v.qs_stride = (unsigned)((rows + 2 * MX_PAD) * 4);
    v.logC = ilog2(C);
    return v;
}
void mx_out(ConvGemmParams& p, const MxView& v, float slope) {
    p.mxo_h = v.h; p.mxo_q4[0] = v.q4[0]; p.mxo_q4[1] = v.q4[1]; p.mxo_qs[0] = v.qs[0]; p.mxo_qs[1] = v.qs[1];
    p.mxo_qs_stride = v.qs_stride; p.mxo_logC = v.logC; p.mxo_slope = slope;
}
void mx_in(ConvGemmParams& p, const MxView& v, int C) {
    p.A = v.h; p.lda = C; p.pro_lrelu = 0;
    p.mx_x4[0] = v.q4[0]; p.mx_x4[1] = v.q4[1]; p.mx_xs[0] = v.qs[0]; p.mx_xs[1] = v.qs[1]; p.mx_xs_stride = v.qs_stride;
}

// EV_PREC_MX decoder: plane set of the conv-FFN's hidden activation [R][4C] and the planes-kernel scratch of its fp32 input [R][C]
struct DecMx { PlaneBuf ffn; char* scratch; size_t scratch_bytes; };

struct RowCtx {     // one row layout (token rate or frame rate)
    int R; const uint8_t* valid; const int32_t* row_seq; const int32_t* seq_off; const int32_t* seq_len; int B; int max_len;
    double n_valid;
};

// Split-K of a token-rate GEMM (ev_config.token_splitk; ConvGemmParams::ksplit): a rule on the layer's shape only -- never on the row count -- so that an
// utterance alone and inside a batch gets the same summation order.  It takes the conv-FFN's second conv (N = hidden, 144 (K-chunk, tap) steps: 4 ranges of 36);
// N <= hidden keeps the partial-sum traffic (ksplit x M x N x 4 bytes, written and read once) small beside the operands.  Measured (bench.py --token-splitk,
// one MI355X): B = 1, 64 / 256 phonemes 4.25 / 5.2 -> 3.95 / 4.85 ms; at 32 x 256 tokens the encoder pays +0.08 ms for the reduction launches.  The predictors'
// k = 3 convs (36 steps) were tried with 3 ranges as well: another -0.07 ms at B = 1 for +0.14 ms at B = 32 -- left in one pass.
void tok_splitk(ev_handle* h, ConvGemmParams& p) {
    if (h->cfg.token_splitk != 0 || p.dtype != DT_F32S || p.N % 64 || p.N > h->cfg.hidden || p.add16_a) return;
    const int nkc = p.K / 32, steps = nkc * p.taps;
    const int S = (steps >= 144 && nkc % 4 == 0) ? 4 : 1;
    if (S <= 1 || !h->tok_ks || (size_t)S * (size_t)p.M * (size_t)p.N * 4 > h->tok_ks_bytes) return;          // (the arena sizes the buffer for the rule's worst case)
    p.ksplit = S; p.mx_scratch = h->tok_ks; p.mx_scratch_size = h->tok_ks_bytes;
}

// Encoder / decoder stack (reference modules/encoder.py:316-324, layer :154-200).  x (fp32 residual stream,
// [R][C]) is updated in place; y receives after_norm(x) in `prec` dtype (and y32_tap in fp32 if given).
int run_stack(ev_handle* h, const char* pre, int layers, int prec, const RowCtx& rc, Buf& x, Buf& hbuf, Buf& qkv, Buf& ctx, Buf& ffn,
              Buf& y, float* y32_tap, std::vector<Buf>* layer_taps, const DecMx* dmx = nullptr) {
    const int C = h->cfg.hidden, F = 4 * C, kf = h->cfg.ffn_kernel;
    const char* wsuf = prec == DT_F16 ? "w16" : "w32";
    const std::string sp(pre);
    const std::string kn = std::string(pre) + (prec == DT_F16 ? "_f16" : "_f32");
    for (int i = 0; i < layers; ++i) {
        const std::string lp = sp + "." + std::to_string(i);
        WPTR(g1, float, lp + ".ln1.g"); WPTR(b1, float, lp + ".ln1.b");
        WPTR(g2, float, lp + ".ln2.g"); WPTR(b2, float, lp + ".ln2.b");
        WPTR(wqkv, char, lp + ".qkv." + wsuf); WPTR(bqkv, float, lp + ".qkv.b");
        WPTR(wout, char, lp + ".out." + wsuf); WPTR(bout, float, lp + ".out.b");
        WPTR(wf1, char, lp + ".ffn1." + wsuf); WPTR(bf1, float, lp + ".ffn1.b");
        WPTR(wf2, char, lp + ".ffn2." + wsuf); WPTR(bf2, float, lp + ".ffn2.b");
        ConvGemmParams p = gemm_defaults();
        p.dtype = prec; p.A = hbuf.p; p.lda = C; p.W = wqkv; p.bias = bqkv; p.M = rc.R; p.N = 3 * C; p.K = C;
        p.row_valid = rc.valid; p.ldo = 3 * C;
        if (prec == DT_F32 && tok_weights(h, lp + ".qkv.w", p)) return -1;
        if (prec == DT_F16) p.out16 = qkv.p; else p.out32 = (float*)qkv.p;
        // EV_PREC_MX decoder: the QKV / output projections on the one-tap MX GEMM (ev_gemm_mx1.h); their fp32 inputs become plane sets in the scratch
        const bool lin_mx = dmx && p.dtype == DT_F32S && h->wt.count(lp + ".qkv.wmx") && h->wt.count(lp + ".out.wmx");
        // ... and the two LayerNorms write the plane sets their consumers (QKV, the conv-FFN's first conv) read straight into that scratch: no fp32 copy of
        // LN(x) and no mx_planes_kernel pass over it (ev_config.decoder_ln_planes = 1 restores the two passes; the planes are the same bits either way)
        const bool ln_pl = dmx && h->cfg.decoder_ln_planes == 0 && C <= 512 && dmx->scratch_bytes >= mx_scratch_bytes(rc.R, C);
        const MxScratchPlanes lnp = ln_pl ? mx_scratch_planes(dmx->scratch, rc.R, C) : MxScratchPlanes{};
        auto ln_to_planes = [&](LayerNormParams& l) {
            l.out32 = nullptr; l.out16 = nullptr;
            l.mxo_h = lnp.h; l.mxo_q4[0] = lnp.q4[0]; l.mxo_q4[1] = lnp.q4[1]; l.mxo_qs[0] = lnp.qs[0]; l.mxo_qs[1] = lnp.qs[1]; l.mxo_qs_stride = lnp.qs_stride;
        };
        auto planes_in = [&](ConvGemmParams& q) {
            q.A = lnp.h; q.lda = C; q.mx_x4[0] = lnp.q4[0]; q.mx_x4[1] = lnp.q4[1]; q.mx_xs[0] = lnp.qs[0]; q.mx_xs[1] = lnp.qs[1]; q.mx_xs_stride = lnp.qs_stride;
        };
        LayerNormParams ln{};
        ln.x = (const float*)x.p; ln.ldx = C; ln.rows = rc.R; ln.C = C; ln.gamma = g1; ln.beta = b1; ln.eps = 1e-12f;
        ln.row_valid = rc.valid; ln.ldo = C;
        if (prec == DT_F16) ln.out16 = hbuf.p; else ln.out32 = (float*)hbuf.p;
        if (lin_mx && ln_pl) ln_to_planes(ln);
        { KScope ks(h, "layernorm", 0, rc.n_valid * C * 6.0); launch_layernorm(ln, h->stream); }
        if (lin_mx) { p.dtype = DT_MX; p.W_mx = h->wt[lp + ".qkv.wmx"].ptr; p.mx_scratch = dmx->scratch; p.mx_scratch_size = dmx->scratch_bytes; }
        if (lin_mx && ln_pl) planes_in(p);
        if (gemm(h, lin_mx ? (std::string(pre) + "_mx_gemm").c_str() : (kn + "_gemm").c_str(), p, rc.n_valid)) return -1;
        AttnParams ap{};
        // decoder in the strict / mx modes: split-precision attention (three fp16 MFMAs per product); the token-rate encoder keeps exact fp32
        const bool att_split = prec == DT_F32 && !strcmp(pre, "dec") && (h->cfg.decoder_precision == EV_PREC_X3 || h->cfg.decoder_precision == EV_PREC_MX) &&
                               C / h->cfg.heads == 48 && h->cfg.decoder_attention == 0;
        ap.qkv = qkv.p; ap.dtype = att_split ? (int)DT_F32S : prec; ap.ld = 3 * C; ap.C = C; ap.heads = h->cfg.heads; ap.seq_off = rc.seq_off;
        ap.seq_len = rc.seq_len; ap.B = rc.B; ap.max_len = rc.max_len; ap.out = ctx.p; ap.ldo = C;
        { KScope ks(h, (kn + "_attention").c_str(), 0, 0); launch_attention(ap, h->stream); }
        p = gemm_defaults();
        p.dtype = prec; p.A = ctx.p; p.lda = C; p.W = wout; p.bias = bout; p.M = rc.R; p.N = C; p.K = C;
        p.row_valid = rc.valid; p.res = x.p; p.res_dtype = DT_F32; p.ldres = C; p.out32 = (float*)x.p; p.ldo = C;
        if (prec == DT_F32 && tok_weights(h, lp + ".out.w", p)) return -1;
        if (lin_mx) { p.dtype = DT_MX; p.W_mx = h->wt[lp + ".out.wmx"].ptr; p.mx_scratch = dmx->scratch; p.mx_scratch_size = dmx->scratch_bytes; }
        if (gemm(h, lin_mx ? (std::string(pre) + "_mx_gemm").c_str() : (kn + "_gemm").c_str(), p, rc.n_valid)) return -1;
        p = gemm_defaults();
        p.dtype = prec; p.A = hbuf.p; p.lda = C; p.W = wf1; p.bias = bf1; p.M = rc.R; p.N = F; p.K = C; p.taps = kf; p.center = (kf - 1) / 2;
        p.row_valid = rc.valid; p.act = ACT_GELU; p.ldo = F;
        if (prec == DT_F32 && tok_weights(h, lp + ".ffn1.w", p)) return -1;
        // EV_PREC_MX decoder: the conv-FFN (72 % of the stack's FLOPs) on the MX kernel; its hidden activation only exists as conv2's operand planes
        const bool ffn_mx = dmx && p.dtype == DT_F32S && h->wt.count(lp + ".ffn1.wmx") && h->wt.count(lp + ".ffn2.wmx");
        ln.gamma = g2; ln.beta = b2;
        if (prec == DT_F16) ln.out16 = hbuf.p; else ln.out32 = (float*)hbuf.p;
        ln.mxo_h = nullptr;
        if (ffn_mx && ln_pl) ln_to_planes(ln);
        { KScope ks(h, "layernorm", 0, rc.n_valid * C * 6.0); launch_layernorm(ln, h->stream); }
        MxView fv{};
        if (ffn_mx) {
            fv = mx_view(dmx->ffn, (size_t)rc.R, F);
            fv.logC = 0;                                          // dense [R][F] geometry (F = 1536 is not a power of two)
            p.dtype = DT_MX; p.W_mx = h->wt[lp + ".ffn1.wmx"].ptr; p.mx_scratch = dmx->scratch; p.mx_scratch_size = dmx->scratch_bytes;
            if (ln_pl) planes_in(p);
            mx_out(p, fv, 1.0f);
        } else if (prec == DT_F16) p.out16 = ffn.p; else p.out32 = (float*)ffn.p;
        if (gemm(h, ffn_mx ? (std::string(pre) + "_mx_gemm").c_str() : (kn + "_gemm").c_str(), p, rc.n_valid)) return -1;
        p = gemm_defaults();
        p.dtype = prec; p.A = ffn.p; p.lda = F; p.W = wf2; p.bias = bf2; p.M = rc.R; p.N = C; p.K = F; p.taps = kf; p.center = (kf - 1) / 2;
        p.row_valid = rc.valid; p.res = x.p; p.res_dtype = DT_F32; p.ldres = C; p.out32 = (float*)x.p; p.ldo = C;
        if (prec == DT_F32 && tok_weights(h, lp + ".ffn2.w", p)) return -1;
        if (!dmx && !strcmp(pre, "enc")) tok_splitk(h, p);
        if (ffn_mx) { p.dtype = DT_MX; p.W_mx = h->wt[lp + ".ffn2.wmx"].ptr; mx_in(p, fv, F); }
        if (gemm(h, ffn_mx ? (std::string(pre) + "_mx_gemm").c_str() : (kn + "_gemm").c_str(), p, rc.n_valid)) return -1;
        if (layer_taps) HIPCHK(h, hipMemcpyAsync((*layer_taps)[i].p, x.p, x.bytes, hipMemcpyDeviceToDevice, h->stream));
    }
    WPTR(ga, float, sp + ".after.g"); WPTR(ba, float, sp + ".after.b");
    LayerNormParams ln{};
    ln.x = (const float*)x.p; ln.ldx = C; ln.rows = rc.R; ln.C = C; ln.gamma = ga; ln.beta = ba; ln.eps = 1e-12f;
    ln.row_valid = rc.valid; ln.ldo = C;
    if (prec == DT_F16) { ln.out16 = y.p; ln.out32 = y32_tap; } else { ln.out32 = (float*)y.p; }
    { KScope ks(h, "layernorm", 0, rc.n_valid * C * 6.0); launch_layernorm(ln, h->stream); }
    return 0;
}

// Variance / duration predictor (reference modules/variance.py:36-56, 101-124): n x [conv k3 -> ReLU -> LN] -> Linear(C,1)
int run_predictor(ev_handle* h, const char* name, int layers, const RowCtx& rc, const Buf& xin, Buf& t1, Buf& t2, float* out_rows,
                  hipStream_t st = nullptr) {
    if (!st) st = h->stream;
    const int C = h->cfg.hidden;
    const std::string sp(name);
    const void* cur = xin.p;
    for (int i = 0; i < layers; ++i) {
        const std::string lp = sp + "." + std::to_string(i);
        WPTR(w, char, lp + ".conv.w32"); WPTR(b, float, lp + ".conv.b");
        // kernel size = the packed weight's tap dimension ([C][k][C]): duration / pitch / energy predictors have their own sizes in
        // the reference (model_open_source.py:46-76: duration_kernel_size, variance_kernel_size, energy hard-coded to 3)
        const int k = (int)W(h, lp + ".conv.w32")->dims[1];
        if ((k - 1) / 2 > GAP) return fail(h, "%s: kernel %d needs a halo of %d rows > the %d gap rows between utterances", lp.c_str(), k, (k - 1) / 2, GAP);
        WPTR(g, float, lp + ".ln.g"); WPTR(be, float, lp + ".ln.b");
        ConvGemmParams p = gemm_defaults();
        p.dtype = DT_F32; p.A = cur; p.lda = C; p.W = w; p.bias = b; p.M = rc.R; p.N = C; p.K = C; p.taps = k; p.center = (k - 1) / 2;
        p.row_valid = rc.valid; p.act = ACT_RELU; p.out32 = (float*)t1.p; p.ldo = C;
        if (tok_weights(h, lp + ".conv.w", p)) return -1;
        if (gemm(h, "variance_f32_gemm", p, rc.n_valid, st)) return -1;
        LayerNormParams ln{};
        ln.x = (const float*)t1.p; ln.ldx = C; ln.rows = rc.R; ln.C = C; ln.gamma = g; ln.beta = be; ln.eps = 1e-12f;
        ln.row_valid = rc.valid; ln.ldo = C;
        if (i + 1 < layers) {
            ln.out32 = (float*)t2.p;
        } else {
            WPTR(lw, float, sp + ".lin.w");
            float lbv;
            if (get_scalar(h, sp + ".lin.b", &lbv)) return -1;
            ln.dot_w = lw; ln.dot_b = lbv; ln.dot_out = out_rows;
        }
        { KScope ks(h, "layernorm", 0, rc.n_valid * C * 8.0, st); launch_layernorm(ln, st); }
        cur = t2.p;
    }
    return 0;
}

// Generator schedule of one call (make_voc_plan, before the arena passes): per up stage the kernel of the up-conv and of every ResBlock pair, how
// the running MRF sum travels and how the stage's ResBlocks are issued.  plan_vocoder sizes the workspace from it and run_vocoder executes it.
enum class UpKind { F16, Split, MxPlanes, MxScratch };   // MX up-conv: operand planes written by the previous stage / by the planes kernel into the scratch
enum class MrfMode { F16Branches, Planes, F32 };         // rb0, rb1 as fp16 branches added by rb2 / a partial plane set / an fp32 running sum
enum class Issue { Serial, Streams, Grouped };           // ResBlock after ResBlock / three streams / same-level convs as grouped launches
enum class PairKind { FusedC64Mx, FusedC32Mx, Fused, MxLayers, Layers };
struct VocStage {
    int cin, cout, s, U_in, rows_in, rows_out;           // U_in: the upsampling factor in front of the stage
    UpKind up; bool stage_mx, rpl, next_up_mx; MrfMode mrf; Issue issue;
    PairKind pair[3][4];                                 // [ResBlock][dilation]
};
struct VocPlan { bool mx, x3, keep; int Rf, U; size_t scratch_bytes; VocStage st[4]; };

struct VocBufs {
    Buf pre, xu[4], tmp[3], rba[3], rbb[3], nxt[4], mrf32, mrf16a, mrf16b, wavrows; Buf mrf_tap[4]; Buf pre_tap;
    // EV_PREC_MX: plane sets of the up-conv output, conv1's output, the two alternating ResBlock states and the stage output; the
    // planes-kernel scratch of the one fp32 tensor an MX launch reads (conv_pre's output)
    // (tmp / rba / rbb: one set per ResBlock of a stage when the plan issues them on three streams; pl_t / pl_a / pl_b: also when it issues an MX stage
    // as grouped levels; else only [0])
    // pl_mrf: the running MRF sum of a stage as a PARTIAL plane set (hi plane, remainder codes, their scales; ev_config.mx_mrf == 0)
    PlaneBuf pl_xu, pl_t[3], pl_a[3], pl_b[3], pl_nxt, pl_mrf; char* mx_scratch = nullptr;
    float* wav = nullptr; int16_t* wav_i16 = nullptr;    // the packed waveform
};

// weights of one generator conv: fp16 (also the "hi" part of the split) and, in the split-precision mode, the "lo" part
int voc_weights(ev_handle* h, const std::string& base /* e.g. "voc.rb3.c1.0" */, bool x3, ConvGemmParams& p, bool mx = false) {
    const WeightEntry* w = W(h, base + ".w16");
    const WeightEntry* b = W(h, base + ".b");
    if (!w || !b) return -1;
    p.W = w->ptr; p.bias = reinterpret_cast<const float*>(b->ptr);
    if (x3) {
        const WeightEntry* lo = W(h, base + ".w16l");
        if (!lo) return -1;
        p.dtype = DT_F32S; p.W_lo = lo->ptr;
        if (mx) {           // layers with fp4 planes in the blob (N, K % 128 == 0, 3 / 7 / 11 taps: packer.py) take the MX kernel
            auto it = h->wt.find(base + ".wmx");
            if (it == h->wt.end()) it = h->wt.find(base + ".wcmx");          // C = 64 layers: conv_c64_mx_kernel's planes (fp32 in / out)
            if (it != h->wt.end()) { p.dtype = DT_MX; p.W_mx = it->second.ptr; }
        }
    } else {
        p.dtype = DT_F16; p.W_lo = nullptr;
    }
    return 0;
}

int make_voc_plan(ev_handle* h, int Rf, VocPlan& vp) {
    const ev_config& c = h->cfg;
    // EV_PREC_MX: the split-precision data flow (fp32 raw module outputs), but every layer with N, K % 128 == 0 evaluates its products as
    // one fp16 MFMA + two block-scaled fp4 MFMAs (conv_gemm_mx_kernel) and reads its operand as the plane set its producer's epilogue wrote.
    const bool mx = c.vocoder_precision == EV_PREC_MX, x3 = c.vocoder_precision == EV_PREC_X3 || mx, keep = c.keep_stages != 0;
    auto has_wt = [&](const std::string& name) { return h->wt.find(name) != h->wt.end(); };
    auto has_mx = [&](const std::string& base) { return mx && (has_wt(base + ".wmx") || has_wt(base + ".wcmx")); };
    auto k3711 = [](int k) { return k == 3 || k == 7 || k == 11; };
    int seen = 0;          // the ResBlocks' kernel sizes as a set: {3, 7, 11} is what the grouped launches take
    for (int j = 0; j < c.n_rb; ++j) seen |= c.rb_kernels[j] == 3 ? 1 : (c.rb_kernels[j] == 7 ? 2 : (c.rb_kernels[j] == 11 ? 4 : 8));
    vp.mx = mx; vp.x3 = x3; vp.keep = keep; vp.Rf = Rf;
    vp.scratch_bytes = (mx && c.up_init_ch % 128 == 0) ? mx_scratch_bytes(Rf, c.up_init_ch) : 0;
    bool prev_planes = false;           // the previous stage's epilogue writes the plane set of lrelu(its output)
    int ch = c.up_init_ch, U = 1;
    for (int i = 0; i < c.n_up; ++i) {
        VocStage& st = vp.st[i];
        const int s = c.up_rates[i], cout = ch / 2;
        st.cin = ch; st.cout = cout; st.s = s; st.U_in = U; st.rows_in = Rf * U; st.rows_out = st.rows_in * s;
        auto rb = [&](int j) { return "voc.rb" + std::to_string(i * c.n_rb + j); };
        if (!x3) st.up = UpKind::F16;
        else if (!has_mx("voc.up" + std::to_string(i))) st.up = UpKind::Split;
        else if (prev_planes) st.up = UpKind::MxPlanes;
        else if (vp.scratch_bytes && vp.scratch_bytes >= mx_scratch_bytes(st.rows_in, ch)) st.up = UpKind::MxScratch;
        else st.up = UpKind::Split;
        // the ResBlocks of this stage run on the MX kernel iff the up-conv does and all their convs have fp4 planes (shape rule of the packer)
        st.stage_mx = (st.up == UpKind::MxPlanes || st.up == UpKind::MxScratch) && cout % 64 == 0;     // (C = 64: conv_c64_mx_kernel, the same plane-set data flow)
        for (int j = 0; st.stage_mx && j < c.n_rb; ++j) st.stage_mx = has_mx(rb(j) + ".c1.0");
        // MX stage: the residual stream of a ResBlock exists only as the plane set of lrelu(x, .1) its conv1 reads -- conv2's epilogue rebuilds x from
        // the fp16 hi plane + the fp4 remainder codes (ConvGemmParams::res_x4), so neither the up-conv nor a conv2 inside a ResBlock writes an fp32
        // copy (tools/precision_study_mx.py: 3.4e-4 -> 4.4e-4; 8.7 instead of 14.1 bytes per element and conv2 launch).  Default since round 4 (the
        // round-3 driver run XPASSed every reference fixture through it); ev_config.mx_residual = 1 restores the separate fp32 residual tensor.
        st.rpl = st.stage_mx && c.mx_residual == 0;
        st.next_up_mx = st.stage_mx && i + 1 < c.n_up && has_mx("voc.up" + std::to_string(i + 1));
        // MRF sum as partial plane sets (conv_gemm_mx_kernel stages, i.e. >= 128 channels): rb0's last conv writes out_scale * x as fp16 hi plane + fp4 remainder
        // codes, rb1's adds that to its own and rewrites it in place, rb2's adds it and writes the next up-conv's plane set: 2.53 instead of 4 bytes per element
        // and transfer (16 -> 10.1 bytes per stage-output element; tools/precision_study_mx.py: 4.17e-4 -> 4.22e-4 on the zero-mean recipe)
        // (round 6: also at C = 64 -- conv_gemm_mx64_kernel has the same epilogue variants, the fused k = 3 pair writes the partial set itself)
        bool mrf_pl = st.rpl && !keep && c.mx_mrf == 0 && c.n_rb == 3 && cout % 64 == 0 && st.next_up_mx;
        for (int j = 0; mrf_pl && j < c.n_rb; ++j) {
            const int k = c.rb_kernels[j];
            mrf_pl = k3711(k);
            // C = 64, k = 3: only the fused pair kernel writes / the streamed k = 7 / 11 kernel reads partial sets (conv_c64_mx_kernel does neither), and the pair
            // kernel has no plane-set accumulate-in: the k = 3 ResBlock must be the first of the stage and run fused
            if (mrf_pl && cout == 64 && k == 3)
                mrf_pl = j == 0 && c.fused_pairs == 0 && c.rb_dils[j][c.n_rb_dils - 1] <= 8 && has_wt(rb(j) + ".c2." + std::to_string(c.n_rb_dils - 1) + ".wcmx");
        }
        // MRF: fp16 mode with three ResBlocks (the reference config): the first two scaled branches are kept in fp16 and the third adds them in its
        // fp32 epilogue (half the HBM traffic of an fp32 running sum; the two extra fp16 roundings are of the size of the one the stage output gets
        // anyway).  Any other count, and the split-precision mode, use the fp32 running sum.
        st.mrf = (c.n_rb == 3 && !x3) ? MrfMode::F16Branches : mrf_pl ? MrfMode::Planes : MrfMode::F32;
        // The three ResBlocks of a stage only share the stage input and meet again in the MRF sum: the first two run on
        // auxiliary streams beside the third (its last conv waits for both).  A k = 3 chain is HBM-bound and a k = 11 chain
        // MFMA-bound, so their workgroups complement each other on a CU and fill each other's launch tails.  Profiled steps
        // (per-launch events) stay on one stream.  (Split-precision mode: the MRF sum is a running fp32 accumulator shared
        // by the three ResBlocks, so they run in order on the handle's stream.)
        // In the mx mode only small batches (Rf <= 2048 rows; single utterances: the reference's own call pattern) do so: there a generator launch is a
        // handful of tiles whose K loops are sequential chains (tools/probe_b1.py: 39 conv launches of ~35 us each for 64 phonemes while 240 of 256 CUs
        // idle); the running fp32 sum keeps its order rb0, rb1, rb2 through events, so the result has the same bits as the serial order.  At full batches a
        // launch fills the chip and streams only reorder the same work (measured in round 3: 54.99 vs 54.56 ms).
        const bool conc = c.n_rb == 3 && (!x3 || (mx && !keep && Rf <= 2048)) && !h->profiling && c.vocoder_streams != 1 && h->aux[0] && h->aux[1];
        // Large batches on the conv_gemm_mx_kernel stages (round 6, ev_config.mx_group == 0): the three ResBlocks advance level by level -- the three conv1 of a
        // pair position, then the three conv2 -- each level ONE grouped launch (launch_conv_gemm_group3: a launch of its own costs every conv 30-50 us of ramp and
        // tail); the last conv2 of each ResBlock stays a launch of its own (the running MRF sum orders them).  Each ResBlock has its own intermediates; descriptors
        // are built in the usual ResBlock order and issued level by level.  Same kernels' code on the same data: the same bits.  A small batch that may not
        // use the streams (profiled, vocoder_streams = 1) is issued this way too.
        const bool grp = st.rpl && !keep && !conc && c.mx_group == 0 && c.n_rb == 3 && cout % 128 == 0 && seen == 7;
        st.issue = conc ? Issue::Streams : grp ? Issue::Grouped : Issue::Serial;
        for (int j = 0; j < c.n_rb; ++j) {
            const int k = c.rb_kernels[j];
            for (int d = 0; d < c.n_rb_dils; ++d) {
                const int dil = c.rb_dils[j][d];
                const std::string c1 = rb(j) + ".c1." + std::to_string(d), c2 = rb(j) + ".c2." + std::to_string(d);
                PairKind& pk = st.pair[j][d];
                // EV_PREC_MX at C = 64, k = 3 with the residual in the planes: the pair in one persistent kernel (ev_pair64_mx.h), plane sets in / out -- xt
                // never reaches HBM and the residual comes from the slab conv1 reads (6.1 instead of 14.8 bytes per element; the k = 3 chain of stage 2 is HBM-bound)
                if (st.rpl && cout == 64 && k == 3 && dil <= 8 && c.fused_pairs == 0 && has_wt(c1 + ".wcmx") && has_wt(c2 + ".wcmx")) pk = PairKind::FusedC64Mx;
                // EV_PREC_MX at C = 32: the whole pair in one persistent kernel (ev_pair_mx.h), x fp32 in, fp32 out
                else if (mx && cout == 32 && k3711(k) && (k - 1) * (dil + 1) <= 64 && has_wt(c1 + ".wpmx") && has_wt(c2 + ".wpmx") && c.fused_pairs == 0) pk = PairKind::FusedC32Mx;
                // fused fp16 pair kernels: C = 32 (every k) and C = 64 with k = 3 (the HBM-bound end of the generator)
                else if (!st.stage_mx) pk = !x3 && ((cout == 32 && k3711(k)) || (cout == 64 && k == 3)) && c.fused_pairs == 0 ? PairKind::Fused : PairKind::Layers;
                else if (!has_mx(c1) || !has_mx(c2)) return fail(h, "MX stage: %s has no fp4 planes", (has_mx(c1) ? c2 : c1).c_str());
                else pk = PairKind::MxLayers;
            }
        }
        prev_planes = st.next_up_mx;
        ch = cout; U *= s;
    }
    vp.U = U;
    return 0;
}

// ConvTranspose1d(k = 2s, pad = s/2) of stage i == 3-tap conv with N = s * C_out, viewed as [rows_in*s][C_out] (models.py:119)
int voc_up(ev_handle* h, const VocPlan& vp, int i, const void* prev, VocBufs& vb, double n_frames) {
    const VocStage& st = vp.st[i];
    ConvGemmParams p = gemm_defaults();
    if (voc_weights(h, "voc.up" + std::to_string(i), vp.x3, p, vp.mx)) return -1;
    p.A = prev; p.lda = st.cin; p.M = st.rows_in; p.N = st.s * st.cout; p.K = st.cin; p.taps = 3; p.center = 1;
    if (st.cout % 64 == 0 && st.s % 2 == 0) p.polyphase_cout = st.cout;          // (conv_gemm_mx_kernel skips the zero tap of each output phase; other kernels ignore the hint)
    p.row_valid = h->d_frm_valid; p.valid_shift = ilog2(st.U_in); p.ldo = st.s * st.cout;
    if (vp.x3) { p.pro_lrelu = 1; p.pro_slope = 0.1f; p.out32 = (float*)vb.xu[i].p; }     // models.py:118 (the fp16 path has it in the producer's epilogue)
    else p.out16 = vb.xu[i].p;
    if (st.up == UpKind::MxPlanes) mx_in(p, mx_view(vb.pl_nxt, st.rows_in, st.cin), st.cin);            // the previous stage's epilogue wrote lrelu(prev) as planes
    else if (st.up == UpKind::MxScratch) { p.mx_scratch = vb.mx_scratch; p.mx_scratch_size = vp.scratch_bytes; }
    else if (vp.x3) p.dtype = DT_F32S;                  // (an up-conv with planes but no plane-set input: the split kernel)
    if (st.stage_mx) mx_out(p, mx_view(vb.pl_xu, (size_t)st.rows_out, st.cout), 0.1f);      // lrelu(x) of models.py:51, shared by the three ResBlocks
    if (st.rpl && !vp.keep) p.out32 = nullptr;                   // (kept stages still get the raw up-conv output: the voc_up tap)
    const char* name = p.dtype == DT_MX ? (p.N == 64 && p.K == 64 ? "voc_conv_c64_mx" : "voc_conv_gemm_mx") : vp.x3 ? "voc_conv_gemm_x3" : "voc_conv_gemm_f16";
    return gemm(h, name, p, n_frames * st.U_in, nullptr, 2.0 / 3.0);
}

// MRF: xs += resblock(x); x = xs / num_kernels (models.py:121-126), then the next leaky_relu -- the outputs of ResBlock j's last conv in stage i
void voc_mrf_epilogue(ConvGemmParams& p, const ev_config& c, const VocPlan& vp, int i, int j, VocBufs& vb) {
    const VocStage& st = vp.st[i];
    p.out_scale = 1.0f / (float)c.n_rb;
    const MxView mv = st.mrf == MrfMode::Planes ? mx_view(vb.pl_mrf, (size_t)st.rows_out, st.cout) : MxView{};
    if (st.mrf == MrfMode::F16Branches && j == 2) { p.add16_a = vb.mrf16a.p; p.add16_b = vb.mrf16b.p; p.ldadd = st.cout; }
    if (st.mrf == MrfMode::Planes && j > 0) { p.acc_h = mv.h; p.acc_x4 = mv.q4[1]; p.acc_xs = mv.qs[1]; p.acc_xs_stride = mv.qs_stride; p.ldacc = st.cout; }
    if (st.mrf == MrfMode::F32 && j > 0) { p.acc32 = (const float*)vb.mrf32.p; p.ldacc = st.cout; }
    if (j + 1 < c.n_rb) {
        if (st.mrf == MrfMode::F16Branches) p.out16 = (j == 0) ? vb.mrf16a.p : vb.mrf16b.p;
        else if (st.mrf == MrfMode::Planes) { mx_out(p, mv, 1.0f); p.mxo_partial = 1; }
        else p.out32 = (float*)vb.mrf32.p;
    } else if (vp.x3) {
        p.out32 = (float*)vb.nxt[i].p;               // raw MRF mean (= the voc_mrf tap); consumers apply the leaky-relu
        if (st.next_up_mx) {
            mx_out(p, mx_view(vb.pl_nxt, (size_t)st.rows_out, st.cout), 0.1f);      // ... or read these planes (models.py:118)
            if (st.rpl && !vp.keep) p.out32 = nullptr;                              // the next up-conv reads only the planes: no fp32 copy of the stage output
        }
    } else {
        p.post_lrelu = 1; p.post_slope = i == c.n_up - 1 ? 0.01f : 0.1f;   // models.py:118 / :127
        p.out16 = vb.nxt[i].p;
        if (vp.keep) { p.out32 = (float*)vb.mrf_tap[i].p; p.out32_before_post = 1; }
    }
}

// One (ResBlock j, dilation d) pair of stage i, as the plan's kind says: xt = lrelu(c1(lrelu(x))), x = c2(xt) + x (models.py:51-56).  pend (grouped
// levels): receives the two descriptors instead of launching them.
int voc_pair(ev_handle* h, const VocPlan& vp, int i, int j, int d, VocBufs& vb, double valid_out, ConvGemmParams* pend) {
    const ev_config& c = h->cfg;
    const VocStage& st = vp.st[i];
    const PairKind kind = st.pair[j][d];
    const int k = c.rb_kernels[j], dil = c.rb_dils[j][d], cout = st.cout, shift = ilog2(st.U_in * st.s);
    const size_t rows = st.rows_out;
    const bool conc = st.issue == Issue::Streams;
    const int bj = st.issue == Issue::Serial ? 0 : j;
    hipStream_t sj = (conc && j < 2) ? h->aux[j] : h->stream;
    const std::string rb = "voc.rb" + std::to_string(i * c.n_rb + j), c1 = rb + ".c1." + std::to_string(d), c2 = rb + ".c2." + std::to_string(d);
    const char* gname = vp.x3 ? "voc_conv_gemm_x3" : "voc_conv_gemm_f16";
    const char* mxname = cout == 64 ? "voc_conv_c64_mx" : "voc_conv_gemm_mx";
    // x of this pair (fp32 / fp16) and the plane set of lrelu(x, .1): conv1's operand and, with rpl, conv2's residual
    const void* xcur = d == 0 ? vb.xu[i].p : ((d - 1) % 2 == 0 ? vb.rba[bj].p : vb.rbb[bj].p);
    const PlaneBuf& xin = d == 0 ? vb.pl_xu : ((d - 1) % 2 == 0 ? vb.pl_a[bj] : vb.pl_b[bj]);
    ConvGemmParams p = gemm_defaults();
    if (kind == PairKind::MxLayers) {
        // MX stage: xt only ever exists as conv2's operand planes; x travels as fp32 (the residual) + the planes of lrelu(x); with rpl as the planes only
        if (voc_weights(h, c1, vp.x3, p, true)) return -1;
        mx_in(p, mx_view(xin, rows, cout), cout);
        p.M = st.rows_out; p.N = cout; p.K = cout; p.taps = k; p.dil = dil; p.center = (k - 1) / 2;
        p.row_valid = h->d_frm_valid; p.valid_shift = shift; p.act = ACT_LRELU; p.act_slope = 0.1f; p.ldo = cout;
        mx_out(p, mx_view(vb.pl_t[bj], rows, cout), 1.0f);
        if (pend) pend[0] = p;
        else if (gemm(h, mxname, p, valid_out, sj)) return -1;
    } else if (kind == PairKind::Layers) {
        if (voc_weights(h, c1, vp.x3, p, false)) return -1;      // (no plane-set input here: DT_MX would only fall back to the split kernel)
        p.A = xcur; p.lda = cout; p.M = st.rows_out; p.N = cout; p.K = cout;
        p.taps = k; p.dil = dil; p.center = (k - 1) / 2; p.row_valid = h->d_frm_valid; p.valid_shift = shift;
        p.pro_lrelu = 1; p.pro_slope = 0.1f; p.act = ACT_LRELU; p.act_slope = 0.1f; p.ldo = cout;
        if (vp.x3) p.out32 = (float*)vb.tmp[bj].p; else p.out16 = vb.tmp[bj].p;
        if (gemm(h, gname, p, valid_out, sj)) return -1;
    }
    // conv2 (the fused kinds: the epilogue of the pair kernel)
    p = gemm_defaults();
    if (voc_weights(h, c2, vp.x3, p, st.stage_mx)) return -1;
    p.A = vb.tmp[bj].p; p.lda = cout; p.M = st.rows_out; p.N = cout; p.K = cout;
    if (st.stage_mx) mx_in(p, mx_view(vb.pl_t[bj], rows, cout), cout);
    p.taps = k; p.dil = 1; p.center = (k - 1) / 2; p.row_valid = h->d_frm_valid; p.valid_shift = shift;
    p.res = xcur; p.res_dtype = vp.x3 ? DT_F32 : DT_F16; p.ldres = cout; p.ldo = cout;
    if (st.rpl) {
        const MxView xv = mx_view(xin, rows, cout);
        p.res = xv.h; p.res_dtype = DT_MX; p.res_x4 = xv.q4[1]; p.res_xs = xv.qs[1]; p.res_xs_stride = xv.qs_stride; p.res_inv_slope = 10.0f;
    }
    if (d + 1 < c.n_rb_dils) {
        void* dst = (d % 2 == 0) ? vb.rba[bj].p : vb.rbb[bj].p;
        if (!st.rpl || vp.keep) { if (vp.x3) p.out32 = (float*)dst; else p.out16 = dst; }     // (rpl: the next pair reads the planes below; the fp32 copy only feeds stage taps)
        if (st.stage_mx) mx_out(p, mx_view(d % 2 == 0 ? vb.pl_a[bj] : vb.pl_b[bj], rows, cout), 0.1f);     // the next conv1's operand
    } else {
        voc_mrf_epilogue(p, c, vp, i, j, vb);
        if (conc && j == 2) {               // the MRF sum reads the other two branches
            (void)hipStreamWaitEvent(h->stream, h->ev_join[0], 0);
            (void)hipStreamWaitEvent(h->stream, h->ev_join[1], 0);
        }
        // fp32 running sum (split-precision / mx modes): rb1's last conv adds onto what rb0's wrote (the sum keeps the serial order's bits)
        if (conc && vp.x3 && j == 1) (void)hipStreamWaitEvent(h->aux[1], h->ev_join[0], 0);
    }
    if (pend) { pend[1] = p; return 0; }
    if (kind == PairKind::MxLayers || kind == PairKind::Layers) return gemm(h, kind == PairKind::MxLayers ? mxname : gname, p, valid_out, sj);
    // conv1 -> LDS -> conv2 + residual / MRF epilogue in one persistent kernel
    WPTR(w1, char, c1 + ".w16"); WPTR(b1, float, c1 + ".b");
    ResPairParams rp;
    memset(&rp, 0, sizeof rp);
    rp.x = p.res; rp.ldx = cout; rp.w1 = w1; rp.b1 = b1; rp.w2 = p.W; rp.M = p.M; rp.k = k; rp.dil = dil; rp.epi = p;
    const double fl = 2.0 * 2.0 * valid_out * cout * (double)cout * k;
    ConvGemmParams shape = p; shape.dil = dil;
    if (kind == PairKind::FusedC64Mx) {
        WPTR(w1m, char, c1 + ".wcmx");
        const MxView xv = mx_view(xin, rows, cout);
        rp.w1_mx = w1m; rp.w2_mx = p.W_mx;
        rp.epi.mx_x4[0] = xv.q4[0]; rp.epi.mx_x4[1] = xv.q4[1]; rp.epi.mx_xs[0] = xv.qs[0]; rp.epi.mx_xs[1] = xv.qs[1]; rp.epi.mx_xs_stride = xv.qs_stride;
        KScope ks(h, "voc_resblock_pair_c64_mx", fl, valid_out * cout * 3.0625 * 2.0, sj, &shape);
        if (launch_resblock_pair_c64_mx(rp, sj)) return fail(h, "fused MX pair (C = 64): unsupported call (k %d, dil %d)", k, dil);
    } else if (kind == PairKind::FusedC32Mx) {
        WPTR(w1m, char, c1 + ".wpmx"); WPTR(w2m, char, c2 + ".wpmx");
        rp.w1_mx = w1m; rp.w2_mx = w2m; rp.gmax = st.rows_out;
        if (c.mx_act_format != 0) rp.epi.reserved0 |= 16;          // block-scaled fp4 activation operands (rounds 3-5) instead of E5M2
        KScope ks(h, "voc_resblock_pair_c32_mx", fl, valid_out * cout * 4.0 * 2.0, sj, &shape);
        if (launch_resblock_pair_c32_mx(rp, sj)) return fail(h, "fused MX pair: unsupported call (k %d, dil %d)", k, dil);
    } else {
        rp.gmax = st.rows_out;
        KScope ks(h, cout == 32 ? "voc_resblock_pair_c32" : "voc_resblock_pair_c64", fl, valid_out * cout * 2.0 * 2.0, sj, &shape);
        if (cout == 32) launch_resblock_pair_c32(rp, sj);
        else launch_resblock_pair_c64(rp, sj);
    }
    return 0;
}

// The ResBlocks of stage i and their MRF sum into vb.nxt[i], issued as the plan says
int voc_resblocks(ev_handle* h, const VocPlan& vp, int i, VocBufs& vb, double n_frames) {
    const ev_config& c = h->cfg;
    const VocStage& st = vp.st[i];
    const double valid_out = n_frames * st.U_in * st.s;
    const bool conc = st.issue == Issue::Streams, grp = st.issue == Issue::Grouped;
    std::vector<ConvGemmParams> pend(grp ? (size_t)c.n_rb * 2 * c.n_rb_dils : 0);
    if (conc) {
        (void)hipEventRecord(h->ev_fork, h->stream);
        (void)hipStreamWaitEvent(h->aux[0], h->ev_fork, 0);
        (void)hipStreamWaitEvent(h->aux[1], h->ev_fork, 0);
    }
    for (int j = 0; j < c.n_rb; ++j) {
        for (int d = 0; d < c.n_rb_dils; ++d)
            if (voc_pair(h, vp, i, j, d, vb, valid_out, grp ? &pend[((size_t)j * c.n_rb_dils + d) * 2] : nullptr)) return -1;
        if (conc && j < 2) (void)hipEventRecord(h->ev_join[j], h->aux[j]);
    }
    for (int lvl = 0; grp && lvl < 2 * c.n_rb_dils; ++lvl) {
        ConvGemmParams ps[3];
        for (int j = 0; j < 3; ++j) ps[j] = pend[((size_t)j * c.n_rb_dils) * 2 + lvl];
        if (lvl + 1 < 2 * c.n_rb_dils) {
            if (gemm_group3(h, "voc_conv_gemm_mx", ps, valid_out)) return -1;
        } else {
            for (int j = 0; j < 3; ++j)
                if (gemm(h, "voc_conv_gemm_mx", ps[j], valid_out)) return -1;
        }
    }
    return 0;
}

// HiFi-GAN generator (reference models/hifigan/models.py:115-131) on channels-last rows.
// vocoder_precision F16: fp16 activations, every leaky-relu fused into the producer (post_lrelu) or the consumer's staging.
// vocoder_precision X3:  fp32 activations, split-precision products; every stored tensor is the RAW module output of the
// reference (so the Appendix-C taps are the buffers themselves) and each consumer applies its leaky-relu while staging.
int run_vocoder(ev_handle* h, const VocPlan& vp, const Buf& melin, double n_frames, VocBufs& vb) {
    const ev_config& c = h->cfg;
    const bool x3 = vp.x3;
    ConvGemmParams p = gemm_defaults();
    if (voc_weights(h, "voc.pre", x3, p)) return -1;
    p.A = melin.p; p.lda = MEL_PAD; p.M = vp.Rf; p.N = c.up_init_ch; p.K = MEL_PAD;
    p.taps = 7; p.center = 3; p.row_valid = h->d_frm_valid; p.valid_shift = 0; p.ldo = c.up_init_ch;
    if (x3) p.out32 = (float*)vb.pre.p;
    else {
        p.out16 = vb.pre.p;
        p.post_lrelu = 1; p.post_slope = 0.1f;      // leaky_relu(0.1) of models.py:118 fused into the producer
        if (vp.keep) { p.out32 = (float*)vb.pre_tap.p; p.out32_before_post = 1; }
    }
    if (gemm(h, x3 ? "voc_conv_gemm_x3" : "voc_conv_gemm_f16", p, n_frames)) return -1;
    for (int i = 0; i < c.n_up; ++i)
        if (voc_up(h, vp, i, i ? vb.nxt[i - 1].p : vb.pre.p, vb, n_frames) || voc_resblocks(h, vp, i, vb, n_frames)) return -1;
    const void* prev = vb.nxt[c.n_up - 1].p;
    const int ch = vp.st[c.n_up - 1].cout;
    WPTR(wpost, float, "voc.post.w");
    float bpv;
    if (get_scalar(h, "voc.post.b", &bpv)) return -1;
    {
        KScope ks(h, "voc_conv_post", 2.0 * n_frames * vp.U * ch * 7, n_frames * vp.U * (ch * (double)(x3 ? 4 : 2) + 4.0));
        launch_conv_post(prev, x3 ? 1 : 0, ch, wpost, bpv, 7, x3 ? 0.01f : 1.0f, h->d_frm_valid, ilog2(vp.U), (float*)vb.wavrows.p, vp.Rf * vp.U, ch, h->stream);
    }
    return 0;
}

// the generator's share of the frame arena, as far as the plan uses it, and the packed waveform behind it
void plan_vocoder(ArenaPlan& ap, const VocPlan& vp, VocBufs& vb) {
    const ev_config& c = ap.h->cfg;
    const bool x3 = vp.x3, keep = vp.keep;
    const int Rf = vp.Rf;
    const size_t ves = x3 ? 4 : 2;
    vb.pre = ap.rows(Rf, c.up_init_ch, ves);
    if (keep && !x3) vb.pre_tap = ap.rows(Rf, c.up_init_ch, 4);
    size_t max_elems = 0;
    bool streams = false, planes_per_rb = false, mrf16 = false, mrf32 = false, pl_mrf = false, scratch = false;
    for (int i = 0; i < c.n_up; ++i) {
        const VocStage& st = vp.st[i];
        max_elems = std::max(max_elems, (size_t)st.rows_out * st.cout);
        streams |= st.issue == Issue::Streams;
        planes_per_rb |= st.stage_mx && st.issue != Issue::Serial;
        mrf16 |= st.mrf == MrfMode::F16Branches; mrf32 |= st.mrf == MrfMode::F32; pl_mrf |= st.mrf == MrfMode::Planes;
        scratch |= st.up == UpKind::MxScratch;
    }
    // stage buffers are re-used across stages unless taps are kept
    for (int i = 0; keep && i < c.n_up; ++i) {
        vb.xu[i] = ap.rows((size_t)vp.st[i].rows_out, vp.st[i].cout, ves);
        vb.nxt[i] = ap.rows((size_t)vp.st[i].rows_out, vp.st[i].cout, ves);
        if (!x3) vb.mrf_tap[i] = ap.rows((size_t)vp.st[i].rows_out, vp.st[i].cout, 4);
    }
    // row pitch differs per stage, so size by elements with the largest pad (C = 256 rows of slack)
    auto mk2 = [&](size_t es) { Buf b; const size_t pad = (size_t)PAD_ROWS * 512 * es; b.bytes = max_elems * es; b.base = ap.take(pad + b.bytes + pad); b.p = ap.dry ? nullptr : b.base + pad; return b; };
    if (!keep) {
        const Buf shared_xu = mk2(ves), shared_nxt[2] = {mk2(ves), mk2(ves)};
        for (int i = 0; i < c.n_up; ++i) { vb.xu[i] = shared_xu; vb.nxt[i] = shared_nxt[i & 1]; }
    }
    for (int j = 0; j < (streams ? 3 : 1); ++j) { vb.tmp[j] = mk2(ves); vb.rba[j] = mk2(ves); vb.rbb[j] = mk2(ves); }
    if (mrf16) { vb.mrf16a = mk2(2); vb.mrf16b = mk2(2); }
    if (mrf32) vb.mrf32 = mk2(4);
    vb.wavrows = ap.rows((size_t)Rf * vp.U, 1, 4);
    if (vp.mx) {
        // plane sets, re-used across the stages that run on the MX kernel (C % 64 == 0): sized by the largest
        size_t hb = 0, qb = 0, sb = 0;
        for (int i = 0; i < c.n_up; ++i) {
            const int ch = vp.st[i].cout;
            if (ch % 64) continue;
            const size_t R = (size_t)vp.st[i].rows_out + 2 * MX_PAD;
            hb = std::max(hb, R * ch * 2); qb = std::max(qb, R * (ch / 2)); sb = std::max(sb, (size_t)std::max(1, ch / 128) * R * 4);
        }
        std::vector<PlaneBuf*> sets = {&vb.pl_xu, &vb.pl_nxt};
        if (pl_mrf) sets.push_back(&vb.pl_mrf);
        for (int j = 0; j < (planes_per_rb ? 3 : 1); ++j) { sets.push_back(&vb.pl_t[j]); sets.push_back(&vb.pl_a[j]); sets.push_back(&vb.pl_b[j]); }
        for (PlaneBuf* b : sets) {
            if (!hb) break;
            b->h = ap.take(hb);
            for (int i = 0; i < 2; ++i) { b->q4[i] = ap.take(qb); b->qs[i] = ap.take(sb); }
        }
        vb.mx_scratch = scratch ? ap.take(vp.scratch_bytes) : nullptr;
    }
    vb.wav = ap.arr<float>((size_t)ap.h->total_frames * vp.U);
    vb.wav_i16 = ap.arr<int16_t>((size_t)ap.h->total_frames * vp.U);
}

// frame rows of a batch: GAP rows before every utterance and after the last, padded to ROW_ALIGN
int frame_rows(const int32_t* mel_lens, int B) {
    int64_t rows = GAP;
    for (int b = 0; b < B; ++b) rows += mel_lens[b] + GAP;
    return (int)align_up((size_t)rows, ROW_ALIGN);
}

// frame layout from mel lengths (host) -> device maps; returns Rf
int build_frame_layout(ev_handle* h, ArenaPlan& ap, bool dry, int B) {
    int64_t rows = GAP;
    h->frm_off.resize(B);
    h->mel_offs.assign(B + 1, 0);
    for (int b = 0; b < B; ++b) {
        h->frm_off[b] = (int32_t)rows;
        rows += h->mel_lens[b] + GAP;
        h->mel_offs[b + 1] = h->mel_offs[b] + h->mel_lens[b];
    }
    h->total_frames = h->mel_offs[B];
    const int Rf = frame_rows(h->mel_lens.data(), B);
    h->d_frm_seq = ap.arr<int32_t>(Rf); h->d_frm_pos = ap.arr<int32_t>(Rf); h->d_frm_valid = ap.arr<uint8_t>(Rf);
    h->d_frm_off = ap.arr<int32_t>(B);
    h->d_frm_len = ap.arr<int32_t>(B);
    if (!dry) {
        // only the B first-row offsets and lengths travel; the per-row maps are built on the device (no host loop over rows, no
        // synchronisation: the pinned frame region [PIN_FRAME, ...) is not rewritten before the call's final synchronisation)
        int32_t* off = (int32_t*)(h->pinned + PIN_FRAME); int32_t* len = off + B;
        for (int b = 0; b < B; ++b) { off[b] = h->frm_off[b]; len[b] = h->mel_lens[b]; }
        (void)hipMemcpyAsync(h->d_frm_off, off, (size_t)B * 4, hipMemcpyHostToDevice, h->stream);
        (void)hipMemcpyAsync(h->d_frm_len, len, (size_t)B * 4, hipMemcpyHostToDevice, h->stream);
        launch_row_maps(h->d_frm_off, h->d_frm_len, B, h->d_frm_seq, h->d_frm_pos, h->d_frm_valid, Rf, h->stream);
    }
    return Rf;
}

// gather per-utterance valid rows of a row-layout buffer into a packed fp32 device buffer
int pack_level(ev_handle* h, const void* src, int dtype, int ld, int C, int level_shift, bool token_level, float* dst, int64_t* d_scratch3B) {
    const int B = h->B;
    // host staging lives in the handle (a ring of slots: one call packs at most 4 levels + the stage taps of a test) so that no
    // synchronisation is needed for it to outlive the asynchronous copies
    h->pack_slot = (h->pack_slot + 1) % 8;
    std::vector<int64_t>& host = h->pack_host[h->pack_slot];
    std::vector<int32_t>& rows32 = h->pack_rows[h->pack_slot];
    host.assign(3 * (size_t)B, 0);
    rows32.assign(B, 0);
    int64_t max_rows = 0, out = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t n = token_level ? h->tok_len[b] : ((int64_t)h->mel_lens[b] << level_shift);
        host[b] = token_level ? h->tok_off[b] : ((int64_t)h->frm_off[b] << level_shift);
        host[B + b] = out;
        rows32[b] = (int32_t)n;
        out += n; max_rows = std::max(max_rows, n);
    }
    int64_t* d_row_off = d_scratch3B; int64_t* d_out_off = d_scratch3B + B; int32_t* d_rows = (int32_t*)(d_scratch3B + 2 * B);
    HIPCHK(h, hipMemcpyAsync(d_row_off, host.data(), (size_t)2 * B * 8, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_rows, rows32.data(), (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
    launch_pack_rows(src, dtype, ld, C, d_row_off, d_out_off, d_rows, B, max_rows, dst, h->stream);
    return 0;
}

void add_tap(ev_handle* h, const char* name, const void* ptr, int dtype, int ld, int C, int level, int shift) {
    Tap t{ptr, dtype, ld, C, level, shift};
    h->taps[name] = t;
}

}  // namespace

// =================================================================== C ABI

extern "C" {

void ev_default_config(ev_config* c) {
    memset(c, 0, sizeof *c);
    c->abi_version = EV_ABI_VERSION;
    c->n_vocab = 502; c->n_speaker = 2014; c->n_mels = 80; c->hidden = 384; c->heads = 8; c->enc_layers = 4; c->dec_layers = 4;
    c->ffn_kernel = 3; c->bert_dim = 768; c->dur_layers = 2; c->pitch_layers = 3; c->energy_layers = 2; c->var_kernel = 3;
    c->var_embed_kernel = 9; c->n_up = 4;
    const int ur[4] = {8, 8, 2, 2}, uk[4] = {16, 16, 4, 4}, rk[3] = {3, 7, 11}, rd[3] = {1, 3, 5};
    for (int i = 0; i < 4; ++i) { c->up_rates[i] = ur[i]; c->up_kernels[i] = uk[i]; }
    c->up_init_ch = 512; c->n_rb = 3; c->n_rb_dils = 3;
    for (int j = 0; j < 3; ++j) { c->rb_kernels[j] = rk[j]; for (int d = 0; d < 3; ++d) c->rb_dils[j][d] = rd[d]; }
    c->sample_rate = 16000; c->keep_stages = 0; c->token_rate_split = 1;
    // the default IS the contract mode (north_star: waveform within 1e-3 relative L2 of the reference, zero-mean audio included): a caller that follows
    // INTEGRATION.md literally -- ev_default_config, no field overridden -- gets it; fp16 operands (2.4e-3 on zero-mean audio) and strict are opt-ins
    c->decoder_precision = EV_PREC_MX; c->vocoder_precision = EV_PREC_MX;
}

int ev_abi_info(size_t sizes[4]) {
    if (sizes) { sizes[0] = sizeof(ev_config); sizes[1] = sizeof(ev_result); sizes[2] = sizeof(ev_conv_gemm_desc); sizes[3] = sizeof(ev_res_pair_desc); }
    return EV_ABI_VERSION;
}

const char* ev_last_error(ev_handle* h) { return h ? h->err.c_str() : g_create_error.c_str(); }

int ev_create(int device_id, const ev_config* cfg, ev_handle** out) {
    if (!cfg || !out) return fail(nullptr, "ev_create: null argument");
    if (cfg->abi_version != EV_ABI_VERSION) return fail(nullptr, "ev_create: abi_version %d != %d", cfg->abi_version, EV_ABI_VERSION);
    if (cfg->hidden != 384 || cfg->heads != 8) return fail(nullptr, "ev_create: only hidden=384 / heads=8 (d_k=48) kernels are built");
    if (cfg->hidden % 128 || cfg->n_mels > MEL_PAD) return fail(nullptr, "ev_create: unsupported shape");
    if (cfg->n_up < 1 || cfg->n_up > 4 || cfg->n_rb < 1 || cfg->n_rb > 3 || cfg->n_rb_dils < 1 || cfg->n_rb_dils > 4)
        return fail(nullptr, "ev_create: generator layout outside the built range (n_up 1-4, n_rb 1-3, dilations 1-4)");
    for (int i = 0; i < cfg->n_up; ++i)
        if (cfg->up_kernels[i] != 2 * cfg->up_rates[i] || (cfg->up_rates[i] & (cfg->up_rates[i] - 1)))
            return fail(nullptr, "ev_create: upsample stage %d must have kernel = 2*stride and a power-of-two stride", i);
    // shapes the kernels would silently mishandle are rejected here (not discovered as garbage audio):
    //  * conv_post and the last stage exist for 32 channels only; every stage needs C % 32 == 0
    //  * GAP zero rows between utterances must cover every token- / frame-rate conv halo
    //  * a generator conv's span (k-1)*dilation must fit the 64 staged halo rows and the stage's gap rows
    if ((cfg->up_init_ch >> cfg->n_up) != 32 || (cfg->up_init_ch & (cfg->up_init_ch - 1)))
        return fail(nullptr, "ev_create: upsample_initial_channel / 2^n_up must be 32 (got %d / 2^%d)", cfg->up_init_ch, cfg->n_up);
    if ((cfg->ffn_kernel - 1) / 2 > GAP || (cfg->var_embed_kernel - 1) / 2 > GAP || (cfg->var_kernel - 1) / 2 > GAP ||
        !(cfg->ffn_kernel & 1) || !(cfg->var_embed_kernel & 1))
        return fail(nullptr, "ev_create: token / frame-rate conv kernels must be odd and <= %d taps", 2 * GAP + 1);
    {
        int U = 1;
        for (int i = 0; i < cfg->n_up; ++i) {
            U *= cfg->up_rates[i];
            for (int j = 0; j < cfg->n_rb; ++j)
                for (int d = 0; d < cfg->n_rb_dils; ++d) {
                    const int k = cfg->rb_kernels[j], span = (k - 1) * cfg->rb_dils[j][d];
                    if (!(k & 1) || k < 1 || cfg->rb_dils[j][d] < 1 || span > 64 || span / 2 > GAP * U)
                        return fail(nullptr, "ev_create: ResBlock kernel %d / dilation %d at stage %d exceeds the staged halo", k, cfg->rb_dils[j][d], i);
                }
        }
    }
    if (cfg->decoder_precision != EV_PREC_F16 && cfg->decoder_precision != EV_PREC_F32 && cfg->decoder_precision != EV_PREC_X3 &&
        cfg->decoder_precision != EV_PREC_MX)
        return fail(nullptr, "ev_create: unknown decoder_precision %d", cfg->decoder_precision);
    if (cfg->vocoder_precision != EV_PREC_F16 && cfg->vocoder_precision != EV_PREC_X3 && cfg->vocoder_precision != EV_PREC_MX)
        return fail(nullptr, "ev_create: vocoder_precision must be EV_PREC_F16, EV_PREC_X3 or EV_PREC_MX");
    if ((cfg->mx_residual | cfg->decoder_attention | cfg->fused_pairs | cfg->mx_mrf | cfg->decoder_ln_planes | cfg->token_splitk | cfg->mx_act_format | cfg->mx_group) & ~1)
        return fail(nullptr, "ev_create: mx_residual / decoder_attention / fused_pairs / mx_mrf / decoder_ln_planes / token_splitk / mx_act_format / mx_group must be 0 or 1");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return fail(nullptr, "ev_create: no HIP device available (%s) -- the product path has no CPU fallback", hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev) return fail(nullptr, "ev_create: device %d out of range (%d devices)", device_id, ndev);
    ev_handle* h = new ev_handle();
    h->cfg = *cfg; h->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking) != hipSuccess) {
        delete h;
        return fail(nullptr, "ev_create: cannot create stream on device %d", device_id);
    }
    h->stream = h->own_stream;
    if (init_device_kernels(device_id) != 0) {
        (void)hipStreamDestroy(h->own_stream);
        delete h;
        return fail(nullptr, "ev_create: kernel setup failed on device %d (large-LDS opt-in)", device_id);
    }
    for (int j = 0; j < 2; ++j) {
        if (hipStreamCreateWithFlags(&h->aux[j], hipStreamNonBlocking) != hipSuccess) h->aux[j] = nullptr;
        (void)hipEventCreateWithFlags(&h->ev_join[j], hipEventDisableTiming);
    }
    (void)hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming);
    *out = h;
    return 0;
}

void ev_destroy(ev_handle* h) {
    if (!h) return;
    (void)hipSetDevice(h->device);
    (void)hipStreamSynchronize(h->stream);
    for (int i = 0; i < 11; ++i) if (h->arena[i]) (void)hipFree(h->arena[i]);
    if (h->rs_tab) (void)hipFree(h->rs_tab);
    if (h->st_tab) (void)hipFree(h->st_tab);
    if (h->feat_basis) (void)hipFree(h->feat_basis);
    if (h->feat_melT) (void)hipFree(h->feat_melT);
    if (h->sblob) (void)hipFree(h->sblob);
    if (h->pinned) (void)hipHostFree(h->pinned);
    if (h->pe_dev) (void)hipFree(h->pe_dev);
    if (h->wblob && h->wblob_owned) (void)hipFree(h->wblob);
    for (auto e : h->evt_pool) (void)hipEventDestroy(e);
    for (auto& kv : h->region_evt) { (void)hipEventDestroy(kv.second.first); (void)hipEventDestroy(kv.second.second); }
    for (int j = 0; j < 2; ++j) { if (h->aux[j]) (void)hipStreamDestroy(h->aux[j]); if (h->ev_join[j]) (void)hipEventDestroy(h->ev_join[j]); }
    if (h->ev_fork) (void)hipEventDestroy(h->ev_fork);
    if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
    delete h;
}

int ev_set_stream(ev_handle* h, void* s) {
    if (!h) return -1;
    (void)hipStreamSynchronize(h->stream);
    h->stream = s ? (hipStream_t)s : h->own_stream;
    return 0;
}

int ev_load_weights(ev_handle* h, const void* blob, size_t nbytes, const char*) {
    if (!h || !blob) return fail(h, "ev_load_weights: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    if (h->wblob && h->wblob_owned) HIPCHK(h, hipFree(h->wblob));
    h->wblob = nullptr;
    HIPCHK(h, hipMalloc((void**)&h->wblob, nbytes));
    h->wblob_owned = true; h->wbytes = nbytes;
    HIPCHK(h, hipMemcpy(h->wblob, blob, nbytes, hipMemcpyHostToDevice));
    return parse_blob(h, (const char*)blob, nbytes, false);
}

int ev_load_weights_device(ev_handle* h, const void* dptr, size_t nbytes, const char*) {
    if (!h || !dptr) return fail(h, "ev_load_weights_device: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    if (h->wblob && h->wblob_owned) HIPCHK(h, hipFree(h->wblob));
    h->wblob = (char*)dptr; h->wblob_owned = false; h->wbytes = nbytes;
    if (nbytes < 16) return fail(h, "weight blob too small");
    uint32_t count = 0;
    char hdr[16];
    HIPCHK(h, hipMemcpy(hdr, dptr, 16, hipMemcpyDeviceToHost));
    memcpy(&count, hdr + 8, 4);
    const size_t tbl = 16 + (size_t)count * sizeof(BlobEntry);
    if (tbl > nbytes) return fail(h, "weight blob: truncated table");
    std::vector<char> host(tbl);
    HIPCHK(h, hipMemcpy(host.data(), dptr, tbl, hipMemcpyDeviceToHost));
    // parse_blob validates offsets against the full size
    std::vector<char> fake(host);
    return parse_blob(h, fake.data(), nbytes >= tbl ? nbytes : tbl) == 0 ? 0 : -1;
}

int ev_set_forced_durations(ev_handle* h, const int64_t* d, int64_t n) {
    if (!h) return -1;
    h->forced_dur.assign(d, d + n);
    return 0;
}

int ev_memcpy_d2h(ev_handle* h, void* dst, const void* src, size_t n) {
    if (!h || !dst || !src) return fail(h, "ev_memcpy_d2h: null argument");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipMemcpy(dst, src, n, hipMemcpyDeviceToHost));
    return 0;
}

int ev_set_profiling(ev_handle* h, int enable) { if (!h) return -1; h->profiling = enable != 0; return 0; }
int ev_get_timing(ev_handle* h, const char* name, float* ms) {
    if (!h || !ms) return -1;
    auto it = h->timings.find(name);
    if (it == h->timings.end()) return fail(h, "no timing named %s", name);
    *ms = it->second;
    return 0;
}
int ev_launch_record_count(ev_handle* h) { return h ? (int)h->launches.size() : -1; }
int ev_get_launch_record(ev_handle* h, int idx, ev_launch_record* out) {
    if (!h || !out || idx < 0 || idx >= (int)h->launches.size()) return -1;
    const LaunchRec& r = h->launches[idx];
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", r.name.c_str());
    out->M = r.M; out->N = r.N; out->K = r.K; out->taps = r.taps; out->dil = r.dil; out->ms = r.ms; out->flops = r.flops; out->bytes = r.bytes;
    return 0;
}
int ev_kernel_stat_count(ev_handle* h) { return h ? (int)h->stats.size() : -1; }
int ev_get_kernel_stat(ev_handle* h, int idx, ev_kernel_stat* out) {
    if (!h || !out || idx < 0 || idx >= (int)h->stats.size()) return -1;
    memset(out, 0, sizeof *out);
    snprintf(out->name, sizeof out->name, "%s", h->stats[idx].name.c_str());
    out->launches = h->stats[idx].launches; out->ms = h->stats[idx].ms; out->flops = h->stats[idx].flops; out->bytes = h->stats[idx].bytes;
    return 0;
}

// ------------------------------------------------------------------- vocoder-only entry
static int finish_wav(ev_handle* h, const VocPlan& vp, VocBufs& vb, int64_t* d_scr, uint32_t flags, ev_result* out) {
    const int U = vp.U;
    if (pack_level(h, vb.wavrows.p, DT_F32, 1, 1, ilog2(U), false, vb.wav, d_scr)) return -1;
    if (flags & EV_FLAG_WANT_INT16) launch_wav_to_i16(vb.wav, vb.wav_i16, h->total_frames * U, h->stream);
    out->wav = vb.wav;
    out->wav_i16 = (flags & EV_FLAG_WANT_INT16) ? vb.wav_i16 : nullptr;
    out->total_samples = h->total_frames * U;
    return 0;
}

static void register_voc_taps(ev_handle* h, const VocPlan& vp, VocBufs& vb) {
    const ev_config& c = h->cfg;
    const bool x3 = vp.x3;     // split-precision / MX modes: the stored tensors ARE the raw module outputs
    add_tap(h, "voc_pre", x3 ? vb.pre.p : vb.pre_tap.p, DT_F32, c.up_init_ch, c.up_init_ch, 1, 0);
    for (int i = 0; i < c.n_up; ++i) {
        const int ch = vp.st[i].cout, shift = ilog2(vp.st[i].U_in * vp.st[i].s);
        add_tap(h, ("voc_up" + std::to_string(i)).c_str(), vb.xu[i].p, x3 ? DT_F32 : DT_F16, ch, ch, 2 + i, shift);
        add_tap(h, ("voc_mrf" + std::to_string(i)).c_str(), x3 ? vb.nxt[i].p : vb.mrf_tap[i].p, DT_F32, ch, ch, 2 + i, shift);
    }
}

int ev_vocoder(ev_handle* h, int B, const void* mel, int mel_is_f16, const int32_t* mel_lens, uint32_t flags, ev_result* out) {
    if (!h || !mel || !mel_lens || !out || B <= 0) return fail(h, "ev_vocoder: bad argument");
    if (!h->wt.count("voc.post.w")) return fail(h, "ev_vocoder: weights not loaded");
    HIPCHK(h, hipSetDevice(h->device));
    const ev_config& c = h->cfg;
    const bool voc_x3 = c.vocoder_precision != EV_PREC_F16;      // X3 and MX: fp32 mel rows
    profiling_reset(h);
    h->taps.clear(); h->aln_lp = nullptr;
    h->B = B; h->total_tokens = 0;
    h->mel_lens.assign(mel_lens, mel_lens + B);
    for (int b = 0; b < B; ++b) if (mel_lens[b] <= 0) return fail(h, "ev_vocoder: mel_lens[%d] = %d", b, mel_lens[b]);
    std::vector<int64_t> elem_off(B);
    int64_t eo = 0;
    for (int b = 0; b < B; ++b) { elem_off[b] = eo; eo += (int64_t)c.n_mels * mel_lens[b]; }
    const size_t es = mel_is_f16 ? 2 : 4;

    Buf mel16; VocBufs vb; int64_t* d_scr = nullptr; int64_t* d_eoff = nullptr;
    void* d_melin = nullptr;
    const int Rf = frame_rows(mel_lens, B);
    VocPlan vp;
    if (make_voc_plan(h, Rf, vp)) return -1;
    if ((size_t)B > PIN_MAX_B) return fail(h, "at most %zu utterances per call", PIN_MAX_B);
    if (pinned_reserve(h, PIN_BYTES)) return -1;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 1, pass == 0};
        if (pass == 1 && arena_reserve(h, 1, need)) return -1;
        build_frame_layout(h, ap, pass == 0, B);
        h->d_mel_len = ap.arr<int32_t>(B);
        d_eoff = ap.arr<int64_t>(B);
        d_scr = ap.arr<int64_t>(3 * (size_t)B + 8);
        if (!(flags & EV_FLAG_DEVICE_INPUTS)) d_melin = ap.take((size_t)eo * es);
        mel16 = ap.rows(Rf, MEL_PAD, voc_x3 ? 4 : 2);      // the generator's input rows (fp32 in the split-precision mode)
        plan_vocoder(ap, vp, vb);
        need = ap.off;
    }
    HIPCHK(h, hipMemcpyAsync(h->d_mel_len, mel_lens, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_eoff, elem_off.data(), (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
    const void* melsrc = mel;
    if (!(flags & EV_FLAG_DEVICE_INPUTS)) { HIPCHK(h, hipMemcpyAsync(d_melin, mel, (size_t)eo * es, hipMemcpyHostToDevice, h->stream)); melsrc = d_melin; }
    HIPCHK(h, hipStreamSynchronize(h->stream));
    region_begin(h, "total");
    launch_mel_to_rows(melsrc, mel_is_f16, d_eoff, h->d_frm_seq, h->d_frm_pos, h->d_mel_len, mel16.p, voc_x3 ? 1 : 0, Rf, c.n_mels, MEL_PAD, h->stream);
    region_begin(h, "vocoder");
    if (run_vocoder(h, vp, mel16, (double)h->total_frames, vb)) return -1;
    HIPCHK(h, hipGetLastError());       // a rejected launch (bad configuration, missing LDS opt-in) must not return stale audio
    region_end(h, "vocoder");
    memset(out, 0, sizeof *out);
    if (finish_wav(h, vp, vb, d_scr, flags, out)) return -1;
    HIPCHK(h, hipGetLastError());
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    profiling_collect(h);
    if (vp.keep) register_voc_taps(h, vp, vb);
    out->batch = B; out->total_frames = h->total_frames; out->mel_lens = h->mel_lens.data(); out->mel_offsets = h->mel_offs.data();
    return 0;
}

// ------------------------------------------------------------------- full synthesis
// ev_synthesize_prosody's host-side checks (include/evhip.h): everything that can be validated without touching the device, before anything
// is launched.  Per-token device arrays are left to the kernels (non-finite / negative = predicted, durations clamped).
static int check_prosody(ev_handle* h, const ev_prosody* p, int B, int NT, float alpha, uint32_t flags) {
    // one layout exists so far: a smaller size is no earlier version but a truncated struct, a larger one carries fields this library does
    // not know.  The change that appends fields keeps accepting this size, with the missing fields read as NULL.
    if (p->struct_size != sizeof(ev_prosody)) return fail(h, "ev_synthesize_prosody: prosody.struct_size %u != sizeof(ev_prosody) %zu", p->struct_size, sizeof(ev_prosody));
    if (p->reserved0 != 0) return fail(h, "ev_synthesize_prosody: prosody.reserved0 must be 0");
    if (flags & EV_FLAG_FORCED_DURATIONS) return fail(h, "ev_synthesize_prosody: prosody cannot be combined with EV_FLAG_FORCED_DURATIONS (use prosody.durations)");
    if (!p->alpha && !(alpha > 0.f && std::isfinite(alpha))) return fail(h, "ev_synthesize_prosody: alpha %g must be > 0 and finite", (double)alpha);
    const struct { const float* v; const char* name; } per_utt[] = {
        {p->pitch_scale, "pitch_scale"}, {p->pitch_shift, "pitch_shift"}, {p->energy_scale, "energy_scale"}, {p->energy_shift, "energy_shift"}};
    for (int b = 0; b < B; ++b) {
        if (p->alpha && !(p->alpha[b] > 0.f && std::isfinite(p->alpha[b])))
            return fail(h, "ev_synthesize_prosody: prosody.alpha[%d] = %g must be > 0 and finite", b, (double)p->alpha[b]);
        for (const auto& f : per_utt)
            if (f.v && !std::isfinite(f.v[b])) return fail(h, "ev_synthesize_prosody: prosody.%s[%d] = %g is not finite", f.name, b, (double)f.v[b]);
    }
    if (!(flags & EV_FLAG_DEVICE_INPUTS)) {
        for (int j = 0; j < NT; ++j) {
            if (p->pitch && std::isinf(p->pitch[j])) return fail(h, "ev_synthesize_prosody: prosody.pitch[%d] is infinite (NaN = predicted)", j);
            if (p->energy && std::isinf(p->energy[j])) return fail(h, "ev_synthesize_prosody: prosody.energy[%d] is infinite (NaN = predicted)", j);
            if (p->durations && (p->durations[j] < -1 || p->durations[j] > EV_PROSODY_MAX_DURATION))
                return fail(h, "ev_synthesize_prosody: prosody.durations[%d] = %lld outside [-1, %d]", j, (long long)p->durations[j], EV_PROSODY_MAX_DURATION);
        }
    }
    return 0;
}

// ev_synthesize and ev_synthesize_prosody: pros == NULL is the plain call (the launches and bits of ev_synthesize)
static int synthesize(ev_handle* h, int B, const int64_t* ling, const int32_t* cu, const int64_t* speaker, const float* style,
                      const float* content, float alpha, const ev_prosody* pros, uint32_t flags, ev_result* out) {
    if (!h || !ling || !cu || !speaker || !style || !content || !out || B <= 0) return fail(h, "ev_synthesize: bad argument");
    if (!h->wt.count("tok_emb")) return fail(h, "ev_synthesize: weights not loaded");
    if (cu[0] != 0) return fail(h, "ev_synthesize: cu_seqlens[0] must be 0");
    HIPCHK(h, hipSetDevice(h->device));
    const ev_config& c = h->cfg;
    const int C = c.hidden;
    const bool keep = c.keep_stages != 0;
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0;
    const int dec_prec = c.decoder_precision == EV_PREC_F16 ? DT_F16 : DT_F32;      // X3 and F32 both keep fp32 activations
    const bool voc_x3 = c.vocoder_precision != EV_PREC_F16;      // X3 and MX: fp32 mel rows
    profiling_reset(h);
    h->taps.clear(); h->aln_lp = nullptr;
    h->B = B;
    const int NT = cu[B];
    h->total_tokens = NT;
    int max_tok = 0;
    h->tok_off.resize(B); h->tok_len.resize(B);
    int64_t rows = GAP;
    for (int b = 0; b < B; ++b) {
        const int n = cu[b + 1] - cu[b];
        if (n <= 0) return fail(h, "ev_synthesize: utterance %d has %d tokens", b, n);
        h->tok_off[b] = (int32_t)rows; h->tok_len[b] = n; rows += n + GAP; max_tok = std::max(max_tok, n);
    }
    const int Rt = (int)align_up((size_t)rows, ROW_ALIGN);
    h->Rt = Rt;
    if ((flags & EV_FLAG_FORCED_DURATIONS) && (int64_t)h->forced_dur.size() != NT) return fail(h, "forced durations: expected %d values", NT);
    if (!dev_in) {      // nn.Embedding raises IndexError on these (model_open_source.py:107,109); device inputs are clamped by the kernels
        for (int j = 0; j < NT; ++j)
            if (ling[j] < 0 || ling[j] >= c.n_vocab) return fail(h, "ev_synthesize: phoneme id %lld at position %d outside [0, %d)", (long long)ling[j], j, c.n_vocab);
        for (int b = 0; b < B; ++b)
            if (speaker[b] < 0 || speaker[b] >= c.n_speaker) return fail(h, "ev_synthesize: speaker id %lld of utterance %d outside [0, %d)", (long long)speaker[b], b, c.n_speaker);
    }
    if (pros && check_prosody(h, pros, B, NT, alpha, flags)) return -1;
    if (ensure_pe(h, max_tok)) return -1;

    // ---------------- phase 1: token-rate arena
    struct TokBufs {
        Buf x, hb, qkv, ctx, ffn, y, xp, xvar, t1, t2, t1b, t2b, t1c, t2c, pitch, energy, logd, centre;
        std::vector<Buf> ltaps; Buf tokemb_tap;
        int64_t* d_ling; int64_t* d_spk; float* d_style; float* d_content; float* d_u;
        int64_t* d_dur; float* d_logd_packed; float* d_pitch_packed; float* d_energy_packed; int64_t* d_forced; int64_t* d_scr;
        // ev_synthesize_prosody only: per-utterance controls (SoA [5][B]), per-token overrides, effective durations and track rows
        float* d_pctrl; float* d_povr_pitch; float* d_povr_energy; int64_t* d_povr_dur; int64_t* d_dur_eff; Buf pitch_eff, energy_eff;
    } tb{};
    size_t tok_arena_end = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 0, pass == 0};
        if (pass == 1 && arena_reserve(h, 0, tok_arena_end)) return -1;
        h->d_tok_seq = ap.arr<int32_t>(Rt); h->d_tok_pos = ap.arr<int32_t>(Rt); h->d_tok_valid = ap.arr<uint8_t>(Rt);
        h->d_tok_off = ap.arr<int32_t>(B); h->d_tok_len = ap.arr<int32_t>(B); h->d_cu = ap.arr<int32_t>(B + 1);
        h->d_mel_len = ap.arr<int32_t>(B);
        tb.d_ling = ap.arr<int64_t>(NT); tb.d_spk = ap.arr<int64_t>(B); tb.d_style = ap.arr<float>((size_t)B * c.bert_dim);
        tb.d_content = ap.arr<float>((size_t)B * c.bert_dim); tb.d_u = ap.arr<float>((size_t)B * C);
        tb.d_dur = ap.arr<int64_t>(NT); tb.d_logd_packed = ap.arr<float>(NT); tb.d_pitch_packed = ap.arr<float>(NT);
        tb.d_energy_packed = ap.arr<float>(NT); tb.d_forced = ap.arr<int64_t>(NT); tb.d_scr = ap.arr<int64_t>(3 * (size_t)B + 8);
        tb.x = ap.rows(Rt, C, 4); tb.hb = ap.rows(Rt, C, 4); tb.qkv = ap.rows(Rt, 3 * C, 4); tb.ctx = ap.rows(Rt, C, 4);
        tb.ffn = ap.rows(Rt, 4 * C, 4); tb.y = ap.rows(Rt, C, 4); tb.xp = ap.rows(Rt, C, 4); tb.xvar = ap.rows(Rt, C, 4);
        tb.t1 = ap.rows(Rt, C, 4); tb.t2 = ap.rows(Rt, C, 4);
        tb.t1b = ap.rows(Rt, C, 4); tb.t2b = ap.rows(Rt, C, 4); tb.t1c = ap.rows(Rt, C, 4); tb.t2c = ap.rows(Rt, C, 4);
        tb.pitch = ap.rows(Rt, 1, 4); tb.energy = ap.rows(Rt, 1, 4); tb.logd = ap.rows(Rt, 1, 4); tb.centre = ap.rows(Rt, 1, 4);
        if (keep) { tb.ltaps.resize(c.enc_layers); for (auto& b : tb.ltaps) b = ap.rows(Rt, C, 4); tb.tokemb_tap = ap.rows(Rt, C, 4); }
        if (pros) {
            tb.d_pctrl = ap.arr<float>(5 * (size_t)B);
            tb.d_povr_pitch = pros->pitch ? ap.arr<float>(NT) : nullptr;
            tb.d_povr_energy = pros->energy ? ap.arr<float>(NT) : nullptr;
            tb.d_povr_dur = pros->durations ? ap.arr<int64_t>(NT) : nullptr;
            tb.d_dur_eff = ap.arr<int64_t>(NT);
            tb.pitch_eff = ap.rows(Rt, 1, 4); tb.energy_eff = ap.rows(Rt, 1, 4);
        }
        {          // split-K partial sums (tok_splitk): 4 ranges x hidden columns
            const Buf kb = (c.token_splitk == 0 && c.token_rate_split != 0) ? ap.rows(Rt, 4 * C, 4) : Buf{};
            h->tok_ks = kb.p; h->tok_ks_bytes = kb.p ? (size_t)Rt * 4 * C * 4 : 0;
        }
        tok_arena_end = ap.off;
    }
    // token layout: B offsets / lengths / cu_seqlens through the pinned token region, per-row maps built on the device
    if ((size_t)B > PIN_MAX_B) return fail(h, "ev_synthesize: at most %zu utterances per call", PIN_MAX_B);
    if (pinned_reserve(h, pros ? PIN_BYTES_PROSODY : PIN_BYTES)) return -1;
    {
        int32_t* off = (int32_t*)h->pinned; int32_t* len = off + B; int32_t* pcu = len + B;
        for (int b = 0; b < B; ++b) { off[b] = h->tok_off[b]; len[b] = h->tok_len[b]; }
        memcpy(pcu, cu, (size_t)(B + 1) * 4);
        HIPCHK(h, hipMemcpyAsync(h->d_tok_off, off, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_tok_len, len, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_cu, pcu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, h->stream));
        launch_row_maps(h->d_tok_off, h->d_tok_len, B, h->d_tok_seq, h->d_tok_pos, h->d_tok_valid, Rt, h->stream);
        // caller-owned inputs: borrowed for the duration of the call (host pointers are pageable: the runtime stages them before
        // hipMemcpyAsync returns; device pointers are read in stream order)
        const hipMemcpyKind kind = dev_in ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIPCHK(h, hipMemcpyAsync(tb.d_ling, ling, (size_t)NT * 8, kind, h->stream));
        HIPCHK(h, hipMemcpyAsync(tb.d_spk, speaker, (size_t)B * 8, kind, h->stream));
        HIPCHK(h, hipMemcpyAsync(tb.d_style, style, (size_t)B * c.bert_dim * 4, kind, h->stream));
        HIPCHK(h, hipMemcpyAsync(tb.d_content, content, (size_t)B * c.bert_dim * 4, kind, h->stream));
        if (flags & EV_FLAG_FORCED_DURATIONS)
            HIPCHK(h, hipMemcpyAsync(tb.d_forced, h->forced_dur.data(), (size_t)NT * 8, hipMemcpyHostToDevice, h->stream));
        if (pros) {         // per-utterance controls through the pinned prosody region, per-token overrides like ling
            float* ctrl = (float*)(h->pinned + PIN_PROSODY);
            const float* src[5] = {pros->alpha, pros->pitch_scale, pros->pitch_shift, pros->energy_scale, pros->energy_shift};
            const float dflt[5] = {alpha, 1.0f, 0.0f, 1.0f, 0.0f};
            for (int i = 0; i < 5; ++i)
                for (int b = 0; b < B; ++b) ctrl[(size_t)i * B + b] = src[i] ? src[i][b] : dflt[i];
            HIPCHK(h, hipMemcpyAsync(tb.d_pctrl, ctrl, (size_t)5 * B * 4, hipMemcpyHostToDevice, h->stream));
            if (pros->pitch) HIPCHK(h, hipMemcpyAsync(tb.d_povr_pitch, pros->pitch, (size_t)NT * 4, kind, h->stream));
            if (pros->energy) HIPCHK(h, hipMemcpyAsync(tb.d_povr_energy, pros->energy, (size_t)NT * 4, kind, h->stream));
            if (pros->durations) HIPCHK(h, hipMemcpyAsync(tb.d_povr_dur, pros->durations, (size_t)NT * 8, kind, h->stream));
        }
    }
    region_begin(h, "total");
    region_begin(h, "am");
    region_begin(h, "encoder");
    RowCtx trc{Rt, h->d_tok_valid, h->d_tok_seq, h->d_tok_off, h->d_tok_len, B, max_tok, (double)NT};
    WPTR(tok_emb, float, "tok_emb"); WPTR(spk_emb, float, "spk_emb");
    float alphas[2];
    if (get_scalar(h, "enc.alpha", &alphas[0]) || get_scalar(h, "dec.alpha", &alphas[1])) return -1;
    { KScope ks(h, "embed_pe", 0, (double)NT * C * 12.0);
      launch_embed_pe(tb.d_ling, h->d_cu, h->d_tok_seq, h->d_tok_pos, tok_emb, c.n_vocab, h->pe_dev, alphas[0], (float*)tb.x.p, keep ? (float*)tb.tokemb_tap.p : nullptr, Rt, C, h->stream); }
    if (run_stack(h, "enc", c.enc_layers, DT_F32, trc, tb.x, tb.hb, tb.qkv, tb.ctx, tb.ffn, tb.y, nullptr, keep ? &tb.ltaps : nullptr)) return -1;
    HIPCHK(h, hipGetLastError());
    region_end(h, "encoder");
    region_begin(h, "variance");
    // embed_projection1 (model_open_source.py:109-111): time-varying part as a GEMM, conditioning part as a per-utterance vector
    WPTR(wcond, float, "proj.wcond"); WPTR(bproj, float, "proj.b"); WPTR(wproj, char, "proj.w32");
    { KScope ks(h, "cond_vector", 2.0 * B * C * (C + 2.0 * c.bert_dim), 0);
      launch_cond_vector(tb.d_spk, tb.d_style, tb.d_content, spk_emb, c.n_speaker, wcond, bproj, tb.d_u, B, C, c.bert_dim, h->stream); }
    {
        ConvGemmParams p = gemm_defaults();
        p.dtype = DT_F32; p.A = tb.y.p; p.lda = C; p.W = wproj; p.M = Rt; p.N = C; p.K = C; p.row_valid = h->d_tok_valid;
        p.row_seq = h->d_tok_seq; p.seq_bias = tb.d_u; p.ld_seq_bias = C; p.out32 = (float*)tb.xp.p; p.ldo = C;
        if (tok_weights(h, "proj.w", p)) return -1;
        if (gemm(h, "variance_f32_gemm", p, NT)) return -1;
    }
    {
        // the three predictors only share their input: pitch and energy run on the auxiliary streams beside the duration
        // predictor (each conv is one partial wave of 396 workgroups on 256 CUs)
        const bool conc = !h->profiling && c.vocoder_streams != 1 && h->aux[0] && h->aux[1];
        if (conc) {
            (void)hipEventRecord(h->ev_fork, h->stream);
            (void)hipStreamWaitEvent(h->aux[0], h->ev_fork, 0);
            (void)hipStreamWaitEvent(h->aux[1], h->ev_fork, 0);
        }
        if (run_predictor(h, "pitch", c.pitch_layers, trc, tb.xp, tb.t1b, tb.t2b, (float*)tb.pitch.p, conc ? h->aux[0] : nullptr)) return -1;
        if (run_predictor(h, "energy", c.energy_layers, trc, tb.xp, tb.t1c, tb.t2c, (float*)tb.energy.p, conc ? h->aux[1] : nullptr)) return -1;
        if (conc) { (void)hipEventRecord(h->ev_join[0], h->aux[0]); (void)hipEventRecord(h->ev_join[1], h->aux[1]); }
        if (run_predictor(h, "dur", c.dur_layers, trc, tb.xp, tb.t1, tb.t2, (float*)tb.logd.p)) return -1;
        if (conc) { (void)hipStreamWaitEvent(h->stream, h->ev_join[0], 0); (void)hipStreamWaitEvent(h->stream, h->ev_join[1], 0); }
    }
    // prosody (after the join, on the handle's stream): the effective tracks replace the predictions as the embeddings' input
    const float* pitch_in = (const float*)tb.pitch.p;
    const float* energy_in = (const float*)tb.energy.p;
    if (pros) {
        KScope ks(h, "prosody_tracks", 0, (double)NT * 16.0);
        launch_prosody_tracks((const float*)tb.pitch.p, (const float*)tb.energy.p, h->d_tok_seq, h->d_tok_pos, h->d_cu, tb.d_povr_pitch, tb.d_povr_energy,
                              tb.d_pctrl, B, (float*)tb.pitch_eff.p, (float*)tb.energy_eff.p, Rt, h->stream);
        pitch_in = (const float*)tb.pitch_eff.p; energy_in = (const float*)tb.energy_eff.p;
    }
    {
        WPTR(wp, float, "pitch_emb.w"); WPTR(bp, float, "pitch_emb.b"); WPTR(we, float, "energy_emb.w"); WPTR(be, float, "energy_emb.b");
        KScope ks(h, "var_embed_add", 0, (double)NT * C * 8.0);
        launch_var_embed_add((const float*)tb.xp.p, pitch_in, energy_in, wp, bp, we, be, h->d_tok_valid,
                             (float*)tb.xvar.p, Rt, C, c.var_embed_kernel, h->stream);
    }
    if (pros) {
        KScope ks(h, "durations_prosody", 0, 0);
        launch_durations_prosody((const float*)tb.logd.p, h->d_tok_off, h->d_tok_len, B, alpha, pros->alpha ? tb.d_pctrl : nullptr, tb.d_povr_dur,
                                 EV_PROSODY_MAX_DURATION, h->d_cu, tb.d_dur, tb.d_dur_eff, tb.d_logd_packed, (float*)tb.centre.p, h->d_mel_len, h->stream);
    } else {
      KScope ks(h, "durations", 0, 0);
      launch_durations((const float*)tb.logd.p, h->d_tok_off, h->d_tok_len, B, alpha, (flags & EV_FLAG_FORCED_DURATIONS) ? tb.d_forced : nullptr,
                       h->d_cu, tb.d_dur, tb.d_logd_packed, (float*)tb.centre.p, h->d_mel_len, h->stream); }
    HIPCHK(h, hipGetLastError());
    region_end(h, "variance");
    // the reference has the same host sync here (alignment.py:195 `.item()`)
    h->mel_lens.resize(B);
    HIPCHK(h, hipMemcpyAsync(h->mel_lens.data(), h->d_mel_len, (size_t)B * 4, hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    int max_frames = 0;
    for (int b = 0; b < B; ++b) {
        if (h->mel_lens[b] <= 0) return fail(h, "utterance %d produced %d mel frames", b, h->mel_lens[b]);
        max_frames = std::max(max_frames, h->mel_lens[b]);
    }
    if (ensure_pe(h, max_frames)) return -1;
    const float* pe = h->pe_dev;

    // ---------------- phase 2: frame-rate arena (placed after the token arena)
    struct FrmBufs { Buf x, hb, qkv, ctx, ffn, y, mel32, mel16, up_tap, y_tap; std::vector<Buf> ltaps; float* d_mel; } fb;
    VocBufs vb;
    const int Rf = frame_rows(h->mel_lens.data(), B);
    VocPlan vp;
    if (!(flags & EV_FLAG_NO_VOCODER) && make_voc_plan(h, Rf, vp)) return -1;
    const size_t esd = dec_prec == DT_F16 ? 2 : 4;
    const bool dec_mx = c.decoder_precision == EV_PREC_MX && C % 128 == 0;
    DecMx dmx{};
    size_t frm_need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 1, pass == 0};
        if (pass == 1 && arena_reserve(h, 1, frm_need)) return -1;
        build_frame_layout(h, ap, pass == 0, B);
        fb.x = ap.rows(Rf, C, 4); fb.hb = ap.rows(Rf, C, esd); fb.qkv = ap.rows(Rf, 3 * C, esd); fb.ctx = ap.rows(Rf, C, esd);
        fb.ffn = ap.rows(Rf, 4 * C, esd); fb.y = ap.rows(Rf, C, esd); fb.mel32 = ap.rows(Rf, MEL_PAD, 4); fb.mel16 = ap.rows(Rf, MEL_PAD, 2);
        if (dec_mx) {
            const size_t R = (size_t)Rf + 2 * MX_PAD, F = 4 * (size_t)C;
            dmx.ffn.h = ap.take(R * F * 2);
            for (int i = 0; i < 2; ++i) { dmx.ffn.q4[i] = ap.take(R * F / 2); dmx.ffn.qs[i] = ap.take(F / 128 * R * 4); }
            dmx.scratch_bytes = mx_scratch_bytes(Rf, C);
            dmx.scratch = ap.take(dmx.scratch_bytes);
        }
        if (keep) { fb.ltaps.resize(c.dec_layers); for (auto& b : fb.ltaps) b = ap.rows(Rf, C, 4); fb.up_tap = ap.rows(Rf, C, 4); fb.y_tap = ap.rows(Rf, C, 4); }
        fb.d_mel = ap.arr<float>((size_t)h->total_frames * c.n_mels);
        if (!(flags & EV_FLAG_NO_VOCODER)) plan_vocoder(ap, vp, vb);
        frm_need = ap.off;
    }
    h->Rf = Rf;
    region_begin(h, "decoder");
    RowCtx frc{Rf, h->d_frm_valid, h->d_frm_seq, h->d_frm_off, h->d_mel_len, B, max_frames, (double)h->total_frames};
    { KScope ks(h, "gauss_upsample", 0, (double)h->total_frames * C * 8.0);
      launch_gauss_upsample((const float*)tb.xvar.p, (const float*)tb.centre.p, h->d_tok_off, h->d_tok_len, h->d_frm_seq, h->d_frm_pos, pe,
                            alphas[1], 0.1f, (float*)fb.x.p, keep ? (float*)fb.up_tap.p : nullptr, Rf, C, h->stream); }
    if (run_stack(h, "dec", c.dec_layers, dec_prec, frc, fb.x, fb.hb, fb.qkv, fb.ctx, fb.ffn, fb.y,
                  (keep && dec_prec == DT_F16) ? (float*)fb.y_tap.p : nullptr, keep ? &fb.ltaps : nullptr, dec_mx ? &dmx : nullptr)) return -1;
    {
        WPTR(wm, char, dec_prec == DT_F16 ? "to_mel.w16" : "to_mel.w32"); WPTR(bm, float, "to_mel.b");
        ConvGemmParams p = gemm_defaults();
        p.dtype = dec_prec; p.A = fb.y.p; p.lda = C; p.W = wm; p.bias = bm; p.M = Rf; p.N = MEL_PAD; p.K = C; p.row_valid = h->d_frm_valid;
        p.out32 = (float*)fb.mel32.p; p.ldo = MEL_PAD;
        if (!voc_x3) p.out16 = fb.mel16.p;            // the fp16 generator reads fp16 mel rows, the split-precision one the fp32 rows
        if (dec_prec == DT_F32 && tok_weights(h, "to_mel.w", p)) return -1;
        if (gemm(h, dec_prec == DT_F16 ? "dec_f16_gemm" : "dec_f32_gemm", p, (double)h->total_frames)) return -1;
    }
    HIPCHK(h, hipGetLastError());
    region_end(h, "decoder");
    region_end(h, "am");
    // packed outputs
    if (pack_level(h, fb.mel32.p, DT_F32, MEL_PAD, c.n_mels, 0, false, fb.d_mel, tb.d_scr)) return -1;
    if (pack_level(h, tb.pitch.p, DT_F32, 1, 1, 0, true, tb.d_pitch_packed, tb.d_scr)) return -1;
    if (pack_level(h, tb.energy.p, DT_F32, 1, 1, 0, true, tb.d_energy_packed, tb.d_scr)) return -1;
    memset(out, 0, sizeof *out);
    if (!(flags & EV_FLAG_NO_VOCODER)) {
        region_begin(h, "vocoder");
        if (run_vocoder(h, vp, voc_x3 ? fb.mel32 : fb.mel16, (double)h->total_frames, vb)) return -1;
        HIPCHK(h, hipGetLastError());
        region_end(h, "vocoder");
        if (finish_wav(h, vp, vb, tb.d_scr, flags, out)) return -1;
        HIPCHK(h, hipGetLastError());
    }
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    profiling_collect(h);
    if (keep) {
        add_tap(h, "tok_emb", tb.tokemb_tap.p, DT_F32, C, C, 0, 0);
        for (int i = 0; i < c.enc_layers; ++i) add_tap(h, ("enc_l" + std::to_string(i)).c_str(), tb.ltaps[i].p, DT_F32, C, C, 0, 0);
        add_tap(h, "enc_out", tb.y.p, DT_F32, C, C, 0, 0);
        add_tap(h, "x_proj", tb.xp.p, DT_F32, C, C, 0, 0);
        add_tap(h, "pitch_eff", pros ? tb.pitch_eff.p : tb.pitch.p, DT_F32, 1, 1, 0, 0);      // the tracks pitch_embed / energy_embed read
        add_tap(h, "energy_eff", pros ? tb.energy_eff.p : tb.energy.p, DT_F32, 1, 1, 0, 0);
        add_tap(h, "x_var", tb.xvar.p, DT_F32, C, C, 0, 0);
        add_tap(h, "upsampled", fb.up_tap.p, DT_F32, C, C, 1, 0);
        for (int i = 0; i < c.dec_layers; ++i) add_tap(h, ("dec_l" + std::to_string(i)).c_str(), fb.ltaps[i].p, DT_F32, C, C, 1, 0);
        if (dec_prec == DT_F16) add_tap(h, "dec_out", fb.y_tap.p, DT_F32, C, C, 1, 0);
        else add_tap(h, "dec_out", fb.y.p, DT_F32, C, C, 1, 0);
        add_tap(h, "mel", fb.mel32.p, DT_F32, MEL_PAD, c.n_mels, 1, 0);
        if (!(flags & EV_FLAG_NO_VOCODER)) register_voc_taps(h, vp, vb);
    }
    out->batch = B; out->total_tokens = NT; out->total_frames = h->total_frames;
    out->mel = fb.d_mel; out->durations = tb.d_dur; out->log_durations = tb.d_logd_packed; out->pitch = tb.d_pitch_packed;
    out->energy = tb.d_energy_packed; out->mel_lens = h->mel_lens.data(); out->mel_offsets = h->mel_offs.data();
    h->last_dur = tb.d_dur;
    h->last_dur_eff = pros ? tb.d_dur_eff : tb.d_dur;
    return 0;
}

int ev_synthesize(ev_handle* h, int B, const int64_t* ling, const int32_t* cu, const int64_t* speaker, const float* style,
                  const float* content, float alpha, uint32_t flags, ev_result* out) {
    return synthesize(h, B, ling, cu, speaker, style, content, alpha, nullptr, flags, out);
}

int ev_synthesize_prosody(ev_handle* h, int B, const int64_t* ling, const int32_t* cu, const int64_t* speaker, const float* style,
                          const float* content, float alpha, const ev_prosody* prosody, uint32_t flags, ev_result* out) {
    return synthesize(h, B, ling, cu, speaker, style, content, alpha, prosody, flags, out);
}

// ------------------------------------------------------------------- forced alignment (include/evhip.h: ev_align)
int ev_align(ev_handle* h, int B, const int64_t* ling, const int32_t* cu, const int64_t* speaker, const float* style, const float* content,
             const void* mel, int mel_is_f16, const int32_t* mel_lens, const float* pitch_frames, const float* energy_frames, uint32_t flags,
             ev_align_result* out) {
    if (!h) return -1;
    if (!ling || !cu || !speaker || !style || !content || !mel || !mel_lens || !out || B <= 0) return fail(h, "ev_align: bad argument");
    if (out->struct_size != sizeof(ev_align_result))
        return fail(h, "ev_align: out->struct_size %u != sizeof(ev_align_result) %zu", out->struct_size, sizeof(ev_align_result));
    if (!h->wt.count("tok_emb")) return fail(h, "ev_align: weights not loaded");
    if (!h->wt.count("aln.t1.b")) return fail(h, "ev_align: the weight blob has no aligner (aln.*): pack a state dict that carries am.alignment_module.*");
    if (cu[0] != 0) return fail(h, "ev_align: cu_seqlens[0] must be 0");
    if ((size_t)B > PIN_MAX_B) return fail(h, "ev_align: at most %zu utterances per call", PIN_MAX_B);
    const ev_config& c = h->cfg;
    const int C = c.hidden;
    const bool keep = c.keep_stages != 0;
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0;
    const bool dev_mel = dev_in || (flags & EV_FLAG_DEVICE_MEL) != 0;     // mel / pitch_frames / energy_frames already on the device
    const int NT = cu[B];
    int max_tok = 0, max_frames = 0;
    int64_t rows = GAP, lp_elems = 0, total_frames = 0;
    std::vector<int32_t> tok_off(B), tok_len(B);
    for (int b = 0; b < B; ++b) {
        const int n = cu[b + 1] - cu[b], T = mel_lens[b];
        if (n <= 0) return fail(h, "ev_align: utterance %d has %d tokens", b, n);
        if (n > EV_ALIGN_MAX_TOKENS) return fail(h, "ev_align: utterance %d has %d tokens > EV_ALIGN_MAX_TOKENS %d", b, n, EV_ALIGN_MAX_TOKENS);
        if (T > EV_ALIGN_MAX_FRAMES) return fail(h, "ev_align: mel_lens[%d] = %d > EV_ALIGN_MAX_FRAMES %d", b, T, EV_ALIGN_MAX_FRAMES);
        if (T < n) return fail(h, "ev_align: mel_lens[%d] = %d < its %d tokens: no monotonic path gives every token a frame", b, T, n);
        tok_off[b] = (int32_t)rows; tok_len[b] = n; rows += n + GAP; max_tok = std::max(max_tok, n); max_frames = std::max(max_frames, T);
        lp_elems += (int64_t)T * n; total_frames += T;
    }
    if (!dev_in) {
        for (int j = 0; j < NT; ++j)
            if (ling[j] < 0 || ling[j] >= c.n_vocab) return fail(h, "ev_align: phoneme id %lld at position %d outside [0, %d)", (long long)ling[j], j, c.n_vocab);
        for (int b = 0; b < B; ++b)
            if (speaker[b] < 0 || speaker[b] >= c.n_speaker) return fail(h, "ev_align: speaker id %lld of utterance %d outside [0, %d)", (long long)speaker[b], b, c.n_speaker);
    }
    HIPCHK(h, hipSetDevice(h->device));
    if (ensure_pe(h, max_tok)) return -1;
    // the state of the last call: this one (ev_get_stage reads it); no synthesis' durations survive it
    profiling_reset(h);
    h->taps.clear(); h->aln_lp = nullptr;
    h->last_dur = nullptr; h->last_dur_eff = nullptr;
    h->B = B; h->total_tokens = NT;
    h->tok_off = tok_off; h->tok_len = tok_len;
    h->mel_lens.assign(mel_lens, mel_lens + B);
    const int Rt = (int)align_up((size_t)rows, ROW_ALIGN);
    const int Rf = frame_rows(mel_lens, B);
    h->Rt = Rt; h->Rf = Rf;
    std::vector<int64_t> elem_off(B);
    for (int b = 0, e = 0; b < B; ++b) { elem_off[b] = (int64_t)e * c.n_mels; e += mel_lens[b]; }
    const size_t mel_es = mel_is_f16 ? 2 : 4;

    struct {
        Buf x, hb, qkv, ctx, ffn, y, xp, t1, t2, melrows, f1, f2, f3;
        int64_t *d_ling, *d_spk, *d_eoff, *d_dur; float *d_style, *d_content, *d_u, *d_pf, *d_ef, *d_pitch, *d_energy, *d_score, *d_lp;
        void* d_mel; AlignSeq* d_seqs; uint32_t* d_bits;
    } ab{};
    if (pinned_reserve(h, PIN_BYTES)) return -1;      // (build_frame_layout stages through the pinned frame region)
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 3, pass == 0};
        if (pass == 1 && arena_reserve(h, 3, need)) return -1;
        h->d_tok_seq = ap.arr<int32_t>(Rt); h->d_tok_pos = ap.arr<int32_t>(Rt); h->d_tok_valid = ap.arr<uint8_t>(Rt);
        h->d_tok_off = ap.arr<int32_t>(B); h->d_tok_len = ap.arr<int32_t>(B); h->d_cu = ap.arr<int32_t>(B + 1);
        h->d_mel_len = ap.arr<int32_t>(B);
        build_frame_layout(h, ap, pass == 0, B);
        ab.d_ling = ap.arr<int64_t>(NT); ab.d_spk = ap.arr<int64_t>(B); ab.d_style = ap.arr<float>((size_t)B * c.bert_dim);
        ab.d_content = ap.arr<float>((size_t)B * c.bert_dim); ab.d_u = ap.arr<float>((size_t)B * C); ab.d_eoff = ap.arr<int64_t>(B);
        ab.d_mel = dev_mel ? nullptr : ap.take((size_t)total_frames * c.n_mels * mel_es);
        ab.d_pf = (pitch_frames && !dev_mel) ? ap.arr<float>(total_frames) : nullptr;
        ab.d_ef = (energy_frames && !dev_mel) ? ap.arr<float>(total_frames) : nullptr;
        ab.d_seqs = ap.arr<AlignSeq>(B); ab.d_bits = ap.arr<uint32_t>((size_t)total_frames * 64);
        ab.d_dur = ap.arr<int64_t>(NT); ab.d_pitch = pitch_frames ? ap.arr<float>(NT) : nullptr; ab.d_energy = energy_frames ? ap.arr<float>(NT) : nullptr;
        ab.d_score = ap.arr<float>(B); ab.d_lp = ap.arr<float>((size_t)lp_elems);
        ab.x = ap.rows(Rt, C, 4); ab.hb = ap.rows(Rt, C, 4); ab.qkv = ap.rows(Rt, 3 * C, 4); ab.ctx = ap.rows(Rt, C, 4);
        ab.ffn = ap.rows(Rt, 4 * C, 4); ab.y = ap.rows(Rt, C, 4); ab.xp = ap.rows(Rt, C, 4); ab.t1 = ap.rows(Rt, C, 4); ab.t2 = ap.rows(Rt, C, 4);
        ab.melrows = ap.rows(Rf, MEL_PAD, 4); ab.f1 = ap.rows(Rf, C, 4); ab.f2 = ap.rows(Rf, C, 4); ab.f3 = ap.rows(Rf, C, 4);
        {          // split-K partial sums of the encoder (tok_splitk), as in ev_synthesize
            const Buf kb = (c.token_splitk == 0 && c.token_rate_split != 0) ? ap.rows(Rt, 4 * C, 4) : Buf{};
            h->tok_ks = kb.p; h->tok_ks_bytes = kb.p ? (size_t)Rt * 4 * C * 4 : 0;
        }
        need = ap.off;
    }
    h->aln_mel_lens.assign(mel_lens, mel_lens + B);
    h->aln_mel_offs = h->mel_offs;
    h->aln_seqs.resize(B);
    {
        int64_t lo = 0;
        for (int b = 0; b < B; ++b) {
            AlignSeq& q = h->aln_seqs[b];
            q.tok_row = tok_off[b]; q.tokens = tok_len[b]; q.frm_row = h->frm_off[b]; q.frames = mel_lens[b];
            q.lp_off = lo; q.tok_packed = cu[b]; q.frm_packed = h->mel_offs[b]; q.bits_off = h->mel_offs[b] * 64;
            lo += (int64_t)q.frames * q.tokens;
        }
    }
    {
        int32_t* poff = (int32_t*)h->pinned; int32_t* plen = poff + B; int32_t* pcu = plen + B;
        for (int b = 0; b < B; ++b) { poff[b] = tok_off[b]; plen[b] = tok_len[b]; }
        memcpy(pcu, cu, (size_t)(B + 1) * 4);
        HIPCHK(h, hipMemcpyAsync(h->d_tok_off, poff, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_tok_len, plen, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_cu, pcu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, h->stream));
        launch_row_maps(h->d_tok_off, h->d_tok_len, B, h->d_tok_seq, h->d_tok_pos, h->d_tok_valid, Rt, h->stream);
        const hipMemcpyKind kind = dev_in ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIPCHK(h, hipMemcpyAsync(ab.d_ling, ling, (size_t)NT * 8, kind, h->stream));
        HIPCHK(h, hipMemcpyAsync(ab.d_spk, speaker, (size_t)B * 8, kind, h->stream));
        HIPCHK(h, hipMemcpyAsync(ab.d_style, style, (size_t)B * c.bert_dim * 4, kind, h->stream));
        HIPCHK(h, hipMemcpyAsync(ab.d_content, content, (size_t)B * c.bert_dim * 4, kind, h->stream));
        HIPCHK(h, hipMemcpyAsync(h->d_mel_len, mel_lens, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(ab.d_eoff, elem_off.data(), (size_t)B * 8, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(ab.d_seqs, h->aln_seqs.data(), (size_t)B * sizeof(AlignSeq), hipMemcpyHostToDevice, h->stream));
        if (!dev_mel) {
            HIPCHK(h, hipMemcpyAsync(ab.d_mel, mel, (size_t)total_frames * c.n_mels * mel_es, hipMemcpyHostToDevice, h->stream));
            if (pitch_frames) HIPCHK(h, hipMemcpyAsync(ab.d_pf, pitch_frames, (size_t)total_frames * 4, hipMemcpyHostToDevice, h->stream));
            if (energy_frames) HIPCHK(h, hipMemcpyAsync(ab.d_ef, energy_frames, (size_t)total_frames * 4, hipMemcpyHostToDevice, h->stream));
        }
    }
    const void* melsrc = dev_mel ? mel : ab.d_mel;
    const float* pf = dev_mel ? pitch_frames : ab.d_pf;
    const float* ef = dev_mel ? energy_frames : ab.d_ef;
    region_begin(h, "total");
    // text side: the token-rate path of ev_synthesize up to embed_projection1 (same kernels, same layout: the same x_proj bits)
    RowCtx trc{Rt, h->d_tok_valid, h->d_tok_seq, h->d_tok_off, h->d_tok_len, B, max_tok, (double)NT};
    WPTR(tok_emb, float, "tok_emb"); WPTR(spk_emb, float, "spk_emb");
    float enc_alpha;
    if (get_scalar(h, "enc.alpha", &enc_alpha)) return -1;
    { KScope ks(h, "embed_pe", 0, (double)NT * C * 12.0);
      launch_embed_pe(ab.d_ling, h->d_cu, h->d_tok_seq, h->d_tok_pos, tok_emb, c.n_vocab, h->pe_dev, enc_alpha, (float*)ab.x.p, nullptr, Rt, C, h->stream); }
    if (run_stack(h, "enc", c.enc_layers, DT_F32, trc, ab.x, ab.hb, ab.qkv, ab.ctx, ab.ffn, ab.y, nullptr, nullptr)) return -1;
    WPTR(wcond, float, "proj.wcond"); WPTR(bproj, float, "proj.b"); WPTR(wproj, char, "proj.w32");
    { KScope ks(h, "cond_vector", 2.0 * B * C * (C + 2.0 * c.bert_dim), 0);
      launch_cond_vector(ab.d_spk, ab.d_style, ab.d_content, spk_emb, c.n_speaker, wcond, bproj, ab.d_u, B, C, c.bert_dim, h->stream); }
    {
        ConvGemmParams p = gemm_defaults();
        p.dtype = DT_F32; p.A = ab.y.p; p.lda = C; p.W = wproj; p.M = Rt; p.N = C; p.K = C; p.row_valid = h->d_tok_valid;
        p.row_seq = h->d_tok_seq; p.seq_bias = ab.d_u; p.ld_seq_bias = C; p.out32 = (float*)ab.xp.p; p.ldo = C;
        if (tok_weights(h, "proj.w", p)) return -1;
        if (gemm(h, "variance_f32_gemm", p, NT)) return -1;
    }
    // the aligner's convs (split-precision GEMMs whatever the frame-rate precision): text on the token rows, mel on the frame rows
    auto aln_conv = [&](const char* w, const void* A, int lda, int K, int taps, int act, const Buf& o, const RowCtx& rc) -> int {
        WPTR(bias, float, std::string("aln.") + w + ".b");
        ConvGemmParams p = gemm_defaults();
        p.dtype = DT_F32; p.A = A; p.lda = lda; p.M = rc.R; p.N = C; p.K = K; p.taps = taps; p.center = (taps - 1) / 2; p.bias = bias;
        p.row_valid = rc.valid; p.act = act; p.out32 = (float*)o.p; p.ldo = C;
        if (tok_weights(h, std::string("aln.") + w + ".w", p)) return -1;
        return gemm(h, "align_f32_gemm", p, rc.n_valid);
    };
    RowCtx frc{Rf, h->d_frm_valid, h->d_frm_seq, h->d_frm_off, h->d_mel_len, B, max_frames, (double)total_frames};
    if (aln_conv("t1", ab.xp.p, C, C, 3, ACT_RELU, ab.t1, trc) || aln_conv("t2", ab.t1.p, C, C, 1, ACT_NONE, ab.t2, trc)) return -1;
    { KScope ks(h, "mel_to_rows", 0, (double)total_frames * c.n_mels * (mel_es + 4));
      launch_mel_to_rows(melsrc, mel_is_f16, ab.d_eoff, h->d_frm_seq, h->d_frm_pos, h->d_mel_len, ab.melrows.p, 1, Rf, c.n_mels, MEL_PAD, h->stream); }
    if (aln_conv("f1", ab.melrows.p, MEL_PAD, MEL_PAD, 3, ACT_RELU, ab.f1, frc) || aln_conv("f2", ab.f1.p, C, C, 3, ACT_RELU, ab.f2, frc) ||
        aln_conv("f3", ab.f2.p, C, C, 1, ACT_NONE, ab.f3, frc)) return -1;
    { KScope ks(h, "align_score", 3.0 * (double)lp_elems * C, (double)lp_elems * 8.0 + (double)(NT + total_frames) * C * 4.0);
      launch_align_score((const float*)ab.t2.p, (const float*)ab.f3.p, C, ab.d_seqs, B, max_frames, ab.d_lp, h->stream); }
    { KScope ks(h, "align_mas", 2.0 * (double)lp_elems, (double)lp_elems * 4.0 + (double)total_frames * 64 * 4 * 2);
      launch_align_mas(ab.d_lp, ab.d_seqs, B, max_tok, ab.d_bits, pf, ef, ab.d_dur, ab.d_pitch, ab.d_energy, ab.d_score, h->stream); }
    HIPCHK(h, hipGetLastError());
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    profiling_collect(h);
    h->aln_lp = ab.d_lp; h->aln_lp_elems = lp_elems;
    if (keep) {
        add_tap(h, "x_proj", ab.xp.p, DT_F32, C, C, 0, 0);
        add_tap(h, "aln_text", ab.t2.p, DT_F32, C, C, 0, 0);
        add_tap(h, "aln_feats", ab.f3.p, DT_F32, C, C, 1, 0);
    }
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz; out->batch = B; out->total_tokens = NT; out->total_frames = total_frames;
    out->durations = ab.d_dur; out->pitch = ab.d_pitch; out->energy = ab.d_energy; out->score = ab.d_score;
    out->mel_lens = h->aln_mel_lens.data(); out->mel_offsets = h->aln_mel_offs.data();
    return 0;
}

// ------------------------------------------------------------------- acoustic features (include/evhip.h: ev_features)
static_assert(EV_FEATURES_MAX_NFFT == STFT_MAX_NFFT && EV_FEATURES_MAX_MELS == STFT_MAX_MELS && EV_FEATURES_MAX_RUN == STFT_MAX_RUN,
              "include/evhip.h states the limits of ev_features.hip");
void ev_default_features_config(ev_features_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof(ev_features_config);
    c->n_fft = 1024; c->hop = 256; c->n_mels = 80; c->mel_clip = 1e-5f; c->energy_floor = 1e-10f;
}

static int features_check_config(ev_handle* h, const char* who, int n_fft, int hop, int n_mels) {
    if (n_fft < 128 || n_fft % 128 || n_fft > STFT_MAX_NFFT) return fail(h, "%s: n_fft %d must be a multiple of 128 in [128, %d]", who, n_fft, STFT_MAX_NFFT);
    if (n_mels < 1 || n_mels > STFT_MAX_MELS) return fail(h, "%s: n_mels %d outside [1, %d]", who, n_mels, STFT_MAX_MELS);
    if (hop < 8 || hop % 8 || hop > n_fft) return fail(h, "%s: hop %d must be a multiple of 8 in [8, n_fft]", who, hop);
    if (!stft_shape_ok(n_fft, hop, n_mels)) return fail(h, "%s: hop %d: the 63 hop + n_fft samples of a 64-frame tile exceed %d", who, hop, STFT_MAX_RUN);
    return 0;
}

// packs the basis planes on the host and uploads them; *basis / *melT are hipMalloc'ed
static int features_upload_tables(ev_handle* h, int n_fft, int n_mels, const float* mel_basis, const float* window, char** basis, float** melT) {
    std::vector<uint16_t> hb(stft_basis_halfs(n_fft));
    std::vector<float> hm(stft_melT_floats(n_fft));
    stft_pack_basis(n_fft, window, hb.data());
    stft_pack_mel(n_fft, n_mels, mel_basis, hm.data());
    *basis = nullptr; *melT = nullptr;
    hipError_t e = hipMalloc((void**)basis, hb.size() * 2);
    if (e == hipSuccess) e = hipMalloc((void**)melT, hm.size() * 4);
    if (e == hipSuccess) e = hipMemcpy(*basis, hb.data(), hb.size() * 2, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(*melT, hm.data(), hm.size() * 4, hipMemcpyHostToDevice);
    if (e != hipSuccess) {       // nothing half-built is left behind
        if (*basis) (void)hipFree(*basis);
        if (*melT) (void)hipFree(*melT);
        *basis = nullptr; *melT = nullptr;
        return fail(h, "ev_features: uploading the basis planes failed: %s", hipGetErrorString(e));
    }
    return 0;
}

int ev_features_setup(ev_handle* h, const ev_features_config* cfg) {
    if (!h) return -1;
    if (!cfg) return fail(h, "ev_features_setup: null config");
    if (cfg->struct_size != sizeof(ev_features_config))
        return fail(h, "ev_features_setup: struct_size %u != sizeof(ev_features_config) %zu", cfg->struct_size, sizeof(ev_features_config));
    if (features_check_config(h, "ev_features_setup", cfg->n_fft, cfg->hop, cfg->n_mels)) return -1;
    if (!cfg->mel_basis) return fail(h, "ev_features_setup: mel_basis is required");
    if (!(cfg->mel_clip > 0.f) || !std::isfinite(cfg->mel_clip)) return fail(h, "ev_features_setup: mel_clip must be positive and finite");
    if (!(cfg->energy_floor >= 0.f) || !std::isfinite(cfg->energy_floor)) return fail(h, "ev_features_setup: energy_floor must be >= 0 and finite");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    h->feat_ready = false;
    if (h->feat_basis) { HIPCHK(h, hipFree(h->feat_basis)); h->feat_basis = nullptr; }
    if (h->feat_melT) { HIPCHK(h, hipFree(h->feat_melT)); h->feat_melT = nullptr; }
    if (features_upload_tables(h, cfg->n_fft, cfg->n_mels, cfg->mel_basis, cfg->window, &h->feat_basis, &h->feat_melT)) return -1;
    h->fcfg = *cfg; h->fcfg.mel_basis = nullptr; h->fcfg.window = nullptr;
    h->feat_ready = true;
    return 0;
}

// frame counts, offsets and the tile table of a batch; 0 or the index + 1 of the first utterance that is too short (-(index + 1): too long)
static int features_layout(int B, const int64_t* wav_lens, int n_fft, int hop, std::vector<StftSeq>& seqs, std::vector<StftTile>& tiles,
                           std::vector<int32_t>& lens, std::vector<int64_t>& offs) {
    seqs.resize(B); lens.resize(B); offs.resize((size_t)B + 1); tiles.clear();
    int64_t wo = 0, fo = 0;
    for (int b = 0; b < B; ++b) {
        if (wav_lens[b] < n_fft / 2 + 1) return b + 1;
        const int64_t T = wav_lens[b] / hop + 1;
        if (T > EV_ALIGN_MAX_FRAMES) return -(b + 1);
        seqs[b] = StftSeq{wo, wav_lens[b], fo, (int32_t)T, 0};
        lens[b] = (int32_t)T; offs[b] = fo;
        for (int t0 = 0; t0 < T; t0 += 64) tiles.push_back(StftTile{b, t0});
        wo += wav_lens[b]; fo += T;
    }
    offs[B] = fo;
    return 0;
}

int ev_features(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* wav_lens, float energy_mean, float energy_std, uint32_t flags,
                ev_features_result* out) {
    if (!h) return -1;
    if (!wav || !wav_lens || !out || B <= 0) return fail(h, "ev_features: bad argument");
    if (out->struct_size != sizeof(ev_features_result))
        return fail(h, "ev_features: out->struct_size %u != sizeof(ev_features_result) %zu", out->struct_size, sizeof(ev_features_result));
    if (!h->feat_ready) return fail(h, "ev_features: ev_features_setup has not been called");
    if ((size_t)B > PIN_MAX_B) return fail(h, "ev_features: at most %zu utterances per call", PIN_MAX_B);
    if (!std::isfinite(energy_std) || !(energy_std > 0.f)) return fail(h, "ev_features: energy_std must be positive and finite");
    if (!std::isfinite(energy_mean)) return fail(h, "ev_features: energy_mean must be finite");
    const ev_features_config& fc = h->fcfg;
    const int n_bins = fc.n_fft / 2 + 1;
    std::vector<StftSeq> seqs; std::vector<StftTile> tiles; std::vector<int32_t> lens; std::vector<int64_t> offs;
    const int bad = features_layout(B, wav_lens, fc.n_fft, fc.hop, seqs, tiles, lens, offs);
    if (bad > 0) return fail(h, "ev_features: wav_lens[%d] = %lld < n_fft / 2 + 1 = %d (reflect padding needs that many samples)", bad - 1, (long long)wav_lens[bad - 1], fc.n_fft / 2 + 1);
    if (bad < 0) return fail(h, "ev_features: utterance %d has %lld frames > EV_ALIGN_MAX_FRAMES %d", -bad - 1, (long long)(wav_lens[-bad - 1] / fc.hop + 1), EV_ALIGN_MAX_FRAMES);
    const int64_t total_frames = offs[B], total_samples = seqs[B - 1].wav_off + seqs[B - 1].len;
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0, keep = h->cfg.keep_stages != 0;
    const size_t es = wav_is_i16 ? 2 : 4;
    HIPCHK(h, hipSetDevice(h->device));
    profiling_reset(h);
    h->feat_mag = nullptr;
    void* d_wav = nullptr; StftSeq* d_seqs = nullptr; StftTile* d_tiles = nullptr; float *d_mel = nullptr, *d_energy = nullptr, *d_mag = nullptr;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 4, pass == 0};
        if (pass == 1 && arena_reserve(h, 4, need)) return -1;
        d_wav = dev_in ? nullptr : ap.take((size_t)total_samples * es);
        d_seqs = ap.arr<StftSeq>(B); d_tiles = ap.arr<StftTile>(tiles.size());
        d_mel = ap.arr<float>((size_t)total_frames * fc.n_mels); d_energy = ap.arr<float>((size_t)total_frames);
        d_mag = keep ? ap.arr<float>((size_t)total_frames * n_bins) : nullptr;
        need = ap.off;
    }
    if (!dev_in) HIPCHK(h, hipMemcpyAsync(d_wav, wav, (size_t)total_samples * es, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_seqs, seqs.data(), (size_t)B * sizeof(StftSeq), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(StftTile), hipMemcpyHostToDevice, h->stream));
    region_begin(h, "total");
    {
        StftParams p{};
        p.wav = dev_in ? wav : d_wav; p.wav_is_i16 = wav_is_i16 != 0; p.seqs = d_seqs; p.tiles = d_tiles; p.n_tiles = (int)tiles.size();
        p.basis = h->feat_basis; p.melT = h->feat_melT; p.n_fft = fc.n_fft; p.hop = fc.hop; p.n_mels = fc.n_mels; p.nmi = stft_mels_per_group(fc.n_mels);
        p.n_bins = n_bins; p.n_btiles = stft_bin_tiles(fc.n_fft); p.mel_clip = fc.mel_clip; p.energy_floor = fc.energy_floor;
        p.energy_mean = energy_mean; p.energy_std = energy_std; p.mel = d_mel; p.energy = d_energy; p.mag = d_mag;
        const double tile_frames = 64.0 * (double)tiles.size();
        KScope ks(h, "stft_mel", 2.0 * 3.0 * tile_frames * fc.n_fft * 2.0 * n_bins + 2.0 * tile_frames * n_bins * fc.n_mels,
                  (double)total_samples * es + (double)total_frames * (fc.n_mels + 1) * 4.0);
        if (launch_stft_mel(p, h->stream)) return fail(h, "ev_features: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    profiling_collect(h);
    h->feat_mel_lens = lens; h->feat_mel_offs = offs;
    h->feat_mag = d_mag; h->feat_mag_elems = keep ? total_frames * n_bins : 0;
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz; out->batch = B; out->total_frames = total_frames; out->mel = d_mel; out->energy = d_energy;
    out->mel_lens = h->feat_mel_lens.data(); out->mel_offsets = h->feat_mel_offs.data();
    return 0;
}

// ------------------------------------------------------------------- pitch extraction (include/evhip.h: ev_pitch)
static_assert(EV_PITCH_TILE_FRAMES == PITCH_TF && EV_PITCH_MAX_WIN == PITCH_MAX_WIN && EV_PITCH_MAX_LDS == PITCH_MAX_LDS,
              "include/evhip.h states the limits of ev_pitch.hip");
void ev_default_pitch_config(ev_pitch_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof(ev_pitch_config);
    c->sample_rate = 16000; c->hop = 256; c->win = 1024; c->f_min = 80.f; c->f_max = 400.f; c->threshold = 0.15f; c->silence_rms = 1e-3f;
}

// every rejection of a config, in the order include/evhip.h lists them; sets the lag range
static int pitch_check_config(ev_handle* h, const char* who, const ev_pitch_config& c, int* tau_min, int* tau_max) {
    if (c.sample_rate < 1) return fail(h, "%s: sample_rate %d must be positive", who, c.sample_rate);
    if (c.win < 1 || c.win > PITCH_MAX_WIN) return fail(h, "%s: win %d outside [1, EV_PITCH_MAX_WIN %d]", who, c.win, PITCH_MAX_WIN);
    if (c.hop < 1 || c.hop > c.win) return fail(h, "%s: hop %d outside [1, win %d]", who, c.hop, c.win);
    if (!std::isfinite(c.f_min) || !std::isfinite(c.f_max) || !(c.f_min > 0.f) || !(c.f_min < c.f_max) || !((double)c.f_max <= (double)c.sample_rate / 4.0))
        return fail(h, "%s: f_min %g / f_max %g must be finite with 0 < f_min < f_max <= sample_rate / 4 = %g", who, (double)c.f_min, (double)c.f_max, (double)c.sample_rate / 4.0);
    const double tmax = std::ceil((double)c.sample_rate / (double)c.f_min);
    const int tmin = (int)std::floor((double)c.sample_rate / (double)c.f_max);
    if (tmax + 1.0 > (double)c.win) return fail(h, "%s: tau_max + 1 = %.0f > win %d (f_min %g is too low for the window)", who, tmax + 1.0, c.win, (double)c.f_min);
    if (!(c.threshold > 0.f) || !(c.threshold <= 1.f)) return fail(h, "%s: threshold %g outside (0, 1]", who, (double)c.threshold);
    if (!std::isfinite(c.silence_rms) || c.silence_rms < 0.f) return fail(h, "%s: silence_rms must be >= 0 and finite", who);
    if (!pitch_shape_ok(c.hop, c.win, tmin, (int)tmax))
        return fail(h, "%s: win %d, hop %d, tau %d .. %d: the kernel needs win >= 8, tau_min < tau_max and a tile of %zu bytes within EV_PITCH_MAX_LDS %d", who,
                    c.win, c.hop, tmin, (int)tmax, pitch_lds_bytes(c.hop, c.win, (int)tmax), PITCH_MAX_LDS);
    *tau_min = tmin; *tau_max = (int)tmax;
    return 0;
}

// frame counts, offsets and the tile table of a batch; 0 or the index + 1 of the first empty utterance (-(index + 1): too long)
static int pitch_layout(int B, const int64_t* wav_lens, int hop, std::vector<StftSeq>& seqs, std::vector<StftTile>& tiles, std::vector<int32_t>& lens,
                        std::vector<int64_t>& offs) {
    seqs.resize(B); lens.resize(B); offs.resize((size_t)B + 1); tiles.clear();
    int64_t wo = 0, fo = 0;
    for (int b = 0; b < B; ++b) {
        if (wav_lens[b] < 1) return b + 1;
        const int64_t T = wav_lens[b] / hop + 1;
        if (T > EV_ALIGN_MAX_FRAMES) return -(b + 1);
        seqs[b] = StftSeq{wo, wav_lens[b], fo, (int32_t)T, 0};
        lens[b] = (int32_t)T; offs[b] = fo;
        for (int t0 = 0; t0 < T; t0 += PITCH_TF) tiles.push_back(StftTile{b, t0});
        wo += wav_lens[b]; fo += T;
    }
    offs[B] = fo;
    return 0;
}

static PitchParams pitch_params(const ev_pitch_config& c, int tau_min, int tau_max) {
    PitchParams p{};
    p.sample_rate = c.sample_rate; p.hop = c.hop; p.win = c.win; p.tau_min = tau_min; p.tau_max = tau_max; p.threshold = c.threshold;
    p.e0_floor = (double)c.win * (double)c.silence_rms * (double)c.silence_rms;
    return p;
}

int ev_pitch(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* wav_lens, const ev_pitch_config* cfg, float pitch_mean,
             float pitch_std, uint32_t flags, ev_pitch_result* out) {
    if (!h) return -1;
    if (!wav || !wav_lens || !out || B <= 0) return fail(h, "ev_pitch: bad argument");
    if (out->struct_size != sizeof(ev_pitch_result))
        return fail(h, "ev_pitch: out->struct_size %u != sizeof(ev_pitch_result) %zu", out->struct_size, sizeof(ev_pitch_result));
    ev_pitch_config pc;
    ev_default_pitch_config(&pc);
    if (cfg) {
        if (cfg->struct_size != sizeof(ev_pitch_config))
            return fail(h, "ev_pitch: cfg->struct_size %u != sizeof(ev_pitch_config) %zu", cfg->struct_size, sizeof(ev_pitch_config));
        pc = *cfg;
    }
    int tau_min = 0, tau_max = 0;
    if (pitch_check_config(h, "ev_pitch", pc, &tau_min, &tau_max)) return -1;
    if ((size_t)B > PIN_MAX_B) return fail(h, "ev_pitch: at most %zu utterances per call", PIN_MAX_B);
    if (!std::isfinite(pitch_std) || !(pitch_std > 0.f)) return fail(h, "ev_pitch: pitch_std must be positive and finite");
    if (!std::isfinite(pitch_mean)) return fail(h, "ev_pitch: pitch_mean must be finite");
    std::vector<StftSeq> seqs; std::vector<StftTile> tiles; std::vector<int32_t> lens; std::vector<int64_t> offs;
    const int bad = pitch_layout(B, wav_lens, pc.hop, seqs, tiles, lens, offs);
    if (bad > 0) return fail(h, "ev_pitch: wav_lens[%d] = %lld < 1", bad - 1, (long long)wav_lens[bad - 1]);
    if (bad < 0) return fail(h, "ev_pitch: utterance %d has %lld frames > EV_ALIGN_MAX_FRAMES %d", -bad - 1, (long long)(wav_lens[-bad - 1] / pc.hop + 1), EV_ALIGN_MAX_FRAMES);
    const int64_t total_frames = offs[B], total_samples = seqs[B - 1].wav_off + seqs[B - 1].len;
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0;
    const size_t es = wav_is_i16 ? 2 : 4;
    HIPCHK(h, hipSetDevice(h->device));
    profiling_reset(h);
    void* d_wav = nullptr; StftSeq* d_seqs = nullptr; StftTile* d_tiles = nullptr; float *d_pitch = nullptr, *d_f0 = nullptr, *d_ap = nullptr;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 5, pass == 0};
        if (pass == 1 && arena_reserve(h, 5, need)) return -1;
        d_wav = dev_in ? nullptr : ap.take((size_t)total_samples * es);
        d_seqs = ap.arr<StftSeq>(B); d_tiles = ap.arr<StftTile>(tiles.size());
        d_pitch = ap.arr<float>((size_t)total_frames); d_f0 = ap.arr<float>((size_t)total_frames); d_ap = ap.arr<float>((size_t)total_frames);
        need = ap.off;
    }
    if (!dev_in) HIPCHK(h, hipMemcpyAsync(d_wav, wav, (size_t)total_samples * es, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_seqs, seqs.data(), (size_t)B * sizeof(StftSeq), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(StftTile), hipMemcpyHostToDevice, h->stream));
    region_begin(h, "total");
    {
        PitchParams p = pitch_params(pc, tau_min, tau_max);
        p.wav = dev_in ? wav : d_wav; p.wav_is_i16 = wav_is_i16 != 0; p.seqs = d_seqs; p.tiles = d_tiles; p.n_tiles = (int)tiles.size();
        p.f0 = d_f0; p.ap = d_ap; p.tau = nullptr;
        KScope ks(h, "pitch_yin", 3.0 * (double)total_frames * (tau_max + 2.0) * pc.win, (double)total_samples * es + (double)total_frames * 8.0);
        if (launch_pitch_yin(p, h->stream)) return fail(h, "ev_pitch: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {
        KScope ks(h, "pitch_fill", 8.0 * (double)total_frames, (double)total_frames * 8.0);
        launch_pitch_fill(d_f0, d_seqs, B, pitch_mean, pitch_std, d_pitch, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    profiling_collect(h);
    h->pit_mel_lens = lens; h->pit_mel_offs = offs;
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz; out->batch = B; out->total_frames = total_frames; out->pitch = d_pitch; out->f0_hz = d_f0; out->aperiodicity = d_ap;
    out->mel_lens = h->pit_mel_lens.data(); out->mel_offsets = h->pit_mel_offs.data();
    return 0;
}

// ------------------------------------------------------------------- sample-rate conversion and trimming (include/evhip.h: ev_resample)
static_assert(EV_RESAMPLE_TILE == RS_TM, "include/evhip.h states the tile of ev_resample.hip");
static const int64_t RS_MAX_OUT = (int64_t)EV_ALIGN_MAX_FRAMES * 256;
void ev_default_resample_config(ev_resample_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof(ev_resample_config);
    c->sr_in = 16000; c->sr_out = 16000;
}

static double bessel_i0(double x) {      // the power series: every term positive, so it converges to the last bit for any x >= 0
    const double q = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 1000; ++k) {
        term *= q / ((double)k * (double)k);
        sum += term;
        if (term < 1e-17 * sum) break;
    }
    return sum;
}

static int resample_ratio(int sr_in, int sr_out, int* up, int* down) {      // 0, or -1 for a rate < 1
    if (sr_in < 1 || sr_out < 1) return -1;
    int a = sr_in, b = sr_out;
    while (b) { const int t = a % b; a = b; b = t; }
    *up = sr_out / a; *down = sr_in / a;
    return 0;
}

int ev_resample_design(int sr_in, int sr_out, int zeros, double rolloff, double beta, float* taps, int cap) {
    int up = 0, down = 0;
    if (resample_ratio(sr_in, sr_out, &up, &down) || up > EV_RESAMPLE_MAX_RATIO || down > EV_RESAMPLE_MAX_RATIO) return 0;
    if (zeros < 1 || zeros > 4096 || !(rolloff > 0.0) || !(rolloff <= 1.0) || !std::isfinite(beta) || beta < 0.0) return 0;
    const int q = std::max(up, down), half = zeros * q, n = 2 * half + 1;
    if (cap < n || !taps) return -n;
    std::vector<double> g((size_t)n);
    const double i0b = bessel_i0(beta);
    double sum = 0.0;
    for (int i = -half; i <= half; ++i) {
        const double x = rolloff * (double)i / (double)q, r = (double)i / (double)half;
        const double px = M_PI * x;
        const double sinc = i == 0 ? 1.0 : sin(px) / px;
        g[(size_t)(i + half)] = sinc * bessel_i0(beta * sqrt(std::max(0.0, 1.0 - r * r))) / i0b;
    }
    for (int i = 0; i < n; ++i) sum += g[(size_t)i];
    for (int i = 0; i < n; ++i) taps[i] = (float)((double)up * g[(size_t)i] / sum);
    return half;
}

// every rejection of a config, in the order include/evhip.h lists them; gives the ratio and the taps (the caller's or the default design)
static int resample_check_config(ev_handle* h, const char* who, const ev_resample_config& c, int* up, int* down, int* half, std::vector<float>& taps) {
    if (c.sr_in < 1 || c.sr_out < 1) return fail(h, "%s: sr_in %d / sr_out %d must be positive", who, c.sr_in, c.sr_out);
    (void)resample_ratio(c.sr_in, c.sr_out, up, down);
    if (*up > EV_RESAMPLE_MAX_RATIO || *down > EV_RESAMPLE_MAX_RATIO)
        return fail(h, "%s: sr_in %d -> sr_out %d is up %d / down %d; both must be <= EV_RESAMPLE_MAX_RATIO %d", who, c.sr_in, c.sr_out, *up, *down, EV_RESAMPLE_MAX_RATIO);
    if (c.taps) {
        if (c.half_len < 1) return fail(h, "%s: half_len %d must be >= 1 with taps", who, c.half_len);
        if (2 * (int64_t)c.half_len + 1 > EV_RESAMPLE_MAX_TAPS) return fail(h, "%s: half_len %d gives more than EV_RESAMPLE_MAX_TAPS %d taps", who, c.half_len, EV_RESAMPLE_MAX_TAPS);
        taps.assign(c.taps, c.taps + 2 * (size_t)c.half_len + 1);
        for (size_t i = 0; i < taps.size(); ++i)
            if (!std::isfinite(taps[i])) return fail(h, "%s: taps[%zu] is not finite", who, i);
        *half = c.half_len;
    } else {
        const int n = -ev_resample_design(c.sr_in, c.sr_out, 16, 0.945, 9.0, nullptr, 0);
        if (n < 3 || n > EV_RESAMPLE_MAX_TAPS) return fail(h, "%s: the default design has %d taps > EV_RESAMPLE_MAX_TAPS %d", who, n, EV_RESAMPLE_MAX_TAPS);
        taps.resize((size_t)n);
        *half = ev_resample_design(c.sr_in, c.sr_out, 16, 0.945, 9.0, taps.data(), n);
    }
    if (!std::isfinite(c.trim_frac) || c.trim_frac < 0.f || !(c.trim_frac < 1.f)) return fail(h, "%s: trim_frac %g outside [0, 1)", who, (double)c.trim_frac);
    if (c.trim_pad < 0) return fail(h, "%s: trim_pad %d must be >= 0", who, c.trim_pad);
    return 0;
}

// the table on the device (hipMalloc'ed); nothing half-built is left behind
static int resample_upload_table(int up, int half, const std::vector<float>& taps, float** tab, size_t* floats) {
    std::vector<float> ht(resample_table_floats(up, half));
    resample_pack_table(up, half, taps.data(), ht.data());
    *tab = nullptr;
    if (hipMalloc((void**)tab, ht.size() * 4) != hipSuccess) return -1;
    if (hipMemcpy(*tab, ht.data(), ht.size() * 4, hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(*tab); *tab = nullptr; return -1; }
    *floats = ht.size();
    return 0;
}

int ev_resample_setup(ev_handle* h, const ev_resample_config* cfg) {
    if (!h) return -1;
    if (!cfg) return fail(h, "ev_resample_setup: null config");
    if (cfg->struct_size != sizeof(ev_resample_config))
        return fail(h, "ev_resample_setup: struct_size %u != sizeof(ev_resample_config) %zu", cfg->struct_size, sizeof(ev_resample_config));
    int up = 0, down = 0, half = 0;
    std::vector<float> taps;
    if (resample_check_config(h, "ev_resample_setup", *cfg, &up, &down, &half, taps)) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    float* tab = nullptr; size_t floats = 0;
    if (resample_upload_table(up, half, taps, &tab, &floats)) return fail(h, "ev_resample_setup: uploading the tap table failed");
    if (h->rs_tab) (void)hipFree(h->rs_tab);
    h->rs_tab = tab; h->rs_tab_floats = floats; h->rs_up = up; h->rs_down = down; h->rs_half = half;
    h->rcfg = *cfg; h->rcfg.taps = nullptr;
    h->rs_ready = true;
    return 0;
}

// output lengths, offsets and the tile table of a batch; 0 or the index + 1 of the first empty utterance (-(index + 1): too long with `extra` added)
static int resample_layout(int B, const int64_t* wav_lens, int up, int down, int64_t extra, std::vector<ResampleSeq>& seqs, std::vector<ResampleTile>& tiles) {
    seqs.resize(B); tiles.clear();
    int64_t io = 0, oo = 0;
    for (int b = 0; b < B; ++b) {
        if (wav_lens[b] < 1) return b + 1;
        if (wav_lens[b] > RS_MAX_OUT * EV_RESAMPLE_MAX_RATIO) return -(b + 1);      // keeps L up inside int64
        const int64_t n = (wav_lens[b] * up + down - 1) / down;
        if (n + extra > RS_MAX_OUT) return -(b + 1);
        seqs[b] = ResampleSeq{io, wav_lens[b], oo, n};
        for (int64_t m0 = 0; m0 < n; m0 += RS_TM) tiles.push_back(ResampleTile{b, (int32_t)m0});
        io += wav_lens[b]; oo += n;
    }
    return 0;
}

static int resample_launch(const void* wav, int wav_is_i16, int up, int down, int half, const float* tab, const ResampleSeq* d_seqs, const ResampleTile* d_tiles,
                           int n_tiles, int64_t total_in, float* y, hipStream_t s) {
    if (up == 1 && down == 1) { launch_resample_copy(wav, wav_is_i16, total_in, y, s); return 0; }
    ResampleParams p{};
    p.wav = wav; p.wav_is_i16 = wav_is_i16; p.seqs = d_seqs; p.tiles = d_tiles; p.n_tiles = n_tiles;
    p.up = up; p.down = down; p.half = half; p.row = resample_row_len(up, half); p.tab = tab; p.out = y;
    return launch_resample_poly(p, s);
}

// cuts (first, last per utterance, from trim_scan) -> the result's lens / offsets / start / end and the gather table; returns the longest output
static int64_t trim_plan(int B, const std::vector<ResampleSeq>& seqs, const int64_t* cuts, int pad, std::vector<TrimSeq>& ts, int64_t* lens, int64_t* offs,
                         int64_t* start, int64_t* end) {
    ts.resize(B);
    int64_t o = 0, longest = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t s = cuts[2 * b], e = cuts[2 * b + 1], n = e - s + 2 * (int64_t)pad;
        ts[b] = TrimSeq{seqs[b].out_off + s, o, e - s};
        lens[b] = n; start[b] = s; end[b] = e;
        if (offs) offs[b] = o;
        o += n; longest = std::max(longest, n);
    }
    if (offs) offs[B] = o;
    return longest;
}

int ev_resample(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* wav_lens, uint32_t flags, ev_resample_result* out) {
    if (!h) return -1;
    if (!wav || !wav_lens || !out) return fail(h, "ev_resample: bad argument");
    if (out->struct_size != sizeof(ev_resample_result))
        return fail(h, "ev_resample: out->struct_size %u != sizeof(ev_resample_result) %zu", out->struct_size, sizeof(ev_resample_result));
    if (!h->rs_ready) return fail(h, "ev_resample: ev_resample_setup has not been called");
    if (B < 1 || B > 65535) return fail(h, "ev_resample: B %d outside [1, 65535]", B);
    const ev_resample_config& rc = h->rcfg;
    const int up = h->rs_up, down = h->rs_down, half = h->rs_half, pad = rc.trim_pad;
    const bool trim = rc.trim_frac > 0.f;
    std::vector<ResampleSeq> seqs; std::vector<ResampleTile> tiles;
    const int bad = resample_layout(B, wav_lens, up, down, trim ? 2 * (int64_t)pad : 0, seqs, tiles);
    if (bad > 0) return fail(h, "ev_resample: wav_lens[%d] = %lld < 1", bad - 1, (long long)wav_lens[bad - 1]);
    if (bad < 0) return fail(h, "ev_resample: utterance %d (%lld samples) gives more than EV_ALIGN_MAX_FRAMES * 256 = %lld output samples", -bad - 1,
                             (long long)wav_lens[-bad - 1], (long long)RS_MAX_OUT);
    const int64_t total_in = seqs[B - 1].in_off + seqs[B - 1].len, total_n = seqs[B - 1].out_off + seqs[B - 1].n;
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0, keep = h->cfg.keep_stages != 0;
    const size_t es = wav_is_i16 ? 2 : 4;
    HIPCHK(h, hipSetDevice(h->device));
    profiling_reset(h);
    h->rs_raw = nullptr;
    void* d_wav = nullptr; ResampleSeq* d_seqs = nullptr; ResampleTile* d_tiles = nullptr; TrimSeq* d_ts = nullptr; int64_t* d_cuts = nullptr;
    float *d_y = nullptr, *d_out = nullptr;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 6, pass == 0};
        if (pass == 1 && arena_reserve(h, 6, need)) return -1;
        d_wav = dev_in ? nullptr : ap.take((size_t)total_in * es);
        d_seqs = ap.arr<ResampleSeq>(B); d_tiles = ap.arr<ResampleTile>(tiles.size());
        d_y = ap.arr<float>((size_t)total_n);
        if (trim) { d_ts = ap.arr<TrimSeq>(B); d_cuts = ap.arr<int64_t>(2 * (size_t)B); d_out = ap.arr<float>((size_t)total_n + 2 * (size_t)pad * B); }
        need = ap.off;
    }
    if (!dev_in) HIPCHK(h, hipMemcpyAsync(d_wav, wav, (size_t)total_in * es, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_seqs, seqs.data(), (size_t)B * sizeof(ResampleSeq), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(ResampleTile), hipMemcpyHostToDevice, h->stream));
    std::vector<int64_t> lens((size_t)B), offs((size_t)B + 1), start((size_t)B), end((size_t)B);
    region_begin(h, "total");
    {
        const bool copy = up == 1 && down == 1;
        KScope ks(h, copy ? "resample_copy" : "resample_poly", copy ? 0.0 : 2.0 * (double)total_n * (2.0 * half / up + 1.0), (double)total_in * es + (double)total_n * 4.0);
        if (resample_launch(dev_in ? wav : d_wav, wav_is_i16 != 0, up, down, half, h->rs_tab, d_seqs, d_tiles, (int)tiles.size(), total_in, d_y, h->stream))
            return fail(h, "ev_resample: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    if (trim) {
        {
            KScope ks(h, "trim_scan", 2.0 * (double)total_n, 2.0 * (double)total_n * 4.0);
            launch_trim_scan(d_y, d_seqs, B, rc.trim_frac, d_cuts, h->stream);
        }
        HIPCHK(h, hipGetLastError());
        std::vector<int64_t> cuts(2 * (size_t)B);
        HIPCHK(h, hipMemcpyAsync(cuts.data(), d_cuts, cuts.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        std::vector<TrimSeq> ts;
        const int64_t longest = trim_plan(B, seqs, cuts.data(), pad, ts, lens.data(), offs.data(), start.data(), end.data());
        HIPCHK(h, hipMemcpyAsync(d_ts, ts.data(), (size_t)B * sizeof(TrimSeq), hipMemcpyHostToDevice, h->stream));
        {
            KScope ks(h, "trim_gather", 0.0, 2.0 * (double)offs[B] * 4.0);
            launch_trim_gather(d_y, d_ts, B, longest, pad, d_out, h->stream);
        }
        HIPCHK(h, hipGetLastError());
    } else {
        for (int b = 0; b < B; ++b) { lens[b] = seqs[b].n; offs[b] = seqs[b].out_off; start[b] = 0; end[b] = seqs[b].n; }
        offs[B] = total_n;
    }
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    profiling_collect(h);
    h->rs_lens = lens; h->rs_offs = offs; h->rs_start = start; h->rs_end = end;
    h->rs_raw = keep ? d_y : nullptr; h->rs_raw_elems = keep ? total_n : 0;
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz; out->batch = B; out->total_samples = offs[B]; out->wav = trim ? d_out : d_y;
    out->wav_lens = h->rs_lens.data(); out->wav_offsets = h->rs_offs.data(); out->trim_start = h->rs_start.data(); out->trim_end = h->rs_end.data();
    return 0;
}

// ------------------------------------------------------------------- long-form stitching (include/evhip.h: ev_stitch)
static_assert(EV_STITCH_MAX_FADE == ST_MAX_FADE, "include/evhip.h states the ramp table's limit of ev_stitch.hip");
void ev_default_stitch_config(ev_stitch_config* c) {
    if (!c) return;
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof(ev_stitch_config);
}

int ev_stitch_ramp(int F, float* tab) {
    if (F < 0 || F > EV_STITCH_MAX_FADE || (F > 0 && !tab)) return -1;
    for (int i = 0; i < F; ++i) tab[i] = (float)(0.5 - 0.5 * cos(M_PI * ((double)i + 0.5) / (double)F));
    return F;
}

static int stitch_check_trim(ev_handle* h, const char* who, float trim_frac, float trim_abs) {
    if (!std::isfinite(trim_frac) || trim_frac < 0.f || !(trim_frac < 1.f)) return fail(h, "%s: trim_frac %g outside [0, 1)", who, (double)trim_frac);
    if (!std::isfinite(trim_abs) || trim_abs < 0.f) return fail(h, "%s: trim_abs %g must be finite and >= 0", who, (double)trim_abs);
    return 0;
}

// the config and the per-segment arrays that do not depend on the waveform: the number of documents, or -1 with the message
static int stitch_check(ev_handle* h, const char* who, int S, const int32_t* seg_doc, const int32_t* pause_after, const ev_stitch_config* c) {
    if (!c || !seg_doc || !pause_after) return fail(h, "%s: bad argument", who);
    if (c->struct_size != sizeof(ev_stitch_config))
        return fail(h, "%s: cfg->struct_size %u != sizeof(ev_stitch_config) %zu", who, c->struct_size, sizeof(ev_stitch_config));
    if (S < 1 || S > 65535) return fail(h, "%s: S %d outside [1, 65535]", who, S);
    if (stitch_check_trim(h, who, c->trim_frac, c->trim_abs)) return -1;
    if (c->keep < 0) return fail(h, "%s: keep %d must be >= 0", who, c->keep);
    if (c->fade < 0 || c->fade > EV_STITCH_MAX_FADE) return fail(h, "%s: fade %d outside [0, EV_STITCH_MAX_FADE = %d]", who, c->fade, EV_STITCH_MAX_FADE);
    if (c->lead < 0) return fail(h, "%s: lead %d must be >= 0", who, c->lead);
    if (c->tail < 0) return fail(h, "%s: tail %d must be >= 0", who, c->tail);
    if (seg_doc[0] != 0) return fail(h, "%s: seg_doc[0] = %d, the documents count from 0", who, seg_doc[0]);
    for (int s = 1; s < S; ++s)
        if (seg_doc[s] != seg_doc[s - 1] && seg_doc[s] != seg_doc[s - 1] + 1)
            return fail(h, "%s: seg_doc[%d] = %d after %d: neither the same document nor the next", who, s, seg_doc[s], seg_doc[s - 1]);
    for (int s = 0; s + 1 < S; ++s)
        if (seg_doc[s + 1] == seg_doc[s] && (pause_after[s] < -EV_STITCH_MAX_FADE || pause_after[s] > EV_STITCH_MAX_PAUSE))
            return fail(h, "%s: pause_after[%d] = %d outside [-EV_STITCH_MAX_FADE, EV_STITCH_MAX_PAUSE]", who, s, pause_after[s]);
    return seg_doc[S - 1] + 1;
}

int ev_stitch_plan(int S, const int64_t* n, const int32_t* seg_doc, const int32_t* pause_after, const ev_stitch_config* cfg, int64_t* pos, int32_t* fl,
                   int32_t* fr, int64_t* doc_lens) {
    const int D = stitch_check(nullptr, "ev_stitch_plan", S, seg_doc, pause_after, cfg);
    if (D < 0) return -1;
    if (!n || !pos || !fl || !fr || !doc_lens) return fail(nullptr, "ev_stitch_plan: bad argument");
    for (int s = 0; s < S; ++s)
        if (n[s] < 0 || n[s] > EV_STITCH_MAX_DOC) return fail(nullptr, "ev_stitch_plan: n[%d] = %lld outside [0, EV_STITCH_MAX_DOC]", s, (long long)n[s]);
    const int64_t F = cfg->fade;
    for (int s = 0; s < S; ++s) {
        if (s == 0 || seg_doc[s] != seg_doc[s - 1]) { pos[s] = cfg->lead; fl[s] = (int32_t)std::min(F, n[s] / 2); }
        if (s == S - 1 || seg_doc[s + 1] != seg_doc[s]) {
            fr[s] = (int32_t)std::min(F, n[s] / 2);
            const int64_t len = pos[s] + n[s] + cfg->tail;
            if (len > EV_STITCH_MAX_DOC)
                return fail(nullptr, "ev_stitch_plan: document %d has %lld samples, more than EV_STITCH_MAX_DOC = %d", seg_doc[s], (long long)len, EV_STITCH_MAX_DOC);
            doc_lens[seg_doc[s]] = len;
            continue;
        }
        int64_t ov = 0;
        if (pause_after[s] < 0 && n[s] > 0 && n[s + 1] > 0) ov = std::min(std::min(-(int64_t)pause_after[s], F), std::min(n[s] / 2, n[s + 1] / 2));
        const int64_t gap = ov > 0 ? 0 : std::max((int64_t)pause_after[s], (int64_t)0);
        pos[s + 1] = pos[s] + n[s] + gap - ov;
        fr[s] = (int32_t)(ov > 0 ? ov : std::min(F, n[s] / 2));
        fl[s + 1] = (int32_t)(ov > 0 ? ov : std::min(F, n[s + 1] / 2));
    }
    return D;
}

// the planned segments -> the mix kernel's tables and the documents' offsets (D + 1); returns the packed length
static int64_t stitch_tables(int S, int D, const int64_t* src, const int64_t* n, const int32_t* seg_doc, const int64_t* pos, const int32_t* fl, const int32_t* fr,
                             const int64_t* doc_lens, std::vector<StitchMixSeg>& ms, std::vector<StitchDoc>& docs, std::vector<StitchTile>& tiles, int64_t* offs) {
    ms.resize((size_t)S); docs.assign((size_t)D, StitchDoc{0, 0, 0, 0}); tiles.clear();
    for (int s = 0; s < S; ++s) {
        ms[(size_t)s] = StitchMixSeg{src[s], pos[s], (int32_t)n[s], fl[s], fr[s], 0};
        StitchDoc& d = docs[(size_t)seg_doc[s]];
        if (d.nseg == 0) d.seg0 = s;
        d.nseg++;
    }
    int64_t o = 0;
    for (int d = 0; d < D; ++d) {
        docs[(size_t)d].out_off = o; docs[(size_t)d].len = doc_lens[d];
        offs[d] = o;
        for (int64_t t = 0; t * ST_TILE < doc_lens[d]; ++t) tiles.push_back(StitchTile{d, (int32_t)t});
        o += doc_lens[d];
    }
    offs[D] = o;
    return o;
}

int ev_stitch(ev_handle* h, int S, const float* wav, const int64_t* seg_offsets, const int64_t* seg_lens, const int32_t* seg_doc, const int32_t* pause_after,
              const ev_stitch_config* cfg, uint32_t flags, ev_stitch_result* out) {
    if (!h) return -1;
    if (!wav || !seg_offsets || !seg_lens || !seg_doc || !pause_after || !out) return fail(h, "ev_stitch: bad argument");
    if (out->struct_size != sizeof(ev_stitch_result))
        return fail(h, "ev_stitch: out->struct_size %u != sizeof(ev_stitch_result) %zu", out->struct_size, sizeof(ev_stitch_result));
    ev_stitch_config dflt;
    if (!cfg) { ev_default_stitch_config(&dflt); cfg = &dflt; }
    const int D = stitch_check(h, "ev_stitch", S, seg_doc, pause_after, cfg);
    if (D < 0) return -1;
    const ev_stitch_config c = *cfg;
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0, trim = c.trim_frac > 0.f || c.trim_abs > 0.f, i16 = c.want_i16 != 0;
    // the layout of the input, and each document's length before any cut: what the workspace is sized for and what EV_STITCH_MAX_DOC is judged on
    std::vector<StitchSeg> segs((size_t)S);
    std::vector<int64_t> bound((size_t)D, (int64_t)c.lead + c.tail);
    int64_t lo_off = INT64_MAX, hi_end = 0, n_part = 0, max_len = 0;
    for (int s = 0; s < S; ++s) {
        if (seg_offsets[s] < 0) return fail(h, "ev_stitch: seg_offsets[%d] = %lld < 0", s, (long long)seg_offsets[s]);
        if (seg_lens[s] < 1) return fail(h, "ev_stitch: seg_lens[%d] = %lld < 1", s, (long long)seg_lens[s]);
        int64_t& bd = bound[(size_t)seg_doc[s]];
        bd += std::min(seg_lens[s], (int64_t)EV_STITCH_MAX_DOC + 1);
        if (s + 1 < S && seg_doc[s + 1] == seg_doc[s]) bd += std::max(pause_after[s], 0);
        if (bd > EV_STITCH_MAX_DOC)
            return fail(h, "ev_stitch: document %d exceeds EV_STITCH_MAX_DOC = %d samples at segment %d (lead + tail + segments + pauses, before the cut)",
                        seg_doc[s], EV_STITCH_MAX_DOC, s);
        segs[(size_t)s] = StitchSeg{seg_offsets[s], seg_lens[s], n_part};
        n_part += (seg_lens[s] + ST_PEAK_CHUNK - 1) / ST_PEAK_CHUNK;
        lo_off = std::min(lo_off, seg_offsets[s]); hi_end = std::max(hi_end, seg_offsets[s] + seg_lens[s]); max_len = std::max(max_len, seg_lens[s]);
    }
    if (!dev_in) for (auto& sg : segs) sg.off -= lo_off;      // the host's samples lo_off .. hi_end are copied
    int64_t cap_out = 0, cap_tiles = 0;
    for (int d = 0; d < D; ++d) { cap_out += bound[(size_t)d]; cap_tiles += (bound[(size_t)d] + ST_TILE - 1) / ST_TILE; }
    HIPCHK(h, hipSetDevice(h->device));
    profiling_reset(h);
    float* d_wav = nullptr; StitchSeg* d_segs = nullptr; float *d_part = nullptr, *d_peak = nullptr; int64_t* d_cuts = nullptr;
    StitchMixSeg* d_ms = nullptr; StitchDoc* d_docs = nullptr; StitchTile* d_tiles = nullptr; float* d_out = nullptr; int16_t* d_i16 = nullptr;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 7, pass == 0};
        if (pass == 1 && arena_reserve(h, 7, need)) return -1;
        d_wav = dev_in ? nullptr : ap.arr<float>((size_t)(hi_end - lo_off));
        if (trim) { d_segs = ap.arr<StitchSeg>(S); d_part = ap.arr<float>((size_t)n_part); d_peak = ap.arr<float>(S); d_cuts = ap.arr<int64_t>(2 * (size_t)S); }
        d_ms = ap.arr<StitchMixSeg>(S); d_docs = ap.arr<StitchDoc>(D); d_tiles = ap.arr<StitchTile>((size_t)cap_tiles);
        d_out = ap.arr<float>((size_t)cap_out);
        if (i16) d_i16 = ap.arr<int16_t>((size_t)cap_out);
        need = ap.off;
    }
    if (!h->st_tab) HIPCHK(h, hipMalloc((void**)&h->st_tab, (size_t)EV_STITCH_MAX_FADE * sizeof(float)));
    h->st_tab_host.resize((size_t)c.fade);
    (void)ev_stitch_ramp(c.fade, h->st_tab_host.data());
    h->st_F = c.fade;
    if (c.fade > 0) HIPCHK(h, hipMemcpyAsync(h->st_tab, h->st_tab_host.data(), (size_t)c.fade * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (!dev_in) HIPCHK(h, hipMemcpyAsync(d_wav, wav + lo_off, (size_t)(hi_end - lo_off) * sizeof(float), hipMemcpyHostToDevice, h->stream));
    const float* x = dev_in ? wav : d_wav;
    std::vector<int64_t> a((size_t)S, 0), b((size_t)S), n((size_t)S), src((size_t)S);
    std::vector<float> peak((size_t)S, 0.f);
    for (int s = 0; s < S; ++s) b[(size_t)s] = seg_lens[s];
    region_begin(h, "total");
    if (trim) {
        HIPCHK(h, hipMemcpyAsync(d_segs, segs.data(), (size_t)S * sizeof(StitchSeg), hipMemcpyHostToDevice, h->stream));
        {
            KScope ks(h, "stitch_peak", 0.0, (double)(hi_end - lo_off) * 4.0);
            launch_stitch_peak(x, d_segs, S, max_len, d_part, h->stream);
        }
        HIPCHK(h, hipGetLastError());
        {
            KScope ks(h, "stitch_edges", 0.0, (double)n_part * 4.0);
            launch_stitch_edges(x, d_segs, S, d_part, c.trim_frac, c.trim_abs, d_peak, d_cuts, h->stream);
        }
        HIPCHK(h, hipGetLastError());
        std::vector<int64_t> cuts(2 * (size_t)S);
        HIPCHK(h, hipMemcpyAsync(cuts.data(), d_cuts, cuts.size() * 8, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipMemcpyAsync(peak.data(), d_peak, (size_t)S * 4, hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));
        for (int s = 0; s < S; ++s) {
            const int64_t first = cuts[2 * (size_t)s], last = cuts[2 * (size_t)s + 1];
            a[(size_t)s] = first < 0 ? 0 : std::max((int64_t)0, first - c.keep);
            b[(size_t)s] = first < 0 ? 0 : std::min(seg_lens[s], last + 1 + c.keep);
        }
    }
    for (int s = 0; s < S; ++s) { n[(size_t)s] = b[(size_t)s] - a[(size_t)s]; src[(size_t)s] = segs[(size_t)s].off + a[(size_t)s]; }
    std::vector<int64_t> pos((size_t)S), doc_lens((size_t)D), offs((size_t)D + 1);
    std::vector<int32_t> fl((size_t)S), fr((size_t)S);
    if (ev_stitch_plan(S, n.data(), seg_doc, pause_after, &c, pos.data(), fl.data(), fr.data(), doc_lens.data()) != D)
        return fail(h, "ev_stitch: %s", ev_last_error(nullptr));
    std::vector<StitchMixSeg> ms; std::vector<StitchDoc> docs; std::vector<StitchTile> tiles;
    const int64_t total = stitch_tables(S, D, src.data(), n.data(), seg_doc, pos.data(), fl.data(), fr.data(), doc_lens.data(), ms, docs, tiles, offs.data());
    if (total > cap_out || (int64_t)tiles.size() > cap_tiles) return fail(h, "ev_stitch: the plan outgrew its workspace");      // the cut only shortens
    HIPCHK(h, hipMemcpyAsync(d_ms, ms.data(), (size_t)S * sizeof(StitchMixSeg), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_docs, docs.data(), (size_t)D * sizeof(StitchDoc), hipMemcpyHostToDevice, h->stream));
    if (!tiles.empty()) HIPCHK(h, hipMemcpyAsync(d_tiles, tiles.data(), tiles.size() * sizeof(StitchTile), hipMemcpyHostToDevice, h->stream));
    {
        KScope ks(h, "stitch_mix", 0.0, (double)total * (i16 ? 10.0 : 8.0));
        if (launch_stitch_mix(x, d_ms, d_docs, d_tiles, (int64_t)tiles.size(), h->st_tab, c.fade, d_out, i16 ? d_i16 : nullptr, h->stream))
            return fail(h, "ev_stitch: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));
    profiling_collect(h);
    h->st_doc_lens = doc_lens; h->st_doc_offs = offs; h->st_pos = pos; h->st_start = a; h->st_end = b; h->st_peak = peak;
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz; out->batch_docs = D; out->batch_segs = S; out->total_samples = total; out->wav = d_out; out->wav_i16 = i16 ? d_i16 : nullptr;
    out->doc_lens = h->st_doc_lens.data(); out->doc_offsets = h->st_doc_offs.data(); out->seg_pos = h->st_pos.data();
    out->seg_start = h->st_start.data(); out->seg_end = h->st_end.data(); out->seg_peak = h->st_peak.data();
    return 0;
}

// ------------------------------------------------------------------- signal comparison (include/evhip.h: ev_compare)
static_assert(EV_COMPARE_CHUNK == CMP_CHUNK, "include/evhip.h states the chunk of ev_compare.hip");
int ev_compare(ev_handle* h, int B, const float* a, const float* b, const int64_t* lens, uint32_t flags, ev_compare_result* out) {
    if (!h) return -1;
    if (!a) return fail(h, "ev_compare: a is NULL");
    if (!b) return fail(h, "ev_compare: b is NULL");
    if (!lens) return fail(h, "ev_compare: lens is NULL");
    if (!out) return fail(h, "ev_compare: out is NULL");
    if (out->struct_size != sizeof(ev_compare_result))
        return fail(h, "ev_compare: out->struct_size %u != sizeof(ev_compare_result) %zu", out->struct_size, sizeof(ev_compare_result));
    if (B < 1 || B > 65535) return fail(h, "ev_compare: B = %d outside [1, 65535]", B);
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0;
    std::vector<int64_t> coffs((size_t)B + 1, 0);
    int64_t total = 0;
    for (int s = 0; s < B; ++s) {      // the chunk table's size is judged before it is built
        if (lens[s] < 1) return fail(h, "ev_compare: lens[%d] = %lld < 1", s, (long long)lens[s]);
        if (lens[s] > (int64_t)INT_MAX * CMP_CHUNK || coffs[(size_t)s] + (lens[s] + CMP_CHUNK - 1) / CMP_CHUNK > INT_MAX)
            return fail(h, "ev_compare: lens[%d] = %lld: more than %d chunks of %d elements in one call", s, (long long)lens[s], INT_MAX, CMP_CHUNK);
        coffs[(size_t)s + 1] = coffs[(size_t)s] + (lens[s] + CMP_CHUNK - 1) / CMP_CHUNK;
        total += lens[s];
    }
    const int64_t NC = coffs[(size_t)B];
    std::vector<CompareChunk> chunks;
    chunks.reserve((size_t)NC);
    for (int64_t s = 0, off = 0; s < B; off += lens[s], ++s)
        for (int64_t i = 0; i < lens[s]; i += CMP_CHUNK) chunks.push_back(CompareChunk{off + i, (int32_t)std::min<int64_t>(CMP_CHUNK, lens[s] - i), 0});
    HIPCHK(h, hipSetDevice(h->device));
    profiling_reset(h);
    float *d_a = nullptr, *d_b = nullptr; CompareChunk* d_chunks = nullptr; int64_t* d_coffs = nullptr; double *d_sums = nullptr, *d_maxd = nullptr;
    int32_t *d_argd = nullptr, *d_nonf = nullptr; float* d_peak = nullptr; CompareSeg* d_seg = nullptr;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 8, pass == 0};
        if (pass == 1 && arena_reserve(h, 8, need)) return -1;
        if (!dev_in) { d_a = ap.arr<float>((size_t)total); d_b = ap.arr<float>((size_t)total); }
        d_chunks = ap.arr<CompareChunk>((size_t)NC); d_coffs = ap.arr<int64_t>((size_t)B + 1);
        d_sums = ap.arr<double>(4 * (size_t)NC); d_maxd = ap.arr<double>((size_t)NC);
        d_argd = ap.arr<int32_t>((size_t)NC); d_nonf = ap.arr<int32_t>((size_t)NC); d_peak = ap.arr<float>((size_t)NC);
        d_seg = ap.arr<CompareSeg>((size_t)B);
        need = ap.off;
    }
    if (!dev_in) {
        HIPCHK(h, hipMemcpyAsync(d_a, a, (size_t)total * sizeof(float), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_b, b, (size_t)total * sizeof(float), hipMemcpyHostToDevice, h->stream));
    }
    HIPCHK(h, hipMemcpyAsync(d_chunks, chunks.data(), (size_t)NC * sizeof(CompareChunk), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_coffs, coffs.data(), ((size_t)B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    region_begin(h, "total");
    {
        KScope ks(h, "compare_chunks", 8.0 * (double)total, 8.0 * (double)total + 64.0 * (double)NC);
        if (launch_compare_chunks(dev_in ? a : d_a, dev_in ? b : d_b, d_chunks, NC, d_sums, d_maxd, d_argd, d_peak, d_nonf, h->stream))
            return fail(h, "ev_compare: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {
        KScope ks(h, "compare_finish", 4.0 * (double)NC, 52.0 * (double)NC + (double)B * sizeof(CompareSeg));
        launch_compare_finish(B, d_coffs, d_sums, NC, d_maxd, d_argd, d_peak, d_nonf, d_seg, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    region_end(h, "total");
    std::vector<CompareSeg> seg((size_t)B);
    std::vector<double> cd2((size_t)NC), cy2((size_t)NC);
    HIPCHK(h, hipMemcpyAsync(seg.data(), d_seg, (size_t)B * sizeof(CompareSeg), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(cd2.data(), d_sums + NC, (size_t)NC * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(cy2.data(), d_sums + 3 * NC, (size_t)NC * sizeof(double), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    profiling_collect(h);
    // from here on nothing fails: the previous result is replaced
    const size_t nb = (size_t)B;
    h->cmp_d.resize(nb); h->cmp_d2.resize(nb); h->cmp_y.resize(nb); h->cmp_y2.resize(nb); h->cmp_rel.resize(nb); h->cmp_rel_ac.resize(nb);
    h->cmp_max_d.resize(nb); h->cmp_peak_y.resize(nb); h->cmp_arg.resize(nb); h->cmp_nonf.resize(nb);
    for (size_t s = 0; s < nb; ++s) {
        const CompareSeg& g = seg[s];
        const double n = (double)lens[s], num = sqrt(g.sum[1]);
        const double var = g.sum[3] - (g.sum[2] * g.sum[2]) / n;      // the quotient sits between the product and the difference: nothing to fuse
        h->cmp_d[s] = g.sum[0]; h->cmp_d2[s] = g.sum[1]; h->cmp_y[s] = g.sum[2]; h->cmp_y2[s] = g.sum[3];
        h->cmp_rel[s] = num / sqrt(std::max(g.sum[3], EV_COMPARE_FLOOR));
        h->cmp_rel_ac[s] = num / sqrt(std::max(var, EV_COMPARE_FLOOR));
        h->cmp_max_d[s] = (float)g.max_d; h->cmp_peak_y[s] = g.peak_y; h->cmp_arg[s] = g.arg; h->cmp_nonf[s] = g.nonfinite;
    }
    h->cmp_chunk_d2.swap(cd2); h->cmp_chunk_y2.swap(cy2); h->cmp_chunk_offs.swap(coffs);
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz; out->batch = B; out->total = total;
    out->sum_d = h->cmp_d.data(); out->sum_d2 = h->cmp_d2.data(); out->sum_y = h->cmp_y.data(); out->sum_y2 = h->cmp_y2.data();
    out->rel_l2 = h->cmp_rel.data(); out->rel_l2_ac = h->cmp_rel_ac.data(); out->max_abs_d = h->cmp_max_d.data(); out->argmax_d = h->cmp_arg.data();
    out->peak_y = h->cmp_peak_y.data(); out->nonfinite = h->cmp_nonf.data();
    out->chunk_d2 = h->cmp_chunk_d2.data(); out->chunk_y2 = h->cmp_chunk_y2.data(); out->chunk_offsets = h->cmp_chunk_offs.data();
    return 0;
}

// ------------------------------------------------------------------- FLAC encoding (include/evhip.h: ev_flac)
void ev_default_flac_config(ev_flac_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c; c->sample_rate = 16000; c->block_size = 4096; c->max_fixed_order = 4; c->max_partition_order = 5; c->convert = EV_FLAC_WRAP;
}

static int flac_block_code(int block_size) {      // the frame header's code of N, or -1
    for (int i = 0; i < 5; ++i) if (block_size == 256 << i) return 8 + i;
    return -1;
}
static int flac_rate_code(int sample_rate) {
    static const int rates[7] = {8000, 16000, 22050, 24000, 32000, 44100, 48000};
    for (int i = 0; i < 7; ++i) if (sample_rate == rates[i]) return 4 + i;
    return -1;
}

int64_t ev_flac_bound(int64_t n, int block_size) {
    if (n < 1 || n > EV_FLAC_MAX_SAMPLES || flac_block_code(block_size) < 0) return -1;
    const int64_t full = n / block_size, rest = n % block_size;
    return FLAC_STREAM_HEADER + full * (2 * (int64_t)block_size + 15) + (rest ? 2 * rest + 15 : 0);
}

int ev_flac(ev_handle* h, int B, const void* pcm, int pcm_is_i16, const int64_t* lens, const ev_flac_config* cfg, uint32_t flags, ev_flac_result* out) {
    if (!h) return -1;
    if (!pcm) return fail(h, "ev_flac: pcm is NULL");
    if (!lens) return fail(h, "ev_flac: lens is NULL");
    if (!out) return fail(h, "ev_flac: out is NULL");
    if (out->struct_size != sizeof(ev_flac_result))
        return fail(h, "ev_flac: out->struct_size %u != sizeof(ev_flac_result) %zu", out->struct_size, sizeof(ev_flac_result));
    ev_flac_config dflt;
    if (!cfg) { ev_default_flac_config(&dflt); cfg = &dflt; }
    if (cfg->struct_size != sizeof(ev_flac_config))
        return fail(h, "ev_flac: cfg->struct_size %u != sizeof(ev_flac_config) %zu", cfg->struct_size, sizeof(ev_flac_config));
    const ev_flac_config c = *cfg;
    const int sr_code = flac_rate_code(c.sample_rate), bs_code = flac_block_code(c.block_size);
    if (sr_code < 0) return fail(h, "ev_flac: sample_rate = %d is not one of 8000, 16000, 22050, 24000, 32000, 44100, 48000", c.sample_rate);
    if (bs_code < 0) return fail(h, "ev_flac: block_size = %d is not one of 256, 512, 1024, 2048, 4096", c.block_size);
    if (c.max_fixed_order < 0 || c.max_fixed_order > 4) return fail(h, "ev_flac: max_fixed_order = %d outside [0, 4]", c.max_fixed_order);
    if (c.max_partition_order < 0 || c.max_partition_order > 6) return fail(h, "ev_flac: max_partition_order = %d outside [0, 6]", c.max_partition_order);
    if (c.convert != EV_FLAC_WRAP && c.convert != EV_FLAC_CLAMP) return fail(h, "ev_flac: convert = %d is neither EV_FLAC_WRAP nor EV_FLAC_CLAMP", c.convert);
    if (B < 1 || B > 65535) return fail(h, "ev_flac: B = %d outside [1, 65535]", B);
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0, i16 = pcm_is_i16 != 0;
    const int N = c.block_size, stride = 2 * N + 24;
    int64_t total = 0, NF = 0, cap = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) return fail(h, "ev_flac: lens[%d] = %lld < 1", b, (long long)lens[b]);
        if (lens[b] > EV_FLAC_MAX_SAMPLES) return fail(h, "ev_flac: lens[%d] = %lld > EV_FLAC_MAX_SAMPLES = %d", b, (long long)lens[b], EV_FLAC_MAX_SAMPLES);
        total += lens[b]; NF += (lens[b] + N - 1) / N; cap += ev_flac_bound(lens[b], N);
        if (NF > INT_MAX) return fail(h, "ev_flac: lens[%d] = %lld: more than %d frames in one call", b, (long long)lens[b], INT_MAX);
    }
    std::vector<FlacFrame> frames;
    frames.reserve((size_t)NF);
    std::vector<int64_t> sframes((size_t)B);
    for (int64_t b = 0, off = 0; b < B; off += lens[b], ++b) {
        sframes[(size_t)b] = (lens[b] + N - 1) / N;
        for (int64_t i = 0; i < lens[b]; i += N) frames.push_back(FlacFrame{off + i, (int32_t)std::min<int64_t>(N, lens[b] - i), (int32_t)(i / N), (int32_t)b, 0});
    }
    HIPCHK(h, hipSetDevice(h->device));
    profiling_reset(h);
    const size_t es = i16 ? sizeof(int16_t) : sizeof(float);
    char* d_pcm = nullptr; FlacFrame* d_frames = nullptr; int32_t* d_sizes = nullptr; uint32_t* d_desc = nullptr; uint8_t *d_scratch = nullptr, *d_hdr = nullptr, *d_bytes = nullptr;
    int64_t* d_foffs = nullptr;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 9, pass == 0};
        if (pass == 1 && arena_reserve(h, 9, need)) return -1;
        if (!dev_in) d_pcm = ap.arr<char>((size_t)total * es);
        d_frames = ap.arr<FlacFrame>((size_t)NF); d_sizes = ap.arr<int32_t>((size_t)NF); d_desc = ap.arr<uint32_t>((size_t)NF);
        d_foffs = ap.arr<int64_t>((size_t)NF); d_hdr = ap.arr<uint8_t>((size_t)B * FLAC_HEADER_STRIDE);
        d_scratch = ap.arr<uint8_t>((size_t)NF * (size_t)stride + 16); d_bytes = ap.arr<uint8_t>((size_t)cap);
        need = ap.off;
    }
    if (!dev_in) HIPCHK(h, hipMemcpyAsync(d_pcm, pcm, (size_t)total * es, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_frames, frames.data(), (size_t)NF * sizeof(FlacFrame), hipMemcpyHostToDevice, h->stream));
    FlacParams fp{};
    fp.pcm = dev_in ? pcm : d_pcm; fp.pcm_is_i16 = i16; fp.convert = c.convert; fp.block_size = N; fp.bs_code = bs_code; fp.sr_code = sr_code;
    fp.max_fixed_order = c.max_fixed_order; fp.max_partition_order = c.max_partition_order; fp.frames = d_frames; fp.scratch = d_scratch; fp.stride = stride;
    fp.sizes = d_sizes; fp.desc = d_desc;
    region_begin(h, "total");
    {
        KScope ks(h, "flac_encode", 0.0, (double)total * (double)es + (double)NF * (double)stride);
        if (launch_flac_encode(fp, NF, h->stream)) return fail(h, "ev_flac: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    std::vector<int32_t> sizes((size_t)NF); std::vector<uint32_t> desc((size_t)NF);
    HIPCHK(h, hipMemcpyAsync(sizes.data(), d_sizes, (size_t)NF * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(desc.data(), d_desc, (size_t)NF * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // the layout: per stream its header, then its frames; the header needs the stream's smallest and largest frame
    std::vector<int64_t> soffs((size_t)B + 1, 0), foffs((size_t)NF + 1, 0);
    std::vector<uint8_t> hdr((size_t)B * FLAC_HEADER_STRIDE, 0), kind((size_t)NF), porder((size_t)NF);
    int64_t pos = 0, f = 0;
    for (int b = 0; b < B; ++b) {
        soffs[(size_t)b] = pos;
        pos += FLAC_STREAM_HEADER;
        int32_t lo = INT_MAX, hi = 0;
        for (int64_t i = 0; i < sframes[(size_t)b]; ++i, ++f) {
            const int32_t sz = sizes[(size_t)f];
            if (sz < 1 || sz > 2 * N + 15) return fail(h, "ev_flac: frame %lld of segment %d reports %d bytes", (long long)i, b, sz);
            foffs[(size_t)f] = pos; pos += sz; lo = std::min(lo, sz); hi = std::max(hi, sz);
            kind[(size_t)f] = (uint8_t)(desc[(size_t)f] & 0xFFu); porder[(size_t)f] = (uint8_t)(desc[(size_t)f] >> 8 & 0xFFu);
        }
        uint8_t* p = hdr.data() + (size_t)b * FLAC_HEADER_STRIDE;
        const uint64_t n = (uint64_t)lens[b], v = (uint64_t)c.sample_rate << 44 | (uint64_t)15 << 36 | n;      // 20 + 3 + 5 + 36 bits
        memcpy(p, "fLaC", 4);
        p[4] = 0x80; p[5] = 0; p[6] = 0; p[7] = 0x22;
        p[8] = p[10] = (uint8_t)(N >> 8); p[9] = p[11] = (uint8_t)(N & 0xFF);
        p[12] = (uint8_t)(lo >> 16); p[13] = (uint8_t)(lo >> 8); p[14] = (uint8_t)lo;
        p[15] = (uint8_t)(hi >> 16); p[16] = (uint8_t)(hi >> 8); p[17] = (uint8_t)hi;
        for (int i = 0; i < 8; ++i) p[18 + i] = (uint8_t)(v >> (56 - 8 * i));      // p[26 .. 42): the MD5, zero
    }
    soffs[(size_t)B] = pos; foffs[(size_t)NF] = pos;
    if (pos > cap) return fail(h, "ev_flac: the streams outgrew their bound");
    HIPCHK(h, hipMemcpyAsync(d_foffs, foffs.data(), (size_t)NF * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_hdr, hdr.data(), hdr.size(), hipMemcpyHostToDevice, h->stream));
    {
        KScope ks(h, "flac_gather", 0.0, 2.0 * (double)pos);
        launch_flac_gather(d_scratch, stride, d_frames, NF, d_sizes, d_foffs, d_hdr, d_bytes, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));      // the uploads above read host vectors that end with this call
    profiling_collect(h);
    h->fl_stream_offs.swap(soffs); h->fl_stream_frames.swap(sframes); h->fl_frame_offs.swap(foffs); h->fl_kind.swap(kind); h->fl_porder.swap(porder);
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz; out->batch = B; out->total_bytes = pos; out->total_frames = NF; out->bytes = d_bytes;
    out->stream_offsets = h->fl_stream_offs.data(); out->stream_frames = h->fl_stream_frames.data(); out->frame_offsets = h->fl_frame_offs.data();
    out->frame_kind = h->fl_kind.data(); out->frame_porder = h->fl_porder.data();
    return 0;
}

// ------------------------------------------------------------------- loudness normalisation (include/evhip.h: ev_loudness)
static_assert(EV_LOUDNESS_TILE == LOUD_TILE, "include/evhip.h states the tile of ev_loudness.hip");
void ev_default_loudness_config(ev_loudness_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c; c->sample_rate = 16000; c->target_lufs = NAN; c->max_gain_db = 20.0; c->peak_ceiling = (float)pow(10.0, -1.0 / 20.0); c->want_i16 = 0;
}

int ev_loudness_design(int sample_rate, double coef[10]) {
    if (flac_rate_code(sample_rate) < 0 || !coef) return -1;
    const double pi = 3.14159265358979323846, fs = (double)sample_rate;
    {
        const double f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196;
        const double K = tan(pi * f0 / fs), Vh = pow(10.0, G / 20.0), Vb = pow(Vh, 0.4996667741545416), a0 = 1.0 + K / Q + K * K;
        coef[0] = (Vh + Vb * K / Q + K * K) / a0; coef[1] = 2.0 * (K * K - Vh) / a0; coef[2] = (Vh - Vb * K / Q + K * K) / a0;
        coef[3] = 2.0 * (K * K - 1.0) / a0; coef[4] = (1.0 - K / Q + K * K) / a0;
    }
    {
        const double f0 = 38.13547087602444, Q = 0.5003270373238773;
        const double K = tan(pi * f0 / fs), a0 = 1.0 + K / Q + K * K;
        coef[5] = 1.0; coef[6] = -2.0; coef[7] = 1.0;
        coef[8] = 2.0 * (K * K - 1.0) / a0; coef[9] = (1.0 - K / Q + K * K) / a0;
    }
    return 0;
}

// the kernels' constants: the coefficients and the powers A^(LOUD_RUN 2^d), d = 0 .. 8, of the cascade's transition matrix (transposed direct form II,
// states: the shelf's two, then the high-pass's two), squared up in long double and rounded once
static void loudness_coef(const double coef[10], LoudCoef* lc) {
    for (int q = 0; q < 2; ++q) {
        for (int i = 0; i < 3; ++i) lc->b[q][i] = coef[5 * q + i];
        for (int i = 0; i < 2; ++i) lc->a[q][i] = coef[5 * q + 3 + i];
    }
    const long double a1 = coef[3], a2 = coef[4], c0 = coef[5], c1 = coef[6], c2 = coef[7], d1 = coef[8], d2 = coef[9];
    long double M[16] = {-a1, 1, 0, 0, -a2, 0, 0, 0, c1 - d1 * c0, 0, -d1, 1, c2 - d2 * c0, 0, -d2, 0}, T[16];
    auto square = [&]() {
        for (int i = 0; i < 4; ++i) for (int j = 0; j < 4; ++j) {
            long double acc = 0;
            for (int k = 0; k < 4; ++k) acc += M[i * 4 + k] * M[k * 4 + j];
            T[i * 4 + j] = acc;
        }
        memcpy(M, T, sizeof M);
    };
    int run = 1;
    while (run < LOUD_RUN) { square(); run *= 2; }
    for (int d = 0; d < 9; ++d) {
        for (int i = 0; i < 16; ++i) lc->P[d][i] = (double)M[i];
        square();
    }
}

static double loudness_lufs(double z) { return -0.691 + 10.0 * log10(z); }      // z = 0: -inf

int ev_loudness(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const ev_loudness_config* cfg, uint32_t flags,
                ev_loudness_result* out) {
    if (!h) return -1;
    if (!wav) return fail(h, "ev_loudness: wav is NULL");
    if (!lens) return fail(h, "ev_loudness: lens is NULL");
    if (!out) return fail(h, "ev_loudness: out is NULL");
    if (out->struct_size != sizeof(ev_loudness_result))
        return fail(h, "ev_loudness: out->struct_size %u != sizeof(ev_loudness_result) %zu", out->struct_size, sizeof(ev_loudness_result));
    ev_loudness_config dflt;
    if (!cfg) { ev_default_loudness_config(&dflt); cfg = &dflt; }
    if (cfg->struct_size != sizeof(ev_loudness_config))
        return fail(h, "ev_loudness: cfg->struct_size %u != sizeof(ev_loudness_config) %zu", cfg->struct_size, sizeof(ev_loudness_config));
    const ev_loudness_config c = *cfg;
    double coef[10];
    if (ev_loudness_design(c.sample_rate, coef))
        return fail(h, "ev_loudness: sample_rate = %d is not one of 8000, 16000, 22050, 24000, 32000, 44100, 48000", c.sample_rate);
    const bool measure_only = std::isnan(c.target_lufs);
    if (!measure_only && !(c.target_lufs >= -70.0 && c.target_lufs <= 0.0))
        return fail(h, "ev_loudness: target_lufs = %g is neither NaN (measure only) nor in [-70, 0]", c.target_lufs);
    if (!(std::isfinite(c.max_gain_db) && c.max_gain_db >= 0.0)) return fail(h, "ev_loudness: max_gain_db = %g is not finite and >= 0", c.max_gain_db);
    if (!(c.peak_ceiling > 0.f && c.peak_ceiling <= 1.f)) return fail(h, "ev_loudness: peak_ceiling = %g outside (0, 1]", (double)c.peak_ceiling);
    if (B < 1 || B > 65535) return fail(h, "ev_loudness: B = %d outside [1, 65535]", B);
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0, in16 = wav_is_i16 != 0, i16 = c.want_i16 != 0 && !measure_only;
    const int64_t step = c.sample_rate / 10, block = 4 * step;
    int64_t total = 0, NT = 0, NB = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1) return fail(h, "ev_loudness: lens[%d] = %lld < 1", b, (long long)lens[b]);
        if (lens[b] > EV_LOUDNESS_MAX_SAMPLES)
            return fail(h, "ev_loudness: lens[%d] = %lld > EV_LOUDNESS_MAX_SAMPLES = %d", b, (long long)lens[b], EV_LOUDNESS_MAX_SAMPLES);
        total += lens[b]; NT += (lens[b] + LOUD_TILE - 1) / LOUD_TILE; NB += lens[b] >= block ? (lens[b] - block) / step + 1 : 1;
        if (NT > INT_MAX || (total + 1023) / 1024 > INT_MAX)
            return fail(h, "ev_loudness: lens[%d] = %lld: more than %d tiles in one call", b, (long long)lens[b], INT_MAX);
    }
    std::vector<LoudTile> tiles;
    tiles.reserve((size_t)NT);
    std::vector<LoudSeg> segs((size_t)B);
    std::vector<int64_t> offs((size_t)B + 1, 0);
    for (int64_t b = 0, off = 0; b < B; off += lens[b], ++b) {
        segs[(size_t)b] = LoudSeg{(int64_t)tiles.size(), (lens[b] + LOUD_TILE - 1) / LOUD_TILE};
        offs[(size_t)b + 1] = off + lens[b];
        for (int64_t i = 0; i < lens[b]; i += LOUD_TILE) tiles.push_back(LoudTile{off + i, i, (int32_t)std::min<int64_t>(LOUD_TILE, lens[b] - i), (int32_t)b});
    }
    LoudCoef lc;
    loudness_coef(coef, &lc);
    HIPCHK(h, hipSetDevice(h->device));
    profiling_reset(h);
    const size_t es = in16 ? sizeof(int16_t) : sizeof(float);
    char* d_in = nullptr; LoudTile* d_tiles = nullptr; LoudSeg* d_segs = nullptr; LoudCoef* d_coef = nullptr; double *d_ends = nullptr, *d_init = nullptr;
    LoudTileOut* d_outs = nullptr; int64_t* d_offs = nullptr; float *d_gain = nullptr, *d_wav = nullptr; int16_t* d_i16 = nullptr;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 10, pass == 0};
        if (pass == 1 && arena_reserve(h, 10, need)) return -1;
        if (!dev_in) d_in = ap.arr<char>((size_t)total * es);
        d_tiles = ap.arr<LoudTile>((size_t)NT); d_segs = ap.arr<LoudSeg>((size_t)B); d_coef = ap.arr<LoudCoef>(1);
        d_ends = ap.arr<double>(4 * (size_t)NT); d_init = ap.arr<double>(4 * (size_t)NT); d_outs = ap.arr<LoudTileOut>((size_t)NT);
        d_offs = ap.arr<int64_t>((size_t)B + 1); d_gain = ap.arr<float>((size_t)B);
        if (!measure_only) d_wav = ap.arr<float>((size_t)total);
        if (i16) d_i16 = ap.arr<int16_t>((size_t)total);
        need = ap.off;
    }
    if (!dev_in) HIPCHK(h, hipMemcpyAsync(d_in, wav, (size_t)total * es, hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_tiles, tiles.data(), (size_t)NT * sizeof(LoudTile), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_segs, segs.data(), (size_t)B * sizeof(LoudSeg), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_coef, &lc, sizeof lc, hipMemcpyHostToDevice, h->stream));
    const void* x = dev_in ? wav : (const void*)d_in;
    region_begin(h, "total");
    {
        KScope ks(h, "loudness_measure", 60.0 * (double)total, 2.0 * (double)total * (double)es + (double)NT * (64.0 + sizeof(LoudTileOut)));
        if (launch_loudness_measure(x, in16, d_tiles, NT, d_segs, B, d_coef, (int)step, d_ends, d_init, d_outs, h->stream))
            return fail(h, "ev_loudness: the kernels do not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    std::vector<LoudTileOut> touts((size_t)NT);
    HIPCHK(h, hipMemcpyAsync(touts.data(), d_outs, (size_t)NT * sizeof(LoudTileOut), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    // the host half: step sums from the tiles' in ascending tile order, blocks, the two gates, the gain
    std::vector<double> loud((size_t)B), rel((size_t)B), ms; std::vector<float> gain((size_t)B), peak((size_t)B); std::vector<uint8_t> fl((size_t)B), state;
    std::vector<int64_t> nonf((size_t)B), boffs((size_t)B + 1, 0);
    ms.reserve((size_t)NB); state.reserve((size_t)NB);
    std::vector<double> S;
    const double ninf = -std::numeric_limits<double>::infinity();
    for (int b = 0; b < B; ++b) {
        const int64_t n = lens[b], nbins = (n + step - 1) / step;
        S.assign((size_t)nbins, 0.0);
        float pk = 0.f; int64_t nf = 0;
        for (int64_t t = 0; t < segs[(size_t)b].ntiles; ++t) {
            const LoudTileOut& o = touts[(size_t)(segs[(size_t)b].tile0 + t)];
            const int64_t pos = t * LOUD_TILE, tb0 = pos / step, nsl = (std::min<int64_t>(pos + LOUD_TILE, n) - 1) / step - tb0 + 1;
            for (int64_t k = 0; k < nsl; ++k) S[(size_t)(tb0 + k)] += o.sum[k];
            pk = std::max(pk, o.peak); nf += o.nonfinite;
        }
        const size_t j0 = ms.size();
        if (n >= block) {
            const int64_t nblk = (n - block) / step + 1;
            for (int64_t j = 0; j < nblk; ++j) ms.push_back((((S[(size_t)j] + S[(size_t)j + 1]) + S[(size_t)j + 2]) + S[(size_t)j + 3]) / (double)block);
        } else {
            double acc = 0.0;
            for (int64_t m = 0; m < nbins; ++m) acc += S[(size_t)m];
            ms.push_back(acc / (double)n);
        }
        const size_t j1 = ms.size();
        state.resize(j1, 0);
        double acc = 0.0; int64_t cnt = 0;
        for (size_t j = j0; j < j1; ++j) if (loudness_lufs(ms[j]) > -70.0) { state[j] = 1; acc += ms[j]; ++cnt; }
        double L = ninf, gamma = ninf;
        if (cnt > 0) {
            gamma = loudness_lufs(acc / (double)cnt) - 10.0;
            acc = 0.0; cnt = 0;
            for (size_t j = j0; j < j1; ++j) if (state[j] == 1 && loudness_lufs(ms[j]) > gamma) { state[j] = 2; acc += ms[j]; ++cnt; }
            if (cnt > 0) L = loudness_lufs(acc / (double)cnt);
        }
        uint8_t f = L == ninf ? EV_LOUDNESS_UNDEFINED : 0;
        double g = 1.0;
        if (!measure_only) {
            if (L != ninf) g = pow(10.0, (c.target_lufs - L) / 20.0);
            const double gmax = pow(10.0, c.max_gain_db / 20.0);
            if (g > gmax) { g = gmax; f |= EV_LOUDNESS_BOOST_LIMITED; }
            if (pk > 0.f) {
                const double gpk = (double)c.peak_ceiling / (double)pk;
                if (g > gpk) { g = gpk; f |= EV_LOUDNESS_PEAK_LIMITED; }
            }
        }
        loud[(size_t)b] = L; rel[(size_t)b] = gamma; gain[(size_t)b] = (float)g; peak[(size_t)b] = pk; fl[(size_t)b] = f; nonf[(size_t)b] = nf;
        boffs[(size_t)b + 1] = (int64_t)j1;
    }
    if (!measure_only) {
        HIPCHK(h, hipMemcpyAsync(d_offs, offs.data(), ((size_t)B + 1) * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_gain, gain.data(), (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
        {
            KScope ks(h, "loudness_gain", (double)total, (double)total * ((double)es + (i16 ? 6.0 : 4.0)));
            if (launch_loudness_gain(x, in16, d_offs, B, d_gain, total, d_wav, i16 ? d_i16 : nullptr, h->stream))
                return fail(h, "ev_loudness: the kernels do not build this shape");
        }
        HIPCHK(h, hipGetLastError());
    }
    region_end(h, "total");
    HIPCHK(h, hipStreamSynchronize(h->stream));      // the uploads above read host vectors that end with this call
    profiling_collect(h);
    h->ld_loud.swap(loud); h->ld_rel.swap(rel); h->ld_ms.swap(ms); h->ld_gain.swap(gain); h->ld_peak.swap(peak); h->ld_flags.swap(fl); h->ld_state.swap(state);
    h->ld_nonf.swap(nonf); h->ld_boffs.swap(boffs);
    const uint32_t sz = out->struct_size;
    memset(out, 0, sizeof *out);
    out->struct_size = sz; out->batch = B; out->total = total; out->wav = measure_only ? nullptr : d_wav; out->wav_i16 = i16 ? d_i16 : nullptr;
    out->loudness = h->ld_loud.data(); out->rel_threshold = h->ld_rel.data(); out->gain = h->ld_gain.data(); out->peak = h->ld_peak.data();
    out->flags = h->ld_flags.data(); out->nonfinite = h->ld_nonf.data(); out->block_offsets = h->ld_boffs.data(); out->block_ms = h->ld_ms.data();
    out->block_state = h->ld_state.data();
    return 0;
}

// ------------------------------------------------------------------- SimBERT prompt / content encoder
void ev_default_bert_config(ev_bert_config* c) {
    memset(c, 0, sizeof *c);
    c->vocab_size = 13685; c->hidden = 768; c->layers = 12; c->heads = 12; c->intermediate = 3072; c->max_position = 512;
    c->type_vocab = 2; c->ln_eps = 1e-12f;
}

int ev_style_load_weights(ev_handle* h, const ev_bert_config* cfg, const void* blob, size_t nbytes) {
    if (!h || !cfg || !blob) return fail(h, "ev_style_load_weights: null argument");
    if (cfg->hidden % 128 || cfg->hidden > 1024 || cfg->heads <= 0 || cfg->hidden / cfg->heads != 64 || cfg->intermediate % 64 || cfg->layers <= 0)
        return fail(h, "ev_style_load_weights: only hidden %% 128 == 0 (<= 1024) with 64-wide heads is built (BERT-base: 768 / 12)");
    HIPCHK(h, hipSetDevice(h->device));
    if (h->sblob) { HIPCHK(h, hipStreamSynchronize(h->stream)); HIPCHK(h, hipFree(h->sblob)); h->sblob = nullptr; }
    h->style_loaded = false;
    HIPCHK(h, hipMalloc((void**)&h->sblob, nbytes));
    h->sbytes = nbytes;
    HIPCHK(h, hipMemcpy(h->sblob, blob, nbytes, hipMemcpyHostToDevice));
    if (parse_blob(h, (const char*)blob, nbytes, true)) return -1;
    const WeightEntry* we = W(h, "sb.emb.word");
    if (!we) return -1;
    if ((int)we->dims[0] != cfg->vocab_size || (int)we->dims[1] != cfg->hidden) return fail(h, "ev_style_load_weights: word embedding %llu x %llu does not match the config", (unsigned long long)we->dims[0], (unsigned long long)we->dims[1]);
    h->bcfg = *cfg;
    h->style_loaded = true;
    return 0;
}

// BertModel.forward -> pooler_output for B texts packed back to back (reference simbert.py:49-55 through
// inference_am_vocoder_joint.py:25-38, which tokenises one text per call: attention_mask all ones; here each text attends to its
// own tokens only, the same B = 1 semantics).  fp32-class arithmetic throughout (split-precision GEMMs, exact-fp32 MFMA
// attention): the pooled output conditions the duration predictor, whose integer output must stay bit-exact.
int ev_style_embed(ev_handle* h, int B, const int64_t* input_ids, const int64_t* token_type_ids, const int32_t* cu, uint32_t flags, float* out) {
    if (!h || !input_ids || !cu || !out || B <= 0) return fail(h, "ev_style_embed: bad argument");
    if (!h->style_loaded) return fail(h, "ev_style_embed: ev_style_load_weights first");
    if (cu[0] != 0) return fail(h, "ev_style_embed: cu_seqlens[0] must be 0");
    HIPCHK(h, hipSetDevice(h->device));
    const ev_bert_config& bc = h->bcfg;
    const int H = bc.hidden, I = bc.intermediate;
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0;
    const int NT = cu[B];
    std::vector<int32_t> off(B), len(B);
    int64_t rows = GAP; int max_len = 0;
    for (int b = 0; b < B; ++b) {
        const int n = cu[b + 1] - cu[b];
        if (n <= 0) return fail(h, "ev_style_embed: text %d has %d tokens", b, n);
        if (n > bc.max_position) return fail(h, "ev_style_embed: text %d has %d tokens > max_position_embeddings %d", b, n, bc.max_position);
        off[b] = (int32_t)rows; len[b] = n; rows += n + GAP; max_len = std::max(max_len, n);
    }
    if (!dev_in)
        for (int j = 0; j < NT; ++j)
            if (input_ids[j] < 0 || input_ids[j] >= bc.vocab_size) return fail(h, "ev_style_embed: token id %lld at position %d outside [0, %d)", (long long)input_ids[j], j, bc.vocab_size);
    const int Rt = (int)align_up((size_t)rows, ROW_ALIGN);
    Buf x, t, qkv, ctx, ffn; int32_t *d_seq, *d_pos, *d_off, *d_len, *d_cu; uint8_t* d_valid; int64_t *d_ids, *d_tt; float* d_out;
    size_t need = 0;
    for (int pass = 0; pass < 2; ++pass) {
        ArenaPlan ap{h, 2, pass == 0};
        if (pass == 1 && arena_reserve(h, 2, need)) return -1;
        d_seq = ap.arr<int32_t>(Rt); d_pos = ap.arr<int32_t>(Rt); d_valid = ap.arr<uint8_t>(Rt);
        d_off = ap.arr<int32_t>(B); d_len = ap.arr<int32_t>(B); d_cu = ap.arr<int32_t>(B + 1);
        d_ids = ap.arr<int64_t>(NT); d_tt = ap.arr<int64_t>(NT); d_out = ap.arr<float>((size_t)B * H);
        x = ap.rows(Rt, H, 4); t = ap.rows(Rt, H, 4); qkv = ap.rows(Rt, 3 * H, 4); ctx = ap.rows(Rt, H, 4); ffn = ap.rows(Rt, I, 4);
        need = ap.off;
    }
    if ((size_t)B > PIN_MAX_B) return fail(h, "ev_style_embed: at most %zu texts per call", PIN_MAX_B);
    if (pinned_reserve(h, PIN_BYTES)) return -1;
    {
        int32_t* poff = (int32_t*)h->pinned; int32_t* plen = poff + B; int32_t* pcu = plen + B;
        for (int b = 0; b < B; ++b) { poff[b] = off[b]; plen[b] = len[b]; }
        memcpy(pcu, cu, (size_t)(B + 1) * 4);
        HIPCHK(h, hipMemcpyAsync(d_off, poff, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_len, plen, (size_t)B * 4, hipMemcpyHostToDevice, h->stream));
        HIPCHK(h, hipMemcpyAsync(d_cu, pcu, (size_t)(B + 1) * 4, hipMemcpyHostToDevice, h->stream));
        launch_row_maps(d_off, d_len, B, d_seq, d_pos, d_valid, Rt, h->stream);
        const hipMemcpyKind kind = dev_in ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        HIPCHK(h, hipMemcpyAsync(d_ids, input_ids, (size_t)NT * 8, kind, h->stream));
        if (token_type_ids) HIPCHK(h, hipMemcpyAsync(d_tt, token_type_ids, (size_t)NT * 8, kind, h->stream));
    }
    WPTR(wword, float, "sb.emb.word"); WPTR(wpos, float, "sb.emb.pos"); WPTR(wtype, float, "sb.emb.type");
    WPTR(eg, float, "sb.emb.ln.g"); WPTR(eb, float, "sb.emb.ln.b");
    launch_bert_embed(d_ids, token_type_ids ? d_tt : nullptr, d_cu, d_seq, d_pos, wword, wpos, wtype, bc.vocab_size, bc.max_position, bc.type_vocab,
                      (float*)t.p, Rt, H, h->stream);
    LayerNormParams ln{};
    ln.ldx = H; ln.rows = Rt; ln.C = H; ln.eps = bc.ln_eps; ln.row_valid = d_valid; ln.ldo = H;
    ln.x = (const float*)t.p; ln.gamma = eg; ln.beta = eb; ln.out32 = (float*)x.p;
    launch_layernorm(ln, h->stream);
    auto bert_gemm = [&](const std::string& base, ConvGemmParams& p) -> int {
        const WeightEntry* hi = W(h, base + ".w16"); const WeightEntry* lo = W(h, base + ".w32l"); const WeightEntry* bias = W(h, base + ".b");
        if (!hi || !lo || !bias) return -1;
        p.dtype = DT_F32S; p.W = hi->ptr; p.W_lo = lo->ptr; p.bias = reinterpret_cast<const float*>(bias->ptr);
        p.M = Rt; p.row_valid = d_valid;
        return gemm(h, "style_gemm", p, (double)NT);
    };
    for (int i = 0; i < bc.layers; ++i) {
        const std::string lp = "sb." + std::to_string(i);
        WPTR(g1, float, lp + ".ln1.g"); WPTR(b1, float, lp + ".ln1.b"); WPTR(g2, float, lp + ".ln2.g"); WPTR(b2, float, lp + ".ln2.b");
        ConvGemmParams p = gemm_defaults();
        p.A = x.p; p.lda = H; p.N = 3 * H; p.K = H; p.out32 = (float*)qkv.p; p.ldo = 3 * H;
        if (bert_gemm(lp + ".qkv", p)) return -1;
        AttnParams ap{};
        ap.qkv = qkv.p; ap.dtype = DT_F32; ap.ld = 3 * H; ap.C = H; ap.heads = bc.heads; ap.seq_off = d_off; ap.seq_len = d_len; ap.B = B;
        ap.max_len = max_len; ap.out = ctx.p; ap.ldo = H;
        launch_attention(ap, h->stream);
        p = gemm_defaults();           // BertSelfOutput: LayerNorm(dense(ctx) + x)
        p.A = ctx.p; p.lda = H; p.N = H; p.K = H; p.res = x.p; p.res_dtype = DT_F32; p.ldres = H; p.out32 = (float*)t.p; p.ldo = H;
        if (bert_gemm(lp + ".out", p)) return -1;
        ln.x = (const float*)t.p; ln.gamma = g1; ln.beta = b1; ln.out32 = (float*)x.p;
        launch_layernorm(ln, h->stream);
        p = gemm_defaults();           // BertIntermediate: gelu(dense(x)) (erf form)
        p.A = x.p; p.lda = H; p.N = I; p.K = H; p.act = ACT_GELU; p.out32 = (float*)ffn.p; p.ldo = I;
        if (bert_gemm(lp + ".ffn1", p)) return -1;
        p = gemm_defaults();           // BertOutput: LayerNorm(dense(h) + x)
        p.A = ffn.p; p.lda = I; p.N = H; p.K = I; p.res = x.p; p.res_dtype = DT_F32; p.ldres = H; p.out32 = (float*)t.p; p.ldo = H;
        if (bert_gemm(lp + ".ffn2", p)) return -1;
        ln.x = (const float*)t.p; ln.gamma = g2; ln.beta = b2; ln.out32 = (float*)x.p;
        launch_layernorm(ln, h->stream);
    }
    WPTR(pw, float, "sb.pool.w"); WPTR(pb, float, "sb.pool.b");
    launch_bert_pooler((const float*)x.p, H, d_off, pw, pb, d_out, B, H, h->stream);
    HIPCHK(h, hipGetLastError());
    HIPCHK(h, hipMemcpyAsync(out, d_out, (size_t)B * H * 4, dev_in ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    return 0;
}

int64_t ev_get_stage(ev_handle* h, const char* name, void* host_dst, size_t cap) {
    if (!h || !name) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    if (!strcmp(name, "dur")) {
        const size_t need = (size_t)h->total_tokens * 8;
        if (!host_dst) return (int64_t)need;
        if (cap < need || !h->last_dur) return fail(h, "ev_get_stage(dur): buffer too small or no synthesis yet");
        HIPCHK(h, hipMemcpy(host_dst, h->last_dur, need, hipMemcpyDeviceToHost));
        return (int64_t)need;
    }
    if (!strcmp(name, "dur_eff")) {
        const size_t need = (size_t)h->total_tokens * 8;
        if (!host_dst) return (int64_t)need;
        if (cap < need || !h->last_dur_eff) return fail(h, "ev_get_stage(dur_eff): buffer too small or no synthesis yet");
        HIPCHK(h, hipMemcpy(host_dst, h->last_dur_eff, need, hipMemcpyDeviceToHost));
        return (int64_t)need;
    }
    if (!strcmp(name, "feat_mag")) {       // ev_features (keep_stages): the (total_frames, n_fft / 2 + 1) magnitudes of the last ev_features
        const size_t need = (size_t)h->feat_mag_elems * 4;
        if (!h->feat_mag) return fail(h, "ev_get_stage(feat_mag): no ev_features call with keep_stages yet");
        if (!host_dst) return (int64_t)need;
        if (cap < need) return fail(h, "ev_get_stage(feat_mag): need %zu bytes, cap %zu", need, cap);
        if (hipMemcpy(host_dst, h->feat_mag, need, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, "ev_get_stage(feat_mag): D2H failed");
        return (int64_t)need;
    }
    if (!strcmp(name, "resample_taps")) {  // ev_resample_setup: the (up, row) phase-major table in use
        const size_t need = h->rs_tab_floats * 4;
        if (!h->rs_ready) return fail(h, "ev_get_stage(resample_taps): ev_resample_setup has not been called");
        if (!host_dst) return (int64_t)need;
        if (cap < need) return fail(h, "ev_get_stage(resample_taps): need %zu bytes, cap %zu", need, cap);
        if (hipMemcpy(host_dst, h->rs_tab, need, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, "ev_get_stage(resample_taps): D2H failed");
        return (int64_t)need;
    }
    if (!strcmp(name, "stitch_ramp")) {    // ev_stitch: the F floats of the ramp table of the last call
        if (h->st_F < 0) return fail(h, "ev_get_stage(stitch_ramp): no ev_stitch call yet");
        const size_t need = (size_t)h->st_F * 4;
        if (!host_dst) return (int64_t)need;
        if (cap < need) return fail(h, "ev_get_stage(stitch_ramp): need %zu bytes, cap %zu", need, cap);
        if (need && hipMemcpy(host_dst, h->st_tab, need, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, "ev_get_stage(stitch_ramp): D2H failed");
        return (int64_t)need;
    }
    if (!strcmp(name, "resample_raw")) {   // ev_resample (keep_stages): the untrimmed y of the last ev_resample, packed
        const size_t need = (size_t)h->rs_raw_elems * 4;
        if (!h->rs_raw) return fail(h, "ev_get_stage(resample_raw): no ev_resample call with keep_stages yet");
        if (!host_dst) return (int64_t)need;
        if (cap < need) return fail(h, "ev_get_stage(resample_raw): need %zu bytes, cap %zu", need, cap);
        if (hipMemcpy(host_dst, h->rs_raw, need, hipMemcpyDeviceToHost) != hipSuccess) return fail(h, "ev_get_stage(resample_raw): D2H failed");
        return (int64_t)need;
    }
    if (!strcmp(name, "log_p_attn")) {     // ev_align: the (T_b, N_b) blocks of the utterances, concatenated
        const size_t need = (size_t)h->aln_lp_elems * 4;
        if (!h->aln_lp) return fail(h, "ev_get_stage(log_p_attn): the last call was not ev_align");
        if (!host_dst) return (int64_t)need;
        if (cap < need) return fail(h, "ev_get_stage(log_p_attn): need %zu bytes, cap %zu", need, cap);
        HIPCHK(h, hipMemcpy(host_dst, h->aln_lp, need, hipMemcpyDeviceToHost));
        return (int64_t)need;
    }
    if (!strcmp(name, "mel_len")) {
        const size_t need = (size_t)h->B * 8;
        if (!host_dst) return (int64_t)need;
        if (cap < need) return fail(h, "ev_get_stage(mel_len): buffer too small");
        for (int b = 0; b < h->B; ++b) ((int64_t*)host_dst)[b] = h->mel_lens[b];
        return (int64_t)need;
    }
    auto it = h->taps.find(name);
    if (it == h->taps.end()) return fail(h, "ev_get_stage: unknown stage '%s' (keep_stages=%d)", name, h->cfg.keep_stages);
    const Tap& t = it->second;
    int64_t nrows = 0;
    for (int b = 0; b < h->B; ++b) nrows += t.level == 0 ? h->tok_len[b] : ((int64_t)h->mel_lens[b] << t.shift);
    const size_t need = (size_t)nrows * t.C * 4;
    if (!host_dst) return (int64_t)need;
    if (cap < need) return fail(h, "ev_get_stage(%s): need %zu bytes, cap %zu", name, need, cap);
    float* d_tmp = nullptr; int64_t* d_scr = nullptr;
    HIPCHK(h, hipMalloc((void**)&d_tmp, need));
    HIPCHK(h, hipMalloc((void**)&d_scr, (3 * (size_t)h->B + 8) * 8));
    int rc = pack_level(h, t.ptr, t.dtype, t.ld, t.C, t.shift, t.level == 0, d_tmp, d_scr);
    if (rc == 0 && hipStreamSynchronize(h->stream) != hipSuccess) rc = fail(h, "ev_get_stage: gather failed");
    if (rc == 0 && hipMemcpy(host_dst, d_tmp, need, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(h, "ev_get_stage: D2H failed");
    (void)hipFree(d_tmp); (void)hipFree(d_scr);
    return rc ? -1 : (int64_t)need;
}

// ------------------------------------------------------------------- per-kernel test entry points (include/evhip_ops.h)
// what ev_op_conv_gemm and ev_op_conv_gemm_group3 refuse (-2) before any launcher sees the descriptor
static bool op_conv_gemm_desc_ok(const ConvGemmParams& p) {
    const int es = p.dtype == DT_F16 ? 2 : 4;
    if (p.M % ROW_ALIGN || p.N % 32 || (p.K * es) % 64 || (p.taps - 1) * p.dil > 64) return false;
    if (p.dtype == DT_F32S && (p.K % 32 || !p.W_lo)) return false;
    if (p.dtype == DT_MX && (p.K % 32 || !p.W)) return false;
    if (mx_check(p) || splitk_check(p)) return false;
    if (!p.out16 && !p.out32 && !p.mxo_h) return false;
    if (p.pro_lrelu && !(p.pro_slope >= 0.f && p.pro_slope <= 1.f)) return false;
    return true;
}
int ev_op_conv_gemm(const ev_conv_gemm_desc* d, void* stream) {
    static_assert(sizeof(ev_conv_gemm_desc) == sizeof(ConvGemmParams), "descriptor layout must match ConvGemmParams");
    ConvGemmParams p;
    memcpy(&p, d, sizeof p);
    if (!op_conv_gemm_desc_ok(p)) return -2;
    launch_conv_gemm(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
// three descriptors as ONE grouped grid (launch_conv_gemm_group3): 0 = launched (check_only: would be), -1 = not a triple the grouped kernel takes (nothing launched)
int ev_op_conv_gemm_group3(const ev_conv_gemm_desc* d3, int check_only, void* stream) {
    ConvGemmParams ps[3];
    memcpy(ps, d3, sizeof ps);
    for (int i = 0; i < 3; ++i)
        if (!op_conv_gemm_desc_ok(ps[i])) return -2;
    if (launch_conv_gemm_group3(ps, (hipStream_t)stream, check_only != 0)) return -1;
    if (check_only) return 0;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
size_t ev_op_mx_scratch_bytes(int M, int K) { return mx_scratch_bytes(M, K); }
int ev_op_resblock_pair_c32(const ev_res_pair_desc* d, void* stream) {
    static_assert(sizeof(ev_res_pair_desc) == sizeof(ResPairParams), "descriptor layout must match ResPairParams");
    ResPairParams p;
    memcpy(&p, d, sizeof p);
    if (p.k != 3 && p.k != 7 && p.k != 11) return -2;
    if (p.epi.post_lrelu && !(p.epi.post_slope >= 0.f && p.epi.post_slope <= 1.f)) return -2;   // max(v, s v) form of leaky-relu
    launch_resblock_pair_c32(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_resblock_pair_c32_mx(const ev_res_pair_desc* d, void* stream) {
    static_assert(sizeof(ev_res_pair_desc) == sizeof(ResPairParams), "descriptor layout must match ResPairParams");
    ResPairParams p;
    memcpy(&p, d, sizeof p);
    if (p.M <= 0 || p.dil < 1 || (p.k - 1) * p.dil > 64) return -2;
    if (launch_resblock_pair_c32_mx(p, (hipStream_t)stream)) return -2;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_resblock_pair_c64_mx(const ev_res_pair_desc* d, void* stream) {
    ResPairParams p;
    memcpy(&p, d, sizeof p);
    if (launch_resblock_pair_c64_mx(p, (hipStream_t)stream)) return -2;
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_resblock_pair_c64(const ev_res_pair_desc* d, void* stream) {
    ResPairParams p;
    memcpy(&p, d, sizeof p);
    if (p.k != 3) return -2;
    if (p.epi.post_lrelu && !(p.epi.post_slope >= 0.f && p.epi.post_slope <= 1.f)) return -2;
    launch_resblock_pair_c64(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_layernorm(const float* x, int rows, int C, const float* gamma, const float* beta, float eps, const uint8_t* row_valid,
                    void* out16, float* out32, const float* dot_w, float dot_b, float* dot_out, void* stream) {
    if (rows <= 0 || C < 128 || C > 1024 || C % 128 || (dot_w && !dot_out)) return -2;      // one wave per row, NV float2 chunks of 128 channels per lane
    LayerNormParams p{};
    p.x = x; p.ldx = C; p.rows = rows; p.C = C; p.gamma = gamma; p.beta = beta; p.eps = eps; p.row_valid = row_valid; p.out16 = out16;
    p.out32 = out32; p.ldo = C; p.dot_w = dot_w; p.dot_b = dot_b; p.dot_out = dot_out;
    launch_layernorm(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_layernorm_planes(const float* x, int rows, int C, const float* gamma, const float* beta, float eps, const uint8_t* row_valid,
                           void* h, void* q4h, void* q4l, void* qsh, void* qsl, unsigned qs_stride, void* stream) {
    if (rows <= 0 || C < 128 || C > 512 || C % 128 || !h || !q4h || !q4l || !qsh || !qsl) return -2;
    LayerNormParams p{};
    p.x = x; p.ldx = C; p.rows = rows; p.C = C; p.gamma = gamma; p.beta = beta; p.eps = eps; p.row_valid = row_valid; p.ldo = C;
    p.mxo_h = h; p.mxo_q4[0] = q4h; p.mxo_q4[1] = q4l; p.mxo_qs[0] = qsh; p.mxo_qs[1] = qsl; p.mxo_qs_stride = qs_stride;
    launch_layernorm(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_attention(const void* qkv, int is_f16, int C, int heads, const int32_t* seq_off, const int32_t* seq_len, int B, int max_len,
                    void* out, void* stream) {
    const int dk = heads > 0 && C % heads == 0 ? C / heads : 0;
    if (is_f16 < 0 || is_f16 > 2 || B <= 0 || max_len <= 0) return -2;
    if (is_f16 == 0 ? (dk != 48 && dk != 64) : dk != 48) return -2;          // the MFMA kernels are built for d_k = 48 (fp32: also 64)
    AttnParams p{};
    // is_f16 == 2: fp32 rows, split-precision products
    p.qkv = qkv; p.dtype = is_f16 == 1 ? DT_F16 : (is_f16 == 2 ? DT_F32S : DT_F32); p.ld = 3 * C; p.C = C; p.heads = heads; p.seq_off = seq_off; p.seq_len = seq_len;
    p.B = B; p.max_len = max_len; p.out = out; p.ldo = C;
    launch_attention(p, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}

// The non-GEMM launchers (ev_misc.hip, ev_align.hip).  Each wrapper refuses (-2) what its kernel silently assumes; include/evhip_ops.h states the limits.
int ev_op_embed_pe(const int64_t* ling, const int32_t* cu_seqlens, const int32_t* row_seq, const int32_t* row_pos, const float* emb, int n_vocab,
                   const float* pe, float alpha, float* out, float* tap_out, int rows, int C, void* stream) {
    if (rows <= 0 || C <= 0 || C % 2 || n_vocab < 1 || !out) return -2;
    launch_embed_pe(ling, cu_seqlens, row_seq, row_pos, emb, n_vocab, pe, alpha, out, tap_out, rows, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_bert_embed(const int64_t* ids, const int64_t* type_ids, const int32_t* cu_seqlens, const int32_t* row_seq, const int32_t* row_pos,
                     const float* word, const float* pos_emb, const float* type_emb, int vocab, int max_pos, int n_types, float* out, int rows,
                     int C, void* stream) {
    if (rows <= 0 || C <= 0 || C % 2 || vocab < 1 || max_pos < 1 || n_types < 1 || !out) return -2;
    launch_bert_embed(ids, type_ids, cu_seqlens, row_seq, row_pos, word, pos_emb, type_emb, vocab, max_pos, n_types, out, rows, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_bert_pooler(const float* x, int ldx, const int32_t* seq_off, const float* W, const float* bias, float* out, int B, int C, void* stream) {
    if (B <= 0 || B > 65535 || C <= 0 || ldx < C) return -2;
    launch_bert_pooler(x, ldx, seq_off, W, bias, out, B, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_cond_vector(const int64_t* speaker, const float* style, const float* content, const float* spk_emb, int n_speaker, const float* Wcond,
                      const float* bias, float* u, int B, int C, int bert, void* stream) {
    if (B <= 0 || B > 65535 || C <= 0 || bert < 0 || n_speaker < 1) return -2;
    launch_cond_vector(speaker, style, content, spk_emb, n_speaker, Wcond, bias, u, B, C, bert, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_var_embed_add(const float* x, const float* pitch, const float* energy, const float* wp, const float* bp, const float* we, const float* be,
                        const uint8_t* row_valid, float* out, int rows, int C, int k, void* stream) {
    if (rows <= 0 || C <= 0 || C % 2 || k < 1 || k % 2 == 0 || !row_valid) return -2;
    launch_var_embed_add(x, pitch, energy, wp, bp, we, be, row_valid, out, rows, C, k, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_prosody_tracks(const float* pitch, const float* energy, const int32_t* row_seq, const int32_t* row_pos, const int32_t* cu_seqlens,
                         const float* pitch_ovr, const float* energy_ovr, const float* ctrl, int B, float* pitch_out, float* energy_out, int rows,
                         void* stream) {
    if (rows <= 0 || B <= 0 || !ctrl) return -2;
    launch_prosody_tracks(pitch, energy, row_seq, row_pos, cu_seqlens, pitch_ovr, energy_ovr, ctrl, B, pitch_out, energy_out, rows, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_durations(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const int64_t* forced,
                    const int32_t* cu_seqlens, int64_t* dur_packed, float* logd_packed, float* centre_rows, int32_t* mel_len, void* stream) {
    if (B <= 0 || !(alpha > 0.f)) return -2;
    launch_durations(log_d, tok_off, tok_len, B, alpha, forced, cu_seqlens, dur_packed, logd_packed, centre_rows, mel_len, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_durations_prosody(const float* log_d, const int32_t* tok_off, const int32_t* tok_len, int B, float alpha, const float* alpha_b,
                            const int64_t* partial, int64_t dur_cap, const int32_t* cu_seqlens, int64_t* dur_packed, int64_t* dur_eff,
                            float* logd_packed, float* centre_rows, int32_t* mel_len, void* stream) {
    if (B <= 0 || !(alpha > 0.f) || dur_cap < 0 || dur_cap > (int64_t)1 << 20 || !dur_eff) return -2;
    launch_durations_prosody(log_d, tok_off, tok_len, B, alpha, alpha_b, partial, dur_cap, cu_seqlens, dur_packed, dur_eff, logd_packed, centre_rows,
                             mel_len, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_gauss_upsample(const float* xvar, const float* centre_rows, const int32_t* tok_off, const int32_t* tok_len, const int32_t* frm_row_seq,
                         const int32_t* frm_row_pos, const float* pe, float pe_alpha, float delta, float* out, float* tap_out, int rows, int C,
                         void* stream) {
    if (rows <= 0 || C <= 0 || C > 512 || C % 2 || !(delta > 0.f)) return -2;      // acc[4]: four float2 chunks of 128 channels per lane
    launch_gauss_upsample(xvar, centre_rows, tok_off, tok_len, frm_row_seq, frm_row_pos, pe, pe_alpha, delta, out, tap_out, rows, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_mel_to_rows(const void* mel, int is_f16, const int64_t* mel_elem_off, const int32_t* frm_row_seq, const int32_t* frm_row_pos,
                      const int32_t* mel_len, void* out, int out_f32, int rows, int n_mels, int ldo, void* stream) {
    if (rows <= 0 || n_mels <= 0 || ldo < n_mels) return -2;
    launch_mel_to_rows(mel, is_f16, mel_elem_off, frm_row_seq, frm_row_pos, mel_len, out, out_f32, rows, n_mels, ldo, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_conv_post(const void* x, int is_f32, int ldx, const float* w, float bias, int k, float pre_slope, const uint8_t* row_valid, int valid_shift,
                    float* wav_rows, int rows, int C, void* stream) {
    if (rows <= 0 || C != 32 || k < 1 || k > 15 || k % 2 == 0 || ldx < C || ldx % (is_f32 ? 4 : 8)) return -2;      // 16 taps of weights and 256 + 16 rows fit the LDS
    if (!row_valid || valid_shift < 0 || valid_shift > 30 || !(pre_slope >= 0.f && pre_slope <= 1.f)) return -2;  // max(v, s v) form of leaky-relu
    launch_conv_post(x, is_f32, ldx, w, bias, k, pre_slope, row_valid, valid_shift, wav_rows, rows, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_row_maps(const int32_t* off, const int32_t* len, int B, int32_t* seq, int32_t* pos, uint8_t* valid, int rows, void* stream) {
    if (rows <= 0 || B <= 0) return -2;
    launch_row_maps(off, len, B, seq, pos, valid, rows, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_pack_rows(const void* src, int is_f16, int ld, int C, const int64_t* seq_row_off, const int64_t* seq_out_off, const int32_t* seq_rows, int B,
                    int64_t max_rows, float* dst, void* stream) {
    if (B <= 0 || B > 65535 || C <= 0 || ld < C || max_rows < 0) return -2;
    launch_pack_rows(src, is_f16 ? DT_F16 : DT_F32, ld, C, seq_row_off, seq_out_off, seq_rows, B, max_rows, dst, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_wav_to_i16(const float* wav, int16_t* out, int64_t n, void* stream) {
    if (n <= 0) return -2;
    launch_wav_to_i16(wav, out, n, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_pe_extend(float* pe, const float* div, int row0, int row1, int C, void* stream) {
    if (row0 < 0 || row1 <= row0 || C <= 0 || C % 2) return -2;
    launch_pe_extend(pe, div, row0, row1, C, (hipStream_t)stream);
    return hipGetLastError() == hipSuccess ? 0 : -1;
}
int ev_op_stft_mel(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, const float* mel_basis, const float* window, int n_fft, int hop,
                   int n_mels, float mel_clip, float energy_floor, float energy_mean, float energy_std, float* mel, float* energy, float* mag,
                   void* stream) {
    if (!wav || !wav_lens || !mel_basis || !mel || !energy || B < 1 || B > 65535 || !stft_shape_ok(n_fft, hop, n_mels)) return -2;
    std::vector<StftSeq> seqs; std::vector<StftTile> tiles; std::vector<int32_t> lens; std::vector<int64_t> offs;
    if (features_layout(B, wav_lens, n_fft, hop, seqs, tiles, lens, offs)) return -2;
    char* basis = nullptr; float* melT = nullptr; char* tab = nullptr;
    int rc = features_upload_tables(nullptr, n_fft, n_mels, mel_basis, window, &basis, &melT) ? -1 : 0;
    const size_t sb = (size_t)B * sizeof(StftSeq), tb = tiles.size() * sizeof(StftTile);
    if (rc == 0 && hipMalloc((void**)&tab, sb + tb) != hipSuccess) rc = -1;
    if (rc == 0 && (hipMemcpy(tab, seqs.data(), sb, hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(tab + sb, tiles.data(), tb, hipMemcpyHostToDevice) != hipSuccess)) rc = -1;
    if (rc == 0) {
        StftParams p{};
        p.wav = wav; p.wav_is_i16 = wav_is_i16 != 0; p.seqs = (const StftSeq*)tab; p.tiles = (const StftTile*)(tab + sb); p.n_tiles = (int)tiles.size();
        p.basis = basis; p.melT = melT; p.n_fft = n_fft; p.hop = hop; p.n_mels = n_mels; p.nmi = stft_mels_per_group(n_mels); p.n_bins = n_fft / 2 + 1;
        p.n_btiles = stft_bin_tiles(n_fft); p.mel_clip = mel_clip; p.energy_floor = energy_floor; p.energy_mean = energy_mean; p.energy_std = energy_std;
        p.mel = mel; p.energy = energy; p.mag = mag;
        if (launch_stft_mel(p, (hipStream_t)stream)) rc = -2;
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -1;
    }
    if (basis) (void)hipFree(basis);
    if (melT) (void)hipFree(melT);
    if (tab) (void)hipFree(tab);
    return rc;
}

int ev_op_pitch_yin(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, int sample_rate, int hop, int win, float f_min, float f_max,
                    float threshold, float silence_rms, float* f0_hz, float* aperiodicity, int32_t* tau, void* stream) {
    if (!wav || !wav_lens || !f0_hz || !aperiodicity || B < 1 || B > 65535) return -2;
    ev_pitch_config c;
    ev_default_pitch_config(&c);
    c.sample_rate = sample_rate; c.hop = hop; c.win = win; c.f_min = f_min; c.f_max = f_max; c.threshold = threshold; c.silence_rms = silence_rms;
    int tau_min = 0, tau_max = 0;
    if (pitch_check_config(nullptr, "ev_op_pitch_yin", c, &tau_min, &tau_max)) return -2;
    std::vector<StftSeq> seqs; std::vector<StftTile> tiles; std::vector<int32_t> lens; std::vector<int64_t> offs;
    if (pitch_layout(B, wav_lens, hop, seqs, tiles, lens, offs)) return -2;
    char* tab = nullptr;
    const size_t sb = (size_t)B * sizeof(StftSeq), tb = tiles.size() * sizeof(StftTile);
    if (hipMalloc((void**)&tab, sb + tb) != hipSuccess) return -1;
    int rc = 0;
    if (hipMemcpy(tab, seqs.data(), sb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(tab + sb, tiles.data(), tb, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (rc == 0) {
        PitchParams p = pitch_params(c, tau_min, tau_max);
        p.wav = wav; p.wav_is_i16 = wav_is_i16 != 0; p.seqs = (const StftSeq*)tab; p.tiles = (const StftTile*)(tab + sb); p.n_tiles = (int)tiles.size();
        p.f0 = f0_hz; p.ap = aperiodicity; p.tau = tau;
        if (launch_pitch_yin(p, (hipStream_t)stream)) rc = -2;
        else if (hipGetLastError() != hipSuccess) rc = -1;
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -1;
    }
    (void)hipFree(tab);
    return rc;
}
int ev_op_pitch_fill(const float* f0_hz, int B, const int32_t* frames, float pitch_mean, float pitch_std, float* pitch, void* stream) {
    if (!f0_hz || !frames || !pitch || pitch == f0_hz || B < 1 || B > 65535) return -2;
    if (!std::isfinite(pitch_mean) || !std::isfinite(pitch_std) || !(pitch_std > 0.f)) return -2;
    std::vector<StftSeq> seqs((size_t)B);
    int64_t fo = 0;
    for (int b = 0; b < B; ++b) {
        if (frames[b] < 1 || frames[b] > EV_ALIGN_MAX_FRAMES) return -2;
        seqs[(size_t)b] = StftSeq{0, 0, fo, frames[b], 0};
        fo += frames[b];
    }
    StftSeq* d = nullptr;
    if (hipMalloc((void**)&d, seqs.size() * sizeof(StftSeq)) != hipSuccess) return -1;
    int rc = hipMemcpy(d, seqs.data(), seqs.size() * sizeof(StftSeq), hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    if (rc == 0) {
        launch_pitch_fill(f0_hz, d, B, pitch_mean, pitch_std, pitch, (hipStream_t)stream);
        if (hipGetLastError() != hipSuccess) rc = -1;
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -1;
    }
    (void)hipFree(d);
    return rc;
}

int ev_op_resample(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, int sr_in, int sr_out, const float* taps, int half_len, float* y,
                   void* stream) {
    if (!wav || !wav_lens || !y || B < 1 || B > 65535) return -2;
    ev_resample_config c;
    ev_default_resample_config(&c);
    c.sr_in = sr_in; c.sr_out = sr_out; c.taps = taps; c.half_len = half_len;
    int up = 0, down = 0, half = 0;
    std::vector<float> ht;
    if (resample_check_config(nullptr, "ev_op_resample", c, &up, &down, &half, ht)) return -2;
    std::vector<ResampleSeq> seqs; std::vector<ResampleTile> tiles;
    if (resample_layout(B, wav_lens, up, down, 0, seqs, tiles)) return -2;
    float* tab = nullptr; size_t floats = 0;
    if (resample_upload_table(up, half, ht, &tab, &floats)) return -1;
    char* lay = nullptr;
    const size_t sb = (size_t)B * sizeof(ResampleSeq), tb = tiles.size() * sizeof(ResampleTile);
    int rc = hipMalloc((void**)&lay, sb + tb) == hipSuccess ? 0 : -1;
    if (rc == 0 && (hipMemcpy(lay, seqs.data(), sb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(lay + sb, tiles.data(), tb, hipMemcpyHostToDevice) != hipSuccess)) rc = -1;
    if (rc == 0) {
        if (resample_launch(wav, wav_is_i16 != 0, up, down, half, tab, (const ResampleSeq*)lay, (const ResampleTile*)(lay + sb), (int)tiles.size(),
                            seqs[B - 1].in_off + seqs[B - 1].len, y, (hipStream_t)stream)) rc = -2;
        else if (hipGetLastError() != hipSuccess) rc = -1;
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -1;
    }
    if (lay) (void)hipFree(lay);
    (void)hipFree(tab);
    return rc;
}
int ev_op_trim(const float* y, int B, const int64_t* lens, float trim_frac, int trim_pad, float* out, int64_t* out_lens, int64_t* trim_start,
               int64_t* trim_end, void* stream) {
    if (!y || !lens || !out || !out_lens || !trim_start || !trim_end || out == y || B < 1 || B > 65535) return -2;
    if (!std::isfinite(trim_frac) || !(trim_frac > 0.f) || !(trim_frac < 1.f) || trim_pad < 0) return -2;
    std::vector<ResampleSeq> seqs((size_t)B);
    int64_t o = 0;
    for (int b = 0; b < B; ++b) {
        if (lens[b] < 1 || lens[b] + 2 * (int64_t)trim_pad > RS_MAX_OUT) return -2;
        seqs[(size_t)b] = ResampleSeq{o, lens[b], o, lens[b]};
        o += lens[b];
    }
    char* lay = nullptr;
    const size_t sb = (size_t)B * sizeof(ResampleSeq), cb = 2 * (size_t)B * sizeof(int64_t), tb = (size_t)B * sizeof(TrimSeq);
    if (hipMalloc((void**)&lay, sb + cb + tb) != hipSuccess) return -1;
    hipStream_t s = (hipStream_t)stream;
    int64_t* d_cuts = (int64_t*)(lay + sb);
    std::vector<int64_t> cuts(2 * (size_t)B);
    std::vector<TrimSeq> ts;
    int rc = hipMemcpy(lay, seqs.data(), sb, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    if (rc == 0) {
        launch_trim_scan(y, (const ResampleSeq*)lay, B, trim_frac, d_cuts, s);
        if (hipGetLastError() != hipSuccess || hipStreamSynchronize(s) != hipSuccess) rc = -1;
    }
    if (rc == 0 && hipMemcpy(cuts.data(), d_cuts, cb, hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    if (rc == 0) {
        const int64_t longest = trim_plan(B, seqs, cuts.data(), trim_pad, ts, out_lens, nullptr, trim_start, trim_end);
        if (hipMemcpy(lay + sb + cb, ts.data(), tb, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
        if (rc == 0) {
            launch_trim_gather(y, (const TrimSeq*)(lay + sb + cb), B, longest, trim_pad, out, s);
            if (hipGetLastError() != hipSuccess) rc = -1;
            if (hipStreamSynchronize(s) != hipSuccess) rc = -1;
        }
    }
    (void)hipFree(lay);
    return rc;
}

int ev_op_stitch_scan(const float* wav, int S, const int64_t* seg_offsets, const int64_t* seg_lens, float trim_frac, float trim_abs, float* peak,
                      int64_t* first, int64_t* last, void* stream) {
    if (!wav || !seg_offsets || !seg_lens || !peak || !first || !last || S < 1 || S > 65535) return -2;
    if (stitch_check_trim(nullptr, "ev_op_stitch_scan", trim_frac, trim_abs)) return -2;
    std::vector<StitchSeg> segs((size_t)S);
    int64_t n_part = 0, max_len = 0;
    for (int s = 0; s < S; ++s) {
        if (seg_offsets[s] < 0 || seg_lens[s] < 1) return -2;
        segs[(size_t)s] = StitchSeg{seg_offsets[s], seg_lens[s], n_part};
        n_part += (seg_lens[s] + ST_PEAK_CHUNK - 1) / ST_PEAK_CHUNK;
        max_len = std::max(max_len, seg_lens[s]);
    }
    const size_t sb = (size_t)S * sizeof(StitchSeg), cb = 2 * (size_t)S * sizeof(int64_t), pb = align_up((size_t)S * sizeof(float), 8), qb = (size_t)n_part * sizeof(float);
    char* lay = nullptr;
    if (hipMalloc((void**)&lay, sb + cb + pb + qb) != hipSuccess) return -1;
    hipStream_t s = (hipStream_t)stream;
    int64_t* d_cuts = (int64_t*)(lay + sb); float* d_peak = (float*)(lay + sb + cb); float* d_part = (float*)(lay + sb + cb + pb);
    std::vector<int64_t> cuts(2 * (size_t)S);
    int rc = hipMemcpy(lay, segs.data(), sb, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    if (rc == 0) {
        launch_stitch_peak(wav, (const StitchSeg*)lay, S, max_len, d_part, s);
        launch_stitch_edges(wav, (const StitchSeg*)lay, S, d_part, trim_frac, trim_abs, d_peak, d_cuts, s);
        if (hipGetLastError() != hipSuccess) rc = -1;
        if (hipStreamSynchronize(s) != hipSuccess) rc = -1;
    }
    if (rc == 0 && (hipMemcpy(cuts.data(), d_cuts, cb, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(peak, d_peak, (size_t)S * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
    if (rc == 0) for (int i = 0; i < S; ++i) { first[i] = cuts[2 * (size_t)i]; last[i] = cuts[2 * (size_t)i + 1]; }
    (void)hipFree(lay);
    return rc;
}
int ev_op_flac_encode(const void* pcm, int pcm_is_i16, int B, const int64_t* lens, const ev_flac_config* cfg, uint8_t* slots, int32_t* sizes,
                      uint8_t* kind, uint8_t* porder, void* stream) {
    ev_flac_config c;
    if (cfg) c = *cfg; else ev_default_flac_config(&c);
    if (!pcm || !lens || !slots || !sizes || !kind || !porder || B < 1 || B > 65535 || c.struct_size != sizeof(ev_flac_config)) return -2;
    const int sr_code = flac_rate_code(c.sample_rate), bs_code = flac_block_code(c.block_size);
    if (sr_code < 0 || bs_code < 0 || c.max_fixed_order < 0 || c.max_fixed_order > 4 || c.max_partition_order < 0 || c.max_partition_order > 6 ||
        (c.convert != EV_FLAC_WRAP && c.convert != EV_FLAC_CLAMP) || (reinterpret_cast<uintptr_t>(slots) & 3)) return -2;
    const int N = c.block_size;
    std::vector<FlacFrame> frames;
    int64_t off = 0;
    for (int b = 0; b < B; off += lens[b], ++b) {
        if (lens[b] < 1 || lens[b] > EV_FLAC_MAX_SAMPLES || (int64_t)frames.size() + (lens[b] + N - 1) / N > INT_MAX) return -2;
        for (int64_t i = 0; i < lens[b]; i += N) frames.push_back(FlacFrame{off + i, (int32_t)std::min<int64_t>(N, lens[b] - i), (int32_t)(i / N), (int32_t)b, 0});
    }
    const size_t NF = frames.size(), fb = NF * sizeof(FlacFrame), sb = NF * sizeof(int32_t);
    char* lay = nullptr;
    if (hipMalloc((void**)&lay, fb + 2 * sb) != hipSuccess) return -1;
    hipStream_t s = (hipStream_t)stream;
    FlacParams fp{};
    fp.pcm = pcm; fp.pcm_is_i16 = pcm_is_i16 != 0; fp.convert = c.convert; fp.block_size = N; fp.bs_code = bs_code; fp.sr_code = sr_code;
    fp.max_fixed_order = c.max_fixed_order; fp.max_partition_order = c.max_partition_order; fp.frames = (const FlacFrame*)lay; fp.scratch = slots;
    fp.stride = 2 * N + 24; fp.sizes = (int32_t*)(lay + fb); fp.desc = (uint32_t*)(lay + fb + sb);
    std::vector<uint32_t> desc(NF);
    int rc = hipMemcpy(lay, frames.data(), fb, hipMemcpyHostToDevice) == hipSuccess ? 0 : -1;
    if (rc == 0) {
        if (launch_flac_encode(fp, (int64_t)NF, s) || hipGetLastError() != hipSuccess) rc = -1;
        if (hipStreamSynchronize(s) != hipSuccess) rc = -1;
    }
    if (rc == 0 && (hipMemcpy(sizes, fp.sizes, sb, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(desc.data(), fp.desc, sb, hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
    if (rc == 0) for (size_t f = 0; f < NF; ++f) { kind[f] = (uint8_t)(desc[f] & 0xFFu); porder[f] = (uint8_t)(desc[f] >> 8 & 0xFFu); }
    (void)hipFree(lay);
    return rc;
}
int ev_op_stitch_mix(const float* wav, int S, const int64_t* src, const int64_t* n, const int32_t* seg_doc, const int64_t* pos, const int32_t* fl,
                     const int32_t* fr, const float* tab, int F, int D, const int64_t* doc_lens, float* out, int16_t* out_i16, void* stream) {
    if (!wav || !src || !n || !seg_doc || !pos || !fl || !fr || !doc_lens || !out || S < 1 || S > 65535) return -2;
    if (F < 0 || F > EV_STITCH_MAX_FADE || (F > 0 && !tab) || seg_doc[0] != 0) return -2;
    for (int s = 0; s < S; ++s) {
        const bool head = s == 0 || seg_doc[s] != seg_doc[s - 1];
        if (s > 0 && seg_doc[s] != seg_doc[s - 1] && seg_doc[s] != seg_doc[s - 1] + 1) return -2;
        if (seg_doc[s] >= D || src[s] < 0 || n[s] < 0 || n[s] > EV_STITCH_MAX_DOC || pos[s] < 0) return -2;
        if (doc_lens[seg_doc[s]] < 0 || doc_lens[seg_doc[s]] > EV_STITCH_MAX_DOC || pos[s] + n[s] > doc_lens[seg_doc[s]]) return -2;
        if (fl[s] < 0 || fr[s] < 0 || fl[s] > std::min((int64_t)F, n[s]) || fr[s] > std::min((int64_t)F, n[s])) return -2;
        if (!head && (pos[s] < pos[s - 1] || pos[s] + n[s] < pos[s - 1] + n[s - 1])) return -2;
        if (!head && s >= 2 && seg_doc[s - 2] == seg_doc[s] && pos[s] < pos[s - 2] + n[s - 2]) return -2;
    }
    if (seg_doc[S - 1] + 1 != D) return -2;
    std::vector<StitchMixSeg> ms; std::vector<StitchDoc> docs; std::vector<StitchTile> tiles; std::vector<int64_t> offs((size_t)D + 1);
    stitch_tables(S, D, src, n, seg_doc, pos, fl, fr, doc_lens, ms, docs, tiles, offs.data());
    const size_t mb = (size_t)S * sizeof(StitchMixSeg), db = (size_t)D * sizeof(StitchDoc), tb = tiles.size() * sizeof(StitchTile), fb = (size_t)F * sizeof(float);
    char* lay = nullptr;
    if (hipMalloc((void**)&lay, mb + db + tb + fb + 16) != hipSuccess) return -1;
    int rc = 0;
    if (hipMemcpy(lay, ms.data(), mb, hipMemcpyHostToDevice) != hipSuccess || hipMemcpy(lay + mb, docs.data(), db, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (rc == 0 && tb && hipMemcpy(lay + mb + db, tiles.data(), tb, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (rc == 0 && fb && hipMemcpy(lay + mb + db + tb, tab, fb, hipMemcpyHostToDevice) != hipSuccess) rc = -1;
    if (rc == 0) {
        if (launch_stitch_mix(wav, (const StitchMixSeg*)lay, (const StitchDoc*)(lay + mb), (const StitchTile*)(lay + mb + db), (int64_t)tiles.size(),
                              (const float*)(lay + mb + db + tb), F, out, out_i16, (hipStream_t)stream)) rc = -2;
        else if (hipGetLastError() != hipSuccess) rc = -1;
        if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -1;
    }
    (void)hipFree(lay);
    return rc;
}

// The AlignSeq table of the two aligner kernels is built here from per-utterance HOST arrays (no struct crosses the boundary); both calls
// copy it to the device, launch, and wait for the stream before releasing it.
static int op_align_table(int B, const int32_t* tok_row, const int32_t* tokens, const int32_t* frm_row, const int32_t* frames, const int64_t* lp_off,
                          const int64_t* tok_packed, const int64_t* frm_packed, const int64_t* bits_off, bool mas, AlignSeq** d_out, int* max_tok,
                          int* max_frm) {
    if (B <= 0 || B > 65535 || !tokens || !frames || !lp_off) return -2;
    std::vector<AlignSeq> tab((size_t)B);
    *max_tok = 0; *max_frm = 0;
    for (int b = 0; b < B; ++b) {
        if (tokens[b] < 1 || tokens[b] > EV_ALIGN_MAX_TOKENS || frames[b] < 1 || frames[b] > EV_ALIGN_MAX_FRAMES || lp_off[b] < 0) return -2;
        if (mas && frames[b] < tokens[b]) return -2;          // a monotonic path gives every token at least one frame
        AlignSeq q{};
        q.tok_row = tok_row ? tok_row[b] : 0; q.tokens = tokens[b]; q.frm_row = frm_row ? frm_row[b] : 0; q.frames = frames[b];
        q.lp_off = lp_off[b]; q.tok_packed = tok_packed ? tok_packed[b] : 0; q.frm_packed = frm_packed ? frm_packed[b] : 0;
        q.bits_off = bits_off ? bits_off[b] : 0;
        if (q.tok_row < 0 || q.frm_row < 0 || q.tok_packed < 0 || q.frm_packed < 0 || q.bits_off < 0) return -2;
        tab[(size_t)b] = q;
        *max_tok = std::max(*max_tok, tokens[b]); *max_frm = std::max(*max_frm, frames[b]);
    }
    AlignSeq* d = nullptr;
    if (hipMalloc((void**)&d, tab.size() * sizeof(AlignSeq)) != hipSuccess) return -1;
    if (hipMemcpy(d, tab.data(), tab.size() * sizeof(AlignSeq), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(d); return -1; }
    *d_out = d;
    return 0;
}
int ev_op_align_score(const float* text, const float* feats, int C, int B, const int32_t* tok_row, const int32_t* tokens, const int32_t* frm_row,
                      const int32_t* frames, const int64_t* lp_off, float* log_p, void* stream) {
    if (C <= 0 || C % 32 || !tok_row || !frm_row || !log_p) return -2;      // channels are staged 32 at a time
    AlignSeq* d = nullptr; int max_tok = 0, max_frm = 0;
    int rc = op_align_table(B, tok_row, tokens, frm_row, frames, lp_off, nullptr, nullptr, nullptr, false, &d, &max_tok, &max_frm);
    if (rc) return rc;
    launch_align_score(text, feats, C, d, B, max_frm, log_p, (hipStream_t)stream);
    rc = hipGetLastError() == hipSuccess ? 0 : -1;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -1;
    (void)hipFree(d);
    return rc;
}
int ev_op_align_mas(const float* log_p, int B, const int32_t* tokens, const int32_t* frames, const int64_t* lp_off, const int64_t* tok_packed,
                    const int64_t* frm_packed, const int64_t* bits_off, uint32_t* bits, const float* pitch_frames, const float* energy_frames,
                    int64_t* dur, float* pitch_tok, float* energy_tok, float* score, void* stream) {
    if (!log_p || !tok_packed || !frm_packed || !bits_off || !bits || !dur || !score) return -2;
    if ((pitch_frames && !pitch_tok) || (energy_frames && !energy_tok)) return -2;
    AlignSeq* d = nullptr; int max_tok = 0, max_frm = 0;
    int rc = op_align_table(B, nullptr, tokens, nullptr, frames, lp_off, tok_packed, frm_packed, bits_off, true, &d, &max_tok, &max_frm);
    if (rc) return rc;
    launch_align_mas(log_p, d, B, max_tok, bits, pitch_frames, energy_frames, dur, pitch_tok, energy_tok, score, (hipStream_t)stream);
    rc = hipGetLastError() == hipSuccess ? 0 : -1;
    if (hipStreamSynchronize((hipStream_t)stream) != hipSuccess) rc = -1;
    (void)hipFree(d);
    return rc;
}

}  // extern "C"
