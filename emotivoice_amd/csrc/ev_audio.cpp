// libevhip.so host side: the audio utilities of include/evhip.h -- ev_features, ev_pitch, ev_resample, ev_stitch, ev_compare, ev_flac, ev_loudness, ev_limit, ev_deliver, ev_score, ev_denoise, ev_stretch, ev_watermark -- with
// their config, setup, design and plan entry points, and the per-kernel test entry points (include/evhip_ops.h) of their kernels and of the aligner's.
// Every utility call has the same shape: check the arguments, lay the batch out on the host (ev_layout.h), call_begin, plan its arena, upload, launch,
// call_end, publish the result.  The result stays valid until the next call of the same utility: each has its own arena and its own host vectors.
#include <math.h>
#include <stdlib.h>

#include <algorithm>
#include <cmath>
#include <limits>

#include "ev_host.h"

using namespace ev;
using namespace evh;

namespace {

// a host table to its place in the arena, on the handle's stream (the vector must live until the stream has been waited for)
template <typename T> int upload(ev_handle* h, T* dst, const std::vector<T>& v) {
    HIPCHK(h, hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, h->stream));
    return 0;
}

// The waveform a utility call reads: the caller's own pointer with EV_FLAG_DEVICE_INPUTS, else a staging buffer in the utility's arena that copy() fills
// on the handle's stream.  `bytes` is what the kernel reads of it.
struct WavIn {
    const void* src; size_t bytes; bool dev; void* stage = nullptr;
    WavIn(const void* p, int64_t elements, int wav_is_i16, uint32_t flags)
        : src(p), bytes((size_t)elements * (wav_is_i16 ? 2 : 4)), dev((flags & EV_FLAG_DEVICE_INPUTS) != 0) {}
    void plan(ArenaPlan& ap) { stage = dev ? nullptr : ap.take(bytes); }
    int copy(ev_handle* h) const {
        if (!dev) HIPCHK(h, hipMemcpyAsync(stage, src, bytes, hipMemcpyHostToDevice, h->stream));
        return 0;
    }
    const void* ptr() const { return dev ? src : stage; }
};

// what every forward STFT kernel takes (StftFront, ev_kernels.h)
StftFront stft_front(const void* wav, int wav_is_i16, const StftSeq* seqs, const StftTile* tiles, size_t n_tiles, const void* basis, int n_fft, int hop) {
    return StftFront{wav, wav_is_i16 != 0, seqs, tiles, (int)n_tiles, basis, n_fft, hop, stft_bin_tiles(n_fft)};
}

// the checks ev_denoise, ev_watermark and ev_watermark_detect share, and the frame grid of the batch: 0, or -1 with the message set.  `unit` is what
// the caller's messages call an element of the batch
int stft_grid(ev_handle* h, const char* who, const char* unit, int n_fft, int hop, int B, const void* wav, const int64_t* lens, FrameGrid& g) {
    if (!wav) return fail(h, "%s: wav is NULL", who);
    if (!lens) return fail(h, "%s: lens is NULL", who);
    if (B < 1 || B > 65535) return fail(h, "%s: B = %d outside [1, 65535]", who, B);
    const int bad = frame_grid_layout(B, lens, n_fft / 2 + 1, hop, 64, g);
    if (bad > 0) return fail(h, "%s: lens[%d] = %lld < n_fft / 2 + 1 = %d (reflect padding needs that many samples)", who, bad - 1, (long long)lens[bad - 1], n_fft / 2 + 1);
    if (bad < 0) return fail(h, "%s: %s %d has %lld frames > EV_ALIGN_MAX_FRAMES %d", who, unit, -bad - 1, (long long)(lens[-bad - 1] / hop + 1), EV_ALIGN_MAX_FRAMES);
    return 0;
}

// The second half of ev_denoise and ev_watermark: the scratch planes that the caller's forward kernel fills, their inverse STFT and the packed result.
// Used like WavIn: built from the grid, plan() inside the arena's plan, copy() with the uploads, then -- after the forward launch into hi / lo --
// inverse(), and finish() once the call has ended.
struct IstftTrip {
    std::vector<IstftSeq> seqs; std::vector<StftTile> tiles;
    int n_fft, hop, KP; bool want16; int64_t total_frames, total_out;
    IstftSeq* d_seqs = nullptr; StftTile* d_tiles = nullptr; uint16_t *hi = nullptr, *lo = nullptr; float* out = nullptr; int16_t* out_i16 = nullptr;
    IstftTrip(const FrameGrid& g, int n_fft_, int hop_, bool want16_)
        : n_fft(n_fft_), hop(hop_), KP(denoise_k_pad(n_fft_)), want16(want16_), total_frames(g.offs.back()),
          total_out(istft_layout((int)g.lens.size(), g.lens.data(), n_fft_, hop_, seqs, tiles)) {}
    void plan(ArenaPlan& ap) {
        d_seqs = ap.arr<IstftSeq>(seqs.size()); d_tiles = ap.arr<StftTile>(tiles.size());
        hi = ap.arr<uint16_t>((size_t)total_frames * KP); lo = ap.arr<uint16_t>((size_t)total_frames * KP);
        out = ap.arr<float>((size_t)total_out); out_i16 = want16 ? ap.arr<int16_t>((size_t)total_out) : nullptr;
    }
    int copy(ev_handle* h) const { return upload(h, d_seqs, seqs) || upload(h, d_tiles, tiles); }
    double plane_bytes() const { return 4.0 * (double)total_frames * KP; }      // both planes, as the forward kernel writes them
    int inverse(ev_handle* h, const char* who, const StftTables& t) const {
        if (!tiles.empty()) {
            const IstftParams p{hi, lo, d_seqs, d_tiles, (int)tiles.size(), t.ibasis.get(), t.env.as<float>(), n_fft, hop, n_fft / hop, KP, out, out_i16};
            KScope ks(h, "istft_ola", 2.0 * 3.0 * (double)DN_TJ * (double)tiles.size() * (double)p.R * KP * hop, plane_bytes() + (double)total_out * (want16 ? 6.0 : 4.0));
            if (launch_istft_ola(p, h->stream)) return fail(h, "%s: the kernel does not build this shape", who);
        }
        HIPCHK(h, hipGetLastError());
        return 0;
    }
    template <typename R> void finish(WavOut& keep, R* res) const {      // R: ev_denoise_result or ev_watermark_result
        const size_t B = seqs.size();
        keep.lens.resize(B); keep.offs.resize(B + 1);
        for (size_t b = 0; b < B; ++b) { keep.lens[b] = seqs[b].out_len; keep.offs[b] = seqs[b].out_off; }
        keep.offs[B] = total_out;
        reset_result(res);
        res->batch = (int)B; res->total = total_out; res->wav = out; res->wav_i16 = out_i16;
        res->lens_out = keep.lens.data(); res->offsets = keep.offs.data();
    }
};

// The device side of a per-kernel test entry point (the end of this file): ONE allocation that holds the host tables appended with add() and the
// scratch reserved with room(), each at an aligned offset.  commit() allocates and uploads, at<T>() turns an offset into its pointer, and the end
// of the scope frees -- after the wrapper has waited for the stream.
struct DevTable {
    struct Part { size_t off; const void* src; size_t bytes; };
    std::vector<Part> parts; size_t size = 0; DevMem mem;
    size_t room(size_t bytes) { const size_t off = align_up(size, 256); size = off + bytes; return off; }
    size_t add(const void* src, size_t bytes) { const size_t off = room(bytes); parts.push_back(Part{off, src, bytes}); return off; }
    template <typename T> size_t add(const std::vector<T>& v) { return add(v.data(), v.size() * sizeof(T)); }
    int commit() {      // 0, or -1
        if (mem.alloc(size + 16) != hipSuccess) return -1;
        for (const Part& p : parts)
            if (p.bytes && hipMemcpy(mem.as<char>() + p.off, p.src, p.bytes, hipMemcpyHostToDevice) != hipSuccess) return -1;
        return 0;
    }
    template <typename T> T* at(size_t off) const { return reinterpret_cast<T*>(mem.as<char>() + off); }
};

// The end of a per-kernel test entry point, after its last launch: -2 for a launch the wrapper refused, -1 (over -2) for a launch error or a failed
// wait for the stream, else 0.  The tables may go once it has returned.
int op_finish(int launch_rc, hipStream_t s) {
    int rc = launch_rc ? -2 : 0;
    if (hipGetLastError() != hipSuccess) rc = -1;
    if (hipStreamSynchronize(s) != hipSuccess) rc = -1;
    return rc;
}

}  // namespace

extern "C" {

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

// packs the basis planes on the host and uploads them into fresh allocations; nothing half-built is left behind
static int features_upload_tables(ev_handle* h, int n_fft, int n_mels, const float* mel_basis, const float* window, DevMem& basis, DevMem& melT) {
    std::vector<uint16_t> hb(stft_basis_halfs(n_fft));
    std::vector<float> hm(stft_melT_floats(n_fft));
    stft_pack_basis(n_fft, window, hb.data());
    stft_pack_mel(n_fft, n_mels, mel_basis, hm.data());
    hipError_t e = dev_upload(basis, hb);
    if (e == hipSuccess) e = dev_upload(melT, hm);
    if (e == hipSuccess) return 0;
    basis.reset();
    return fail(h, "ev_features: uploading the basis planes failed: %s", hipGetErrorString(e));
}

int ev_features_setup(ev_handle* h, const ev_features_config* cfg) {
    if (!h) return -1;
    if (!cfg) return fail(h, "ev_features_setup: null config");
    if (check_struct_size(h, "ev_features_setup", "struct_size", cfg->struct_size, "ev_features_config", sizeof(ev_features_config))) return -1;
    if (features_check_config(h, "ev_features_setup", cfg->n_fft, cfg->hop, cfg->n_mels)) return -1;
    if (!cfg->mel_basis) return fail(h, "ev_features_setup: mel_basis is required");
    if (!(cfg->mel_clip > 0.f) || !std::isfinite(cfg->mel_clip)) return fail(h, "ev_features_setup: mel_clip must be positive and finite");
    if (!(cfg->energy_floor >= 0.f) || !std::isfinite(cfg->energy_floor)) return fail(h, "ev_features_setup: energy_floor must be >= 0 and finite");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    DevMem basis, melT;
    if (features_upload_tables(h, cfg->n_fft, cfg->n_mels, cfg->mel_basis, cfg->window, basis, melT)) return -1;
    h->feat.basis = std::move(basis); h->feat.melT = std::move(melT);
    h->feat.cfg = *cfg; h->feat.cfg.mel_basis = nullptr; h->feat.cfg.window = nullptr;
    h->feat.ready = true;
    return 0;
}

int ev_features(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* wav_lens, float energy_mean, float energy_std, uint32_t flags,
                ev_features_result* out) {
    if (!h) return -1;
    if (!wav || !wav_lens || !out || B <= 0) return fail(h, "ev_features: bad argument");
    if (check_struct_size(h, "ev_features", "out->struct_size", out->struct_size, "ev_features_result", sizeof(ev_features_result))) return -1;
    if (!h->feat.ready) return fail(h, "ev_features: ev_features_setup has not been called");
    if ((size_t)B > PIN_MAX_B) return fail(h, "ev_features: at most %zu utterances per call", PIN_MAX_B);
    if (!std::isfinite(energy_std) || !(energy_std > 0.f)) return fail(h, "ev_features: energy_std must be positive and finite");
    if (!std::isfinite(energy_mean)) return fail(h, "ev_features: energy_mean must be finite");
    const ev_features_config& fc = h->feat.cfg;
    const int n_bins = fc.n_fft / 2 + 1;
    FrameGrid g;
    const int bad = frame_grid_layout(B, wav_lens, fc.n_fft / 2 + 1, fc.hop, 64, g);
    if (bad > 0) return fail(h, "ev_features: wav_lens[%d] = %lld < n_fft / 2 + 1 = %d (reflect padding needs that many samples)", bad - 1, (long long)wav_lens[bad - 1], fc.n_fft / 2 + 1);
    if (bad < 0) return fail(h, "ev_features: utterance %d has %lld frames > EV_ALIGN_MAX_FRAMES %d", -bad - 1, (long long)(wav_lens[-bad - 1] / fc.hop + 1), EV_ALIGN_MAX_FRAMES);
    const int64_t total_frames = g.offs[B], total_samples = g.seqs[B - 1].wav_off + g.seqs[B - 1].len;
    const bool keep = h->cfg.keep_stages != 0;
    WavIn in(wav, total_samples, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    h->feat.mag = nullptr;
    StftSeq* d_seqs = nullptr; StftTile* d_tiles = nullptr; float *d_mel = nullptr, *d_energy = nullptr, *d_mag = nullptr;
    if (arena_plan(h, ARENA_FEATURES, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_seqs = ap.arr<StftSeq>(B); d_tiles = ap.arr<StftTile>(g.tiles.size());
        d_mel = ap.arr<float>((size_t)total_frames * fc.n_mels); d_energy = ap.arr<float>((size_t)total_frames);
        d_mag = keep ? ap.arr<float>((size_t)total_frames * n_bins) : nullptr;
    })) return -1;
    if (in.copy(h) || upload(h, d_seqs, g.seqs) || upload(h, d_tiles, g.tiles)) return -1;
    region_begin(h, "total");
    {
        const StftParams p{stft_front(in.ptr(), wav_is_i16, d_seqs, d_tiles, g.tiles.size(), h->feat.basis.get(), fc.n_fft, fc.hop), h->feat.melT.as<float>(),
                           fc.n_mels, fc.mel_clip, fc.energy_floor, energy_mean, energy_std, d_mel, d_energy, d_mag};
        const double tile_frames = 64.0 * (double)g.tiles.size();
        KScope ks(h, "stft_mel", 2.0 * 3.0 * tile_frames * fc.n_fft * 2.0 * n_bins + 2.0 * tile_frames * n_bins * fc.n_mels,
                  (double)in.bytes + (double)total_frames * (fc.n_mels + 1) * 4.0);
        if (launch_stft_mel(p, h->stream)) return fail(h, "ev_features: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    if (call_end(h)) return -1;
    h->feat.mel_lens.swap(g.lens); h->feat.mel_offs.swap(g.offs);
    h->feat.mag = d_mag; h->feat.mag_elems = keep ? total_frames * n_bins : 0;
    reset_result(out);
    out->batch = B; out->total_frames = total_frames; out->mel = d_mel; out->energy = d_energy;
    out->mel_lens = h->feat.mel_lens.data(); out->mel_offsets = h->feat.mel_offs.data();
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
    if (check_struct_size(h, "ev_pitch", "out->struct_size", out->struct_size, "ev_pitch_result", sizeof(ev_pitch_result))) return -1;
    ev_pitch_config pc;
    ev_default_pitch_config(&pc);
    if (cfg) {
        if (check_struct_size(h, "ev_pitch", "cfg->struct_size", cfg->struct_size, "ev_pitch_config", sizeof(ev_pitch_config))) return -1;
        pc = *cfg;
    }
    int tau_min = 0, tau_max = 0;
    if (pitch_check_config(h, "ev_pitch", pc, &tau_min, &tau_max)) return -1;
    if ((size_t)B > PIN_MAX_B) return fail(h, "ev_pitch: at most %zu utterances per call", PIN_MAX_B);
    if (!std::isfinite(pitch_std) || !(pitch_std > 0.f)) return fail(h, "ev_pitch: pitch_std must be positive and finite");
    if (!std::isfinite(pitch_mean)) return fail(h, "ev_pitch: pitch_mean must be finite");
    FrameGrid g;
    const int bad = frame_grid_layout(B, wav_lens, 1, pc.hop, PITCH_TF, g);
    if (bad > 0) return fail(h, "ev_pitch: wav_lens[%d] = %lld < 1", bad - 1, (long long)wav_lens[bad - 1]);
    if (bad < 0) return fail(h, "ev_pitch: utterance %d has %lld frames > EV_ALIGN_MAX_FRAMES %d", -bad - 1, (long long)(wav_lens[-bad - 1] / pc.hop + 1), EV_ALIGN_MAX_FRAMES);
    const int64_t total_frames = g.offs[B], total_samples = g.seqs[B - 1].wav_off + g.seqs[B - 1].len;
    WavIn in(wav, total_samples, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    StftSeq* d_seqs = nullptr; StftTile* d_tiles = nullptr; float *d_pitch = nullptr, *d_f0 = nullptr, *d_ap = nullptr;
    if (arena_plan(h, ARENA_PITCH, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_seqs = ap.arr<StftSeq>(B); d_tiles = ap.arr<StftTile>(g.tiles.size());
        d_pitch = ap.arr<float>((size_t)total_frames); d_f0 = ap.arr<float>((size_t)total_frames); d_ap = ap.arr<float>((size_t)total_frames);
    })) return -1;
    if (in.copy(h) || upload(h, d_seqs, g.seqs) || upload(h, d_tiles, g.tiles)) return -1;
    region_begin(h, "total");
    {
        PitchParams p = pitch_params(pc, tau_min, tau_max);
        p.wav = in.ptr(); p.wav_is_i16 = wav_is_i16 != 0; p.seqs = d_seqs; p.tiles = d_tiles; p.n_tiles = (int)g.tiles.size();
        p.f0 = d_f0; p.ap = d_ap; p.tau = nullptr;
        KScope ks(h, "pitch_yin", 3.0 * (double)total_frames * (tau_max + 2.0) * pc.win, (double)in.bytes + (double)total_frames * 8.0);
        if (launch_pitch_yin(p, h->stream)) return fail(h, "ev_pitch: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {
        KScope ks(h, "pitch_fill", 8.0 * (double)total_frames, (double)total_frames * 8.0);
        launch_pitch_fill(d_f0, d_seqs, B, pitch_mean, pitch_std, d_pitch, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    if (call_end(h)) return -1;
    h->pitch.mel_lens.swap(g.lens); h->pitch.mel_offs.swap(g.offs);
    reset_result(out);
    out->batch = B; out->total_frames = total_frames; out->pitch = d_pitch; out->f0_hz = d_f0; out->aperiodicity = d_ap;
    out->mel_lens = h->pitch.mel_lens.data(); out->mel_offsets = h->pitch.mel_offs.data();
    return 0;
}

// ------------------------------------------------------------------- sample-rate conversion and trimming (include/evhip.h: ev_resample)
static_assert(EV_RESAMPLE_TILE == RS_TM, "include/evhip.h states the tile of ev_resample.hip");
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

// the phase-major table, packed on the host and uploaded into a fresh allocation; nothing half-built is left behind
static int resample_upload_table(int up, int half, const std::vector<float>& taps, DevMem& tab) {
    std::vector<float> ht(resample_table_floats(up, half));
    resample_pack_table(up, half, taps.data(), ht.data());
    return dev_upload(tab, ht) == hipSuccess ? 0 : -1;
}

int ev_resample_setup(ev_handle* h, const ev_resample_config* cfg) {
    if (!h) return -1;
    if (!cfg) return fail(h, "ev_resample_setup: null config");
    if (check_struct_size(h, "ev_resample_setup", "struct_size", cfg->struct_size, "ev_resample_config", sizeof(ev_resample_config))) return -1;
    int up = 0, down = 0, half = 0;
    std::vector<float> taps;
    if (resample_check_config(h, "ev_resample_setup", *cfg, &up, &down, &half, taps)) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    DevMem tab;
    if (resample_upload_table(up, half, taps, tab)) return fail(h, "ev_resample_setup: uploading the tap table failed");
    h->rs.tab = std::move(tab); h->rs.tab_floats = resample_table_floats(up, half); h->rs.up = up; h->rs.down = down; h->rs.half = half;
    h->rs.cfg = *cfg; h->rs.cfg.taps = nullptr;
    h->rs.ready = true;
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
    if (check_struct_size(h, "ev_resample", "out->struct_size", out->struct_size, "ev_resample_result", sizeof(ev_resample_result))) return -1;
    if (!h->rs.ready) return fail(h, "ev_resample: ev_resample_setup has not been called");
    if (B < 1 || B > 65535) return fail(h, "ev_resample: B %d outside [1, 65535]", B);
    const ev_resample_config& rc = h->rs.cfg;
    const int up = h->rs.up, down = h->rs.down, half = h->rs.half, pad = rc.trim_pad;
    const bool trim = rc.trim_frac > 0.f;
    std::vector<ResampleSeq> seqs; std::vector<ResampleTile> tiles;
    const int bad = resample_layout(B, wav_lens, up, down, trim ? 2 * (int64_t)pad : 0, seqs, tiles);
    if (bad > 0) return fail(h, "ev_resample: wav_lens[%d] = %lld < 1", bad - 1, (long long)wav_lens[bad - 1]);
    if (bad < 0) return fail(h, "ev_resample: utterance %d (%lld samples) gives more than EV_ALIGN_MAX_FRAMES * 256 = %lld output samples", -bad - 1,
                             (long long)wav_lens[-bad - 1], (long long)RS_MAX_OUT);
    const int64_t total_in = seqs[B - 1].in_off + seqs[B - 1].len, total_n = seqs[B - 1].out_off + seqs[B - 1].n;
    const bool keep = h->cfg.keep_stages != 0;
    WavIn in(wav, total_in, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    h->rs.raw = nullptr;
    ResampleSeq* d_seqs = nullptr; ResampleTile* d_tiles = nullptr; TrimSeq* d_ts = nullptr; int64_t* d_cuts = nullptr;
    float *d_y = nullptr, *d_out = nullptr;
    if (arena_plan(h, ARENA_RESAMPLE, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_seqs = ap.arr<ResampleSeq>(B); d_tiles = ap.arr<ResampleTile>(tiles.size());
        d_y = ap.arr<float>((size_t)total_n);
        if (trim) { d_ts = ap.arr<TrimSeq>(B); d_cuts = ap.arr<int64_t>(2 * (size_t)B); d_out = ap.arr<float>((size_t)total_n + 2 * (size_t)pad * B); }
    })) return -1;
    if (in.copy(h) || upload(h, d_seqs, seqs) || upload(h, d_tiles, tiles)) return -1;
    std::vector<int64_t> lens((size_t)B), offs((size_t)B + 1), start((size_t)B), end((size_t)B);
    region_begin(h, "total");
    {
        const bool copy = up == 1 && down == 1;
        KScope ks(h, copy ? "resample_copy" : "resample_poly", copy ? 0.0 : 2.0 * (double)total_n * (2.0 * half / up + 1.0), (double)in.bytes + (double)total_n * 4.0);
        if (resample_launch(in.ptr(), wav_is_i16 != 0, up, down, half, h->rs.tab.as<float>(), d_seqs, d_tiles, (int)tiles.size(), total_in, d_y, h->stream))
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
        if (upload(h, d_ts, ts)) return -1;
        {
            KScope ks(h, "trim_gather", 0.0, 2.0 * (double)offs[B] * 4.0);
            launch_trim_gather(d_y, d_ts, B, longest, pad, d_out, h->stream);
        }
        HIPCHK(h, hipGetLastError());
    } else {
        for (int b = 0; b < B; ++b) { lens[b] = seqs[b].n; offs[b] = seqs[b].out_off; start[b] = 0; end[b] = seqs[b].n; }
        offs[B] = total_n;
    }
    if (call_end(h)) return -1;
    h->rs.lens = lens; h->rs.offs = offs; h->rs.start = start; h->rs.end = end;
    h->rs.raw = keep ? d_y : nullptr; h->rs.raw_elems = keep ? total_n : 0;
    reset_result(out);
    out->batch = B; out->total_samples = offs[B]; out->wav = trim ? d_out : d_y;
    out->wav_lens = h->rs.lens.data(); out->wav_offsets = h->rs.offs.data(); out->trim_start = h->rs.start.data(); out->trim_end = h->rs.end.data();
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
    if (check_struct_size(h, who, "cfg->struct_size", c->struct_size, "ev_stitch_config", sizeof(ev_stitch_config))) return -1;
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
    if (check_struct_size(h, "ev_stitch", "out->struct_size", out->struct_size, "ev_stitch_result", sizeof(ev_stitch_result))) return -1;
    ev_stitch_config dflt;
    if (!cfg) { ev_default_stitch_config(&dflt); cfg = &dflt; }
    const int D = stitch_check(h, "ev_stitch", S, seg_doc, pause_after, cfg);
    if (D < 0) return -1;
    const ev_stitch_config c = *cfg;
    const bool trim = c.trim_frac > 0.f || c.trim_abs > 0.f, i16 = c.want_i16 != 0;
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
    for (auto& sg : segs) sg.off -= lo_off;      // the call reads the samples lo_off .. hi_end, and a host's are copied
    WavIn in(wav + lo_off, hi_end - lo_off, 0, flags);
    int64_t cap_out = 0, cap_tiles = 0;
    for (int d = 0; d < D; ++d) { cap_out += bound[(size_t)d]; cap_tiles += (bound[(size_t)d] + ST_TILE - 1) / ST_TILE; }
    if (call_begin(h)) return -1;
    StitchSeg* d_segs = nullptr; float *d_part = nullptr, *d_peak = nullptr; int64_t* d_cuts = nullptr;
    StitchMixSeg* d_ms = nullptr; StitchDoc* d_docs = nullptr; StitchTile* d_tiles = nullptr; float* d_out = nullptr; int16_t* d_i16 = nullptr;
    if (arena_plan(h, ARENA_STITCH, [&](ArenaPlan& ap) {
        in.plan(ap);
        if (trim) { d_segs = ap.arr<StitchSeg>(S); d_part = ap.arr<float>((size_t)n_part); d_peak = ap.arr<float>(S); d_cuts = ap.arr<int64_t>(2 * (size_t)S); }
        d_ms = ap.arr<StitchMixSeg>(S); d_docs = ap.arr<StitchDoc>(D); d_tiles = ap.arr<StitchTile>((size_t)cap_tiles);
        d_out = ap.arr<float>((size_t)cap_out);
        if (i16) d_i16 = ap.arr<int16_t>((size_t)cap_out);
    })) return -1;
    if (!h->stitch.tab) HIPCHK(h, h->stitch.tab.alloc((size_t)EV_STITCH_MAX_FADE * sizeof(float)));
    h->stitch.tab_host.resize((size_t)c.fade);
    (void)ev_stitch_ramp(c.fade, h->stitch.tab_host.data());
    h->stitch.F = c.fade;
    if (c.fade > 0) HIPCHK(h, hipMemcpyAsync(h->stitch.tab.get(), h->stitch.tab_host.data(), (size_t)c.fade * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (in.copy(h)) return -1;
    const float* x = static_cast<const float*>(in.ptr());
    std::vector<int64_t> a((size_t)S, 0), b((size_t)S), n((size_t)S), src((size_t)S);
    std::vector<float> peak((size_t)S, 0.f);
    for (int s = 0; s < S; ++s) b[(size_t)s] = seg_lens[s];
    region_begin(h, "total");
    if (trim) {
        if (upload(h, d_segs, segs)) return -1;
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
    if (upload(h, d_ms, ms) || upload(h, d_docs, docs) || (!tiles.empty() && upload(h, d_tiles, tiles))) return -1;
    {
        KScope ks(h, "stitch_mix", 0.0, (double)total * (i16 ? 10.0 : 8.0));
        if (launch_stitch_mix(x, d_ms, d_docs, d_tiles, (int64_t)tiles.size(), h->stitch.tab.as<float>(), c.fade, d_out, i16 ? d_i16 : nullptr, h->stream))
            return fail(h, "ev_stitch: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    if (call_end(h)) return -1;
    h->stitch.doc_lens = doc_lens; h->stitch.doc_offs = offs; h->stitch.pos = pos; h->stitch.start = a; h->stitch.end = b; h->stitch.peak = peak;
    reset_result(out);
    out->batch_docs = D; out->batch_segs = S; out->total_samples = total; out->wav = d_out; out->wav_i16 = i16 ? d_i16 : nullptr;
    out->doc_lens = h->stitch.doc_lens.data(); out->doc_offsets = h->stitch.doc_offs.data(); out->seg_pos = h->stitch.pos.data();
    out->seg_start = h->stitch.start.data(); out->seg_end = h->stitch.end.data(); out->seg_peak = h->stitch.peak.data();
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
    if (check_struct_size(h, "ev_compare", "out->struct_size", out->struct_size, "ev_compare_result", sizeof(ev_compare_result))) return -1;
    if (B < 1 || B > 65535) return fail(h, "ev_compare: B = %d outside [1, 65535]", B);
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
    WavIn ia(a, total, 0, flags), ib(b, total, 0, flags);
    if (call_begin(h)) return -1;
    CompareChunk* d_chunks = nullptr; int64_t* d_coffs = nullptr; double *d_sums = nullptr, *d_maxd = nullptr;
    int32_t *d_argd = nullptr, *d_nonf = nullptr; float* d_peak = nullptr; CompareSeg* d_seg = nullptr;
    if (arena_plan(h, ARENA_COMPARE, [&](ArenaPlan& ap) {
        ia.plan(ap); ib.plan(ap);
        d_chunks = ap.arr<CompareChunk>((size_t)NC); d_coffs = ap.arr<int64_t>((size_t)B + 1);
        d_sums = ap.arr<double>(4 * (size_t)NC); d_maxd = ap.arr<double>((size_t)NC);
        d_argd = ap.arr<int32_t>((size_t)NC); d_nonf = ap.arr<int32_t>((size_t)NC); d_peak = ap.arr<float>((size_t)NC);
        d_seg = ap.arr<CompareSeg>((size_t)B);
    })) return -1;
    if (ia.copy(h) || ib.copy(h) || upload(h, d_chunks, chunks) || upload(h, d_coffs, coffs)) return -1;
    region_begin(h, "total");
    {
        KScope ks(h, "compare_chunks", 8.0 * (double)total, 8.0 * (double)total + 64.0 * (double)NC);
        if (launch_compare_chunks(static_cast<const float*>(ia.ptr()), static_cast<const float*>(ib.ptr()), d_chunks, NC, d_sums, d_maxd, d_argd, d_peak, d_nonf, h->stream))
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
    h->cmp.d.resize(nb); h->cmp.d2.resize(nb); h->cmp.y.resize(nb); h->cmp.y2.resize(nb); h->cmp.rel.resize(nb); h->cmp.rel_ac.resize(nb);
    h->cmp.max_d.resize(nb); h->cmp.peak_y.resize(nb); h->cmp.arg.resize(nb); h->cmp.nonf.resize(nb);
    for (size_t s = 0; s < nb; ++s) {
        const CompareSeg& g = seg[s];
        const double n = (double)lens[s], num = sqrt(g.sum[1]);
        const double var = g.sum[3] - (g.sum[2] * g.sum[2]) / n;      // the quotient sits between the product and the difference: nothing to fuse
        h->cmp.d[s] = g.sum[0]; h->cmp.d2[s] = g.sum[1]; h->cmp.y[s] = g.sum[2]; h->cmp.y2[s] = g.sum[3];
        h->cmp.rel[s] = num / sqrt(std::max(g.sum[3], EV_COMPARE_FLOOR));
        h->cmp.rel_ac[s] = num / sqrt(std::max(var, EV_COMPARE_FLOOR));
        h->cmp.max_d[s] = (float)g.max_d; h->cmp.peak_y[s] = g.peak_y; h->cmp.arg[s] = g.arg; h->cmp.nonf[s] = g.nonfinite;
    }
    h->cmp.chunk_d2.swap(cd2); h->cmp.chunk_y2.swap(cy2); h->cmp.chunk_offs.swap(coffs);
    reset_result(out);
    out->batch = B; out->total = total;
    out->sum_d = h->cmp.d.data(); out->sum_d2 = h->cmp.d2.data(); out->sum_y = h->cmp.y.data(); out->sum_y2 = h->cmp.y2.data();
    out->rel_l2 = h->cmp.rel.data(); out->rel_l2_ac = h->cmp.rel_ac.data(); out->max_abs_d = h->cmp.max_d.data(); out->argmax_d = h->cmp.arg.data();
    out->peak_y = h->cmp.peak_y.data(); out->nonfinite = h->cmp.nonf.data();
    out->chunk_d2 = h->cmp.chunk_d2.data(); out->chunk_y2 = h->cmp.chunk_y2.data(); out->chunk_offsets = h->cmp.chunk_offs.data();
    return 0;
}

// ------------------------------------------------------------------- FLAC encoding (include/evhip.h: ev_flac)
void ev_default_flac_config(ev_flac_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c; c->sample_rate = 16000; c->block_size = 4096; c->max_fixed_order = 4; c->max_partition_order = 5; c->convert = EV_FLAC_WRAP;
}

int64_t ev_flac_bound(int64_t n, int block_size) {
    if (n < 1 || n > EV_FLAC_MAX_SAMPLES || flac_block_code(block_size) < 0) return -1;
    return flac_bound(n, block_size);
}

// the encoder's constants from a config flac_check_config has accepted; the caller adds the pointers
static FlacParams flac_params(const ev_flac_config& c, int sr_code, int bs_code) {
    FlacParams fp{};
    fp.convert = c.convert; fp.block_size = c.block_size; fp.bs_code = bs_code; fp.sr_code = sr_code;
    fp.max_fixed_order = c.max_fixed_order; fp.max_partition_order = c.max_partition_order; fp.stride = 2 * c.block_size + 24;
    return fp;
}

void ev_default_flac_ext(ev_flac_ext* e) {
    memset(e, 0, sizeof *e);
    e->struct_size = sizeof *e; e->max_lpc_order = 8; e->qlp_precision = 12; e->md5 = 1;
}

// ev_flac (ext NULL) and ev_flac_lpc; who names the entry point in messages
static int flac_run(ev_handle* h, const char* who, int B, const void* pcm, int pcm_is_i16, const int64_t* lens, const ev_flac_config* cfg, const ev_flac_ext* ext,
                    uint32_t flags, ev_flac_result* out) {
    if (!h) return -1;
    if (!pcm) return fail(h, "%s: pcm is NULL", who);
    if (!lens) return fail(h, "%s: lens is NULL", who);
    if (!out) return fail(h, "%s: out is NULL", who);
    if (check_struct_size(h, who, "out->struct_size", out->struct_size, "ev_flac_result", sizeof(ev_flac_result))) return -1;
    ev_flac_config dflt;
    if (!cfg) { ev_default_flac_config(&dflt); cfg = &dflt; }
    if (check_struct_size(h, who, "cfg->struct_size", cfg->struct_size, "ev_flac_config", sizeof(ev_flac_config))) return -1;
    const ev_flac_config c = *cfg;
    int sr_code = 0, bs_code = 0;
    switch (flac_check_config(c, &sr_code, &bs_code)) {
    case FLAC_OK: break;
    case FLAC_BAD_RATE: return fail(h, "%s: sample_rate = %d is not one of 8000, 16000, 22050, 24000, 32000, 44100, 48000", who, c.sample_rate);
    case FLAC_BAD_BLOCK: return fail(h, "%s: block_size = %d is not one of 256, 512, 1024, 2048, 4096", who, c.block_size);
    case FLAC_BAD_FIXED_ORDER: return fail(h, "%s: max_fixed_order = %d outside [0, 4]", who, c.max_fixed_order);
    case FLAC_BAD_PARTITION_ORDER: return fail(h, "%s: max_partition_order = %d outside [0, 6]", who, c.max_partition_order);
    case FLAC_BAD_CONVERT: return fail(h, "%s: convert = %d is neither EV_FLAC_WRAP nor EV_FLAC_CLAMP", who, c.convert);
    }
    int lpc_order = 0, lpc_q = 12; bool md5 = false;
    if (ext) {
        if (check_struct_size(h, who, "ext->struct_size", ext->struct_size, "ev_flac_ext", sizeof(ev_flac_ext))) return -1;
        if (ext->max_lpc_order < 0 || ext->max_lpc_order > FLAC_LPC_MAX_ORDER) return fail(h, "%s: ext->max_lpc_order = %d outside [0, %d]", who, ext->max_lpc_order, FLAC_LPC_MAX_ORDER);
        if (ext->qlp_precision < 5 || ext->qlp_precision > 15) return fail(h, "%s: ext->qlp_precision = %d outside [5, 15]", who, ext->qlp_precision);
        if (ext->md5 != 0 && ext->md5 != 1) return fail(h, "%s: ext->md5 = %d is neither 0 nor 1", who, ext->md5);
        for (int i = 0; i < 4; ++i) if (ext->reserved[i] != 0) return fail(h, "%s: ext->reserved[%d] = %d is not 0", who, i, ext->reserved[i]);
        lpc_order = ext->max_lpc_order; lpc_q = ext->qlp_precision; md5 = ext->md5 != 0;
    }
    if (B < 1 || B > 65535) return fail(h, "%s: B = %d outside [1, 65535]", who, B);
    const bool i16 = pcm_is_i16 != 0;
    const int N = c.block_size, stride = 2 * N + 24;
    FlacPlan plan;
    int at = 0;
    switch (flac_plan(B, lens, N, plan, &at)) {
    case LEN_OK: break;
    case LEN_SHORT: return fail(h, "%s: lens[%d] = %lld < 1", who, at, (long long)lens[at]);
    case LEN_LONG: return fail(h, "%s: lens[%d] = %lld > EV_FLAC_MAX_SAMPLES = %d", who, at, (long long)lens[at], EV_FLAC_MAX_SAMPLES);
    case LEN_COUNT: return fail(h, "%s: lens[%d] = %lld: more than %d frames in one call", who, at, (long long)lens[at], INT_MAX);
    }
    const int64_t total = plan.total, NF = (int64_t)plan.frames.size(), cap = plan.cap;
    WavIn in(pcm, total, pcm_is_i16, flags);
    if (call_begin(h)) return -1;
    FlacFrame* d_frames = nullptr; int32_t* d_sizes = nullptr; uint32_t* d_desc = nullptr; uint8_t *d_scratch = nullptr, *d_hdr = nullptr, *d_bytes = nullptr;
    int64_t* d_foffs = nullptr; FlacMd5Seg* d_segs = nullptr; uint32_t* d_md5 = nullptr;
    if (arena_plan(h, ARENA_FLAC, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_frames = ap.arr<FlacFrame>((size_t)NF); d_sizes = ap.arr<int32_t>((size_t)NF); d_desc = ap.arr<uint32_t>((size_t)NF);
        d_foffs = ap.arr<int64_t>((size_t)NF); d_hdr = ap.arr<uint8_t>((size_t)B * FLAC_HEADER_STRIDE);
        d_scratch = ap.arr<uint8_t>((size_t)NF * (size_t)stride + 16); d_bytes = ap.arr<uint8_t>((size_t)cap);
        if (md5) { d_segs = ap.arr<FlacMd5Seg>((size_t)B); d_md5 = ap.arr<uint32_t>(4 * (size_t)B); }
    })) return -1;
    if (in.copy(h) || upload(h, d_frames, plan.frames)) return -1;
    FlacParams fp = flac_params(c, sr_code, bs_code);
    fp.pcm = in.ptr(); fp.pcm_is_i16 = i16; fp.frames = d_frames; fp.scratch = d_scratch; fp.sizes = d_sizes; fp.desc = d_desc;
    region_begin(h, "total");
    {
        KScope ks(h, "flac_encode", 0.0, (double)in.bytes + (double)NF * (double)stride);
        if (lpc_order > 0 ? launch_flac_encode_lpc(fp, FlacLpc{lpc_order, lpc_q}, NF, h->stream) : launch_flac_encode(fp, NF, h->stream))
            return fail(h, "%s: the kernel does not build this shape", who);
    }
    HIPCHK(h, hipGetLastError());
    std::vector<int32_t> sizes((size_t)NF); std::vector<uint32_t> desc((size_t)NF), digest(md5 ? 4 * (size_t)B : 0);
    if (md5) {      // one chain per segment, before the synchronisation the frame sizes need anyway
        std::vector<FlacMd5Seg> segs((size_t)B);
        int64_t off = 0;
        for (int b = 0; b < B; ++b) { segs[(size_t)b] = FlacMd5Seg{off, lens[b]}; off += lens[b]; }
        if (upload(h, d_segs, segs)) return -1;
        {
            KScope ks(h, "flac_md5", 0.0, (double)in.bytes);
            launch_flac_md5(fp, d_segs, B, d_md5, h->stream);
        }
        HIPCHK(h, hipGetLastError());
        HIPCHK(h, hipMemcpyAsync(digest.data(), d_md5, digest.size() * sizeof(uint32_t), hipMemcpyDeviceToHost, h->stream));
    }
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
        for (int64_t i = 0; i < plan.stream_frames[(size_t)b]; ++i, ++f) {
            const int32_t sz = sizes[(size_t)f];
            if (sz < 1 || sz > 2 * N + 15) return fail(h, "%s: frame %lld of segment %d reports %d bytes", who, (long long)i, b, sz);
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
        for (int i = 0; i < 8; ++i) p[18 + i] = (uint8_t)(v >> (56 - 8 * i));      // p[26 .. 42): the MD5, or zero
        if (md5) for (int i = 0; i < 16; ++i) p[26 + i] = (uint8_t)(digest[4 * (size_t)b + (size_t)(i >> 2)] >> (8 * (i & 3)));
    }
    soffs[(size_t)B] = pos; foffs[(size_t)NF] = pos;
    if (pos > cap) return fail(h, "%s: the streams outgrew their bound", who);
    HIPCHK(h, hipMemcpyAsync(d_foffs, foffs.data(), (size_t)NF * sizeof(int64_t), hipMemcpyHostToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_hdr, hdr.data(), hdr.size(), hipMemcpyHostToDevice, h->stream));
    {
        KScope ks(h, "flac_gather", 0.0, 2.0 * (double)pos);
        launch_flac_gather(d_scratch, stride, d_frames, NF, d_sizes, d_foffs, d_hdr, d_bytes, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    if (call_end(h)) return -1;
    h->flac.stream_offs.swap(soffs); h->flac.stream_frames.swap(plan.stream_frames); h->flac.frame_offs.swap(foffs); h->flac.kind.swap(kind); h->flac.porder.swap(porder);
    reset_result(out);
    out->batch = B; out->total_bytes = pos; out->total_frames = NF; out->bytes = d_bytes;
    out->stream_offsets = h->flac.stream_offs.data(); out->stream_frames = h->flac.stream_frames.data(); out->frame_offsets = h->flac.frame_offs.data();
    out->frame_kind = h->flac.kind.data(); out->frame_porder = h->flac.porder.data();
    return 0;
}

int ev_flac(ev_handle* h, int B, const void* pcm, int pcm_is_i16, const int64_t* lens, const ev_flac_config* cfg, uint32_t flags, ev_flac_result* out) {
    return flac_run(h, "ev_flac", B, pcm, pcm_is_i16, lens, cfg, nullptr, flags, out);
}

int ev_flac_lpc(ev_handle* h, int B, const void* pcm, int pcm_is_i16, const int64_t* lens, const ev_flac_config* cfg, const ev_flac_ext* ext, uint32_t flags,
                ev_flac_result* out) {
    return flac_run(h, "ev_flac_lpc", B, pcm, pcm_is_i16, lens, cfg, ext, flags, out);
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
    if (check_struct_size(h, "ev_loudness", "out->struct_size", out->struct_size, "ev_loudness_result", sizeof(ev_loudness_result))) return -1;
    ev_loudness_config dflt;
    if (!cfg) { ev_default_loudness_config(&dflt); cfg = &dflt; }
    if (check_struct_size(h, "ev_loudness", "cfg->struct_size", cfg->struct_size, "ev_loudness_config", sizeof(ev_loudness_config))) return -1;
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
    const bool in16 = wav_is_i16 != 0, i16 = c.want_i16 != 0 && !measure_only;
    const int64_t step = c.sample_rate / 10, block = 4 * step;
    LoudPlan plan;
    int at = 0;
    switch (loudness_plan(B, lens, step, plan, &at)) {
    case LEN_OK: break;
    case LEN_SHORT: return fail(h, "ev_loudness: lens[%d] = %lld < 1", at, (long long)lens[at]);
    case LEN_LONG: return fail(h, "ev_loudness: lens[%d] = %lld > EV_LOUDNESS_MAX_SAMPLES = %d", at, (long long)lens[at], EV_LOUDNESS_MAX_SAMPLES);
    case LEN_COUNT: return fail(h, "ev_loudness: lens[%d] = %lld: more than %d tiles in one call", at, (long long)lens[at], INT_MAX);
    }
    const std::vector<LoudSeg>& segs = plan.segs;
    const int64_t total = plan.total, NT = (int64_t)plan.tiles.size(), NB = plan.n_blocks;
    LoudCoef lc;
    loudness_coef(coef, &lc);
    WavIn in(wav, total, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    LoudTile* d_tiles = nullptr; LoudSeg* d_segs = nullptr; LoudCoef* d_coef = nullptr; double *d_ends = nullptr, *d_init = nullptr;
    LoudTileOut* d_outs = nullptr; int64_t* d_offs = nullptr; float *d_gain = nullptr, *d_wav = nullptr; int16_t* d_i16 = nullptr;
    if (arena_plan(h, ARENA_LOUDNESS, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_tiles = ap.arr<LoudTile>((size_t)NT); d_segs = ap.arr<LoudSeg>((size_t)B); d_coef = ap.arr<LoudCoef>(1);
        d_ends = ap.arr<double>(4 * (size_t)NT); d_init = ap.arr<double>(4 * (size_t)NT); d_outs = ap.arr<LoudTileOut>((size_t)NT);
        d_offs = ap.arr<int64_t>((size_t)B + 1); d_gain = ap.arr<float>((size_t)B);
        if (!measure_only) d_wav = ap.arr<float>((size_t)total);
        if (i16) d_i16 = ap.arr<int16_t>((size_t)total);
    })) return -1;
    if (in.copy(h) || upload(h, d_tiles, plan.tiles) || upload(h, d_segs, plan.segs)) return -1;
    HIPCHK(h, hipMemcpyAsync(d_coef, &lc, sizeof lc, hipMemcpyHostToDevice, h->stream));
    const void* x = in.ptr();
    region_begin(h, "total");
    {
        KScope ks(h, "loudness_measure", 60.0 * (double)total, 2.0 * (double)in.bytes + (double)NT * (64.0 + sizeof(LoudTileOut)));
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
        if (upload(h, d_offs, plan.offs) || upload(h, d_gain, gain)) return -1;
        {
            KScope ks(h, "loudness_gain", (double)total, (double)in.bytes + (double)total * (i16 ? 6.0 : 4.0));
            if (launch_loudness_gain(x, in16, d_offs, B, d_gain, total, d_wav, i16 ? d_i16 : nullptr, h->stream))
                return fail(h, "ev_loudness: the kernels do not build this shape");
        }
        HIPCHK(h, hipGetLastError());
    }
    if (call_end(h)) return -1;
    h->loud.loud.swap(loud); h->loud.rel.swap(rel); h->loud.ms.swap(ms); h->loud.gain.swap(gain); h->loud.peak.swap(peak); h->loud.flags.swap(fl); h->loud.state.swap(state);
    h->loud.nonf.swap(nonf); h->loud.boffs.swap(boffs);
    reset_result(out);
    out->batch = B; out->total = total; out->wav = measure_only ? nullptr : d_wav; out->wav_i16 = i16 ? d_i16 : nullptr;
    out->loudness = h->loud.loud.data(); out->rel_threshold = h->loud.rel.data(); out->gain = h->loud.gain.data(); out->peak = h->loud.peak.data();
    out->flags = h->loud.flags.data(); out->nonfinite = h->loud.nonf.data(); out->block_offsets = h->loud.boffs.data(); out->block_ms = h->loud.ms.data();
    out->block_state = h->loud.state.data();
    return 0;
}

// ------------------------------------------------------------------- true-peak metering and limiting (include/evhip.h: ev_limit)
static_assert(EV_LIMIT_TILE == LIMIT_TILE && EV_LIMIT_MAX_LOOKAHEAD == LIMIT_MAX_LOOKAHEAD && EV_LIMIT_MAX_HOLD == LIMIT_MAX_HOLD && EV_LIMIT_MAX_LDS == LIMIT_MAX_LDS,
              "include/evhip.h states the tile and the limits of ev_limit.hip");
static_assert(EV_LIMIT_LDS_BYTES(EV_LIMIT_MAX_LOOKAHEAD, EV_LIMIT_MAX_HOLD) == limit_apply_lds_bytes(LIMIT_MAX_LOOKAHEAD, LIMIT_MAX_HOLD) &&
              EV_LIMIT_LDS_BYTES(80, 800) == limit_apply_lds_bytes(80, 800), "include/evhip.h states the LDS formula of ev_limit.hip");
void ev_default_limit_config(ev_limit_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c; c->sample_rate = 16000; c->ceiling = (float)pow(10.0, -1.0 / 20.0); c->lookahead = 80; c->hold = 800; c->want_i16 = 0;
}

int ev_limit_design(int L, float* w) {
    if (L < 0 || L > EV_LIMIT_MAX_LOOKAHEAD || !w) return -1;
    const double pi = 3.14159265358979323846;
    std::vector<double> g((size_t)L + 1);
    double sum = 0.0;
    for (int j = 0; j <= L; ++j) { g[(size_t)j] = 1.0 - cos(2.0 * pi * (double)(j + 1) / (double)(L + 2)); sum += g[(size_t)j]; }
    for (int j = 0; j <= L; ++j) w[j] = (float)(g[(size_t)j] / sum);
    for (;;) {      // the fp32 taps must not sum above one: s <= r rests on it
        double acc = 0.0;
        int top = 0;
        for (int j = 0; j <= L; ++j) { acc += (double)w[j]; if (w[j] > w[top]) top = j; }
        if (!(acc > 1.0)) break;
        w[top] = nextafterf(w[top], 0.0f);
    }
    return L + 1;
}

// the interpolator's phase table and the window as the kernels read them
static int limit_tables(int L, double tab[LIMIT_TAB], std::vector<double>& win) {
    float h[LIMIT_TAPS];
    if (ev_resample_design(1, 4, LIMIT_HALO, 0.945, 9.0, h, LIMIT_TAPS) != (LIMIT_TAPS - 1) / 2) return -1;
    limit_pack_taps(h, tab);
    std::vector<float> w((size_t)L + 1);
    if (ev_limit_design(L, w.data()) != L + 1) return -1;
    win.assign(w.begin(), w.end());
    return 0;
}
// the first field of a config that is out of range, in the order include/evhip.h lists them
enum LimitBad { LIMIT_OK = 0, LIMIT_BAD_RATE, LIMIT_BAD_CEILING, LIMIT_BAD_LOOKAHEAD, LIMIT_BAD_HOLD };
static LimitBad limit_check_config(const ev_limit_config& c) {
    if (flac_rate_code(c.sample_rate) < 0) return LIMIT_BAD_RATE;
    if (!(c.ceiling > 0.f && c.ceiling <= 1.f)) return LIMIT_BAD_CEILING;
    if (c.lookahead < 0 || c.lookahead > EV_LIMIT_MAX_LOOKAHEAD) return LIMIT_BAD_LOOKAHEAD;
    if (c.hold < 0 || c.hold > EV_LIMIT_MAX_HOLD) return LIMIT_BAD_HOLD;
    return LIMIT_OK;
}
static int limit_bad_gain(int B, const float* gains) {      // -1, or the first index of a gain that is negative, NaN or infinite
    if (gains) for (int b = 0; b < B; ++b) if (!(std::isfinite(gains[b]) && gains[b] >= 0.f)) return b;
    return -1;
}
// tile records -> segment records, in ascending tile order
static void limit_fold_peaks(const LimitPlan& plan, int B, const LimitPeakOut* t, float* sp, float* tp, int64_t* nf) {
    for (int b = 0; b < B; ++b) {
        float s = 0.f, p = 0.f; int64_t n = 0;
        for (int64_t i = plan.tile0[(size_t)b]; i < plan.tile0[(size_t)b + 1]; ++i) { s = std::max(s, t[i].sample_peak); p = std::max(p, t[i].true_peak); n += t[i].nonfinite; }
        sp[b] = s; tp[b] = p; if (nf) nf[b] = n;
    }
}
static void limit_fold_gains(const LimitPlan& plan, int B, const LimitApplyOut* t, float* mn, int64_t* limited) {
    for (int b = 0; b < B; ++b) {
        float m = 1.0f; int64_t n = 0;
        for (int64_t i = plan.tile0[(size_t)b]; i < plan.tile0[(size_t)b + 1]; ++i) { m = std::min(m, t[i].min_gain); n += t[i].limited; }
        mn[b] = m; limited[b] = n;
    }
}

int ev_limit(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const float* gains, const ev_limit_config* cfg, uint32_t flags,
             ev_limit_result* out) {
    if (!h) return -1;
    if (!wav) return fail(h, "ev_limit: wav is NULL");
    if (!lens) return fail(h, "ev_limit: lens is NULL");
    if (!out) return fail(h, "ev_limit: out is NULL");
    if (check_struct_size(h, "ev_limit", "out->struct_size", out->struct_size, "ev_limit_result", sizeof(ev_limit_result))) return -1;
    ev_limit_config dflt;
    if (!cfg) { ev_default_limit_config(&dflt); cfg = &dflt; }
    if (check_struct_size(h, "ev_limit", "cfg->struct_size", cfg->struct_size, "ev_limit_config", sizeof(ev_limit_config))) return -1;
    const ev_limit_config c = *cfg;
    switch (limit_check_config(c)) {
    case LIMIT_OK: break;
    case LIMIT_BAD_RATE: return fail(h, "ev_limit: sample_rate = %d is not one of 8000, 16000, 22050, 24000, 32000, 44100, 48000", c.sample_rate);
    case LIMIT_BAD_CEILING: return fail(h, "ev_limit: ceiling = %g outside (0, 1]", (double)c.ceiling);
    case LIMIT_BAD_LOOKAHEAD: return fail(h, "ev_limit: lookahead = %d outside [0, EV_LIMIT_MAX_LOOKAHEAD = %d]", c.lookahead, EV_LIMIT_MAX_LOOKAHEAD);
    case LIMIT_BAD_HOLD: return fail(h, "ev_limit: hold = %d outside [0, EV_LIMIT_MAX_HOLD = %d]", c.hold, EV_LIMIT_MAX_HOLD);
    }
    if (B < 1 || B > 65535) return fail(h, "ev_limit: B = %d outside [1, 65535]", B);
    LimitPlan plan;
    int at = 0;
    switch (limit_plan(B, lens, plan, &at)) {
    case LEN_OK: break;
    case LEN_SHORT: return fail(h, "ev_limit: lens[%d] = %lld < 1", at, (long long)lens[at]);
    case LEN_LONG: return fail(h, "ev_limit: lens[%d] = %lld > EV_LIMIT_MAX_SAMPLES = %d", at, (long long)lens[at], EV_LIMIT_MAX_SAMPLES);
    case LEN_COUNT: return fail(h, "ev_limit: lens[%d] = %lld: more than %d tiles in one call", at, (long long)lens[at], INT_MAX);
    }
    at = limit_bad_gain(B, gains);
    if (at >= 0) return fail(h, "ev_limit: gains[%d] = %g is not finite and >= 0", at, (double)gains[at]);
    const bool in16 = wav_is_i16 != 0, i16 = c.want_i16 != 0;
    const int L = c.lookahead, Hd = c.hold;
    const int64_t total = plan.total, NT = (int64_t)plan.tiles.size();
    double tab[LIMIT_TAB];
    std::vector<double> win;
    if (limit_tables(L, tab, win)) return fail(h, "ev_limit: the interpolator's design failed");
    WavIn in(wav, total, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    LimitTile* d_tiles = nullptr; double *d_tab = nullptr, *d_win = nullptr; float *d_gain = nullptr, *d_r = nullptr, *d_wav = nullptr;
    int16_t* d_i16 = nullptr; LimitPeakOut *d_pin = nullptr, *d_pout = nullptr; LimitApplyOut* d_app = nullptr;
    if (arena_plan(h, ARENA_LIMIT, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_tiles = ap.arr<LimitTile>((size_t)NT); d_tab = ap.arr<double>(LIMIT_TAB); d_win = ap.arr<double>((size_t)L + 1);
        if (gains) d_gain = ap.arr<float>((size_t)B);
        d_r = ap.arr<float>((size_t)total); d_wav = ap.arr<float>((size_t)total);
        if (i16) d_i16 = ap.arr<int16_t>((size_t)total);
        d_pin = ap.arr<LimitPeakOut>((size_t)NT); d_pout = ap.arr<LimitPeakOut>((size_t)NT); d_app = ap.arr<LimitApplyOut>((size_t)NT);
    })) return -1;
    if (in.copy(h) || upload(h, d_tiles, plan.tiles) || upload(h, d_win, win)) return -1;
    HIPCHK(h, hipMemcpyAsync(d_tab, tab, sizeof tab, hipMemcpyHostToDevice, h->stream));
    if (gains) HIPCHK(h, hipMemcpyAsync(d_gain, gains, (size_t)B * sizeof(float), hipMemcpyHostToDevice, h->stream));
    const void* x = in.ptr();
    const double meter_flops = 2.0 * LIMIT_TAB * (double)total, rec = (double)NT * sizeof(LimitPeakOut);
    region_begin(h, "total");
    {
        KScope ks(h, "limit_peak", meter_flops, (double)in.bytes + (double)total * 4.0 + rec);
        if (launch_limit_peak(x, in16, d_gain, d_tiles, NT, d_tab, c.ceiling, d_r, d_pin, h->stream)) return fail(h, "ev_limit: the kernels do not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {
        KScope ks(h, "limit_apply", 2.0 * (double)(L + 1) * (double)total, (double)in.bytes + (double)total * (8.0 + (i16 ? 2.0 : 0.0)) + (double)NT * sizeof(LimitApplyOut));
        if (launch_limit_apply(x, in16, d_gain, d_tiles, NT, d_r, d_win, L, Hd, d_wav, i16 ? d_i16 : nullptr, nullptr, d_app, h->stream))
            return fail(h, "ev_limit: the kernels do not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {
        KScope ks(h, "limit_measure", meter_flops, 4.0 * (double)total + rec);
        if (launch_limit_peak(d_wav, 0, nullptr, d_tiles, NT, d_tab, c.ceiling, nullptr, d_pout, h->stream)) return fail(h, "ev_limit: the kernels do not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    std::vector<LimitPeakOut> pin((size_t)NT), pout((size_t)NT); std::vector<LimitApplyOut> app((size_t)NT);
    HIPCHK(h, hipMemcpyAsync(pin.data(), d_pin, (size_t)NT * sizeof(LimitPeakOut), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(pout.data(), d_pout, (size_t)NT * sizeof(LimitPeakOut), hipMemcpyDeviceToHost, h->stream));
    HIPCHK(h, hipMemcpyAsync(app.data(), d_app, (size_t)NT * sizeof(LimitApplyOut), hipMemcpyDeviceToHost, h->stream));
    if (call_end(h)) return -1;
    std::vector<float> tp_in((size_t)B), sp_in((size_t)B), tp_out((size_t)B), sp_out((size_t)B), mn((size_t)B); std::vector<int64_t> limited((size_t)B), nonf((size_t)B);
    limit_fold_peaks(plan, B, pin.data(), sp_in.data(), tp_in.data(), nonf.data());
    limit_fold_peaks(plan, B, pout.data(), sp_out.data(), tp_out.data(), nullptr);
    limit_fold_gains(plan, B, app.data(), mn.data(), limited.data());
    h->lim.tp_in.swap(tp_in); h->lim.sp_in.swap(sp_in); h->lim.tp_out.swap(tp_out); h->lim.sp_out.swap(sp_out); h->lim.min_gain.swap(mn);
    h->lim.limited.swap(limited); h->lim.nonf.swap(nonf);
    reset_result(out);
    out->batch = B; out->total = total; out->wav = d_wav; out->wav_i16 = i16 ? d_i16 : nullptr;
    out->true_peak_in = h->lim.tp_in.data(); out->sample_peak_in = h->lim.sp_in.data(); out->true_peak_out = h->lim.tp_out.data();
    out->sample_peak_out = h->lim.sp_out.data(); out->min_gain = h->lim.min_gain.data(); out->limited = h->lim.limited.data(); out->nonfinite = h->lim.nonf.data();
    return 0;
}

// ------------------------------------------------------------------- response delivery (include/evhip.h: ev_deliver)
static_assert(EV_DELIVER_TILE == DL_TILE && EV_DELIVER_F32 == DL_F32 && EV_DELIVER_S16 == DL_S16 && EV_DELIVER_ULAW == DL_ULAW && EV_DELIVER_ALAW == DL_ALAW,
              "include/evhip.h states the tile and the encodings of ev_deliver.hip");
void ev_default_deliver_config(ev_deliver_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof(ev_deliver_config);
    c->sr_in = 16000; c->sr_out = 16000; c->encoding = EV_DELIVER_S16;
}

int ev_deliver_setup(ev_handle* h, const ev_deliver_config* cfg) {
    if (!h) return -1;
    if (!cfg) return fail(h, "ev_deliver_setup: null config");
    if (check_struct_size(h, "ev_deliver_setup", "struct_size", cfg->struct_size, "ev_deliver_config", sizeof(ev_deliver_config))) return -1;
    if (cfg->encoding < EV_DELIVER_F32 || cfg->encoding > EV_DELIVER_ALAW)
        return fail(h, "ev_deliver_setup: encoding = %d is not one of EV_DELIVER_F32, EV_DELIVER_S16, EV_DELIVER_ULAW, EV_DELIVER_ALAW", cfg->encoding);
    if (cfg->dither != 0 && cfg->dither != 1) return fail(h, "ev_deliver_setup: dither = %d is not 0 (none) or 1 (TPDF)", cfg->dither);
    if (cfg->dither && cfg->encoding == EV_DELIVER_F32) return fail(h, "ev_deliver_setup: dither = %d with encoding EV_DELIVER_F32: nothing is quantised", cfg->dither);
    ev_resample_config rc;      // the ratio and the taps: ev_resample's own checks and default design
    ev_default_resample_config(&rc);
    rc.sr_in = cfg->sr_in; rc.sr_out = cfg->sr_out; rc.taps = cfg->taps; rc.half_len = cfg->half_len;
    int up = 0, down = 0, half = 0;
    std::vector<float> taps;
    if (resample_check_config(h, "ev_deliver_setup", rc, &up, &down, &half, taps)) return -1;
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    DevMem tab;
    if (!(up == 1 && down == 1) && resample_upload_table(up, half, taps, tab)) return fail(h, "ev_deliver_setup: uploading the tap table failed");
    h->dlv.tab = std::move(tab); h->dlv.up = up; h->dlv.down = down; h->dlv.half = half;
    h->dlv.cfg = *cfg; h->dlv.cfg.taps = nullptr;
    h->dlv.ready = true;
    return 0;
}

int ev_deliver(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const uint32_t* seeds, uint32_t flags, ev_deliver_result* out) {
    if (!h) return -1;
    if (!wav) return fail(h, "ev_deliver: wav is NULL");
    if (!lens) return fail(h, "ev_deliver: lens is NULL");
    if (!out) return fail(h, "ev_deliver: out is NULL");
    if (check_struct_size(h, "ev_deliver", "out->struct_size", out->struct_size, "ev_deliver_result", sizeof(ev_deliver_result))) return -1;
    if (!h->dlv.ready) return fail(h, "ev_deliver: ev_deliver_setup has not been called");
    if (B < 1 || B > 65535) return fail(h, "ev_deliver: B = %d outside [1, 65535]", B);
    const ev_deliver_config& c = h->dlv.cfg;
    const int up = h->dlv.up, down = h->dlv.down, half = h->dlv.half;
    const int es_out = c.encoding == EV_DELIVER_F32 ? 4 : c.encoding == EV_DELIVER_S16 ? 2 : 1;
    std::vector<DeliverSeq> seqs; std::vector<DeliverTile> tiles;
    int64_t total_bytes = 0;
    const int bad = deliver_layout(B, lens, up, down, es_out, seeds, c.seed, seqs, tiles, &total_bytes);
    if (bad > 0) return fail(h, "ev_deliver: lens[%d] = %lld < 1", bad - 1, (long long)lens[bad - 1]);
    if (bad < 0) return fail(h, "ev_deliver: utterance %d (lens[%d] = %lld samples) gives more than EV_ALIGN_MAX_FRAMES * 256 = %lld output samples", -bad - 1, -bad - 1,
                             (long long)lens[-bad - 1], (long long)RS_MAX_OUT);
    const int64_t total_in = seqs[B - 1].in_off + seqs[B - 1].len;
    int64_t total_n = 0;
    for (int b = 0; b < B; ++b) total_n += seqs[b].n;
    const bool copy = up == 1 && down == 1;
    const size_t NT = tiles.size();
    WavIn in(wav, total_in, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    DeliverSeq* d_seqs = nullptr; DeliverTile* d_tiles = nullptr; DeliverPart* d_parts = nullptr; DeliverOut* d_outs = nullptr;
    uint8_t* d_data = nullptr;
    if (arena_plan(h, ARENA_DELIVER, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_seqs = ap.arr<DeliverSeq>(B); d_tiles = ap.arr<DeliverTile>(NT); d_parts = ap.arr<DeliverPart>(NT); d_outs = ap.arr<DeliverOut>(B);
        d_data = ap.arr<uint8_t>((size_t)total_bytes);
    })) return -1;
    if (in.copy(h) || upload(h, d_seqs, seqs) || upload(h, d_tiles, tiles)) return -1;
    DeliverParams p{};
    p.wav = in.ptr(); p.wav_is_i16 = wav_is_i16 != 0; p.seqs = d_seqs; p.tiles = d_tiles; p.n_tiles = (int)NT;
    p.up = up; p.down = down; p.half = half; p.row = copy ? 0 : resample_row_len(up, half); p.tab = h->dlv.tab.as<float>();
    p.encoding = c.encoding; p.dither = c.dither; p.out = d_data; p.parts = d_parts;
    region_begin(h, "total");
    {
        KScope ks(h, copy ? "deliver_copy" : "deliver_poly", copy ? 0.0 : 2.0 * (double)total_n * (2.0 * half / up + 1.0), (double)in.bytes + (double)total_bytes);
        if (launch_deliver(p, h->stream)) return fail(h, "ev_deliver: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {
        KScope ks(h, "deliver_fold", 0.0, (double)NT * sizeof(DeliverPart) + (double)B * sizeof(DeliverOut));
        launch_deliver_fold(d_parts, d_seqs, B, d_outs, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    std::vector<DeliverOut> outs((size_t)B);
    HIPCHK(h, hipMemcpyAsync(outs.data(), d_outs, (size_t)B * sizeof(DeliverOut), hipMemcpyDeviceToHost, h->stream));
    if (call_end(h)) return -1;
    std::vector<int64_t> offs((size_t)B + 1), n((size_t)B), clipped((size_t)B); std::vector<float> peak((size_t)B);
    for (int b = 0; b < B; ++b) { offs[b] = seqs[b].byte_off; n[b] = seqs[b].n; peak[b] = outs[b].peak; clipped[b] = outs[b].clipped; }
    offs[B] = total_bytes;
    h->dlv.offs.swap(offs); h->dlv.n.swap(n); h->dlv.clipped.swap(clipped); h->dlv.peak.swap(peak);
    reset_result(out);
    out->batch = B; out->total_bytes = total_bytes; out->data = d_data;
    out->byte_offsets = h->dlv.offs.data(); out->n_samples = h->dlv.n.data(); out->peak = h->dlv.peak.data(); out->clipped = h->dlv.clipped.data();
    return 0;
}

// ------------------------------------------------------------------- vocoder bias removal (include/evhip.h: ev_denoise)
static_assert(EV_DENOISE_MAX_R == DN_MAX_R, "include/evhip.h states the limit of ev_denoise.hip");
void ev_default_denoise_config(ev_denoise_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof(ev_denoise_config);
    c->n_fft = 1024; c->hop = 256; c->strength = 0.01f;
}

static int denoise_check_shape(ev_handle* h, const char* who, int n_fft, int hop) {
    if (features_check_config(h, who, n_fft, hop, 1)) return -1;
    if (n_fft % hop || n_fft / hop > DN_MAX_R) return fail(h, "%s: hop %d must divide n_fft %d with n_fft / hop <= %d", who, hop, n_fft, DN_MAX_R);
    return 0;
}

// the three tables of a shape, packed on the host and uploaded, one allocation each: 0, or -1 (the caller's local frees what was built)
static int denoise_upload_tables(int n_fft, int hop, const float* window, StftTables& t) {
    std::vector<uint16_t> hb(stft_basis_halfs(n_fft)), hi(istft_basis_halfs(n_fft, hop));
    std::vector<float> he(istft_envelope_floats(n_fft, hop));
    stft_pack_basis(n_fft, window, hb.data());
    istft_pack_basis(n_fft, hop, window, hi.data());
    istft_pack_envelope(n_fft, hop, window, he.data());
    return dev_upload(t.basis, hb) == hipSuccess && dev_upload(t.ibasis, hi) == hipSuccess && dev_upload(t.env, he) == hipSuccess ? 0 : -1;
}

static int denoise_bad_value(int n, const float* v) {      // -1, or the first index of a value that is negative, NaN or infinite
    for (int i = 0; i < n; ++i) if (!(v[i] >= 0.f) || !std::isfinite(v[i])) return i;
    return -1;
}

int ev_denoise_setup(ev_handle* h, const ev_denoise_config* cfg, const float* bias) {
    if (!h) return -1;
    if (!cfg) return fail(h, "ev_denoise_setup: null config");
    if (check_struct_size(h, "ev_denoise_setup", "struct_size", cfg->struct_size, "ev_denoise_config", sizeof(ev_denoise_config))) return -1;
    if (denoise_check_shape(h, "ev_denoise_setup", cfg->n_fft, cfg->hop)) return -1;
    if (!(cfg->strength >= 0.f) || !std::isfinite(cfg->strength)) return fail(h, "ev_denoise_setup: strength must be >= 0 and finite");
    const int n_bins = cfg->n_fft / 2 + 1;
    if (bias) {
        const int bad = denoise_bad_value(n_bins, bias);
        if (bad >= 0) return fail(h, "ev_denoise_setup: bias[%d] must be >= 0 and finite", bad);
    } else if (!h->wt.count("voc.post.w")) {
        return fail(h, "ev_denoise_setup: bias is NULL and no weights are loaded to measure one with");
    }
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    StftTables tab; DevMem d_bias;
    if (denoise_upload_tables(cfg->n_fft, cfg->hop, cfg->window, tab)) return fail(h, "ev_denoise_setup: uploading the tables failed");
    if (bias) {
        if (dev_upload(d_bias, bias, (size_t)n_bins * 4) != hipSuccess) return fail(h, "ev_denoise_setup: uploading the bias failed");
    } else {      // the vocoder's answer to a zero mel; the magnitudes of its frame 0 go straight into d_bias
        if (d_bias.alloc((size_t)n_bins * 4) != hipSuccess) return fail(h, "ev_denoise_setup: no memory for the bias");
        const int32_t frames = EV_DENOISE_BIAS_FRAMES;
        std::vector<float> mel((size_t)h->cfg.n_mels * frames, 0.f);
        ev_result r;
        if (ev_vocoder(h, 1, mel.data(), 0, &frames, 0, &r)) return -1;
        const int64_t L = r.total_samples;
        if (L < cfg->n_fft / 2 + 1) return fail(h, "ev_denoise_setup: the vocoder's %lld samples are fewer than n_fft / 2 + 1", (long long)L);
        const StftSeq sq{0, L, 0, (int32_t)(L / cfg->hop + 1), 0};
        const StftTile tile{0, 0};
        DevTable dt;
        const size_t so = dt.add(&sq, sizeof sq), to = dt.add(&tile, sizeof tile);
        if (dt.commit()) return fail(h, "ev_denoise_setup: no memory for the bias measurement");
        StftGainParams p{stft_front(r.wav, 0, dt.at<StftSeq>(so), dt.at<StftTile>(to), 1, tab.basis.get(), cfg->n_fft, cfg->hop)};
        p.mag = d_bias.as<float>(); p.mag_frames = 1;
        if (launch_stft_gain(p, h->stream)) return fail(h, "ev_denoise_setup: the kernel does not build this shape");
        if (hipStreamSynchronize(h->stream) != hipSuccess) return fail(h, "ev_denoise_setup: measuring the bias failed");
    }
    h->dn.tab = std::move(tab); h->dn.bias = std::move(d_bias);
    h->dn.cfg = *cfg; h->dn.cfg.window = nullptr;
    h->dn.ready = true;
    return 0;
}

int ev_denoise_bias(ev_handle* h, float* out) {
    if (!h) return -1;
    if (!out) return fail(h, "ev_denoise_bias: out is NULL");
    if (!h->dn.ready) return fail(h, "ev_denoise_bias: ev_denoise_setup has not been called");
    HIPCHK(h, hipSetDevice(h->device));
    HIPCHK(h, hipStreamSynchronize(h->stream));
    HIPCHK(h, hipMemcpy(out, h->dn.bias.get(), (size_t)(h->dn.cfg.n_fft / 2 + 1) * 4, hipMemcpyDeviceToHost));
    return 0;
}

int ev_denoise(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const float* strengths, uint32_t flags, ev_denoise_result* out) {
    if (!h) return -1;
    if (!out) return fail(h, "ev_denoise: out is NULL");
    if (check_struct_size(h, "ev_denoise", "out->struct_size", out->struct_size, "ev_denoise_result", sizeof(ev_denoise_result))) return -1;
    if (!h->dn.ready) return fail(h, "ev_denoise: ev_denoise_setup has not been called");
    const ev_denoise_config& c = h->dn.cfg;
    const int n_fft = c.n_fft, hop = c.hop;
    FrameGrid g;
    if (stft_grid(h, "ev_denoise", "utterance", n_fft, hop, B, wav, lens, g)) return -1;
    if (strengths) {
        const int bad = denoise_bad_value(B, strengths);
        if (bad >= 0) return fail(h, "ev_denoise: strengths[%d] must be >= 0 and finite", bad);
    }
    IstftTrip trip(g, n_fft, hop, c.want_i16 != 0);
    std::vector<float> st((size_t)B);
    for (int b = 0; b < B; ++b) st[b] = strengths ? strengths[b] : c.strength;
    WavIn in(wav, g.seqs[B - 1].wav_off + g.seqs[B - 1].len, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    StftSeq* d_seqs = nullptr; StftTile* d_tiles = nullptr; float* d_st = nullptr;
    if (arena_plan(h, ARENA_DENOISE, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_seqs = ap.arr<StftSeq>(B); d_tiles = ap.arr<StftTile>(g.tiles.size()); d_st = ap.arr<float>(B);
        trip.plan(ap);
    })) return -1;
    if (in.copy(h) || upload(h, d_seqs, g.seqs) || upload(h, d_tiles, g.tiles) || upload(h, d_st, st) || trip.copy(h)) return -1;
    region_begin(h, "total");
    {
        StftGainParams p{stft_front(in.ptr(), wav_is_i16, d_seqs, d_tiles, g.tiles.size(), h->dn.tab.basis.get(), n_fft, hop)};
        p.bias = h->dn.bias.as<float>(); p.strengths = d_st; p.spec_hi = trip.hi; p.spec_lo = trip.lo;
        const double tile_frames = (double)64 * (double)g.tiles.size();
        KScope ks(h, "stft_gain", 2.0 * 3.0 * tile_frames * n_fft * 2.0 * (n_fft / 2 + 1), (double)in.bytes + trip.plane_bytes());
        if (launch_stft_gain(p, h->stream)) return fail(h, "ev_denoise: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    if (trip.inverse(h, "ev_denoise", h->dn.tab)) return -1;
    if (call_end(h)) return -1;
    trip.finish(h->dn.res, out);
    return 0;
}

// ------------------------------------------------------------------- time-scale modification (include/evhip.h: ev_stretch)
static_assert(EV_STRETCH_FRAME == STRETCH_FRAME && EV_STRETCH_HOP == STRETCH_HOP && EV_STRETCH_LAGS == STRETCH_LAGS,
              "include/evhip.h states the frame, the hop and the lags of ev_stretch.hip");
void ev_default_stretch_config(ev_stretch_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c;
}

int ev_stretch_window(float* w) {
    if (!w) return -1;
    const double pi = 3.14159265358979323846;
    for (int j = 0; j < EV_STRETCH_HOP; ++j) w[j] = (float)(rint(8388608.0 * (0.5 - 0.5 * cos(2.0 * pi * (double)j / (double)EV_STRETCH_FRAME))) / 8388608.0);
    return EV_STRETCH_HOP;
}

// the message of a pair of lengths that stretch_check rejects
static int stretch_fail(ev_handle* h, const char* who, StretchBad bad, int b, int64_t len_in, int64_t len_out) {
    switch (bad) {
    case STRETCH_OK: return 0;
    case STRETCH_IN_SHORT: return fail(h, "%s: lens[%d] = %lld < 1", who, b, (long long)len_in);
    case STRETCH_OUT_SHORT: return fail(h, "%s: lens_out[%d] = %lld < 1", who, b, (long long)len_out);
    case STRETCH_IN_LONG: return fail(h, "%s: lens[%d] = %lld > EV_STRETCH_MAX_SAMPLES = %d", who, b, (long long)len_in, EV_STRETCH_MAX_SAMPLES);
    case STRETCH_OUT_LONG: return fail(h, "%s: lens_out[%d] = %lld > EV_STRETCH_MAX_SAMPLES = %d", who, b, (long long)len_out, EV_STRETCH_MAX_SAMPLES);
    case STRETCH_RATIO: return fail(h, "%s: segment %d: %lld -> %lld samples lies outside the ratios [0.5, 2]", who, b, (long long)len_in, (long long)len_out);
    case STRETCH_COUNT: return fail(h, "%s: lens_out[%d] = %lld: more than %d tiles in one call", who, b, (long long)len_out, INT_MAX);
    }
    return -1;
}

int ev_stretch_plan(int B, const int64_t* lens, const double* speeds, const int64_t* targets, int64_t* lens_out) {
    if (!lens) return fail(nullptr, "ev_stretch_plan: lens is NULL");
    if (!lens_out) return fail(nullptr, "ev_stretch_plan: lens_out is NULL");
    if (B < 1 || B > 65535) return fail(nullptr, "ev_stretch_plan: B = %d outside [1, 65535]", B);
    std::vector<int64_t> lo((size_t)B);
    for (int b = 0; b < B; ++b) {
        if (targets && targets[b] != 0) lo[(size_t)b] = targets[b];
        else {
            const double s = speeds ? speeds[b] : 1.0;
            if (!(std::isfinite(s) && s > 0.0)) return fail(nullptr, "ev_stretch_plan: speeds[%d] = %g is not finite and > 0", b, s);
            const double v = nearbyint((double)lens[b] / s);      // ties to even (the default rounding mode)
            lo[(size_t)b] = v >= 4e18 ? INT64_MAX : std::max<int64_t>(1, (int64_t)v);
        }
        const StretchBad bad = stretch_check(lens[b], lo[(size_t)b]);
        if (bad != STRETCH_OK) return stretch_fail(nullptr, "ev_stretch_plan", bad, b, lens[b], lo[(size_t)b]);
    }
    std::copy(lo.begin(), lo.end(), lens_out);
    return 0;
}

int ev_stretch(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const int64_t* lens_out, const ev_stretch_config* cfg,
               uint32_t flags, ev_stretch_result* out) {
    if (!h) return -1;
    if (!wav) return fail(h, "ev_stretch: wav is NULL");
    if (!lens) return fail(h, "ev_stretch: lens is NULL");
    if (!lens_out) return fail(h, "ev_stretch: lens_out is NULL");
    if (!out) return fail(h, "ev_stretch: out is NULL");
    if (check_struct_size(h, "ev_stretch", "out->struct_size", out->struct_size, "ev_stretch_result", sizeof(ev_stretch_result))) return -1;
    ev_stretch_config dflt;
    if (!cfg) { ev_default_stretch_config(&dflt); cfg = &dflt; }
    if (check_struct_size(h, "ev_stretch", "cfg->struct_size", cfg->struct_size, "ev_stretch_config", sizeof(ev_stretch_config))) return -1;
    if (B < 1 || B > 65535) return fail(h, "ev_stretch: B = %d outside [1, 65535]", B);
    StretchPlan plan;
    int at = 0;
    const StretchBad bad = stretch_plan(B, lens, lens_out, plan, &at);
    if (bad != STRETCH_OK) return stretch_fail(h, "ev_stretch", bad, at, lens[at], lens_out[at]);
    const bool in16 = wav_is_i16 != 0, i16 = cfg->want_int16 != 0;
    const int64_t total = plan.total_out, NF = plan.total_frames, NT = (int64_t)plan.tiles.size();
    std::vector<float> win(EV_STRETCH_HOP);
    ev_stretch_window(win.data());
    WavIn in(wav, plan.total_in, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    StretchSeg* d_segs = nullptr; StretchTile* d_tiles = nullptr; StretchFig* d_figs = nullptr; float *d_win = nullptr, *d_wav = nullptr;
    int16_t *d_deltas = nullptr, *d_i16 = nullptr;
    if (arena_plan(h, ARENA_STRETCH, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_segs = ap.arr<StretchSeg>((size_t)B); d_tiles = ap.arr<StretchTile>((size_t)NT); d_figs = ap.arr<StretchFig>((size_t)B);
        d_win = ap.arr<float>(EV_STRETCH_HOP); d_deltas = ap.arr<int16_t>((size_t)NF); d_wav = ap.arr<float>((size_t)total);
        if (i16) d_i16 = ap.arr<int16_t>((size_t)total);
    })) return -1;
    if (in.copy(h) || upload(h, d_segs, plan.segs) || upload(h, d_tiles, plan.tiles) || upload(h, d_win, win)) return -1;
    const double es = in16 ? 2.0 : 4.0;
    region_begin(h, "total");
    {      // per frame 256 lags of 512 terms, three operations a term; each frame stages 1023 samples
        KScope ks(h, "wsola_search", 3.0 * STRETCH_LAGS * STRETCH_FRAME * (double)NF, (in16 ? 0.0 : (double)in.bytes) + 1023.0 * es * (double)NF + 2.0 * (double)NF);
        if (launch_wsola_search(in.ptr(), in16, d_segs, B, d_deltas, d_figs, h->stream)) return fail(h, "ev_stretch: the kernels do not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {
        KScope ks(h, "wsola_ola", 3.0 * (double)total, (2.0 * es + 4.0 + (i16 ? 2.0 : 0.0)) * (double)total + 2.0 * (double)NF);
        if (launch_wsola_ola(in.ptr(), in16, d_segs, d_tiles, NT, d_deltas, d_win, d_wav, d_i16, h->stream)) return fail(h, "ev_stretch: the kernels do not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    std::vector<StretchFig> figs((size_t)B);
    HIPCHK(h, hipMemcpyAsync(figs.data(), d_figs, (size_t)B * sizeof(StretchFig), hipMemcpyDeviceToHost, h->stream));
    if (call_end(h)) return -1;
    std::vector<int32_t> edges((size_t)B); std::vector<uint64_t> sd((size_t)B); std::vector<int64_t> nonf((size_t)B);
    for (int b = 0; b < B; ++b) { edges[(size_t)b] = figs[(size_t)b].edge_frames; sd[(size_t)b] = figs[(size_t)b].sum_dist; nonf[(size_t)b] = figs[(size_t)b].nonfinite; }
    h->str.lens_out.swap(plan.lens_out); h->str.offs.swap(plan.offs); h->str.frame_offs.swap(plan.frame_offs); h->str.frames.swap(plan.frames);
    h->str.edges.swap(edges); h->str.sum_dist.swap(sd); h->str.nonf.swap(nonf);
    reset_result(out);
    out->batch = B; out->total = total; out->wav = d_wav; out->wav_i16 = d_i16;
    out->lens_out = h->str.lens_out.data(); out->offsets = h->str.offs.data(); out->frames = h->str.frames.data(); out->frame_offsets = h->str.frame_offs.data();
    out->deltas = d_deltas; out->edge_frames = h->str.edges.data(); out->sum_dist = h->str.sum_dist.data(); out->nonfinite = h->str.nonf.data();
    return 0;
}

// ------------------------------------------------------------------- audio watermark (include/evhip.h: ev_watermark, ev_watermark_detect)
static_assert(EV_WATERMARK_NFFT == WM_NFFT && EV_WATERMARK_HOP == WM_HOP && EV_WATERMARK_BAND0 == WM_BAND0 && EV_WATERMARK_BANDS == WM_BANDS &&
              EV_WATERMARK_TILE == WM_TILE && EV_WATERMARK_PERIOD == WM_PERIOD && EV_WATERMARK_CHIPS == WM_CHIPS && EV_WATERMARK_OFFSETS == WM_OFFSETS &&
              EV_WATERMARK_MAX_BITS == WM_MAX_BITS, "include/evhip.h states the constants of ev_watermark.hip");
void ev_default_watermark_config(ev_watermark_config* c) {
    memset(c, 0, sizeof *c);
    c->struct_size = sizeof *c;
    c->strength_db = 1.0f;
}

static bool watermark_payload_ok(int nbits, uint32_t payload) { return nbits >= 0 && nbits <= WM_MAX_BITS && (uint64_t)payload < (1ull << nbits); }

int ev_watermark_pattern(uint32_t key, int nbits, uint32_t payload, int8_t* signs) {
    if (!signs || !watermark_payload_ok(nbits, payload)) return -1;
    watermark_pattern(key, nbits, payload, signs, nullptr);
    return 0;
}

// ev_denoise's tables at the watermark's shape, once per handle
static int watermark_tables(ev_handle* h, const char* who) {
    if (h->wm.ready) return 0;
    HIPCHK(h, hipSetDevice(h->device));
    StftTables tab;
    if (denoise_upload_tables(WM_NFFT, WM_HOP, nullptr, tab)) return fail(h, "%s: uploading the tables failed", who);
    h->wm.tab = std::move(tab);
    h->wm.ready = true;
    return 0;
}

int ev_watermark(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, const ev_watermark_config* cfg, const uint32_t* payloads,
                 const int32_t* nbits, const float* strengths_db, uint32_t flags, ev_watermark_result* out) {
    if (!h) return -1;
    if (!out) return fail(h, "ev_watermark: out is NULL");
    if (check_struct_size(h, "ev_watermark", "out->struct_size", out->struct_size, "ev_watermark_result", sizeof(ev_watermark_result))) return -1;
    ev_watermark_config dflt;
    if (!cfg) { ev_default_watermark_config(&dflt); cfg = &dflt; }
    if (check_struct_size(h, "ev_watermark", "cfg->struct_size", cfg->struct_size, "ev_watermark_config", sizeof(ev_watermark_config))) return -1;
    FrameGrid g;
    if (stft_grid(h, "ev_watermark", "segment", WM_NFFT, WM_HOP, B, wav, lens, g)) return -1;
    std::vector<int8_t> signs((size_t)B * WM_CHIPS);
    std::vector<float> gains((size_t)B * 2);
    for (int b = 0; b < B; ++b) {
        const int nb = nbits ? nbits[b] : cfg->nbits;
        const uint32_t pl = payloads ? payloads[b] : cfg->payload;
        const float db = strengths_db ? strengths_db[b] : cfg->strength_db;
        if (nb < 0 || nb > WM_MAX_BITS) return fail(h, "ev_watermark: nbits[%d] = %d outside [0, %d]", b, nb, WM_MAX_BITS);
        if (!watermark_payload_ok(nb, pl)) return fail(h, "ev_watermark: payloads[%d] = %u does not fit %d bits", b, pl, nb);
        if (!(db >= 0.f && db <= EV_WATERMARK_MAX_DB)) return fail(h, "ev_watermark: strengths_db[%d] = %g outside [0, %g]", b, (double)db, (double)EV_WATERMARK_MAX_DB);
        watermark_pattern(cfg->key, nb, pl, signs.data() + (size_t)b * WM_CHIPS, nullptr);
        const float a = (float)pow(10.0, (double)db / 20.0);
        gains[2 * (size_t)b] = a;
        gains[2 * (size_t)b + 1] = 1.0f / a;
    }
    IstftTrip trip(g, WM_NFFT, WM_HOP, cfg->want_i16 != 0);
    WavIn in(wav, g.seqs[B - 1].wav_off + g.seqs[B - 1].len, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    if (watermark_tables(h, "ev_watermark")) return -1;
    StftSeq* d_seqs = nullptr; StftTile* d_tiles = nullptr; float* d_gains = nullptr; int8_t* d_signs = nullptr;
    if (arena_plan(h, ARENA_WATERMARK, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_seqs = ap.arr<StftSeq>(B); d_tiles = ap.arr<StftTile>(g.tiles.size()); d_gains = ap.arr<float>(gains.size()); d_signs = ap.arr<int8_t>(signs.size());
        trip.plan(ap);
    })) return -1;
    if (in.copy(h) || upload(h, d_seqs, g.seqs) || upload(h, d_tiles, g.tiles) || upload(h, d_gains, gains) || upload(h, d_signs, signs) || trip.copy(h)) return -1;
    region_begin(h, "total");
    {
        const WmEmbedParams p{stft_front(in.ptr(), wav_is_i16, d_seqs, d_tiles, g.tiles.size(), h->wm.tab.basis.get(), WM_NFFT, WM_HOP), d_signs, d_gains, trip.hi, trip.lo};
        KScope ks(h, "wm_embed", 2.0 * 3.0 * 64.0 * (double)g.tiles.size() * WM_NFFT * 2.0 * (WM_NFFT / 2 + 1), (double)in.bytes + trip.plane_bytes());
        if (launch_wm_embed(p, h->stream)) return fail(h, "ev_watermark: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    if (trip.inverse(h, "ev_watermark", h->wm.tab)) return -1;
    if (call_end(h)) return -1;
    trip.finish(h->wm.res, out);
    return 0;
}

int ev_watermark_detect(ev_handle* h, int B, const void* wav, int wav_is_i16, const int64_t* lens, uint32_t key, int nbits, uint32_t flags,
                        ev_watermark_detect_result* out) {
    if (!h) return -1;
    if (!out) return fail(h, "ev_watermark_detect: out is NULL");
    if (check_struct_size(h, "ev_watermark_detect", "out->struct_size", out->struct_size, "ev_watermark_detect_result", sizeof(ev_watermark_detect_result))) return -1;
    FrameGrid g;
    if (stft_grid(h, "ev_watermark_detect", "segment", WM_NFFT, WM_HOP, B, wav, lens, g)) return -1;
    if (nbits < 0 || nbits > WM_MAX_BITS) return fail(h, "ev_watermark_detect: nbits = %d outside [0, %d]", nbits, WM_MAX_BITS);
    std::vector<int8_t> tabs(3 * (size_t)WM_CHIPS);      // the pilots' signs (0 for a payload chip), every sign at payload 0, every role
    watermark_pattern(key, nbits, 0, tabs.data() + WM_CHIPS, reinterpret_cast<uint8_t*>(tabs.data()) + 2 * WM_CHIPS);
    for (int i = 0; i < WM_CHIPS; ++i) tabs[(size_t)i] = (uint8_t)tabs[2 * (size_t)WM_CHIPS + i] == WM_PILOT ? tabs[(size_t)WM_CHIPS + i] : (int8_t)0;
    const int64_t total_frames = g.offs[B], total_in = g.seqs[B - 1].wav_off + g.seqs[B - 1].len;
    WavIn in(wav, total_in, wav_is_i16, flags);
    if (call_begin(h)) return -1;
    if (watermark_tables(h, "ev_watermark_detect")) return -1;
    StftSeq* d_seqs = nullptr; StftTile* d_tiles = nullptr; int32_t *d_q = nullptr, *d_win = nullptr; int8_t* d_tabs = nullptr; WmFig* d_figs = nullptr;
    if (arena_plan(h, ARENA_WM_DETECT, [&](ArenaPlan& ap) {
        in.plan(ap);
        d_seqs = ap.arr<StftSeq>(B); d_tiles = ap.arr<StftTile>(g.tiles.size()); d_tabs = ap.arr<int8_t>(tabs.size()); d_figs = ap.arr<WmFig>(B);
        d_q = ap.arr<int32_t>((size_t)total_frames * WM_BANDS); d_win = ap.arr<int32_t>((size_t)total_frames * WM_BANDS);
    })) return -1;
    if (in.copy(h) || upload(h, d_seqs, g.seqs) || upload(h, d_tiles, g.tiles) || upload(h, d_tabs, tabs)) return -1;
    region_begin(h, "total");
    {
        const WmBandParams p{stft_front(in.ptr(), wav_is_i16, d_seqs, d_tiles, g.tiles.size(), h->wm.tab.basis.get(), WM_NFFT, WM_HOP), d_q};
        KScope ks(h, "wm_bands", 2.0 * 3.0 * 64.0 * (double)g.tiles.size() * WM_NFFT * 2.0 * (WM_NFFT / 2 + 1), (double)in.bytes + 4.0 * (double)total_frames * WM_BANDS);
        if (launch_wm_bands(p, h->stream)) return fail(h, "ev_watermark_detect: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {      // per (tile, band) one contrast, added into 16 offsets per phase, 8 phases
        KScope ks(h, "wm_correlate", 2.0 * WM_OFFSETS * (double)total_frames / WM_TILE * WM_BANDS, 4.0 * 10.0 * (double)total_frames * WM_BANDS);
        if (launch_wm_correlate(d_q, d_win, d_seqs, B, d_tabs, d_figs, h->stream)) return fail(h, "ev_watermark_detect: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    std::vector<WmFig> figs((size_t)B);
    HIPCHK(h, hipMemcpyAsync(figs.data(), d_figs, (size_t)B * sizeof(WmFig), hipMemcpyDeviceToHost, h->stream));
    if (call_end(h)) return -1;
    evh::WatermarkState& w = h->wm;
    w.offset.resize((size_t)B); w.C.resize((size_t)B); w.n.resize((size_t)B); w.bit_C.resize((size_t)B * WM_MAX_BITS); w.bit_n.resize((size_t)B * WM_MAX_BITS);
    for (int b = 0; b < B; ++b) {
        w.offset[(size_t)b] = figs[(size_t)b].offset; w.C[(size_t)b] = figs[(size_t)b].C; w.n[(size_t)b] = figs[(size_t)b].n;
        std::copy(figs[(size_t)b].bit_C, figs[(size_t)b].bit_C + WM_MAX_BITS, w.bit_C.begin() + (size_t)b * WM_MAX_BITS);
        std::copy(figs[(size_t)b].bit_n, figs[(size_t)b].bit_n + WM_MAX_BITS, w.bit_n.begin() + (size_t)b * WM_MAX_BITS);
    }
    w.frames.swap(g.lens); w.frame_offs.swap(g.offs);
    reset_result(out);
    out->batch = B; out->nbits = nbits; out->offset = w.offset.data(); out->C = w.C.data(); out->n = w.n.data(); out->bit_C = w.bit_C.data(); out->bit_n = w.bit_n.data();
    out->frames = w.frames.data(); out->frame_offsets = w.frame_offs.data(); out->q = d_q;
    return 0;
}

// ------------------------------------------------------------------- objective scoring (include/evhip.h: ev_score)
static_assert(EV_SCORE_MAX_FRAMES == SCORE_MAX_FRAMES && EV_SCORE_MAX_CEPS == SCORE_MAX_CEPS && EV_FEATURES_MAX_MELS == SCORE_MAX_MELS &&
              EV_SCORE_CLAMP == SCORE_CLAMP && EV_SCORE_Q == 65536, "include/evhip.h states the limits of ev_score.hip");
static int score_check_shape(ev_handle* h, const char* who, int n_mels, int n_ceps) {
    if (n_mels < 1 || n_mels > EV_FEATURES_MAX_MELS) return fail(h, "%s: n_mels = %d outside [1, %d]", who, n_mels, EV_FEATURES_MAX_MELS);
    const int top = std::min(n_mels - 1, EV_SCORE_MAX_CEPS);
    if (n_ceps < 1 || n_ceps > top) return fail(h, "%s: n_ceps = %d outside [1, min(n_mels - 1, %d) = %d]", who, n_ceps, EV_SCORE_MAX_CEPS, top);
    return 0;
}

int ev_score_design(int n_mels, int n_ceps, float* basis) {
    if (!basis) return fail(nullptr, "ev_score_design: basis is NULL");
    if (score_check_shape(nullptr, "ev_score_design", n_mels, n_ceps)) return -1;
    const double M = (double)n_mels, g = sqrt(2.0 / M);
    for (int d = 1; d <= n_ceps; ++d)
        for (int m = 0; m < n_mels; ++m) basis[(size_t)(d - 1) * n_mels + m] = (float)(g * cos(M_PI * (double)d * ((double)m + 0.5) / M));
    return 0;
}

// the words (uint32) of a pair's distances and of its decisions, in the order the warp visits them (ev_kernels.h)
static int64_t score_dist_words(int Ta, int Tb) { return ((int64_t)Tb + 63) * score_run(Ta) * 64; }
static int64_t score_dec_total(int Ta, int Tb) { return ((int64_t)Tb + 63) * score_dec_words(score_run(Ta)) * 64; }
// consecutive pairs form a pass while the distances and decisions of all of them fit EV_SCORE_WORKSPACE together; the lengths are validated
static int score_plan(int B, const int32_t* la, const int32_t* lb, int32_t* pass_of, int64_t* pass_bytes) {
    int n = 0;
    int64_t bytes = 0;
    for (int b = 0; b < B; ++b) {
        const int64_t need = 4 * (score_dist_words(la[b], lb[b]) + score_dec_total(la[b], lb[b]));
        if (n == 0 || bytes + need > EV_SCORE_WORKSPACE) { ++n; bytes = 0; }
        bytes += need;
        pass_of[b] = n - 1; pass_bytes[n - 1] = bytes;
    }
    return n;
}

int ev_score_plan(int B, const int32_t* lens_a, const int32_t* lens_b, int32_t* pass_of, int64_t* pass_bytes) {
    if (!lens_a || !lens_b || !pass_of || !pass_bytes) return fail(nullptr, "ev_score_plan: NULL argument");
    if (B < 1 || B > 65535) return fail(nullptr, "ev_score_plan: B = %d outside [1, 65535]", B);
    for (int b = 0; b < B; ++b) {
        if (lens_a[b] < 1 || lens_a[b] > EV_SCORE_MAX_FRAMES) return fail(nullptr, "ev_score_plan: lens_a[%d] = %d outside [1, %d]", b, lens_a[b], EV_SCORE_MAX_FRAMES);
        if (lens_b[b] < 1 || lens_b[b] > EV_SCORE_MAX_FRAMES) return fail(nullptr, "ev_score_plan: lens_b[%d] = %d outside [1, %d]", b, lens_b[b], EV_SCORE_MAX_FRAMES);
    }
    return score_plan(B, lens_a, lens_b, pass_of, pass_bytes);
}

int ev_score_load(ev_handle* h, int side, int B, int n_mels, int n_ceps, const float* mel, const int32_t* lens, const float* f0_hz, uint32_t flags) {
    if (!mel) return fail(h, "ev_score_load: mel is NULL");
    if (!lens) return fail(h, "ev_score_load: lens is NULL");
    if (side != 0 && side != 1) return fail(h, "ev_score_load: side = %d is not 0 (a, under test) or 1 (b, the yardstick)", side);
    if (B < 1 || B > 65535) return fail(h, "ev_score_load: B = %d outside [1, 65535]", B);
    if (score_check_shape(h, "ev_score_load", n_mels, n_ceps)) return -1;
    for (int b = 0; b < B; ++b)
        if (lens[b] < 1 || lens[b] > EV_SCORE_MAX_FRAMES) return fail(h, "ev_score_load: lens[%d] = %d outside [1, %d]", b, lens[b], EV_SCORE_MAX_FRAMES);
    if (!h) return fail(nullptr, "ev_score_load: h is NULL");
    const bool dev_in = (flags & EV_FLAG_DEVICE_INPUTS) != 0;
    const int M = n_mels, D = n_ceps;
    std::vector<int64_t> offs((size_t)B + 1, 0);
    std::vector<ScoreTile> tiles; std::vector<ScoreSig> sigs((size_t)B);
    for (int b = 0; b < B; ++b) {
        offs[(size_t)b + 1] = offs[(size_t)b] + lens[b];
        sigs[(size_t)b] = ScoreSig{offs[(size_t)b], lens[b], 0};
        for (int t0 = 0; t0 < lens[b]; t0 += SCORE_TF) tiles.push_back(ScoreTile{offs[(size_t)b] * M, offs[(size_t)b], lens[b], t0, b, 0});
    }
    const int64_t total = offs[(size_t)B];
    std::vector<float> basis((size_t)D * M);
    (void)ev_score_design(M, D, basis.data());
    ScoreSide& sd = h->score.side[side];
    if (call_begin(h)) return -1;
    int32_t *d_cq = nullptr, *d_bad = nullptr, *d_nonf = nullptr; float *d_f0 = nullptr, *d_basis = nullptr, *d_mel = nullptr;
    ScoreTile* d_tiles = nullptr; ScoreSig* d_sigs = nullptr;
    sd.loaded = false;      // from here on the side's arena is rewritten
    if (arena_plan(h, side ? ARENA_SCORE_B : ARENA_SCORE_A, [&](ArenaPlan& ap) {
        d_cq = ap.arr<int32_t>((size_t)total * D); d_f0 = f0_hz ? ap.arr<float>((size_t)total) : nullptr;
        d_bad = ap.arr<int32_t>((size_t)total); d_nonf = ap.arr<int32_t>((size_t)B); d_basis = ap.arr<float>((size_t)D * M);
        d_tiles = ap.arr<ScoreTile>(tiles.size()); d_sigs = ap.arr<ScoreSig>((size_t)B);
        d_mel = dev_in ? nullptr : ap.arr<float>((size_t)total * M);
    })) return -1;
    if (!dev_in) HIPCHK(h, hipMemcpyAsync(d_mel, mel, (size_t)total * M * sizeof(float), hipMemcpyHostToDevice, h->stream));
    if (f0_hz) HIPCHK(h, hipMemcpyAsync(d_f0, f0_hz, (size_t)total * sizeof(float), dev_in ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, h->stream));
    if (upload(h, d_basis, basis) || upload(h, d_tiles, tiles) || upload(h, d_sigs, sigs)) return -1;
    region_begin(h, "total");
    {
        KScope ks(h, "score_cepstra", 2.0 * (double)total * M * D, 4.0 * (double)total * (M + D + 1));
        if (launch_score_cepstra(dev_in ? mel : d_mel, d_tiles, (int64_t)tiles.size(), d_basis, M, D, d_cq, d_bad, h->stream))
            return fail(h, "ev_score_load: the kernel does not build this shape");
    }
    HIPCHK(h, hipGetLastError());
    {
        KScope ks(h, "score_count", 0.0, 4.0 * (double)total);
        launch_score_count(d_bad, d_sigs, B, d_nonf, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    std::vector<int32_t> nonf((size_t)B);
    HIPCHK(h, hipMemcpyAsync(nonf.data(), d_nonf, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
    if (call_end(h)) return -1;
    sd.B = B; sd.n_mels = M; sd.n_ceps = D; sd.total = total; sd.cq = d_cq; sd.f0 = d_f0;
    sd.lens.assign(lens, lens + B); sd.nonf.swap(nonf); sd.offs.swap(offs);
    sd.loaded = true;
    return 0;
}

int ev_score(ev_handle* h, uint32_t flags, ev_score_result* out) {
    if (!out) return fail(h, "ev_score: out is NULL");
    if (check_struct_size(h, "ev_score", "out->struct_size", out->struct_size, "ev_score_result", sizeof(ev_score_result))) return -1;
    if (!h) return fail(nullptr, "ev_score: h is NULL");
    const ScoreSide &sa = h->score.side[0], &sb = h->score.side[1];
    if (!sa.loaded) return fail(h, "ev_score: side 0 (a) is not loaded: call ev_score_load(h, 0, ...)");
    if (!sb.loaded) return fail(h, "ev_score: side 1 (b) is not loaded: call ev_score_load(h, 1, ...)");
    if (sa.B != sb.B) return fail(h, "ev_score: the sides differ in B: %d signals on side 0, %d on side 1", sa.B, sb.B);
    if (sa.n_mels != sb.n_mels) return fail(h, "ev_score: the sides differ in n_mels: %d on side 0, %d on side 1", sa.n_mels, sb.n_mels);
    if (sa.n_ceps != sb.n_ceps) return fail(h, "ev_score: the sides differ in n_ceps: %d on side 0, %d on side 1", sa.n_ceps, sb.n_ceps);
    const int B = sa.B, D = sa.n_ceps;
    const bool linear = (flags & EV_SCORE_LINEAR) != 0;
    const bool f0 = sa.f0 && sb.f0;
    // the pair table; for a warp also the passes (score_plan) and, per pass and run, the pairs of a launch
    std::vector<ScorePair> pairs((size_t)B); std::vector<int32_t> sel, pass_of((size_t)B, 0); std::vector<int64_t> pass_bytes((size_t)B, 0);
    std::vector<int64_t> poffs((size_t)B + 1, 0);
    int64_t rev_total = 0, path_cap = 0, ws_words = 0;
    const int n_passes = linear ? 0 : score_plan(B, sa.lens.data(), sb.lens.data(), pass_of.data(), pass_bytes.data());
    for (int q = 0; q < n_passes; ++q) {
        if (pass_bytes[(size_t)q] > EV_SCORE_WORKSPACE) return fail(h, "ev_score: pass %d plans %lld bytes of workspace, more than EV_SCORE_WORKSPACE", q, (long long)pass_bytes[(size_t)q]);
        ws_words = std::max(ws_words, pass_bytes[(size_t)q] / 4);
    }
    {
        std::vector<int64_t> dist_n((size_t)n_passes + 1, 0), dec_n((size_t)n_passes + 1, 0);
        for (int b = 0; b < B; ++b) {
            ScorePair& p = pairs[(size_t)b];
            p = ScorePair{};
            p.fa_off = sa.offs[(size_t)b]; p.fb_off = sb.offs[(size_t)b]; p.Ta = sa.lens[(size_t)b]; p.Tb = sb.lens[(size_t)b];
            p.rm = score_run(p.Ta);
            if (linear) {
                p.K = std::min(p.Ta, p.Tb); p.path_off = path_cap; path_cap += p.K;
                poffs[(size_t)b + 1] = path_cap;
                continue;
            }
            const size_t q = (size_t)pass_of[(size_t)b];
            p.dist_off = dist_n[q]; p.dec_off = dec_n[q];
            dist_n[q] += score_dist_words(p.Ta, p.Tb); dec_n[q] += score_dec_total(p.Ta, p.Tb);
            p.rev_off = rev_total; rev_total += 2 * ((int64_t)p.Ta + p.Tb - 1);
            path_cap += (int64_t)p.Ta + p.Tb - 1;
        }
        if (!linear) for (int b = 0; b < B; ++b) pairs[(size_t)b].dec_off += dist_n[(size_t)pass_of[(size_t)b]];      // a pass' decisions lie behind its distances
    }
    struct Launch { int pass, rm, first, n, max_steps; double cells; };      // the pairs of one pass with one run, sel[first .. first + n)
    std::vector<Launch> launches;
    for (int q = 0, b0 = 0; q < n_passes; ++q) {
        int b1 = b0;
        while (b1 < B && pass_of[(size_t)b1] == q) ++b1;
        for (int rm = 1; rm <= 64; rm *= 2) {
            Launch l{q, rm, (int)sel.size(), 0, 0, 0.0};
            for (int b = b0; b < b1; ++b) {
                const ScorePair& p = pairs[(size_t)b];
                if (p.rm != rm) continue;
                sel.push_back(b);
                l.n += 1; l.max_steps = std::max(l.max_steps, p.Tb + 63); l.cells += (double)p.Ta * p.Tb;
            }
            if (l.n) launches.push_back(l);
        }
        b0 = b1;
    }
    if (call_begin(h)) return -1;
    ScorePair* d_pairs = nullptr; int32_t *d_sel = nullptr, *d_rev = nullptr, *d_cqa = nullptr, *d_cqb = nullptr, *d_pa = nullptr, *d_pb = nullptr;
    ScoreWarp* d_warp = nullptr; ScoreSums* d_sums = nullptr; uint32_t* d_ws = nullptr;
    if (arena_plan(h, ARENA_SCORE, [&](ArenaPlan& ap) {
        d_pairs = ap.arr<ScorePair>((size_t)B); d_sel = ap.arr<int32_t>((size_t)B); d_warp = ap.arr<ScoreWarp>((size_t)B); d_sums = ap.arr<ScoreSums>((size_t)B);
        d_cqa = ap.arr<int32_t>((size_t)sa.total * D); d_cqb = ap.arr<int32_t>((size_t)sb.total * D);
        d_pa = ap.arr<int32_t>((size_t)path_cap); d_pb = ap.arr<int32_t>((size_t)path_cap);
        d_rev = ap.arr<int32_t>((size_t)rev_total); d_ws = ap.arr<uint32_t>((size_t)ws_words);
    })) return -1;
    HIPCHK(h, hipMemcpyAsync(d_cqa, sa.cq, (size_t)sa.total * D * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    HIPCHK(h, hipMemcpyAsync(d_cqb, sb.cq, (size_t)sb.total * D * sizeof(int32_t), hipMemcpyDeviceToDevice, h->stream));
    if (upload(h, d_pairs, pairs)) return -1;
    if (!sel.empty() && upload(h, d_sel, sel)) return -1;
    region_begin(h, "total");
    std::vector<ScoreWarp> warp((size_t)B);
    if (!linear) {
        // the stream orders the passes, which reuse the workspace; inside a pass every run's distances, then every run's warp
        for (size_t l0 = 0; l0 < launches.size();) {
            size_t l1 = l0;
            while (l1 < launches.size() && launches[l1].pass == launches[l0].pass) ++l1;
            for (size_t li = l0; li < l1; ++li) {
                const Launch& l = launches[li];
                KScope ks(h, "score_dist", 3.0 * l.cells * D, 4.0 * l.cells);
                if (launch_score_dist(d_cqa, d_cqb, D, d_pairs, d_sel + l.first, l.n, l.rm, l.max_steps, d_ws, h->stream))
                    return fail(h, "ev_score: the distance kernel does not build this shape");
            }
            HIPCHK(h, hipGetLastError());
            for (size_t li = l0; li < l1; ++li) {
                const Launch& l = launches[li];
                KScope ks(h, "score_dtw", 8.0 * l.cells, 4.5 * l.cells);
                if (launch_score_dtw(l.rm, d_pairs, d_sel + l.first, l.n, d_ws, d_ws, d_rev, d_warp, h->stream))
                    return fail(h, "ev_score: the warp kernel does not build this shape");
            }
            HIPCHK(h, hipGetLastError());
            l0 = l1;
        }
        HIPCHK(h, hipMemcpyAsync(warp.data(), d_warp, (size_t)B * sizeof(ScoreWarp), hipMemcpyDeviceToHost, h->stream));
        HIPCHK(h, hipStreamSynchronize(h->stream));      // the paths' lengths lay the result out
        int64_t off = 0;
        for (int b = 0; b < B; ++b) {
            ScorePair& p = pairs[(size_t)b];
            if (warp[(size_t)b].K < std::max(p.Ta, p.Tb) || warp[(size_t)b].K > p.Ta + p.Tb - 1) {
                (void)call_end(h);      // the call is closed; its workspace has been rewritten, so no result is valid after this failure
                return fail(h, "ev_score: pair %d: the backtrack returned a path of %d cells for %d x %d frames", b, warp[(size_t)b].K, p.Ta, p.Tb);
            }
            p.K = warp[(size_t)b].K; p.path_off = off; off += p.K;
            poffs[(size_t)b + 1] = off;
        }
        if (upload(h, d_pairs, pairs)) return -1;
    }
    {
        KScope ks(h, "score_sums", 0.0, 16.0 * (double)poffs[(size_t)B]);
        launch_score_sums(d_pairs, B, linear ? 1 : 0, d_cqa, d_cqb, D, d_rev, d_warp, f0 ? sa.f0 : nullptr, f0 ? sb.f0 : nullptr, d_pa, d_pb, d_sums, h->stream);
    }
    HIPCHK(h, hipGetLastError());
    std::vector<ScoreSums> sums((size_t)B);
    HIPCHK(h, hipMemcpyAsync(sums.data(), d_sums, (size_t)B * sizeof(ScoreSums), hipMemcpyDeviceToHost, h->stream));
    if (call_end(h)) return -1;
    // from here on nothing fails: the previous result is replaced
    ScoreState& st = h->score;
    const size_t nb = (size_t)B;
    st.sum_dist.resize(nb); st.K.resize(nb); st.sum_c.resize(nb); st.sum_c2.resize(nb); st.mcd.resize(nb); st.rmse.resize(nb); st.bias.resize(nb);
    st.vuv.resize(nb); st.warp.resize(nb);
    for (auto& c : st.cnt) c.resize(nb);
    for (size_t b = 0; b < nb; ++b) {
        const ScoreSums& g = sums[b];
        const int K = pairs[b].K;
        const int32_t cnt[7] = {g.n_diag, g.n_a, g.n_b, g.n_vv, g.n_vu, g.n_uv, g.n_uu};
        for (int k = 0; k < 7; ++k) st.cnt[k][b] = cnt[k];
        st.sum_dist[b] = g.sum_dist; st.K[b] = K; st.sum_c[b] = g.sum_c; st.sum_c2[b] = g.sum_c2;
        st.mcd[b] = (10.0 / log(10.0)) * sqrt(2.0) * ((double)g.sum_dist / 65536.0) / (double)K;
        st.rmse[b] = g.n_vv ? sqrt(g.sum_c2 / (double)g.n_vv) : (double)NAN;
        st.bias[b] = g.n_vv ? g.sum_c / (double)g.n_vv : (double)NAN;
        st.vuv[b] = (double)(g.n_vu + g.n_uv) / (double)K;
        st.warp[b] = (double)(g.n_a + g.n_b) / (double)K;
    }
    st.lens_a = sa.lens; st.lens_b = sb.lens; st.nonf_a = sa.nonf; st.nonf_b = sb.nonf; st.path_offs.swap(poffs);
    reset_result(out);
    out->batch = B; out->n_ceps = D; out->linear = linear ? 1 : 0; out->total_frames_a = sa.total; out->total_frames_b = sb.total;
    out->sum_dist = st.sum_dist.data(); out->path_len = st.K.data();
    out->n_diag = st.cnt[0].data(); out->n_a = st.cnt[1].data(); out->n_b = st.cnt[2].data();
    out->n_vv = st.cnt[3].data(); out->n_vu = st.cnt[4].data(); out->n_uv = st.cnt[5].data(); out->n_uu = st.cnt[6].data();
    out->sum_c = st.sum_c.data(); out->sum_c2 = st.sum_c2.data(); out->mcd_db = st.mcd.data(); out->f0_rmse_cents = st.rmse.data();
    out->f0_bias_cents = st.bias.data(); out->vuv_error = st.vuv.data(); out->warp = st.warp.data();
    out->lens_a = st.lens_a.data(); out->lens_b = st.lens_b.data(); out->nonfinite_a = st.nonf_a.data(); out->nonfinite_b = st.nonf_b.data();
    out->path_offsets = st.path_offs.data(); out->path_a = d_pa; out->path_b = d_pb; out->cq_a = d_cqa; out->cq_b = d_cqb;
    return 0;
}

// ------------------------------------------------------------------- per-kernel test entry points of the utilities (include/evhip_ops.h)
// Each builds its kernel's tables from per-utterance HOST arrays (no struct crosses the boundary), launches on the caller's stream and waits for it
// before the tables go.  -2: a rejected argument or shape; -1: a runtime failure.
int ev_op_stft_mel(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, const float* mel_basis, const float* window, int n_fft, int hop,
                   int n_mels, float mel_clip, float energy_floor, float energy_mean, float energy_std, float* mel, float* energy, float* mag,
                   void* stream) {
    if (!wav || !wav_lens || !mel_basis || !mel || !energy || B < 1 || B > 65535 || !stft_shape_ok(n_fft, hop, n_mels)) return -2;
    FrameGrid g;
    if (frame_grid_layout(B, wav_lens, n_fft / 2 + 1, hop, 64, g)) return -2;
    DevMem basis, melT;
    DevTable t;
    const size_t so = t.add(g.seqs), to = t.add(g.tiles);
    if (features_upload_tables(nullptr, n_fft, n_mels, mel_basis, window, basis, melT) || t.commit()) return -1;
    const StftParams p{stft_front(wav, wav_is_i16, t.at<StftSeq>(so), t.at<StftTile>(to), g.tiles.size(), basis.get(), n_fft, hop), melT.as<float>(),
                       n_mels, mel_clip, energy_floor, energy_mean, energy_std, mel, energy, mag};
    return op_finish(launch_stft_mel(p, (hipStream_t)stream), (hipStream_t)stream);
}

int ev_op_stft_gain(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, const float* window, int n_fft, int hop, const float* bias,
                    const float* strengths, void* spec_hi, void* spec_lo, float* mag, void* stream) {
    if (!wav || !wav_lens || B < 1 || B > 65535 || !denoise_shape_ok(n_fft, hop)) return -2;
    if (!mag && (!bias || !strengths || !spec_hi || !spec_lo)) return -2;
    FrameGrid g;
    if (frame_grid_layout(B, wav_lens, n_fft / 2 + 1, hop, 64, g)) return -2;
    std::vector<uint16_t> hb(stft_basis_halfs(n_fft));
    stft_pack_basis(n_fft, window, hb.data());
    DevTable t;
    const size_t so = t.add(g.seqs), to = t.add(g.tiles), bo = t.add(hb);
    if (t.commit()) return -1;
    StftGainParams p{stft_front(wav, wav_is_i16, t.at<StftSeq>(so), t.at<StftTile>(to), g.tiles.size(), t.at<char>(bo), n_fft, hop)};
    p.bias = bias; p.strengths = strengths; p.spec_hi = (uint16_t*)spec_hi; p.spec_lo = (uint16_t*)spec_lo;
    p.mag = mag; p.mag_frames = EV_ALIGN_MAX_FRAMES;
    return op_finish(launch_stft_gain(p, (hipStream_t)stream), (hipStream_t)stream);
}

int ev_op_istft(const void* spec_hi, const void* spec_lo, int B, const int32_t* frames, const float* window, int n_fft, int hop, float* out,
                int16_t* out_i16, void* stream) {
    if (!spec_hi || !spec_lo || !frames || !out || B < 1 || B > 65535 || !denoise_shape_ok(n_fft, hop)) return -2;
    for (int b = 0; b < B; ++b) if (frames[b] < 1 || frames[b] > EV_ALIGN_MAX_FRAMES) return -2;
    std::vector<IstftSeq> seqs; std::vector<StftTile> tiles;
    istft_layout(B, frames, n_fft, hop, seqs, tiles);
    if (tiles.empty()) return 0;      // one frame per utterance: no output
    std::vector<uint16_t> hi(istft_basis_halfs(n_fft, hop));
    std::vector<float> he(istft_envelope_floats(n_fft, hop));
    istft_pack_basis(n_fft, hop, window, hi.data());
    istft_pack_envelope(n_fft, hop, window, he.data());
    DevTable t;
    const size_t so = t.add(seqs), to = t.add(tiles), bo = t.add(hi), eo = t.add(he);
    if (t.commit()) return -1;
    IstftParams p{};
    p.spec_hi = (const uint16_t*)spec_hi; p.spec_lo = (const uint16_t*)spec_lo; p.seqs = t.at<IstftSeq>(so); p.tiles = t.at<StftTile>(to);
    p.n_tiles = (int)tiles.size(); p.ibasis = t.at<char>(bo); p.env = t.at<float>(eo);
    p.n_fft = n_fft; p.hop = hop; p.R = n_fft / hop; p.k_pad = denoise_k_pad(n_fft); p.out = out; p.out_i16 = out_i16;
    return op_finish(launch_istft_ola(p, (hipStream_t)stream), (hipStream_t)stream);
}

int ev_op_pitch_yin(const void* wav, int wav_is_i16, int B, const int64_t* wav_lens, int sample_rate, int hop, int win, float f_min, float f_max,
                    float threshold, float silence_rms, float* f0_hz, float* aperiodicity, int32_t* tau, void* stream) {
    if (!wav || !wav_lens || !f0_hz || !aperiodicity || B < 1 || B > 65535) return -2;
    ev_pitch_config c;
    ev_default_pitch_config(&c);
    c.sample_rate = sample_rate; c.hop = hop; c.win = win; c.f_min = f_min; c.f_max = f_max; c.threshold = threshold; c.silence_rms = silence_rms;
    int tau_min = 0, tau_max = 0;
    if (pitch_check_config(nullptr, "ev_op_pitch_yin", c, &tau_min, &tau_max)) return -2;
    FrameGrid g;
    if (frame_grid_layout(B, wav_lens, 1, hop, PITCH_TF, g)) return -2;
    DevTable t;
    const size_t so = t.add(g.seqs), to = t.add(g.tiles);
    if (t.commit()) return -1;
    PitchParams p = pitch_params(c, tau_min, tau_max);
    p.wav = wav; p.wav_is_i16 = wav_is_i16 != 0; p.seqs = t.at<StftSeq>(so); p.tiles = t.at<StftTile>(to); p.n_tiles = (int)g.tiles.size();
    p.f0 = f0_hz; p.ap = aperiodicity; p.tau = tau;
    return op_finish(launch_pitch_yin(p, (hipStream_t)stream), (hipStream_t)stream);
}
int ev_op_pitch_fill(const float* f0_hz, int B, const int32_t* frames, float pitch_mean, float pitch_std, float* pitch, void* stream) {
    if (!f0_hz || !frames || !pitch || pitch == f0_hz || B < 1 || B > 65535) return -2;
    if (!std::isfinite(pitch_mean) || !std::isfinite(pitch_std) || !(pitch_std > 0.f)) return -2;
    // the frame grid of utterances of frames - 1 samples at hop 1: T = frames.  The kernel reads a sequence's frame offset and count only.
    std::vector<int64_t> lens((size_t)B);
    for (int b = 0; b < B; ++b) lens[(size_t)b] = (int64_t)frames[b] - 1;
    FrameGrid g;
    if (frame_grid_layout(B, lens.data(), 0, 1, PITCH_TF, g)) return -2;
    DevTable t;
    const size_t so = t.add(g.seqs);
    if (t.commit()) return -1;
    launch_pitch_fill(f0_hz, t.at<StftSeq>(so), B, pitch_mean, pitch_std, pitch, (hipStream_t)stream);
    return op_finish(0, (hipStream_t)stream);
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
    DevMem tab;
    if (resample_upload_table(up, half, ht, tab)) return -1;
    DevTable t;
    const size_t so = t.add(seqs), to = t.add(tiles);
    if (t.commit()) return -1;
    return op_finish(resample_launch(wav, wav_is_i16 != 0, up, down, half, tab.as<float>(), t.at<ResampleSeq>(so), t.at<ResampleTile>(to), (int)tiles.size(),
                                     seqs[B - 1].in_off + seqs[B - 1].len, y, (hipStream_t)stream), (hipStream_t)stream);
}
int ev_op_trim(const float* y, int B, const int64_t* lens, float trim_frac, int trim_pad, float* out, int64_t* out_lens, int64_t* trim_start,
               int64_t* trim_end, void* stream) {
    if (!y || !lens || !out || !out_lens || !trim_start || !trim_end || out == y || B < 1 || B > 65535) return -2;
    if (!std::isfinite(trim_frac) || !(trim_frac > 0.f) || !(trim_frac < 1.f) || trim_pad < 0) return -2;
    std::vector<ResampleSeq> seqs; std::vector<ResampleTile> tiles;      // y as the output of a 1 : 1 conversion (the tiles are not used)
    if (resample_layout(B, lens, 1, 1, 2 * (int64_t)trim_pad, seqs, tiles)) return -2;
    DevTable t;
    const size_t cb = 2 * (size_t)B * sizeof(int64_t), so = t.add(seqs), co = t.room(cb), to = t.room((size_t)B * sizeof(TrimSeq));
    if (t.commit()) return -1;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int64_t> cuts(2 * (size_t)B);
    std::vector<TrimSeq> ts;
    launch_trim_scan(y, t.at<ResampleSeq>(so), B, trim_frac, t.at<int64_t>(co), s);
    if (op_finish(0, s)) return -1;
    if (hipMemcpy(cuts.data(), t.at<int64_t>(co), cb, hipMemcpyDeviceToHost) != hipSuccess) return -1;
    const int64_t longest = trim_plan(B, seqs, cuts.data(), trim_pad, ts, out_lens, nullptr, trim_start, trim_end);
    if (hipMemcpy(t.at<TrimSeq>(to), ts.data(), (size_t)B * sizeof(TrimSeq), hipMemcpyHostToDevice) != hipSuccess) return -1;
    launch_trim_gather(y, t.at<TrimSeq>(to), B, longest, trim_pad, out, s);
    return op_finish(0, s);
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
    DevTable t;
    const size_t cb = 2 * (size_t)S * sizeof(int64_t);
    const size_t so = t.add(segs), co = t.room(cb), po = t.room((size_t)S * sizeof(float)), qo = t.room((size_t)n_part * sizeof(float));
    if (t.commit()) return -1;
    hipStream_t s = (hipStream_t)stream;
    std::vector<int64_t> cuts(2 * (size_t)S);
    launch_stitch_peak(wav, t.at<StitchSeg>(so), S, max_len, t.at<float>(qo), s);
    launch_stitch_edges(wav, t.at<StitchSeg>(so), S, t.at<float>(qo), trim_frac, trim_abs, t.at<float>(po), t.at<int64_t>(co), s);
    int rc = op_finish(0, s);
    if (rc == 0 && (hipMemcpy(cuts.data(), t.at<int64_t>(co), cb, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(peak, t.at<float>(po), (size_t)S * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
    if (rc == 0) for (int i = 0; i < S; ++i) { first[i] = cuts[2 * (size_t)i]; last[i] = cuts[2 * (size_t)i + 1]; }
    return rc;
}
int ev_op_flac_encode(const void* pcm, int pcm_is_i16, int B, const int64_t* lens, const ev_flac_config* cfg, uint8_t* slots, int32_t* sizes,
                      uint8_t* kind, uint8_t* porder, void* stream) {
    ev_flac_config c;
    if (cfg) c = *cfg; else ev_default_flac_config(&c);
    if (!pcm || !lens || !slots || !sizes || !kind || !porder || B < 1 || B > 65535 || c.struct_size != sizeof(ev_flac_config)) return -2;
    int sr_code = 0, bs_code = 0, at = 0;
    FlacPlan plan;
    if (flac_check_config(c, &sr_code, &bs_code) != FLAC_OK || (reinterpret_cast<uintptr_t>(slots) & 3)) return -2;
    if (flac_plan(B, lens, c.block_size, plan, &at) != LEN_OK) return -2;
    const size_t NF = plan.frames.size(), sb = NF * sizeof(int32_t);
    DevTable t;
    const size_t fo = t.add(plan.frames), so = t.room(sb), d_o = t.room(sb);
    if (t.commit()) return -1;
    hipStream_t s = (hipStream_t)stream;
    FlacParams fp = flac_params(c, sr_code, bs_code);
    fp.pcm = pcm; fp.pcm_is_i16 = pcm_is_i16 != 0; fp.frames = t.at<FlacFrame>(fo); fp.scratch = slots; fp.sizes = t.at<int32_t>(so); fp.desc = t.at<uint32_t>(d_o);
    std::vector<uint32_t> desc(NF);
    int rc = op_finish(launch_flac_encode(fp, (int64_t)NF, s), s);
    if (rc == 0 && (hipMemcpy(sizes, fp.sizes, sb, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(desc.data(), fp.desc, sb, hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
    if (rc == 0) for (size_t f = 0; f < NF; ++f) { kind[f] = (uint8_t)(desc[f] & 0xFFu); porder[f] = (uint8_t)(desc[f] >> 8 & 0xFFu); }
    return rc;
}
int ev_op_flac_lpc(const void* pcm, int pcm_is_i16, int B, const int64_t* lens, const ev_flac_config* cfg, int max_lpc_order, int qlp_precision, int64_t* R,
                   int32_t* shift, int32_t* coef, void* stream) {
    ev_flac_config c;
    if (cfg) c = *cfg; else ev_default_flac_config(&c);
    if (!pcm || !lens || !R || !shift || !coef || B < 1 || B > 65535 || c.struct_size != sizeof(ev_flac_config)) return -2;
    if (max_lpc_order < 0 || max_lpc_order > FLAC_LPC_MAX_ORDER || qlp_precision < 5 || qlp_precision > 15) return -2;
    int sr_code = 0, bs_code = 0, at = 0;
    FlacPlan plan;
    if (flac_check_config(c, &sr_code, &bs_code) != FLAC_OK) return -2;
    if (flac_plan(B, lens, c.block_size, plan, &at) != LEN_OK) return -2;
    const size_t NF = plan.frames.size(), rb = NF * 13 * sizeof(int64_t), sb = NF * FLAC_LPC_MAX_ORDER * sizeof(int32_t), cb = sb * FLAC_LPC_MAX_ORDER;
    DevTable t;
    const size_t fo = t.add(plan.frames), ro = t.room(rb), so = t.room(sb), co = t.room(cb);
    if (t.commit()) return -1;
    hipStream_t s = (hipStream_t)stream;
    FlacParams fp = flac_params(c, sr_code, bs_code);
    fp.pcm = pcm; fp.pcm_is_i16 = pcm_is_i16 != 0; fp.frames = t.at<FlacFrame>(fo);
    int rc = op_finish(launch_flac_lpc_analysis(fp, FlacLpc{max_lpc_order, qlp_precision}, (int64_t)NF, t.at<int64_t>(ro), t.at<int32_t>(so), t.at<int32_t>(co), s), s);
    if (rc == 0 && (hipMemcpy(R, t.at<int64_t>(ro), rb, hipMemcpyDeviceToHost) != hipSuccess || hipMemcpy(shift, t.at<int32_t>(so), sb, hipMemcpyDeviceToHost) != hipSuccess ||
                    hipMemcpy(coef, t.at<int32_t>(co), cb, hipMemcpyDeviceToHost) != hipSuccess)) rc = -1;
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
    DevTable t;
    const size_t mo = t.add(ms), d_o = t.add(docs), to = t.add(tiles), fo = t.add(tab, (size_t)F * sizeof(float));
    if (t.commit()) return -1;
    return op_finish(launch_stitch_mix(wav, t.at<StitchMixSeg>(mo), t.at<StitchDoc>(d_o), t.at<StitchTile>(to), (int64_t)tiles.size(), t.at<float>(fo), F, out,
                                       out_i16, (hipStream_t)stream), (hipStream_t)stream);
}

// The AlignSeq table of the two aligner kernels, from per-utterance host arrays: 0, or -2
static int op_align_table(int B, const int32_t* tok_row, const int32_t* tokens, const int32_t* frm_row, const int32_t* frames, const int64_t* lp_off,
                          const int64_t* tok_packed, const int64_t* frm_packed, const int64_t* bits_off, bool mas, std::vector<AlignSeq>& tab, int* max_tok,
                          int* max_frm) {
    if (B <= 0 || B > 65535 || !tokens || !frames || !lp_off) return -2;
    tab.resize((size_t)B);
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
    return 0;
}
int ev_op_align_score(const float* text, const float* feats, int C, int B, const int32_t* tok_row, const int32_t* tokens, const int32_t* frm_row,
                      const int32_t* frames, const int64_t* lp_off, float* log_p, void* stream) {
    if (C <= 0 || C % 32 || !tok_row || !frm_row || !log_p) return -2;      // channels are staged 32 at a time
    std::vector<AlignSeq> tab; int max_tok = 0, max_frm = 0;
    if (op_align_table(B, tok_row, tokens, frm_row, frames, lp_off, nullptr, nullptr, nullptr, false, tab, &max_tok, &max_frm)) return -2;
    DevTable t;
    const size_t o = t.add(tab);
    if (t.commit()) return -1;
    launch_align_score(text, feats, C, t.at<AlignSeq>(o), B, max_frm, log_p, (hipStream_t)stream);
    return op_finish(0, (hipStream_t)stream);
}
int ev_op_align_mas(const float* log_p, int B, const int32_t* tokens, const int32_t* frames, const int64_t* lp_off, const int64_t* tok_packed,
                    const int64_t* frm_packed, const int64_t* bits_off, uint32_t* bits, const float* pitch_frames, const float* energy_frames,
                    int64_t* dur, float* pitch_tok, float* energy_tok, float* score, void* stream) {
    if (!log_p || !tok_packed || !frm_packed || !bits_off || !bits || !dur || !score) return -2;
    if ((pitch_frames && !pitch_tok) || (energy_frames && !energy_tok)) return -2;
    std::vector<AlignSeq> tab; int max_tok = 0, max_frm = 0;
    if (op_align_table(B, nullptr, tokens, nullptr, frames, lp_off, tok_packed, frm_packed, bits_off, true, tab, &max_tok, &max_frm)) return -2;
    DevTable t;
    const size_t o = t.add(tab);
    if (t.commit()) return -1;
    launch_align_mas(log_p, t.at<AlignSeq>(o), B, max_tok, bits, pitch_frames, energy_frames, dur, pitch_tok, energy_tok, score, (hipStream_t)stream);
    return op_finish(0, (hipStream_t)stream);
}

int ev_op_limit_peak(const void* wav, int wav_is_i16, int B, const int64_t* lens, const float* gains, float ceiling, float* r, float* sample_peak,
                     float* true_peak, int64_t* nonfinite, void* stream) {
    if (!wav || !lens || !sample_peak || !true_peak || !nonfinite || B < 1 || B > 65535 || !(ceiling > 0.f && ceiling <= 1.f)) return -2;
    LimitPlan plan;
    int at = 0;
    if (limit_plan(B, lens, plan, &at) != LEN_OK || limit_bad_gain(B, gains) >= 0) return -2;
    double tab[LIMIT_TAB];
    std::vector<double> win;
    if (limit_tables(0, tab, win)) return -1;
    const size_t NT = plan.tiles.size();
    DevTable t;
    const size_t to = t.add(plan.tiles), ho = t.add(tab, sizeof tab), go = gains ? t.add(gains, (size_t)B * sizeof(float)) : 0, oo = t.room(NT * sizeof(LimitPeakOut));
    if (t.commit()) return -1;
    hipStream_t s = (hipStream_t)stream;
    std::vector<LimitPeakOut> outs(NT);
    int rc = op_finish(launch_limit_peak(wav, wav_is_i16 != 0, gains ? t.at<float>(go) : nullptr, t.at<LimitTile>(to), (int64_t)NT, t.at<double>(ho), ceiling, r,
                                         t.at<LimitPeakOut>(oo), s), s);
    if (rc == 0 && hipMemcpy(outs.data(), t.at<LimitPeakOut>(oo), NT * sizeof(LimitPeakOut), hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    if (rc == 0) limit_fold_peaks(plan, B, outs.data(), sample_peak, true_peak, nonfinite);
    return rc;
}
int ev_op_limit_apply(const void* wav, int wav_is_i16, int B, const int64_t* lens, const float* gains, const float* r, int lookahead, int hold, float* out,
                      int16_t* out_i16, float* s_out, float* min_gain, int64_t* limited, void* stream) {
    if (!wav || !lens || !r || !out || !min_gain || !limited || B < 1 || B > 65535) return -2;
    if (lookahead < 0 || lookahead > EV_LIMIT_MAX_LOOKAHEAD || hold < 0 || hold > EV_LIMIT_MAX_HOLD) return -2;
    LimitPlan plan;
    int at = 0;
    if (limit_plan(B, lens, plan, &at) != LEN_OK || limit_bad_gain(B, gains) >= 0) return -2;
    double tab[LIMIT_TAB];
    std::vector<double> win;
    if (limit_tables(lookahead, tab, win)) return -1;
    const size_t NT = plan.tiles.size();
    DevTable t;
    const size_t to = t.add(plan.tiles), wo = t.add(win), go = gains ? t.add(gains, (size_t)B * sizeof(float)) : 0, oo = t.room(NT * sizeof(LimitApplyOut));
    if (t.commit()) return -1;
    hipStream_t s = (hipStream_t)stream;
    std::vector<LimitApplyOut> outs(NT);
    int rc = op_finish(launch_limit_apply(wav, wav_is_i16 != 0, gains ? t.at<float>(go) : nullptr, t.at<LimitTile>(to), (int64_t)NT, r, t.at<double>(wo), lookahead, hold,
                                          out, out_i16, s_out, t.at<LimitApplyOut>(oo), s), s);
    if (rc == 0 && hipMemcpy(outs.data(), t.at<LimitApplyOut>(oo), NT * sizeof(LimitApplyOut), hipMemcpyDeviceToHost) != hipSuccess) rc = -1;
    if (rc == 0) limit_fold_gains(plan, B, outs.data(), min_gain, limited);
    return rc;
}

}  // extern "C"
