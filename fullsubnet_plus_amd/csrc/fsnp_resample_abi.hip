// fsnp_resample_abi.hip - the entry points of include/fsnp_resample.h that do not run the model (fsnp_enhance_wave_rate sits next to
// the call it extends, in fsnp_stft_abi.hip), the pair arithmetic and the handle's table cache.  Host code only; kernels: resample.hip.
#include <climits>

#include "fsnp_handle.h"
#include "pcm.h"
#include "resample.h"

namespace fsnp {

int resample_plan(const char* where, int from_rate, int to_rate, ResamplePlan& plan) {
    if (from_rate <= 0 || to_rate <= 0) {
        set_error("%s: sample rates must be positive (from %d Hz to %d Hz)", where, from_rate, to_rate);
        return 2;
    }
    int a = from_rate, b = to_rate;
    while (b) { const int r = a % b; a = b; b = r; }
    const long up = to_rate / a, down = from_rate / a;
    if (up > kResampleMaxRatio || down > kResampleMaxRatio) {
        set_error("%s: %d Hz -> %d Hz is the ratio %ld : %ld; max(up, down) is limited to %d (the filter has %d max(up, down) taps on "
                  "either side of its centre)", where, from_rate, to_rate, up, down, kResampleMaxRatio, kResampleZ);
        return 2;
    }
    plan.up = (int)up;
    plan.down = (int)down;
    plan.half = kResampleZ * (int)(up > down ? up : down);
    plan.J = plan.half / plan.up;
    plan.tpp = plan.J + (plan.half + plan.up - 1) / plan.up + 1;
    return 0;
}

// The table of a pair, cached in the handle and - on first use - uploaded in stream order on s from the handle's own host copy.
// Callers are between order_after_last_forward and mark_forward_done, which is what orders a later call on another stream behind
// the upload.  `room`: how many new pairs this call may still add, checked by resample_room before anything is enqueued.
static const ResampleCached* find_table(const fsnp_handle* h, const ResamplePlan& p) {
    for (const ResampleCached& c : h->resample)
        if (c.plan.up == p.up && c.plan.down == p.down) return &c;
    return nullptr;
}
int resample_room(const fsnp_handle* h, const char* where, const ResamplePlan* plans, int count) {
    int fresh = 0;
    for (int i = 0; i < count; ++i) {
        if (plans[i].up == plans[i].down || find_table(h, plans[i])) continue;
        bool seen = false;
        for (int j = 0; j < i; ++j) seen = seen || (plans[j].up == plans[i].up && plans[j].down == plans[i].down);
        fresh += seen ? 0 : 1;
    }
    if ((int)h->resample.size() + fresh > kResampleMaxPairs) {
        set_error("%s: this handle already keeps the tables of %d (up, down) pairs, the most it holds (they are never evicted: launches "
                  "in flight may read them); the pair %d : %d needs another handle", where, (int)h->resample.size(),
                  plans[count - 1].up, plans[count - 1].down);
        return 2;
    }
    return 0;
}
int resample_table(fsnp_handle* h, const ResamplePlan& p, hipStream_t s, ResampleTable& t) {
    t = ResampleTable{nullptr, p.up, p.down, p.half, p.J, p.tpp};
    if (p.up == p.down) return 0;                                  // equal rates: no filter, no table
    const ResampleCached* c = find_table(h, p);
    if (!c) {
        h->resample.reserve(kResampleMaxPairs);                    // (entries never move: uploads in flight read their host copies)
        h->resample.emplace_back();
        ResampleCached& n = h->resample.back();
        n.plan = p;
        n.host.resize((size_t)p.up * p.tpp);
        resample_build_table(p, n.host.data());
        const size_t bytes = n.host.size() * sizeof(float);
        hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&n.dev), bytes, s);
        if (e == hipSuccess) e = hipMemcpyAsync(n.dev, n.host.data(), bytes, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) {
            if (n.dev) (void)hipFreeAsync(n.dev, s);
            h->resample.pop_back();
            set_error("resample table %d : %d: %s", p.up, p.down, hipGetErrorString(e));
            return 4;
        }
        c = &n;
    }
    t.taps = c->dev;
    return 0;
}

}  // namespace fsnp

extern "C" {

int fsnp_resample_plan(int32_t from_rate, int32_t to_rate, int32_t* up, int32_t* down, int32_t* half) {
    ResamplePlan p{};
    if (const int rc = resample_plan("fsnp_resample_plan", from_rate, to_rate, p)) return rc;
    if (up) *up = p.up;
    if (down) *down = p.down;
    if (half) *half = p.half;
    return 0;
}

int fsnp_resample_length(int32_t from_rate, int32_t to_rate, int64_t n, int64_t* n_out) {
    if (!n_out) { set_error("fsnp_resample_length: null argument"); return 1; }
    ResamplePlan p{};
    if (const int rc = resample_plan("fsnp_resample_length", from_rate, to_rate, p)) return rc;
    if (n < 0 || n > INT64_MAX / (2 * kResampleMaxRatio)) { set_error("fsnp_resample_length: n = %lld out of range", (long long)n); return 2; }
    *n_out = resample_length(p, n);
    return 0;
}

int fsnp_resample_taps(int32_t from_rate, int32_t to_rate, float* taps, int32_t capacity) {
    if (!taps) { set_error("fsnp_resample_taps: null argument"); return 1; }
    ResamplePlan p{};
    if (const int rc = resample_plan("fsnp_resample_taps", from_rate, to_rate, p)) return rc;
    if (capacity < 2 * p.half + 1) {
        set_error("fsnp_resample_taps: capacity %d below the 2 half + 1 = %d taps of %d : %d", (int)capacity, 2 * p.half + 1, p.up, p.down);
        return 2;
    }
    resample_build_taps(p, taps);
    return 0;
}

int fsnp_resample_pcm(fsnp_handle* h, const void* in, int32_t in_format, int64_t in_stride, int64_t in_step, void* out,
                      int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch, int32_t max_samples,
                      int32_t from_rate, int32_t to_rate, int32_t* clipped, void* hip_stream) {
    const char* where = "fsnp_resample_pcm";
    if (!h || !in || !out) { set_error("%s: null argument", where); return 1; }
    if (const int rc = check_sample_format(where, "input", in_format, in_step, false)) return rc;
    if (const int rc = check_sample_format(where, "output", out_format, out_step, true)) return rc;
    if (batch <= 0 || max_samples <= 0) { set_error("%s: empty input", where); return 2; }
    ResamplePlan p{};
    if (const int rc = resample_plan(where, from_rate, to_rate, p)) return rc;
    const long long cols = resample_length(p, max_samples);
    if (cols > INT_MAX - 2 * kResampleBlock) { set_error("%s: %lld output samples per row do not fit 32 bits", where, cols); return 2; }
    for (int b = 0; samples && b < batch; ++b)
        if (samples[b] < 0 || samples[b] > max_samples) {
            set_error("%s: row %d: %d samples outside [0, %d]", where, b, (int)samples[b], (int)max_samples);
            return 2;
        }
    if (const int rc = resample_room(h, where, &p, 1)) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    if (order_after_last_forward(h, s)) return 4;
    // FSNP_SAMPLE_S16_PEAK: fp32 rows and the rows' maxima in the io area first, as in fsnp_enhance_wave_pcm
    const size_t stage_bytes = align_up((size_t)batch * cols * 4, 256);
    if (out_format == FSNP_SAMPLE_S16_PEAK && ensure_io(h, stage_bytes + (size_t)batch * 4, s)) return 4;
    ResampleTable t{};
    if (const int rc = resample_table(h, p, s, t)) return rc;
    PcmOut o{out, (long)out_stride, (long)out_step, out_format, out_format == FSNP_SAMPLE_S16 ? clipped : nullptr, nullptr};
    if (clipped) FSNP_HIP_CHECK(hipMemsetAsync(clipped, 0, (size_t)batch * 4, s));
    if (out_format == FSNP_SAMPLE_S16_PEAK) {
        unsigned* peak = reinterpret_cast<unsigned*>(h->io + stage_bytes);
        FSNP_HIP_CHECK(hipMemsetAsync(peak, 0, (size_t)batch * 4, s));
        o = PcmOut{h->io, (long)cols, 1, kPcmPeak, nullptr, peak};
    }
    launch_resample(PcmIn{in, (long)in_stride, (long)in_step, in_format}, o, t, batch, samples, max_samples, (int)cols, false, s);
    if (out_format == FSNP_SAMPLE_S16_PEAK)
        launch_pcm_peak_scale(reinterpret_cast<const float*>(h->io), cols, o.peak, PcmOut{out, (long)out_stride, (long)out_step, kPcmS16, nullptr, nullptr},
                              batch, (int)cols, s);
    FSNP_HIP_CHECK(hipGetLastError());
    return mark_forward_done(h, s);
}

int fsnp_reserve_rate(fsnp_handle* h, int32_t max_batch, int32_t max_samples, int32_t sample_rate, int32_t model_rate, void* hip_stream) {
    const char* where = "fsnp_reserve_rate";
    if (!h) { set_error("%s: null handle", where); return 1; }
    if (max_batch <= 0 || max_samples <= 0) { set_error("%s: bad argument", where); return 2; }
    ResamplePlan p[2] = {};
    if (const int rc = resample_plan(where, sample_rate, model_rate, p[0])) return rc;
    if (const int rc = resample_plan(where, model_rate, sample_rate, p[1])) return rc;
    if (h->cfg.output_size != 2) { set_error("%s: the waveform path needs output_size = 2 (this handle: %d)", where, h->cfg.output_size); return 2; }
    const long long max16 = resample_length(p[0], max_samples);
    if (max16 > INT_MAX / 2) { set_error("%s: %lld model-rate samples per clip do not fit", where, max16); return 2; }
    if (const int rc = resample_room(h, where, p, 2)) return rc;
    if (ensure_stft(h)) return 2;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    if (order_after_last_forward(h, s)) return 4;
    const bool same = p[0].up == p[0].down;
    if (ensure_io(h, wave_io(stft_plan(h), max_batch, (int)max16, same ? 0 : max_samples).total, s)) return 4;
    ResampleTable t{};
    for (int i = 0; i < 2; ++i)
        if (const int rc = resample_table(h, p[i], s, t)) return rc;
    return mark_forward_done(h, s);
}

}  // extern "C"
