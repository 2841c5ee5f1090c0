// fsnp_wave_rate_stream_abi.hip - include/fsnp_wave_rate_stream.h: wave sessions at any input sample rate.
//
// A rate session is a wave session between two streaming converters.  It holds an ordinary wave session (default or live) at the
// model's rate, created for max(floor(max_samples up / down) + 1, ceil(half / down)) samples per call, and drives it through wave_push
// and wave_finish (fsnp_handle.h) - the bodies of that session's public entry points - on rows of a workspace of its own; per slot a
// rate record behind the inner record (layout: resample.h, RateArgs).  One push on the caller's stream, nothing allocated, nothing
// synchronised:
//   rate_in_kernel    the model-rate samples ready(P) .. ready(P + c) - 1 of every slot from its input history + the new samples;
//                     history, count and pair advanced
//   wave_push         the inner session on those rows, ready(P + c) - ready(P) as each slot's count (not run when every count is 0:
//                     such a push leaves every inner record as it is)
//   rate_out_kernel   this push's c samples at the caller's rate from the enhanced history + the inner output; history advanced
// finish: rate_in (the last total(L) - ready(L) samples, input clamped), wave_push, wave_finish (the inner session's last D_M samples),
// rate_out over history + both outputs (enhanced clip clamped), both records reset.  The host mirrors every slot's count at the
// caller's rate; the inner session's counts follow from it (resample_ready), so nothing is asked of the device.
#include <algorithm>
#include <climits>
#include <string>
#include <vector>

#include "fsnp_handle.h"
#include "pcm.h"
#include "resample.h"

struct fsnp_wave_rate_stream {
    fsnp_handle* h = nullptr;
    fsnp_wave_stream* inner = nullptr;
    int S = 0, max_samples = 0, model_max = 0, rate = 0, model_rate = 0, n_half = 0;      // n_half: the inner session's n_fft / 2
    ResamplePlan pin{}, pout{};       // caller -> model, model -> caller
    ResampleTable tin{}, tout{};
    long long DM = 0, DR = 0;
    int HI = 0, HE = 0;
    size_t inner_bytes = 0;           // one slot's inner wave-session state
    SlotRecords rec;                  // the slots' rate records behind it
    size_t o_he = 0, o_count = 0;
    unsigned char* ws = nullptr;
    size_t ws_bytes = 0, w_meta = 0, w_xin = 0, w_xout = 0, w_fin = 0;
    long xs = 0, fs = 0;              // floats between the slots' rows of xin / xout, of the inner finish's output
    std::vector<int64_t> samples;     // host mirror of the slots' counts at the caller's rate
    std::vector<int32_t> cm;          // [2 S] scratch of a call: the inner session's counts, the inner finish's slot list
};

namespace {

long long ready_of(const fsnp_wave_rate_stream* r, long long P) { return resample_ready(r->pin.up, r->pin.down, r->pin.half, P); }
long long total_of(const fsnp_wave_rate_stream* r, long long L) { return resample_total(r->pin.up, r->pin.down, L); }

RateArgs rate_args(const fsnp_wave_rate_stream* r) {
    RateArgs a{};
    a.state = r->rec.base; a.stride = r->rec.bytes; a.o_he = r->o_he; a.o_count = r->o_count;
    a.meta = reinterpret_cast<RateMeta*>(r->ws + r->w_meta);
    a.S = r->S; a.HI = r->HI; a.HE = r->HE; a.up = r->pin.up; a.down = r->pin.down; a.half = r->pin.half; a.DM = r->DM; a.DR = r->DR;
    return a;
}
float* ws_floats(const fsnp_wave_rate_stream* r, size_t off) { return reinterpret_cast<float*>(r->ws + off); }

int rate_create(fsnp_handle* h, int32_t slots, int32_t max_samples, int32_t rate, int32_t model_rate, int live, const char* where,
                fsnp_wave_rate_stream** out) {
    if (!h || !out) { set_error("%s: null argument", where); return 1; }
    *out = nullptr;
    ResamplePlan p[2] = {};
    if (const int rc = resample_plan(where, rate, model_rate, p[0])) return rc;
    if (const int rc = resample_plan(where, model_rate, rate, p[1])) return rc;
    if (rate == model_rate) {
        set_error("%s: sample_rate %d Hz is the model's rate: there is nothing to convert, open %s", where, rate,
                  live ? "fsnp_wave_stream_create_live" : "fsnp_wave_stream_create");
        return 2;
    }
    if (max_samples < 1) { set_error("%s: max_samples %d < 1", where, max_samples); return 2; }
    const long long mm = std::max<long long>(resample_push_max(p[0], max_samples), resample_finish_max(p[0]));
    if (mm > INT_MAX / 2) { set_error("%s: max_samples %d at %d Hz is %lld model-rate samples per call: too many", where, max_samples, rate, mm); return 2; }
    if (const int rc = resample_room(h, where, p, 2)) return rc;
    fsnp_wave_stream* inner = nullptr;
    if (const int rc = live ? fsnp_wave_stream_create_live(h, slots, (int)mm, &inner) : fsnp_wave_stream_create(h, slots, (int)mm, &inner)) {
        if (rc == 2) {
            const std::string why = fsnp_last_error();
            set_error("%s: max_samples %d at %d Hz is up to %lld samples per call of the inner wave session at %d Hz (a finish pushes up to "
                      "%d), which was refused: %s", where, max_samples, rate, mm, model_rate, resample_finish_max(p[0]), why.c_str());
        }
        return rc;
    }
    fsnp_wave_rate_stream* r = new fsnp_wave_rate_stream();
    r->h = h; r->inner = inner; r->S = slots; r->max_samples = max_samples; r->model_max = (int)mm; r->rate = rate; r->model_rate = model_rate;
    r->n_half = stft_plan(h).half;
    r->pin = p[0]; r->pout = p[1];
    r->DM = fsnp_wave_stream_delay(inner);
    r->DR = resample_stream_delay(p[0], r->DM);
    r->HI = resample_hist_in(p[0]); r->HE = resample_hist_out(p[0]);
    r->inner_bytes = (size_t)fsnp_wave_stream_state_bytes(inner);
    r->o_he = (size_t)r->HI * 4;
    r->o_count = align_up(r->o_he + (size_t)r->HE * 4, 8);
    const size_t rec_bytes = align_up(r->o_count + 16, 16);
    r->xs = (long)align_up((size_t)mm, 4);
    r->fs = (long)align_up((size_t)r->DM, 4);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t at = o; o = align_up(o + bytes, 256); return at; };
    r->w_meta = take((size_t)slots * sizeof(RateMeta));
    r->w_xin = take((size_t)slots * r->xs * 4);
    r->w_xout = take((size_t)slots * r->xs * 4);
    r->w_fin = take((size_t)slots * r->fs * 4);
    r->ws_bytes = o;
    fsnp::DeviceGuard g(h->device);
    hipError_t e = r->rec.create(rec_bytes, slots);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&r->ws), r->ws_bytes);
    if (e == hipSuccess) e = hipMemset(r->ws, 0, r->ws_bytes);
    int rc = 0;
    if (e != hipSuccess) {
        set_error("%s: %s (rate state %zu bytes x %d slots, workspace %zu bytes)", where, hipGetErrorString(e), rec_bytes, slots, r->ws_bytes);
        rc = 4;
    }
    // both tables now, on the null stream, and waited for: no push on any stream ever meets the first-use upload
    if (!rc) rc = order_after_last_forward(h, nullptr) ? 4 : 0;
    if (!rc) rc = resample_table(h, p[0], nullptr, r->tin);
    if (!rc) rc = resample_table(h, p[1], nullptr, r->tout);
    if (!rc) rc = mark_forward_done(h, nullptr) ? 4 : 0;
    if (!rc && (e = hipDeviceSynchronize()) != hipSuccess) { set_error("%s: %s", where, hipGetErrorString(e)); rc = 4; }
    if (rc) {
        r->rec.free();
        if (r->ws) (void)hipFree(r->ws);
        fsnp_wave_stream_destroy(inner);
        delete r;
        return rc;
    }
    r->samples.assign(slots, 0);
    r->cm.assign(2 * (size_t)slots, 0);
    *out = r;
    return 0;
}

int rate_reset(fsnp_wave_rate_stream* r, const int32_t* slots, int32_t num, void* hip_stream) {
    if (const int rc = fsnp_wave_stream_reset(r->inner, slots, num, hip_stream)) return rc;
    FSNP_ON_DEVICE(r->h);
    if (const int rc = r->rec.reset(slots, num, static_cast<hipStream_t>(hip_stream))) return rc;
    if (!slots) std::fill(r->samples.begin(), r->samples.end(), 0);
    else for (int i = 0; i < num; ++i) r->samples[slots[i]] = 0;
    return 0;
}

}  // namespace

extern "C" {

int fsnp_resample_ready(int32_t from_rate, int32_t to_rate, int64_t n, int64_t* ready) {
    if (!ready) { set_error("fsnp_resample_ready: null argument"); return 1; }
    ResamplePlan p{};
    if (const int rc = resample_plan("fsnp_resample_ready", from_rate, to_rate, p)) return rc;
    if (n < 0 || n > INT64_MAX / (2 * kResampleMaxRatio)) { set_error("fsnp_resample_ready: n = %lld out of range", (long long)n); return 2; }
    *ready = resample_ready(p.up, p.down, p.half, n);
    return 0;
}

int fsnp_wave_rate_stream_create(fsnp_handle* h, int32_t slots, int32_t max_samples, int32_t sample_rate, int32_t model_rate,
                                 fsnp_wave_rate_stream** out) {
    return rate_create(h, slots, max_samples, sample_rate, model_rate, 0, "fsnp_wave_rate_stream_create", out);
}

int fsnp_wave_rate_stream_create_live(fsnp_handle* h, int32_t slots, int32_t max_samples, int32_t sample_rate, int32_t model_rate,
                                      fsnp_wave_rate_stream** out) {
    return rate_create(h, slots, max_samples, sample_rate, model_rate, 1, "fsnp_wave_rate_stream_create_live", out);
}

void fsnp_wave_rate_stream_destroy(fsnp_wave_rate_stream* r) {
    if (!r) return;
    {
        fsnp::DeviceGuard g(r->h->device);
        r->rec.free();
        if (r->ws) (void)hipFree(r->ws);
    }
    fsnp_wave_stream_destroy(r->inner);
    delete r;
}

int fsnp_wave_rate_stream_push_pcm(fsnp_wave_rate_stream* r, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step,
                                   const int32_t* counts, void* out, int32_t out_format, int64_t out_stride, int64_t out_step, int32_t n,
                                   void* hip_stream) {
    const char* where = "fsnp_wave_rate_stream_push_pcm";
    if (!r || !wav || !out) { set_error("%s: null argument", where); return 1; }
    if (const int rc = check_sample_format(where, "input", in_format, wav_step, false)) return rc;
    if (const int rc = check_sample_format(where, "output", out_format, out_step, false)) return rc;
    if (n < 1 || n > r->max_samples) { set_error("%s: n = %d outside [1, max_samples = %d]", where, n, r->max_samples); return 2; }
    SlotCounts c{};
    if (const int rc = read_counts(where, counts, r->S, n, c)) return rc;
    if (const int rc = push_preamble(r->h, where)) return rc;
    std::vector<int32_t>& cm = r->cm;
    int nm = 0;
    for (int b = 0; b < r->S; ++b) {
        cm[b] = (int32_t)(ready_of(r, r->samples[b] + c.v[b]) - ready_of(r, r->samples[b]));
        nm = std::max(nm, (int)cm[b]);
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const RateArgs a = rate_args(r);
    {
        FSNP_ON_DEVICE(r->h);
        launch_rate_in(a, c, 0, PcmIn{wav, (long)wav_stride, (long)wav_step, in_format}, r->tin, ws_floats(r, r->w_xin), r->xs, s);
    }
    if (nm > 0)
        if (const int rc = wave_push(r->inner, where, pcm_in_f32(ws_floats(r, r->w_xin), r->xs), cm.data(),
                                     pcm_out_f32(ws_floats(r, r->w_xout), r->xs), nm, hip_stream))
            return rc;
    FSNP_ON_DEVICE(r->h);
    launch_rate_out(a, r->tout, ws_floats(r, r->w_xout), r->xs, nullptr, 0,
                    PcmOut{out, (long)out_stride, (long)out_step, out_format, nullptr, nullptr}, n, s);
    FSNP_HIP_CHECK(hipGetLastError());
    for (int b = 0; b < r->S; ++b) r->samples[b] += c.v[b];
    return 0;
}

int fsnp_wave_rate_stream_finish_pcm(fsnp_wave_rate_stream* r, const int32_t* slots, int32_t num, void* out, int32_t out_format,
                                     int64_t out_stride, int64_t out_step, void* hip_stream) {
    const char* where = "fsnp_wave_rate_stream_finish_pcm";
    if (!r || !out) { set_error("%s: null argument", where); return 1; }
    if (const int rc = check_sample_format(where, "output", out_format, out_step, false)) return rc;
    if (const int rc = check_slots(where, slots, num, r->S)) return rc;
    SlotCounts c{};
    if (slots) for (int i = 0; i < num; ++i) c.v[slots[i]] = 1;
    else for (int b = 0; b < r->S; ++b) c.v[b] = 1;
    std::vector<int32_t>& cm = r->cm;                          // [0, S): the inner push's counts; behind them the inner finish's slots
    std::fill(cm.begin(), cm.end(), 0);
    int nm = 0, nfin = 0;
    for (int b = 0; b < r->S; ++b) {
        if (!c.v[b]) continue;
        const long long L = r->samples[b];
        if (L == 0) { c.v[b] = 0; continue; }                  // nothing to finish: a row of zeros
        if (total_of(r, L) <= r->n_half) {
            set_error("%s: slot %d holds %lld samples at %d Hz, %lld at the model's %d Hz: a clip needs more than n_fft/2 = %d there "
                      "(reflect padding)", where, b, L, r->rate, total_of(r, L), r->model_rate, r->n_half);
            return 2;
        }
        cm[b] = (int32_t)(total_of(r, L) - ready_of(r, L));
        nm = std::max(nm, (int)cm[b]);
        cm[r->S + nfin++] = b;
    }
    if (const int rc = push_preamble(r->h, where)) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const RateArgs a = rate_args(r);
    {
        FSNP_ON_DEVICE(r->h);
        launch_rate_in(a, c, 1, PcmIn{nullptr, 0, 1, kPcmF32}, r->tin, ws_floats(r, r->w_xin), r->xs, s);
    }
    if (nm > 0)
        if (const int rc = wave_push(r->inner, where, pcm_in_f32(ws_floats(r, r->w_xin), r->xs), cm.data(),
                                     pcm_out_f32(ws_floats(r, r->w_xout), r->xs), nm, hip_stream))
            return rc;
    if (nfin > 0)                                              // (else every row is zeros: the out kernel writes them)
        if (const int rc = wave_finish(r->inner, where, cm.data() + r->S, nfin, pcm_out_f32(ws_floats(r, r->w_fin), r->fs), hip_stream))
            return rc;
    {
        FSNP_ON_DEVICE(r->h);
        launch_rate_out(a, r->tout, ws_floats(r, r->w_xout), r->xs, ws_floats(r, r->w_fin), r->fs,
                        PcmOut{out, (long)out_stride, (long)out_step, out_format, nullptr, nullptr}, (int)r->DR, s);
        FSNP_HIP_CHECK(hipGetLastError());
        if (const int rc = r->rec.reset(cm.data() + r->S, nfin, s)) return rc;
    }
    for (int i = 0; i < nfin; ++i) r->samples[cm[r->S + i]] = 0;
    return 0;
}

int fsnp_wave_rate_stream_reset(fsnp_wave_rate_stream* r, const int32_t* slots, int32_t num, void* hip_stream) {
    if (!r) { set_error("fsnp_wave_rate_stream_reset: null argument"); return 1; }
    if (const int rc = check_slots("fsnp_wave_rate_stream_reset", slots, num, r->S)) return rc;
    return rate_reset(r, slots, num, hip_stream);
}

int fsnp_wave_rate_stream_delay(const fsnp_wave_rate_stream* r) { return r ? (int)r->DR : 0; }
int fsnp_wave_rate_stream_model_delay(const fsnp_wave_rate_stream* r) { return r ? (int)r->DM : 0; }
int fsnp_wave_rate_stream_model_max_samples(const fsnp_wave_rate_stream* r) { return r ? r->model_max : 0; }

int64_t fsnp_wave_rate_stream_state_bytes(const fsnp_wave_rate_stream* r) { return r ? (int64_t)(r->inner_bytes + r->rec.bytes) : 0; }

int fsnp_wave_rate_stream_get_state(fsnp_wave_rate_stream* r, int32_t slot, void* dev_dst, void* hip_stream) {
    if (!r || !dev_dst) { set_error("fsnp_wave_rate_stream_get_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_wave_rate_stream_get_state", slot, r->S)) return rc;
    if (const int rc = fsnp_wave_stream_get_state(r->inner, slot, dev_dst, hip_stream)) return rc;
    FSNP_ON_DEVICE(r->h);
    return r->rec.get(slot, dev_dst, r->inner_bytes, static_cast<hipStream_t>(hip_stream));
}

int fsnp_wave_rate_stream_set_state(fsnp_wave_rate_stream* r, int32_t slot, const void* dev_src, void* hip_stream) {
    const char* where = "fsnp_wave_rate_stream_set_state";
    if (!r || !dev_src) { set_error("%s: null argument", where); return 1; }
    if (const int rc = check_slot(where, slot, r->S)) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    // a migration call: count and pair in one copy, one wait - before anything is loaded, so a record of another pair changes nothing
    struct { long long count; int up, down; } tail{};
    {
        FSNP_ON_DEVICE(r->h);
        FSNP_HIP_CHECK(hipMemcpyAsync(&tail, static_cast<const unsigned char*>(dev_src) + r->inner_bytes + r->o_count, 16, hipMemcpyDeviceToHost, s));
        FSNP_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (tail.count < 0) { set_error("%s: slot %d: the loaded record holds a negative sample count", where, slot); return 2; }
    const bool empty = tail.count == 0 && tail.up == 0 && tail.down == 0;
    if (!empty && (tail.up != r->pin.up || tail.down != r->pin.down)) {
        set_error("%s: slot %d: the record was saved by a session of the ratio %d : %d, this one converts %d Hz -> %d Hz at %d : %d", where,
                  slot, tail.up, tail.down, r->rate, r->model_rate, r->pin.up, r->pin.down);
        return 2;
    }
    const long long inner_count = ready_of(r, tail.count);     // the inner session's count follows from ours: it need not read it back
    if (const int rc = wave_set_state(r->inner, slot, dev_src, &inner_count, hip_stream)) return rc;
    FSNP_ON_DEVICE(r->h);
    if (const int rc = r->rec.set(slot, dev_src, r->inner_bytes, s)) return rc;
    r->samples[slot] = tail.count;
    return 0;
}

int fsnp_wave_rate_stream_samples(fsnp_wave_rate_stream* r, int32_t slot, int64_t* pushed) {
    if (!r || !pushed) { set_error("fsnp_wave_rate_stream_samples: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_wave_rate_stream_samples", slot, r->S)) return rc;
    *pushed = r->samples[slot];
    return 0;
}

}  // extern "C"
