// fsnp_wave_stream_abi.hip - include/fsnp_wave_stream.h: waveform sessions of the original FullSubNet (samples in, samples out).
//
// A wave session is a spectrum session between two transforms.  It holds a mag-stream session (fsnp_stream_abi.hip) of
// max(max_samples / hop + 1, ceil(n_fft / (2 hop)) + look_ahead) frames per call with, per slot, a wave record behind the mag-stream record (layout: fsnp_common.h, WaveArgs;
// the look-ahead ring lies inside it) and a workspace of its own, allocated and zeroed at creation.  One push on the caller's stream,
// nothing allocated, nothing synchronised:
//   wave_gather_kernel   the rows of the newly complete frames from the carried samples + the new ones, the carry and the count advanced
//   launch_linear_act    forward DFT (the handle's d_stft matrices, window folded in) -> spectra, one workspace row per frame
//   spec_push_body       the ring push of a spectrum session on those rows, the frames each slot completed as its counts: |X|, the mag
//                        push, cIRM of step j times the noisy spectrum of frame P_f + j - look_ahead into row j (zeros where there is
//                        none), ring advanced
//   launch_linear_act    inverse DFT -> windowed frames
//   wave_ola_kernel      overlap-add + envelope division into the fifo, this push's c samples out (zeros before D and past c)
// fsnp_wave_stream_finish runs the same chain with the clip's last frames (1 + L / hop - nf(L) <= ceil(n_fft / (2 hop)) of them, each
// reflected at the end) and look_ahead zero frames into the model, emits the remaining D samples and resets the slots.  The session keeps
// the hop its handle had at creation (include/fsnp_stft_geometry.h).  The host mirrors every slot's sample count,
// so frames per slot are known without asking the device.  The fp32 entry points and the ones of include/fsnp_pcm.h are one push and
// one finish behind two sets of checks: the sample format is a property of the two kernels' loads and stores (pcm.h), not of the session.
#include <algorithm>
#include <vector>

#include "fsnp_handle.h"
#include "pcm.h"

struct fsnp_wave_stream {
    fsnp_handle* h = nullptr;
    fsnp_stream* mag = nullptr;       // the model's state and its push
    int S = 0, max_samples = 0, NF = 0, hop = 0, half = 0, LA = 0, D = 0;
    StftPlan p{};
    size_t mag_bytes = 0;             // one slot's mag-stream record
    SlotRecords rec;                  // the slots' wave records behind it
    size_t o_ring = 0, o_tail = 0, o_fifo = 0, o_count = 0;       // byte offsets inside a wave record (carry at 0)
    unsigned char* ws = nullptr;
    size_t ws_bytes = 0;
    size_t w_meta = 0, w_xfr = 0, w_spec = 0, w_mag = 0, w_mask = 0, w_enh = 0, w_fr = 0;
    std::vector<int64_t> samples;     // host mirror of the slots' sample counts (fsnp_wave_stream_set_state reads the loaded one back)
};

namespace {

// the chain of one push (fin = 0, c.v = samples per slot) or one finish (fin = 1, c.v = 1 for the slots that end): checks are done
int wave_run(fsnp_wave_stream* w, const SlotCounts& c, int fin, const PcmIn& wav, const PcmOut& out, int ncols, hipStream_t s) {
    fsnp_handle* h = w->h;
    const StftPlan& p = w->p;
    SlotCounts spectra{}, steps{};
    int nrow = 1, frames = 0;
    for (int b = 0; b < w->S; ++b) {
        const WaveStep st = wave_step(w->samples[b], fin ? 0 : c.v[b], fin ? c.v[b] : 0, w->hop, w->half, w->LA);
        spectra.v[b] = st.ks; steps.v[b] = st.km;
        nrow = std::max(nrow, st.km);
        frames += st.km;
    }
    FSNP_ON_DEVICE(h);
    auto fptr = [&](size_t off) { return reinterpret_cast<float*>(w->ws + off); };
    WaveArgs a{};
    a.state = w->rec.base; a.stride = w->rec.bytes; a.o_tail = w->o_tail; a.o_fifo = w->o_fifo; a.o_count = w->o_count;
    a.meta = reinterpret_cast<WaveMeta*>(w->ws + w->w_meta);
    a.S = w->S; a.hop = w->hop; a.half = w->half; a.LA = w->LA; a.nrow = nrow; a.xl = p.xl;
    const int rows = w->S * nrow;
    launch_wave_gather(a, c, fin, wav, fptr(w->w_xfr), s);
    if (frames > 0)
        launch_linear_act(fptr(w->w_xfr), p.xl, h->d_stft + p.o_fwd, p.fwd_ld, h->d_stft + p.o_zero, fptr(w->w_spec), p.sp, p.n_fft, p.N2, 1,
                          rows, FSNP_ACT_NONE, h->num_cus, s);
    // spectra and enhanced spectra [S][nrow][sp] floats as complex (slot, f, frame); without frames there is nothing to transform back,
    // so the ring push need not write the zero rows of such a call (write_idle = false)
    const int64_t cst[3] = {(int64_t)nrow * (p.sp / 2), 1, p.sp / 2};
    if (const int rc = spec_push_body(w->mag, SpecRing{w->rec.base + w->o_ring, w->rec.bytes, w->LA}, fptr(w->w_mag), fptr(w->w_mask),
                                      fptr(w->w_spec), cst, spectra, steps, fptr(w->w_enh), cst, false, nrow, s))
        return rc;
    if (frames > 0)
        launch_linear_act(fptr(w->w_enh), p.sp, h->d_stft + p.o_inv, p.inv_ld, h->d_stft + p.o_zero, fptr(w->w_fr), p.n_fft, p.N2, p.n_fft, 1,
                          rows, FSNP_ACT_NONE, h->num_cus, s, 0, p.N2);
    launch_wave_ola(a, fptr(w->w_fr), h->d_stft + p.o_win, out, ncols, s);
    FSNP_HIP_CHECK(hipGetLastError());
    return 0;
}

// stream-ordered zeroing of both records of the (checked) slots (NULL = all), the host mirror with them
int wave_reset(fsnp_wave_stream* w, const int32_t* slots, int32_t num, void* hip_stream) {
    if (const int rc = fsnp_stream_reset(w->mag, slots, num, hip_stream)) return rc;
    FSNP_ON_DEVICE(w->h);
    if (const int rc = w->rec.reset(slots, num, static_cast<hipStream_t>(hip_stream))) return rc;
    if (!slots) std::fill(w->samples.begin(), w->samples.end(), 0);
    else for (int i = 0; i < num; ++i) w->samples[slots[i]] = 0;
    return 0;
}

// fsnp_wave_stream_create (live = 0) / fsnp_wave_stream_create_live (live = 1: the mag session inside is a live one)
int wave_create(fsnp_handle* h, int32_t slots, int32_t max_samples, int live, const char* where, fsnp_wave_stream** out) {
    if (!h || !out) { set_error("%s: null argument", where); return 1; }
    *out = nullptr;
    if (h->cfg.output_size != 2) { set_error("%s: the cIRM epilogue needs output_size = 2 (this handle: %d)", where, h->cfg.output_size); return 2; }
    if (max_samples < 1) { set_error("%s: max_samples %d < 1", where, max_samples); return 2; }
    if (h->F - 1 > 4096) { set_error("%s: num_freqs - 1 = %d > 4096: a slot's carry and overlap-add sums must fit one workgroup's LDS", where, h->F - 1); return 2; }
    const StftPlan p = stft_plan(h);                  // the session keeps this geometry whatever the handle is told later
    if (const int rc = check_hop_length(h->F, p.hop, where)) return rc;
    const int hop = p.hop, half = p.half, LA = h->cfg.look_ahead;
    const int fin_rows = wave_finish_rows(hop, half, LA);
    const int NF = std::max(max_samples / hop + 1, fin_rows);
    if (live && fin_rows > kLiveMaxChunk) {
        set_error("%s: finishing a clip takes up to ceil(n_fft / (2 hop_length)) + look_ahead = %d frames in one call (n_fft %d, hop_length %d, "
                  "look_ahead %d), a live session runs at most %d: open a default session (fsnp_wave_stream_create)", where, fin_rows,
                  p.n_fft, hop, LA, kLiveMaxChunk);
        return 2;
    }
    fsnp_stream* mag = nullptr;
    // every refusal of a mag session, with its reason (live: frames per push = max_samples / hop + 1 <= 16)
    if (const int rc = live ? stream_create(h, slots, NF, 1, where, &mag) : fsnp_stream_create(h, slots, NF, &mag)) return rc;
    if (ensure_stft(h)) { fsnp_stream_destroy(mag); return 2; }
    fsnp_wave_stream* w = new fsnp_wave_stream();
    w->h = h; w->mag = mag; w->S = slots; w->max_samples = max_samples; w->NF = NF; w->hop = hop; w->half = half; w->LA = LA;
    w->D = p.n_fft + LA * hop;
    w->p = p;
    w->mag_bytes = (size_t)fsnp_stream_state_bytes(mag);
    w->o_ring = align_up((size_t)(p.n_fft + 1) * 4, 8);
    w->o_tail = w->o_ring + (size_t)LA * p.F * 8;
    w->o_fifo = w->o_tail + (size_t)(p.n_fft - hop) * 4;
    w->o_count = align_up(w->o_fifo + (size_t)hop * 4, 8);
    const size_t rec_bytes = align_up(w->o_count + 8, 16);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    const size_t S = slots, rows = S * NF;
    w->w_meta = take(S * sizeof(WaveMeta));
    w->w_xfr = take(rows * p.xl * 4);
    w->w_spec = take(rows * p.sp * 4);
    w->w_mag = take(rows * h->FP * 4);
    w->w_mask = take(rows * 2 * p.F * 4);
    w->w_enh = take(rows * p.sp * 4);
    w->w_fr = take(rows * p.n_fft * 4);
    w->ws_bytes = o;
    fsnp::DeviceGuard g(h->device);
    hipError_t e = w->rec.create(rec_bytes, slots);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&w->ws), w->ws_bytes);
    if (e == hipSuccess) e = hipMemset(w->ws, 0, w->ws_bytes);      // (pad columns of the spectrum rows stay 0 for good)
    if (e != hipSuccess) {
        set_error("%s: %s (wave state %zu bytes x %d slots, workspace %zu bytes)", where, hipGetErrorString(e), rec_bytes, slots,
                  w->ws_bytes);
        w->rec.free();
        if (w->ws) (void)hipFree(w->ws);
        fsnp_stream_destroy(mag);
        delete w;
        return 4;
    }
    w->samples.assign(S, 0);
    *out = w;
    return 0;
}

}  // namespace

namespace fsnp {

// fsnp_wave_stream_push / _push_pcm and fsnp_wave_stream_finish / _finish_pcm behind their own checks (fsnp_handle.h: a rate session,
// fsnp_wave_rate_stream_abi.hip, drives its inner session through these same bodies)
int wave_push(fsnp_wave_stream* w, const char* where, const PcmIn& wav, const int32_t* counts, const PcmOut& out, int32_t n, void* hip_stream) {
    if (n < 1 || n > w->max_samples) { set_error("%s: n = %d outside [1, max_samples = %d]", where, n, w->max_samples); return 2; }
    SlotCounts c{};
    if (const int rc = read_counts(where, counts, w->S, n, c)) return rc;
    if (const int rc = push_preamble(w->h, where)) return rc;
    if (const int rc = wave_run(w, c, 0, wav, out, n, static_cast<hipStream_t>(hip_stream))) return rc;
    for (int b = 0; b < w->S; ++b) w->samples[b] += c.v[b];
    return 0;
}

int wave_finish(fsnp_wave_stream* w, const char* where, const int32_t* slots, int32_t num, const PcmOut& out, void* hip_stream) {
    if (const int rc = check_slots(where, slots, num, w->S)) return rc;
    SlotCounts c{};
    if (slots) for (int i = 0; i < num; ++i) c.v[slots[i]] = 1;
    else for (int b = 0; b < w->S; ++b) c.v[b] = 1;
    for (int b = 0; b < w->S; ++b) {
        if (!c.v[b]) continue;
        if (w->samples[b] == 0) { c.v[b] = 0; continue; }      // nothing to finish: a row of zeros
        if (w->samples[b] <= w->half) {
            set_error("%s: slot %d holds %lld samples: a clip needs more than n_fft/2 = %d (reflect padding)", where, b,
                      (long long)w->samples[b], w->half);
            return 2;
        }
    }
    if (const int rc = push_preamble(w->h, where)) return rc;
    if (const int rc = wave_run(w, c, 1, PcmIn{nullptr, 0, 1, kPcmF32}, out, w->D, static_cast<hipStream_t>(hip_stream))) return rc;
    return wave_reset(w, slots, num, hip_stream);
}

// fsnp_wave_stream_set_state behind its checks.  known = NULL: a migration call - the frames a later push completes follow from the
// slot's sample count, which the host must know - one wait.  A caller that knows the count (a rate session: it follows from its own) waits itself.
int wave_set_state(fsnp_wave_stream* w, int32_t slot, const void* dev_src, const long long* known, void* hip_stream) {
    if (const int rc = fsnp_stream_set_state(w->mag, slot, dev_src, hip_stream)) return rc;
    FSNP_ON_DEVICE(w->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (const int rc = w->rec.set(slot, dev_src, w->mag_bytes, s)) return rc;
    long long v = 0;
    if (known) v = *known;
    else {
        FSNP_HIP_CHECK(hipMemcpyAsync(&v, static_cast<const unsigned char*>(dev_src) + w->mag_bytes + w->o_count, 8, hipMemcpyDeviceToHost, s));
        FSNP_HIP_CHECK(hipStreamSynchronize(s));
    }
    if (v < 0) { set_error("fsnp_wave_stream_set_state: slot %d: the loaded record holds a negative sample count", slot); return 2; }
    w->samples[slot] = v;
    return 0;
}

}  // namespace fsnp

extern "C" {

int fsnp_wave_stream_create(fsnp_handle* h, int32_t slots, int32_t max_samples, fsnp_wave_stream** out) {
    return wave_create(h, slots, max_samples, 0, "fsnp_wave_stream_create", out);
}

int fsnp_wave_stream_create_live(fsnp_handle* h, int32_t slots, int32_t max_samples, fsnp_wave_stream** out) {
    return wave_create(h, slots, max_samples, 1, "fsnp_wave_stream_create_live", out);
}

void fsnp_wave_stream_destroy(fsnp_wave_stream* w) {
    if (!w) return;
    {
        fsnp::DeviceGuard g(w->h->device);
        w->rec.free();
        if (w->ws) (void)hipFree(w->ws);
    }
    fsnp_stream_destroy(w->mag);
    delete w;
}

int fsnp_wave_stream_push(fsnp_wave_stream* w, const float* wav, int64_t wav_stride, const int32_t* counts, float* out, int64_t out_stride,
                          int32_t n, void* hip_stream) {
    if (!w || !wav || !out) { set_error("fsnp_wave_stream_push: null argument"); return 1; }
    return wave_push(w, "fsnp_wave_stream_push", pcm_in_f32(wav, (long)wav_stride), counts, pcm_out_f32(out, (long)out_stride), n, hip_stream);
}

int fsnp_wave_stream_push_pcm(fsnp_wave_stream* w, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step,
                              const int32_t* counts, void* out, int32_t out_format, int64_t out_stride, int64_t out_step, int32_t n,
                              void* hip_stream) {
    if (!w || !wav || !out) { set_error("fsnp_wave_stream_push_pcm: null argument"); return 1; }
    if (const int rc = check_sample_format("fsnp_wave_stream_push_pcm", "input", in_format, wav_step, false)) return rc;
    if (const int rc = check_sample_format("fsnp_wave_stream_push_pcm", "output", out_format, out_step, false)) return rc;
    return wave_push(w, "fsnp_wave_stream_push_pcm", PcmIn{wav, (long)wav_stride, (long)wav_step, in_format}, counts,
                     PcmOut{out, (long)out_stride, (long)out_step, out_format, nullptr, nullptr}, n, hip_stream);
}

int fsnp_wave_stream_finish(fsnp_wave_stream* w, const int32_t* slots, int32_t num, float* out, int64_t out_stride, void* hip_stream) {
    if (!w || !out) { set_error("fsnp_wave_stream_finish: null argument"); return 1; }
    return wave_finish(w, "fsnp_wave_stream_finish", slots, num, pcm_out_f32(out, (long)out_stride), hip_stream);
}

int fsnp_wave_stream_finish_pcm(fsnp_wave_stream* w, const int32_t* slots, int32_t num, void* out, int32_t out_format, int64_t out_stride,
                                int64_t out_step, void* hip_stream) {
    if (!w || !out) { set_error("fsnp_wave_stream_finish_pcm: null argument"); return 1; }
    if (const int rc = check_sample_format("fsnp_wave_stream_finish_pcm", "output", out_format, out_step, false)) return rc;
    return wave_finish(w, "fsnp_wave_stream_finish_pcm", slots, num, PcmOut{out, (long)out_stride, (long)out_step, out_format, nullptr, nullptr},
                       hip_stream);
}

int fsnp_wave_stream_reset(fsnp_wave_stream* w, const int32_t* slots, int32_t num, void* hip_stream) {
    if (!w) { set_error("fsnp_wave_stream_reset: null argument"); return 1; }
    if (const int rc = check_slots("fsnp_wave_stream_reset", slots, num, w->S)) return rc;
    return wave_reset(w, slots, num, hip_stream);
}

int fsnp_wave_stream_delay(const fsnp_wave_stream* w) { return w ? w->D : 0; }

int64_t fsnp_wave_stream_state_bytes(const fsnp_wave_stream* w) { return w ? (int64_t)(w->mag_bytes + w->rec.bytes) : 0; }

int fsnp_wave_stream_get_state(fsnp_wave_stream* w, int32_t slot, void* dev_dst, void* hip_stream) {
    if (!w || !dev_dst) { set_error("fsnp_wave_stream_get_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_wave_stream_get_state", slot, w->S)) return rc;
    if (const int rc = fsnp_stream_get_state(w->mag, slot, dev_dst, hip_stream)) return rc;
    FSNP_ON_DEVICE(w->h);
    return w->rec.get(slot, dev_dst, w->mag_bytes, static_cast<hipStream_t>(hip_stream));
}

int fsnp_wave_stream_set_state(fsnp_wave_stream* w, int32_t slot, const void* dev_src, void* hip_stream) {
    if (!w || !dev_src) { set_error("fsnp_wave_stream_set_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_wave_stream_set_state", slot, w->S)) return rc;
    return wave_set_state(w, slot, dev_src, nullptr, hip_stream);
}

int fsnp_wave_stream_samples(fsnp_wave_stream* w, int32_t slot, int64_t* pushed) {
    if (!w || !pushed) { set_error("fsnp_wave_stream_samples: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_wave_stream_samples", slot, w->S)) return rc;
    *pushed = w->samples[slot];
    return 0;
}

}  // extern "C"
