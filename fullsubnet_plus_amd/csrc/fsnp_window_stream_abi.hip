// fsnp_window_stream_abi.hip - include/session/fsnp_window_stream.h: window sessions of either model (blocks of samples in, as many
// out, one window late; the plan of include/ext/fsnp_windowed.h run block by block).  Host code only; kernels: window_stream.hip and
// the windowed call's own (windowed.hip).  DESIGN.md section 8g.
//
// One push on the caller's stream, nothing allocated, nothing synchronised; which windows complete follows from the host's mirror of
// the slots' sample counts:
//   window_append_kernel      the caller's block behind each slot's input history
//   per forward of <= max_batch completed windows (none in most pushes):
//     stft_pad_window_kernel  the windows, read from the histories, reflect-padded into the handle's io area
//     enhance_padded          STFT -> model -> cIRM -> inverse DFT       (a copy session: the padded rows' centres, copied)
//     launch_istft_ola        overlap-add into the session's fp32 staging rows
//   window_emit_kernel        the output rows from the pending samples and the staged rows; new pending samples and tail
//   window_compact_kernel     the histories moved on to their first incomplete window
// fsnp_window_stream_finish_pcm runs the same chain without the first and the last step, on the clips' last windows at their true
// lengths, and resets the slots.
#include <algorithm>
#include <climits>
#include <vector>

#include "../../include/session/fsnp_window_stream.h"
#include "fsnp_handle.h"
#include "pcm.h"
#include "window_stream.h"

struct fsnp_window_stream {
    fsnp_handle* h = nullptr;
    bool model = true;                // false: fsnp_debug_window_stream_create_copy
    int slots = 0, W = 0, V = 0, S = 0, max_samples = 0, max_batch = 0, HC = 0, rows_cap = 0, min_frames = 1;
    StftPlan p{};                     // the geometry the handle had at creation, kept like a wave session's: its offsets into d_stft do not
                                      // depend on the hop, and pad, DFTs, frame floor and overlap-add all run at this plan's hop
    unsigned char* dev = nullptr;     // one allocation: the slots' records (window_stream.h), then the staging rows [rows_cap][W]
    StreamState st{};
    float* stage = nullptr;
    // the host's mirror of every slot: samples pushed, the record's current halves, the oldest pending sample's index
    std::vector<long long> samples;
    std::vector<int> par, pend_off;
    // one call's tables: sized at creation, so that a push allocates nothing
    std::vector<StreamRow> rows;
    std::vector<WindowRow> windows;
    std::vector<int32_t> lens, frames, counts;
};

namespace {

struct SlotView { long done; int fill, pending; };      // complete windows, samples in hist, merged samples not yet due
SlotView slot_view(const fsnp_window_stream* w, int b) {
    const long P = w->samples[b], done = windows_complete(P, w->W, w->V);
    return SlotView{done, (int)(P - done * w->S), done > 0 ? (int)(done * w->S - (P - w->W)) : 0};
}

// One push (fin = false, c = samples per slot) or one finish (fin = true, c = 1 for the slots that end).  Every check has been made
// except those of a ragged forward, which come before anything is enqueued.
int window_run(fsnp_window_stream* w, const char* where, bool fin, const int32_t* c, const PcmIn& wav, const PcmOut& out, int ncols,
               void* hip_stream) {
    fsnp_handle* h = w->h;
    const StftPlan& p = w->p;
    const int W = w->W, V = w->V, S = w->S;
    w->rows.clear();
    w->windows.clear();
    for (int b = 0; b < w->slots; ++b) {
        StreamRow r{};
        r.par = w->par[b]; r.pend_off = w->pend_off[b]; r.total = w->samples[b];
        if (c[b] > 0) {
            const long P = (long)w->samples[b];
            const SlotView v = slot_view(w, b);
            r.fill = v.fill; r.pcount = v.pending; r.fade0 = v.done > 0; r.first = (int)w->windows.size();
            r.lead = (int)std::max(0L, std::min((long)W - P, (long)(fin ? W : c[b])));
            if (!fin) {
                r.c = r.cnt = c[b];
                r.total = P + c[b];
                r.m = (int)(windows_complete(P + c[b], W, V) - v.done);
                for (int k = 0; k < r.m; ++k) w->windows.push_back(WindowRow{b, r.par * w->HC + k * S, W});
                if (r.m > 0) {
                    r.u0 = (int)(P + c[b] - W - v.done * S);
                    r.npc = r.m * S - r.u0;
                    r.keep = r.fill + r.c - r.m * S;
                }
            } else {
                r.fin = 1; r.cnt = W;
                r.total = 0;                                    // the emit leaves the record's count reset
                r.m = (int)(window_count(P, W, V) - v.done);      // 0 (the pushes ran the last window: P = k S + W) or 1
                if (r.m) w->windows.push_back(WindowRow{b, r.par * w->HC, r.fill});
            }
        }
        if (!fin && r.m == 0 && r.cnt - r.lead > r.pcount) {      // an output due without its window: the schedule rules it out
            set_error("%s: slot %d: %d samples due, %d pending and no window completed (internal error)", where, b, r.cnt - r.lead, r.pcount);
            return 4;
        }
        w->rows.push_back(r);
    }
    const int total = (int)w->windows.size();
    if (total > w->rows_cap) { set_error("%s: %d windows in one call, staging rows for %d", where, total, w->rows_cap); return 4; }
    // the forwards: max_batch consecutive windows each; only a finish can mix lengths
    int nmax = 0, longest = 0;
    for (int f0 = 0; f0 < total; f0 += w->max_batch) {
        const int n = std::min(total - f0, w->max_batch);
        int most = 0;
        bool ragged = false;
        for (int r = 0; r < n; ++r) {
            w->lens[f0 + r] = w->windows[f0 + r].len;
            w->frames[f0 + r] = 1 + w->lens[f0 + r] / p.hop;
            most = std::max(most, w->lens[f0 + r]);
            ragged = ragged || w->lens[f0 + r] != w->lens[f0];
        }
        if (w->model && ragged)
            if (const int rc = check_lengths(h, w->frames.data() + f0, n, 1 + most / p.hop, where)) return rc;
        nmax = std::max(nmax, n);
        longest = std::max(longest, most);
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    if (total) {      // the model's io area is the handle's: behind its last user, and as large as creation left it or larger
        const WaveIo io_max = wave_io(p, nmax, longest);
        if (order_after_last_forward(h, s)) return 4;
        if (ensure_io(h, w->model ? io_max.total : io_max.noisy, s)) return 4;
    }
    const float* g = find_window_fade(h, V)->dev;      // uploaded at creation, never evicted
    PcmOut o = out;
    if (out.clipped) FSNP_HIP_CHECK(hipMemsetAsync(out.clipped, 0, (size_t)w->slots * 4, s));
    if (out.fmt != kPcmS16) o.clipped = nullptr;
    if (!fin) launch_window_append(w->st, wav, w->rows.data(), w->slots, s);
    const PcmIn hist{w->st.hist, 2L * w->HC, 1, kPcmF32};
    for (int f0 = 0; f0 < total; f0 += w->max_batch) {
        const int n = std::min(total - f0, w->max_batch);
        int most = 0;
        bool ragged = false;
        for (int r = 0; r < n; ++r) { most = std::max(most, w->lens[f0 + r]); ragged = ragged || w->lens[f0 + r] != w->lens[f0]; }
        const WaveIo io = wave_io(p, n, most);
        float* xp = reinterpret_cast<float*>(h->io + io.xp);
        float* rows = w->stage + (size_t)f0 * W;
        launch_stft_pad_window(hist, xp, io.xs, w->windows.data() + f0, n, p.n_fft, s);
        if (!w->model) {
            FSNP_HIP_CHECK(hipMemcpy2DAsync(rows, (size_t)W * 4, xp + p.half, (size_t)io.xs * 4, (size_t)most * 4, n, hipMemcpyDeviceToDevice, s));
            continue;
        }
        if (const int rc = enhance_padded(h, p, io, n, ragged ? w->frames.data() + f0 : nullptr, hip_stream)) return rc;
        launch_istft_ola(reinterpret_cast<const float*>(h->io + io.fr), h->d_stft + p.o_win, pcm_out_f32(rows, W), n, io.T, most,
                         ragged ? w->lens.data() + f0 : nullptr, p.n_fft, p.hop, s);
    }
    launch_window_emit(w->st, w->stage, g, o, w->rows.data(), w->slots, ncols, s);
    if (!fin) launch_window_compact(w->st, w->rows.data(), w->slots, s);
    FSNP_HIP_CHECK(hipGetLastError());
    if (total)
        if (const int rc = mark_forward_done(h, s)) return rc;
    // the call is enqueued whole: the mirror follows
    for (int b = 0; b < w->slots && !fin; ++b) {
        const StreamRow& r = w->rows[b];
        if (r.c == 0) continue;
        w->samples[b] = r.total;
        if (r.m > 0) { w->par[b] ^= 1; w->pend_off[b] = 0; }
        else w->pend_off[b] += r.cnt - r.lead;
    }
    return 0;
}

int window_reset(fsnp_window_stream* w, const int32_t* slots, int32_t num, void* hip_stream) {
    FSNP_ON_DEVICE(w->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (!slots) FSNP_HIP_CHECK(hipMemsetAsync(w->st.count, 0, (size_t)w->slots * 8, s));
    for (int i = 0; i < (slots ? num : w->slots); ++i) {
        const int b = slots ? slots[i] : i;
        if (slots) FSNP_HIP_CHECK(hipMemsetAsync(w->st.count + b, 0, 8, s));
        w->samples[b] = 0;
        w->pend_off[b] = 0;
    }
    return 0;
}

int window_create(fsnp_handle* h, int32_t slots, int32_t W, int32_t V, int32_t max_samples, int32_t max_batch, bool model,
                  const char* where, fsnp_window_stream** out) {
    if (!h || !out) { set_error("%s: null argument", where); return 1; }
    *out = nullptr;
    if (slots < 1 || slots > (1 << 20)) { set_error("%s: slots %d outside [1, %d]", where, (int)slots, 1 << 20); return 2; }
    if (max_samples < 1 || max_samples > (1 << 28)) { set_error("%s: max_samples %d outside [1, %d]", where, (int)max_samples, 1 << 28); return 2; }
    if (max_batch < 1) { set_error("%s: max_batch %d < 1", where, (int)max_batch); return 2; }
    if (model) {
        if (!h->committed) { set_error("%s: weights not committed (call fsnp_commit_weights)", where); return 2; }
        if (h->cfg.output_size != 2) { set_error("%s: the cIRM epilogue needs output_size = 2 (this handle: %d)", where, h->cfg.output_size); return 2; }
        if (ensure_stft(h)) return 2;
    }
    const StftPlan p = stft_plan(h);
    if (W < 2 || V < p.half || V > W / 2) {
        set_error("%s: overlap %d outside [n_fft / 2, window / 2] = [%d, %d] (window %d, n_fft = 2 (num_freqs - 1) = %d): a window's last "
                  "part must be a clip of its own, and a sample may lie in two windows at most", where, (int)V, p.half, (int)(W / 2), (int)W, p.n_fft);
        return 2;
    }
    if (W > (1 << 28)) { set_error("%s: window %d does not fit", where, (int)W); return 2; }
    if (!find_window_fade(h, V) && (int)h->win_fades.size() >= kWindowMaxFades) {
        set_error("%s: this handle already keeps the cross-fade tables of %d overlaps, the most it holds (they are never evicted: launches "
                  "in flight may read them); overlap %d needs another handle", where, kWindowMaxFades, (int)V);
        return 2;
    }
    const int S = W - V, min_frames = model ? min_clip_frames(h) : 1;
    if (1 + (V + 1) / p.hop < min_frames) {
        set_error("%s: overlap %d: a clip's last window may be as short as overlap + 1 = %d samples = %d frames, below the model's own "
                  "minimum clip of %d frames (%d samples at hop_length %d: its largest TSSE kernel less look_ahead); a finish could then "
                  "be refused, so the session is refused instead", where, (int)V, (int)V + 1, 1 + (V + 1) / p.hop, min_frames, (min_frames - 1) * p.hop, p.hop);
        return 2;
    }
    if (model && max_batch > 1) {      // a finish of several slots is ragged in general; with one window per forward nothing ever is
        if (h->model != FSNP_MODEL_FULLSUBNET && h->cfg.subband_num > 1) {
            set_error("%s: max_batch %d > 1: forwards of windows of different lengths are not supported with subband_num = %d > 1 "
                      "(open the session with max_batch = 1)", where, (int)max_batch, h->cfg.subband_num);
            return 2;
        }
        if (h->sb_tcn) {
            set_error("%s: max_batch %d > 1: forwards of windows of different lengths are not supported with the sub-band sequence_model "
                      "\"TCN\" (open the session with max_batch = 1)", where, (int)max_batch);
            return 2;
        }
    }
    const long long rows_cap = (long long)slots * (1 + (max_samples + S - 1) / S);
    if (rows_cap > INT_MAX / 2) { set_error("%s: %lld windows in one call do not fit (slots %d, max_samples %d)", where, rows_cap, (int)slots, (int)max_samples); return 2; }
    fsnp_window_stream* w = new fsnp_window_stream();
    w->h = h; w->model = model; w->slots = slots; w->W = W; w->V = V; w->S = S; w->max_samples = max_samples; w->max_batch = max_batch;
    w->HC = W + max_samples; w->rows_cap = (int)rows_cap; w->min_frames = min_frames; w->p = p;
    const size_t n = slots;
    const size_t o_pend = align_up(n * 2 * w->HC * 4, 256), o_tail = align_up(o_pend + n * 2 * S * 4, 256);
    const size_t o_count = align_up(o_tail + n * 2 * V * 4, 256), o_stage = align_up(o_count + n * 8, 256);
    const size_t bytes = o_stage + (size_t)rows_cap * W * 4;
    const WaveIo io = wave_io(p, (int)std::min<long long>(max_batch, rows_cap), W);
    fsnp::DeviceGuard guard(h->device);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&w->dev), bytes);
    if (e == hipSuccess) e = hipMemset(w->dev, 0, o_stage);
    if (e != hipSuccess) {
        set_error("%s: %s (%zu bytes: %d slots, window %d, max_samples %d, %lld staging rows)", where, hipGetErrorString(e), bytes, (int)slots,
                  (int)W, (int)max_samples, rows_cap);
        if (w->dev) (void)hipFree(w->dev);
        delete w;
        return 4;
    }
    w->st = StreamState{reinterpret_cast<float*>(w->dev), reinterpret_cast<float*>(w->dev + o_pend), reinterpret_cast<float*>(w->dev + o_tail),
                        reinterpret_cast<long long*>(w->dev + o_count), w->HC, W, V};
    w->stage = reinterpret_cast<float*>(w->dev + o_stage);
    // the handle's side: its io area for the largest forward and the fade table, so that no push allocates or uploads
    const float* g = nullptr;
    int rc = order_after_last_forward(h, nullptr) ? 4 : 0;
    if (!rc) rc = ensure_io(h, model ? io.total : io.noisy, nullptr);
    if (!rc) rc = window_fade_device(h, V, nullptr, g);
    if (!rc) rc = mark_forward_done(h, nullptr);
    if (rc) {
        (void)hipFree(w->dev);
        delete w;
        return rc;
    }
    w->samples.assign(n, 0); w->par.assign(n, 0); w->pend_off.assign(n, 0);
    w->rows.reserve(n); w->windows.reserve(rows_cap); w->lens.assign(rows_cap, 0); w->frames.assign(rows_cap, 0); w->counts.assign(n, 0);
    *out = w;
    return 0;
}

}  // namespace

extern "C" {

int fsnp_window_stream_plan(int64_t pushed, int64_t count, int32_t window, int32_t overlap, int64_t* first, int64_t* num) {
    if (window < 2 || overlap < 1 || overlap > window / 2 || pushed < 0 || count < 0 || !first || !num) return -1;
    if (pushed > INT64_MAX - count) return -1;
    *first = windows_complete((long)pushed, window, overlap);
    *num = windows_complete((long)(pushed + count), window, overlap) - *first;
    return 0;
}

int fsnp_window_stream_create(fsnp_handle* h, int32_t slots, int32_t window, int32_t overlap, int32_t max_samples, int32_t max_batch,
                              fsnp_window_stream** out) {
    return window_create(h, slots, window, overlap, max_samples, max_batch, true, "fsnp_window_stream_create", out);
}

int fsnp_debug_window_stream_create_copy(fsnp_handle* h, int32_t slots, int32_t window, int32_t overlap, int32_t max_samples,
                                         int32_t max_batch, fsnp_window_stream** out) {
    return window_create(h, slots, window, overlap, max_samples, max_batch, false, "fsnp_debug_window_stream_create_copy", out);
}

void fsnp_window_stream_destroy(fsnp_window_stream* w) {
    if (!w) return;
    {
        fsnp::DeviceGuard g(w->h->device);
        if (w->dev) (void)hipFree(w->dev);      // (hipFree waits for the device: pushes still in flight finish first)
    }
    delete w;
}

int fsnp_window_stream_push_pcm(fsnp_window_stream* w, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step,
                                const int32_t* counts, void* out, int32_t out_format, int64_t out_stride, int64_t out_step, int32_t n,
                                int32_t* clipped, void* hip_stream) {
    const char* where = "fsnp_window_stream_push_pcm";
    if (!w || !wav || !out) { set_error("%s: null argument", where); return 1; }
    if (const int rc = check_sample_format(where, "input", in_format, wav_step, false)) return rc;
    if (const int rc = check_sample_format(where, "output", out_format, out_step, false)) return rc;
    if (n < 1 || n > w->max_samples) { set_error("%s: n = %d outside [1, max_samples = %d]", where, (int)n, w->max_samples); return 2; }
    for (int b = 0; b < w->slots; ++b) {
        const int v = counts ? counts[b] : n;
        if (v < 0 || v > n) { set_error("%s: slot %d: count %d outside [0, n = %d]", where, b, v, (int)n); return 2; }
        w->counts[b] = v;
    }
    if (w->model)
        if (const int rc = push_preamble(w->h, where)) return rc;
    return window_run(w, where, false, w->counts.data(), PcmIn{wav, (long)wav_stride, (long)wav_step, in_format},
                      PcmOut{out, (long)out_stride, (long)out_step, out_format, clipped, nullptr}, n, hip_stream);
}

int fsnp_window_stream_finish_pcm(fsnp_window_stream* w, const int32_t* slots, int32_t num, void* out, int32_t out_format,
                                  int64_t out_stride, int64_t out_step, int32_t* clipped, void* hip_stream) {
    const char* where = "fsnp_window_stream_finish_pcm";
    if (!w || !out) { set_error("%s: null argument", where); return 1; }
    if (const int rc = check_sample_format(where, "output", out_format, out_step, false)) return rc;
    if (const int rc = check_slots(where, slots, num, w->slots)) return rc;
    std::fill(w->counts.begin(), w->counts.end(), slots ? 0 : 1);
    for (int i = 0; slots && i < num; ++i) w->counts[slots[i]] = 1;
    for (int b = 0; b < w->slots; ++b) {
        if (!w->counts[b]) continue;
        const long long L = w->samples[b];
        if (L == 0) { w->counts[b] = 0; continue; }      // nothing to finish: a row of zeros
        if (L <= w->p.half) {
            set_error("%s: slot %d holds %lld samples: a clip needs more than n_fft/2 = %d (reflect padding)", where, b, L, w->p.half);
            return 2;
        }
        if (L <= w->W && 1 + (int)L / w->p.hop < w->min_frames) {
            set_error("%s: slot %d holds %lld samples = %d frames: too few frames for the model, whose smallest clip has %d (%d samples)", where,
                      b, L, 1 + (int)L / w->p.hop, w->min_frames, (w->min_frames - 1) * w->p.hop);
            return 2;
        }
    }
    if (w->model)
        if (const int rc = push_preamble(w->h, where)) return rc;
    if (const int rc = window_run(w, where, true, w->counts.data(), PcmIn{nullptr, 0, 1, kPcmF32},
                                  PcmOut{out, (long)out_stride, (long)out_step, out_format, clipped, nullptr}, w->W, hip_stream))
        return rc;
    // the slots that ended start afresh: the emit wrote their records' counts as 0, the mirror follows
    for (int b = 0; b < w->slots; ++b)
        if (w->counts[b]) { w->samples[b] = 0; w->pend_off[b] = 0; }
    return 0;
}

int fsnp_window_stream_reset(fsnp_window_stream* w, const int32_t* slots, int32_t num, void* hip_stream) {
    if (!w) { set_error("fsnp_window_stream_reset: null argument"); return 1; }
    if (const int rc = check_slots("fsnp_window_stream_reset", slots, num, w->slots)) return rc;
    return window_reset(w, slots, num, hip_stream);
}

int fsnp_window_stream_delay(const fsnp_window_stream* w) { return w ? w->W : 0; }

int fsnp_window_stream_samples(fsnp_window_stream* w, int32_t slot, int64_t* pushed) {
    if (!w || !pushed) { set_error("fsnp_window_stream_samples: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_window_stream_samples", slot, w->slots)) return rc;
    *pushed = w->samples[slot];
    return 0;
}

int64_t fsnp_window_stream_state_bytes(const fsnp_window_stream* w) { return w ? (int64_t)w->W * 8 + 8 : 0; }

int fsnp_window_stream_get_state(fsnp_window_stream* w, int32_t slot, void* dev_dst, void* hip_stream) {
    if (!w || !dev_dst) { set_error("fsnp_window_stream_get_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_window_stream_get_state", slot, w->slots)) return rc;
    FSNP_ON_DEVICE(w->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const SlotView v = slot_view(w, slot);
    const size_t b = slot, par = w->par[slot], W = w->W, V = w->V, S = w->S;
    unsigned char* dst = static_cast<unsigned char*>(dev_dst);
    FSNP_HIP_CHECK(hipMemsetAsync(dst, 0, W * 8, s));
    if (v.fill) FSNP_HIP_CHECK(hipMemcpyAsync(dst, w->st.hist + (b * 2 + par) * w->HC, (size_t)v.fill * 4, hipMemcpyDeviceToDevice, s));
    if (v.done) FSNP_HIP_CHECK(hipMemcpyAsync(dst + W * 4, w->st.tail + (b * 2 + par) * V, V * 4, hipMemcpyDeviceToDevice, s));
    if (v.pending)
        FSNP_HIP_CHECK(hipMemcpyAsync(dst + (W + V) * 4, w->st.pend + (b * 2 + par) * S + w->pend_off[slot], (size_t)v.pending * 4,
                                      hipMemcpyDeviceToDevice, s));
    FSNP_HIP_CHECK(hipMemcpyAsync(dst + W * 8, w->st.count + b, 8, hipMemcpyDeviceToDevice, s));
    return 0;
}

int fsnp_window_stream_set_state(fsnp_window_stream* w, int32_t slot, const void* dev_src, void* hip_stream) {
    if (!w || !dev_src) { set_error("fsnp_window_stream_set_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_window_stream_set_state", slot, w->slots)) return rc;
    FSNP_ON_DEVICE(w->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const size_t b = slot, par = w->par[slot], W = w->W, V = w->V, S = w->S;
    const unsigned char* src = static_cast<const unsigned char*>(dev_src);
    long long count = 0;
    FSNP_HIP_CHECK(hipMemcpyAsync(&count, src + W * 8, 8, hipMemcpyDeviceToHost, s));
    FSNP_HIP_CHECK(hipStreamSynchronize(s));
    if (count < 0) { set_error("fsnp_window_stream_set_state: slot %d: the loaded record holds a negative sample count", (int)slot); return 2; }
    FSNP_HIP_CHECK(hipMemcpyAsync(w->st.hist + (b * 2 + par) * w->HC, src, W * 4, hipMemcpyDeviceToDevice, s));
    FSNP_HIP_CHECK(hipMemcpyAsync(w->st.tail + (b * 2 + par) * V, src + W * 4, V * 4, hipMemcpyDeviceToDevice, s));
    FSNP_HIP_CHECK(hipMemcpyAsync(w->st.pend + (b * 2 + par) * S, src + (W + V) * 4, S * 4, hipMemcpyDeviceToDevice, s));
    FSNP_HIP_CHECK(hipMemcpyAsync(w->st.count + b, src + W * 8, 8, hipMemcpyDeviceToDevice, s));
    w->samples[slot] = count;
    w->pend_off[slot] = 0;
    return 0;
}

}  // extern "C"
