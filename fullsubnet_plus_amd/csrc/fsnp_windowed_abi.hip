// fsnp_windowed_abi.hip - the entry points of include/ext/fsnp_windowed.h: a long recording enhanced in overlapping windows that are
// cross-faded on the device.  Host code only: the plan, the refusals, and the forwards of enhance_wave_any (fsnp_stft_abi.hip) over the
// window list; kernels: windowed.hip.
#include <climits>
#include <vector>

#include "../../include/ext/fsnp_windowed.h"
#include "fsnp_handle.h"
#include "pcm.h"
#include "windowed.h"

namespace fsnp {
namespace {

int ensure_window_stage(fsnp_handle* h, size_t bytes, hipStream_t s) {      // stream-ordered, like ensure_io
    if (bytes <= h->win_stage_bytes) return 0;
    if (order_after_last_forward(h, s)) return 4;
    unsigned char* n = nullptr;
    FSNP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&n), bytes, s));
    if (h->win_stage) FSNP_HIP_CHECK(hipFreeAsync(h->win_stage, s));
    h->win_stage = n;
    h->win_stage_bytes = bytes;
    return 0;
}

}  // namespace

// (shared with the window sessions, fsnp_window_stream_abi.hip: fsnp_handle.h)
const WindowFade* find_window_fade(const fsnp_handle* h, int V) {
    for (const WindowFade& f : h->win_fades)
        if (f.overlap == V) return &f;
    return nullptr;
}
// the fade table of overlap V on s, built and uploaded on first use (the caller is between order_after_last_forward and
// mark_forward_done, and has checked that the handle has room for it)
int window_fade_device(fsnp_handle* h, int V, hipStream_t s, const float*& g) {
    const WindowFade* f = find_window_fade(h, V);
    if (!f) {
        h->win_fades.reserve(kWindowMaxFades);                     // (entries never move: uploads in flight read their host copies)
        h->win_fades.emplace_back();
        WindowFade& n = h->win_fades.back();
        n.overlap = V;
        n.host.resize(V);
        window_fade_table(V, n.host.data());
        hipError_t e = hipMallocAsync(reinterpret_cast<void**>(&n.dev), (size_t)V * 4, s);
        if (e == hipSuccess) e = hipMemcpyAsync(n.dev, n.host.data(), (size_t)V * 4, hipMemcpyHostToDevice, s);
        if (e != hipSuccess) {
            if (n.dev) (void)hipFreeAsync(n.dev, s);
            h->win_fades.pop_back();
            set_error("cross-fade table of overlap %d: %s", V, hipGetErrorString(e));
            return 4;
        }
        f = &n;
    }
    g = f->dev;
    return 0;
}

namespace {

// Both entry points.  model = false (fsnp_debug_window_roundtrip): a forward copies every padded row's centre into its staging row.
int windowed_any(fsnp_handle* h, const char* where, const PcmIn& wav, const PcmOut& out, const int32_t* samples, int32_t batch,
                 int32_t max_samples, int32_t W, int32_t V, int32_t max_batch, void* hip_stream, bool model) {
    if (batch <= 0 || max_samples <= 0) { set_error("%s: empty input", where); return 2; }
    if (max_samples > INT_MAX - 4096) { set_error("%s: max_samples %d does not fit", where, (int)max_samples); return 2; }
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
    if (W > INT_MAX / 2) { set_error("%s: window %d does not fit", where, (int)W); return 2; }
    if (!find_window_fade(h, V) && (int)h->win_fades.size() >= kWindowMaxFades) {
        set_error("%s: this handle already keeps the cross-fade tables of %d overlaps, the most it holds (they are never evicted: launches "
                  "in flight may read them); overlap %d needs another handle", where, kWindowMaxFades, (int)V);
        return 2;
    }
    // the plan: the windows of all clips, clip by clip
    const int S = W - V;
    std::vector<ClipRow> clips(batch);
    std::vector<WindowRow> windows;
    for (int b = 0; b < batch; ++b) {
        const int L = samples ? samples[b] : max_samples;
        if (L <= p.half || L > max_samples) {
            set_error("%s: clip %d: %d samples outside (n_fft/2 = %d, %d] (reflect padding)", where, b, L, p.half, (int)max_samples);
            return 2;
        }
        const long K = window_count(L, W, V);
        if ((long)windows.size() + K > INT_MAX / 2) { set_error("%s: more than %d windows", where, INT_MAX / 2); return 2; }
        clips[b] = ClipRow{(int)windows.size(), L, (int)K};
        for (long k = 0; k < K; ++k) {
            const long at = k * S;
            windows.push_back(WindowRow{b, (int)at, (int)(L - at < W ? L - at : W)});
        }
    }
    const int total = (int)windows.size();
    // the forwards: max_batch consecutive windows each.  Every check of every forward before anything is enqueued
    struct Forward { int first, n, longest; bool ragged; };
    std::vector<Forward> forwards;
    std::vector<int32_t> lens(total), frames(total);
    int nmax = 0, longest = 0;
    for (int f0 = 0; f0 < total; f0 += max_batch) {
        Forward f{f0, total - f0 < max_batch ? total - f0 : (int)max_batch, 0, false};
        for (int r = 0; r < f.n; ++r) {
            lens[f0 + r] = windows[f0 + r].len;
            frames[f0 + r] = 1 + lens[f0 + r] / p.hop;
            f.longest = lens[f0 + r] > f.longest ? lens[f0 + r] : f.longest;
            f.ragged = f.ragged || lens[f0 + r] != lens[f0];
        }
        if (model && f.ragged)
            if (const int rc = check_lengths(h, frames.data() + f0, f.n, 1 + f.longest / p.hop, where)) return rc;
        nmax = f.n > nmax ? f.n : nmax;
        longest = f.longest > longest ? f.longest : longest;
        forwards.push_back(f);
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    // areas: the model's io area for the largest forward (wave_io grows with both arguments, so every forward's own layout fits), the
    // staging rows [total][W] and, for FSNP_SAMPLE_S16_PEAK, the merged fp32 rows [batch][max_samples] and their maxima behind them
    const WaveIo io_max = wave_io(p, nmax, longest);
    const size_t stage_rows = align_up((size_t)total * W * 4, 256), peak_rows = align_up((size_t)batch * max_samples * 4, 256);
    if (order_after_last_forward(h, s)) return 4;
    if (ensure_io(h, model ? io_max.total : io_max.noisy, s)) return 4;
    if (ensure_window_stage(h, stage_rows + (out.fmt == kPcmPeak ? peak_rows + (size_t)batch * 4 : 0), s)) return 4;
    const float* g = nullptr;
    if (const int rc = window_fade_device(h, V, s, g)) return rc;
    float* stage = reinterpret_cast<float*>(h->win_stage);
    for (const Forward& f : forwards) {
        const WaveIo io = wave_io(p, f.n, f.longest);
        float* xp = reinterpret_cast<float*>(h->io + io.xp);
        float* rows = stage + (size_t)f.first * W;
        launch_stft_pad_window(wav, xp, io.xs, windows.data() + f.first, f.n, p.n_fft, s);
        if (!model) {
            FSNP_HIP_CHECK(hipMemcpy2DAsync(rows, (size_t)W * 4, xp + p.half, (size_t)io.xs * 4, (size_t)f.longest * 4, f.n,
                                            hipMemcpyDeviceToDevice, s));
            continue;
        }
        if (const int rc = enhance_padded(h, p, io, f.n, f.ragged ? frames.data() + f.first : nullptr, hip_stream)) return rc;
        launch_istft_ola(reinterpret_cast<const float*>(h->io + io.fr), h->d_stft + p.o_win, pcm_out_f32(rows, W), f.n, io.T, f.longest,
                         f.ragged ? lens.data() + f.first : nullptr, p.n_fft, p.hop, s);
    }
    // the samples out, in the caller's format (FSNP_SAMPLE_S16_PEAK: merged fp32 rows and the clips' maxima first, as in enhance_wave_any)
    PcmOut o = out;
    if (out.clipped) FSNP_HIP_CHECK(hipMemsetAsync(out.clipped, 0, (size_t)batch * 4, s));
    if (out.fmt != kPcmS16) o.clipped = nullptr;
    float* merged = reinterpret_cast<float*>(h->win_stage + stage_rows);
    if (out.fmt == kPcmPeak) {
        unsigned* peak = reinterpret_cast<unsigned*>(h->win_stage + stage_rows + peak_rows);
        FSNP_HIP_CHECK(hipMemsetAsync(peak, 0, (size_t)batch * 4, s));
        o = PcmOut{merged, (long)max_samples, 1, kPcmPeak, nullptr, peak};
    }
    launch_window_merge(stage, g, o, clips.data(), batch, max_samples, W, V, s);
    if (out.fmt == kPcmPeak)
        launch_pcm_peak_scale(merged, max_samples, o.peak, PcmOut{out.p, out.stride, out.step, kPcmS16, nullptr, nullptr}, batch, max_samples, s);
    FSNP_HIP_CHECK(hipGetLastError());
    return mark_forward_done(h, s);
}

int windowed_entry(fsnp_handle* h, const char* where, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                   int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch, int32_t max_samples,
                   int32_t window, int32_t overlap, int32_t max_batch, int32_t* clipped, void* hip_stream, bool model) {
    if (!h || !wav || !out) { set_error("%s: null argument", where); return 1; }
    if (const int rc = check_sample_format(where, "input", in_format, wav_step, false)) return rc;
    if (const int rc = check_sample_format(where, "output", out_format, out_step, true)) return rc;
    return windowed_any(h, where, PcmIn{wav, (long)wav_stride, (long)wav_step, in_format},
                        PcmOut{out, (long)out_stride, (long)out_step, out_format, clipped, nullptr}, samples, batch, max_samples, window,
                        overlap, max_batch, hip_stream, model);
}

}  // namespace
}  // namespace fsnp

extern "C" {

int64_t fsnp_window_count(int64_t samples, int32_t window, int32_t overlap) {
    if (window < 2 || overlap < 1 || overlap > window / 2 || samples < 1) return -1;
    return window_count((long)samples, window, overlap);
}

int fsnp_enhance_wave_windowed(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                               int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch,
                               int32_t max_samples, int32_t window, int32_t overlap, int32_t max_batch, int32_t* clipped,
                               void* hip_stream) {
    return windowed_entry(h, "fsnp_enhance_wave_windowed", wav, in_format, wav_stride, wav_step, out, out_format, out_stride, out_step,
                          samples, batch, max_samples, window, overlap, max_batch, clipped, hip_stream, true);
}

int fsnp_debug_window_roundtrip(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                                int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch,
                                int32_t max_samples, int32_t window, int32_t overlap, int32_t max_batch, int32_t* clipped,
                                void* hip_stream) {
    return windowed_entry(h, "fsnp_debug_window_roundtrip", wav, in_format, wav_stride, wav_step, out, out_format, out_stride, out_step,
                          samples, batch, max_samples, window, overlap, max_batch, clipped, hip_stream, false);
}

}  // extern "C"
