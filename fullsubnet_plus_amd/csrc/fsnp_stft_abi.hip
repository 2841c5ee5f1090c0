// fsnp_stft_abi.hip - the STFT / iSTFT / waveform entry points of the C ABI: torch.stft / torch.istft of
// audio_zen/acoustics/feature.py:10-56 as DFT GEMMs (kernels: stft.hip, tcn.hip) and the inferencer's inner loop
// (fullsubnet_plus/inferencer/inferencer.py:142-158) as one call.  Host code only.
#include <vector>

#include "fsnp_handle.h"
#include "pcm.h"
#include "resample.h"

// ---------------------------------------------------------------------------------------------- STFT / iSTFT (f-3)
namespace fsnp {
StftPlan stft_plan(const fsnp_handle* h) {
    StftPlan p{};
    p.F = h->F; p.n_fft = 2 * (h->F - 1); p.half = p.n_fft / 2; p.hop = h->hop_length ? h->hop_length : p.half;
    p.N2 = 2 * p.F; p.sp = (int)align_up(p.N2, 4);
    p.fwd_ld = (int)align_up(p.n_fft, 16); p.inv_ld = (int)align_up(p.N2, 16); p.xl = (int)align_up(p.n_fft, 4);
    p.o_fwd = 0;
    p.o_inv = p.o_fwd + align_up(p.N2, 384) * (size_t)p.fwd_ld;
    p.o_win = p.o_inv + align_up(p.n_fft, 384) * (size_t)p.inv_ld;
    p.o_zero = p.o_win + align_up(p.n_fft, 64);
    p.total = p.o_zero + align_up(p.N2 > p.n_fft ? p.N2 : p.n_fft, 384);
    return p;
}
// the rules of include/fsnp_stft_geometry.h
int check_hop_length(int F, int hop, const char* where) {
    const int n_fft = 2 * (F - 1);
    if (F < 3) { set_error("%s: the waveform path needs num_freqs >= 3 (n_fft = 2 (num_freqs - 1)); this handle: %d", where, F); return 2; }
    if (hop <= 0 || 2L * hop > n_fft || 8L * hop < n_fft) {
        set_error("%s: hop_length %d outside [n_fft / 8, n_fft / 2] = [%d, %d] (n_fft = 2 (num_freqs - 1) = %d): above it frames no longer "
                  "cover the clip's tail, below it is outside what the waveform path is built for", where, hop, (n_fft + 7) / 8, n_fft / 2, n_fft);
        return 2;
    }
    if (hop % 4) {
        set_error("%s: hop_length %d is not a multiple of 4: the forward DFT GEMM reads frame t at float t * hop_length of the padded signal "
                  "as 16-byte vectors", where, hop);
        return 2;
    }
    return 0;
}
int ensure_stft(fsnp_handle* h) {
    if (check_hop_length(h->F, stft_plan(h).hop, "STFT")) return 2;       // (the default hop of a num_freqs - 1 that is no multiple of 4)
    if (h->d_stft) return 0;
    const StftPlan p = stft_plan(h);
    std::vector<float> host(p.total, 0.0f);
    stft_build_matrices(p.n_fft, host.data() + p.o_fwd, host.data() + p.o_inv, host.data() + p.o_win);
    FSNP_ON_DEVICE(h);
    FSNP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->d_stft), p.total * sizeof(float)));
    FSNP_HIP_CHECK(hipMemcpy(h->d_stft, host.data(), p.total * sizeof(float), hipMemcpyHostToDevice));
    return 0;
}
int ensure_io(fsnp_handle* h, size_t bytes, hipStream_t s) {      // stream-ordered, like ensure_workspace
    if (bytes <= h->io_bytes) return 0;
    if (order_after_last_forward(h, s)) return 4;
    unsigned char* nio = nullptr;
    FSNP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&nio), bytes, s));
    if (h->io) FSNP_HIP_CHECK(hipFreeAsync(h->io, s));
    h->io = nio;
    h->io_bytes = bytes;
    return 0;
}
__global__ void spec_repack_kernel(const float2* __restrict__ in, long sb, long sf, long st, float2* __restrict__ out, int B,
                                   int F, int T, int spc) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;     // (b, t, f) over the padded row of spc complex elements
    if (i >= (long)B * T * spc) return;
    const int f = (int)(i % spc), t = (int)((i / spc) % T), b = (int)(i / ((long)spc * T));
    out[i] = f < F ? in[b * sb + f * sf + t * st] : make_float2(0.f, 0.f);
}
WaveIo wave_io(const StftPlan& p, int batch, int max_samples, int stage_samples) {
    WaveIo io{};
    io.T = 1 + max_samples / p.hop;
    io.xs = (long)align_up((size_t)max_samples + p.n_fft, 4);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    const size_t spec = (size_t)batch * io.T * p.sp * 4 + 256;
    io.xp = take((size_t)batch * io.xs * 4);
    io.noisy = take(spec);
    io.enh = take(spec);
    io.mask = take((size_t)batch * 2 * p.F * io.T * 4);
    io.fr = o;
    io.total = io.fr + (size_t)batch * io.T * p.n_fft * 4;
    io.stage = align_up(io.total, 256);
    if (stage_samples > 0) io.total = io.stage + (size_t)batch * stage_samples * 4;
    return io;
}
// fsnp_enhance_wave_rate: the clips arrive and leave at another rate.  Every row holds n samples at the caller's rate (the call's
// max_samples is then the model-rate count ceil(n up / down) of the `in` direction, its `samples` NULL); the caller's output rows
// have cols >= n columns, written as 0 from n on
struct WaveRate {
    ResamplePlan in, out;      // caller's rate -> model's rate, and back
    int32_t n, cols;
};
// wav [B][L] -> spectrum rows [B][T][ldc] (interleaved complex), T = 1 + L / hop; samples: NULL, or each row's own HOST sample count
// (reflect padding at each clip's own end; frames past 1 + samples[b] / hop see zeros behind it)
static void stft_into(fsnp_handle* h, const StftPlan& p, const PcmIn& wav, float* xp, long xs, float* spec, int ldc, int B, int L,
                      const int* samples, hipStream_t s) {
    const int T = 1 + L / p.hop;
    launch_stft_pad(wav, xp, xs, B, L, samples, p.n_fft, s);
    launch_linear_act(xp, p.hop, h->d_stft + p.o_fwd, p.fwd_ld, h->d_stft + p.o_zero, spec, ldc, p.n_fft, p.N2, B, T,
                      FSNP_ACT_NONE, h->num_cus, s, xs, p.n_fft);
}
// spectrum rows [B][T][sp] -> wav [B][L]
static void istft_from(fsnp_handle* h, const StftPlan& p, const float* spec, float* frames, float* wav, long wav_stride, int B,
                       int T, int L, hipStream_t s) {
    launch_linear_act(spec, p.sp, h->d_stft + p.o_inv, p.inv_ld, h->d_stft + p.o_zero, frames, p.n_fft, p.N2, p.n_fft, B, T,
                      FSNP_ACT_NONE, h->num_cus, s, (long)T * p.sp, p.N2);
    launch_istft_ola(frames, h->d_stft + p.o_win, pcm_out_f32(wav, wav_stride), B, T, L, nullptr, p.n_fft, p.hop, s);   // all T frames
}
// the format and step rules of include/fsnp_pcm.h for one buffer (peak_ok: FSNP_SAMPLE_S16_PEAK is a format of this buffer)
int check_sample_format(const char* where, const char* what, int32_t format, int64_t step, bool peak_ok) {
    if (format != FSNP_SAMPLE_F32 && format != FSNP_SAMPLE_S16 && format != FSNP_SAMPLE_S16_PEAK) {
        set_error("%s: unknown %s format %d (FSNP_SAMPLE_F32 = 0, FSNP_SAMPLE_S16 = 1, FSNP_SAMPLE_S16_PEAK = 2)", where, what, (int)format);
        return 2;
    }
    if (format == FSNP_SAMPLE_S16_PEAK && !peak_ok) {
        set_error("%s: FSNP_SAMPLE_S16_PEAK is an output format of whole-clip calls only (%s): a stream has no peak, an input no scale", where, what);
        return 2;
    }
    if (step < 1) { set_error("%s: %s step %lld < 1 (elements between consecutive samples of a row)", where, what, (long long)step); return 2; }
    return 0;
}

// The model between the two sample kernels of a waveform call: the padded rows xp [batch][io.xs] of h->io (already written on the
// stream) -> the inverse DFT's frames [batch][io.T][n_fft] at io.fr.  frames: NULL (every row has io.T frames), or each row's own HOST
// frame count, already accepted by check_lengths.  Shared by enhance_wave_any and the windowed call (fsnp_windowed_abi.hip).
int enhance_padded(fsnp_handle* h, const StftPlan& p, const WaveIo& io, int batch, const int32_t* frames, void* hip_stream) {
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    const int T = io.T;
    float* xp = reinterpret_cast<float*>(h->io + io.xp);
    float* noisy = reinterpret_cast<float*>(h->io + io.noisy);
    float* enh = reinterpret_cast<float*>(h->io + io.enh);
    float* mask = reinterpret_cast<float*>(h->io + io.mask);
    float* fr = reinterpret_cast<float*>(h->io + io.fr);
    launch_linear_act(xp, p.hop, h->d_stft + p.o_fwd, p.fwd_ld, h->d_stft + p.o_zero, noisy, p.sp, p.n_fft, p.N2, batch, T,
                      FSNP_ACT_NONE, h->num_cus, s, io.xs, p.n_fft);
    const int64_t cst[3] = {(int64_t)T * (p.sp / 2), 1, p.sp / 2};       // complex-element strides of [B][T][sp/2] as (b, f, t)
    const int rc = frames ? fsnp_forward_complex_lengths(h, noisy, cst, frames, mask, batch, T, hip_stream)
                          : fsnp_forward_complex(h, noisy, cst, mask, batch, T, FSNP_MODE_FULL, 0, batch, hip_stream);
    if (rc) return rc;
    // pipelined mode: the forward left chunks of the sub-band plan on the side stream (at B = 1 the whole plan); `mask` is read
    // right here and lives in the single-buffered io area, so `s` waits for them now (fsnp_flush) - nothing of this call is deferred
    if (h->pipeline && fsnp_flush(h, hip_stream)) return 4;
    // the pad column of every row of `enh` is never written by apply_cirm and multiplies zero weights: clear it once
    FSNP_HIP_CHECK(hipMemsetAsync(enh, 0, io.mask - io.enh, s));
    launch_apply_cirm(mask, noisy, cst, enh, cst, batch, p.F, T, frames, s);      // frames >= T_b: 0
    launch_linear_act(enh, p.sp, h->d_stft + p.o_inv, p.inv_ld, h->d_stft + p.o_zero, fr, p.n_fft, p.N2, p.n_fft, batch, T,
                      FSNP_ACT_NONE, h->num_cus, s, (long)T * p.sp, p.N2);
    return 0;
}

namespace {
int stft_any(fsnp_handle* h, const char* where, const PcmIn& wav, float* spec, int32_t batch, int32_t samples, void* hip_stream) {
    if (batch <= 0) { set_error("%s: empty input", where); return 2; }
    if (ensure_stft(h)) return 2;
    const StftPlan p = stft_plan(h);
    if (samples <= p.half) { set_error("%s: need more than n_fft/2 = %d samples (reflect padding)", where, p.half); return 2; }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    const long xs = (long)align_up((size_t)samples + p.n_fft, 4);
    if (order_after_last_forward(h, s)) return 4;
    if (ensure_io(h, (size_t)batch * xs * 4, s)) return 4;
    stft_into(h, p, wav, reinterpret_cast<float*>(h->io), xs, spec, p.N2, batch, samples, nullptr, s);
    FSNP_HIP_CHECK(hipGetLastError());
    return mark_forward_done(h, s);
}

// fsnp_enhance_wave (samples = NULL: every row holds max_samples samples) and fsnp_enhance_wave_lengths behind every entry point;
// out.fmt may be kPcmPeak, out.clipped the caller's (NULL or device int32 [batch], overwritten)
int enhance_wave_any(fsnp_handle* h, const char* where, const PcmIn& wav, const PcmOut& out, const int32_t* samples, int32_t batch,
                     int32_t max_samples, void* hip_stream, const WaveRate* rate = nullptr) {
    if (batch <= 0) { set_error("%s: empty input", where); return 2; }
    if (!h->committed) { set_error("%s: weights not committed (call fsnp_commit_weights)", where); return 2; }
    // the cIRM epilogue multiplies by exactly two mask planes (decompress_cIRM, audio_zen/acoustics/mask.py:60-63) and the io area is
    // sized for them: a model built with another output_size has no waveform path
    if (h->cfg.output_size != 2) { set_error("%s: the cIRM epilogue needs output_size = 2 (this handle: %d)", where, h->cfg.output_size); return 2; }
    if (ensure_stft(h)) return 2;
    const StftPlan p = stft_plan(h);
    if (max_samples <= p.half) {
        set_error("%s: need more than n_fft/2 = %d samples%s (reflect padding)", where, p.half, rate ? " at the model's rate" : "");
        return 2;
    }
    // every check of the forward too, before anything is enqueued: each clip's frame count is its own STFT's, T_b = 1 + samples[b] / hop
    const int T = 1 + max_samples / p.hop;
    std::vector<int32_t> frames;
    if (samples) {
        frames.resize(batch);
        for (int b = 0; b < batch; ++b) {
            if (samples[b] <= p.half || samples[b] > max_samples) {
                set_error("%s: utterance %d: %d samples outside (n_fft/2 = %d, %d]", where, b, (int)samples[b], p.half, max_samples);
                return 2;
            }
            frames[b] = 1 + samples[b] / p.hop;
        }
        if (const int rc = check_lengths(h, frames.data(), batch, T, where)) return rc;
    }
    if (rate) {
        const ResamplePlan both[2] = {rate->in, rate->out};
        if (const int rc = resample_room(h, where, both, 2)) return rc;
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    const WaveIo io = wave_io(p, batch, max_samples, rate ? rate->cols : 0);
    const long xs = io.xs;
    if (order_after_last_forward(h, s)) return 4;
    if (ensure_io(h, io.total, s)) return 4;
    ResampleTable tin{}, tout{};
    if (rate) {
        if (const int rc = resample_table(h, rate->in, s, tin)) return rc;
        if (const int rc = resample_table(h, rate->out, s, tout)) return rc;
    }
    float* xp = reinterpret_cast<float*>(h->io + io.xp);
    float* noisy = reinterpret_cast<float*>(h->io + io.noisy);
    float* fr = reinterpret_cast<float*>(h->io + io.fr);
    // inferencer.py:142-158: stft -> (mag, real, imag) -> model -> decompress_cIRM, complex multiply -> istft(length); with lengths
    // the reflect padding at each clip's end (frames past T_b see zeros: the forward never reads them)
    if (rate) launch_stft_pad_resample(wav, xp, xs, batch, nullptr, rate->n, p.n_fft, tin, s);
    else launch_stft_pad(wav, xp, xs, batch, max_samples, samples, p.n_fft, s);
    if (const int rc = enhance_padded(h, p, io, batch, samples ? frames.data() : nullptr, hip_stream)) return rc;
    // the samples out, in the caller's format.  FSNP_SAMPLE_S16_PEAK needs the clip's peak before any sample can be written: the
    // overlap-add stages fp32 rows where the padded input was and folds |v| into per-row maxima where the noisy spectra were (both are
    // dead by now, so the area fsnp_reserve sized is enough), and a second kernel scales and truncates
    PcmOut o = out;
    if (out.clipped) FSNP_HIP_CHECK(hipMemsetAsync(out.clipped, 0, (size_t)batch * 4, s));
    if (out.fmt != kPcmS16) o.clipped = nullptr;                          // nothing clips in the other formats
    if (rate) {
        // another rate out: the overlap-add stages its fp32 model-rate rows where the padded input was, as the peak format does, and
        // the resample kernel converts them into the caller's first n samples in the caller's format (n <= what n16 samples convert to).
        // FSNP_SAMPLE_S16_PEAK: its first pass, into the staging rows at the caller's rate behind everything else
        launch_istft_ola(fr, h->d_stft + p.o_win, pcm_out_f32(xp, xs), batch, T, max_samples, samples, p.n_fft, p.hop, s);
        float* stage = reinterpret_cast<float*>(h->io + io.stage);
        if (out.fmt == kPcmPeak) {
            FSNP_HIP_CHECK(hipMemsetAsync(noisy, 0, (size_t)batch * 4, s));
            o = PcmOut{stage, (long)rate->cols, 1, kPcmPeak, nullptr, reinterpret_cast<unsigned*>(noisy)};
        }
        launch_resample(pcm_in_f32(xp, xs), o, tout, batch, nullptr, rate->n, rate->cols, true, s);
        if (out.fmt == kPcmPeak)
            launch_pcm_peak_scale(stage, rate->cols, o.peak, PcmOut{out.p, out.stride, out.step, kPcmS16, nullptr, nullptr}, batch, rate->cols, s);
        FSNP_HIP_CHECK(hipGetLastError());
        return mark_forward_done(h, s);
    }
    if (out.fmt == kPcmPeak) {
        FSNP_HIP_CHECK(hipMemsetAsync(noisy, 0, (size_t)batch * 4, s));
        o = PcmOut{xp, xs, 1, kPcmPeak, nullptr, reinterpret_cast<unsigned*>(noisy)};
    }
    launch_istft_ola(fr, h->d_stft + p.o_win, o, batch, T, max_samples, samples, p.n_fft, p.hop, s);
    if (out.fmt == kPcmPeak)
        launch_pcm_peak_scale(xp, xs, o.peak, PcmOut{out.p, out.stride, out.step, kPcmS16, nullptr, nullptr}, batch, max_samples, s);
    FSNP_HIP_CHECK(hipGetLastError());
    return mark_forward_done(h, s);
}
}  // namespace
}  // namespace fsnp

extern "C" {

int fsnp_stft(fsnp_handle* h, const float* wav, int64_t wav_stride, float* spec, int32_t batch, int32_t samples, void* hip_stream) {
    if (!h || !wav || !spec) { set_error("fsnp_stft: null argument"); return 1; }
    return stft_any(h, "fsnp_stft", pcm_in_f32(wav, (long)wav_stride), spec, batch, samples, hip_stream);
}

int fsnp_stft_pcm(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, float* spec, int32_t batch,
                  int32_t samples, void* hip_stream) {
    if (!h || !wav || !spec) { set_error("fsnp_stft_pcm: null argument"); return 1; }
    if (const int rc = check_sample_format("fsnp_stft_pcm", "input", in_format, wav_step, false)) return rc;
    return stft_any(h, "fsnp_stft_pcm", PcmIn{wav, (long)wav_stride, (long)wav_step, in_format}, spec, batch, samples, hip_stream);
}

int fsnp_istft(fsnp_handle* h, const float* spec, const int64_t strides[3], float* wav, int64_t wav_stride, int32_t batch,
               int32_t frames, int32_t samples, void* hip_stream) {
    if (!h || !spec || !strides || !wav) { set_error("fsnp_istft: null argument"); return 1; }
    if (batch <= 0 || frames <= 0 || samples <= 0) { set_error("fsnp_istft: empty input"); return 2; }
    if (ensure_stft(h)) return 2;
    const StftPlan p = stft_plan(h);
    if ((long)(frames - 1) * p.hop + p.n_fft < (long)samples + p.half) { set_error("fsnp_istft: %d frames do not cover %d samples", frames, samples); return 2; }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    const size_t spec_b = align_up((size_t)batch * frames * p.sp * 4 + 256, 256), fr_b = (size_t)batch * frames * p.n_fft * 4;
    if (order_after_last_forward(h, s)) return 4;
    if (ensure_io(h, spec_b + fr_b, s)) return 4;
    float* sp = reinterpret_cast<float*>(h->io);
    float* fr = reinterpret_cast<float*>(h->io + spec_b);
    const long n = (long)batch * frames * (p.sp / 2);
    hipLaunchKernelGGL(spec_repack_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, reinterpret_cast<const float2*>(spec),
                       (long)strides[0], (long)strides[1], (long)strides[2], reinterpret_cast<float2*>(sp), batch, p.F, frames, p.sp / 2);
    istft_from(h, p, sp, fr, wav, wav_stride, batch, frames, samples, s);
    FSNP_HIP_CHECK(hipGetLastError());
    return mark_forward_done(h, s);
}

int fsnp_enhance_wave(fsnp_handle* h, const float* wav, int64_t wav_stride, float* out, int64_t out_stride, int32_t batch,
                      int32_t samples, void* hip_stream) {
    if (!h || !wav || !out) { set_error("fsnp_enhance_wave: null argument"); return 1; }
    return enhance_wave_any(h, "fsnp_enhance_wave", pcm_in_f32(wav, (long)wav_stride), pcm_out_f32(out, (long)out_stride), nullptr, batch,
                            samples, hip_stream);
}

int fsnp_enhance_wave_lengths(fsnp_handle* h, const float* wav, int64_t wav_stride, float* out, int64_t out_stride, const int32_t* samples,
                              int32_t batch, int32_t max_samples, void* hip_stream) {
    if (!h || !wav || !out || !samples) { set_error("fsnp_enhance_wave_lengths: null argument"); return 1; }
    return enhance_wave_any(h, "fsnp_enhance_wave_lengths", pcm_in_f32(wav, (long)wav_stride), pcm_out_f32(out, (long)out_stride), samples,
                            batch, max_samples, hip_stream);
}

int fsnp_enhance_wave_pcm(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                          int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch,
                          int32_t max_samples, int32_t* clipped, void* hip_stream) {
    if (!h || !wav || !out) { set_error("fsnp_enhance_wave_pcm: null argument"); return 1; }
    if (const int rc = check_sample_format("fsnp_enhance_wave_pcm", "input", in_format, wav_step, false)) return rc;
    if (const int rc = check_sample_format("fsnp_enhance_wave_pcm", "output", out_format, out_step, true)) return rc;
    return enhance_wave_any(h, "fsnp_enhance_wave_pcm", PcmIn{wav, (long)wav_stride, (long)wav_step, in_format},
                            PcmOut{out, (long)out_stride, (long)out_step, out_format, clipped, nullptr}, samples, batch, max_samples, hip_stream);
}

// include/fsnp_resample.h: the same call at another sample rate (the other entry points of that header: fsnp_resample_abi.hip)
int fsnp_enhance_wave_rate(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                           int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch,
                           int32_t max_samples, int32_t* clipped, int32_t sample_rate, int32_t model_rate, void* hip_stream) {
    const char* where = "fsnp_enhance_wave_rate";
    if (!h || !wav || !out) { set_error("%s: null argument", where); return 1; }
    WaveRate rate{};
    if (const int rc = resample_plan(where, sample_rate, model_rate, rate.in)) return rc;
    if (const int rc = resample_plan(where, model_rate, sample_rate, rate.out)) return rc;
    if (rate.in.up == rate.in.down)
        return fsnp_enhance_wave_pcm(h, wav, in_format, wav_stride, wav_step, out, out_format, out_stride, out_step, samples, batch,
                                     max_samples, clipped, hip_stream);
    if (const int rc = check_sample_format(where, "input", in_format, wav_step, false)) return rc;
    if (const int rc = check_sample_format(where, "output", out_format, out_step, true)) return rc;
    if (batch <= 0 || max_samples <= 0) { set_error("%s: empty input", where); return 2; }
    const long long max16 = resample_length(rate.in, max_samples);
    if (max16 > INT32_MAX / 2) { set_error("%s: %lld model-rate samples per clip do not fit", where, max16); return 2; }
    rate.n = rate.cols = max_samples;
    const PcmIn in{wav, (long)wav_stride, (long)wav_step, in_format};
    const PcmOut o{out, (long)out_stride, (long)out_step, out_format, clipped, nullptr};
    if (!samples) return enhance_wave_any(h, where, in, o, nullptr, batch, (int32_t)max16, hip_stream, &rate);
    // With `samples`, row b IS that clip run alone: one call of batch 1 per row, so that a row has the bits of the clip converted,
    // enhanced and converted back on its own.  (One batch over all rows would not: the model's kernels are chosen by the batch size,
    // and their fp32 sums then run in another order - 1e-6 relative.)  A caller who prefers one batch's throughput to that pads the
    // clips to one length.  Every row is checked before anything is enqueued.
    if (ensure_stft(h)) return 2;
    const int half = stft_plan(h).half;
    for (int b = 0; b < batch; ++b) {
        if (samples[b] < 1 || samples[b] > max_samples) {
            set_error("%s: utterance %d: %d samples outside [1, %d]", where, b, (int)samples[b], (int)max_samples);
            return 2;
        }
        if (resample_length(rate.in, samples[b]) <= half) {
            set_error("%s: utterance %d: %d samples are %lld at the model's rate; need more than n_fft/2 = %d (reflect padding)", where, b,
                      (int)samples[b], resample_length(rate.in, samples[b]), half);
            return 2;
        }
    }
    for (int b = 0; b < batch; ++b) {
        PcmIn ib = in;
        PcmOut ob = o;
        ib.p = static_cast<const char*>(in.p) + (long)b * in.stride * (in.fmt == kPcmF32 ? 4 : 2);
        ob.p = static_cast<char*>(o.p) + (long)b * o.stride * (o.fmt == kPcmF32 ? 4 : 2);      // (the CALLER's buffer: int16 for both int16 formats)
        if (clipped) ob.clipped = clipped + b;
        rate.n = samples[b];
        if (const int rc = enhance_wave_any(h, where, ib, ob, nullptr, 1, (int32_t)resample_length(rate.in, samples[b]), hip_stream, &rate))
            return rc;
    }
    return 0;
}

// ---------------------------------------------------------------------------------------------- include/fsnp_stft_geometry.h
int fsnp_set_hop_length(fsnp_handle* h, int32_t hop_length) {
    if (!h) { set_error("fsnp_set_hop_length: null handle"); return 1; }
    if (const int rc = check_hop_length(h->F, hop_length, "fsnp_set_hop_length")) return rc;
    h->hop_length = hop_length;
    return 0;
}

int32_t fsnp_hop_length(const fsnp_handle* h) { return h ? stft_plan(h).hop : 0; }

}  // extern "C"
