/*
 * fsnp_windowed.h - one long recording enhanced in overlapping windows that are cross-faded on the device.  An extension header of
 * libfsnp_hip.so: it includes fsnp.h, fsnp.h does not include it; same library, same FSNP_ABI_VERSION.  The contract below, with the
 * kernels' side and the measurements, is DESIGN.md section 8f; a serving example is in INTEGRATION.md ("One long recording").
 *
 * Why.  Both models see the whole input (offline norms, pooling, GroupNorm, non-causal convolutions): a clip is the unit they were
 * trained on, 2 - 10 s.  A recording of minutes is therefore cut into windows of such a length, every window is enhanced as a clip of
 * its own, and the windows are joined by a raised-cosine cross-fade over their overlap.
 *
 * Plan (all counts in samples at the model's rate).  window W, overlap V with n_fft / 2 <= V <= W / 2 (n_fft = 2 (num_freqs - 1)),
 * stride S = W - V.  A clip of L > n_fft / 2 samples has
 *     K = 1                       if L <= W
 *     K = ceil((L - V) / S)       otherwise
 * windows; window k covers [k S, min(k S + W, L)).  Every window but the last has W samples, the last one of K > 1 has more than V,
 * every sample lies in one or two windows, and windows k - 1 and k share exactly [k S, k S + V).
 *
 * Result.  y_k = fsnp_enhance_wave of window k alone (its own reflect padding, frames and norms; all bins).  Sample i of the clip, with
 * k = min(i / S, K - 1) and j = i - k S:
 *     out[i] = y_k[j]                                                    if k = 0 or j >= V
 *     out[i] = fmaf(g[j], y_k[j] - y_{k-1}[S + j], y_{k-1}[S + j])       otherwise
 * g[j] = 0.5 - 0.5 cos(pi j / V), j = 0 ... V - 1, computed in double and rounded to fp32.  The clip's own start and end are not
 * faded.  With `samples`, row b is this result of its first samples[b] samples alone and exactly 0 behind them.  The result is NOT
 * fsnp_enhance_wave of the whole clip (every statistic there is taken over the whole recording).
 *
 * Execution.  The windows of all clips are listed clip by clip, and the model runs on max_batch consecutive windows of that list at
 * a time (a forward may hold windows of several clips).  A forward whose windows all have one length is the equal-length call; one
 * with different lengths is the fsnp_forward_complex_lengths call of fsnp_lengths.h, with what that refuses.  A call in which every
 * clip has one window and batch <= max_batch is therefore the forward of fsnp_enhance_wave_pcm, bit for bit.
 *
 * Memory.  Windows are read in place from `wav`; their enhanced fp32 samples wait in a staging area of the handle of
 * 4 W sum_b K_b bytes (FSNP_SAMPLE_S16_PEAK: + 4 batch (max_samples + 1)), grown in stream order like the handle's other areas and
 * freed by fsnp_destroy; the model's areas are those of a batch of min(max_batch, sum_b K_b) clips of W samples.
 *
 * Stream-ordered on hip_stream, no host or device synchronisation.  Refusals come before anything is enqueued, with the reason in
 * fsnp_last_error: code 1 for a NULL handle or buffer, code 2 for the rest (each message names the function and the offending value).
 */
#ifndef FSNP_EXT_WINDOWED_H
#define FSNP_EXT_WINDOWED_H

#include "../fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* K of the plan above for a clip of `samples` samples.  Host arithmetic, no handle, no GPU.  -1 for what needs no handle to refuse:
 * window < 2, overlap outside [1, window / 2], samples < 1.  (n_fft / 2 <= overlap is a rule of a handle's geometry.) */
int64_t fsnp_window_count(int64_t samples, int32_t window, int32_t overlap);

/* wav -> out as defined above.  Buffers, formats and steps as in fsnp_pcm.h (out_format may be FSNP_SAMPLE_S16_PEAK: the peak is
 * that of the clip's merged samples); `out` must not overlap `wav`.  samples: NULL (every row holds max_samples samples) or HOST
 * int32 [batch], read during the call.  clipped: NULL or DEVICE int32 [batch], as in fsnp_pcm.h.
 * Code 2: overlap outside [n_fft / 2, window / 2] at the handle's geometry; max_batch < 1; a clip of <= n_fft / 2 samples; a model that
 * fsnp_forward_complex_lengths refuses (subband_num > 1, sub-band sequence_model "TCN") or a window that it refuses, whenever a
 * planned forward holds windows of different lengths; output_size != 2; weights not committed; a ninth distinct overlap on one
 * handle (the cross-fade table of an overlap is uploaded once and kept until fsnp_destroy, eight per handle). */
int fsnp_enhance_wave_windowed(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                               int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch,
                               int32_t max_samples, int32_t window, int32_t overlap, int32_t max_batch, int32_t* clipped,
                               void* hip_stream);

/* Test hook: the same call with STFT -> model -> iSTFT replaced by a device copy of every padded window's centre into its staging
 * row, so that only the plan, the window-pad kernel and the merge kernel run.  Needs no committed weights.  fmaf(g, a - a, a) = a:
 * the output equals the input bit for bit (fp32 in -> fp32 out, int16 in -> FSNP_SAMPLE_S16 out), 0 behind every clip's length. */
int fsnp_debug_window_roundtrip(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                                int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch,
                                int32_t max_samples, int32_t window, int32_t overlap, int32_t max_batch, int32_t* clipped,
                                void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_EXT_WINDOWED_H */
