/*
 * fsnp_lengths.h - batches of clips of different lengths (ABI 13): the forward, the STFT-domain forward, the cIRM epilogue and the
 * waveform path with a length per utterance.  Part of the public surface of libfsnp_hip.so next to fsnp.h (which includes this header), same
 * FSNP_ABI_VERSION.  What "a batch of clips of different lengths" computes, and why the caller cannot get it by zero padding, is
 * in DESIGN.md ("Clips of different lengths"); how to batch a directory of clips with it is in INTEGRATION.md.
 */
#ifndef FSNP_LENGTHS_H
#define FSNP_LENGTHS_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Clips of different lengths in one batch (ABI 12).  Row b of the [batch, 1, F, frames] input holds a clip of lengths[b] frames,
 * 1 <= lengths[b] <= frames; what lies at frames >= lengths[b] is never read (it may be anything, NaN included).  Row b of `out`
 * ([batch, output_size, F, frames], FULL mode: all bins, per-utterance semantics) is, at frames [0, lengths[b]), the B = 1 forward of
 * that clip alone (x[b:b+1, ..., :lengths[b]]): every per-utterance reduction - both offline norms, the channel attention's pooling
 * over time, the GroupNorms of the full-band TCN blocks, the non-causal depthwise conv's zero padding - ends at the clip's own
 * lengths[b] + look_ahead frames; at frames [lengths[b], frames) it is written as exactly 0.
 *   lengths : HOST int32 [batch], read during the call only (the caller may reuse the buffer as soon as it returns).  They reach the
 *             device as kernel arguments: the call is stream-ordered like fsnp_forward, with no host or device synchronisation.
 * Validated before anything is enqueued; code 2, naming the utterance, for a length outside [1, frames] or (TSSE) below the largest
 * kersize minus look_ahead; code 2 as well for handles these calls do not cover: subband_num > 1 and the sub-band sequence_model
 * "TCN".  Pipelining (fsnp_set_pipeline), fsnp_set_verify / fsnp_set_verify_sample and fsnp_watch_weights apply as to fsnp_forward;
 * after fsnp_reserve(h, max_batch, max_frames, FSNP_MODE_FULL, ...) these calls never grow the workspace.  Other arguments as
 * fsnp_forward / fsnp_forward_complex with mode = FSNP_MODE_FULL, batch_offset = 0, global_batch = batch. */
int fsnp_forward_lengths(fsnp_handle* h, const float* mag, const float* real, const float* imag, const int64_t strides[3][3],
                         const int32_t* lengths, float* out, int32_t batch, int32_t frames, void* hip_stream);
int fsnp_forward_complex_lengths(fsnp_handle* h, const float* noisy, const int64_t strides[3], const int32_t* lengths, float* out,
                                 int32_t batch, int32_t frames, void* hip_stream);
/* fsnp_apply_cirm (fsnp.h) of clips of different lengths: row b is lengths[b] frames long (HOST int32 [batch], 1 <= lengths[b] <=
 * frames, read during the call and passed as kernel arguments).  Element (b, f, t) of `out` is fsnp_apply_cirm's at t < lengths[b] and
 * exactly 0 at t >= lengths[b]; neither `mask` nor `noisy` is read there (they may hold anything, NaN included).  Code 2, naming the
 * utterance, for a length outside [1, frames]. */
int fsnp_apply_cirm_lengths(const float* mask, const float* noisy, const int64_t strides[3], float* out, const int64_t out_strides[3],
                            const int32_t* lengths, int32_t batch, int32_t freqs, int32_t frames, void* hip_stream);
/* fsnp_enhance_wave of clips of different lengths: row b of wav holds samples[b] samples (HOST int32 [batch], read during the call),
 * n_fft / 2 < samples[b] <= max_samples.  The STFT reflects at each clip's own end and gives it T_b = 1 + samples[b] / hop frames, the
 * model runs as fsnp_forward_complex_lengths with those, the iSTFT overlap-adds and normalises over those T_b frames only and trims to
 * samples[b] (the cIRM epilogue is fsnp_apply_cirm_lengths with those T_b); out row b at samples >= samples[b] is written as 0.  Row b
 * equals fsnp_enhance_wave of that clip alone. */
int fsnp_enhance_wave_lengths(fsnp_handle* h, const float* wav, int64_t wav_stride, float* out, int64_t out_stride,
                              const int32_t* samples, int32_t batch, int32_t max_samples, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_LENGTHS_H */
