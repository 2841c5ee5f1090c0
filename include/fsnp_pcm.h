/*
 * fsnp_pcm.h - 16-bit PCM at the boundary of the waveform path: int16 or strided samples in, int16 samples out.  Part of the public
 * surface of libfsnp_hip.so next to fsnp.h (which includes this header), same FSNP_ABI_VERSION.  The rules below, once more with the
 * kernels' side, are in DESIGN.md ("PCM I/O"); a PCM serving loop and the reference CLI's tail are in INTEGRATION.md.
 *
 * The entry points here are those of the waveform path (fsnp_stft, fsnp_enhance_wave, fsnp_enhance_wave_lengths of fsnp.h and
 * fsnp_lengths.h; fsnp_wave_stream_push, fsnp_wave_stream_finish of fsnp_wave_stream.h) with a sample format and a sample step on
 * every sample buffer.  The conversion happens in the loads and stores of the kernels that touch samples anyway, not in launches
 * around them; everything between them - transforms, model, overlap-add arithmetic, a wave session's records - is fp32 as before, so
 * the fp32 entry points and the ones here may be mixed freely on one handle or session, and the state of a session moves between them.
 *
 * Buffers.  A buffer is `const void*` / `void*` with its format next to it.  Strides and steps are in ELEMENTS of the buffer's own
 * type (float or int16_t): row b starts at element b * stride, consecutive samples of a row are `step` elements apart.  step = 1 is
 * planar audio, step = C takes one channel of C-channel interleaved audio in place (row stride 1, or whatever the layout has).  An
 * int16 buffer needs 2-byte alignment only; rows may start at odd element offsets and have odd strides.
 *
 * Formats.
 *   FSNP_SAMPLE_F32       fp32, as everywhere else in the library.
 *   FSNP_SAMPLE_S16       int16, full scale.
 *     in:   x = (float)s * (1.0f / 32768.0f), exact in fp32: an int16 input gives, bit for bit, what the fp32 call gives for
 *           s.float() / 32768.
 *     out:  q = rint(v * 32768.0f) (round half to even), saturated to [-32768, 32767]; +-inf saturates, NaN becomes 0.  A sample
 *           counts as CLIPPED when it saturated or was NaN (-1.0f gives -32768 and is not clipped).
 *   FSNP_SAMPLE_S16_PEAK  int16, peak-normalised; OUTPUT of whole-clip calls only.  The tail of the reference CLI
 *           (audio_zen/inferencer/base_inferencer.py:148-152, np.int16(0.8 * 32767 * enhanced / max|enhanced|)) in its own fp32
 *           arithmetic: peak = max |v| over the clip's own samples, q = trunc_toward_zero((26213.6f * v) / peak), where 26213.6f is
 *           the fp32 rounding of 0.8 * 32767, the product is rounded to fp32 and the division is the IEEE fp32 one.  (The library
 *           is compiled without fast-math and must stay so for this: a reciprocal multiply or a contracted product gives other
 *           bits.)  A clip whose peak is 0 comes out as all zeros, where numpy would produce NaN.  Nothing clips in this format; a
 *           NaN sample does not take part in the peak and comes out as 0.
 *
 * Clipped counts.  `clipped`: NULL, or DEVICE int32 [batch], overwritten by the call (stream-ordered) with the number of clipped
 * samples of each row; always 0 for the formats that cannot clip.  Session calls take no `clipped` argument: a live caller that
 * needs the count takes fp32 out.
 *
 * Like the fp32 calls, every call here is stream-ordered on hip_stream, allocates nothing once the handle's areas have their size
 * (fsnp_reserve) and synchronises neither host nor device; FSNP_SAMPLE_S16_PEAK runs its reduction and a second pass on the device.
 *
 * Refusals, before anything is enqueued and with the reason in fsnp_last_error: code 1 for a NULL handle, session or buffer;
 * code 2 for an unknown format, FSNP_SAMPLE_S16_PEAK as an input format or in a session call (a stream has no peak), a step below
 * 1, and everything the fp32 call of the same name refuses.
 */
#ifndef FSNP_PCM_H
#define FSNP_PCM_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

#define FSNP_SAMPLE_F32 0
#define FSNP_SAMPLE_S16 1
#define FSNP_SAMPLE_S16_PEAK 2

/* fsnp_enhance_wave (samples = NULL: every row holds max_samples samples) or fsnp_enhance_wave_lengths (samples: HOST int32 [batch],
 * read during the call) with formatted buffers: sample j of row b at wav[b * wav_stride + j * wav_step] and
 * out[b * out_stride + j * out_step].  Samples past a row's length come out as exactly 0 in every format and are never read. */
int fsnp_enhance_wave_pcm(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                          int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch,
                          int32_t max_samples, int32_t* clipped, void* hip_stream);
/* fsnp_stft of an int16 or strided input: the same spectrum out ([batch][T][num_freqs] complex64, interleaved). */
int fsnp_stft_pcm(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, float* spec, int32_t batch,
                  int32_t samples, void* hip_stream);

/* fsnp_wave_stream_push / fsnp_wave_stream_finish (fsnp_wave_stream.h) with formatted buffers, on any wave session, default or
 * live, freely mixed with the fp32 calls: the session's records stay fp32 and fsnp_wave_stream_state_bytes does not change.
 * in_format: FSNP_SAMPLE_F32 or FSNP_SAMPLE_S16; out_format: the same two (FSNP_SAMPLE_S16_PEAK: code 2).  No `clipped`. */
int fsnp_wave_stream_push_pcm(fsnp_wave_stream* ws, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step,
                              const int32_t* counts, void* out, int32_t out_format, int64_t out_stride, int64_t out_step, int32_t n,
                              void* hip_stream);
int fsnp_wave_stream_finish_pcm(fsnp_wave_stream* ws, const int32_t* slots, int32_t num, void* out, int32_t out_format,
                                int64_t out_stride, int64_t out_step, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_PCM_H */
