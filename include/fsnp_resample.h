/*
 * fsnp_resample.h - the whole-clip waveform path at any input sample rate: samples in at the caller's rate, samples out at the
 * caller's rate, converted to and from the model's rate on the device.  Part of the public surface of libfsnp_hip.so next to fsnp.h
 * (which includes this header), same FSNP_ABI_VERSION.  The kernels' side is in DESIGN.md ("Sample rates"), a 48 kHz serving call in
 * INTEGRATION.md.  Whole-clip calls here; wave sessions at another rate are fsnp_wave_rate_stream.h (this filter, push by push);
 * spectrum and stream sessions see no samples and take no rate.
 *
 * The converter is ONE filter, a rational polyphase FIR with zero phase.  For from_rate -> to_rate:
 *
 *   g = gcd(from_rate, to_rate);  up = to_rate / g;  down = from_rate / g;  M = max(up, down)
 *   Z = 32, rho = 0.91, beta = 8.6;  half = Z * M
 *   h[i] = (rho / M) * sinc(rho * i / M) * I0(beta * sqrt(1 - (i / half)^2)) / I0(beta),   -half <= i <= half,
 *          sinc(x) = sin(pi x) / (pi x), I0 the modified Bessel function of order 0
 *   n_out = ceil(n * up / down)                                                      (64-bit integer arithmetic)
 *   y[m] = sum over 0 <= k < n with |m * down - k * up| <= half of  t[m * down - k * up] * x[k],      t[i] = fp32(up * h[i])
 *
 * Samples outside [0, n) are zeros and are never read.  The taps are built on the host in double and rounded once to fp32
 * (fsnp_resample_taps returns them).  On the device one thread sums one output: from 0.0f, over ascending k, every step an explicit
 * fmaf(t, x, acc) - in one device function that the free-standing call and the fused calls share, so they agree bit for bit:
 * fsnp_enhance_wave_rate gives exactly fsnp_resample_pcm to the model's rate (fp32 out), fsnp_enhance_wave_pcm there, and
 * fsnp_resample_pcm of its fp32 result back, cut to the caller's samples.
 *
 * from_rate == to_rate is not a filter: fsnp_resample_pcm is then a format-converting copy, bit exact, and fsnp_enhance_wave_rate is
 * fsnp_enhance_wave_pcm.
 *
 * Tables.  A handle keeps the taps of every (up, down) pair it has run, at most 8; they are uploaded once, stream-ordered, from host
 * memory the handle owns, and never evicted (launches in flight may read them).  A call that needs a ninth pair is refused.
 *
 * Buffers, formats, strides, steps and `clipped` are those of fsnp_pcm.h, applied to the samples at the caller's rate.  Every call is
 * stream-ordered on hip_stream, allocates nothing once the handle's areas have their size (fsnp_reserve, fsnp_reserve_rate) and its
 * pairs their tables, and synchronises neither host nor device.
 *
 * Refusals, before anything is enqueued and with the reason in fsnp_last_error: code 1 for a NULL handle or buffer; code 2 for a
 * rate <= 0, max(up, down) > 640 (among 8 / 11.025 / 12 / 16 / 22.05 / 24 / 32 / 44.1 / 48 / 88.2 / 96 / 192 kHz every pair passes
 * except 11.025 kHz against 32, 96 and 192 kHz and 22.05 kHz against 192 kHz; each of them converts to and from 16 kHz;
 * 16000 <-> 44101 does not), a ninth pair on one handle, and everything fsnp_pcm.h refuses.
 */
#ifndef FSNP_RESAMPLE_H
#define FSNP_RESAMPLE_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Host arithmetic only.  up, down, half of a pair (any of the three pointers may be NULL). */
int fsnp_resample_plan(int32_t from_rate, int32_t to_rate, int32_t* up, int32_t* down, int32_t* half);
/* Host arithmetic only.  n_out = ceil(n * up / down) for n >= 0. */
int fsnp_resample_length(int32_t from_rate, int32_t to_rate, int64_t n, int64_t* n_out);
/* Host.  taps[i + half] = t[i] for -half <= i <= half: 2 half + 1 values; capacity (in floats) below that: code 2. */
int fsnp_resample_taps(int32_t from_rate, int32_t to_rate, float* taps, int32_t capacity);

/* in [batch][max_samples] at from_rate -> out [batch][ceil(max_samples * up / down)] at to_rate: sample j of row b at
 * in[b * in_stride + j * in_step] and out[b * out_stride + j * out_step].  samples: NULL (every row holds max_samples samples), or
 * HOST int32 [batch] in [0, max_samples], read during the call: row b is then that clip converted alone, exactly 0 from its
 * ceil(samples[b] * up / down) on, and its input past samples[b] is never read.  in_format: FSNP_SAMPLE_F32 / FSNP_SAMPLE_S16;
 * out_format: those, or FSNP_SAMPLE_S16_PEAK (peak over each row's own output samples). */
int fsnp_resample_pcm(fsnp_handle* h, const void* in, int32_t in_format, int64_t in_stride, int64_t in_step, void* out,
                      int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch, int32_t max_samples,
                      int32_t from_rate, int32_t to_rate, int32_t* clipped, void* hip_stream);

/* fsnp_enhance_wave_pcm of clips that arrive, and leave, at sample_rate on a model that runs at model_rate: wav and out hold
 * max_samples samples per row at sample_rate.  The input conversion is part of the loads of the kernel that pads the clip for the
 * STFT (no model-rate copy of the clip is written); the model-rate result is converted back into the caller's first max_samples
 * (samples[b]) samples.  With `samples`, row b is that clip run alone: n16_b = ceil(samples[b] * up / down) model-rate samples and
 * 1 + n16_b / hop_length frames - literally: the rows run one after the other as calls of batch 1, so each has, bit for bit, what
 * its clip gives converted, enhanced and converted back on its own (the model's kernels are chosen by the batch size, and one batch
 * over all rows would differ from that in the last bits).  That costs the batch's throughput: clips padded to one length, without
 * `samples`, run as one batch.  Refuses (code 2) a clip whose model-rate length is not above n_fft / 2.
 * sample_rate == model_rate forwards to fsnp_enhance_wave_pcm unchanged. */
int fsnp_enhance_wave_rate(fsnp_handle* h, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step, void* out,
                           int32_t out_format, int64_t out_stride, int64_t out_step, const int32_t* samples, int32_t batch,
                           int32_t max_samples, int32_t* clipped, int32_t sample_rate, int32_t model_rate, void* hip_stream);

/* The part of fsnp_reserve that max_samples sizes, for fsnp_enhance_wave_rate calls of <= max_batch clips of <= max_samples samples
 * at sample_rate (the staging of FSNP_SAMPLE_S16_PEAK at the caller's rate included), and the tables of both directions. */
int fsnp_reserve_rate(fsnp_handle* h, int32_t max_batch, int32_t max_samples, int32_t sample_rate, int32_t model_rate, void* hip_stream);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_RESAMPLE_H */
