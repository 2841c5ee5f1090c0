/*
 * fsnp_wave_stream.h - streaming waveforms through the original FullSubNet: samples in, samples out at a fixed delay.  Part of the
 * public surface of libfsnp_hip.so next to fsnp.h (which includes this header), same FSNP_ABI_VERSION.  The contract, the state
 * layout and the kernels are in DESIGN.md ("Streaming", waveform sessions); a serving loop is in INTEGRATION.md.
 *
 * A wave session is made from a committed FullSubNet handle that a stream session accepts (fsnp_stream.h: FSNP_MODEL_FULLSUBNET, a
 * cumulative norm, LSTM cells, sub-band sizes on the row-tile kernel) with output_size = 2, as the whole-clip waveform call demands,
 * and owns `slots` independent live audio streams.  It runs at the STFT geometry the handle has when the session is created
 * (fsnp_stft_geometry.h: n_fft = 2 (num_freqs - 1), hop = fsnp_hop_length(h), n_fft / 2 by default) and keeps it: a later
 * fsnp_set_hop_length does not touch the session.  Its delay is D = n_fft + look_ahead * hop samples ((2 + look_ahead) * hop at the
 * default hop).
 *
 * Push.  For a slot that has received P samples since its last reset or finish, a push of c samples (0 <= c <= n <= max_samples)
 * returns c samples: column j < c of the slot's output row is enhanced sample P + j - D of the clip, exactly 0.0f while P + j < D.
 * Columns c .. n-1 are written as exactly 0 and the input is never read there (it may hold anything, NaN included).  c = 0 leaves
 * the slot's state untouched, bit for bit.
 *
 * Finish.  On a slot that has received L samples it returns exactly D samples - enhanced samples L - D .. L - 1, exactly 0 where
 * the index is negative - and leaves the slot reset: it forms the clip's last STFT frames (those of the 1 + L / hop that L samples
 * did not complete: one at the default hop, up to ceil(n_fft / (2 hop)) in general) with the reflect padding at the end, steps the
 * model through the reference's look_ahead zero frames and overlap-adds the remainder.
 *
 * So for any chunking, idle pushes included, all push outputs of a clip followed by its finish output are L + D samples, and
 * dropping the first D gives the whole-clip waveform call of that clip alone (torch.stft -> model -> cIRM -> torch.istft(length=L)).
 *
 * Pushes and finishes are stream-ordered like forwards: nothing is allocated and neither host nor device is synchronised.  Errors,
 * the weight watch and the polling calls behave as for a push of fsnp_stream.h.  A session must be destroyed before its handle.
 */
#ifndef FSNP_WAVE_STREAM_H
#define FSNP_WAVE_STREAM_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fsnp_wave_stream fsnp_wave_stream;

/* Allocates the state of `slots` streams (all reset) and the workspace of a push of up to max_samples samples per slot; builds the
 * handle's DFT matrices if no waveform call has yet.  Code 1: null argument.  Code 2, with the reason: every refusal of a stream
 * session (fsnp_stream.h), output_size != 2, a hop length the rules of fsnp_stft_geometry.h refuse (only the default of a
 * num_freqs - 1 that is no multiple of 4 can get this far), num_freqs - 1 > 4096, max_samples < 1; for fsnp_wave_stream_create_live
 * also a finish that would need more than 16 frames in one call (ceil(n_fft / (2 hop)) + look_ahead). */
int fsnp_wave_stream_create(fsnp_handle* h, int32_t slots, int32_t max_samples, fsnp_wave_stream** out);
void fsnp_wave_stream_destroy(fsnp_wave_stream* ws);
/* One push.  wav: device, sample j of slot b at wav[b * wav_stride + j]; counts: HOST int32 [slots] (read during the call only) or
 * NULL = n samples for every slot; out: device, sample j of slot b at out[b * out_stride + j], all n columns of every row are
 * written; 1 <= n <= max_samples.  Code 2, before anything is enqueued and naming the slot, for a count outside [0, n]. */
int fsnp_wave_stream_push(fsnp_wave_stream* ws, const float* wav, int64_t wav_stride, const int32_t* counts, float* out,
                          int64_t out_stride, int32_t n, void* hip_stream);
/* Ends the clips of slots[0 .. num) (HOST int32 indices; NULL = every slot): out, device, [slots][D] with out_stride floats between
 * rows, gets each clip's last D samples; rows of slots not listed, and of listed slots that hold no samples, are written as exactly
 * 0 and their state is untouched.  Code 2, before anything is enqueued and naming the slot, for a slot that holds 1 .. n_fft / 2 samples
 * (the whole-clip call refuses such a clip too: reflect padding needs more than n_fft / 2 samples). */
int fsnp_wave_stream_finish(fsnp_wave_stream* ws, const int32_t* slots, int32_t num, float* out, int64_t out_stride, void* hip_stream);
/* Stream-ordered zeroing of the state of slots[0 .. num) (HOST int32 indices; NULL = every slot). */
int fsnp_wave_stream_reset(fsnp_wave_stream* ws, const int32_t* slots, int32_t num, void* hip_stream);
/* D = n_fft + look_ahead * hop, in samples (0 for NULL). */
int fsnp_wave_stream_delay(const fsnp_wave_stream* ws);
/* Bytes of one slot's state: the record of fsnp_stream.h followed by the wave record - fp32 input carry [n_fft + 1] (padded to 8
 * bytes), complex64 spectrum ring [look_ahead][F] (frame g in row g % look_ahead), fp32 partial overlap-add sums [n_fft - hop]
 * (of the samples behind the finished ones; at the default hop the second half of the newest enhanced frame), fp32 output FIFO
 * [hop], int64 sample count.  The layout does not depend on the kernels or on `slots`; its size does not depend on the hop, its
 * meaning does: load a state only into a session of the hop it was saved at. */
int64_t fsnp_wave_stream_state_bytes(const fsnp_wave_stream* ws);
/* Stream-ordered copy of one slot's state to / from DEVICE memory of that many bytes (any session of a handle of the same sizes may
 * load it).  set_state is a migration call and the only one here that waits: it synchronises hip_stream once to read the loaded
 * sample count into the session's host mirror. */
int fsnp_wave_stream_get_state(fsnp_wave_stream* ws, int32_t slot, void* dev_dst, void* hip_stream);
int fsnp_wave_stream_set_state(fsnp_wave_stream* ws, int32_t slot, const void* dev_src, void* hip_stream);
/* Samples pushed into `slot` since its last reset or finish (counted on the host, no synchronisation). */
int fsnp_wave_stream_samples(fsnp_wave_stream* ws, int32_t slot, int64_t* pushed);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_WAVE_STREAM_H */
