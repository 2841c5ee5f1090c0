/*
 * fsnp_spec_stream.h - spectrum sessions of the original FullSubNet: noisy STFT frames in, enhanced STFT frames out.  Part of the
 * public surface of libfsnp_hip.so next to fsnp.h (which includes this header), same FSNP_ABI_VERSION.  The layer between a mag
 * session (fsnp_stream.h: magnitudes in, cIRM masks out) and a wave session (fsnp_wave_stream.h: samples in, samples out), for a
 * caller who owns the STFT - any window, any overlap, shared with an echo canceller or a beamformer.  DESIGN.md ("Streaming", 8b)
 * has the kernels; a serving loop is in INTEGRATION.md (2c).
 *
 * A spectrum session is made from a committed handle that a stream session accepts (every refusal of fsnp_stream.h applies, with
 * the same messages) and that has output_size = 2, and owns `slots` independent streams.  For a slot that has received P frames
 * since its last reset, a push of c frames (0 <= c <= n <= max_chunk) reads c noisy complex64 frames and writes n complex64
 * columns, with la = look_ahead:
 *   column j < c is the enhanced frame P + j - la: the cIRM of model step P + j, decompressed (K = 10, limit 9.9) and
 *     complex-multiplied with the noisy frame P + j - la - the arithmetic of fsnp_apply_cirm.  The noisy frame waits for its mask
 *     inside the slot's state; where P + j < la the column is exactly 0 + 0i;
 *   columns c .. n-1 are exactly 0 and the input is never read there (it may hold anything, NaN included);
 *   c = 0 leaves the slot's state untouched, bit for bit.
 * The magnitude the model sees is hypotf(re, im), as fsnp_forward_complex takes it; from there on the push IS the mag push of
 * fsnp_stream.h.  So a clip of T frames pushed in any chunking, followed by la all-zero frames, gives [la zero columns | the
 * T enhanced frames of fsnp_forward_complex + fsnp_apply_cirm of that clip alone in FULL mode].
 *
 * Pushes are stream-ordered: nothing is allocated and neither host nor device is synchronised.  Errors, fsnp_poll_errors /
 * fsnp_check_errors and fsnp_watch_weights behave as for fsnp_stream_push.  A session must be destroyed before its handle.
 */
#ifndef FSNP_SPEC_STREAM_H
#define FSNP_SPEC_STREAM_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fsnp_spec_stream fsnp_spec_stream;

/* Allocates the state of `slots` streams (all reset) and the workspace of a push of up to max_chunk frames per slot.  Codes and
 * messages of fsnp_stream_create; code 2 in addition for output_size != 2. */
int fsnp_spec_stream_create(fsnp_handle* h, int32_t slots, int32_t max_chunk, fsnp_spec_stream** out);
/* The same with a live session inside (fsnp_stream_live.h: per-step kernels for a few streams fed one hop at a time).  Code 2 in
 * addition for max_chunk > 16, as fsnp_stream_create_live.  Every other function of this header works on both. */
int fsnp_spec_stream_create_live(fsnp_handle* h, int32_t slots, int32_t max_chunk, fsnp_spec_stream** out);
void fsnp_spec_stream_destroy(fsnp_spec_stream* ss);
/* One push.  spec and out: device, interleaved (re, im) float pairs; element (slot, f, j) at complex index
 * slot * strides[0] + f * strides[1] + j * strides[2] (strides in complex elements, as fsnp_forward_complex takes them: torch.stft's
 * [slots, F, n] view of a [slots][n][F] buffer works for both without a copy).  out must not overlap spec.  counts: HOST int32
 * [slots] (read during the call only) or NULL = n frames for every slot; 1 <= n <= max_chunk.  Code 2, before anything is enqueued
 * and naming the slot, for a count outside [0, n]. */
int fsnp_spec_stream_push(fsnp_spec_stream* ss, const float* spec, const int64_t strides[3], const int32_t* counts, float* out,
                          const int64_t out_strides[3], int32_t n, void* hip_stream);
/* Stream-ordered zeroing of the state of slots[0 .. num) (HOST int32 indices; NULL = every slot). */
int fsnp_spec_stream_reset(fsnp_spec_stream* ss, const int32_t* slots, int32_t num, void* hip_stream);
/* Bytes of one slot's state: the record of fsnp_stream_state_bytes, then the noisy spectra of the newest look_ahead frames as
 * complex64 [look_ahead][F] (frame g in row g % look_ahead; empty for look_ahead = 0), padded to 16 bytes.  The layout does not
 * depend on the kernels, on the session's mode or on `slots`. */
int64_t fsnp_spec_stream_state_bytes(const fsnp_spec_stream* ss);
/* Stream-ordered copy of one slot's state to / from DEVICE memory of fsnp_spec_stream_state_bytes bytes (any spectrum session,
 * default or live, of a handle of the same sizes may load it).  Neither waits: the ring's position follows from the frame count
 * inside the record. */
int fsnp_spec_stream_get_state(fsnp_spec_stream* ss, int32_t slot, void* dev_dst, void* hip_stream);
int fsnp_spec_stream_set_state(fsnp_spec_stream* ss, int32_t slot, const void* dev_src, void* hip_stream);
/* Frames pushed into `slot` since its last reset, as fsnp_stream_frames counts them. */
int fsnp_spec_stream_frames(fsnp_spec_stream* ss, int32_t slot, int64_t* pushed);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_SPEC_STREAM_H */
