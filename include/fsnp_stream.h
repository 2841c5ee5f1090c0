/*
 * fsnp_stream.h - streaming the original FullSubNet: chunked forwards that carry their state.  Part of the public surface of
 * libfsnp_hip.so next to fsnp.h (which includes this header), same FSNP_ABI_VERSION.  The contract, the state layout and the
 * kernels are in DESIGN.md ("Streaming"); a serving loop is in INTEGRATION.md.
 *
 * A stream session is made from a committed FullSubNet handle (FSNP_MODEL_FULLSUBNET, a cumulative norm, LSTM cells) and owns
 * `slots` independent live streams.  For a slot that has received P frames since its last reset, a push of c frames
 * (0 <= c <= n) runs steps P .. P+c-1 of exactly the recurrences and prefix sums the whole-clip forward runs, from the slot's
 * state.  Column j < c of the slot's output row is the model's output of step P + j, i.e. the cIRM of absolute frame
 * P + j - look_ahead (the reference pads look_ahead zero frames at the end and drops the first look_ahead outputs); where
 * P + j < look_ahead it is written as exactly 0.  Columns c .. n-1 are written as exactly 0 and the input is never read there
 * (it may hold anything, NaN included).  c = 0 leaves the slot's state untouched, bit for bit.  So a clip of T frames pushed in
 * any chunking, followed by look_ahead all-zero frames, gives - after dropping the first look_ahead columns - the [2, F, T]
 * mask of fsnp_forward of that clip alone in FULL mode.
 *
 * FullSubNet+ is refused: its full-band TCN blocks are not causal and normalise over the whole clip, TSSE pools over all of
 * time.  The offline norms need the clip's total, GRU cells and sub-band sizes outside the row-tile kernel are not built.
 *
 * Pushes are stream-ordered like forwards: nothing is allocated and neither host nor device is synchronised.  Errors,
 * fsnp_poll_errors / fsnp_check_errors and fsnp_watch_weights behave as for fsnp_forward.  Pipelining (fsnp_set_pipeline) and
 * the exchange verifications (fsnp_set_verify, fsnp_set_verify_sample) do not apply to pushes: a push runs no column-split
 * kernel and wholly on the caller's stream.  Several sessions may exist on one handle; pushes and forwards on one handle are
 * ordered by the caller's stream.  A session must be destroyed before its handle.
 */
#ifndef FSNP_STREAM_H
#define FSNP_STREAM_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fsnp_stream fsnp_stream;

/* Allocates the state of `slots` streams (all reset) and the workspace of a push of up to max_chunk frames per slot.
 * Code 1: null argument.  Code 2, with the reason: a handle the session does not cover (see above), weights not committed,
 * slots outside [1, 32 * (CUs / 16)] (the full-band model's limit of a whole-clip forward), max_chunk < 1. */
int fsnp_stream_create(fsnp_handle* h, int32_t slots, int32_t max_chunk, fsnp_stream** out);
void fsnp_stream_destroy(fsnp_stream* st);
/* One push.  mag: device, element (slot, f, j) at mag[slot * strides[0] + f * strides[1] + j * strides[2]]; counts: HOST int32
 * [slots] (read during the call only; they travel as kernel arguments) or NULL = n frames for every slot; out: device, contiguous
 * [slots, 2, F, n]; 1 <= n <= max_chunk.  Code 2, before anything is enqueued and naming the slot, for a count outside [0, n]. */
int fsnp_stream_push(fsnp_stream* st, const float* mag, const int64_t strides[3], const int32_t* counts, float* out, int32_t n,
                     void* hip_stream);
/* Stream-ordered zeroing of the state of slots[0 .. num) (HOST int32 indices; NULL = every slot). */
int fsnp_stream_reset(fsnp_stream* st, const int32_t* slots, int32_t num, void* hip_stream);
/* Bytes of one slot's state: fp32 sub-band [F][layer][h|c][H], fp32 full-band [layer][h|c][CH], fp64 sub-band norm sums [F][2],
 * fp64 full-band norm sums [2], int64 frame count.  The layout does not depend on the kernels or on `slots`. */
int64_t fsnp_stream_state_bytes(const fsnp_stream* st);
/* Stream-ordered copy of one slot's state to / from DEVICE memory of fsnp_stream_state_bytes bytes (any session of a handle of
 * the same sizes may load it). */
int fsnp_stream_get_state(fsnp_stream* st, int32_t slot, void* dev_dst, void* hip_stream);
int fsnp_stream_set_state(fsnp_stream* st, int32_t slot, const void* dev_src, void* hip_stream);
/* Frames pushed into `slot` since its last reset.  Counted on the host, no synchronisation - except after
 * fsnp_stream_set_state of that slot, whose count lives in the loaded state: the first call then waits for that copy. */
int fsnp_stream_frames(fsnp_stream* st, int32_t slot, int64_t* pushed);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_STREAM_H */
