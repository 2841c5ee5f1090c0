/*
 * fsnp_window_stream.h - window sessions: live audio through either model in the cross-faded windows of ext/fsnp_windowed.h, samples
 * in, samples out at a fixed delay of one window.  A session header of libfsnp_hip.so: it includes fsnp.h and ext/fsnp_windowed.h,
 * fsnp.h does not include it; same library, same FSNP_ABI_VERSION.  The contract below, with the kernels' side, the record and the
 * memory per slot, is DESIGN.md section 8g; a serving loop is in INTEGRATION.md ("Live audio through FullSubNet+").
 *
 * Why.  FullSubNet+ has no online form (offline norms, pooling, GroupNorm and non-causal convolutions over the whole clip), so the only
 * way it processes unbounded audio is the plan of ext/fsnp_windowed.h: window W, overlap V, stride S = W - V, fade g, the merge
 * formula and K windows for a clip of L samples, all as defined there.  A window session is that plan run block by block: it equals
 * fsnp_enhance_wave_windowed of the whole clip for any chunking, and it works for both models.
 *
 * A session is made from a committed handle and owns `slots` independent streams.  All counts are samples at the model's rate.  Its
 * delay is D = W.  Like a wave session it runs at the STFT geometry the handle has when it is created (fsnp_stft_geometry.h) and keeps
 * it: a later fsnp_set_hop_length does not touch the session, which then equals fsnp_enhance_wave_windowed at the hop of its creation.
 *
 * Push.  For a slot that has received P samples since its last reset or finish, a push of c samples (0 <= c <= n <= max_samples)
 * returns c samples: column j < c of the slot's output row is sample P + j - D of the merged result, exactly 0 while P + j < D.
 * Columns c .. n-1 are written as exactly 0 and the input is never read there.  c = 0 leaves the slot untouched, bit for bit.
 * Window k of a slot is complete when the slot holds k S + W samples, and the push that completes it runs it: padded from the slot's
 * input history, enhanced as a clip of its own, overlap-added into an fp32 row.  The windows that one push completes, across slots,
 * are listed slot by slot (a slot's windows in order; more than one per slot when n > S) and forwarded max_batch at a time; they all
 * have W samples, so every forward is the equal-length call.  A push that completes no window runs no model.
 *
 * Finish.  On a listed slot that holds L samples it returns exactly D samples - merged samples L - D .. L - 1, exactly 0 where the
 * index is negative - and leaves the slot reset.  It first runs the plan's last window if the pushes have not (the window of
 * L - (K - 1) S samples, or the whole clip when L <= W; nothing when L = k S + W).  The last windows of the listed slots go through
 * the model max_batch at a time; a forward whose windows differ in length is the fsnp_forward_complex_lengths call, as in the
 * whole-clip function, a forward of one window is always the equal-length call.
 *
 * So for any chunking, idle pushes included, all push outputs of a clip followed by its finish output are L + W samples, and dropping
 * the first W gives fsnp_enhance_wave_windowed(clip, W, V) of that clip alone.  With max_batch = 1 on both sides the two are the same
 * sequence of single-window forwards and the same fmaf: equal bit for bit, whatever the number of slots and the block sizes.
 *
 * A session never loses a stream's tail to a refusal: whatever can be refused is refused at creation (below).  What remains for finish
 * is a slot whose whole clip is shorter than the model accepts.
 *
 * Formats (fsnp_pcm.h).  Input FSNP_SAMPLE_F32 or FSNP_SAMPLE_S16 at any stride and step, read in place; output the same two
 * (FSNP_SAMPLE_S16_PEAK: code 2 - a live clip's peak is not known).  clipped: NULL, or DEVICE int32 [slots], overwritten by the call
 * with each row's clipped samples (0 for fp32 out).  A slot's record is fp32, so formats mix freely between pushes.
 *
 * Pushes and finishes are stream-ordered on hip_stream: nothing is allocated, neither host nor device is synchronised, and which
 * windows complete is decided from host-side counts.  Errors, the weight watch and the polling calls behave as for
 * fsnp_enhance_wave_windowed.  Code 1: a NULL session or buffer; code 2, before anything is enqueued, for the rest.  A session must be
 * destroyed before its handle.
 */
#ifndef FSNP_SESSION_WINDOW_STREAM_H
#define FSNP_SESSION_WINDOW_STREAM_H

#include "../fsnp.h"
#include "../ext/fsnp_windowed.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fsnp_window_stream fsnp_window_stream;

/* The session's scheduling rule.  Host arithmetic, no handle, no GPU: a push of `count` samples on a slot that held `pushed` completes
 * the windows [*first, *first + *num) of the plan (window k is complete at k S + window samples).  -1 for what needs no handle to
 * refuse: window < 2, overlap outside [1, window / 2], pushed < 0, count < 0, a NULL result. */
int fsnp_window_stream_plan(int64_t pushed, int64_t count, int32_t window, int32_t overlap, int64_t* first, int64_t* num);

/* Allocates the state of `slots` streams (all reset), the staging rows of the windows one call can complete
 * (slots * (1 + ceil(max_samples / S)) rows of W floats) and reserves the handle's io area for min(max_batch, that many) windows;
 * builds the handle's DFT matrices and the fade table of `overlap` if no call has yet.  max_samples: the largest block of one push;
 * max_batch: the most windows per forward.  Code 1: null argument.  Code 2, naming the function and the offending value: every
 * refusal of fsnp_enhance_wave_windowed (overlap outside [n_fft / 2, window / 2] at the handle's geometry, output_size != 2, weights
 * not committed, a ninth fade table); slots, max_samples or max_batch < 1; an overlap for which a last window of overlap + 1 samples
 * has fewer frames than the model's own minimum clip (TSSE: largest kernel - look_ahead frames; 8 frames, 1792 samples at the
 * default geometry); a model the lengths path refuses (subband_num > 1, sub-band sequence_model "TCN") unless max_batch = 1. */
int fsnp_window_stream_create(fsnp_handle* h, int32_t slots, int32_t window, int32_t overlap, int32_t max_samples, int32_t max_batch,
                              fsnp_window_stream** out);
void fsnp_window_stream_destroy(fsnp_window_stream* ws);
/* One push.  wav: device, sample j of slot b at wav[b * wav_stride + j * wav_step]; counts: HOST int32 [slots] (read during the call
 * only) or NULL = n samples for every slot; out: device, sample j of slot b at out[b * out_stride + j * out_step], all n columns of
 * every row are written; 1 <= n <= max_samples.  Code 2, naming the slot, for a count outside [0, n]. */
int fsnp_window_stream_push_pcm(fsnp_window_stream* ws, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step,
                                const int32_t* counts, void* out, int32_t out_format, int64_t out_stride, int64_t out_step, int32_t n,
                                int32_t* clipped, void* hip_stream);
/* Ends the clips of slots[0 .. num) (HOST int32 indices; NULL = every slot): out, device, [slots][D]; rows of slots not listed, and of
 * listed slots that hold no samples, are written as exactly 0 and their state is untouched.  Code 2, naming the slot and with every
 * slot's state untouched, for a listed slot whose whole clip the model does not accept: 1 .. n_fft / 2 samples, or L <= window with
 * fewer frames than the model's minimum clip. */
int fsnp_window_stream_finish_pcm(fsnp_window_stream* ws, const int32_t* slots, int32_t num, void* out, int32_t out_format,
                                  int64_t out_stride, int64_t out_step, int32_t* clipped, void* hip_stream);
/* Stream-ordered reset of slots[0 .. num) (HOST int32 indices; NULL = every slot): their next push starts a fresh clip. */
int fsnp_window_stream_reset(fsnp_window_stream* ws, const int32_t* slots, int32_t num, void* hip_stream);
/* D = window, in samples (0 for NULL). */
int fsnp_window_stream_delay(const fsnp_window_stream* ws);
/* Samples pushed into `slot` since its last reset or finish (counted on the host, no synchronisation). */
int fsnp_window_stream_samples(fsnp_window_stream* ws, int32_t slot, int64_t* pushed);
/* Bytes of one slot's state, 8 W + 8: fp32 input history [W] (the samples from the start of the slot's first incomplete window), the
 * newest window's un-faded tail [V], the merged samples not yet due [S] (oldest first), the int64 sample count.  Entries that hold
 * nothing are 0.  The layout depends on window and overlap only, not on slots, max_samples or max_batch. */
int64_t fsnp_window_stream_state_bytes(const fsnp_window_stream* ws);
/* Stream-ordered copy of one slot's state to / from DEVICE memory of that many bytes (any session of the same window and overlap may
 * load it).  set_state is a migration call and the only one here that waits: it synchronises hip_stream once to read the loaded
 * sample count into the session's host mirror. */
int fsnp_window_stream_get_state(fsnp_window_stream* ws, int32_t slot, void* dev_dst, void* hip_stream);
int fsnp_window_stream_set_state(fsnp_window_stream* ws, int32_t slot, const void* dev_src, void* hip_stream);

/* Test hook, like fsnp_debug_window_roundtrip: a session whose forwards are the device copy of every padded row's centre into its
 * staging row, so that only the schedule and the session's kernels run.  Needs no committed weights and skips the model's minimum
 * clip.  fmaf(g, a - a, a) = a: such a session returns its input delayed by W, bit for bit. */
int fsnp_debug_window_stream_create_copy(fsnp_handle* h, int32_t slots, int32_t window, int32_t overlap, int32_t max_samples,
                                         int32_t max_batch, fsnp_window_stream** out);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_SESSION_WINDOW_STREAM_H */
