/*
 * fsnp_stream_live.h - live stream sessions: the session mode for a FEW streams fed one hop at a time.  Part of the public surface
 * of libfsnp_hip.so next to fsnp.h (which includes this header), same FSNP_ABI_VERSION.  DESIGN.md ("Streaming", 8b) has the
 * kernels and the measured crossover between the two modes.
 *
 * A default session (fsnp_stream_create, fsnp_wave_stream_create) runs the two recurrent models of a push as one launch each that
 * stays resident over the push's frames: right for long chunks and many slots, wasteful for one frame of one call (one row tile
 * per CU, one workgroup for the full-band model).  A live session runs them as one short launch per layer and time step, each cut
 * by columns over the whole chip, with stream order as the only synchronisation.  It ALWAYS takes that path, whatever the number
 * of active slots or n, so a slot's output bits do not depend on its neighbours.
 *
 * Everything else is the session of fsnp_stream.h / fsnp_wave_stream.h: every other function of those headers works on the
 * sessions returned here, the state record and fsnp_stream_state_bytes are the same, and a record saved from a session of one
 * mode loads into a session of the other.  The two modes agree within the model's tolerance, not bit for bit.  Same checks, same
 * error codes, same fsnp_watch_weights / fsnp_poll_errors behaviour; a push allocates nothing and synchronises nothing.
 */
#ifndef FSNP_STREAM_LIVE_H
#define FSNP_STREAM_LIVE_H

#include "fsnp_stream.h"
#include "fsnp_wave_stream.h"

#ifdef __cplusplus
extern "C" {
#endif

/* As fsnp_stream_create.  Code 2 in addition for max_chunk > 16: a live push costs a handful of launches per frame by design;
 * longer chunks belong to a default session. */
int fsnp_stream_create_live(fsnp_handle* h, int32_t slots, int32_t max_chunk, fsnp_stream** out);
/* As fsnp_wave_stream_create, with a live session inside: max(max_samples / hop + 1, 1 + look_ahead) frames per push must be <= 16. */
int fsnp_wave_stream_create_live(fsnp_handle* h, int32_t slots, int32_t max_samples, fsnp_wave_stream** out);
/* 1 for a session made by fsnp_stream_create_live, else 0 (NULL included). */
int fsnp_stream_is_live(const fsnp_stream* st);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_STREAM_LIVE_H */
