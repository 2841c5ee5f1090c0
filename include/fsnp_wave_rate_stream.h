/*
 * fsnp_wave_rate_stream.h - wave sessions at any input sample rate: samples in at the caller's rate R, samples out at R, converted to
 * and from the model's rate M on the device, push by push.  Part of the public surface of libfsnp_hip.so next to fsnp.h (which includes
 * this header), same FSNP_ABI_VERSION.  The kernels' side is in DESIGN.md ("Sample rates", rate sessions), a 48 kHz live call in
 * INTEGRATION.md.
 *
 * A rate session is a wave session (fsnp_wave_stream.h) between two streaming converters, as a wave session is a spectrum session
 * between two transforms.  It holds an ordinary wave session - default or live - at rate M and drives it through the code of that
 * session's own push and finish; the converter is the one filter of fsnp_resample.h, and every output sample is that header's sum
 * (from 0.0f, ascending k, explicit fmaf, taps from the handle's table of the pair) over the same k range a whole-clip call has.
 *
 * Let (up, down, half) = fsnp_resample_plan(R, M); the way back is (down, up, half).  D_M = n_fft + look_ahead * hop is the inner
 * session's delay.  All arithmetic is 64-bit.
 *
 * Ready samples.  Model-rate sample j needs input samples up to floor((j * down + half) / up), so P input samples give
 *     ready(P) = P * up <= half ? 0 : (P * up - half - 1) / down + 1
 * model-rate samples whose whole window has arrived (fsnp_resample_ready); a clip of L samples has total(L) = ceil(L * up / down)
 * (fsnp_resample_length).
 *
 * Delay.  D_R = ceil((D_M * down + 2 * half + 1) / up) - 1 samples at rate R: the smallest delay at which every push can return as many
 * samples as it took.  At n_fft 512, hop 256, look_ahead 2 (D_M = 1024, 64 ms): 48 kHz 3264 samples (68.0 ms), 44.1 kHz 2998
 * (67.98 ms), 8 kHz 576 (72 ms).
 *
 * Push.  A push of c samples (0 <= c <= n <= max_samples) into a slot that holds P returns n columns: column j < c is enhanced sample
 * m = P + j - D_R at rate R, exactly 0 while m < 0; columns c .. n-1 are exactly 0 and the input there is never read; c = 0 leaves
 * the slot's record untouched, bit for bit.  Inside: (1) model-rate samples ready(P) .. ready(P + c) - 1 - at most
 * floor(c * up / down) + 1 - are summed from the carried input history and the new samples; (2) they go into the inner session as the
 * slot's count, which may be 0; (3) its output, the enhanced model-rate stream D_M late, joins the carried enhanced history; (4) the c
 * outputs are summed from it:  y[m] = sum over k >= 0 with |m * up - k * down| <= half of  t[m * up - k * down] * e[k].  Neither sum
 * has an upper clamp before finish: the samples it needs have arrived.
 *
 * Finish.  Refused (code 2, before anything is enqueued, naming the slot) if a listed slot holds L > 0 samples with
 * total(L) <= n_fft / 2 - the whole-clip refusal.  A slot that holds no samples gives a row of zeros.  Otherwise: (1) the remaining
 * total(L) - ready(L) <= ceil(half / down) model-rate samples (32 when decimating, 64 from 8 kHz to 16 kHz) are summed with the input
 * clamped at L - 1; (2) one inner push takes them; (3) the inner finish gives the last D_M model-rate samples; (4) samples
 * L - D_R .. L - 1 at rate R are summed with the enhanced clip clamped at total(L) - 1, exactly 0 where the index is negative;
 * (5) both records are reset.  The inner session is therefore created for max(floor(max_samples * up / down) + 1, ceil(half / down))
 * samples per call (fsnp_wave_rate_stream_model_max_samples).
 *
 * Result.  For any chunking, idle pushes included, all push outputs of a clip followed by its finish output are L + D_R samples; the
 * first D_R are exactly 0 and the rest is fsnp_enhance_wave_rate of that clip alone, within the tolerance of a wave session against
 * fsnp_enhance_wave.  Bit for bit it is this composition of public calls: x_M = fsnp_resample_pcm(clip, R -> M); a wave session of the
 * same kind, slot count and max_samples = model_max_samples pushed ready(P + c) - ready(P) samples of x_M wherever the rate session was
 * pushed c, then the remaining total(L) - ready(L), then finished; e = its outputs without the first D_M;
 * [D_R zeros | the first L samples of fsnp_resample_pcm(e, M -> R)].
 *
 * State.  A slot's record is the inner wave-session record (fsnp_wave_stream.h) followed by the rate record: fp32 input history
 * [floor(2 * half / up)] (the newest samples at rate R; int16 input is stored as the fp32 it converts to, exactly), fp32 enhanced
 * history [ceil(2 * half / down)] (the newest enhanced model-rate samples), int64 count of samples at rate R, int32 up, int32 down
 * (written by the first push that brings samples; padded to 16 bytes).  A record loads into any rate session of the same pair on a
 * handle of the same sizes and hop, default or live; a record that never took a sample is all zeros and loads into every pair.
 *
 * Pushes and finishes are stream-ordered like those of a wave session: nothing is allocated - the tap tables of both directions are
 * built and uploaded when the session is created - and neither host nor device is synchronised.  Errors, the weight watch and the
 * polling calls behave as for a push of fsnp_stream.h.  Buffers, formats, strides and steps are those of fsnp_pcm.h (FSNP_SAMPLE_F32,
 * FSNP_SAMPLE_S16; a stream has no peak).  A session must be destroyed before its handle.  Spectrum and stream sessions see no samples
 * and take no rate.
 */
#ifndef FSNP_WAVE_RATE_STREAM_H
#define FSNP_WAVE_RATE_STREAM_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct fsnp_wave_rate_stream fsnp_wave_rate_stream;

/* Host arithmetic only.  ready = the samples at to_rate whose whole filter window lies inside the first n >= 0 samples at from_rate. */
int fsnp_resample_ready(int32_t from_rate, int32_t to_rate, int64_t n, int64_t* ready);

/* `slots` streams of up to max_samples samples per push at sample_rate on a handle whose model runs at model_rate; _create_live: the
 * inner wave session is a live one (fsnp_stream_live.h).  Builds and uploads the tables of both directions and waits for them.
 * Code 1: null argument.  Code 2, with the reason: sample_rate == model_rate (open fsnp_wave_stream_create: there is nothing to
 * convert), everything fsnp_resample_plan refuses (a rate <= 0, max(up, down) > 640), a ninth table pair on the handle,
 * max_samples < 1 or a model-rate count that does not fit, and every refusal of the inner session, whose message is kept and which
 * names both max_samples and the model-rate samples per call it turned into (a live session runs at most 16 frames per call). */
int fsnp_wave_rate_stream_create(fsnp_handle* h, int32_t slots, int32_t max_samples, int32_t sample_rate, int32_t model_rate,
                                 fsnp_wave_rate_stream** out);
int fsnp_wave_rate_stream_create_live(fsnp_handle* h, int32_t slots, int32_t max_samples, int32_t sample_rate, int32_t model_rate,
                                      fsnp_wave_rate_stream** out);
void fsnp_wave_rate_stream_destroy(fsnp_wave_rate_stream* rs);
/* One push, as fsnp_wave_stream_push_pcm: sample j of slot b at wav[b * wav_stride + j * wav_step] and out[b * out_stride + j * out_step]
 * (elements of the buffer's own type), counts HOST int32 [slots] or NULL = n for every slot, all n columns of every row written;
 * 1 <= n <= max_samples.  The fp32 call is in_format = out_format = FSNP_SAMPLE_F32. */
int fsnp_wave_rate_stream_push_pcm(fsnp_wave_rate_stream* rs, const void* wav, int32_t in_format, int64_t wav_stride, int64_t wav_step,
                                   const int32_t* counts, void* out, int32_t out_format, int64_t out_stride, int64_t out_step, int32_t n,
                                   void* hip_stream);
/* Ends the clips of slots[0 .. num) (HOST int32 indices; NULL = every slot): out [slots][D_R]; rows of slots not listed, and of listed
 * slots that hold no samples, are exactly 0 and their state is untouched. */
int fsnp_wave_rate_stream_finish_pcm(fsnp_wave_rate_stream* rs, const int32_t* slots, int32_t num, void* out, int32_t out_format,
                                     int64_t out_stride, int64_t out_step, void* hip_stream);
/* Stream-ordered zeroing of both records of slots[0 .. num) (HOST int32 indices; NULL = every slot). */
int fsnp_wave_rate_stream_reset(fsnp_wave_rate_stream* rs, const int32_t* slots, int32_t num, void* hip_stream);
/* D_R in samples at sample_rate; the inner session's D_M at model_rate; its max_samples (0 for NULL). */
int fsnp_wave_rate_stream_delay(const fsnp_wave_rate_stream* rs);
int fsnp_wave_rate_stream_model_delay(const fsnp_wave_rate_stream* rs);
int fsnp_wave_rate_stream_model_max_samples(const fsnp_wave_rate_stream* rs);
/* Bytes of one slot's state (see State above), and its stream-ordered copy to / from DEVICE memory of that many bytes.  set_state is
 * a migration call and the only one here that waits: it synchronises hip_stream once, to read the loaded count and pair; code 2, with
 * nothing loaded, for a record of another pair or a negative count. */
int64_t fsnp_wave_rate_stream_state_bytes(const fsnp_wave_rate_stream* rs);
int fsnp_wave_rate_stream_get_state(fsnp_wave_rate_stream* rs, int32_t slot, void* dev_dst, void* hip_stream);
int fsnp_wave_rate_stream_set_state(fsnp_wave_rate_stream* rs, int32_t slot, const void* dev_src, void* hip_stream);
/* Samples at sample_rate pushed into `slot` since its last reset or finish (counted on the host, no synchronisation). */
int fsnp_wave_rate_stream_samples(fsnp_wave_rate_stream* rs, int32_t slot, int64_t* pushed);

#ifdef __cplusplus
}
#endif
#endif /* FSNP_WAVE_RATE_STREAM_H */
