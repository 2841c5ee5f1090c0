/*
 * fsnp_device_weights.h - handing the weights over in DEVICE memory and packing them on the GPU.  Part of the public surface of
 * libfsnp_hip.so next to fsnp.h (which includes this header), same FSNP_ABI_VERSION.  DESIGN.md ("Device-side weight hand-over")
 * has the arena, the kernels and the ordering; the table of INTEGRATION.md section 2 has the row of the two calls.
 *
 * A caller whose parameters already live on the GPU (PyTorch after `.to(device)`) need not bring them to the host first:
 * fsnp_set_weight_device takes a device pointer, fsnp_commit_weights_on builds the packed blob with kernels.  The blob is
 * byte for byte what fsnp_set_weight + fsnp_commit_weights build from the same values, so every result is bit-identical.
 */
#ifndef FSNP_DEVICE_WEIGHTS_H
#define FSNP_DEVICE_WEIGHTS_H

#include "fsnp.h"

#ifdef __cplusplus
extern "C" {
#endif

/* fsnp_set_weight for a tensor in DEVICE memory (contiguous fp32 on the handle's device, the reference's name and shape): the same
 * name and size checks with the same codes and messages (code 1: null argument, nothing is touched).  The tensor is copied device
 * to device on `hip_stream` into an arena the handle owns (one allocation for all parameters, made by the first call), so the
 * caller may change or free it afterwards in stream order.  Does not wait for the device.  Marks the handle uncommitted and drops
 * the weight watch, as fsnp_set_weight does.  Host-given and device-given tensors may be mixed freely; per tensor the last call
 * counts. */
int fsnp_set_weight_device(fsnp_handle* h, const char* name, const float* dev_data, int64_t numel, void* hip_stream);

/* fsnp_commit_weights on a stream.  When every tensor of the parameter tree was last given through fsnp_set_weight_device, the blob
 * is packed on the device: one kernel per weight image on `hip_stream`, nothing is copied to the host, and a re-commit packs into
 * the existing allocation (no hipFree / hipMalloc; the pointers the kernels hold stay valid).  The pack is ordered behind the
 * handle's earlier forwards (whatever their stream) and deferred chunks; a RE-commit still waits for the device before it
 * overwrites the blob (DESIGN.md says why), the first commit waits for nothing.  Otherwise - some tensors host-given - the
 * device-given ones are copied down and the host path of fsnp_commit_weights runs: always correct, no faster than before.  A
 * missing tensor is the error of fsnp_commit_weights.
 *
 * The call returns with the pack ENQUEUED, not finished.  Work on `hip_stream` itself is behind it by stream order.  On any other
 * stream these calls wait for it on the device (an event, no host wait) before they read the blob:
 *   fsnp_forward, fsnp_forward_complex, fsnp_forward_lengths, fsnp_forward_complex_lengths, fsnp_enhance_wave,
 *   fsnp_enhance_wave_lengths, fsnp_lstm2_fc, fsnp_channel_attention, fsnp_fullband_model, fsnp_reserve,
 *   and every push of a stream, wave or spectrum session (fsnp_stream_push, fsnp_wave_stream_push / _finish,
 *   fsnp_spec_stream_push);
 * a later fsnp_set_weight_device waits for it before it overwrites the arena, and fsnp_watch_weights and the profiling /
 * calibration hooks of fsnp_debug.h synchronise the device.  No other entry point reads the blob.
 *
 * fsnp_commit_weights itself keeps its behaviour; with device-given tensors it copies them down first and packs on the host. */
int fsnp_commit_weights_on(fsnp_handle* h, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* FSNP_DEVICE_WEIGHTS_H */
