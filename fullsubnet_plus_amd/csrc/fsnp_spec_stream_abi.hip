// fsnp_spec_stream_abi.hip - include/fsnp_spec_stream.h: spectrum sessions of the original FullSubNet (STFT frames in, enhanced frames out).
//
// A session is a mag-stream session (fsnp_stream_abi.hip; a live one for fsnp_spec_stream_create_live) of max_chunk frames per push
// with, per slot, a ring of waiting noisy spectra behind the mag-stream record (layout: fsnp_common.h, SpecArgs) and a workspace of
// its own (the magnitudes and the mask of one push: the mask never leaves the device), allocated and zeroed at creation.  A push is its
// checks and spec_push_body (fsnp_stream_abi.hip) on the caller's tensors; a wave session (fsnp_wave_stream_abi.hip) calls the same body on its workspace
// rows, between its two DFT GEMMs, with the ring inside its wave record.  On the caller's stream, nothing allocated, nothing
// synchronised:
//   spec_mag_kernel     |X| of the new spectra of every slot from the strided complex input, in the mag push's own input layout
//   stream_push_body    the mag push (its epilogue zeroes the mask columns that hold no step)
//   spec_apply_kernel   cIRM of step P + j times the noisy frame P + j - look_ahead (this push's or the ring's), the exact zeros, ring advanced
// The ring's position is the mag record's frame count on the device (StreamMeta.p), so set_state waits for nothing.
#include <algorithm>

#include "fsnp_handle.h"

struct fsnp_spec_stream {
    fsnp_handle* h = nullptr;
    fsnp_stream* mag = nullptr;       // the model's state and its push
    int S = 0, N = 0, LA = 0;
    size_t mag_bytes = 0;             // one slot's mag-stream record
    SlotRecords ring;                 // the slots' rings behind it (0 bytes for look_ahead = 0)
    unsigned char* ws = nullptr;
    size_t ws_bytes = 0;
    size_t w_mag = 0, w_mask = 0;
};

namespace {

// fsnp_spec_stream_create (live = 0) / fsnp_spec_stream_create_live (live = 1: the mag session inside is a live one)
int spec_create(fsnp_handle* h, int32_t slots, int32_t max_chunk, int live, const char* where, fsnp_spec_stream** out) {
    if (!h || !out) { set_error("%s: null argument", where); return 1; }
    *out = nullptr;
    if (h->cfg.output_size != 2) { set_error("%s: the cIRM epilogue needs output_size = 2 (this handle: %d)", where, h->cfg.output_size); return 2; }
    fsnp_stream* mag = nullptr;
    // every refusal of a mag session, with its reason (live: max_chunk <= 16)
    if (const int rc = stream_create(h, slots, max_chunk, live, where, &mag)) return rc;
    fsnp_spec_stream* ss = new fsnp_spec_stream();
    ss->h = h; ss->mag = mag; ss->S = slots; ss->N = max_chunk; ss->LA = h->cfg.look_ahead;
    ss->mag_bytes = (size_t)fsnp_stream_state_bytes(mag);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    const size_t rows = (size_t)slots * max_chunk;
    ss->w_mag = take(rows * h->FP * 4);
    ss->w_mask = take(rows * 2 * h->F * 4);
    ss->ws_bytes = o;
    fsnp::DeviceGuard g(h->device);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&ss->ws), ss->ws_bytes);
    if (e == hipSuccess) e = hipMemset(ss->ws, 0, ss->ws_bytes);
    if (e == hipSuccess) e = ss->ring.create(align_up((size_t)ss->LA * h->F * 8, 16), slots);
    if (e != hipSuccess) {
        set_error("%s: %s (ring %zu bytes x %d slots, workspace %zu bytes)", where, hipGetErrorString(e), ss->ring.bytes, slots, ss->ws_bytes);
        ss->ring.free();
        if (ss->ws) (void)hipFree(ss->ws);
        fsnp_stream_destroy(mag);
        delete ss;
        return 4;
    }
    *out = ss;
    return 0;
}

}  // namespace

extern "C" {

int fsnp_spec_stream_create(fsnp_handle* h, int32_t slots, int32_t max_chunk, fsnp_spec_stream** out) {
    return spec_create(h, slots, max_chunk, 0, "fsnp_spec_stream_create", out);
}

int fsnp_spec_stream_create_live(fsnp_handle* h, int32_t slots, int32_t max_chunk, fsnp_spec_stream** out) {
    return spec_create(h, slots, max_chunk, 1, "fsnp_spec_stream_create_live", out);
}

void fsnp_spec_stream_destroy(fsnp_spec_stream* ss) {
    if (!ss) return;
    {
        fsnp::DeviceGuard g(ss->h->device);
        ss->ring.free();
        if (ss->ws) (void)hipFree(ss->ws);
    }
    fsnp_stream_destroy(ss->mag);
    delete ss;
}

int fsnp_spec_stream_push(fsnp_spec_stream* ss, const float* spec, const int64_t strides[3], const int32_t* counts, float* out,
                          const int64_t out_strides[3], int32_t n, void* hip_stream) {
    if (!ss || !spec || !strides || !out || !out_strides) { set_error("fsnp_spec_stream_push: null argument"); return 1; }
    if (n < 1 || n > ss->N) { set_error("fsnp_spec_stream_push: n = %d outside [1, max_chunk = %d]", n, ss->N); return 2; }
    SlotCounts c{};
    if (const int rc = read_counts("fsnp_spec_stream_push", counts, ss->S, n, c)) return rc;
    if (const int rc = push_preamble(ss->h, "fsnp_spec_stream_push")) return rc;
    return spec_push_body(ss->mag, SpecRing{ss->ring.base, ss->ring.bytes, ss->LA}, reinterpret_cast<float*>(ss->ws + ss->w_mag),
                          reinterpret_cast<float*>(ss->ws + ss->w_mask), spec, strides, c, c, out, out_strides, true, n,
                          static_cast<hipStream_t>(hip_stream));
}

int fsnp_spec_stream_reset(fsnp_spec_stream* ss, const int32_t* slots, int32_t num, void* hip_stream) {
    if (!ss) { set_error("fsnp_spec_stream_reset: null argument"); return 1; }
    if (const int rc = check_slots("fsnp_spec_stream_reset", slots, num, ss->S)) return rc;
    if (const int rc = fsnp_stream_reset(ss->mag, slots, num, hip_stream)) return rc;
    FSNP_ON_DEVICE(ss->h);
    return ss->ring.reset(slots, num, static_cast<hipStream_t>(hip_stream));
}

int64_t fsnp_spec_stream_state_bytes(const fsnp_spec_stream* ss) { return ss ? (int64_t)(ss->mag_bytes + ss->ring.bytes) : 0; }

int fsnp_spec_stream_get_state(fsnp_spec_stream* ss, int32_t slot, void* dev_dst, void* hip_stream) {
    if (!ss || !dev_dst) { set_error("fsnp_spec_stream_get_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_spec_stream_get_state", slot, ss->S)) return rc;
    if (const int rc = fsnp_stream_get_state(ss->mag, slot, dev_dst, hip_stream)) return rc;
    FSNP_ON_DEVICE(ss->h);
    return ss->ring.get(slot, dev_dst, ss->mag_bytes, static_cast<hipStream_t>(hip_stream));
}

int fsnp_spec_stream_set_state(fsnp_spec_stream* ss, int32_t slot, const void* dev_src, void* hip_stream) {
    if (!ss || !dev_src) { set_error("fsnp_spec_stream_set_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_spec_stream_set_state", slot, ss->S)) return rc;
    if (const int rc = fsnp_stream_set_state(ss->mag, slot, dev_src, hip_stream)) return rc;
    FSNP_ON_DEVICE(ss->h);
    return ss->ring.set(slot, dev_src, ss->mag_bytes, static_cast<hipStream_t>(hip_stream));
}

int fsnp_spec_stream_frames(fsnp_spec_stream* ss, int32_t slot, int64_t* pushed) {
    if (!ss || !pushed) { set_error("fsnp_spec_stream_frames: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_spec_stream_frames", slot, ss->S)) return rc;
    return fsnp_stream_frames(ss->mag, slot, pushed);
}

}  // extern "C"
