// fsnp_spec_stream_abi.hip - include/fsnp_spec_stream.h: spectrum sessions of the original FullSubNet (STFT frames in, enhanced frames out).
//
// A session is a mag-stream session (fsnp_stream_abi.hip; a live one for fsnp_spec_stream_create_live) of max_chunk frames per push
// with, per slot, a ring of waiting noisy spectra behind the mag-stream record (layout: fsnp_common.h, SpecArgs) and a workspace of
// its own (the magnitudes and the mask of one push: the mask never leaves the device), allocated and zeroed at creation.  One push on
// the caller's stream, nothing allocated, nothing synchronised:
//   spec_mag_kernel     |X| of the new frames of every slot from the strided complex input, in the mag push's own input layout
//   stream_push_body    the mag push (its epilogue zeroes the mask columns that hold no step)
//   spec_apply_kernel   cIRM of step P + j times the noisy frame P + j - look_ahead (this push's or the ring's), the exact zeros, ring advanced
// The ring's position is the mag record's frame count on the device (StreamMeta.p), so set_state waits for nothing.
#include <algorithm>

#include "fsnp_handle.h"

static_assert(sizeof(SpecCounts) == sizeof(StreamCounts), "one count per slot of a mag session");

struct fsnp_spec_stream {
    fsnp_handle* h = nullptr;
    fsnp_stream* mag = nullptr;       // the model's state and its push
    int S = 0, N = 0, LA = 0;
    size_t mag_bytes = 0, ring_bytes = 0;      // one slot: mag-stream record, ring (0 for look_ahead = 0)
    unsigned char* ring = nullptr;    // [S][ring_bytes]
    unsigned char* ws = nullptr;
    size_t ws_bytes = 0;
    size_t w_mag = 0, w_mask = 0;
    const StreamMeta* meta = nullptr; // the mag session's per-slot push facts (its workspace)
};

namespace {

int check_slots(const fsnp_spec_stream* ss, const int32_t* slots, int32_t num, const char* where) {
    if (!slots) return 0;
    if (num < 0) { set_error("%s: num = %d", where, num); return 2; }
    for (int i = 0; i < num; ++i)
        if (slots[i] < 0 || slots[i] >= ss->S) { set_error("%s: slot %d outside [0, %d)", where, slots[i], ss->S); return 2; }
    return 0;
}

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
    ss->ring_bytes = align_up((size_t)ss->LA * h->F * 8, 16);
    ss->meta = stream_meta(mag);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    const size_t rows = (size_t)slots * max_chunk;
    ss->w_mag = take(rows * h->FP * 4);
    ss->w_mask = take(rows * 2 * h->F * 4);
    ss->ws_bytes = o;
    fsnp::DeviceGuard g(h->device);
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&ss->ws), ss->ws_bytes);
    if (e == hipSuccess) e = hipMemset(ss->ws, 0, ss->ws_bytes);
    if (e == hipSuccess && ss->ring_bytes) e = hipMalloc(reinterpret_cast<void**>(&ss->ring), ss->ring_bytes * slots);
    if (e == hipSuccess && ss->ring_bytes) e = hipMemset(ss->ring, 0, ss->ring_bytes * slots);
    if (e != hipSuccess) {
        set_error("%s: %s (ring %zu bytes x %d slots, workspace %zu bytes)", where, hipGetErrorString(e), ss->ring_bytes, slots, ss->ws_bytes);
        if (ss->ring) (void)hipFree(ss->ring);
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
        // (hipFree waits for the device: pushes still in flight finish first)
        if (ss->ring) (void)hipFree(ss->ring);
        if (ss->ws) (void)hipFree(ss->ws);
    }
    fsnp_stream_destroy(ss->mag);
    delete ss;
}

int fsnp_spec_stream_push(fsnp_spec_stream* ss, const float* spec, const int64_t strides[3], const int32_t* counts, float* out,
                          const int64_t out_strides[3], int32_t n, void* hip_stream) {
    if (!ss || !spec || !strides || !out || !out_strides) { set_error("fsnp_spec_stream_push: null argument"); return 1; }
    fsnp_handle* h = ss->h;
    if (n < 1 || n > ss->N) { set_error("fsnp_spec_stream_push: n = %d outside [1, max_chunk = %d]", n, ss->N); return 2; }
    StreamCounts c{};
    SpecCounts sc{};
    int frames = 0;
    for (int b = 0; b < ss->S; ++b) {
        const int v = counts ? counts[b] : n;
        if (v < 0 || v > n) { set_error("fsnp_spec_stream_push: slot %d: count %d outside [0, n = %d]", b, v, n); return 2; }
        c.v[b] = v; sc.v[b] = v;
        frames += v;
    }
    if (!h->committed) { set_error("fsnp_spec_stream_push: weights not committed (call fsnp_commit_weights)"); return 2; }
    if (const int ec = take_device_errors(h, "an earlier call on this handle failed")) return ec;
    FSNP_ON_DEVICE(h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    float* mag = reinterpret_cast<float*>(ss->ws + ss->w_mag);
    float* mask = reinterpret_cast<float*>(ss->ws + ss->w_mask);
    SpecArgs a{};
    a.ring = ss->ring; a.ring_stride = ss->ring_bytes; a.meta = ss->meta;
    a.S = ss->S; a.F = h->F; a.FP = h->FP; a.LA = ss->LA; a.n = n;
    if (frames > 0) launch_spec_mag(a, sc, spec, strides, mag, s);
    const int64_t mst[3] = {(int64_t)n * h->FP, 1, h->FP};             // mag [S][n][FP] as (slot, f, frame)
    if (const int rc = stream_push_body(ss->mag, mag, mst, c, mask, n, s)) return rc;
    launch_spec_apply(a, mask, spec, strides, out, out_strides, s);
    FSNP_HIP_CHECK(hipGetLastError());
    return 0;
}

int fsnp_spec_stream_reset(fsnp_spec_stream* ss, const int32_t* slots, int32_t num, void* hip_stream) {
    if (!ss) { set_error("fsnp_spec_stream_reset: null argument"); return 1; }
    if (const int rc = check_slots(ss, slots, num, "fsnp_spec_stream_reset")) return rc;
    if (const int rc = fsnp_stream_reset(ss->mag, slots, num, hip_stream)) return rc;
    if (!ss->ring_bytes) return 0;
    FSNP_ON_DEVICE(ss->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (!slots) {
        FSNP_HIP_CHECK(hipMemsetAsync(ss->ring, 0, ss->ring_bytes * ss->S, s));
        return 0;
    }
    for (int i = 0; i < num; ++i) FSNP_HIP_CHECK(hipMemsetAsync(ss->ring + (size_t)slots[i] * ss->ring_bytes, 0, ss->ring_bytes, s));
    return 0;
}

int64_t fsnp_spec_stream_state_bytes(const fsnp_spec_stream* ss) { return ss ? (int64_t)(ss->mag_bytes + ss->ring_bytes) : 0; }

int fsnp_spec_stream_get_state(fsnp_spec_stream* ss, int32_t slot, void* dev_dst, void* hip_stream) {
    if (!ss || !dev_dst) { set_error("fsnp_spec_stream_get_state: null argument"); return 1; }
    if (slot < 0 || slot >= ss->S) { set_error("fsnp_spec_stream_get_state: slot %d outside [0, %d)", slot, ss->S); return 2; }
    if (const int rc = fsnp_stream_get_state(ss->mag, slot, dev_dst, hip_stream)) return rc;
    if (!ss->ring_bytes) return 0;
    FSNP_ON_DEVICE(ss->h);
    FSNP_HIP_CHECK(hipMemcpyAsync(static_cast<unsigned char*>(dev_dst) + ss->mag_bytes, ss->ring + (size_t)slot * ss->ring_bytes, ss->ring_bytes,
                                  hipMemcpyDeviceToDevice, static_cast<hipStream_t>(hip_stream)));
    return 0;
}

int fsnp_spec_stream_set_state(fsnp_spec_stream* ss, int32_t slot, const void* dev_src, void* hip_stream) {
    if (!ss || !dev_src) { set_error("fsnp_spec_stream_set_state: null argument"); return 1; }
    if (slot < 0 || slot >= ss->S) { set_error("fsnp_spec_stream_set_state: slot %d outside [0, %d)", slot, ss->S); return 2; }
    if (const int rc = fsnp_stream_set_state(ss->mag, slot, dev_src, hip_stream)) return rc;
    if (!ss->ring_bytes) return 0;
    FSNP_ON_DEVICE(ss->h);
    FSNP_HIP_CHECK(hipMemcpyAsync(ss->ring + (size_t)slot * ss->ring_bytes, static_cast<const unsigned char*>(dev_src) + ss->mag_bytes,
                                  ss->ring_bytes, hipMemcpyDeviceToDevice, static_cast<hipStream_t>(hip_stream)));
    return 0;
}

int fsnp_spec_stream_frames(fsnp_spec_stream* ss, int32_t slot, int64_t* pushed) {
    if (!ss || !pushed) { set_error("fsnp_spec_stream_frames: null argument"); return 1; }
    if (slot < 0 || slot >= ss->S) { set_error("fsnp_spec_stream_frames: slot %d outside [0, %d)", slot, ss->S); return 2; }
    return fsnp_stream_frames(ss->mag, slot, pushed);
}

}  // extern "C"
