// fsnp_stream_abi.hip - include/fsnp_stream.h: stream sessions of the original FullSubNet (chunked forwards that carry their state).
//
// A session owns, per slot, one contiguous kernel-independent state record
//   [ sub-band  fp32 [F][layer][h|c][H] | full-band fp32 [layer][h|c][CH] | sub-band norm fp64 [F][sum, sumsq] |
//     full-band norm fp64 [sum, sumsq] | frames int64 ]
// and a workspace of its own for one push of `max_chunk` frames (allocated and zeroed at creation: a push allocates nothing and
// synchronises nothing).  One push on the caller's stream:
//   stream_prologue_kernel   counts (kernel arguments) -> per-slot {P, count}, the slots' frame counts advanced, the row lists of the
//                            active slots (slots without frames are in no row list)
//   launch_frontend_mag_stream   repack + per-frame sums + the full-band cumulative norm continued from the carried sums (frontend.hip)
//   launch_lstm_generic_stream   full-band LSTM(F -> CH x 2) from the carried (h, c), every slot count (lstm_generic.hip)
//   launch_linear_act            Linear(CH, F) + fb_act, as the whole-clip forward
//   launch_subband_stats_stream  the sub-band cumulative norm continued from the carried per-(slot, f) sums (subband.hip)
//   launch_lstm_stream           the fp32 MFMA row-tile kernel from the carried (h0, c0, h1, c1) (lstm.hip), tiles of 32 rows
//   stream_epilogue_kernel       columns past a slot's count and columns of steps before look_ahead written as exactly 0
// A LIVE session (include/fsnp_stream_live.h, max_chunk <= 16) keeps every stage but the two recurrent launches, which become launches per
// layer and step (lstm_step.hip): the slot records' h into the session's parity-0 buffers, then for t < the largest count full-band
// layer 0, layer 1 - Linear, sub-band statistics - and sub-band layer 0, layer 1, Linear(H, 2) per step.  Always, whatever the number of
// active slots or n: a slot's bits do not depend on its neighbours.  Same records, same workspace rules, 4 (H x rows_pad x 32 + S x CH)
// floats of h buffers more.
#include <algorithm>
#include <vector>

#include "fsnp_handle.h"

struct fsnp_stream {
    fsnp_handle* h = nullptr;
    int S = 0, N = 0;                 // slots, max_chunk
    size_t state_bytes = 0;           // one slot
    size_t o_fb = 0, o_sbsum = 0, o_fbsum = 0, o_count = 0;       // byte offsets inside a slot's state
    unsigned char* state = nullptr;   // [S][state_bytes]
    unsigned char* ws = nullptr;
    size_t ws_bytes = 0;
    size_t w_raw = 0, w_fb = 0, w_y1 = 0, w_md = 0, w_frame = 0, w_md_row = 0, w_rows = 0, w_fb_rows = 0, w_meta = 0, w_cnt = 0;
    int rows_pad = 0, fb_rows_pad = 0;
    int live = 0;                     // 1 = a live session (include/fsnp_stream_live.h): every push runs on the per-step kernels of lstm_step.hip
    size_t w_sbh = 0, w_fbh = 0;      // live: sub-band h images [h0 | h1][parity][tile], full-band h vectors [h0 | h1][parity][slot][CH]
    std::vector<int64_t> frames;      // host mirror of the slots' frame counts
    std::vector<char> frames_known;   // 0: the count came with fsnp_stream_set_state (read back on demand)
    hipStream_t last_stream = nullptr;
};

namespace fsnp {

// the streaming path's own plan: tiles of 32 rows over the active slots' F rows each, in rounds of one tile per CU
struct StreamPlan { int rows, tiles, rounds; };
static StreamPlan plan_stream(int active_slots, int F, int num_cus) {
    StreamPlan p{};
    p.rows = active_slots * F;
    p.tiles = cdiv(p.rows, 32);
    p.rounds = cdiv(p.tiles, num_cus > 0 ? num_cus : 1);
    return p;
}

__global__ __launch_bounds__(256) void stream_prologue_kernel(StreamCounts c, int S, int nact, int F, int n, RowDesc* __restrict__ rows,
                                                              int rows_pad, RowDesc* __restrict__ fb_rows, int fb_rows_pad,
                                                              StreamMeta* __restrict__ meta, int* __restrict__ cnt,
                                                              unsigned char* __restrict__ state, size_t state_bytes, size_t o_count) {
    __shared__ int act[kStreamMaxSlots];
    const int tid = threadIdx.x;
    for (int b = tid; b < S; b += 256) {
        if (c.v[b] <= 0) continue;
        int idx = 0;
        for (int i = 0; i < b; ++i) idx += c.v[i] > 0 ? 1 : 0;
        act[idx] = b;
    }
    __syncthreads();
    const int r = blockIdx.x * 256 + tid;
    if (r < rows_pad) {
        const int i = r / F, f = r % F;
        RowDesc rd{0, 0, 0, 0};
        if (i < nact) { const int b = act[i]; rd = RowDesc{b, f, (b * 2 * F + f) * n, c.v[b]}; }
        rows[r] = rd;
    }
    if (blockIdx.x == 0) {
        for (int i = tid; i < fb_rows_pad; i += 256) fb_rows[i] = i < nact ? RowDesc{act[i], 0, 0, c.v[act[i]]} : RowDesc{0, 0, 0, 0};
        for (int b = tid; b < S; b += 256) {
            long long* pc = reinterpret_cast<long long*>(state + (size_t)b * state_bytes + o_count);
            const long long p = *pc;
            meta[b] = StreamMeta{p, c.v[b], 0};
            cnt[b] = c.v[b];
            if (c.v[b] > 0) *pc = p + c.v[b];
        }
    }
}

// out [S][2][F][n]: column j of slot b is 0 where j >= count (nothing was pushed) or P + j < look_ahead (no such frame yet)
__global__ __launch_bounds__(256) void stream_epilogue_kernel(float* __restrict__ out, const StreamMeta* __restrict__ meta, int LA, int per_slot,
                                                              int n, long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const int j = (int)(i % n);
        const StreamMeta m = meta[i / per_slot];
        if (j >= m.cnt || m.p + j < LA) out[i] = 0.0f;
    }
}

// One push behind its checks (fsnp_stream_push, and the waveform sessions of fsnp_wave_stream_abi.hip with the frames each slot
// completed): mag is device memory with strides, c.v[slot] in [0, n] frames of every slot, out contiguous [slots, 2, F, n].
int stream_push_body(fsnp_stream* st, const float* mag, const int64_t strides[3], const StreamCounts& c, float* out, int n, hipStream_t s) {
    fsnp_handle* h = st->h;
    int nact = 0;
    for (int b = 0; b < st->S; ++b) nact += c.v[b] > 0;
    FSNP_ON_DEVICE(h);
    st->last_stream = s;
    const int S = st->S, F = h->F;
    auto fptr = [&](size_t off) { return reinterpret_cast<float*>(st->ws + off); };
    RowDesc* rows = reinterpret_cast<RowDesc*>(st->ws + st->w_rows);
    RowDesc* fb_rows = reinterpret_cast<RowDesc*>(st->ws + st->w_fb_rows);
    StreamMeta* meta = reinterpret_cast<StreamMeta*>(st->ws + st->w_meta);
    int* cnt = reinterpret_cast<int*>(st->ws + st->w_cnt);
    float* state_f = reinterpret_cast<float*>(st->state);
    double* state_d = reinterpret_cast<double*>(st->state);

    if (h->watch_nseg > 0 && (h->watch_calls++ % h->watch_every) == 0)
        if (launch_weight_watch(h, s, false)) return 4;
    hipLaunchKernelGGL(stream_prologue_kernel, dim3(cdiv(st->rows_pad, 256)), dim3(256), 0, s, c, S, nact, F, n, rows, st->rows_pad, fb_rows,
                       st->fb_rows_pad, meta, cnt, st->state, st->state_bytes, st->o_count);
    if (nact > 0) {
        Dims d{};
        d.B = S; d.T = n; d.Tp = n; d.F = F; d.FP = h->FP; d.CH = h->CH; d.H = h->H; d.NSB = h->NSB; d.NIN = h->NIN; d.LA = 0;
        d.lens = cnt;
        FrontendBuffers fbuf{};
        fbuf.raw = fptr(st->w_raw); fbuf.frame = reinterpret_cast<double*>(st->ws + st->w_frame);
        fbuf.md = reinterpret_cast<NormMD*>(st->ws + st->w_md);
        launch_frontend_mag_stream(d, h->cfg.norm_type, mag, strides, fbuf, meta, state_d + st->o_fbsum / 8, (long)(st->state_bytes / 8), s);

        const int rg = lstm_generic_rows_per_group(h->CH, F, nact, h->num_cus_real);
        const int chp = (int)align_up(h->CH, 4);
        LstmArgs fa{};
        fa.rows = fb_rows; fa.dense = fptr(st->w_raw); fa.dense_stride = h->FP; fa.md_seq = fbuf.md;
        fa.seq_out = fptr(st->w_y1); fa.seq_stride = chp;
        fa.num_rows = nact; fa.num_tiles = cdiv(nact, rg); fa.coop_rows_per_group = rg;
        fa.Tp = n; fa.LA = 0; fa.FP = h->FP; fa.F = F;
        fa.st_fb = state_f + st->o_fb / 4; fa.st_stride = (long)(st->state_bytes / 4);
        int nmax = 0;
        for (int b = 0; b < S; ++b) nmax = std::max(nmax, c.v[b]);
        const StreamPlan plan = plan_stream(nact, F, h->num_cus);
        LiveSbArgs la{};
        LiveFbArgs lf{};
        if (st->live) {
            const size_t sbh = live_sb_h_floats(h->H, st->rows_pad / 32), fbh = (size_t)S * h->CH;
            la.rows = rows; la.tiles = plan.tiles; la.Tp = n;
            la.att_mag = fptr(st->w_raw); la.fb_rel = (int)((st->w_fb - st->w_raw) / 4); la.fb_branch_stride = S * n * h->FP;
            la.FP = h->FP; la.F = F; la.NSBN = h->cfg.sb_num_neighbors; la.NFBN = h->cfg.fb_num_neighbors;
            la.md_row = reinterpret_cast<NormMD*>(st->ws + st->w_md_row);
            la.st = state_f; la.st_stride = (long)(st->state_bytes / 4);
            for (int p = 0; p < 2; ++p) { la.h0[p] = fptr(st->w_sbh) + p * sbh; la.h1[p] = fptr(st->w_sbh) + (2 + p) * sbh; }
            la.out = out; la.out_stride_o = (long)F * n; la.act = h->cfg.sb_act;
            lf.rows = fb_rows; lf.num_rows = nact; lf.Tp = n;
            lf.dense = fptr(st->w_raw); lf.dense_stride = h->FP; lf.md_seq = fbuf.md;
            lf.st = state_f + st->o_fb / 4; lf.st_stride = (long)(st->state_bytes / 4);
            for (int p = 0; p < 2; ++p) { lf.h0[p] = fptr(st->w_fbh) + p * fbh; lf.h1[p] = fptr(st->w_fbh) + (2 + p) * fbh; }
            lf.seq_out = fptr(st->w_y1); lf.seq_stride = chp;
            launch_live_load(la, lf, h->H, h->CH, s);
            for (int t = 0; t < nmax; ++t) {
                lf.t = t; lf.par = t & 1;
                launch_live_fb_step(h->fbw, lf, 0, s);
                launch_live_fb_step(h->fbw, lf, 1, s);
            }
        } else launch_lstm_generic_stream(h->fbw, fa, s);
        launch_linear_act(fptr(st->w_y1), chp, h->fsn_wf, h->fsn_kp, h->fsn_bf, fptr(st->w_fb), h->FP, h->CH, F, S, n, h->cfg.fb_act, h->num_cus, s);

        SubbandBuffers sbuf{};
        sbuf.att_mag = fptr(st->w_raw); sbuf.fb = fptr(st->w_fb); sbuf.NFBN = h->cfg.fb_num_neighbors;
        sbuf.md_row = reinterpret_cast<NormMD*>(st->ws + st->w_md_row);
        launch_subband_stats_stream(d, h->cfg.norm_type, sbuf, rows, plan.rows, meta, state_d + st->o_sbsum / 8, (long)(st->state_bytes / 8), s);

        LstmArgs a{};
        a.att_mag = fptr(st->w_raw); a.fb = fptr(st->w_fb);
        a.fb_rel = (int)((st->w_fb - st->w_raw) / 4);
        a.fb_branch_stride = S * n * h->FP;
        a.rows = rows; a.md_row = sbuf.md_row;
        a.out = out; a.out_stride_o = (long)F * n;
        a.num_rows = plan.rows; a.num_tiles = plan.tiles; a.ex = 0;
        a.Tp = n; a.LA = 0; a.FP = h->FP; a.F = F; a.NSBN = h->cfg.sb_num_neighbors; a.NFBN = h->cfg.fb_num_neighbors;
        a.act = h->cfg.sb_act;
        a.st_sb = state_f; a.st_stride = (long)(st->state_bytes / 4);
        if (st->live) {
            for (int t = 0; t < nmax; ++t) {
                la.t = t; la.par = t & 1;
                launch_live_sb_step(h->lw, la, 0, s);
                launch_live_sb_step(h->lw, la, 1, s);
                launch_live_sb_out(h->lw, la, s);
            }
        } else launch_lstm_stream(h->lw, a, s);
    }
    const long total = (long)S * 2 * F * n;
    hipLaunchKernelGGL(stream_epilogue_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, s, out, meta,
                       h->cfg.look_ahead, 2 * F * n, n, total);
    FSNP_HIP_CHECK(hipGetLastError());
    for (int b = 0; b < S; ++b) st->frames[b] += c.v[b];
    return 0;
}

}  // namespace fsnp

static const char* norm_name(int t) {
    return t == FSNP_NORM_OFFLINE_LAPLACE ? "offline_laplace_norm" : t == FSNP_NORM_OFFLINE_GAUSSIAN ? "offline_gaussian_norm" : "?";
}

namespace fsnp {

// fsnp_stream_create / fsnp_stream_create_live (and the mag session inside a wave session): `where` names the entry point in every message
int stream_create(fsnp_handle* h, int32_t slots, int32_t max_chunk, int live, const char* where, fsnp_stream** out) {
    if (!h || !out) { set_error("%s: null argument", where); return 1; }
    *out = nullptr;
    if (h->model != FSNP_MODEL_FULLSUBNET) {
        set_error("%s: FullSubNet+ cannot be streamed exactly: its full-band TCN blocks are not causal and normalise with "
                  "GroupNorm(1, C) over the whole clip, and TSSE pools over all of time; stream the original FullSubNet", where);
        return 2;
    }
    if (h->cfg.norm_type != FSNP_NORM_CUMULATIVE_LAPLACE && h->cfg.norm_type != FSNP_NORM_CUMULATIVE_LAYER) {
        set_error("%s: norm_type %s needs the whole clip's total; streaming needs cumulative_laplace_norm or cumulative_layer_norm", where,
                  norm_name(h->cfg.norm_type));
        return 2;
    }
    if (h->gru || h->sb_tcn) { set_error("%s: sequence_model \"%s\" is not built for streaming (LSTM only)", where, h->gru ? "GRU" : "TCN"); return 2; }
    if (!h->committed) { set_error("%s: weights not committed (call fsnp_commit_weights)", where); return 2; }
    if (h->generic_sb || !lstm_stream_available(h->lw)) {
        set_error("%s: sb_model_hidden_size %d with %d sub-band inputs is outside the row-tile kernel (hidden 256 / 384, <= 64 inputs): not built for streaming", where,
                  h->H, h->NIN);
        return 2;
    }
    const int max_slots = std::min(32 * (h->num_cus_real / 16), kStreamMaxSlots);
    if (slots < 1 || slots > max_slots) { set_error("%s: %d slots; a session holds 1 ... %d (full-band LSTM residency of a whole-clip forward)", where, slots, max_slots); return 2; }
    if (max_chunk < 1) { set_error("%s: max_chunk %d < 1", where, max_chunk); return 2; }
    if (live && max_chunk > kLiveMaxChunk) {
        set_error("%s: max_chunk %d > %d: a live session costs a handful of launches per frame by design; longer chunks belong to a default "
                  "session (fsnp_stream_create)", where, max_chunk, kLiveMaxChunk);
        return 2;
    }
    if (live && !live_sb_available(h->lw)) { set_error("%s: the 16-unit column-split weight image of the sub-band LSTM is not packed for these sizes", where); return 2; }
    if ((double)slots * max_chunk * h->FP * 2 * 2 > 2.0e9) { set_error("%s: slots x max_chunk too large for 32-bit gather offsets", where); return 2; }
    FSNP_ON_DEVICE(h);
    if (lstm_generic_rows_per_group(h->CH, h->F, 1, 1) == 0) { set_error("%s: fb_model_hidden_size %d is too large for the streaming full-band kernel (LDS)", where, h->CH); return 2; }
    if (lstm_generic_stream_check(h->CH, h->F)) return 2;
    if (live && live_fb_check(h->CH, h->F)) return 2;

    fsnp_stream* st = new fsnp_stream();
    st->h = h; st->S = slots; st->N = max_chunk; st->live = live;
    const size_t F = h->F, H = h->H, CH = h->CH;
    st->o_fb = F * 4 * H * 4;
    st->o_sbsum = align_up(st->o_fb + 4 * CH * 4, 8);
    st->o_fbsum = st->o_sbsum + F * 2 * 8;
    st->o_count = st->o_fbsum + 2 * 8;
    st->state_bytes = align_up(st->o_count + 8, 16);
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    const size_t S = slots, N = max_chunk, chp = align_up(CH, 4);
    st->rows_pad = cdiv(slots * h->F, 32) * 32;
    st->fb_rows_pad = slots + 8;
    st->w_raw = take(S * N * h->FP * 4);
    st->w_fb = take(S * N * h->FP * 4);
    st->w_y1 = take(S * N * chp * 4);
    st->w_md = take(S * N * sizeof(NormMD));
    st->w_frame = take(S * N * 2 * 8);
    st->w_md_row = take((size_t)st->rows_pad * N * sizeof(NormMD));
    st->w_rows = take((size_t)st->rows_pad * sizeof(RowDesc));
    st->w_fb_rows = take((size_t)st->fb_rows_pad * sizeof(RowDesc));
    st->w_meta = take(S * sizeof(StreamMeta));
    st->w_cnt = take(S * 4);
    if (live) {
        st->w_sbh = take(4 * live_sb_h_floats(h->H, st->rows_pad / 32) * 4);
        st->w_fbh = take(4 * S * CH * 4);
    }
    st->ws_bytes = o;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&st->state), st->state_bytes * S);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&st->ws), st->ws_bytes);
    if (e == hipSuccess) e = hipMemset(st->state, 0, st->state_bytes * S);
    if (e == hipSuccess) e = hipMemset(st->ws, 0, st->ws_bytes);
    if (e != hipSuccess) {
        set_error("%s: %s (state %zu bytes x %d slots, workspace %zu bytes)", where, hipGetErrorString(e), st->state_bytes, slots, st->ws_bytes);
        if (st->state) (void)hipFree(st->state);
        if (st->ws) (void)hipFree(st->ws);
        delete st;
        return 4;
    }
    st->frames.assign(S, 0);
    st->frames_known.assign(S, 1);
    *out = st;
    return 0;
}

const StreamMeta* stream_meta(const fsnp_stream* st) { return reinterpret_cast<const StreamMeta*>(st->ws + st->w_meta); }

}  // namespace fsnp

extern "C" {

int fsnp_stream_create(fsnp_handle* h, int32_t slots, int32_t max_chunk, fsnp_stream** out) {
    return stream_create(h, slots, max_chunk, 0, "fsnp_stream_create", out);
}

int fsnp_stream_create_live(fsnp_handle* h, int32_t slots, int32_t max_chunk, fsnp_stream** out) {
    return stream_create(h, slots, max_chunk, 1, "fsnp_stream_create_live", out);
}

int fsnp_stream_is_live(const fsnp_stream* st) { return st ? st->live : 0; }

void fsnp_stream_destroy(fsnp_stream* st) {
    if (!st) return;
    fsnp::DeviceGuard g(st->h->device);
    // (hipFree waits for the device: pushes still in flight finish first)
    if (st->state) (void)hipFree(st->state);
    if (st->ws) (void)hipFree(st->ws);
    delete st;
}

int fsnp_stream_push(fsnp_stream* st, const float* mag, const int64_t strides[3], const int32_t* counts, float* out, int32_t n,
                     void* hip_stream) {
    if (!st || !mag || !strides || !out) { set_error("fsnp_stream_push: null argument"); return 1; }
    fsnp_handle* h = st->h;
    if (n < 1 || n > st->N) { set_error("fsnp_stream_push: n = %d outside [1, max_chunk = %d]", n, st->N); return 2; }
    StreamCounts c{};
    for (int b = 0; b < st->S; ++b) {
        const int v = counts ? counts[b] : n;
        if (v < 0 || v > n) { set_error("fsnp_stream_push: slot %d: count %d outside [0, n = %d]", b, v, n); return 2; }
        c.v[b] = v;
    }
    if (!h->committed) { set_error("fsnp_stream_push: weights not committed (call fsnp_commit_weights)"); return 2; }
    if (const int ec = take_device_errors(h, "an earlier call on this handle failed")) return ec;
    return stream_push_body(st, mag, strides, c, out, n, static_cast<hipStream_t>(hip_stream));
}

int fsnp_stream_reset(fsnp_stream* st, const int32_t* slots, int32_t num, void* hip_stream) {
    if (!st) { set_error("fsnp_stream_reset: null argument"); return 1; }
    if (slots) {
        if (num < 0) { set_error("fsnp_stream_reset: num = %d", num); return 2; }
        for (int i = 0; i < num; ++i)
            if (slots[i] < 0 || slots[i] >= st->S) { set_error("fsnp_stream_reset: slot %d outside [0, %d)", slots[i], st->S); return 2; }
    }
    FSNP_ON_DEVICE(st->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    st->last_stream = s;
    if (!slots) {
        FSNP_HIP_CHECK(hipMemsetAsync(st->state, 0, st->state_bytes * st->S, s));
        std::fill(st->frames.begin(), st->frames.end(), 0);
        std::fill(st->frames_known.begin(), st->frames_known.end(), 1);
        return 0;
    }
    for (int i = 0; i < num; ++i) {
        FSNP_HIP_CHECK(hipMemsetAsync(st->state + (size_t)slots[i] * st->state_bytes, 0, st->state_bytes, s));
        st->frames[slots[i]] = 0; st->frames_known[slots[i]] = 1;
    }
    return 0;
}

int64_t fsnp_stream_state_bytes(const fsnp_stream* st) { return st ? (int64_t)st->state_bytes : 0; }

int fsnp_stream_get_state(fsnp_stream* st, int32_t slot, void* dev_dst, void* hip_stream) {
    if (!st || !dev_dst) { set_error("fsnp_stream_get_state: null argument"); return 1; }
    if (slot < 0 || slot >= st->S) { set_error("fsnp_stream_get_state: slot %d outside [0, %d)", slot, st->S); return 2; }
    FSNP_ON_DEVICE(st->h);
    FSNP_HIP_CHECK(hipMemcpyAsync(dev_dst, st->state + (size_t)slot * st->state_bytes, st->state_bytes, hipMemcpyDeviceToDevice,
                                  static_cast<hipStream_t>(hip_stream)));
    return 0;
}

int fsnp_stream_set_state(fsnp_stream* st, int32_t slot, const void* dev_src, void* hip_stream) {
    if (!st || !dev_src) { set_error("fsnp_stream_set_state: null argument"); return 1; }
    if (slot < 0 || slot >= st->S) { set_error("fsnp_stream_set_state: slot %d outside [0, %d)", slot, st->S); return 2; }
    FSNP_ON_DEVICE(st->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_HIP_CHECK(hipMemcpyAsync(st->state + (size_t)slot * st->state_bytes, dev_src, st->state_bytes, hipMemcpyDeviceToDevice, s));
    st->last_stream = s;
    st->frames[slot] = 0; st->frames_known[slot] = 0;
    return 0;
}

int fsnp_stream_frames(fsnp_stream* st, int32_t slot, int64_t* pushed) {
    if (!st || !pushed) { set_error("fsnp_stream_frames: null argument"); return 1; }
    if (slot < 0 || slot >= st->S) { set_error("fsnp_stream_frames: slot %d outside [0, %d)", slot, st->S); return 2; }
    if (!st->frames_known[slot]) {       // loaded with fsnp_stream_set_state: the count lives in the record (+ what was pushed since)
        FSNP_ON_DEVICE(st->h);
        long long v = 0;
        FSNP_HIP_CHECK(hipMemcpyAsync(&v, st->state + (size_t)slot * st->state_bytes + st->o_count, 8, hipMemcpyDeviceToHost, st->last_stream));
        FSNP_HIP_CHECK(hipStreamSynchronize(st->last_stream));
        st->frames[slot] = v; st->frames_known[slot] = 1;
    }
    *pushed = st->frames[slot];
    return 0;
}

}  // extern "C"
