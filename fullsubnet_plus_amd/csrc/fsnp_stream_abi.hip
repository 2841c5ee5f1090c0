// fsnp_stream_abi.hip - include/fsnp_stream.h: stream sessions of the original FullSubNet (chunked forwards that carry their state).
//
// A session owns, per slot, one contiguous kernel-independent state record (a SlotRecords array, fsnp_handle.h)
//   [ sub-band  fp32 [F][layer][h|c][H] | full-band fp32 [layer][h|c][CH] | sub-band norm fp64 [F][sum, sumsq] |
//     full-band norm fp64 [sum, sumsq] | frames int64 ]
// and a workspace of its own for one push of `max_chunk` frames (allocated and zeroed at creation: a push allocates nothing and
// synchronises nothing).  One push on the caller's stream (stream_push_body, which wave and spectrum sessions reach through
// spec_push_body below):
//   stream_prologue_kernel       counts (kernel arguments) -> per-slot {P, count}, the slots' frame counts advanced, the row lists of the
//                                active slots (slots without frames are in no row list)
//   launch_frontend_mag_stream   repack + per-frame sums + the full-band cumulative norm continued from the carried sums (frontend.hip)
//   full-band recurrent part     chunked_fullband / live_fullband
//   launch_linear_act            Linear(CH, F) + fb_act, as the whole-clip forward
//   launch_subband_stats_stream  the sub-band cumulative norm continued from the carried per-(slot, f) sums (subband.hip)
//   sub-band recurrent part      chunked_subband / live_subband
//   stream_epilogue_kernel       columns past a slot's count and columns of steps before look_ahead written as exactly 0
// The recurrent parts of a default session are one launch each (chunked_*): launch_lstm_generic_stream, the full-band LSTM(F -> CH x 2)
// from the carried (h, c) at every slot count (lstm_generic.hip), and launch_lstm_stream, the fp32 MFMA row-tile kernel from the carried
// (h0, c0, h1, c1) in tiles of 32 rows (lstm.hip).  A LIVE session (include/fsnp_stream_live.h, max_chunk <= 16) runs them as launches per
// layer and step (live_*, lstm_step.hip): the slot records' h into the session's parity-0 buffers, then for t < the largest count
// full-band layer 0, layer 1 - Linear, sub-band statistics - and sub-band layer 0, layer 1, Linear(H, 2) per step.  Always, whatever the
// number of active slots or n: a slot's bits do not depend on its neighbours.  Same records, same workspace rules, 4 (H x rows_pad x 32
// + S x CH) floats of h buffers more.
#include <algorithm>
#include <vector>

#include "fsnp_handle.h"

struct fsnp_stream {
    fsnp_handle* h = nullptr;
    int S = 0, N = 0;                 // slots, max_chunk
    SlotRecords rec;                  // the slots' state records
    size_t o_fb = 0, o_sbsum = 0, o_fbsum = 0, o_count = 0;       // byte offsets inside a record
    unsigned char* ws = nullptr;
    size_t ws_bytes = 0;
    size_t w_raw = 0, w_fb = 0, w_y1 = 0, w_md = 0, w_frame = 0, w_md_row = 0, w_rows = 0, w_fb_rows = 0, w_meta = 0, w_cnt = 0;
    int rows_pad = 0, fb_rows_pad = 0;
    int live = 0;                     // 1 = a live session (include/fsnp_stream_live.h): every push runs on the per-step kernels of lstm_step.hip
    size_t w_sbh = 0, w_fbh = 0;      // live: sub-band h images [h0 | h1][parity][tile], full-band h vectors [h0 | h1][parity][slot][CH]
    std::vector<int64_t> frames;      // host mirror of the slots' frame counts
    std::vector<char> frames_known;   // 0: the count came with fsnp_stream_set_state (read back on demand)
    hipStream_t last_stream = nullptr;
    template <class T> T* at(size_t off) const { return reinterpret_cast<T*>(ws + off); }      // inside the workspace
    float* state_f() const { return reinterpret_cast<float*>(rec.base); }
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

__global__ __launch_bounds__(256) void stream_prologue_kernel(SlotCounts c, int S, int nact, int F, int n, RowDesc* __restrict__ rows,
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

// the arguments of the two recurrent launches of a default session's push: launch_lstm_generic_stream (full-band, every slot from its
// carried (h, c)) and launch_lstm_stream (sub-band row tiles, every row from its carried (h0, c0, h1, c1))
struct ChunkedArgs { LstmArgs fb, sb; };
static ChunkedArgs chunked_args(const fsnp_stream* st, int n, int nact, const StreamPlan& plan, float* out) {
    const fsnp_handle* h = st->h;
    const int rg = lstm_generic_rows_per_group(h->CH, h->F, nact, h->num_cus_real);
    ChunkedArgs c{};
    LstmArgs& fa = c.fb;
    fa.rows = st->at<RowDesc>(st->w_fb_rows); fa.dense = st->at<float>(st->w_raw); fa.dense_stride = h->FP; fa.md_seq = st->at<NormMD>(st->w_md);
    fa.seq_out = st->at<float>(st->w_y1); fa.seq_stride = (int)align_up(h->CH, 4);
    fa.num_rows = nact; fa.num_tiles = cdiv(nact, rg); fa.coop_rows_per_group = rg;
    fa.Tp = n; fa.LA = 0; fa.FP = h->FP; fa.F = h->F;
    fa.st_fb = st->state_f() + st->o_fb / 4; fa.st_stride = (long)(st->rec.bytes / 4);
    LstmArgs& a = c.sb;
    a.att_mag = st->at<float>(st->w_raw); a.fb = st->at<float>(st->w_fb);
    a.fb_rel = (int)((st->w_fb - st->w_raw) / 4);
    a.fb_branch_stride = st->S * n * h->FP;
    a.rows = st->at<RowDesc>(st->w_rows); a.md_row = st->at<NormMD>(st->w_md_row);
    a.out = out; a.out_stride_o = (long)h->F * n;
    a.num_rows = plan.rows; a.num_tiles = plan.tiles; a.ex = 0;
    a.Tp = n; a.LA = 0; a.FP = h->FP; a.F = h->F; a.NSBN = h->cfg.sb_num_neighbors; a.NFBN = h->cfg.fb_num_neighbors;
    a.act = h->cfg.sb_act;
    a.st_sb = st->state_f(); a.st_stride = (long)(st->rec.bytes / 4);
    return c;
}

// the arguments of a live session's launches per layer and step (lstm_step.hip); t and par are the caller's to set
struct LiveArgs { LiveFbArgs fb; LiveSbArgs sb; };
static LiveArgs live_args(const fsnp_stream* st, int n, int nact, const StreamPlan& plan, float* out) {
    const fsnp_handle* h = st->h;
    const int S = st->S;
    const size_t sbh = live_sb_h_floats(h->H, st->rows_pad / 32), fbh = (size_t)S * h->CH;
    LiveArgs l{};
    LiveSbArgs& la = l.sb;
    la.rows = st->at<RowDesc>(st->w_rows); la.tiles = plan.tiles; la.Tp = n;
    la.att_mag = st->at<float>(st->w_raw); la.fb_rel = (int)((st->w_fb - st->w_raw) / 4); la.fb_branch_stride = S * n * h->FP;
    la.FP = h->FP; la.F = h->F; la.NSBN = h->cfg.sb_num_neighbors; la.NFBN = h->cfg.fb_num_neighbors;
    la.md_row = st->at<NormMD>(st->w_md_row);
    la.st = st->state_f(); la.st_stride = (long)(st->rec.bytes / 4);
    for (int p = 0; p < 2; ++p) { la.h0[p] = st->at<float>(st->w_sbh) + p * sbh; la.h1[p] = st->at<float>(st->w_sbh) + (2 + p) * sbh; }
    la.out = out; la.out_stride_o = (long)h->F * n; la.act = h->cfg.sb_act;
    LiveFbArgs& lf = l.fb;
    lf.rows = st->at<RowDesc>(st->w_fb_rows); lf.num_rows = nact; lf.Tp = n;
    lf.dense = st->at<float>(st->w_raw); lf.dense_stride = h->FP; lf.md_seq = st->at<NormMD>(st->w_md);
    lf.st = st->state_f() + st->o_fb / 4; lf.st_stride = (long)(st->rec.bytes / 4);
    for (int p = 0; p < 2; ++p) { lf.h0[p] = st->at<float>(st->w_fbh) + p * fbh; lf.h1[p] = st->at<float>(st->w_fbh) + (2 + p) * fbh; }
    lf.seq_out = st->at<float>(st->w_y1); lf.seq_stride = (int)align_up(h->CH, 4);
    return l;
}

// One push behind its checks (fsnp_stream_push, and spec_push_body for spectrum and wave sessions): mag is device memory with strides,
// c.v[slot] in [0, n] frames of every slot, out contiguous [slots, 2, F, n].
int stream_push_body(fsnp_stream* st, const float* mag, const int64_t strides[3], const SlotCounts& c, float* out, int n, hipStream_t s) {
    fsnp_handle* h = st->h;
    const int S = st->S, F = h->F;
    int nact = 0, nmax = 0;
    for (int b = 0; b < S; ++b) { nact += c.v[b] > 0; nmax = std::max(nmax, c.v[b]); }
    FSNP_ON_DEVICE(h);
    st->last_stream = s;
    if (order_after_weight_pack(h, s)) return 4;      // (a device pack of the weights on another stream: fsnp_commit_weights_on)
    RowDesc* rows = st->at<RowDesc>(st->w_rows);
    StreamMeta* meta = st->at<StreamMeta>(st->w_meta);
    int* cnt = st->at<int>(st->w_cnt);
    double* state_d = reinterpret_cast<double*>(st->rec.base);
    const long sum_stride = (long)(st->rec.bytes / 8);

    if (h->watch_nseg > 0 && (h->watch_calls++ % h->watch_every) == 0)
        if (launch_weight_watch(h, s, false)) return 4;
    hipLaunchKernelGGL(stream_prologue_kernel, dim3(cdiv(st->rows_pad, 256)), dim3(256), 0, s, c, S, nact, F, n, rows, st->rows_pad,
                       st->at<RowDesc>(st->w_fb_rows), st->fb_rows_pad, meta, cnt, st->rec.base, st->rec.bytes, st->o_count);
    if (nact > 0) {
        Dims d{};
        d.B = S; d.T = n; d.Tp = n; d.F = F; d.FP = h->FP; d.CH = h->CH; d.H = h->H; d.NSB = h->NSB; d.NIN = h->NIN; d.LA = 0;
        d.lens = cnt;
        FrontendBuffers fbuf{};
        fbuf.raw = st->at<float>(st->w_raw); fbuf.frame = st->at<double>(st->w_frame); fbuf.md = st->at<NormMD>(st->w_md);
        launch_frontend_mag_stream(d, h->cfg.norm_type, mag, strides, fbuf, meta, state_d + st->o_fbsum / 8, sum_stride, s);

        const StreamPlan plan = plan_stream(nact, F, h->num_cus);
        ChunkedArgs chunked;      // (only the session's own set is filled and read)
        LiveArgs live;
        if (st->live) {
            live = live_args(st, n, nact, plan, out);
            launch_live_load(live.sb, live.fb, h->H, h->CH, s);
            for (int t = 0; t < nmax; ++t) {
                live.fb.t = t; live.fb.par = t & 1;
                launch_live_fb_step(h->fbw, live.fb, 0, s);
                launch_live_fb_step(h->fbw, live.fb, 1, s);
            }
        } else {
            chunked = chunked_args(st, n, nact, plan, out);
            launch_lstm_generic_stream(h->fbw, chunked.fb, s);
        }
        launch_linear_act(st->at<float>(st->w_y1), (int)align_up(h->CH, 4), h->fsn_wf, h->fsn_kp, h->fsn_bf, st->at<float>(st->w_fb), h->FP, h->CH,
                          F, S, n, h->cfg.fb_act, h->num_cus, s);

        SubbandBuffers sbuf{};
        sbuf.att_mag = st->at<float>(st->w_raw); sbuf.fb = st->at<float>(st->w_fb); sbuf.NFBN = h->cfg.fb_num_neighbors;
        sbuf.md_row = st->at<NormMD>(st->w_md_row);
        launch_subband_stats_stream(d, h->cfg.norm_type, sbuf, rows, plan.rows, meta, state_d + st->o_sbsum / 8, sum_stride, s);

        if (st->live) {
            for (int t = 0; t < nmax; ++t) {
                live.sb.t = t; live.sb.par = t & 1;
                launch_live_sb_step(h->lw, live.sb, 0, s);
                launch_live_sb_step(h->lw, live.sb, 1, s);
                launch_live_sb_out(h->lw, live.sb, s);
            }
        } else launch_lstm_stream(h->lw, chunked.sb, s);
    }
    const long total = (long)S * 2 * F * n;
    hipLaunchKernelGGL(stream_epilogue_kernel, dim3((unsigned)std::min<long>((total + 255) / 256, 4096)), dim3(256), 0, s, out, meta,
                       h->cfg.look_ahead, 2 * F * n, n, total);
    FSNP_HIP_CHECK(hipGetLastError());
    for (int b = 0; b < S; ++b) st->frames[b] += c.v[b];
    return 0;
}

// One ring push behind its checks (fsnp_handle.h): the mag push between the two launches of spec_stream.hip, whose apply kernel finds
// {P, steps} of every slot where the prologue kernel above left them.
int spec_push_body(fsnp_stream* st, const SpecRing& ring, float* mag, float* mask, const float* spec, const int64_t strides[3],
                   const SlotCounts& spectra, const SlotCounts& steps, float* out, const int64_t out_strides[3], bool write_idle, int n,
                   hipStream_t s) {
    fsnp_handle* h = st->h;
    SpecArgs a{};
    a.ring = ring.ring; a.ring_stride = ring.ring_stride; a.meta = st->at<StreamMeta>(st->w_meta);
    a.S = st->S; a.F = h->F; a.FP = h->FP; a.LA = ring.look_ahead; a.n = n;
    int total = 0;
    for (int b = 0; b < st->S; ++b) total += steps.v[b];
    FSNP_ON_DEVICE(h);
    if (total > 0) launch_spec_mag(a, spectra, spec, strides, mag, s);
    const int64_t mst[3] = {(int64_t)n * h->FP, 1, h->FP};             // mag [S][n][FP] as (slot, f, frame)
    if (const int rc = stream_push_body(st, mag, mst, steps, mask, n, s)) return rc;
    if (total > 0 || write_idle) launch_spec_apply(a, spectra, mask, spec, strides, out, out_strides, s);
    FSNP_HIP_CHECK(hipGetLastError());
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
    const size_t state_bytes = align_up(st->o_count + 8, 16);
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
    hipError_t e = st->rec.create(state_bytes, slots);
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&st->ws), st->ws_bytes);
    if (e == hipSuccess) e = hipMemset(st->ws, 0, st->ws_bytes);
    if (e != hipSuccess) {
        set_error("%s: %s (state %zu bytes x %d slots, workspace %zu bytes)", where, hipGetErrorString(e), state_bytes, slots, st->ws_bytes);
        st->rec.free();
        if (st->ws) (void)hipFree(st->ws);
        delete st;
        return 4;
    }
    st->frames.assign(S, 0);
    st->frames_known.assign(S, 1);
    *out = st;
    return 0;
}

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
    st->rec.free();
    if (st->ws) (void)hipFree(st->ws);
    delete st;
}

int fsnp_stream_push(fsnp_stream* st, const float* mag, const int64_t strides[3], const int32_t* counts, float* out, int32_t n,
                     void* hip_stream) {
    if (!st || !mag || !strides || !out) { set_error("fsnp_stream_push: null argument"); return 1; }
    if (n < 1 || n > st->N) { set_error("fsnp_stream_push: n = %d outside [1, max_chunk = %d]", n, st->N); return 2; }
    SlotCounts c{};
    if (const int rc = read_counts("fsnp_stream_push", counts, st->S, n, c)) return rc;
    if (const int rc = push_preamble(st->h, "fsnp_stream_push")) return rc;
    return stream_push_body(st, mag, strides, c, out, n, static_cast<hipStream_t>(hip_stream));
}

int fsnp_stream_reset(fsnp_stream* st, const int32_t* slots, int32_t num, void* hip_stream) {
    if (!st) { set_error("fsnp_stream_reset: null argument"); return 1; }
    if (const int rc = check_slots("fsnp_stream_reset", slots, num, st->S)) return rc;
    FSNP_ON_DEVICE(st->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    st->last_stream = s;
    if (const int rc = st->rec.reset(slots, num, s)) return rc;
    if (!slots) {
        std::fill(st->frames.begin(), st->frames.end(), 0);
        std::fill(st->frames_known.begin(), st->frames_known.end(), 1);
    } else
        for (int i = 0; i < num; ++i) { st->frames[slots[i]] = 0; st->frames_known[slots[i]] = 1; }
    return 0;
}

int64_t fsnp_stream_state_bytes(const fsnp_stream* st) { return st ? (int64_t)st->rec.bytes : 0; }

int fsnp_stream_get_state(fsnp_stream* st, int32_t slot, void* dev_dst, void* hip_stream) {
    if (!st || !dev_dst) { set_error("fsnp_stream_get_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_stream_get_state", slot, st->S)) return rc;
    FSNP_ON_DEVICE(st->h);
    return st->rec.get(slot, dev_dst, 0, static_cast<hipStream_t>(hip_stream));
}

int fsnp_stream_set_state(fsnp_stream* st, int32_t slot, const void* dev_src, void* hip_stream) {
    if (!st || !dev_src) { set_error("fsnp_stream_set_state: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_stream_set_state", slot, st->S)) return rc;
    FSNP_ON_DEVICE(st->h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (const int rc = st->rec.set(slot, dev_src, 0, s)) return rc;
    st->last_stream = s;
    st->frames[slot] = 0; st->frames_known[slot] = 0;
    return 0;
}

int fsnp_stream_frames(fsnp_stream* st, int32_t slot, int64_t* pushed) {
    if (!st || !pushed) { set_error("fsnp_stream_frames: null argument"); return 1; }
    if (const int rc = check_slot("fsnp_stream_frames", slot, st->S)) return rc;
    if (!st->frames_known[slot]) {       // loaded with fsnp_stream_set_state: the count lives in the record (+ what was pushed since)
        FSNP_ON_DEVICE(st->h);
        long long v = 0;
        FSNP_HIP_CHECK(hipMemcpyAsync(&v, st->rec.slot(slot) + st->o_count, 8, hipMemcpyDeviceToHost, st->last_stream));
        FSNP_HIP_CHECK(hipStreamSynchronize(st->last_stream));
        st->frames[slot] = v; st->frames_known[slot] = 1;
    }
    *pushed = st->frames[slot];
    return 0;
}

}  // extern "C"
