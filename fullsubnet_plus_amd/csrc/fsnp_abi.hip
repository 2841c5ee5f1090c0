// fsnp_abi.hip - C ABI of libfsnp_hip.so (include/fsnp.h): handle life cycle, workspace management, cost calibration and the forward
// orchestration (its sub-band launches, and the per-device chain of column-split launches).  Host code only; kernels live in
// forward_kernels.hip / frontend.hip / tcn.hip / subband.hip / lstm*.hip; the exchange checks in fsnp_verify.hip, the planner in
// planner.cpp, weight packing in fsnp_weights.hip, the STFT entry points in fsnp_stft_abi.hip, the include/fsnp_debug.h hooks in
// fsnp_debug_abi.hip (shared declarations: fsnp_handle.h).
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "fsnp_common.h"
#include "lstm_common.h"
#include "planner.h"
#include "fsnp_handle.h"

namespace fsnp {

static thread_local std::string g_last_error;

void set_error(const char* fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_last_error = buf;
}

}  // namespace fsnp

using namespace fsnp;

namespace fsnp {

// Decodes and clears the host-mapped error word that finished launches set (fsnp_handle.h: kErr*).  0 = clean.
// The word is TAKEN with one atomic exchange (a bit the device ORs in between a read and a separate clearing store would be lost:
// ADVICE r05) and every condition that was set is named in the message; the return code is the gravest one (5 > 7 > 6).
int take_device_errors(fsnp_handle* h, const char* where) {
    unsigned* e = reinterpret_cast<unsigned*>(h->d_err);
    if (__atomic_load_n(e, __ATOMIC_ACQUIRE) == 0) return 0;
    const unsigned bits = __atomic_exchange_n(e, 0u, __ATOMIC_ACQ_REL);
    if (bits == 0) return 0;
    std::string msg = std::string(where) + ":";
    int rc = 0;
    if (bits & kErrTimeout) {
        msg += " an inter-workgroup wait timed out in a column-split LSTM kernel (its workgroups were not co-resident - is the GPU "
               "shared with another process?); the result of that forward is invalid.  FSNP_LSTM_COOP=0 avoids these kernels.";
        rc = 5;
    }
    if (bits & kErrVerify) {
        // where the two kernels first disagreed: a 64-bit key in DEVICE memory (utterance << 44 | bin << 24 | frame; atomic min), read
        // back here - on the error path only - once the comparing kernel has finished
        unsigned long long key = ~0ull;
        if (h->verify_key || h->verify_key_sampled) {
            fsnp::DeviceGuard guard(h->device);
            (void)hipDeviceSynchronize();
            for (unsigned long long* src : {h->verify_key, h->verify_key_sampled}) {
                unsigned long long k = ~0ull;
                if (src && hipMemcpy(&k, src, 8, hipMemcpyDeviceToHost) != hipSuccess) { (void)hipGetLastError(); k = ~0ull; }
                if (k < key) key = k;
            }
        }
        char at[160];
        if (key != ~0ull) snprintf(at, sizeof(at), ", first at utterance %llu, bin %llu, frame %llu", key >> 44, (key >> 24) & 0xFFFFFull, key & 0xFFFFFFull);
        else at[0] = 0;
        msg += std::string(rc ? " ALSO:" : "") + " exchange verification failed (fsnp_set_verify): the column-split kernels and the exchange-free "
               "kernel disagree" + at + "; the result of that forward is invalid (a sampled check - fsnp_set_verify_sample - reports a forward "
               "of up to a few calls ago).  FSNP_LSTM_COOP=0 avoids the column-split kernels.";
        if (!rc) rc = 7;
    }
    if (bits & kErrStaleWeights) {
        msg += std::string(rc ? " ALSO:" : "") + " the watched source tensors no longer match the packed weights (a parameter was modified in "
               "place through .data after packing): forwards since that edit ran on the OLD weights - re-pack (fsnp_set_weight / "
               "fsnp_commit_weights / fsnp_watch_weights; Python: model.refresh_weights()).";
        if (!rc) rc = 6;
    }
    if (!rc) { msg += " unknown device error bits"; rc = 4; }
    set_error("%s", msg.c_str());
    return rc;
}

// what the planner needs to know of a handle
PlannerCtx pctx(const fsnp_handle* h) {
    PlannerCtx c;
    static_cast<PlannerOptions&>(c) = h->planner;
    c.H = h->H; c.NIN = h->NIN; c.num_cus = h->num_cus; c.num_cus_real = h->num_cus_real;
    c.gru = h->gru != 0; c.sb_tcn = h->sb_tcn != 0; c.generic_sb = h->generic_sb; c.ih_bf16 = h->ih_bf16;
    return c;
}

// The one statement of the TSSE frame floor: a clip's frames + look_ahead must reach the attention's largest kernel (0: no such rule -
// the original FullSubNet, or another attention).  check_lengths, the equal-length forward and min_clip_frames all ask here.
static int tsse_largest_kernel(const fsnp_handle* h) {
    if (h->model == FSNP_MODEL_FULLSUBNET || h->cfg.attention != FSNP_ATT_TSSE) return 0;
    int kmax = 1;
    for (int c = 0; c < 3; ++c) kmax = std::max(kmax, (int)h->cfg.kersize[c]);
    return kmax;
}
int min_clip_frames(const fsnp_handle* h) { return std::max(1, tsse_largest_kernel(h) - (int)h->cfg.look_ahead); }

int check_lengths(const fsnp_handle* h, const int32_t* lengths, int batch, int frames, const char* where) {
    if (!lengths) { set_error("%s: null lengths", where); return 1; }
    const bool fsn = h->model == FSNP_MODEL_FULLSUBNET;
    // out of scope, refused rather than mis-computed: the ECA channel regrouping of subband_num > 1, and the sub-band TCN stack (its
    // GroupNorm is per sub-band sequence, which would need a length per slot)
    if (!fsn && h->cfg.subband_num > 1) { set_error("%s: per-utterance lengths are not supported with subband_num = %d > 1", where, h->cfg.subband_num); return 2; }
    if (h->sb_tcn) { set_error("%s: per-utterance lengths are not supported with the sub-band sequence_model \"TCN\"", where); return 2; }
    const int kmax = tsse_largest_kernel(h);
    for (int b = 0; b < batch; ++b) {
        if (lengths[b] < 1 || lengths[b] > frames) {
            set_error("%s: utterance %d: length %d outside [1, %d]", where, b, (int)lengths[b], frames);
            return 2;
        }
        if (lengths[b] + h->cfg.look_ahead < kmax) {
            set_error("%s: utterance %d: too few frames: length %d + look_ahead %d = %d < largest TSSE kernel %d", where, b, (int)lengths[b],
                      (int)h->cfg.look_ahead, (int)lengths[b] + h->cfg.look_ahead, kmax);
            return 2;
        }
    }
    return 0;
}

// Column-split launches need all their workgroups co-resident.  Two of them running at once (two handles / two streams
// of one process) could each hold part of the chip and wait for peers that cannot be scheduled, so within a process
// they are chained per device: each one waits for the previous one's completion event.  Other kernels always finish,
// so they cannot close a cycle; a foreign PROCESS still can - that case ends in the kernels' wall-clock timeout.
// Two such launches of ONE handle on two streams may run side by side when one of them can always become fully resident whatever the other
// holds, counted per XCD (planner.h coop_side_by_side): the pipelined loop's deferred remainder chunk of forward i (side stream, owns its
// CUs) and the original FullSubNet's full-band LSTM of forward i + 1 (caller's stream) used to wait for each other through this chain,
// which is what kept FullSubNet at B = 32 above its 29 ms bar (29.7 -> 28.5 ms).  Round 6 decided this on whole-chip totals (sum of
// workgroups <= CUs - 8); the dispatcher deals workgroups to the XCDs by index, not by room, so a pair that fits the chip can still
// overflow an XCD (a 2-tile half-tile ping-pong remainder - 24 owned CUs on each of two XCDs - beside a 2-tile full-band launch at one
// workgroup per CU: 24 + 16 > 32).  Everything else (other handles, unknown sizes or occupancy) is chained as before; an earlier launch
// on the same stream is behind this one anyway (waited for - a no-op in stream order - and not counted).
static std::mutex g_coop_mu;
struct CoopSlot {
    hipEvent_t ev = nullptr; bool used = false; const void* owner = nullptr; hipStream_t stream = nullptr;
    bool has_fp = false; CoopFootprint fp{}; unsigned long long seq = 0;
};
static CoopSlot g_coop[64][2];
static unsigned long long g_coop_seq = 0;
// fp = where the launch's workgroups go (nullptr: unknown - chained); counts the earlier launches of `owner` on other streams this one
// runs beside / was chained behind into owner_stats (fsnp_debug_coop_chain_stats)
template <typename F>
static void launch_coop_chained(int dev, hipStream_t s, F launch, const void* owner = nullptr, const CoopFootprint* fp = nullptr,
                                int cus_per_xcd = 0, int64_t* owner_stats = nullptr) {
    if (dev < 0 || dev >= 64) { launch(); return; }
    std::lock_guard<std::mutex> lk(g_coop_mu);
    CoopSlot* sl = g_coop[dev];
    const int order[2] = {sl[0].seq <= sl[1].seq ? 0 : 1, sl[0].seq <= sl[1].seq ? 1 : 0};      // older first
    bool behind[2] = {false, false};
    int beside = -1;                    // a slot this launch runs beside
    for (int o = 0; o < 2; ++o) {
        const int k = order[o];
        CoopSlot& c = sl[k];
        if (!c.used) continue;
        const bool other_stream = c.stream != s, mine = owner && c.owner == owner;
        bool fits = other_stream && mine && fp && c.has_fp;
        if (fits) {
            // (a launch this one already runs beside, on a third stream, may be in flight together with c: both are blockers then)
            const bool both = beside >= 0 && sl[beside].stream != c.stream;
            fits = coop_side_by_side(both ? coop_footprint_sum(*fp, sl[beside].fp) : *fp, c.fp, cus_per_xcd);
        }
        if (fits) beside = k;
        else { (void)hipStreamWaitEvent(s, c.ev, 0); behind[k] = true; }
        if (other_stream && mine && owner_stats) ++owner_stats[fits ? 0 : 1];
    }
    launch();
    // the slot this launch takes: a free one, else one it waited for (that launch is behind it now), else one that has finished, else
    // the older one - after waiting for it
    int k = -1;
    for (int i = 0; i < 2 && k < 0; ++i) if (!sl[i].used) k = i;
    for (int o = 0; o < 2 && k < 0; ++o) if (behind[order[o]]) k = order[o];
    for (int o = 0; o < 2 && k < 0; ++o) {
        if (hipEventQuery(sl[order[o]].ev) == hipSuccess) k = order[o];
        else (void)hipGetLastError();
    }
    if (k < 0) { k = order[0]; (void)hipStreamWaitEvent(s, sl[k].ev, 0); }
    if (!sl[k].ev && hipEventCreateWithFlags(&sl[k].ev, hipEventDisableTiming) != hipSuccess) { sl[k].ev = nullptr; sl[k].used = false; return; }
    sl[k].used = hipEventRecord(sl[k].ev, s) == hipSuccess;
    sl[k].owner = owner; sl[k].stream = s; sl[k].seq = ++g_coop_seq;
    sl[k].has_fp = fp != nullptr;
    if (fp) sl[k].fp = *fp;
}

// The planner itself (cost table, launch shapes, shortest path over tile counts) is host-only code: planner.h / planner.cpp.
// gather_bytes: the furthest byte a recurrent kernel's input gather reaches from its base pointer.  The half-tile ping-pong kernel
// (lstm_hp.hip) addresses its input through ONE buffer descriptor with 32-bit BYTE offsets (2 GiB), the other kernels with 32-bit
// FLOAT offsets from a 64-bit pointer (8 GiB): beyond 2 GiB the planner is told not to use it (its loads would
// otherwise return zeros - out of the descriptor's range - and the sequences run on zero input without any error).
SbPlan plan_sb(const fsnp_handle* h, int num_rows, double gather_bytes) {
    PlannerCtx c = pctx(h);
    if (gather_bytes >= 2147483644.0) c.coop_hp = 0;
    return plan_sb(c, num_rows);
}
// forward: rows are gathered from att_mag [B][Tp][FP] and the full-band planes behind it (plan_workspace: att, fb adjacent)
static double forward_gather_bytes(const fsnp_handle* h, int B, int T) {
    const double nbr = h->model == FSNP_MODEL_FULLSUBNET ? 1 : 3;
    return 2.0 * ((double)align_up((size_t)(nbr * B * ((double)T + h->cfg.look_ahead) * h->FP * 4), 256));
}
int chunk_workgroups(const fsnp_handle* h, const SbChunk& c) { return chunk_workgroups(pctx(h), c); }
// where a sub-band chunk's workgroups go; one per CU (owned or not: the least a launch that does not own its CUs is sure to get)
static CoopFootprint sb_chunk_footprint(const fsnp_handle* h, const SbChunk& c, bool own_cu) { return chunk_footprint(pctx(h), c, own_cu, 1); }
// Launches chunks [first, last) of the plan on stream s.  `bar` = per-tile arrival counters followed (at bar +
// plan.coop_tiles, 64-byte aligned by the caller) by the launch-abort word.
void launch_sb_lstm(const fsnp_handle* h, const SbPlan& plan, const LstmArgs& a, float* hx, unsigned* bar, unsigned* abort_word,
                    hipStream_t s, hipEvent_t after_first, int first_chunk, int last_chunk) {
    const size_t hx_floats_per_tile = lstm_coop_exchange_bytes(h->H, 1) / 4;
    const int nchunks = (int)plan.chunks.size();
    if (last_chunk < 0 || last_chunk > nchunks) last_chunk = nchunks;
    for (int ci = first_chunk; ci < last_chunk; ++ci) {
        const SbChunk& c = plan.chunks[ci];
        if (ci == first_chunk + 1 && after_first) { (void)hipEventRecord(after_first, s); after_first = nullptr; }
        LstmArgs ca = a;
        ca.rows = a.rows + c.slot0;
        ca.num_rows = c.nrows; ca.num_tiles = c.num_tiles; ca.ex = c.ex;
        if (a.md_row) ca.md_row = a.md_row + (size_t)c.slot0 * a.Tp;
        switch (c.kind) {
        case SbKind::RowTile: if (h->gru) launch_gru(h->lw, ca, s); else { ca.clk = h->d_clk; launch_lstm(h->lw, ca, s); } continue;
        case SbKind::HalfTile: launch_lstm16(h->lw, ca, s); continue;
        case SbKind::Generic: ca.coop_rows_per_group = c.rpg; launch_lstm_generic(h->lw, ca, false, s); continue;
        default: break;           // column split: below
        }
        ca.coop_hx = hx + (size_t)c.coop_tile0 * hx_floats_per_tile;
        ca.coop_bar = bar + (size_t)c.coop_tile0 * kCoopCounterStride;
        ca.coop_bar_stride = kCoopCounterStride;
        ca.coop_bar2 = nullptr;
        ca.coop_skew = h->coop_skew;
        ca.coop_chaos = h->coop_chaos;
        // pipelined loop: a deferred K-split chunk shares the chip with the next forward's full-band GEMMs; a GEMM workgroup that
        // lands on one of its CUs runs at ~0.6x (and each GEMM launch lasts as long as its slowest workgroup: stage 1.25 -> 1.85 ms),
        // so the chunk claims its CUs' whole LDS and the GEMM workgroups go to the other CUs
        // (never for a launch planned with two workgroups per CU: they would no longer be co-resident)
        ca.coop_own_cu = (h->side_stream && s == h->side_stream && chunk_workgroups(h, c) <= h->num_cus_real) ? kOwnCuLds : 0;
        ca.coop_err = h->d_err;
        ca.coop_abort = abort_word;
        ca.coop_units = c.units; ca.coop_groups = c.groups; ca.coop_rows_per_group = c.rpg;
        // XCD-local workgroup placement (lstm_common.h), unless the launch was planned with two workgroups per CU
        ca.coop_xcd = chunk_coop_xcd(pctx(h), c);
        const CoopFootprint fp = sb_chunk_footprint(h, c, ca.coop_own_cu > 0);
        launch_coop_chained(h->device, s, [&] {
            switch (c.kind) {
            case SbKind::HalfTilePingPong: (h->lw.hp_wave && lstm_hpw_available(h->lw) ? launch_lstm_hpw : launch_lstm_hp)(h->lw, ca, s); break;
            case SbKind::WaveOwned: launch_lstm_coopw(h->lw, ca, s); break;
            case SbKind::KSplit: launch_lstm_coop(h->lw, ca, s); break;
            default: launch_lstm_coopn(h->lw, ca, s); break;
            }
        }, h, &fp, h->num_cus_real / kNumXcds, h->coop_chain_stats);
    }
    if (after_first) (void)hipEventRecord(after_first, s);      // (a range of one chunk)
}
void take_coop_chain_stats(fsnp_handle* h, int64_t out[2], bool reset) {
    std::lock_guard<std::mutex> lk(g_coop_mu);
    out[0] = h->coop_chain_stats[0]; out[1] = h->coop_chain_stats[1];
    if (reset) h->coop_chain_stats[0] = h->coop_chain_stats[1] = 0;
}
// full-band LSTM of the original FullSubNet: B sequences, always the cooperative kernel (units in {8, 16, 32})
static int fb_row_tiles(int B) { return cdiv(B, 32); }
static int fb_coop_units(const fsnp_handle* h, int B) {
    const int u = lstm_coop_pick_units(h->CH, fb_row_tiles(B), h->num_cus_real, 8);
    return u > 32 ? 0 : u;
}

// Pipelined serving loop (fsnp_set_pipeline): which chunks of a plan go to the side stream (planner.cpp plan_first_deferred)
//   returns: first deferred chunk (== chunks.size(): nothing is deferred; 0: the whole plan)
int plan_first_deferred(const fsnp_handle* h, const SbPlan& plan) { return plan_first_deferred(pctx(h), plan, h->defer_small != 0); }
// which kernel runs the full-band LSTM of a `batch`-utterance FullSubNet forward, in what shape (fsnp_debug_fullband_launch)
FbShape fb_shape(const fsnp_handle* h, int batch) {
    if (h->generic_fb) {               // (runtime-sized kernel for a full-band model no K-split instantiation exists for: workgroups of rg sequences)
        const int rg = lstm_generic_rows_per_group(h->CH, h->F, batch, h->num_cus_real);
        return {FbKernel::Generic, rg > 0 ? cdiv(batch, rg) : 0, rg, 0};
    }
    if (h->fb_valu && lstm_fbv_available(h->fbw, batch, h->num_cus_real)) return {FbKernel::Valu, fb_row_tiles(batch), 32, 0};
    return {FbKernel::KSplitSeq, fb_row_tiles(batch), 32, fb_coop_units(h, batch)};
}
// the full-band LSTM launch of the original FullSubNet (lstm_coop_seq, never owns its CUs): round robin, at the occupancy measured at commit
static CoopFootprint fb_coop_footprint(const PlannerCtx& c, int CH, int batch, int fb_per_cu) {
    const int tiles = fb_row_tiles(batch), u = lstm_coop_pick_units(CH, tiles, c.num_cus_real, 8);      // (fb_coop_units)
    const bool ok = u > 0 && u <= 32;
    return coop_footprint_round_robin(ok ? tiles * (CH / u) : 0, false, ok ? fb_per_cu : 0);
}
static int fb_units_index(int units) { return units == 8 ? 0 : units == 16 ? 1 : 2; }
// The side-by-side decision of the pipelined FullSubNet loop at `batch` utterances (full mode): for every chunk of the plan that goes to
// the side stream, may the next forward's full-band LSTM run beside it?  Records of 9 ints (fsnp_debug.h: fsnp_debug_pipeline_pairing).
//   fb_per_cu: measured occupancy at 8 / 16 / 32 units per workgroup; fb_valu: the full-band LSTM runs on lstm_fbv instead (chained: B <= 4)
int pipeline_pairing(const PlannerCtx& c, bool defer_small, int F, int CH, int batch, const int fb_per_cu[3], bool fb_valu,
                     int32_t* out, int max_records) {
    const SbPlan plan = plan_sb(c, batch * F);
    const int first = plan_first_deferred(c, plan, defer_small), cpx = c.num_cus_real % kNumXcds == 0 ? c.num_cus_real / kNumXcds : 0;
    const int u = lstm_coop_pick_units(CH, fb_row_tiles(batch), c.num_cus_real, 8);
    const CoopFootprint fb = fb_valu ? coop_footprint_round_robin(0, false, 0) : fb_coop_footprint(c, CH, batch, fb_per_cu[fb_units_index(u)]);
    int fb_wgs = 0, fb_max = 0;
    for (int x = 0; x < kNumXcds; ++x) { fb_wgs += fb.per_xcd[x]; fb_max = std::max(fb_max, fb.per_xcd[x]); }
    int n = 0;
    for (int i = first; i < (int)plan.chunks.size() && n < max_records; ++i, ++n) {
        const SbChunk& k = plan.chunks[i];
        const CoopFootprint f = chunk_footprint(c, k, chunk_workgroups(c, k) <= c.num_cus_real, 1);    // (launch_sb_lstm: coop_own_cu)
        const int f_max = *std::max_element(f.per_xcd, f.per_xcd + kNumXcds);
        int32_t* o = out + 9 * n;
        o[0] = i; o[1] = (int)k.kind; o[2] = k.num_tiles; o[3] = chunk_workgroups(c, k); o[4] = f_max;
        o[5] = fb_wgs; o[6] = fb_max; o[7] = fb.per_cu; o[8] = fb_wgs > 0 && coop_side_by_side(f, fb, cpx) ? 1 : 0;
    }
    return n;
}

int rows_per_utt(const fsnp_handle* h, int mode) {
    return mode == FSNP_MODE_PARITY ? h->F / h->cfg.num_groups_in_drop_band : h->F;
}

// ragged: the forward takes per-utterance lengths (fsnp_forward_lengths): room for them behind everything else, so that every other
// offset, and the size of a forward without lengths, are what they are without it
static Workspace plan_workspace(const fsnp_handle* h, int B, int T, int mode, bool ragged = false) {
    Workspace w{};
    const size_t Tp = (size_t)T + h->cfg.look_ahead;
    const bool fsn = h->model == FSNP_MODEL_FULLSUBNET;
    const size_t nbr = fsn ? 1 : 3;
    const size_t xb = nbr * B * Tp * h->FP * 4;
    const size_t yb = nbr * B * Tp * align_up(h->CH, 4) * 4;
    size_t o = 0;
    auto take = [&](size_t bytes) { size_t r = o; o = align_up(o + bytes, 256); return r; };
    w.att = take(xb);                     // FullSubNet: the padded raw magnitude lives here (no attention stage)
    w.fb = take(xb);
    w.raw = take(fsn ? 0 : xb);
    w.x = take(fsn ? 0 : xb);
    w.y1 = take(yb);                      // FullSubNet: h1 sequence of the full-band LSTM [B][Tp][CH]
    w.y2 = take(fsn ? 0 : yb);
    w.gate = take(fsn ? 0 : (size_t)3 * B * h->FP * 4);
    w.md = take(nbr * B * Tp * sizeof(NormMD));
    w.md_utt = take((size_t)B * sizeof(NormMD));
    const SbPlan plan = plan_sb(h, B * rows_per_utt(h, mode), forward_gather_bytes(h, B, T));
    const size_t nrows_pad = (size_t)plan.total_slots;
    const bool cumulative = h->cfg.norm_type == FSNP_NORM_CUMULATIVE_LAPLACE || h->cfg.norm_type == FSNP_NORM_CUMULATIVE_LAYER;
    w.md_row = take(cumulative ? nrows_pad * Tp * sizeof(NormMD) : 0);
    w.rows = take(nrows_pad * sizeof(RowDesc));
    w.fb_rows = take(fsn ? (size_t)fb_row_tiles(B) * 32 * sizeof(RowDesc) : 0);
    w.frame = take(nbr * B * Tp * 2 * 8);
    const size_t sbt_x = h->sb_tcn ? nrows_pad * Tp * h->XS * 4 : 0, sbt_y = h->sb_tcn ? nrows_pad * Tp * h->CH * 4 : 0;
    w.sbt_x0 = take(sbt_x); w.sbt_x = take(sbt_x); w.sbt_fb = take(sbt_x); w.sbt_y1 = take(sbt_y); w.sbt_y2 = take(sbt_y);
    w.zero_begin = o;
    w.fsum = take(fsn ? 0 : (size_t)3 * B * h->FP * 8);
    w.fe_tot = take(fsn ? 0 : (size_t)3 * B * 2 * 8);
    w.gn = take(fsn ? 0 : (size_t)h->NB * 2 * 3 * B * kGnStride * 8);
    w.sb_acc = take((size_t)B * 2 * 8);
    w.coop_hx = take(lstm_coop_exchange_bytes(h->H, plan.coop_tiles));
    w.coop_bar = take(coop_counter_bytes(plan.coop_tiles));      // two arrival counters per row tile (+ the padded copies: lstm_common.h)
    w.coop_abort = take(256);             // [0] sub-band launches, [16] full-band LSTM (FullSubNet)
    w.fb_hx = take(fsn ? lstm_coop_exchange_bytes(h->CH, fb_row_tiles(B)) : 0);
    w.fb_bar = take(fsn ? (size_t)fb_row_tiles(B) * 4 : 0);
    w.sbt_gn = take(h->sb_tcn ? (size_t)8 * 2 * nrows_pad * kGnStride * 8 : 0);
    w.zero_end = o;
    w.dbg_tcn0 = take(h->debug ? (size_t)B * Tp * h->FP * 4 : 0);
    w.lens = take(ragged ? (size_t)2 * B * 4 : 0);
    w.total = o;
    return w;
}

// h->ws holds h->ws_slots (1, or 2 in pipelined mode) halves of h->ws_bytes each.  Growth is STREAM-ORDERED on the caller's
// stream (hipMallocAsync / hipFreeAsync from the device's default pool): no device-wide synchronisation, so a serving loop
// whose clip lengths vary never stalls other streams while it climbs to its high-water mark (fsnp_reserve jumps there at once).
// The old buffer is released behind everything that may still read it: earlier forwards on `s` (in order), their deferred
// chunks on the side stream (an event), forwards on another stream (forward_impl orders `s` behind them before it gets here).
int ensure_workspace(fsnp_handle* h, size_t bytes, hipStream_t s) {
    bytes = align_up(bytes, 4096);
    if (bytes <= h->ws_bytes) return 0;
    unsigned char* nw = nullptr;
    FSNP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&nw), bytes * h->ws_slots, s));
    // a fresh workspace is all zeros: tcn_gemm_dma_kernel DMAs the pad columns [K, lda) of its operand planes (they meet zero
    // weights, but NaN bit patterns left by an earlier owner of the memory would survive that); every kernel that writes a
    // plane writes its pad columns as zeros too, so this only matters for the very first use of a region
    FSNP_HIP_CHECK(hipMemsetAsync(nw, 0, bytes * h->ws_slots, s));
    if (h->ws) {
        for (int k = 0; k < 2; ++k)
            if (h->side_used[k]) FSNP_HIP_CHECK(hipStreamWaitEvent(s, h->ev_side[k], 0));
        FSNP_HIP_CHECK(hipFreeAsync(h->ws, s));
    }
    h->ws = nw;
    h->ws_bytes = bytes;
    h->side_used[0] = h->side_used[1] = false;     // `s` is ordered behind the side stream's work on the old buffer
    h->have_last = false;
    return 0;
}
// Orders `s` behind the last forward of this handle if that ran on ANOTHER stream (the workspace is shared by all of them)
int order_after_last_forward(fsnp_handle* h, hipStream_t s) {
    if (h->done_valid && h->done_stream != s) FSNP_HIP_CHECK(hipStreamWaitEvent(s, h->ev_done, 0));
    return 0;
}
int mark_forward_done(fsnp_handle* h, hipStream_t s) {
    if (!h->ev_done) FSNP_HIP_CHECK(hipEventCreateWithFlags(&h->ev_done, hipEventDisableTiming));
    FSNP_HIP_CHECK(hipEventRecord(h->ev_done, s));
    h->done_stream = s; h->done_valid = true;
    return 0;
}

// hipEvents for the per-forward timing records come from a pool; records that nobody reads are folded into the
// accumulators once 256 have piled up (they completed long ago), so timing never grows without bound.
int drain_timing(fsnp_handle* h) {
    for (auto& r : h->timing_recs) {
        float fb = 0, lstm = 0, all = 0, first = 0;
        // a forward that failed half way leaves events unrecorded: such a record is dropped, not counted
        const bool ok = hipEventSynchronize(r.e[2]) == hipSuccess && hipEventSynchronize(r.e[3]) == hipSuccess &&
                        hipEventElapsedTime(&fb, r.e[0], r.e[1]) == hipSuccess && hipEventElapsedTime(&lstm, r.e[1], r.e[2]) == hipSuccess &&
                        hipEventElapsedTime(&all, r.e[0], r.e[2]) == hipSuccess && hipEventElapsedTime(&first, r.e[1], r.e[3]) == hipSuccess;
        if (ok) {
            h->acc_ms[0] += lstm; h->acc_ms[1] += fb; h->acc_ms[2] += all; h->acc_ms[3] += first;
            for (int i = 0; i < 4; ++i) h->acc_cnt[i] += 1;
        } else {
            (void)hipGetLastError();
        }
        for (auto& e : r.e) h->event_pool.push_back(e);
    }
    h->timing_recs.clear();
    return 0;
}
static int take_timing_rec(fsnp_handle* h, TimingRec& rec) {
    if (h->timing_recs.size() >= 256 && drain_timing(h)) return 1;
    for (auto& e : rec.e) {
        if (!h->event_pool.empty()) { e = h->event_pool.back(); h->event_pool.pop_back(); }
        else FSNP_HIP_CHECK(hipEventCreate(&e));
    }
    return 0;
}



// The fused recurrent model + Linear on a dense input x [num_seq][steps][NIN] with a given plan (fsnp_lstm2_fc, calibration).
static int run_dense_plan(fsnp_handle* h, const SbPlan& plan, const float* x, float* out, int num_seq, int steps, hipStream_t s) {
    const int num_slots = plan.total_slots;
    const bool coop = plan.coop_tiles != 0;
    const size_t coop_off = align_up((size_t)num_slots * sizeof(RowDesc), 256);
    const size_t coop_hx_bytes = coop ? align_up(lstm_coop_exchange_bytes(h->H, plan.coop_tiles), 256) : 0;
    const size_t coop_bar_bytes = align_up(coop_counter_bytes(plan.coop_tiles), 256);
    const size_t coop_bytes = coop ? coop_hx_bytes + coop_bar_bytes + 256 : 0;       // images, counters, abort word
    if (order_after_last_forward(h, s)) return 4;
    if (ensure_workspace(h, coop_off + coop_bytes, s)) return 4;
    if (h->pipeline && h->side_stream) FSNP_HIP_CHECK(hipStreamSynchronize(h->side_stream));   // slot 0 may still be read
    RowDesc* rows = reinterpret_cast<RowDesc*>(h->ws);
    h->have_last = false;   // the workspace no longer holds a forward's stages
    if (coop) FSNP_HIP_CHECK(hipMemsetAsync(h->ws + coop_off, 0, coop_bytes, s));
    launch_build_rows(plan, rows, dense_rows(steps, h->cfg.output_size), s);
    LstmArgs a{};
    a.rows = rows; a.dense = x; a.dense_stride = h->NIN; a.out = out; a.out_stride_o = steps;
    a.num_rows = num_seq; a.Tp = steps; a.LA = 0; a.FP = 0; a.F = 1; a.NSBN = 0; a.act = h->cfg.sb_act;
    launch_sb_lstm(h, plan, a, reinterpret_cast<float*>(h->ws + coop_off),
                   reinterpret_cast<unsigned*>(h->ws + coop_off + coop_hx_bytes),
                   reinterpret_cast<unsigned*>(h->ws + coop_off + coop_hx_bytes + coop_bar_bytes), s);
    FSNP_HIP_CHECK(hipGetLastError());
    return mark_forward_done(h, s);
}

// ---- calibration of the planner's cost table: once per process and (device, cell, sizes), on the first call that plans.
// Every launch shape the planner can pick is run on zeros at two step counts; the per-step cost is the slope (launch and
// prologue cancel).  ~0.1 s and ~60 MB of scratch, then cached for every later handle of the same kind.  FSNP_CALIBRATE=0
// keeps the built-in table (the round-1 measurements).
struct CalKey {
    int dev, H, KX, gru, occ, cus;
    bool operator<(const CalKey& o) const {
        const int a[6] = {dev, H, KX, gru, occ, cus}, b[6] = {o.dev, o.H, o.KX, o.gru, o.occ, o.cus};
        for (int i = 0; i < 6; ++i) if (a[i] != b[i]) return a[i] < b[i];
        return false;
    }
};
static std::mutex g_cal_mu;
static std::map<CalKey, CostTable> g_cal_cache;

int calibrate_costs(fsnp_handle* h, bool adopt, CostTable* measured) {
    if (adopt && (h->planner.cost.calibrated || !h->calibrate)) return 0;
    if (h->sb_tcn || h->generic_sb || !h->committed) return 0;
    int occ_sig = h->planner.coop_occ;
    for (int i = 0; i < 4; ++i) occ_sig = occ_sig * 4 + h->planner.occ_ksplit[i];
    for (int i = 0; i < 2; ++i) occ_sig = occ_sig * 4 + h->planner.occ_coopn[i];
    occ_sig = occ_sig * 2 + h->coop_skew;
    const CalKey key{h->device, h->H, h->KX, h->gru, occ_sig, h->num_cus_real};
    {
        std::lock_guard<std::mutex> lk(g_cal_mu);
        auto it = g_cal_cache.find(key);
        if (it != g_cal_cache.end()) {
            if (measured) *measured = it->second;
            if (adopt) h->planner.cost = it->second;
            return 0;
        }
    }
    // the timing launches overwrite the handle's workspace from a private stream: nothing of an earlier forward may still be
    // in flight on the caller's streams (ensure_workspace only synchronises when it grows)
    FSNP_HIP_CHECK(hipDeviceSynchronize());
    const int S3 = h->H / 128, occ = h->planner.coop_occ >= 2 ? 2 : 1;
    const int steps_a = 8, steps_b = 40;
    const int max_tiles = std::max(h->num_cus_real, (h->num_cus_real * occ / S3) * 2);
    const size_t x_floats = (size_t)max_tiles * 32 * steps_b * h->NIN, o_floats = (size_t)max_tiles * 32 * 2 * steps_b;
    float* scratch = nullptr;
    hipStream_t cs = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    FSNP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&scratch), (x_floats + o_floats) * 4));
    int rc = 0;
    auto cleanup = [&] {
        if (cs) { (void)hipStreamSynchronize(cs); (void)hipStreamDestroy(cs); }
        if (e0) (void)hipEventDestroy(e0);
        if (e1) (void)hipEventDestroy(e1);
        (void)hipFree(scratch);
    };
#define FSNP_CAL_CHECK(expr) do { if ((expr) != hipSuccess) { set_error("calibration: %s failed", #expr); cleanup(); return 4; } } while (0)
    FSNP_CAL_CHECK(hipStreamCreateWithFlags(&cs, hipStreamNonBlocking));
    FSNP_CAL_CHECK(hipEventCreate(&e0));
    FSNP_CAL_CHECK(hipEventCreate(&e1));
    FSNP_CAL_CHECK(hipMemsetAsync(scratch, 0, (x_floats + o_floats) * 4, cs));
    CostTable t = h->planner.cost;
    if (h->planner.rowtile_ok) {            // ramp the clocks: short launches on an idle chip run at a lower power state than a forward does
        SbPlan warm;
        warm.chunks = {row_tile_chunk(0, h->num_cus_real * 32, h->num_cus_real)};
        warm.total_slots = h->num_cus_real * 32;
        for (int k = 0; k < 2; ++k)         // (the scratch buffers hold steps_b steps of max_tiles tiles: stay inside them)
            (void)run_dense_plan(h, warm, scratch, scratch + x_floats, h->num_cus_real * 32, steps_b, cs);
    }
    // one shape: returns its per-step cost in microseconds (< 0 on failure)
    auto time_shape = [&](SbChunk c) -> double {
        c.row0 = 0; c.nrows = c.num_tiles * c.rps; c.slot0 = 0; c.coop_tile0 = 0;
        SbPlan plan;
        plan.chunks = {c}; plan.total_slots = c.num_tiles * c.rps; plan.coop_tiles = is_column_split(c.kind) ? c.num_tiles : 0;
        double ms[2] = {0, 0};
        for (int k = 0; k < 2; ++k) {
            const int steps = k == 0 ? steps_a : steps_b;
            double best = 1e30;
            for (int rep = 0; rep < 3; ++rep) {            // rep 0 warms caches / code / clocks; the faster of reps 1, 2 counts
                if (hipEventRecord(e0, cs) != hipSuccess) return -1.0;
                if (run_dense_plan(h, plan, scratch, scratch + x_floats, c.nrows, steps, cs)) return -1.0;
                if (hipEventRecord(e1, cs) != hipSuccess || hipEventSynchronize(e1) != hipSuccess) return -1.0;
                float f = 0;
                if (hipEventElapsedTime(&f, e0, e1) != hipSuccess) return -1.0;
                if (rep > 0 && f < best) best = f;
            }
            ms[k] = best;
        }
        return (ms[1] - ms[0]) * 1000.0 / (steps_b - steps_a);
    };
    for (int o = 0; o < occ && rc == 0; ++o) {
        const int slots = h->num_cus_real * (o + 1);
        for (int ui = 0; ui < 4 && rc == 0; ++ui) {
            const int u = 8 << ui, S = h->H / u;
            int tiles = slots / S;
            if (o == 1 && (tiles * S <= h->num_cus_real || h->planner.occ_ksplit[ui] < 2)) continue;   // never planned two per CU
            if (tiles <= 0) continue;
            const double us = time_shape(column_chunk(SbKind::KSplit, 0, 0, tiles, u, 0));
            if (us < 0) rc = 4; else t.ksplit[ui][o] = us;
            if (o == 0 && rc == 0) {
                const double u1 = tiles > 1 ? time_shape(column_chunk(SbKind::KSplit, 0, 0, 1, u, 0)) : us;
                if (u1 < 0) rc = 4; else t.ksplit1[ui] = u1 < us ? u1 : us;
            }
        }
        for (int rpg = 1; rpg <= 2 && rc == 0; ++rpg) {
            const int groups = slots / S3;
            if (groups <= 0 || (o == 1 && h->planner.occ_coopn[rpg - 1] < 2)) continue;
            const double us = time_shape(column_chunk(SbKind::ThreeWay, 0, 0, groups * rpg, 0, rpg));
            if (us < 0) rc = 4; else t.coopn[rpg - 1][o] = us;
        }
    }
    if (rc == 0 && h->planner.rowtile_ok) {
        const double us0 = time_shape(row_tile_chunk(0, 0, h->num_cus_real));
        if (us0 < 0) rc = 4;
        else t.rowtile = us0;           // the VALU-row surcharge keeps its measured ratio (0.11 per row)
    }
    if (rc == 0 && h->planner.hp_ok && h->num_cus_real / (h->H / 16) > 0) {
        const int cap = h->num_cus_real / (h->H / 16);
        const double u1 = time_shape(column_chunk(SbKind::HalfTilePingPong, 0, 0, 1, 16, 0)), uf = time_shape(column_chunk(SbKind::HalfTilePingPong, 0, 0, cap, 16, 0));
        if (u1 < 0 || uf < 0) rc = 4; else { t.hp[0] = u1; t.hp[1] = uf; }
    }
    for (int nt = 1; nt <= 3 && rc == 0 && h->planner.coopw_ok; ++nt) {
        const int u = 32 * nt, cap = h->num_cus_real / (h->H / u);
        if (cap <= 0) continue;
        const double u1 = time_shape(column_chunk(SbKind::WaveOwned, 0, 0, 1, u, 0)), uf = cap > 1 ? time_shape(column_chunk(SbKind::WaveOwned, 0, 0, cap, u, 0)) : u1;
        if (u1 < 0 || uf < 0) rc = 4; else { t.coopw[nt - 1][0] = u1; t.coopw[nt - 1][1] = uf; }
    }
    if (rc == 0 && h->planner.lstm16_ok) {
        const double us16 = time_shape(half_tile_chunk(0, 0, h->num_cus_real));
        if (us16 < 0) rc = 4; else t.rowtile16 = us16;
    }
    cleanup();
#undef FSNP_CAL_CHECK
    if (rc) { if (g_last_error.empty()) set_error("calibration of the sub-band planner failed"); return rc; }
    if ((*reinterpret_cast<volatile unsigned*>(h->d_err) & kErrTimeout) != 0) {
        // a calibration launch gave up (its workgroups were not all resident): never plan two workgroups per CU
        *reinterpret_cast<volatile unsigned*>(h->d_err) &= ~kErrTimeout;
        t = default_costs();
        h->planner.coop_occ = 1;
    }
    t.calibrated = 1;
    if (measured) *measured = t;
    if (adopt) h->planner.cost = t;
    std::lock_guard<std::mutex> lk(g_cal_mu);
    g_cal_cache[key] = t;
    return 0;
}

}  // namespace fsnp

extern "C" {

const char* fsnp_last_error(void) { return g_last_error.c_str(); }
const char* fsnp_version(void) { return "fsnp-hip 0.2 (gfx950)"; }
int32_t fsnp_abi_version(void) { return FSNP_ABI_VERSION; }
int32_t fsnp_config_size(void) { return (int32_t)sizeof(fsnp_config); }

int fsnp_create(const fsnp_config* cfg, fsnp_handle** out) {
    if (!cfg || !out) { set_error("fsnp_create: null argument"); return 1; }
    *out = nullptr;
    if (cfg->num_freqs < 2) { set_error("num_freqs must be >= 2"); return 2; }
    if (cfg->look_ahead < 0) { set_error("look_ahead must be >= 0"); return 2; }
    if (cfg->sb_num_neighbors < 0 || cfg->fb_num_neighbors < 0) { set_error("sb_num_neighbors / fb_num_neighbors must be >= 0"); return 2; }
    if (cfg->num_groups_in_drop_band < 1) { set_error("num_groups_in_drop_band must be >= 1"); return 2; }
    // output_size is a constructor argument of the reference (fullsubnet_plus.py:30,104,206: the sub-band model's Linear(H, output_size)
    // and the final reshape); every configuration file uses 2 (the cIRM) and the tuned kernels fuse exactly that Linear(H, 2).  Other
    // values run the sub-band recurrence on the runtime-sized kernel (lstm_generic.hip: OUT is a run-time argument there).
    if (cfg->output_size < 1 || cfg->output_size > 64) { set_error("output_size must be in [1, 64]"); return 2; }
    if (cfg->model == FSNP_MODEL_FULLSUBNET && cfg->output_size != 2) { set_error("FullSubNet has no output_size argument (fullsubnet.py:13-26): 2"); return 2; }
    if (cfg->sb_hidden < 1 && cfg->sequence_model != FSNP_SEQ_TCN) { set_error("sb_model_hidden_size must be >= 1"); return 2; }
    if (cfg->num_tcn_blocks < 0 || cfg->num_tcn_blocks > 8) { set_error("num_tcn_blocks must be in [0,8]"); return 2; }
    if (cfg->model != FSNP_MODEL_FULLSUBNET && cfg->tcn_hidden % 64 != 0) { set_error("tcn_hidden must be a multiple of 64"); return 2; }      // (TCN GEMM tiles; the reference hard-codes 512)
    if (cfg->norm_type < 0 || cfg->norm_type > 3) { set_error("unknown norm_type %d", cfg->norm_type); return 2; }
    if (cfg->attention < 0 || cfg->attention > 3) { set_error("unknown attention model %d", cfg->attention); return 2; }
    if (cfg->model != FSNP_MODEL_FULLSUBNET_PLUS && cfg->model != FSNP_MODEL_FULLSUBNET) { set_error("unknown model %d", cfg->model); return 2; }
    if (cfg->sequence_model < FSNP_SEQ_LSTM || cfg->sequence_model > FSNP_SEQ_TCN) { set_error("unknown sequence_model %d", cfg->sequence_model); return 2; }
    const bool fsn = cfg->model == FSNP_MODEL_FULLSUBNET;
    const int subband_num = cfg->subband_num > 0 ? cfg->subband_num : 1;
    if (cfg->subband_num < 0) { set_error("subband_num must be >= 1"); return 2; }
    if (subband_num > 1 && (fsn || cfg->attention != FSNP_ATT_ECA)) {
        set_error("subband_num > 1 needs channel_attention_model = ECA (the reference's other attention layers fail on it: "
                  "fullsubnet_plus.py:47-50,155-163)");
        return 2;
    }
    if (subband_num > 1 && subband_num - cfg->num_freqs % subband_num >= cfg->num_freqs) { set_error("subband_num too large for num_freqs (reflect pad)"); return 2; }
    if (fsn && cfg->sequence_model == FSNP_SEQ_TCN) { set_error("FullSubNet only supports GRU and LSTM"); return 2; }
    if (fsn && cfg->tcn_hidden < 1) { set_error("fb_model_hidden_size must be >= 1"); return 2; }
    const int nin = 2 * cfg->sb_num_neighbors + 1 + (fsn ? 1 : 3) * (2 * cfg->fb_num_neighbors + 1);
    // sizes without a tuned (MFMA) instantiation run on the runtime-sized kernel (lstm_generic.hip) - as long as one sequence's
    // state fits a CU's LDS
    const bool generic_sb = cfg->sequence_model != FSNP_SEQ_TCN && ((cfg->sb_hidden != 384 && cfg->sb_hidden != 256 && cfg->sb_hidden != 512) || nin > 64 || cfg->output_size != 2);
    if (cfg->sequence_model == FSNP_SEQ_TCN && cfg->output_size > nin) {      // the sub-band TCN's final Linear runs as an nin-column GEMM
        set_error("sequence_model=TCN: output_size %d exceeds the sub-band input width %d (not supported)", cfg->output_size, nin);
        return 2;
    }
    const bool generic_fb = fsn && (cfg->tcn_hidden != 512 || cfg->num_freqs > 264);
    if (generic_sb && lstm_generic_rows_per_group(cfg->sb_hidden, nin, 1, 1) == 0) { set_error("sb_model_hidden_size %d is too large for the runtime-sized kernel (LDS)", cfg->sb_hidden); return 2; }
    if (generic_fb && lstm_generic_rows_per_group(cfg->tcn_hidden, cfg->num_freqs, 1, 1) == 0) { set_error("fb_model_hidden_size %d is too large for the runtime-sized kernel (LDS)", cfg->tcn_hidden); return 2; }
    if (cfg->num_freqs <= cfg->sb_num_neighbors || cfg->num_freqs <= cfg->fb_num_neighbors) { set_error("num_freqs must exceed the neighbour counts (reflect pad)"); return 2; }
    for (int c = 0; c < 3; ++c)
        if (cfg->kersize[c] < 1 || cfg->kersize[c] > 16) { set_error("kersize must be in [1,16]"); return 2; }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
        set_error("no HIP device visible: libfsnp_hip needs an MI355X (gfx950); there is no CPU fallback");
        return 3;
    }
    int dev = 0;
    FSNP_HIP_CHECK(hipGetDevice(&dev));
    hipDeviceProp_t prop;
    FSNP_HIP_CHECK(hipGetDeviceProperties(&prop, dev));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
        set_error("device %d is %s; libfsnp_hip is built for gfx950 only", dev, prop.gcnArchName);
        return 3;
    }
    fsnp_handle* h = new fsnp_handle();
    h->cfg = *cfg;
    h->device = dev;
    h->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    h->num_cus_real = h->num_cus;
    h->generic_sb = generic_sb;
    h->generic_fb = generic_fb;
    if (cfg->sequence_model != FSNP_SEQ_TCN && !generic_sb && h->num_cus_real < cfg->sb_hidden / 8) {
        // the column-split kernels need at least one group of workgroups resident (GRU has no other kernel)
        set_error("device %d exposes %d compute units; the sub-band recurrent kernels need at least %d", dev, h->num_cus_real, cfg->sb_hidden / 8);
        delete h;
        return 3;
    }
    h->model = cfg->model;
    h->gru = cfg->sequence_model == FSNP_SEQ_GRU;
    {
        auto env_is = [](const char* e, char c) { return e && e[0] == c; };
        PlannerSwitches sw;                                    // each: "=0" never plans that kernel; FSNP_COOP_OCC=1: one workgroup per CU
        sw.lstm16 = !env_is(getenv("FSNP_LSTM16"), '0');       // half tiles (lstm16.hip)
        sw.lstm_coop = env_is(getenv("FSNP_LSTM_COOP"), '0') ? 0 : 1;   // column split (where a row-tile kernel exists)
        sw.coop_hp = env_is(getenv("FSNP_COOP_HP"), '0') ? 0 : 1;       // half-tile ping-pong (else: wherever the cost table says it pays)
        sw.coop_w = env_is(getenv("FSNP_COOP_W"), '0') ? 0 : 1;         // wave-owned column split (lstm_coopw.hip)
        sw.coop_occ = env_is(getenv("FSNP_COOP_OCC"), '1') ? 1 : 2;     // (2 is checked against the kernels' occupancy at commit time)
        h->planner = planner_options(cfg->sequence_model, cfg->sb_hidden, nin, generic_sb, sw);
        h->coop_hp_cfg = h->planner.coop_hp;
        h->hp_wave = env_is(getenv("FSNP_HP_WAVE"), '0') ? 0 : 1;       // 0: HalfTilePingPong launches on lstm_hp.hip instead of lstm_hpw.hip
        h->calibrate = env_is(getenv("FSNP_CALIBRATE"), '1') ? 1 : 0;
    }
    h->planner.cost = initial_costs(cfg->sb_hidden, h->gru, cfg->sequence_model == FSNP_SEQ_TCN);
    h->sb_tcn = cfg->sequence_model == FSNP_SEQ_TCN;
    h->XS = (int)align_up(nin, 4);
    h->NG = h->gru ? 3 : 4;
    h->NFB = fsn ? 1 : 3;
    h->F = cfg->num_freqs;
    h->FP = (int)align_up(cfg->num_freqs, 4);
    h->CH = cfg->tcn_hidden;
    h->H = cfg->sb_hidden;
    h->NSB = 2 * cfg->sb_num_neighbors + 1;
    h->NIN = nin;
    h->KX = nin <= 40 ? 40 : 64;       // input width the recurrent kernels are instantiated for (zero-padded K)
    h->NB = fsn ? 0 : cfg->num_tcn_blocks;
    h->Fr = cfg->num_freqs / 2;
    build_specs(h);
    {
        const char* ve = getenv("FSNP_VERIFY_EVERY");      // N > 0: fsnp_set_verify(h, N) from the start (models with an exchange-free kernel)
        if (ve && atoi(ve) > 0 && h->planner.rowtile_ok && !generic_sb && cfg->sequence_model != FSNP_SEQ_TCN) h->verify_every = atoi(ve);
    }
    const char* sk = getenv("FSNP_COOP_SKEW");
    if (sk && sk[0] == '0') h->coop_skew = 0;
    if (hipHostMalloc(reinterpret_cast<void**>(&h->d_err), 256, hipHostMallocMapped) != hipSuccess) {
        set_error("hipHostMalloc of the error word failed");
        delete h;
        return 4;
    }
    memset(h->d_err, 0, 256);
    if (hipMalloc(reinterpret_cast<void**>(&h->d_clk), 64) != hipSuccess || hipMemset(h->d_clk, 0, 64) != hipSuccess) {
        set_error("hipMalloc of the clock stamps failed");
        (void)hipHostFree(h->d_err);
        delete h;
        return 4;
    }
    const char* dbg = getenv("FSNP_DEBUG_STAGES");
    h->debug = dbg && dbg[0] == '1';
    *out = h;
    return 0;
}

void fsnp_destroy(fsnp_handle* h) {
    if (!h) return;
    fsnp::DeviceGuard guard(h->device);
    (void)hipDeviceSynchronize();
    if (h->ws) (void)hipFreeAsync(h->ws, nullptr);        // (allocated from the stream-ordered pool; the device is idle here)
    if (h->io) (void)hipFreeAsync(h->io, nullptr);
    for (auto& r : h->resample) if (r.dev) (void)hipFreeAsync(r.dev, nullptr);      // (include/fsnp_resample.h: the pairs' tap tables)
    if (h->win_stage) (void)hipFreeAsync(h->win_stage, nullptr);                    // (include/ext/fsnp_windowed.h)
    for (auto& f : h->win_fades) if (f.dev) (void)hipFreeAsync(f.dev, nullptr);
    (void)hipDeviceSynchronize();
    if (h->ev_done) (void)hipEventDestroy(h->ev_done);
    if (h->d_stft) (void)hipFree(h->d_stft);
    if (h->d_weights) (void)hipFree(h->d_weights);
    if (h->d_arena) (void)hipFree(h->d_arena);
    if (h->ev_packed) (void)hipEventDestroy(h->ev_packed);
    if (h->ev_arena) (void)hipEventDestroy(h->ev_arena);
    drop_weight_watch(h);
    if (h->verify_out) (void)hipFree(h->verify_out);
    if (h->verify_key) (void)hipFree(h->verify_key);
    if (h->d_clk) (void)hipFree(h->d_clk);
    if (h->vs_buf) (void)hipFree(h->vs_buf);
    if (h->vs_stream) (void)hipStreamDestroy(h->vs_stream);
    if (h->ev_vs_snap) (void)hipEventDestroy(h->ev_vs_snap);
    if (h->ev_vs_done) (void)hipEventDestroy(h->ev_vs_done);
    if (h->d_err) (void)hipHostFree(h->d_err);
    for (auto& r : h->timing_recs)
        for (auto& e : r.e) (void)hipEventDestroy(e);
    for (auto& e : h->event_pool) (void)hipEventDestroy(e);
    if (h->side_stream) (void)hipStreamDestroy(h->side_stream);
    if (h->ev_main) (void)hipEventDestroy(h->ev_main);
    for (auto& e : h->ev_side) if (e) (void)hipEventDestroy(e);
    delete h;
}

size_t fsnp_workspace_bytes(const fsnp_handle* h, int32_t batch, int32_t frames, int32_t mode) {
    if (!h || batch <= 0 || frames <= 0) return 0;
    return plan_workspace(h, batch, frames, mode).total;
}

// ---- the forward, as a list of steps over one Forward

// every refusal of a forward, in this order; fills d.  Nothing is launched.
static int check_forward_args(fsnp_handle* h, const float* mag, const float* real, const float* imag, bool is_complex, const int64_t strides[3][3],
                              const float* out, int batch, int frames, int mode, int batch_offset, int global_batch, const int32_t* lengths,
                              Dims& d) {
    if (batch <= 0 || frames <= 0) { set_error("fsnp_forward: empty input (B=%d, T=%d)", batch, frames); return 2; }
    if (!h || !mag || !out || !strides) { set_error("fsnp_forward: null argument"); return 1; }
    const bool fsn = h->model == FSNP_MODEL_FULLSUBNET;
    if (!fsn && !is_complex && (!real || !imag)) { set_error("fsnp_forward: null argument (FullSubNet+ takes mag, real and imag)"); return 1; }
    if (!h->committed) { set_error("fsnp_forward: weights not committed (call fsnp_commit_weights)"); return 2; }
    if (const int ec = take_device_errors(h, "an earlier forward on this handle failed")) return ec;     // set by a launch that has finished since
    if (mode != FSNP_MODE_FULL && mode != FSNP_MODE_PARITY) { set_error("unknown mode %d", mode); return 2; }
    if (mode == FSNP_MODE_PARITY && (h->cfg.num_groups_in_drop_band < 2 || global_batch <= h->cfg.num_groups_in_drop_band)) {
        set_error("PARITY mode needs num_groups_in_drop_band >= 2 and a global batch larger than it (feature.py:263)");
        return 2;
    }
    if (batch_offset < 0 || global_batch < batch_offset + batch) { set_error("bad batch_offset/global_batch"); return 2; }
    d.B = batch; d.T = frames; d.LA = h->cfg.look_ahead; d.Tp = frames + d.LA; d.F = h->F; d.FP = h->FP;
    d.CH = h->CH; d.H = h->H; d.NSB = h->NSB; d.NIN = h->NIN;
    const int kmax = tsse_largest_kernel(h);
    if (d.Tp < kmax) { set_error("too few frames: T + look_ahead = %d < largest TSSE kernel %d", d.Tp, kmax); return 2; }
    if ((double)3 * d.B * d.Tp * d.FP * 2 > 2.0e9) { set_error("batch too large for 32-bit gather offsets; split the batch"); return 2; }
    if (lengths) {
        if (mode != FSNP_MODE_FULL) { set_error("fsnp_forward_lengths: per-utterance lengths need FULL mode"); return 2; }
        if (const int rc = check_lengths(h, lengths, batch, frames, "fsnp_forward_lengths")) return rc;
    }
    if (fsn && !h->generic_fb && fb_coop_units(h, batch) == 0) { set_error("FullSubNet: at most %d utterances per call (full-band LSTM residency); split the batch", 32 * (h->num_cus_real / 16)); return 2; }
    return 0;
}

// one forward: its stream, plan, workspace half and the buffers its steps share
struct Forward {
    fsnp_handle* h; hipStream_t s; Dims d; int mode, batch_offset, global_batch;
    SbPlan plan; Workspace w; int slot; unsigned char* base; RowDesc* rows; SubbandBuffers sbuf; TimingRec rec;
    float* fptr(size_t off) const { return reinterpret_cast<float*>(base + off); }
};

// orders the forward behind everything that used its workspace half, and starts its timing record
static int bind_workspace(Forward& f, bool ragged) {
    fsnp_handle* h = f.h;
    f.w = plan_workspace(h, f.d.B, f.d.T, f.mode, ragged);
    if (order_after_last_forward(h, f.s)) return 4;
    if (ensure_workspace(h, f.w.total, f.s)) return 4;
    // pipelined mode: alternate between the two workspace halves; the half about to be rebuilt was last read by the
    // deferred remainder chunks of the forward before the previous one
    f.slot = h->pipeline ? h->ws_slot : 0;
    if (h->pipeline) {
        h->ws_slot ^= 1;
        if (h->side_used[f.slot]) FSNP_HIP_CHECK(hipStreamWaitEvent(f.s, h->ev_side[f.slot], 0));
    }
    f.base = h->ws + (size_t)f.slot * h->ws_bytes;
    if (h->timing) {
        if (take_timing_rec(h, f.rec)) return 4;
        h->timing_recs.push_back(f.rec);        // owned by the handle from here on (no leak on an early return)
        FSNP_HIP_CHECK(hipEventRecord(f.rec.e[0], f.s));
    }
    f.rows = reinterpret_cast<RowDesc*>(f.base + f.w.rows);
    const bool cumulative = h->cfg.norm_type == FSNP_NORM_CUMULATIVE_LAPLACE || h->cfg.norm_type == FSNP_NORM_CUMULATIVE_LAYER;
    SubbandBuffers& sbuf = f.sbuf;
    sbuf.att_mag = f.fptr(f.w.att); sbuf.fb = f.fptr(f.w.fb); sbuf.refl_w = h->d_refl_w; sbuf.refl_wfb = h->d_refl_wfb;
    sbuf.NFBN = h->cfg.fb_num_neighbors;
    sbuf.acc = reinterpret_cast<double*>(f.base + f.w.sb_acc);
    sbuf.md_utt = reinterpret_cast<NormMD*>(f.base + f.w.md_utt);
    sbuf.md_row = cumulative ? reinterpret_cast<NormMD*>(f.base + f.w.md_row) : nullptr;
    return 0;
}

// the prologue of both models, one launch: zero the accumulators / exchange images / counters, describe the sub-band rows, and
// - fsnp_watch_weights - fingerprint the caller's source tensors (a .data edit since the pack flags the handle)
static int launch_prologue(Forward& f) {
    fsnp_handle* h = f.h;
    const bool watch = h->watch_nseg > 0 && (h->watch_calls++ % h->watch_every) == 0;
    const RowLayout l{h->F, f.d.T, f.mode, f.batch_offset, f.global_batch, 0, h->cfg.num_groups_in_drop_band, h->cfg.output_size};
    if ((int)f.plan.chunks.size() > kPrologueChunks) {      // (more chunks than the argument block holds: the separate kernels)
        launch_zero_region(f.base + f.w.zero_begin, f.w.zero_end - f.w.zero_begin, f.s);
        launch_build_rows(f.plan, f.rows, l, f.s);
        return watch ? launch_weight_watch(h, f.s, false) : 0;
    }
    launch_prologue_kernel(h, f.plan, f.rows, l, f.base + f.w.zero_begin, f.w.zero_end - f.w.zero_begin, watch, f.s);
    return 0;
}

// FullSubNet+: the three attention branches and the full-band TCN stacks
static void run_fullband_plus(Forward& f, const float* const in[3], const int64_t strides[3][3], bool is_complex) {
    fsnp_handle* h = f.h;
    const Workspace& w = f.w;
    FrontendBuffers fbuf;
    fbuf.raw = f.fptr(w.raw); fbuf.frame = reinterpret_cast<double*>(f.base + w.frame);
    fbuf.md = reinterpret_cast<NormMD*>(f.base + w.md); fbuf.fsum = reinterpret_cast<double*>(f.base + w.fsum);
    fbuf.tot = reinterpret_cast<double*>(f.base + w.fe_tot);
    fbuf.gate = f.fptr(w.gate); fbuf.att = f.fptr(w.att);
    TcnBuffers tbuf;
    tbuf.att = f.fptr(w.att); tbuf.x = f.fptr(w.x); tbuf.y1 = f.fptr(w.y1); tbuf.y2 = f.fptr(w.y2);
    tbuf.gn = reinterpret_cast<double*>(f.base + w.gn); tbuf.fb = f.fptr(w.fb);
    tbuf.dbg_tcn0 = h->debug ? f.fptr(w.dbg_tcn0) : nullptr;
    // the caller's tensors are read by the repack kernel only; everything up to the LSTM then stays in the workspace
    launch_frontend(f.d, h->cfg.norm_type, in, strides, is_complex, h->fw, fbuf, f.s);
    launch_tcn(f.d, h->cfg.fb_act, h->tw, tbuf, f.s);
}

// FullSubNet (fullsubnet.py:82-90): pad, norm(noisy_mag), 2-layer LSTM(F -> CH), Linear(CH, F) + fb_act
static void run_fullband_fullsubnet(Forward& f, const float* mag, const int64_t strides[3], bool is_complex) {
    fsnp_handle* h = f.h;
    const Workspace& w = f.w;
    const Dims& d = f.d;
    hipStream_t s = f.s;
    FrontendBuffers fbuf{};
    fbuf.raw = f.fptr(w.att); fbuf.frame = reinterpret_cast<double*>(f.base + w.frame);
    fbuf.md = reinterpret_cast<NormMD*>(f.base + w.md);
    launch_frontend_mag(d, h->cfg.norm_type, mag, strides, is_complex, fbuf, s);
    const FbShape fbs = fb_shape(h, d.B);
    RowDesc* fb_rows = reinterpret_cast<RowDesc*>(f.base + w.fb_rows);
    launch_build_rows(fb_rows, {d.B, fbs.tiles, fbs.rows_per_tile, 0}, dense_rows(d.T, 2), s);
    LstmArgs fa{};
    fa.rows = fb_rows; fa.dense = f.fptr(w.att); fa.dense_stride = d.FP; fa.md_seq = fbuf.md;
    fa.seq_out = f.fptr(w.y1);
    fa.num_rows = d.B; fa.num_tiles = fbs.tiles; fa.Tp = d.Tp; fa.LA = 0; fa.FP = d.FP; fa.F = d.F;
    fa.coop_hx = f.fptr(w.fb_hx); fa.coop_bar = reinterpret_cast<unsigned*>(f.base + w.fb_bar); fa.coop_err = h->d_err;
    fa.coop_abort = reinterpret_cast<unsigned*>(f.base + w.coop_abort) + 16;
    fa.coop_units = h->generic_fb ? 0 : fb_coop_units(h, d.B); fa.coop_chaos = h->coop_chaos;
    const int chp = (int)align_up(d.CH, 4);           // row stride of the h1 sequence (a float4 multiple; pad columns written as zeros)
    fa.seq_stride = chp;
    switch (fbs.kernel) {
    case FbKernel::Generic: fa.coop_rows_per_group = fbs.rows_per_tile; launch_lstm_generic(h->fbw, fa, true, s); break;
    case FbKernel::Valu: launch_coop_chained(h->device, s, [&] { launch_lstm_fbv(h->fbw, fa, s); }); break;      // B <= 4
    case FbKernel::KSplitSeq: {
        const CoopFootprint fp = fb_coop_footprint(pctx(h), h->CH, d.B, h->occ_fb[fb_units_index(fa.coop_units)]);
        launch_coop_chained(h->device, s, [&] { launch_lstm_coop_seq(h->fbw, fa, s); }, h, &fp, h->num_cus_real / kNumXcds, h->coop_chain_stats);
        break;
    }
    }
    launch_linear_act(f.fptr(w.y1), chp, h->fsn_wf, h->fsn_kp, h->fsn_bf, f.fptr(w.fb), d.FP, d.CH, d.F, d.B, d.Tp, h->cfg.fb_act, h->num_cus, s);
}

// sequence_model="TCN": materialise the normalised sub-band input, run the TCN stack over the sub-band sequences
// (one "utterance" per sequence: GroupNorm(1, 512) statistics are per sequence), Linear(34, 2), scatter
static int run_subband_tcn(Forward& f, float* out) {
    fsnp_handle* h = f.h;
    const Workspace& w = f.w;
    const Dims& d = f.d;
    const int num_slots = f.plan.total_slots;
    SbGatherArgs ga{};
    ga.att_mag = f.fptr(w.att); ga.fb_rel = (int)((w.fb - w.att) / 4); ga.fb_branch_stride = d.B * d.Tp * d.FP;
    ga.rows = f.rows; ga.md_utt = f.sbuf.md_utt; ga.md_row = f.sbuf.md_row;
    ga.x = f.fptr(w.sbt_x0); ga.xstride = h->XS;
    ga.num_slots = num_slots; ga.Tp = d.Tp; ga.FP = d.FP; ga.F = d.F; ga.NSBN = h->cfg.sb_num_neighbors; ga.NIN = h->NIN;
    ga.NFBN = h->cfg.fb_num_neighbors;
    launch_sb_gather(ga, f.s);
    Dims ds = d;
    ds.lens = ds.tpb = nullptr;       // (per-utterance lengths are refused with a sub-band TCN: check_lengths)
    ds.B = num_slots; ds.F = h->NIN; ds.FP = h->XS;
    TcnBuffers tb{};
    tb.att = f.fptr(w.sbt_x0); tb.x = f.fptr(w.sbt_x); tb.y1 = f.fptr(w.sbt_y1); tb.y2 = f.fptr(w.sbt_y2);
    tb.gn = reinterpret_cast<double*>(f.base + w.sbt_gn); tb.fb = f.fptr(w.sbt_fb);
    h->sbt.num_cus = h->num_cus;
    launch_tcn(ds, h->cfg.sb_act, h->sbt, tb, f.s, 1);
    launch_sb_scatter(f.fptr(w.sbt_fb), h->XS, f.rows, out, (long)rows_per_utt(h, f.mode) * d.T, num_slots, d.Tp, d.LA, h->cfg.output_size, f.s);
    if (h->timing) {
        FSNP_HIP_CHECK(hipEventRecord(f.rec.e[2], f.s));
        FSNP_HIP_CHECK(hipEventRecord(f.rec.e[3], f.s));
    }
    return 0;
}

// The recurrent sub-band model.  Chunks [0, k) of the plan run on the caller's stream, [k, n) on the side stream behind them:
// k = n unless the pipelined loop defers the column-split remainder chunks behind a row-tile chunk (after it: next to it they would only
// fight for its CUs), where they overlap the next forward's full-band stages, or a plan that STARTS with a column-split launch (small
// batches: k = 0), whose launches leave CUs idle too (B = 1: 216 of 256 busy, latency-bound).  fsnp_set_verify: every Nth forward with a
// column-split launch is checked against the exchange-free kernel on the caller's stream (nothing deferred then).
static int dispatch_subband_lstm(Forward& f, float* out, const int32_t* lengths) {
    fsnp_handle* h = f.h;
    const Dims& d = f.d;
    const SbPlan& plan = f.plan;
    hipStream_t s = f.s, side = h->side_stream;
    LstmArgs a{};
    a.att_mag = f.fptr(f.w.att); a.fb = f.fptr(f.w.fb);
    a.fb_rel = (int)((f.w.fb - f.w.att) / 4);
    a.fb_branch_stride = d.B * d.Tp * d.FP;
    a.rows = f.rows; a.md_utt = f.sbuf.md_utt; a.md_row = f.sbuf.md_row; a.dense = nullptr;
    a.out = out;
    a.out_stride_o = (long)rows_per_utt(h, f.mode) * d.T;
    a.num_rows = d.B * rows_per_utt(h, f.mode); a.Tp = d.Tp; a.LA = d.LA; a.FP = d.FP; a.F = d.F; a.NSBN = h->cfg.sb_num_neighbors;
    a.NFBN = h->cfg.fb_num_neighbors;
    a.act = h->cfg.sb_act;
    float* hx = f.fptr(f.w.coop_hx);
    unsigned* bar = reinterpret_cast<unsigned*>(f.base + f.w.coop_bar);
    unsigned* abort_word = reinterpret_cast<unsigned*>(f.base + f.w.coop_abort);
    const bool verify_now = h->verify_every > 0 && plan_has_exchange(plan) && (h->verify_calls++ % h->verify_every) == 0;
    // fsnp_set_verify_sample: every Nth forward of a plan made of column-split launches only, one row tile is recomputed off the critical path
    const bool sample_now = !verify_now && h->vs_every > 0 && plan_can_be_sampled(h, plan) && (h->vs_calls++ % h->vs_every) == 0;
    a.coop_corrupt = h->corrupt_exchange; h->corrupt_exchange = 0;
    const int n = (int)plan.chunks.size(), k = verify_now || !h->pipeline ? n : plan_first_deferred(h, plan);
    hipEvent_t after_first = h->timing ? f.rec.e[3] : nullptr;      // recorded on the stream of chunk 0, behind it
    if (k > 0) launch_sb_lstm(h, plan, a, hx, bar, abort_word, s, after_first, 0, k);
    if (k < n) {
        FSNP_HIP_CHECK(hipEventRecord(h->ev_main, s));
        FSNP_HIP_CHECK(hipStreamWaitEvent(side, h->ev_main, 0));
        launch_sb_lstm(h, plan, a, hx, bar, abort_word, side, k == 0 ? after_first : nullptr, k, n);
    }
    if (h->timing) FSNP_HIP_CHECK(hipEventRecord(f.rec.e[2], k < n ? side : s));
    if (k < n) {
        FSNP_HIP_CHECK(hipEventRecord(h->ev_side[f.slot], side));
        h->side_used[f.slot] = true;
    }
    if (verify_now) {
        const size_t out_elems = (size_t)(f.mode == FSNP_MODE_PARITY ? f.global_batch : d.B) * h->cfg.output_size * rows_per_utt(h, f.mode) * d.T;
        if (const int vr = verify_pass(h, plan, d, f.mode, f.batch_offset, f.global_batch, a, f.sbuf, out_elems, s)) return vr;
    }
    if (sample_now) {        // (a plan of column-split launches only runs on ONE stream: the side stream when the pipelined loop defers it, else s)
        if (const int vr = verify_sample(h, plan, d, a, f.sbuf, k == 0 ? side : s)) return vr;
        if (k == 0) FSNP_HIP_CHECK(hipEventRecord(h->ev_side[f.slot], side));       // the snapshot reads this workspace half too
    }
    if (lengths) {
        // behind the last sub-band launch that writes the mask (the side stream's, when the pipelined loop deferred any: those follow the
        // caller's stream's chunks), and behind the verification pass / the sampled check's snapshot, which compare what the model wrote
        launch_zero_tails(out, d.lens, d.B, h->cfg.output_size * rows_per_utt(h, f.mode), d.T, k < n ? side : s);
        if (k < n) FSNP_HIP_CHECK(hipEventRecord(h->ev_side[f.slot], side));     // (it reads this workspace half's lengths)
    }
    return 0;
}

static int finish_forward(Forward& f) {
    FSNP_HIP_CHECK(hipGetLastError());
    f.h->last_ws = f.w; f.h->last_dims = f.d; f.h->have_last = true; f.h->last_base = f.base;
    return mark_forward_done(f.h, f.s);
}

static int forward_impl(fsnp_handle* h, const float* mag, const float* real, const float* imag, bool is_complex,
                        const int64_t strides[3][3], float* out, int32_t batch, int32_t frames,
                        int32_t mode, int32_t batch_offset, int32_t global_batch, void* hip_stream, const int32_t* lengths = nullptr) {
    Forward f{};
    if (const int rc = check_forward_args(h, mag, real, imag, is_complex, strides, out, batch, frames, mode, batch_offset, global_batch,
                                          lengths, f.d))
        return rc;
    FSNP_ON_DEVICE(h);
    if (calibrate_costs(h)) return 4;            // first planning call of the process for this kind of handle only (~0.1 s)
    f.h = h; f.s = static_cast<hipStream_t>(hip_stream); f.mode = mode; f.batch_offset = batch_offset; f.global_batch = global_batch;
    const int num_rows = batch * rows_per_utt(h, mode);
    f.plan = plan_sb(h, num_rows, forward_gather_bytes(h, batch, frames));
    if (f.plan.chunks.empty()) {
        set_error("no kernel plan for %d sub-band sequences on this device (%d CUs): the %s sub-band model needs at least %d",
                  num_rows, h->num_cus_real, h->gru ? "GRU" : "LSTM", h->H / 128);
        return 2;
    }
    if (const int rc = bind_workspace(f, lengths != nullptr)) return rc;
    if (lengths) {
        int* lens = reinterpret_cast<int*>(f.base + f.w.lens);
        launch_set_lengths(lengths, batch, f.d.LA, lens, lens + batch, f.s);
        f.d.lens = lens; f.d.tpb = lens + batch;
    }
    if (launch_prologue(f)) return 4;
    if (h->model == FSNP_MODEL_FULLSUBNET) {
        run_fullband_fullsubnet(f, mag, strides[0], is_complex);
    } else {
        const float* in[3] = {mag, real, imag};
        run_fullband_plus(f, in, strides, is_complex);
    }
    launch_subband_stats(f.d, h->cfg.norm_type, f.sbuf, f.rows, f.plan.total_slots, f.s);
    if (h->timing) FSNP_HIP_CHECK(hipEventRecord(f.rec.e[1], f.s));
    if (const int rc = h->sb_tcn ? run_subband_tcn(f, out) : dispatch_subband_lstm(f, out, lengths)) return rc;
    return finish_forward(f);
}

int fsnp_forward(fsnp_handle* h, const float* mag, const float* real, const float* imag,
                 const int64_t strides[3][3], float* out, int32_t batch, int32_t frames,
                 int32_t mode, int32_t batch_offset, int32_t global_batch, void* hip_stream) {
    return forward_impl(h, mag, real, imag, false, strides, out, batch, frames, mode, batch_offset, global_batch, hip_stream);
}

int fsnp_forward_complex(fsnp_handle* h, const float* noisy, const int64_t strides[3], float* out, int32_t batch,
                         int32_t frames, int32_t mode, int32_t batch_offset, int32_t global_batch, void* hip_stream) {
    if (!strides) { set_error("fsnp_forward_complex: null argument"); return 1; }
    int64_t st[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) st[i][j] = strides[j];
    return forward_impl(h, noisy, nullptr, nullptr, true, st, out, batch, frames, mode, batch_offset, global_batch, hip_stream);
}

int fsnp_forward_lengths(fsnp_handle* h, const float* mag, const float* real, const float* imag, const int64_t strides[3][3],
                         const int32_t* lengths, float* out, int32_t batch, int32_t frames, void* hip_stream) {
    if (!lengths) { set_error("fsnp_forward_lengths: null lengths"); return 1; }
    return forward_impl(h, mag, real, imag, false, strides, out, batch, frames, FSNP_MODE_FULL, 0, batch, hip_stream, lengths);
}

int fsnp_forward_complex_lengths(fsnp_handle* h, const float* noisy, const int64_t strides[3], const int32_t* lengths, float* out,
                                 int32_t batch, int32_t frames, void* hip_stream) {
    if (!strides || !lengths) { set_error("fsnp_forward_complex_lengths: null argument"); return 1; }
    int64_t st[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) st[i][j] = strides[j];
    return forward_impl(h, noisy, nullptr, nullptr, true, st, out, batch, frames, FSNP_MODE_FULL, 0, batch, hip_stream, lengths);
}

int fsnp_reserve(fsnp_handle* h, int32_t max_batch, int32_t max_frames, int32_t mode, int32_t max_samples, void* hip_stream) {
    if (!h || max_batch <= 0 || max_frames <= 0 || max_samples < 0) { set_error("fsnp_reserve: bad argument"); return 1; }
    if (mode != FSNP_MODE_FULL && mode != FSNP_MODE_PARITY) { set_error("unknown mode %d", mode); return 2; }
    if (!h->committed) { set_error("fsnp_reserve: weights not committed (the plan depends on the kernels' occupancy)"); return 2; }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    if (order_after_last_forward(h, s)) return 4;
    if (calibrate_costs(h)) return 4;            // FSNP_CALIBRATE=1: size the workspace for the plans the ADOPTED cost table will make
    // every batch size up to max_batch plans its own launches (the exchange region of a column-split plan can exceed the one of
    // the chip-filling batch): take the largest workspace over all of them - host arithmetic only
    size_t need = 0;
    for (int b = 1; b <= max_batch; ++b) {
        if (mode == FSNP_MODE_PARITY && b <= h->cfg.num_groups_in_drop_band) continue;
        need = std::max(need, plan_workspace(h, b, max_frames, mode, mode == FSNP_MODE_FULL).total);   // (FULL: room for lengths too)
    }
    if (ensure_workspace(h, need, s)) return 4;
    if (max_samples > 0) {
        if (h->cfg.output_size != 2) { set_error("fsnp_reserve: max_samples > 0 sizes the waveform path, which needs output_size = 2 (this handle: %d)", h->cfg.output_size); return 2; }
        if (ensure_stft(h)) return 2;
        if (ensure_io(h, wave_io(stft_plan(h), max_batch, max_samples).total, s)) return 4;
    }
    return mark_forward_done(h, s);
}

int fsnp_apply_cirm(const float* mask, const float* noisy, const int64_t strides[3], float* out,
                    const int64_t out_strides[3], int32_t batch, int32_t freqs, int32_t frames, void* hip_stream) {
    if (!mask || !noisy || !out || !strides || !out_strides) { set_error("fsnp_apply_cirm: null argument"); return 1; }
    if (batch <= 0 || freqs <= 0 || frames <= 0) { set_error("fsnp_apply_cirm: empty input"); return 2; }
    launch_apply_cirm(mask, noisy, strides, out, out_strides, batch, freqs, frames, nullptr, static_cast<hipStream_t>(hip_stream));
    FSNP_HIP_CHECK(hipGetLastError());
    return 0;
}

int fsnp_apply_cirm_lengths(const float* mask, const float* noisy, const int64_t strides[3], float* out, const int64_t out_strides[3],
                            const int32_t* lengths, int32_t batch, int32_t freqs, int32_t frames, void* hip_stream) {
    if (!mask || !noisy || !out || !strides || !out_strides || !lengths) { set_error("fsnp_apply_cirm_lengths: null argument"); return 1; }
    if (batch <= 0 || freqs <= 0 || frames <= 0) { set_error("fsnp_apply_cirm_lengths: empty input"); return 2; }
    for (int b = 0; b < batch; ++b)
        if (lengths[b] < 1 || lengths[b] > frames) {
            set_error("fsnp_apply_cirm_lengths: utterance %d: length %d outside [1, %d]", b, (int)lengths[b], (int)frames);
            return 2;
        }
    launch_apply_cirm(mask, noisy, strides, out, out_strides, batch, freqs, frames, lengths, static_cast<hipStream_t>(hip_stream));
    FSNP_HIP_CHECK(hipGetLastError());
    return 0;
}

int fsnp_lstm2_fc(fsnp_handle* h, const float* x, float* out, int32_t num_seq, int32_t steps, void* hip_stream) {
    if (!h || !x || !out) { set_error("fsnp_lstm2_fc: null argument"); return 1; }
    if (!h->committed) { set_error("fsnp_lstm2_fc: weights not committed"); return 2; }
    if (h->sb_tcn) { set_error("fsnp_lstm2_fc: the sub-band model of this handle is a TCN (no recurrent kernel)"); return 2; }
    if (num_seq <= 0 || steps <= 0) { set_error("fsnp_lstm2_fc: empty input"); return 2; }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    if ((double)num_seq * steps * h->NIN > 2.0e9) { set_error("fsnp_lstm2_fc: input too large for 32-bit offsets"); return 2; }
    if (calibrate_costs(h)) return 4;
    const SbPlan plan = plan_sb(h, num_seq, (double)num_seq * steps * h->NIN * 4.0);
    if (plan.chunks.empty()) { set_error("fsnp_lstm2_fc: no kernel plan for %d sequences on this device", num_seq); return 2; }
    return run_dense_plan(h, plan, x, out, num_seq, steps, s);
}

// ---- the forward's submodules as stages (include/fsnp.h: "third kind")
static int stage_args_ok(const char* fn, const fsnp_handle* h, int32_t branch, const float* in, const int64_t* strides, const float* out, int32_t B, int32_t T) {
    if (!h || !in || !strides || !out) { set_error("%s: null argument", fn); return 1; }
    if (!h->committed) { set_error("%s: weights not committed", fn); return 4; }
    if (h->model != FSNP_MODEL_FULLSUBNET_PLUS) { set_error("%s: FullSubNet+ handles only (the original FullSubNet has no attention layer and a recurrent full-band model)", fn); return 2; }
    if (branch < 0 || branch > 2) { set_error("%s: branch must be 0 (magnitude), 1 (real) or 2 (imaginary)", fn); return 2; }
    if (B <= 0 || T <= 0) { set_error("%s: empty input", fn); return 2; }
    if ((double)B * T * std::max(h->FP, h->CH) * 4.0 > 2.0e9) { set_error("%s: input too large for 32-bit offsets", fn); return 2; }
    return 0;
}
static Dims stage_dims(const fsnp_handle* h, int B, int T) {
    Dims d{};
    d.B = B; d.T = T; d.Tp = T; d.F = h->F; d.FP = h->FP; d.CH = h->CH; d.H = h->H; d.NIN = h->NIN; d.LA = 0;
    return d;
}

int fsnp_channel_attention(fsnp_handle* h, int32_t branch, const float* in, const int64_t strides[3], float* out, int32_t batch,
                           int32_t frames, void* hip_stream) {
    if (const int rc = stage_args_ok("fsnp_channel_attention", h, branch, in, strides, out, batch, frames)) return rc;
    if (branch == 0 && h->fw.subband_num > 1) {
        set_error("fsnp_channel_attention: with subband_num > 1 the magnitude branch's layer runs on the tensor the forward regroups around it (fullsubnet_plus.py:146-153): not a stage");
        return 2;
    }
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    if (order_after_weight_pack(h, s)) return 4;     // (the stage reads the blob: a device pack on another stream must have finished)
    const Dims d = stage_dims(h, batch, frames);
    const size_t plane = align_up((size_t)d.B * d.Tp * d.FP * 4, 256), md_b = align_up((size_t)d.B * d.Tp * sizeof(NormMD), 256);
    const size_t fsum_b = align_up((size_t)d.B * d.FP * 8, 256), tot_b = align_up((size_t)d.B * 2 * 8, 256), gate_b = align_up((size_t)d.B * d.FP * 4, 256);
    unsigned char* work = nullptr;
    FSNP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&work), 2 * plane + md_b + fsum_b + tot_b + gate_b, s));
    FrontendBuffers buf{};
    buf.raw = reinterpret_cast<float*>(work); buf.att = reinterpret_cast<float*>(work + plane);
    buf.md = reinterpret_cast<NormMD*>(work + 2 * plane);
    buf.fsum = reinterpret_cast<double*>(work + 2 * plane + md_b);
    buf.tot = reinterpret_cast<double*>(work + 2 * plane + md_b + fsum_b);
    buf.gate = reinterpret_cast<float*>(work + 2 * plane + md_b + fsum_b + tot_b);
    FSNP_HIP_CHECK(hipMemsetAsync(buf.fsum, 0, fsum_b + tot_b, s));
    FrontendWeights w = h->fw;                      // the branch's weights in slot 0 (the kernels index by grid.y)
    for (int k = 0; k < 3; ++k) { w.conv_w[0][k] = h->fw.conv_w[branch][k]; w.conv_b[0][k] = h->fw.conv_b[branch][k]; }
    w.cat_w[0] = h->fw.cat_w[branch]; w.cat_b[0] = h->fw.cat_b[branch];
    w.fc1_wT[0] = h->fw.fc1_wT[branch]; w.fc1_b[0] = h->fw.fc1_b[branch];
    w.fc2_wT[0] = h->fw.fc2_wT[branch]; w.fc2_b[0] = h->fw.fc2_b[branch];
    launch_attention_stage(d, w, in, strides, buf, s);
    launch_tm_to_bft(buf.att, out, d.B, d.T, d.Tp, d.F, d.FP, s);
    FSNP_HIP_CHECK(hipGetLastError());
    FSNP_HIP_CHECK(hipFreeAsync(work, s));
    return 0;
}

int fsnp_fullband_model(fsnp_handle* h, int32_t branch, const float* in, const int64_t strides[3], float* out, int32_t batch,
                        int32_t frames, void* hip_stream) {
    if (const int rc = stage_args_ok("fsnp_fullband_model", h, branch, in, strides, out, batch, frames)) return rc;
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    FSNP_ON_DEVICE(h);
    if (order_after_weight_pack(h, s)) return 4;     // (the stage reads the blob: a device pack on another stream must have finished)
    const Dims d = stage_dims(h, batch, frames);
    const TcnWeights& t = h->tw;
    const size_t plane = align_up((size_t)d.B * d.Tp * d.FP * 4, 256), yplane = align_up((size_t)d.B * d.Tp * d.CH * 4, 256);
    const size_t gn_b = align_up((size_t)std::max(t.NB, 1) * 2 * d.B * kGnStride * 8, 256);
    unsigned char* work = nullptr;
    FSNP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&work), 3 * plane + 2 * yplane + gn_b, s));
    TcnBuffers tb{};
    float* att = reinterpret_cast<float*>(work);
    tb.att = att; tb.x = reinterpret_cast<float*>(work + plane); tb.fb = reinterpret_cast<float*>(work + 2 * plane);
    tb.y1 = reinterpret_cast<float*>(work + 3 * plane); tb.y2 = reinterpret_cast<float*>(work + 3 * plane + yplane);
    tb.gn = reinterpret_cast<double*>(work + 3 * plane + 2 * yplane);
    FSNP_HIP_CHECK(hipMemsetAsync(tb.gn, 0, gn_b, s));
    // (the running activation's pad columns [F, FP) meet zero weights in every GEMM but must be finite: fresh pool memory is not)
    FSNP_HIP_CHECK(hipMemsetAsync(tb.x, 0, 2 * plane, s));
    TcnWeights wb = t;                              // this branch's slice of every [3][...] array (strides: launch_tcn)
    const long nb = t.NB, br = branch;
    wb.w1 += br * nb * t.N1P * t.K1P; wb.b1 += br * nb * t.N1P; wb.a1 += br * nb;
    wb.g1w += br * nb * d.CH; wb.g1b += br * nb * d.CH; wb.dw += br * nb * 3 * d.CH; wb.db += br * nb * d.CH; wb.a2 += br * nb;
    wb.g2w += br * nb * d.CH; wb.g2b += br * nb * d.CH;
    wb.w2 += br * nb * t.N2P * t.K2P; wb.b2 += br * nb * t.N2P;
    if (wb.w2g) { wb.w2g += br * nb * t.N2P * t.K2P; wb.c1 += br * nb * t.N2P; wb.c2 += br * nb * t.N2P; }
    wb.wf += br * (long)t.N2P * t.K1P; wb.bf += br * t.N2P;
    launch_repack_plane(d, in, strides, att, s);
    launch_tcn(d, h->cfg.fb_act, wb, tb, s, 1);
    launch_tm_to_bft(tb.fb, out, d.B, d.T, d.Tp, d.F, d.FP, s);
    FSNP_HIP_CHECK(hipGetLastError());
    FSNP_HIP_CHECK(hipFreeAsync(work, s));
    return 0;
}

int fsnp_set_precision(fsnp_handle* h, int32_t ih_bf16) {
    if (!h || ih_bf16 < 0 || ih_bf16 > 1) { set_error("fsnp_set_precision: 0 (fp32) or 1 (bf16 ih-GEMM, BASELINE.json configs[4])"); return 1; }
    if (ih_bf16 && (h->gru || h->sb_tcn)) { set_error("fsnp_set_precision: the bf16 ih-GEMM variant exists for the LSTM sub-band model only"); return 2; }
    if (ih_bf16 && h->H != 384) { set_error("fsnp_set_precision: the bf16 variants exist for sb_model_hidden_size = 384 only"); return 2; }
    if (ih_bf16 && (h->KX != 40 || h->NIN >= h->KX)) { set_error("fsnp_set_precision: the bf16 ih-GEMM variant exists for sub-band inputs of <= 39 features only (its layer-0 bias rides in a spare input column)"); return 2; }
    h->ih_bf16 = ih_bf16;
    h->lw.ih_bf16 = ih_bf16 == 1 ? 1 : 0;       // (launch_lstm's own switch: the bf16-ih variant of lstm.hip)
    return 0;
}

int fsnp_poll_errors(fsnp_handle* h) {
    if (!h) { set_error("null handle"); return 1; }
    return take_device_errors(h, "fsnp_poll_errors");
}
int fsnp_set_pipeline(fsnp_handle* h, int32_t enable) {
    if (!h || (enable != 0 && enable != 1)) { set_error("fsnp_set_pipeline: 0 or 1"); return 1; }
    if (enable == h->pipeline) return 0;
    FSNP_ON_DEVICE(h);
    FSNP_HIP_CHECK(hipDeviceSynchronize());              // nothing of either mode is in flight while the workspace is re-shaped
    if (enable && !h->side_stream) {
        // the deferred remainder chunk is a latency-bound chain of inter-workgroup hand-offs: at the highest stream priority
        // its waves win the arbitration against the full-band GEMMs it shares CUs with
        int lo = 0, hi = 0;
        if (hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess && hi != lo)
            FSNP_HIP_CHECK(hipStreamCreateWithPriority(&h->side_stream, hipStreamNonBlocking, hi));
        else
            FSNP_HIP_CHECK(hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking));
        FSNP_HIP_CHECK(hipEventCreateWithFlags(&h->ev_main, hipEventDisableTiming));
        for (auto& e : h->ev_side) FSNP_HIP_CHECK(hipEventCreateWithFlags(&e, hipEventDisableTiming));
    }
    if (h->ws) { FSNP_HIP_CHECK(hipFreeAsync(h->ws, nullptr)); FSNP_HIP_CHECK(hipDeviceSynchronize()); h->ws = nullptr; h->ws_bytes = 0; }
    h->have_last = false;
    h->pipeline = enable;
    h->ws_slots = enable ? 2 : 1;
    h->ws_slot = 0;
    h->side_used[0] = h->side_used[1] = false;
    return 0;
}

int fsnp_flush(fsnp_handle* h, void* hip_stream) {
    if (!h) { set_error("null handle"); return 1; }
    if (!h->pipeline) return 0;
    FSNP_ON_DEVICE(h);
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    for (int k = 0; k < 2; ++k)
        if (h->side_used[k]) FSNP_HIP_CHECK(hipStreamWaitEvent(s, h->ev_side[k], 0));
    return 0;
}

int fsnp_check_errors(fsnp_handle* h) {
    if (!h) { set_error("null handle"); return 1; }
    FSNP_ON_DEVICE(h);
    FSNP_HIP_CHECK(hipDeviceSynchronize());
    return take_device_errors(h, "fsnp_check_errors");
}

int64_t fsnp_dump_config(const fsnp_handle* h, char* buf, int64_t cap) {
    if (!h) { set_error("null handle"); return -1; }
    auto env = [](const char* n) { const char* e = getenv(n); return e ? e : "(unset)"; };
    std::string o;
    char line[512];
    auto add = [&](const char* fmt, ...) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(line, sizeof(line), fmt, ap);
        va_end(ap);
        o += line;
    };
    add("%s, ABI %d, device %d (%d CUs; planner sees %d)\n", fsnp_version(), FSNP_ABI_VERSION, h->device, h->num_cus_real, h->num_cus);
    add("model=%s num_freqs=%d look_ahead=%d sb_hidden=%d tcn_hidden=%d sub-band inputs=%d (kernels instantiated for K=%d) sequence_model=%s norm_type=%d attention=%d subband_num=%d\n",
        h->model == FSNP_MODEL_FULLSUBNET ? "FullSubNet" : "FullSubNet+", h->F, h->cfg.look_ahead, h->H, h->CH, h->NIN, h->KX,
        h->sb_tcn ? "TCN" : h->gru ? "GRU" : "LSTM", h->cfg.norm_type, h->cfg.attention, h->cfg.subband_num > 0 ? h->cfg.subband_num : 1);
    add("waveform path: n_fft=%d hop_length=%d (win_length = n_fft, periodic Hann; fsnp_set_hop_length)\n", 2 * (h->F - 1), (int)fsnp_hop_length(h));
    add("waveform io area: %zu bytes at %p; resample tables: %d of %d (include/fsnp_resample.h)\n", h->io_bytes, (void*)h->io, (int)h->resample.size(), kResampleMaxPairs);
    add("weights committed=%d precision=%d (0 fp32, 1 bf16 ih-GEMM) pipeline=%d timing=%d workspace=%zu bytes x %d\n",
        (int)h->committed, h->ih_bf16, h->pipeline, (int)h->timing, h->ws_bytes, h->ws_slots);
    add("effective settings (environment variable as read at fsnp_create = value in force):\n");
    add("  FSNP_LSTM_COOP=%s -> column-split kernels %s\n", env("FSNP_LSTM_COOP"), h->planner.lstm_coop ? "planned (auto)" : "never");
    add("  FSNP_COOP_HP=%s -> half-tile ping-pong kernel (lstm_hp.hip / lstm_hpw.hip) %s\n", env("FSNP_COOP_HP"), !h->planner.hp_ok ? "not built for this model" : h->planner.coop_hp ? "planned" : "never");
    add("  FSNP_HP_WAVE=%s -> its launches run on %s\n", env("FSNP_HP_WAVE"), h->hp_wave && lstm_hpw_available(h->lw) ? "lstm_hpw.hip (wave-owned units, round 6)" : "lstm_hp.hip (gate-split waves, round 3)");
    add("  FSNP_COOP_W=%s -> wave-owned column split (lstm_coopw.hip) %s\n", env("FSNP_COOP_W"), !h->planner.coopw_ok ? "not built for this model" : h->planner.coop_w ? "planned" : "never");
    add("  FSNP_COOP_SKEW=%s -> K-split schedule %s\n", env("FSNP_COOP_SKEW"), h->coop_skew ? "layer-skewed" : "serial");
    add("  FSNP_COOP_OCC=%s -> column-split workgroups per CU the planner may use: %d\n", env("FSNP_COOP_OCC"), h->planner.coop_occ);
    add("  FSNP_LSTM16=%s -> half-tile kernel %s\n", env("FSNP_LSTM16"), h->planner.lstm16_ok ? "planned" : "not used");
    add("  FSNP_CALIBRATE=%s -> cost table %s\n", env("FSNP_CALIBRATE"), h->planner.cost.calibrated ? "measured / pinned" : h->calibrate ? "to be measured at the first plan" : "built-in");
    add("  FSNP_GEMM_DMA=%s -> %d (0 = the general GEMM kernel everywhere)\n", env("FSNP_GEMM_DMA"), h->tw.gemm_dma);
    add("  FSNP_VERIFY_EVERY=%s -> exchange verification every %d forwards (0 = off)\n", env("FSNP_VERIFY_EVERY"), h->verify_every);
    add("  FSNP_DEBUG_STAGES=%s -> %d\n", env("FSNP_DEBUG_STAGES"), (int)h->debug);
    const CostTable& t = h->planner.cost;
    add("cost table (us per step): K split full %.1f / %.1f / %.1f / %.1f, one tile %.1f / %.1f / %.1f / %.1f, three-way %.1f / %.1f, one tile per CU %.1f (+%.2f per VALU row), half tile %.1f, half-tile ping-pong %.1f / %.1f, wave-owned split full %.1f / %.1f / %.1f, one tile %.1f / %.1f / %.1f\n",
        t.ksplit[0][0], t.ksplit[1][0], t.ksplit[2][0], t.ksplit[3][0], t.ksplit1[0], t.ksplit1[1], t.ksplit1[2], t.ksplit1[3], t.coopn[0][0], t.coopn[1][0],
        t.rowtile, t.rowtile_ex, t.rowtile16, t.hp[0], t.hp[1], t.coopw[0][1], t.coopw[1][1], t.coopw[2][1], t.coopw[0][0], t.coopw[1][0], t.coopw[2][0]);
    if (buf && cap > 0) {
        const size_t n = o.size() < (size_t)cap - 1 ? o.size() : (size_t)cap - 1;
        memcpy(buf, o.data(), n);
        buf[n] = 0;
    }
    return (int64_t)o.size() + 1;
}

}  // extern "C"
