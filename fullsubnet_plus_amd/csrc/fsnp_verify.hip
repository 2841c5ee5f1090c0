// fsnp_verify.hip - the two checks of the column-split sub-band launches against the exchange-free kernels: every Nth forward re-run
// whole (fsnp_set_verify) and one sampled row tile recomputed off the critical path (fsnp_set_verify_sample).  Called by the forward
// (fsnp_abi.hip); a mismatch sets kErrVerify in the handle's error word and a key that take_device_errors decodes.
#include <algorithm>

#include "fsnp_common.h"
#include "lstm_common.h"
#include "planner.h"
#include "fsnp_handle.h"

namespace fsnp {

// The kernels sum K in different orders, so "equal" is a tolerance: |a - b| <= 1e-4 + 1e-3 |b| (kernel-to-kernel differences are
// ~1e-6; one corrupted exchange element moves the mask by 1e-2 and more).  Where a value differs, the key of its (utterance, bin, frame)
// lowers the first-disagreement key: 20 bits of utterance, 20 of bin, 24 of frame - nothing the entry points accept wraps (ADVICE r05:
// the 8 / 10 / 14-bit key did).  (Two helpers: one that also held the branch and the atomics changed the kernels' code.)
__device__ __forceinline__ bool mask_differs(float a, float b) { return !(fabsf(a - b) <= 1e-4f + 1e-3f * fabsf(b)); }
__device__ __forceinline__ unsigned long long mismatch_key(const RowDesc& rd, int t) {
    return ((unsigned long long)(unsigned)rd.b << 44) | ((unsigned long long)((unsigned)rd.f & 0xFFFFFu) << 24) | (unsigned long long)((unsigned)t & 0xFFFFFFu);
}

// ---- fsnp_set_verify: the sequences a plan hands to column-split kernels, run again on the one-tile-per-CU kernel (no inter-workgroup
// exchange at all) into a scratch mask and compared on the device.
__global__ __launch_bounds__(256) void verify_compare_kernel(const float* __restrict__ out, const float* __restrict__ ref, const RowDesc* __restrict__ rows,
                                                             int num_slots, int T, int OC, long stride_o, unsigned* err_host,
                                                             unsigned long long* first_key) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (long)num_slots * OC * T) return;
    const int t = (int)(i % T), o = (int)((i / T) % OC), slot = (int)(i / ((long)OC * T));
    const RowDesc rd = rows[slot];
    if (!rd.valid) return;
    const size_t at = (size_t)rd.out_off + (size_t)o * stride_o + t;
    const float a = out[at], b = ref[at];
    if (mask_differs(a, b)) {
        __hip_atomic_fetch_min(first_key, mismatch_key(rd, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_or(err_host, kErrVerify, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
bool plan_has_exchange(const SbPlan& plan) {
    for (const SbChunk& c : plan.chunks) if (is_column_split(c.kind)) return true;
    return false;
}
// `a` = the arguments of the forward's own sub-band launches (its rows / md_row belong to `plan`); out_elems = floats of the mask tensor
int verify_pass(fsnp_handle* h, const SbPlan& plan, const Dims& d, int mode, int batch_offset, int global_batch, const LstmArgs& a,
                const SubbandBuffers& sbuf, size_t out_elems, hipStream_t s) {
    const bool cumulative = h->cfg.norm_type == FSNP_NORM_CUMULATIVE_LAPLACE || h->cfg.norm_type == FSNP_NORM_CUMULATIVE_LAYER;
    // the exchange-free plan of exactly the column-split chunks' sequences; consecutive chunks (B = 8: three launches over rows
    // [0, 2056)) are re-run as ONE range - one round of half tiles instead of one per launch
    SbPlan vp;
    PlannerCtx pc = pctx(h);
    pc.lstm_coop = 0;
    pc.half_tiles_without_coop = true;
    pc.ih_bf16 = 0;                          // (the re-run is fp32 whatever fsnp_set_precision says: below)
    bool bad = false;
    int run0 = 0, run_n = 0;
    auto flush = [&]() {
        if (run_n == 0) return;
        const SbPlan one = plan_sb(pc, run_n);
        for (SbChunk k : one.chunks) {
            if (k.kind != SbKind::RowTile && k.kind != SbKind::HalfTile) { bad = true; return; }
            k.row0 += run0; k.slot0 = vp.total_slots; k.coop_tile0 = 0;
            vp.total_slots += k.num_tiles * k.rps;
            vp.chunks.push_back(k);
        }
        run_n = 0;
    };
    for (const SbChunk& c : plan.chunks) {
        const bool exch = is_column_split(c.kind);
        if (exch && run_n > 0 && c.row0 == run0 + run_n) { run_n += c.nrows; continue; }
        flush();
        if (exch) { run0 = c.row0; run_n = c.nrows; }
    }
    flush();
    if (bad) { set_error("fsnp_set_verify: no exchange-free kernel for this model"); return 2; }
    if (vp.chunks.empty()) return 0;
    const size_t out_b = align_up(out_elems * 4, 256), rows_b = align_up((size_t)vp.total_slots * sizeof(RowDesc), 256);
    const size_t md_b = cumulative ? align_up((size_t)vp.total_slots * d.Tp * sizeof(NormMD), 256) : 0;
    const size_t need = out_b + rows_b + md_b;
    if (need > h->verify_bytes) {
        if (h->verify_out) FSNP_HIP_CHECK(hipFreeAsync(h->verify_out, s));
        h->verify_out = nullptr; h->verify_bytes = 0;
        FSNP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&h->verify_out), need, s));
        h->verify_bytes = need;
    }
    unsigned char* vb = reinterpret_cast<unsigned char*>(h->verify_out);
    RowDesc* vrows = reinterpret_cast<RowDesc*>(vb + out_b);
    NormMD* vmd = cumulative ? reinterpret_cast<NormMD*>(vb + out_b + rows_b) : nullptr;
    launch_build_rows(vp, vrows, {h->F, d.T, mode, batch_offset, global_batch, 0, h->cfg.num_groups_in_drop_band, h->cfg.output_size}, s);
    if (cumulative) {
        SubbandBuffers vs = sbuf;
        vs.md_row = vmd;
        launch_subband_stats(d, h->cfg.norm_type, vs, vrows, vp.total_slots, s);      // (cumulative norms: per-slot tables only)
    }
    LstmArgs va = a;
    va.rows = vrows; va.md_row = vmd; va.out = reinterpret_cast<float*>(vb);
    // the column-split kernels are fp32 in every precision mode, so their check is too: under fsnp_set_precision(h, 1) the row-tile /
    // half-tile kernels would otherwise run their bf16 ih-GEMM here and differ from a CORRECT exchange by ~1e-3 - a false alarm
    const int keep_bf16 = h->lw.ih_bf16;
    h->lw.ih_bf16 = 0;
    launch_sb_lstm(h, vp, va, nullptr, nullptr, nullptr, s);
    h->lw.ih_bf16 = keep_bf16;
    const long n = (long)vp.total_slots * h->cfg.output_size * d.T;
    if (!h->verify_key) FSNP_HIP_CHECK(hipMalloc(reinterpret_cast<void**>(&h->verify_key), 8));
    FSNP_HIP_CHECK(hipMemsetAsync(h->verify_key, 0xFF, 8, s));
    hipLaunchKernelGGL(verify_compare_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a.out, reinterpret_cast<const float*>(vb), vrows,
                       vp.total_slots, d.T, h->cfg.output_size, a.out_stride_o, h->d_err, h->verify_key);
    FSNP_HIP_CHECK(hipGetLastError());
    h->verify_runs += 1;
    return 0;
}

// ---- fsnp_set_verify_sample: ONE row tile of a column-split launch, recomputed off the critical path.
// The sampled tile's normalised input and the mask values its launch wrote are SNAPSHOT on the launch's own stream (two tiny kernels);
// the recomputation - the exchange-free half-tile kernel on the snapshot, two workgroups, as long as a whole round: ~13 ms at 2 s clips -
// and the comparison run on a stream of their own and touch nothing but private buffers, so the caller may free / overwrite the mask and
// later forwards may rebuild the workspace meanwhile.  A mismatch flags the handle (code 7) whenever it is found: the report names the
// sampled forward's (utterance, bin, frame), the call that notices it is a later one.
__global__ __launch_bounds__(256) void vs_copy_kernel(const float* __restrict__ out, const RowDesc* __restrict__ rows, RowDesc* __restrict__ rows_copy,
                                                      float* __restrict__ snap, int num_slots, int T, int OC, long stride_o) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < num_slots) rows_copy[i] = rows[i];
    if (i >= num_slots * OC * T) return;
    const int t = i % T, o = (i / T) % OC, slot = i / (OC * T);
    const RowDesc rd = rows[slot];
    snap[i] = rd.valid ? out[(size_t)rd.out_off + (size_t)o * stride_o + t] : 0.0f;
}
__global__ __launch_bounds__(256) void vs_compare_kernel(const float* __restrict__ snap, const float* __restrict__ ref, const RowDesc* __restrict__ rows,
                                                         int num_slots, int T, int OC, unsigned* err_host, unsigned long long* first_key) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= num_slots * OC * T) return;
    const int t = i % T, slot = i / (OC * T);
    const RowDesc rd = rows[slot];
    if (!rd.valid) return;
    const float a = snap[i], b = ref[i];                        // ref: the dense run's [slot][o][t]
    if (mask_differs(a, b)) {
        __hip_atomic_fetch_min(first_key, mismatch_key(rd, t), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        __hip_atomic_fetch_or(err_host, kErrVerify, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    }
}
// a plan that can be sampled: column-split launches only, each leaving a CU free ON EVERY XCD.  The recomputation's two workgroups own
// their CUs for ~13 ms (one each on two XCDs), and the dispatcher deals a launch's workgroups to the XCDs by index, not by room: B = 8's
// 252-workgroup launches put 32 on some XCDs - the 32nd waited for the sample to end and the launch (all of whose workgroups must be
// resident) with it: +7.7 ms per sampled forward (profiles/r06_verify_sample.md).  Such plans (B = 3, B = 8) are not sampled.
bool plan_can_be_sampled(const fsnp_handle* h, const SbPlan& plan) {
    if (plan.chunks.empty() || !h->planner.lstm16_ok || h->num_cus_real % 8 != 0) return false;
    const int cpx = h->num_cus_real / 8;
    const PlannerCtx pc = pctx(h);
    for (const SbChunk& c : plan.chunks) {
        if (!is_column_split(c.kind) || c.rps != 32) return false;
        const CoopFootprint f = chunk_footprint(pc, c, true, 1);         // (launch_sb_lstm: XCD-local placement where it fits, else round robin)
        if (*std::max_element(f.per_xcd, f.per_xcd + kNumXcds) > cpx - 1) return false;
    }
    return true;
}
// `st` = the stream the plan's launches were enqueued on (the caller's, or the side stream in the pipelined loop)
int verify_sample(fsnp_handle* h, const SbPlan& plan, const Dims& d, const LstmArgs& a, const SubbandBuffers& sbuf, hipStream_t st) {
    if (h->vs_busy) {
        const hipError_t q = hipEventQuery(h->ev_vs_done);
        if (q == hipErrorNotReady) { (void)hipGetLastError(); h->vs_skipped += 1; return 0; }      // the previous sample is still being recomputed
        h->vs_busy = false;
    }
    const long long n = h->vs_runs;
    const SbChunk& c = plan.chunks[(size_t)(n % (long long)plan.chunks.size())];
    const int tile = (int)((n / (long long)plan.chunks.size()) % c.num_tiles), nslots = 32;
    const int OC = h->cfg.output_size, T = d.T, Tp = d.Tp, NIN = h->NIN;
    const size_t x_b = align_up((size_t)nslots * Tp * NIN * 4, 256), o_b = align_up((size_t)nslots * OC * T * 4, 256);
    const size_t r_b = align_up((size_t)nslots * sizeof(RowDesc), 256);
    const size_t need = x_b + 2 * o_b + 2 * r_b + 256;
    if (!h->vs_stream) {
        FSNP_HIP_CHECK(hipStreamCreateWithFlags(&h->vs_stream, hipStreamNonBlocking));
        FSNP_HIP_CHECK(hipEventCreateWithFlags(&h->ev_vs_snap, hipEventDisableTiming));
        FSNP_HIP_CHECK(hipEventCreateWithFlags(&h->ev_vs_done, hipEventDisableTiming));
    }
    if (need > h->vs_bytes) {                 // (no sample in flight here: the buffer is idle)
        h->verify_key_sampled = nullptr;      // (it points into the buffer: an early return below must not leave it dangling)
        if (h->vs_buf) FSNP_HIP_CHECK(hipFreeAsync(h->vs_buf, st));
        h->vs_buf = nullptr; h->vs_bytes = 0;
        FSNP_HIP_CHECK(hipMallocAsync(reinterpret_cast<void**>(&h->vs_buf), need, st));
        h->vs_bytes = need;
    }
    float* vx = reinterpret_cast<float*>(h->vs_buf);
    float* vsnap = reinterpret_cast<float*>(h->vs_buf + x_b);
    float* vref = reinterpret_cast<float*>(h->vs_buf + x_b + o_b);
    RowDesc* vrows_src = reinterpret_cast<RowDesc*>(h->vs_buf + x_b + 2 * o_b);
    RowDesc* vrows = reinterpret_cast<RowDesc*>(h->vs_buf + x_b + 2 * o_b + r_b);
    unsigned long long* vkey = reinterpret_cast<unsigned long long*>(h->vs_buf + x_b + 2 * o_b + 2 * r_b);
    const size_t slot0 = (size_t)c.slot0 + (size_t)tile * c.rps;
    // ---- snapshot, behind the launches it samples
    SbGatherArgs ga{};
    ga.att_mag = a.att_mag; ga.fb_rel = a.fb_rel; ga.fb_branch_stride = a.fb_branch_stride;
    ga.rows = a.rows + slot0; ga.md_utt = a.md_utt; ga.md_row = a.md_row ? a.md_row + slot0 * Tp : nullptr;
    ga.x = vx; ga.xstride = NIN;
    ga.num_slots = nslots; ga.Tp = Tp; ga.FP = d.FP; ga.F = d.F; ga.NSBN = h->cfg.sb_num_neighbors; ga.NIN = NIN; ga.NFBN = h->cfg.fb_num_neighbors;
    launch_sb_gather(ga, st);
    const int nout = nslots * OC * T;
    hipLaunchKernelGGL(vs_copy_kernel, dim3(cdiv(nout, 256)), dim3(256), 0, st, a.out, a.rows + slot0, vrows_src, vsnap, nslots, T, OC, a.out_stride_o);
    FSNP_HIP_CHECK(hipMemsetAsync(vkey, 0xFF, 8, st));
    FSNP_HIP_CHECK(hipEventRecord(h->ev_vs_snap, st));
    // ---- recomputation and comparison, on their own stream
    hipStream_t vs = h->vs_stream;
    FSNP_HIP_CHECK(hipStreamWaitEvent(vs, h->ev_vs_snap, 0));
    launch_build_rows(vrows, {nslots, 2, 16, 0}, dense_rows(T, OC), vs);
    LstmArgs va{};
    va.rows = vrows; va.dense = vx; va.dense_stride = NIN; va.out = vref; va.out_stride_o = T;
    va.num_rows = nslots; va.num_tiles = 2; va.Tp = Tp; va.LA = d.LA; va.FP = 0; va.F = 1; va.NSBN = 0; va.act = h->cfg.sb_act;
    va.coop_own_cu = 1;                      // its two workgroups share the chip with the following forwards: they own their CUs (lstm16.hip: OWN)
    const int keep_bf16 = h->lw.ih_bf16;     // the column-split kernels are fp32 in every precision mode: so is their check
    h->lw.ih_bf16 = 0;
    launch_lstm16(h->lw, va, vs);
    h->lw.ih_bf16 = keep_bf16;
    hipLaunchKernelGGL(vs_compare_kernel, dim3(cdiv(nout, 256)), dim3(256), 0, vs, vsnap, vref, vrows_src, nslots, T, OC, h->d_err, vkey);
    FSNP_HIP_CHECK(hipGetLastError());
    FSNP_HIP_CHECK(hipEventRecord(h->ev_vs_done, vs));
    h->vs_busy = true;
    h->vs_runs += 1;
    h->verify_key_sampled = vkey;
    return 0;
}

}  // namespace fsnp

extern "C" {

int fsnp_set_verify(fsnp_handle* h, int32_t every) {
    if (!h || every < 0) { set_error("fsnp_set_verify: every must be >= 0 (0 = off)"); return 1; }
    if (every > 0 && (!h->planner.rowtile_ok || h->sb_tcn || h->generic_sb)) {
        set_error("fsnp_set_verify: this model has no exchange-free (one-tile-per-CU) kernel to verify against");
        return 2;
    }
    h->verify_every = every; h->verify_calls = 0;
    return 0;
}

int fsnp_set_verify_sample(fsnp_handle* h, int32_t every) {
    if (!h || every < 0) { set_error("fsnp_set_verify_sample: every must be >= 0 (0 = off)"); return 1; }
    if (every == h->vs_every) return 0;            // (idempotent: a binding may state its setting in front of every forward)
    h->vs_every = every; h->vs_calls = 0;
    return 0;
}

int64_t fsnp_verify_count(const fsnp_handle* h) { return h ? (int64_t)h->verify_runs : -1; }

}  // extern "C"
