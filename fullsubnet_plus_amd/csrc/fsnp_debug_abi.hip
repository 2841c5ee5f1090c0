// fsnp_debug_abi.hip - the test and tuning entry points of include/fsnp_debug.h: stage read-back, timing, plans and costs, the host
// planner over arbitrary chips, launch profiles, fault injection and debug switches, and the weight packers restated by the CPU tests.
// Host code only: they reach the forward's machinery through fsnp_handle.h.
#include <algorithm>
#include <string>

#include "fsnp_common.h"
#include "lstm_common.h"
#include "planner.h"
#include "fsnp_handle.h"
#include "weight_layouts.h"
#include "pcm.h"

static double lstm_flops_per_step(const fsnp_handle* h) {
    if (h->sb_tcn) return 8 * (2.0 * h->NIN * h->CH + 2.0 * h->CH * 3 + 2.0 * h->CH * h->NIN) + 2.0 * h->NIN * h->cfg.output_size;
    const double H = h->H, NIN = h->NIN, OUT = h->cfg.output_size, G = h->NG;
    return 2.0 * G * H * (NIN + H) + 2.0 * G * H * (2 * H) + 2.0 * H * OUT;
}
static double tcn_flops_per_frame(const fsnp_handle* h) {
    const double F = h->F, CH = h->CH;
    return h->NB * (2.0 * F * CH + 2.0 * CH * 3 + 2.0 * CH * F) + 2.0 * F * F;
}
static double fb_lstm_flops_per_frame(const fsnp_handle* h) {   // original FullSubNet: LSTM(F, CH) x 2 + Linear(CH, F)
    const double F = h->F, CH = h->CH;
    return 2.0 * h->NG * CH * (F + CH) + 2.0 * h->NG * CH * (2 * CH) + 2.0 * CH * F;
}

extern "C" {

int fsnp_read_stage(fsnp_handle* h, const char* name, float* host_out, int64_t numel) {
    if (!h || !name || !host_out) { set_error("fsnp_read_stage: null argument"); return 1; }
    if (!h->have_last) { set_error("fsnp_read_stage: no forward has run"); return 2; }
    const Dims& d = h->last_dims;
    const Workspace& w = h->last_ws;
    const size_t plane = (size_t)d.B * d.Tp * d.FP;       // one branch, padded rows
    const std::string n = name;
    const float* src = nullptr;
    bool is_gate = false;
    static const char* tags[3] = {"mag", "real", "imag"};
    for (int b = 0; b < h->NFB; ++b) {
        if (n == std::string("att_") + tags[b]) src = reinterpret_cast<float*>(h->last_base + w.att) + b * plane;
        if (n == std::string("fb_") + tags[b]) src = reinterpret_cast<float*>(h->last_base + w.fb) + b * plane;
        if (h->NFB == 3 && n == std::string("gate_") + tags[b]) { src = reinterpret_cast<float*>(h->last_base + w.gate) + (size_t)b * d.B * d.FP; is_gate = true; }
    }
    if (n == "tcn0_mag") {
        if (!h->debug) { set_error("tcn0_mag needs FSNP_DEBUG_STAGES=1 at fsnp_create time"); return 2; }
        src = reinterpret_cast<float*>(h->last_base + w.dbg_tcn0);
    }
    if (!src) { set_error("unknown stage %s", name); return 2; }
    const int64_t rows = is_gate ? d.B : (int64_t)d.B * d.Tp;
    if (numel != rows * d.F) { set_error("stage %s has %lld elements, caller asked %lld", name, (long long)(rows * d.F), (long long)numel); return 2; }
    FSNP_ON_DEVICE(h);
    FSNP_HIP_CHECK(hipDeviceSynchronize());
    FSNP_HIP_CHECK(hipMemcpy2D(host_out, (size_t)d.F * 4, src, (size_t)d.FP * 4, (size_t)d.F * 4, (size_t)rows, hipMemcpyDeviceToHost));
    return 0;
}

int fsnp_set_timing(fsnp_handle* h, int32_t enable) {
    if (!h) { set_error("null handle"); return 1; }
    h->timing = enable != 0;
    return 0;
}

int fsnp_get_timing(fsnp_handle* h, double ms[4], int64_t count[4], int32_t reset) {
    if (!h || !ms || !count) { set_error("fsnp_get_timing: null argument"); return 1; }
    FSNP_ON_DEVICE(h);
    if (drain_timing(h)) return 1;
    for (int i = 0; i < 4; ++i) { ms[i] = h->acc_ms[i]; count[i] = h->acc_cnt[i]; }
    if (reset) for (int i = 0; i < 4; ++i) { h->acc_ms[i] = 0; h->acc_cnt[i] = 0; }
    return 0;
}

int fsnp_debug_plan_rows(int32_t num_rows, int32_t num_cus, int32_t hidden, int32_t gru, int32_t coop, double composite_gain,
                         int32_t* out, int32_t max_chunks) {
    return fsnp_debug_plan_rows2(num_rows, num_cus, hidden, gru, coop, composite_gain, 1, nullptr, out, max_chunks);
}

// the planner of a handle on a chip of num_cus CUs (host only): fsnp_create's kernels for an LSTM / GRU of 34 sub-band inputs, no switch set;
// test overrides: never the runtime-sized kernel, a one-tile-per-CU kernel at every size but gru = 1 (round-1 shape; gru = 2: the GRU with one)
static PlannerCtx host_ctx(int32_t num_cus, int32_t hidden, int32_t gru, int32_t coop, double composite_gain, int32_t workgroups_per_cu,
                           const double* costs) {
    PlannerSwitches sw;
    sw.lstm_coop = coop; sw.coop_occ = workgroups_per_cu >= 2 ? 2 : 1;
    PlannerCtx h;
    static_cast<PlannerOptions&>(h) = planner_options(gru ? FSNP_SEQ_GRU : FSNP_SEQ_LSTM, hidden, 34, false, sw);
    h.rowtile_ok = gru != 1;
    h.H = hidden; h.NIN = 34; h.num_cus = num_cus; h.num_cus_real = num_cus; h.gru = gru != 0; h.composite_gain = composite_gain;
    for (int i = 0; i < 4; ++i) h.occ_ksplit[i] = h.coop_occ;
    for (int i = 0; i < 2; ++i) h.occ_coopn[i] = h.coop_occ;
    h.cost = default_costs();
    if (costs) costs_from_array(h.cost, costs);
    if (gru == 2) h.cost.rowtile *= 0.75;
    return h;
}

int fsnp_debug_plan_rows2(int32_t num_rows, int32_t num_cus, int32_t hidden, int32_t gru, int32_t coop, double composite_gain,
                          int32_t workgroups_per_cu, const double* costs, int32_t* out, int32_t max_chunks) {
    if (!out || num_rows <= 0 || num_cus <= 0 || hidden < 128 || hidden % 128 != 0 || max_chunks <= 0) { set_error("fsnp_debug_plan_rows: bad argument"); return -1; }
    const PlannerCtx h = host_ctx(num_cus, hidden, gru, coop, composite_gain, workgroups_per_cu, costs);
    const SbPlan plan = plan_sb(h, num_rows);
    int n = 0;
    for (const SbChunk& c : plan.chunks) {
        if (n >= max_chunks) break;
        int32_t* o = out + 8 * n;
        o[0] = (int)c.kind; o[1] = c.row0; o[2] = c.nrows; o[3] = c.num_tiles; o[4] = c.ex; o[5] = c.kind == SbKind::KSplit || c.kind == SbKind::WaveOwned ? c.units : c.groups;
        o[6] = c.rpg; o[7] = c.slot0;
        ++n;
    }
    return n;
}

int fsnp_debug_coop_side_by_side(const int32_t a_per_xcd[8], int32_t a_own_cu, int32_t a_per_cu, const int32_t b_per_xcd[8],
                                 int32_t b_own_cu, int32_t b_per_cu, int32_t cus_per_xcd) {
    if (!a_per_xcd || !b_per_xcd) { set_error("fsnp_debug_coop_side_by_side: null argument"); return -1; }
    CoopFootprint a{}, b{};
    for (int x = 0; x < kNumXcds; ++x) {
        if (a_per_xcd[x] < 0 || b_per_xcd[x] < 0) { set_error("fsnp_debug_coop_side_by_side: negative workgroup count"); return -1; }
        a.per_xcd[x] = a_per_xcd[x]; b.per_xcd[x] = b_per_xcd[x];
    }
    a.own_cu = a_own_cu != 0; a.per_cu = a_per_cu; b.own_cu = b_own_cu != 0; b.per_cu = b_per_cu;
    return coop_side_by_side(a, b, cus_per_xcd) ? 1 : 0;
}

int fsnp_debug_fullsubnet_pairing(int32_t batch, int32_t num_cus, int32_t fb_workgroups_per_cu, const double* costs, int32_t* out,
                                  int32_t max_records) {
    if (!out || batch <= 0 || num_cus <= 0 || max_records <= 0) { set_error("fsnp_debug_fullsubnet_pairing: bad argument"); return -1; }
    const PlannerCtx c = host_ctx(num_cus, 384, 0, 1, 0.97, 1, costs);       // FullSubNet's sub-band model: LSTM, hidden 384
    const int per_cu[3] = {fb_workgroups_per_cu, fb_workgroups_per_cu, fb_workgroups_per_cu};
    return pipeline_pairing(c, true, 257, 512, batch, per_cu, batch <= 4, out, max_records);
}

int fsnp_debug_pipeline_pairing(const fsnp_handle* h, int32_t batch, int32_t* out, int32_t max_records) {
    if (!h || !out || batch <= 0 || max_records <= 0) { set_error("fsnp_debug_pipeline_pairing: bad argument"); return -1; }
    if (!h->committed) { set_error("fsnp_debug_pipeline_pairing: weights not committed (the decision depends on the kernels' occupancy)"); return -1; }
    if (h->model != FSNP_MODEL_FULLSUBNET || h->generic_fb || h->sb_tcn) return 0;      // no column-split launch on the caller's stream
    const bool valu = h->fb_valu && lstm_fbv_available(h->fbw, batch, h->num_cus_real);
    return pipeline_pairing(pctx(h), h->defer_small != 0, h->F, h->CH, batch, h->occ_fb, valu, out, max_records);
}

int fsnp_debug_fullband_launch(const fsnp_handle* h, int32_t batch, int32_t out[4]) {
    if (!h || !out || batch <= 0) { set_error("fsnp_debug_fullband_launch: bad argument"); return 1; }
    if (h->model != FSNP_MODEL_FULLSUBNET) { set_error("fsnp_debug_fullband_launch: FullSubNet+ has no full-band LSTM"); return 2; }
    const FbShape f = fb_shape(h, batch);
    out[0] = (int)f.kernel; out[1] = f.tiles; out[2] = f.rows_per_tile; out[3] = f.units;
    return 0;
}

int fsnp_debug_coop_chain_stats(fsnp_handle* h, int64_t out[2], int32_t reset) {
    if (!h || !out) { set_error("fsnp_debug_coop_chain_stats: null argument"); return 1; }
    take_coop_chain_stats(h, out, reset != 0);
    return 0;
}

int fsnp_get_costs(const fsnp_handle* h, double out[FSNP_NUM_COSTS], int32_t* calibrated, int32_t* occ) {
    if (!h || !out) { set_error("fsnp_get_costs: null argument"); return 1; }
    static_assert(kNumCosts == FSNP_NUM_COSTS, "planner.h and fsnp.h agree on the flat table");
    costs_to_array(h->planner.cost, out);
    if (calibrated) *calibrated = h->planner.cost.calibrated;
    if (occ) *occ = h->planner.coop_occ;
    return 0;
}

int fsnp_measure_costs(fsnp_handle* h, double out[FSNP_NUM_COSTS]) {
    if (!h || !out) { set_error("fsnp_measure_costs: null argument"); return 1; }
    if (!h->committed) { set_error("fsnp_measure_costs: weights not committed"); return 2; }
    if (h->sb_tcn) { set_error("fsnp_measure_costs: the sub-band model of this handle is a TCN (no recurrent kernels)"); return 2; }
    FSNP_ON_DEVICE(h);
    CostTable t = h->planner.cost;
    if (calibrate_costs(h, false, &t)) return 4;
    costs_to_array(t, out);
    return 0;
}

int fsnp_debug_set_costs(fsnp_handle* h, const double* costs, int32_t workgroups_per_cu) {
    if (!h || (workgroups_per_cu != 1 && workgroups_per_cu != 2)) { set_error("fsnp_debug_set_costs: bad argument"); return 1; }
    if (!h->committed) { set_error("fsnp_debug_set_costs: commit the weights first (the kernels' occupancy is checked then)"); return 2; }
    h->planner.cost = initial_costs(h->H, h->gru != 0, h->sb_tcn != 0);
    if (costs) costs_from_array(h->planner.cost, costs);
    h->planner.cost.calibrated = 1;          // pinned: the lazy calibration will not replace it
    h->planner.coop_occ = workgroups_per_cu;
    return 0;
}

int fsnp_describe_plan(const fsnp_handle* h, int32_t batch, int32_t mode, int32_t* out, int32_t max_chunks) {
    if (!h || !out || batch <= 0 || max_chunks <= 0) { set_error("fsnp_describe_plan: bad argument"); return -1; }
    const SbPlan plan = plan_sb(h, batch * rows_per_utt(h, mode));
    int n = 0;
    for (const SbChunk& c : plan.chunks) {
        if (n >= max_chunks) break;
        out[4 * n + 0] = describe_code(c.kind, h->sb_tcn != 0, h->lw.hp_wave && lstm_hpw_available(h->lw));
        out[4 * n + 1] = c.nrows; out[4 * n + 2] = c.num_tiles; out[4 * n + 3] = c.ex;
        ++n;
    }
    return n;
}

int fsnp_describe_plan_ex(const fsnp_handle* h, int32_t batch, int32_t mode, int32_t* out, int32_t max_chunks) {
    if (!h || !out || batch <= 0 || max_chunks <= 0) { set_error("fsnp_describe_plan_ex: bad argument"); return -1; }
    int32_t base[4 * 64];
    const int n = fsnp_describe_plan(h, batch, mode, base, max_chunks < 64 ? max_chunks : 64);
    if (n < 0) return n;
    const SbPlan plan = plan_sb(h, batch * rows_per_utt(h, mode));
    const int first_deferred = plan_first_deferred(h, plan);
    for (int i = 0; i < n; ++i) {
        const SbChunk& c = plan.chunks[i];
        for (int k = 0; k < 4; ++k) out[7 * i + k] = base[4 * i + k];
        // arithmetic of THIS chunk: the bf16 variants exist for the one-tile-per-CU LSTM kernel only (lstm.hip) and the half-tile kernel (lstm16.hip);
        // sequences that the plan hands to any other kernel run in fp32 whatever fsnp_set_precision says
        int prec = 0;
        if (!h->sb_tcn && !h->gru && c.kind == SbKind::RowTile) prec = h->ih_bf16 == 1 ? 1 : 0;
        if (!h->sb_tcn && !h->gru && c.kind == SbKind::HalfTile && h->ih_bf16 == 1 && h->lw.wpack16_bf) prec = 1;       // half-tile kernel: bf16 ih-GEMM too (round 4)
        out[7 * i + 4] = prec;
        out[7 * i + 5] = h->sb_tcn ? 0 : chunk_workgroups(h, c);
        out[7 * i + 6] = i >= first_deferred ? 1 : 0;        // the pipelined loop runs this launch on the side stream
    }
    return n;
}

int fsnp_debug_lstm_profile(fsnp_handle* h, const float* x, float* out, int32_t num_seq, int32_t steps,
                            uint64_t* host_stamps, int64_t num_stamps) {
    if (!h || !x || !out || !host_stamps) { set_error("fsnp_debug_lstm_profile: null argument"); return 1; }
    if (!h->committed) { set_error("fsnp_debug_lstm_profile: weights not committed"); return 2; }
    if (num_stamps != (int64_t)steps * 8) { set_error("fsnp_debug_lstm_profile: need steps*8 stamps"); return 2; }
    if (h->gru || h->sb_tcn || h->H != 384) { set_error("fsnp_debug_lstm_profile: row-tile kernel only (LSTM, hidden 384)"); return 2; }
    FSNP_ON_DEVICE(h);
    const LstmPlan lp = plan_lstm_tiles(num_seq, h->num_cus);
    const int num_slots = lp.num_tiles * lp.rows_per_slot_tile;
    const size_t stamp_off = align_up((size_t)num_slots * sizeof(RowDesc), 256);
    if (ensure_workspace(h, stamp_off + ((size_t)num_stamps + (size_t)lp.num_tiles * 256) * 8, nullptr)) return 4;
    FSNP_HIP_CHECK(hipDeviceSynchronize());
    RowDesc* rows = reinterpret_cast<RowDesc*>(h->ws);
    unsigned long long* dprof = reinterpret_cast<unsigned long long*>(h->ws + stamp_off);
    h->have_last = false;
    launch_build_rows(rows, {num_seq, lp.num_tiles, lp.rows_per_slot_tile, 0}, dense_rows(steps, 2), nullptr);
    LstmArgs a{};
    a.rows = rows; a.dense = x; a.out = out; a.out_stride_o = steps;
    a.num_rows = num_seq; a.num_tiles = lp.num_tiles; a.ex = lp.ex; a.Tp = steps; a.LA = 0; a.F = 1;
    a.act = h->cfg.sb_act; a.prof = dprof;
    launch_lstm(h->lw, a, 0);
    FSNP_HIP_CHECK(hipDeviceSynchronize());
    FSNP_HIP_CHECK(hipMemcpy(host_stamps, dprof, (size_t)num_stamps * 8, hipMemcpyDeviceToHost));
    return 0;
}

int fsnp_debug_pp_profile(fsnp_handle* h, const float* x, float* out, int32_t num_seq, int32_t steps, int32_t tiles_per_group,
                          uint64_t* host_stamps, int64_t num_stamps) {
    if (!h || !x || !out || !host_stamps) { set_error("fsnp_debug_pp_profile: null argument"); return 1; }
    if (!h->committed || (!h->planner.hp_ok && tiles_per_group == 0)) { set_error("fsnp_debug_pp_profile: no half-tile ping-pong kernel for this handle"); return 2; }
    // tiles_per_group: 0 = the half-tile ping-pong kernel (lstm_hp.hip: 2 halves x 16 stamps per step); 32 / 64 = the wave-owned column
    // split (lstm_coopw.hip) at that many units per workgroup (16 stamps per step: 8 per layer phase)
    const bool hp = tiles_per_group == 0, cw = tiles_per_group == 32 || tiles_per_group == 64 || tiles_per_group == 96;
    if ((!hp && !cw) || num_stamps != (int64_t)steps * (hp ? 32 : 16)) { set_error("fsnp_debug_pp_profile: tiles_per_group must be 0 (half-tile ping-pong kernel, steps * 32 stamps) or 32 / 64 (wave-owned column split, steps * 16 stamps)"); return 2; }
    if (cw && !h->planner.coopw_ok) { set_error("fsnp_debug_pp_profile: no wave-owned column split for this handle"); return 2; }
    const int tiles = cdiv(num_seq, 32), groups = tiles, S = hp ? h->H / 16 : h->H / tiles_per_group;
    if (num_seq <= 0 || groups * S > h->num_cus_real) { set_error("fsnp_debug_pp_profile: the launch must fit the chip"); return 2; }
    FSNP_ON_DEVICE(h);
    SbPlan plan;
    plan.chunks = {hp ? column_chunk(SbKind::HalfTilePingPong, 0, num_seq, tiles, 16, 0) : column_chunk(SbKind::WaveOwned, 0, num_seq, tiles, tiles_per_group, 0)};
    plan.total_slots = tiles * 32; plan.coop_tiles = tiles;
    const size_t rows_b = align_up((size_t)plan.total_slots * sizeof(RowDesc), 256), hx_b = align_up(lstm_coop_exchange_bytes(h->H, tiles), 256);
    const size_t bar_b = align_up(coop_counter_bytes(tiles), 256), st_b = (size_t)num_stamps * 8;
    if (order_after_last_forward(h, nullptr)) return 4;
    if (ensure_workspace(h, rows_b + hx_b + bar_b + 256 + st_b, nullptr)) return 4;
    FSNP_HIP_CHECK(hipDeviceSynchronize());
    h->have_last = false;
    RowDesc* rows = reinterpret_cast<RowDesc*>(h->ws);
    FSNP_HIP_CHECK(hipMemsetAsync(h->ws + rows_b, 0, hx_b + bar_b + 256 + st_b, nullptr));
    launch_build_rows(plan, rows, dense_rows(steps, h->cfg.output_size), nullptr);
    LstmArgs a{};
    a.rows = rows; a.dense = x; a.dense_stride = h->NIN; a.out = out; a.out_stride_o = steps;
    a.num_rows = num_seq; a.Tp = steps; a.LA = 0; a.FP = 0; a.F = 1; a.NSBN = 0; a.act = h->cfg.sb_act;
    a.prof = reinterpret_cast<unsigned long long*>(h->ws + rows_b + hx_b + bar_b + 256);
    launch_sb_lstm(h, plan, a, reinterpret_cast<float*>(h->ws + rows_b), reinterpret_cast<unsigned*>(h->ws + rows_b + hx_b),
                   reinterpret_cast<unsigned*>(h->ws + rows_b + hx_b + bar_b), nullptr);
    FSNP_HIP_CHECK(hipDeviceSynchronize());
    FSNP_HIP_CHECK(hipMemcpy(host_stamps, a.prof, st_b, hipMemcpyDeviceToHost));
    return fsnp_check_errors(h);
}

int fsnp_debug_launch_clock(fsnp_handle* h, double out[FSNP_LAUNCH_CLOCK_VALUES]) {
    if (!h || !out) { set_error("fsnp_debug_launch_clock: null argument"); return 1; }
    unsigned long long c[8] = {};
    if (!h->d_clk) { set_error("fsnp_debug_launch_clock: no completed launch of the one-tile-per-CU LSTM kernel on this handle"); return 2; }
    FSNP_ON_DEVICE(h);
    FSNP_HIP_CHECK(hipMemcpy(c, h->d_clk, sizeof(c), hipMemcpyDeviceToHost));
    const unsigned long long t0 = c[0], r0 = c[1], t1 = c[2], r1 = c[3];
    if (r0 == 0 || r1 <= r0 || t1 <= t0) { set_error("fsnp_debug_launch_clock: no completed launch of the one-tile-per-CU LSTM kernel on this handle"); return 2; }
    out[0] = (double)(t1 - t0); out[1] = (double)(r1 - r0);
    out[2] = (double)(r1 - r0) * 1e-5;                          // 100 MHz ticks -> ms
    out[3] = (double)(t1 - t0) / (double)(r1 - r0) * 100.0;     // s_memtime ticks per microsecond
    out[4] = (double)c[4] * 1e-5;                               // the slowest workgroup of the launch, ms
    out[5] = c[6] == ~0ull ? 0.0 : (double)c[6] * 1e-5;         // the fastest
    out[6] = (double)c[5];                                      // the largest s_memtime tick count of a workgroup
    return 0;
}

int fsnp_debug_verify_sample_stats(const fsnp_handle* h, int64_t out[3]) {
    if (!h || !out) { set_error("fsnp_debug_verify_sample_stats: null argument"); return 1; }
    out[0] = h->vs_runs; out[1] = h->vs_skipped; out[2] = h->vs_calls;
    return 0;
}

int fsnp_debug_corrupt_exchange(fsnp_handle* h, int32_t step) {
    if (!h || step < 0) { set_error("fsnp_debug_corrupt_exchange: step must be >= 0 (0 = off)"); return 1; }
    h->corrupt_exchange = step;
    return 0;
}

int fsnp_debug_inject_error(fsnp_handle* h) {
    if (!h) { set_error("null handle"); return 1; }
    *reinterpret_cast<volatile unsigned*>(h->d_err) |= kErrTimeout;
    return 0;
}

int fsnp_debug_set_chaos(fsnp_handle* h, int32_t seed) {
    if (!h) { set_error("null handle"); return 1; }
    h->coop_chaos = seed;
    return 0;
}

int fsnp_debug_set_gemm_dma(fsnp_handle* h, int32_t mode) {
    if (!h || mode < 0 || mode > 3) { set_error("fsnp_debug_set_gemm_dma: mode must be 0 (general GEMM kernel), 1 (DMA kernels where they apply), 2 (as 1, never the small-batch split-K kernel) or 3 (the 128-row DMA kernel only)"); return 1; }
    h->tw.gemm_dma = mode;
    return 0;
}

int fsnp_debug_set_lstm_coop(fsnp_handle* h, int32_t mode) {
    if (!h || mode < 0 || mode > 4 || mode == 3) { set_error("fsnp_debug_set_lstm_coop: mode must be 0 (off), 1 (auto), 2 (auto, serial K-split schedule, no half-tile ping-pong kernel) or 4 (auto + the half-tile ping-pong kernel even where FSNP_COOP_HP=0)"); return 1; }
    h->planner.lstm_coop = mode != 0;
    h->coop_skew = mode != 2;
    h->planner.coop_hp = mode == 4 ? 1 : mode == 1 ? h->coop_hp_cfg : 0;
    h->fb_valu = mode == 1 || mode == 4;   // (FullSubNet: modes 0 and 2 keep the full-band LSTM on the K-split kernel, whatever the batch - mode 0 is
                                           // what the sync error policy retries with after a time-out, so it must not come back to the same exchange)
    h->planner.cost.calibrated = h->calibrate ? 0 : h->planner.cost.calibrated;    // the K-split costs depend on the schedule: measure again
    if (!h->planner.cost.calibrated) h->planner.cost = initial_costs(h->H, h->gru != 0, h->sb_tcn != 0);
    return 0;
}

int fsnp_debug_set_lstm_waves(fsnp_handle* h, int32_t waves) {
    if (!h || (waves != 0 && waves != 4 && waves != 12)) { set_error("fsnp_debug_set_lstm_waves: waves must be 0 (auto), 4 or 12"); return 1; }
    h->lstm_waves = waves;
    h->lw.waves = waves;
    return 0;
}

int fsnp_debug_set_num_cus(fsnp_handle* h, int32_t num_cus) {
    if (!h || num_cus <= 0) { set_error("fsnp_debug_set_num_cus: bad argument"); return 1; }
    h->num_cus = num_cus;
    h->tw.num_cus = num_cus;
    return 0;
}

int fsnp_debug_lstm_pack(int32_t hidden, int32_t input_size, int32_t kx, int32_t waves, const float* wih0, const float* whh0,
                         const float* wih1, const float* whh1, float* out, int64_t out_floats) {
    if (!wih0 || !whh0 || !wih1 || !whh1 || !out) { set_error("fsnp_debug_lstm_pack: null argument"); return 1; }
    if (waves <= 0 || hidden % (32 * waves) != 0 || kx % 8 != 0 || input_size > kx) { set_error("fsnp_debug_lstm_pack: bad sizes"); return 2; }
    if (rnn_image_floats(PK_ROWTILE, hidden, input_size, kx, waves) != out_floats) {
        set_error("fsnp_debug_lstm_pack: need %lld floats", (long long)rnn_image_floats(PK_ROWTILE, hidden, input_size, kx, waves));
        return 2;
    }
    pack_rnn_host(PK_ROWTILE, hidden, input_size, kx, waves, wih0, whh0, wih1, whh1, out);
    return 0;
}

int fsnp_debug_lstm_coop_pack(int32_t hidden, int32_t input_size, int32_t kx, int32_t units, const float* wih0, const float* whh0,
                              const float* wih1, const float* whh1, float* out, int64_t out_floats) {
    if (!wih0 || !whh0 || !wih1 || !whh1 || !out) { set_error("fsnp_debug_lstm_coop_pack: null argument"); return 1; }
    if ((units != 8 && units != 16 && units != 32 && units != 64) || hidden % 64 != 0 || kx % 8 != 0 || input_size > kx) {
        set_error("fsnp_debug_lstm_coop_pack: bad sizes");
        return 2;
    }
    if (rnn_image_floats(PK_KSPLIT, hidden, input_size, kx, units) != out_floats) {
        set_error("fsnp_debug_lstm_coop_pack: need %lld floats", (long long)rnn_image_floats(PK_KSPLIT, hidden, input_size, kx, units));
        return 2;
    }
    pack_rnn_host(PK_KSPLIT, hidden, input_size, kx, units, wih0, whh0, wih1, whh1, out);
    return 0;
}

int fsnp_debug_lstm_hpw_pack(int32_t hidden, int32_t input_size, int32_t kx, const float* wih0, const float* whh0, const float* wih1,
                             const float* whh1, float* out, int64_t out_floats) {
    if (!wih0 || !whh0 || !wih1 || !whh1 || !out) { set_error("fsnp_debug_lstm_hpw_pack: null argument"); return 1; }
    if (hidden % 16 != 0 || kx % 4 != 0 || kx > 64 || input_size > kx) { set_error("fsnp_debug_lstm_hpw_pack: bad sizes"); return 2; }
    if (out_floats != rnn_image_floats(PK_HPW, hidden, input_size, kx, 0)) {
        set_error("fsnp_debug_lstm_hpw_pack: need %lld floats", (long long)rnn_image_floats(PK_HPW, hidden, input_size, kx, 0));
        return 2;
    }
    pack_rnn_host(PK_HPW, hidden, input_size, kx, 0, wih0, whh0, wih1, whh1, out);
    return 0;
}

int fsnp_debug_lstm_coopw_pack(int32_t hidden, int32_t input_size, int32_t kx, const float* wih0, const float* whh0, const float* wih1,
                               const float* whh1, float* out, int64_t out_floats) {
    if (!wih0 || !whh0 || !wih1 || !whh1 || !out) { set_error("fsnp_debug_lstm_coopw_pack: null argument"); return 1; }
    if (hidden % 32 != 0 || kx % 8 != 0 || input_size > kx) { set_error("fsnp_debug_lstm_coopw_pack: bad sizes"); return 2; }
    if (rnn_image_floats(PK_COOPW, hidden, input_size, kx, 0) != out_floats) {
        set_error("fsnp_debug_lstm_coopw_pack: need %lld floats", (long long)rnn_image_floats(PK_COOPW, hidden, input_size, kx, 0));
        return 2;
    }
    pack_rnn_host(PK_COOPW, hidden, input_size, kx, 0, wih0, whh0, wih1, whh1, out);
    return 0;
}

int fsnp_debug_lstm_fbv_pack(int32_t hidden, int32_t input_size, const float* wih0, const float* whh0, const float* wih1, const float* whh1,
                             float* out, int64_t out_floats) {
    if (!wih0 || !whh0 || !wih1 || !whh1 || !out) { set_error("fsnp_debug_lstm_fbv_pack: null argument"); return 1; }
    if (hidden != 512 || input_size < 1 || input_size > 288) { set_error("fsnp_debug_lstm_fbv_pack: hidden 512, <= 288 inputs"); return 2; }
    if (rnn_image_floats(PK_FBV, hidden, input_size, 0, 0) != out_floats) {
        set_error("fsnp_debug_lstm_fbv_pack: need %lld floats", (long long)rnn_image_floats(PK_FBV, hidden, input_size, 0, 0));
        return 2;
    }
    pack_rnn_host(PK_FBV, hidden, input_size, 0, 0, wih0, whh0, wih1, whh1, out);
    return 0;
}

double fsnp_lstm_flops(const fsnp_handle* h, int64_t num_seq, int32_t steps) {
    if (!h) return 0;
    return (double)num_seq * steps * lstm_flops_per_step(h);
}

double fsnp_forward_flops(const fsnp_handle* h, int32_t batch, int32_t frames, int32_t mode) {
    if (!h) return 0;
    const double Tp = frames + h->cfg.look_ahead;
    const double full_band = h->model == FSNP_MODEL_FULLSUBNET ? fb_lstm_flops_per_frame(h) : 3.0 * tcn_flops_per_frame(h);
    return batch * Tp * (rows_per_utt(h, mode) * lstm_flops_per_step(h) + full_band);
}

int fsnp_debug_weight_blob(fsnp_handle* h, void* host_dst, int64_t bytes, int64_t* needed) {
    if (!h) { set_error("fsnp_debug_weight_blob: null handle"); return 1; }
    if (!h->committed || !h->d_weights) { set_error("fsnp_debug_weight_blob: weights not committed"); return 2; }
    const int64_t need = (int64_t)(h->blob_floats * sizeof(float));
    if (needed) *needed = need;
    if (!host_dst) return 0;                      // (a size query)
    if (bytes < need) { set_error("fsnp_debug_weight_blob: need %lld bytes", (long long)need); return 2; }
    FSNP_ON_DEVICE(h);
    FSNP_HIP_CHECK(hipDeviceSynchronize());
    FSNP_HIP_CHECK(hipMemcpy(host_dst, h->d_weights, (size_t)need, hipMemcpyDeviceToHost));
    return 0;
}

const void* fsnp_debug_weight_blob_ptr(const fsnp_handle* h) { return h ? h->d_weights : nullptr; }

int fsnp_debug_commit_stats(const fsnp_handle* h, int64_t out[4]) {
    if (!h || !out) { set_error("fsnp_debug_commit_stats: null argument"); return 1; }
    for (int i = 0; i < 4; ++i) out[i] = h->commit_stats[i];
    return 0;
}

int fsnp_debug_pack_emulate(int32_t kind, const int32_t* sizes, int32_t num_sizes, const float* const* sources, const int64_t* numels,
                            int32_t num_sources, float* out, int64_t out_floats) {
    if (!sizes || !sources || !numels || !out) { set_error("fsnp_debug_pack_emulate: null argument"); return 1; }
    if (kind < 0 || kind >= PK_COUNT || num_sizes < 1 || num_sizes > 5) { set_error("fsnp_debug_pack_emulate: unknown kind / size count"); return 2; }
    int p[5] = {0, 0, 0, 0, 0};
    for (int i = 0; i < num_sizes; ++i) {
        if (sizes[i] < 0) { set_error("fsnp_debug_pack_emulate: negative size"); return 2; }
        p[i] = sizes[i];
    }
    const bool rnn = kind <= PK_SPREAD;
    const int want_sources = rnn ? 8 : kind == PK_FOLDW ? 2 : kind == PK_FOLDC ? 4 : 1;
    // the divisions of the layouts: a recurrent image is cut into whole fragments
    bool ok = p[0] > 0 && num_sources == want_sources;
    if (rnn && kind != PK_BIAS) ok = ok && p[1] > 0;
    if (kind <= PK_FBV) ok = ok && p[0] % 8 == 0;
    if (kind == PK_ROWTILE || kind == PK_ROWTILE_BF || kind == PK_GRU) ok = ok && p[3] > 0 && p[0] % (32 * p[3]) == 0 && p[2] % 8 == 0 && p[1] <= p[2];
    if (kind == PK_ROWTILE_BF) ok = ok && p[1] < p[2] && p[0] % 16 == 0;
    if (kind == PK_HALF || kind == PK_HALF_BF) ok = ok && p[0] % 64 == 0 && p[1] <= p[2];
    if (kind == PK_KSPLIT) ok = ok && p[3] >= 8 && p[3] % 8 == 0 && p[0] % p[3] == 0 && p[0] % 16 == 0 && (4 * p[3]) % 32 == 0 && p[2] % 8 == 0 && p[1] <= p[2] && (coop_kgxp(p[2]) + p[0] / 8) % 4 == 0;
    if (kind == PK_COOPN || kind == PK_COOPW) ok = ok && p[0] % 32 == 0 && p[2] % 8 == 0 && p[1] <= p[2];
    if (kind == PK_HP || kind == PK_HPW) ok = ok && p[0] % 16 == 0 && p[1] <= 16 * gx16(p[2]);
    if (kind == PK_FBV) ok = ok && p[0] == 512 && p[1] <= kFbvXP;
    if (kind == PK_SPREAD) ok = ok && p[3] < 4;
    if (kind == PK_PADMAT || kind == PK_FOLDW) ok = ok && p[1] > 0 && p[0] <= p[2] && p[1] <= p[3];
    if (kind == PK_TRANSPOSE) ok = ok && p[1] > 0;
    if (kind == PK_FOLDC) ok = ok && p[1] > 0 && p[0] <= p[2] && p[3] <= 1;
    if (!ok) { set_error("fsnp_debug_pack_emulate: bad sizes / source count for kind %d", kind); return 2; }
    PackJob J = make_job(kind, p[0], p[1], p[2], p[3], p[4]);
    if (J.n != out_floats) { set_error("fsnp_debug_pack_emulate: need %lld floats", (long long)J.n); return 2; }
    std::vector<float> arena;
    for (int i = 0; i < num_sources; ++i) {
        if (numels[i] < 0 || (numels[i] > 0 && !sources[i])) { set_error("fsnp_debug_pack_emulate: source %d is null / negative", i); return 1; }
        J.s[i] = (long long)arena.size();
        arena.insert(arena.end(), sources[i], sources[i] + numels[i]);
    }
    // every source offset the layout names lies inside its tensor
    auto inside = [&](int a, long long i) { return a < num_sources && i >= 0 && i < numels[a]; };
    if (kind == PK_FOLDC) {
        if (numels[0] < (int64_t)p[0] * p[1] || numels[1] < p[1] || numels[2] < p[1] || numels[3] < p[0]) {
            set_error("fsnp_debug_pack_emulate: a source of the fold is too small"); return 2;
        }
    } else {
        for (long long u = 0; 4 * u < J.n; ++u) {
            const int nj = pack_unit_bf16(J, u) ? 8 : 4;
            for (int j = 0; j < nj; ++j) {
                long long shift;
                const PackRef r = pack_ref(J, u, j, &shift);
                if (r.a < 0) continue;
                if (!inside(r.a, shift + r.ia) || (r.op != OP_ONE && !inside(r.b, shift + r.ib))) {
                    set_error("fsnp_debug_pack_emulate: kind %d, unit %lld: source offset outside its tensor", kind, u);
                    return 3;
                }
            }
        }
    }
    pack_image_host(J, arena.data(), out, J.n);
    return 0;
}

int fsnp_debug_pcm_convert(fsnp_handle* h, const float* dev_in, int16_t* dev_out, int32_t rows, int32_t n, const int32_t* samples,
                           int32_t out_format, int32_t* dev_clipped, void* stream) {
    if (!h || !dev_in || !dev_out) { set_error("fsnp_debug_pcm_convert: null argument"); return 1; }
    if (rows < 1 || n < 1) { set_error("fsnp_debug_pcm_convert: empty input"); return 2; }
    if (out_format != FSNP_SAMPLE_S16 && out_format != FSNP_SAMPLE_S16_PEAK) {
        set_error("fsnp_debug_pcm_convert: out_format %d is neither FSNP_SAMPLE_S16 nor FSNP_SAMPLE_S16_PEAK", (int)out_format);
        return 2;
    }
    for (int b = 0; samples && b < rows; ++b)
        if (samples[b] < 0 || samples[b] > n) { set_error("fsnp_debug_pcm_convert: row %d: %d samples outside [0, n = %d]", b, (int)samples[b], n); return 2; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    FSNP_ON_DEVICE(h);
    PcmOut out{dev_out, n, 1, kPcmS16, nullptr, nullptr};
    if (dev_clipped) FSNP_HIP_CHECK(hipMemsetAsync(dev_clipped, 0, (size_t)rows * 4, s));
    if (out_format == FSNP_SAMPLE_S16) {
        out.clipped = dev_clipped;
        launch_pcm_convert(dev_in, n, out, rows, n, samples, s);
    } else {
        // the two passes of the whole-clip call: fp32 staging rows and per-row maxima in the I/O area, then scale and truncate
        const size_t stage_b = align_up((size_t)rows * n * 4, 256);
        if (order_after_last_forward(h, s)) return 4;
        if (ensure_io(h, stage_b + (size_t)rows * 4, s)) return 4;
        float* stage = reinterpret_cast<float*>(h->io);
        unsigned* peak = reinterpret_cast<unsigned*>(h->io + stage_b);
        FSNP_HIP_CHECK(hipMemsetAsync(peak, 0, (size_t)rows * 4, s));
        launch_pcm_convert(dev_in, n, PcmOut{stage, n, 1, kPcmPeak, nullptr, peak}, rows, n, samples, s);
        launch_pcm_peak_scale(stage, n, peak, out, rows, n, s);
    }
    FSNP_HIP_CHECK(hipGetLastError());
    return mark_forward_done(h, s);
}

}  // extern "C"
