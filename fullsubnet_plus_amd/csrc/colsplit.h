// colsplit.h - what the column-split recurrent kernels (lstm_coop.hip, lstm_coopn.hip, lstm_coopw.hip, lstm_hp.hip, lstm_hpw.hip,
// lstm_fbv.hip) share around their k-loops and cells: the input plan of a row, the three forms of the hand-off over xchg_wait, and
// the Linear sum by column slice 0.  The exchange region's map is CoopRegion (lstm_common.h).  A kernel uses a
// helper only where hipcc's code for every instantiation keeps its figures (tools/asm_diff.py, profiles/colsplit_shared.md).
#pragma once
#include "fsnp_common.h"
#include "lstm_common.h"

namespace fsnp {

// ---- input plan of a row.  Offset of feature j of row rd at t = 0 from the base (dense input: a.dense, rows of a.dense_stride
// floats, rd.b = sequence; else the gathered sub-band input from a.att_mag), -1 = no source (the element is zero).
__device__ __forceinline__ int colsplit_input_offset(const LstmWeights& w, const LstmArgs& a, const RowDesc& rd, int j) {
    int off = -1;
    if (rd.valid && j < w.NIN) {
        if (a.dense != nullptr) off = rd.b * a.Tp * a.dense_stride + j;
        else off = sb_feature_offset(j, rd.f, rd.b * a.Tp * a.FP, a.F, a.NSBN, a.NFBN, a.fb_rel, a.fb_branch_stride);
    }
    return off;
}
// The row's norm source: one (mean, deviation) pair for all steps (md: the utterance's, md_utt; {0, 1} for dense input and for rows
// without a sequence) or a table with an entry per step (md_t != nullptr: of the row's sequence, md_seq, or of its slot, md_row -
// cumulative norms).
__device__ __forceinline__ void colsplit_norms(const LstmArgs& a, const RowDesc& rd, int slot, NormMD& md, const NormMD*& md_t) {
    const bool dense = a.dense != nullptr;
    md = NormMD{0.0f, 1.0f};
    md_t = nullptr;
    if (rd.valid) {
        if (a.md_seq != nullptr) md_t = a.md_seq + (size_t)rd.b * a.Tp;                    // [sequence][t]
        else if (!dense && a.md_row != nullptr) md_t = a.md_row + (size_t)slot * a.Tp;     // [slot][t]
        else if (!dense) md = a.md_utt[rd.b];
    }
}

// ---- the hand-off (write-through protocol of lstm_common.h), each form once.
// Workgroup barrier over the S workgroups of a tile: every storing wave drains, __syncthreads, thread 0 arrives and waits for
// `target` arrivals.  Returns false (to every thread) once the launch is aborted: a peer never arrived (xchg_wait).
__device__ __forceinline__ bool wg_barrier(unsigned* bar, unsigned target, const LstmArgs& a, int tid, int& abort_s) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains its stores
    __syncthreads();
    if (tid == 0) {
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (!xchg_wait(bar, target, a.coop_abort, a.coop_err)) abort_s = 1;
    }
    __syncthreads();
    return abort_s == 0;
}
// The split form: arrive now, wait a phase later.  `early` = the counter as thread 0 read it at the end of the previous MFMA phase
// (wg_poll_early): in lockstep it is already complete, and the wait costs one __syncthreads instead of a fabric round trip.
__device__ __forceinline__ void wg_arrive(unsigned* bar, int tid) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");          // every storing wave drains its write-through stores
    __syncthreads();
    if (tid == 0) __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ unsigned wg_poll_early(const unsigned* bar, int tid) {
    return tid == 0 ? __hip_atomic_load(bar, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) : 0u;
}
__device__ __forceinline__ bool wg_wait(const unsigned* bar, unsigned target, unsigned early, const LstmArgs& a, int tid, int& abort_s) {
    if (tid == 0 && early < target && !xchg_wait(bar, target, a.coop_abort, a.coop_err)) abort_s = 1;
    __syncthreads();
    return abort_s == 0;
}
// The per-wave form: a wave whose stores have drained arrives through lane 0; lane 0 waits and the whole wave learns the outcome.
__device__ __forceinline__ void wave_arrive(unsigned* bar, int lane) {
    if (lane == 0) __hip_atomic_fetch_add(bar, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void wave_drain_arrive(unsigned* bar, int lane) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    wave_arrive(bar, lane);
}
__device__ __forceinline__ bool wave_wait(const unsigned* bar, unsigned target, const LstmArgs& a, int lane) {
    int ok = 1;
    if (lane == 0) ok = xchg_wait(bar, target, a.coop_abort, a.coop_err) ? 1 : 0;
    return __builtin_amdgcn_readfirstlane(ok) != 0;
}
// `early` = the counter as the wave polled it ahead of the wait: complete in lockstep, and then the wait costs nothing
__device__ __forceinline__ bool wave_wait(const unsigned* bar, unsigned target, unsigned early, const LstmArgs& a, int lane) {
    if ((unsigned)__builtin_amdgcn_readfirstlane((int)early) >= target) return true;
    return wave_wait(bar, target, a, lane);
}

// ---- Linear(H, 2) of a finished step t_done: threads (row = tid & 31, output o = tid >> 5) of ONE workgroup per tile (the caller's
// condition, tid < 64) sum the P partials part[p][o][row] in a fixed order and store out[row's plane o][t_done - LA].
template <int P>
__device__ __forceinline__ void colsplit_fc_sum(const LstmWeights& w, const LstmArgs& a, const RowDesc* rows_s, const float* part,
                                                int t_done) {
    const int tid = threadIdx.x;
    const int row = tid & 31, o = tid >> 5;
    const RowDesc rd = rows_s[row];
    float sum = w.bfc[o];
    for (int p = 0; p < P; ++p) sum += xchg_load(part + p * 64 + o * 32 + row);
    if (rd.valid && t_done >= a.LA)
        a.out[(size_t)rd.out_off + (size_t)o * a.out_stride_o + (t_done - a.LA)] = apply_act(sum, a.act);
}

}  // namespace fsnp
