// window_stream.h - include/session/fsnp_window_stream.h inside the library: the schedule (host arithmetic) and the three kernels of a
// window session around the windowed call's own (window_stream.hip; windowed.h).  DESIGN.md section 8g.
//
// A slot's record on the device, every part in two halves of which `par` names the current one (a launch that rewrites a part reads
// one half and writes the other, so no workgroup depends on another's order; the host flips `par` when it has enqueued such a launch):
//   hist  [2][HC]  input samples from the start of the slot's first incomplete window, HC = W + max_samples
//   pend  [2][S]   merged samples not yet due, the oldest at pend_off (a push that completes no window only moves pend_off)
//   tail  [2][V]   samples [S, W) of the newest enhanced window, not yet faded into its successor
//   count          int64 samples pushed (the host's mirror decides everything; this one travels with get_state)
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "pcm.h"
#include "windowed.h"

namespace fsnp {

// windows complete on a slot that holds P >= 0 samples: window k is complete at k S + W
inline long windows_complete(long P, int W, int V) { return P < W ? 0 : (P - W) / (W - V) + 1; }

// one slot in one call: host values as a kernel argument (the WindowRows pattern of windowed.h), kStreamRows slots per launch
struct StreamRow {
    long long total;  // samples pushed after this call, 0 after a finish (written to the record's count for a slot the call gives samples or ends)
    int c;            // samples the push appends (0: a finish, or a slot this call leaves untouched)
    int fill;         // samples in hist before the call
    int par;          // the record's current halves
    int m;            // windows this call runs for the slot: staging rows first ... first + m - 1, W floats each
    int first;
    int fade0;        // the first of them fades in over the kept tail (the slot has an earlier window)
    int lead;         // leading output columns before the clip's first sample: exact zeros
    int cnt;          // output columns the slot gets, `lead` included; exact zeros from there on (0: the whole row)
    int pcount;       // pending samples, at pend[par][pend_off ...]; output column lead + e is pending sample e while e < pcount,
    int pend_off;     //   else sample u = e - pcount of the merged new rows (m = 0, a finish with no window left: of the tail)
    int u0, npc;      // a push with m > 0: the new pending samples are merged samples u0 ... u0 + npc - 1 of the new rows
    int keep;         //   and hist keeps its samples [m S, m S + keep)
    int fin;          // a finish: of the record only the count is rewritten, as 0 (which is the slot's reset)
};
constexpr int kStreamRows = (kKernelArgBytes - kWindowArgRoom) / (int)sizeof(StreamRow);
struct StreamRows { StreamRow v[kStreamRows]; };

// the device side of a session: slot b's parts at hist + b * 2 HC, pend + b * 2 S, tail + b * 2 V, count + b
struct StreamState {
    float *hist, *pend, *tail;
    long long* count;
    int HC, W, V;
};

// hist[par][fill + j] = sample j of the caller's row, j < c
void launch_window_append(const StreamState& st, const PcmIn& wav, const StreamRow* rows, int slots, hipStream_t s);
// the call's output rows [slots][ncols] from the pending samples and the staged rows cross-faded over the kept tail (the formula and
// operand order of window_merge_kernel); a push with new windows also writes the other halves of pend and tail; the count of every slot that got samples or ended
void launch_window_emit(const StreamState& st, const float* stage, const float* g, const PcmOut& out, const StreamRow* rows, int slots,
                        int ncols, hipStream_t s);
// hist[1 - par][q] = hist[par][m S + q], q < keep, for the slots whose windows ran
void launch_window_compact(const StreamState& st, const StreamRow* rows, int slots, hipStream_t s);

}  // namespace fsnp
