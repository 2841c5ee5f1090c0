// window_stream.hip - the three kernels of a window session (window_stream.h; include/session/fsnp_window_stream.h; DESIGN.md
// section 8g) around the windowed call's pad kernel and the model: append the caller's block to the slots' input histories, emit the
// call's output rows from the pending samples and the newly staged windows, move the histories on.  Plain bandwidth kernels in the
// style of windowed.hip: one thread per sample, coalesced along a row, one workgroup inside one slot's row (blockIdx.y) so that a
// wave's clipped count belongs to one slot.  32-bit indices inside a record (W + max_samples < 2^30); 64-bit addresses on the
// caller's buffers (pcm.h) and into the staging rows.
#include "fsnp_common.h"
#include "pcm.h"
#include "window_stream.h"

namespace fsnp {

static_assert(sizeof(StreamRows) + kWindowArgRoom <= kKernelArgBytes, "a row table and the launch's other arguments must fit the kernel-argument block");

template <int FMT>
__global__ __launch_bounds__(256) void window_append_kernel(StreamState st, PcmIn wav, int slot0, StreamRows rows) {
    const int r = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    const StreamRow w = rows.v[r];
    if (j >= w.c) return;                                         // (the input is never read past the slot's count)
    st.hist[((long)(slot0 + r) * 2 + w.par) * st.HC + w.fill + j] = pcm_load<FMT>(wav, r, j);
}

void launch_window_append(const StreamState& st, const PcmIn& wav, const StreamRow* rows, int slots, hipStream_t s) {
    for (int b0 = 0; b0 < slots; b0 += kStreamRows) {
        const int cnt = slots - b0 < kStreamRows ? slots - b0 : kStreamRows;
        StreamRows t{};
        int most = 0;
        for (int r = 0; r < cnt; ++r) { t.v[r] = rows[b0 + r]; most = t.v[r].c > most ? t.v[r].c : most; }
        if (most == 0) continue;
        const dim3 grid((unsigned)((most + 255) / 256), cnt);
        const PcmIn in = pcm_rows(wav, b0);
#define FSNP_CALL(F) hipLaunchKernelGGL((window_append_kernel<F>), grid, dim3(256), 0, s, st, in, b0, t)
        FSNP_PCM_SWITCH2(wav.fmt, FSNP_CALL);
#undef FSNP_CALL
    }
}

// Sample u >= 0 of the slot's merged new rows: window k = min(u / S, m - 1) of them, j = u - k S.  Outside an overlap it is y_k[j]; for
// j < V of a window with a predecessor the cross-fade fmaf(g[j], y_k[j] - a, a), a = the predecessor's sample S + j: of the row
// before, or for the first new row of the kept tail.  m = 0 (a finish whose last window the pushes ran): what is left is that tail.
__device__ __forceinline__ float window_stream_merged(const StreamRow& w, int u, const float* __restrict__ stage, const float* __restrict__ g,
                                                      const float* __restrict__ tail, int W, int V) {
    if (w.m == 0) return tail[u];
    const int S = W - V;
    int k = u / S;
    if (k > w.m - 1) k = w.m - 1;
    const int j = u - k * S;
    const float* row = stage + ((long)w.first + k) * W;
    float v = row[j];
    if (j < V && (k > 0 || w.fade0)) {
        const float a = k > 0 ? (row - W)[S + j] : tail[j];
        v = fmaf(g[j], v - a, a);
    }
    return v;
}

// blockIdx.x < out_blocks: output column i of the slot's row.  The blocks behind them (a push in which some slot has new windows):
// index q of [0, S) = the slot's new pending sample q, of [S, W) = sample q - S of its new tail, both into the halves 1 - par.
template <int FMT>
__global__ __launch_bounds__(256) void window_emit_kernel(StreamState st, const float* __restrict__ stage, const float* __restrict__ g, PcmOut out,
                                                          int ncols, int out_blocks, int slot0, StreamRows rows) {
    const int r = blockIdx.y;
    const StreamRow w = rows.v[r];
    const int W = st.W, V = st.V, S = W - V;
    const long slot = slot0 + r;
    const float* pend = st.pend + (slot * 2 + w.par) * S;
    const float* tail = st.tail + (slot * 2 + w.par) * V;
    if ((int)blockIdx.x < out_blocks) {
        const int i = blockIdx.x * 256 + threadIdx.x;
        float v = 0.0f;
        if (i >= w.lead && i < w.cnt) {
            const int e = i - w.lead;
            v = e < w.pcount ? pend[w.pend_off + e] : window_stream_merged(w, e - w.pcount, stage, g, tail, W, V);
        }
        pcm_store<FMT>(out, r, i, v, i < ncols);
        if (i == 0 && (w.c > 0 || w.fin)) st.count[slot] = w.total;      // (a finish: 0)
        return;
    }
    if (w.m == 0 || w.fin) return;
    const int q = ((int)blockIdx.x - out_blocks) * 256 + threadIdx.x;
    if (q < S) {
        if (q < w.npc) st.pend[(slot * 2 + (1 - w.par)) * S + q] = window_stream_merged(w, w.u0 + q, stage, g, tail, W, V);
    } else if (q < W) {
        st.tail[(slot * 2 + (1 - w.par)) * V + (q - S)] = stage[((long)w.first + w.m - 1) * W + q];
    }
}

void launch_window_emit(const StreamState& st, const float* stage, const float* g, const PcmOut& out, const StreamRow* rows, int slots,
                        int ncols, hipStream_t s) {
    for (int b0 = 0; b0 < slots; b0 += kStreamRows) {
        const int cnt = slots - b0 < kStreamRows ? slots - b0 : kStreamRows;
        StreamRows t{};
        bool rewrite = false;
        for (int r = 0; r < cnt; ++r) { t.v[r] = rows[b0 + r]; rewrite = rewrite || (t.v[r].m > 0 && !t.v[r].fin); }
        const int out_blocks = (ncols + 255) / 256;
        const dim3 grid((unsigned)(out_blocks + (rewrite ? (st.W + 255) / 256 : 0)), cnt);
        const PcmOut o = pcm_rows(out, b0);
#define FSNP_CALL(F) hipLaunchKernelGGL((window_emit_kernel<F>), grid, dim3(256), 0, s, st, stage, g, o, ncols, out_blocks, b0, t)
        FSNP_PCM_SWITCH2(out.fmt, FSNP_CALL);
#undef FSNP_CALL
    }
}

__global__ __launch_bounds__(256) void window_compact_kernel(StreamState st, int S, int slot0, StreamRows rows) {
    const int r = blockIdx.y, q = blockIdx.x * 256 + threadIdx.x;
    const StreamRow w = rows.v[r];
    if (w.m == 0 || w.fin || q >= w.keep) return;
    float* hist = st.hist + (long)(slot0 + r) * 2 * st.HC;
    hist[(long)(1 - w.par) * st.HC + q] = hist[(long)w.par * st.HC + w.m * S + q];
}

void launch_window_compact(const StreamState& st, const StreamRow* rows, int slots, hipStream_t s) {
    for (int b0 = 0; b0 < slots; b0 += kStreamRows) {
        const int cnt = slots - b0 < kStreamRows ? slots - b0 : kStreamRows;
        StreamRows t{};
        int most = 0;
        for (int r = 0; r < cnt; ++r) {
            t.v[r] = rows[b0 + r];
            if (t.v[r].m > 0 && !t.v[r].fin && t.v[r].keep > most) most = t.v[r].keep;
        }
        if (most == 0) continue;
        hipLaunchKernelGGL(window_compact_kernel, dim3((unsigned)((most + 255) / 256), cnt), dim3(256), 0, s, st, st.W - st.V, b0, t);
    }
}

}  // namespace fsnp
