// windowed.hip - the two kernels of include/ext/fsnp_windowed.h (windowed.h): the pad kernel of the STFT reading
// windows where they lie in the caller's clips, and the cross-fade of the windows' enhanced rows into the caller's buffer.  Plain
// bandwidth kernels: one thread per sample, coalesced along a row.  As in stft.hip one workgroup works on one row (blockIdx.y), so
// that a wave's clipped count and peak belong to one clip.
#include <cmath>

#include "fsnp_common.h"
#include "pcm.h"
#include "windowed.h"

namespace fsnp {

static_assert(sizeof(WindowRows) + kWindowArgRoom <= kKernelArgBytes && sizeof(ClipRows) + kWindowArgRoom <= kKernelArgBytes,
              "a row table and the launch's other arguments must fit the kernel-argument block");

// stft_pad_kernel (stft.hip) with the row's samples taken from a window: torch "reflect" at the window's own ends (a window is longer
// than n_fft / 2, so one reflection lands inside it), zeros behind.  Addresses in 64-bit: a clip may hold hours of samples at a step.
template <int FMT>
__global__ __launch_bounds__(256) void stft_pad_window_kernel(PcmIn wav, float* __restrict__ xp, long xp_stride, int half, WindowRows rows) {
    const int r = blockIdx.y;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;      // index into row r of [n][window + 2 half (+ tail)]
    if (p >= xp_stride) return;
    const WindowRow w = rows.v[r];
    float v = 0.0f;
    if (p < w.len + 2 * half) {
        int j = (int)p - half;
        if (j < 0) j = -j;
        if (j >= w.len) j = 2 * (w.len - 1) - j;
        v = pcm_load<FMT>(wav, w.clip, (long)w.offset + j);
    }
    xp[(long)r * xp_stride + p] = v;
}

void launch_stft_pad_window(const PcmIn& wav, float* xp, long xp_stride, const WindowRow* rows, int n, int n_fft, hipStream_t s) {
    for (int r0 = 0; r0 < n; r0 += kWindowRows) {
        const int cnt = n - r0 < kWindowRows ? n - r0 : kWindowRows;
        WindowRows t{};
        for (int r = 0; r < cnt; ++r) t.v[r] = rows[r0 + r];
        const dim3 grid((unsigned)((xp_stride + 255) / 256), cnt);
#define FSNP_CALL(F) hipLaunchKernelGGL((stft_pad_window_kernel<F>), grid, dim3(256), 0, s, wav, xp + (long)r0 * xp_stride, xp_stride, n_fft / 2, t)
        FSNP_PCM_SWITCH2(wav.fmt, FSNP_CALL);
#undef FSNP_CALL
    }
}

// Sample i of clip b: window k = min(i / S, K - 1), j = i - k S.  Outside an overlap it is y_k[j]; in [k S, k S + V) of k > 0 the
// cross-fade fmaf(g[j], y_k[j] - y_{k-1}[S + j], y_{k-1}[S + j]).  Both reads are consecutive along i.
template <int FMT>
__global__ __launch_bounds__(256) void window_merge_kernel(const float* __restrict__ stage, const float* __restrict__ g, PcmOut out, int cols,
                                                           int W, int V, ClipRows clips) {
    const int b = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;      // (clip, sample)
    const ClipRow c = clips.v[b];
    const int S = W - V;
    float v = 0.0f;
    if (i < c.len) {
        int k = i / S;
        if (k > c.count - 1) k = c.count - 1;
        const int j = i - k * S;
        const float* row = stage + ((long)c.first + k) * W;
        v = row[j];
        if (k > 0 && j < V) {
            const float a = (row - W)[S + j];
            v = fmaf(g[j], v - a, a);
        }
    }
    pcm_store<FMT>(out, b, i, v, i < cols);
}

void launch_window_merge(const float* stage, const float* g, const PcmOut& out, const ClipRow* clips, int batch, int cols, int W, int V,
                         hipStream_t s) {
    for (int b0 = 0; b0 < batch; b0 += kMergeRows) {
        const int cnt = batch - b0 < kMergeRows ? batch - b0 : kMergeRows;
        ClipRows t{};
        for (int r = 0; r < cnt; ++r) t.v[r] = clips[b0 + r];
        const dim3 grid((unsigned)((cols + 255) / 256), cnt);
#define FSNP_CALL(F) hipLaunchKernelGGL((window_merge_kernel<F>), grid, dim3(256), 0, s, stage, g, pcm_rows(out, b0), cols, W, V, t)
        FSNP_PCM_SWITCH3(out.fmt, FSNP_CALL);
#undef FSNP_CALL
    }
}

void window_fade_table(int V, float* g) {
    const double pi = 3.14159265358979323846264338327950288;
    for (int j = 0; j < V; ++j) g[j] = (float)(0.5 - 0.5 * cos(pi * j / V));
}

}  // namespace fsnp
