// windowed.h - include/ext/fsnp_windowed.h inside the library: the window plan (host arithmetic) and the two kernels around the model
// (windowed.hip).  A clip is cut into windows of W samples that overlap by V (stride S = W - V), every window is enhanced as a clip of
// its own into an fp32 staging row, and the merge kernel cross-fades the rows into the caller's buffer.  DESIGN.md section 8f.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "pcm.h"

namespace fsnp {

// K of a clip of L >= 1 samples: 1 if L <= W, else ceil((L - V) / S).  Needs 1 <= V <= W / 2.
inline long window_count(long L, int W, int V) { return L <= W ? 1 : (L - V + (W - V) - 1) / (W - V); }

// Per-row tables travel as kernel arguments (no copy to the device, nothing to synchronise: the RowLengths pattern of fsnp_common.h),
// so a launch takes as many rows as fit the 4 KB of kernel arguments next to the launch's other arguments (kWindowArgRoom bytes kept
// for those and for the arguments the compiler appends).
constexpr int kKernelArgBytes = 4096, kWindowArgRoom = 384;
// one window: row `clip` of the caller's buffer, samples [offset, offset + len)
struct WindowRow { int clip, offset, len; };
constexpr int kWindowRows = (kKernelArgBytes - kWindowArgRoom) / (int)sizeof(WindowRow);
struct WindowRows { WindowRow v[kWindowRows]; };
// one clip: its first window's staging row, its samples, its windows
struct ClipRow { int first, len, count; };
constexpr int kMergeRows = (kKernelArgBytes - kWindowArgRoom) / (int)sizeof(ClipRow);
struct ClipRows { ClipRow v[kMergeRows]; };

// stft_pad_kernel per window: row r of xp [n][xp_stride] = window rows[r] of `wav`, read where it lies, reflect-padded by n_fft / 2 at
// the WINDOW's own ends, zeros behind it
void launch_stft_pad_window(const PcmIn& wav, float* xp, long xp_stride, const WindowRow* rows, int n, int n_fft, hipStream_t s);
// out row b = the cross-fade of clip b's staging rows stage[clips[b].first ...][W] by the fade table g [V]; exact zeros from the clip's
// length to `cols`.  out.fmt kPcmF32 / kPcmS16 (out.clipped added to) / kPcmPeak (first pass: fp32 rows in out.p, maxima in out.peak)
void launch_window_merge(const float* stage, const float* g, const PcmOut& out, const ClipRow* clips, int batch, int cols, int W, int V,
                         hipStream_t s);
// g[j] = 0.5 - 0.5 cos(pi j / V) in double, rounded to fp32
void window_fade_table(int V, float* g);
// a handle's table of one overlap: uploaded once, in stream order from `host`, kept until fsnp_destroy (launches in flight may read it)
struct WindowFade {
    int overlap = 0;
    std::vector<float> host;
    float* dev = nullptr;
};
constexpr int kWindowMaxFades = 8;

}  // namespace fsnp
