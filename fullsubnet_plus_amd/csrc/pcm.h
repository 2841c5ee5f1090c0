// pcm.h - the sample formats of include/fsnp_pcm.h inside the kernels that touch samples (stft.hip, stft_stream.hip, pcm.hip): the
// conversion is part of their loads and stores.  One place for the arithmetic; the rules are the header's, restated in DESIGN.md ("PCM I/O").
// Compiled without fast-math (_build.py): the S16_PEAK division must be the IEEE fp32 one.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace fsnp {

// kernel-side format codes = the FSNP_SAMPLE_* values.  As the OUT format of an overlap-add kernel kPcmPeak is the first of the two
// passes: v goes to an fp32 staging row and |v| into the row's maximum; pcm_peak_scale_kernel (pcm.hip) writes the int16 samples.
constexpr int kPcmF32 = 0, kPcmS16 = 1, kPcmPeak = 2;

// a sample buffer: row b at element b * stride, sample j of it step elements further each (elements of the buffer's own type)
struct PcmIn {
    const void* p;
    long stride, step;
    int fmt;
};
struct PcmOut {
    void* p;               // kPcmPeak: the fp32 staging rows
    long stride, step;
    int fmt;
    int* clipped;          // optional [rows]: clipped samples per row, added to (zeroed stream-ordered in front)
    unsigned* peak;        // kPcmPeak: [rows] bit pattern of max |v| (non-negative floats order as unsigned integers), zeroed in front
};
inline PcmIn pcm_in_f32(const float* p, long stride) { return PcmIn{p, stride, 1, kPcmF32}; }
inline PcmOut pcm_out_f32(float* p, long stride) { return PcmOut{p, stride, 1, kPcmF32, nullptr, nullptr}; }
// rows further down the same buffers (launchers that take kLenRows rows per launch)
inline PcmIn pcm_rows(PcmIn v, long b0) {
    v.p = static_cast<const char*>(v.p) + b0 * v.stride * (v.fmt == kPcmF32 ? 4 : 2);
    return v;
}
inline PcmOut pcm_rows(PcmOut v, long b0) {
    v.p = static_cast<char*>(v.p) + b0 * v.stride * (v.fmt == kPcmS16 ? 2 : 4);
    if (v.clipped) v.clipped += b0;
    if (v.peak) v.peak += b0;
    return v;
}

#ifdef __HIPCC__
// sample j of row b.  Element-wide loads only: an int16 row may start at any 2-byte address.
template <int FMT>
__device__ __forceinline__ float pcm_load(const PcmIn& in, long b, long j) {
    const long at = b * in.stride + j * in.step;
    if constexpr (FMT == kPcmS16) return (float)static_cast<const int16_t*>(in.p)[at] * (1.0f / 32768.0f);      // exact in fp32
    else return static_cast<const float*>(in.p)[at];
}

// FSNP_SAMPLE_S16 out: round half to even, saturate, NaN -> 0; clip = it saturated or was NaN
__device__ __forceinline__ int16_t pcm_quantise(float v, bool& clip) {
    const float q = rintf(v * 32768.0f);
    clip = !(q >= -32768.0f && q <= 32767.0f);
    if (q != q) return 0;
    return (int16_t)(q > 32767.0f ? 32767 : q < -32768.0f ? -32768 : (int)q);
}
// FSNP_SAMPLE_S16_PEAK out: np.int16(0.8 * 32767 * v / peak) in fp32 - product rounded, IEEE division, truncation; peak 0 -> 0
__device__ __forceinline__ int16_t pcm_peak_quantise(float v, float peak) {
    if (!(peak > 0.0f)) return 0;
    const float q = (26213.6f * v) / peak;
    return q != q ? (int16_t)0 : (int16_t)(int)q;
}

// One sample out.  `live`: this thread has a sample (j < the row's columns).  With o.clipped (S16) or always (Peak) EVERY thread of the
// workgroup must get here, live or not, and all threads of a wave must be in row b: one wave reduction, at most one atomic per wave.
template <int FMT>
__device__ __forceinline__ void pcm_store(const PcmOut& o, int b, long j, float v, bool live) {
    const long at = (long)b * o.stride + j * o.step;
    if constexpr (FMT == kPcmF32) {
        if (live) static_cast<float*>(o.p)[at] = v;
    } else if constexpr (FMT == kPcmS16) {
        bool clip = false;
        const int16_t q = pcm_quantise(v, clip);
        if (live) static_cast<int16_t*>(o.p)[at] = q;
        if (o.clipped) {
            const unsigned long long m = __ballot(live && clip);
            if (m && (threadIdx.x & (warpSize - 1)) == 0) atomicAdd(o.clipped + b, __popcll(m));
        }
    } else {
        if (live) static_cast<float*>(o.p)[at] = v;
        float a = live ? fabsf(v) : 0.0f;                      // fmaxf drops a NaN operand: NaN samples take no part in the peak
        a = a != a ? 0.0f : a;
        for (int d = warpSize / 2; d > 0; d >>= 1) a = fmaxf(a, __shfl_xor(a, d));
        if (a > 0.0f && (threadIdx.x & (warpSize - 1)) == 0) atomicMax(o.peak + b, __float_as_uint(a));
    }
}
#endif

// kernel<..., FMT> for a runtime format (launchers)
#define FSNP_PCM_SWITCH2(fmt, CALL)                \
    do {                                           \
        if ((fmt) == ::fsnp::kPcmS16) { CALL(::fsnp::kPcmS16); } \
        else { CALL(::fsnp::kPcmF32); }            \
    } while (0)
#define FSNP_PCM_SWITCH3(fmt, CALL)                \
    do {                                           \
        if ((fmt) == ::fsnp::kPcmS16) { CALL(::fsnp::kPcmS16); } \
        else if ((fmt) == ::fsnp::kPcmPeak) { CALL(::fsnp::kPcmPeak); } \
        else { CALL(::fsnp::kPcmF32); }            \
    } while (0)

// pcm.hip
// int16 out[b][j] = pcm_peak_quantise(stage[b * stage_stride + j], peak[b]) for j < n: the second pass of FSNP_SAMPLE_S16_PEAK
void launch_pcm_peak_scale(const float* stage, long stage_stride, const unsigned* peak, const PcmOut& out /*kPcmS16 view*/, int rows, int n,
                           hipStream_t s);
// the output conversion of the overlap-add kernels on a float buffer in [rows][n] (fsnp_debug_pcm_convert): columns >= samples[b] as 0.
// out.fmt kPcmS16, or kPcmPeak = its first pass into out.p / out.peak
void launch_pcm_convert(const float* in, long in_stride, const PcmOut& out, int rows, int n, const int* samples, hipStream_t s);

}  // namespace fsnp
