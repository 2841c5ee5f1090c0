// pcm.hip - the two kernels of include/fsnp_pcm.h that are not a load or a store of a kernel that touches samples anyway:
//   pcm_peak_scale_kernel   the second pass of FSNP_SAMPLE_S16_PEAK.  The overlap-add kernel (stft.hip, pcm_store<kPcmPeak>) has written
//                           every sample as fp32 into a staging row and folded |v| into the row's maximum; this one scales and truncates
//                           (pcm_peak_quantise: the reference CLI's np.int16(0.8 * 32767 * v / peak) in its own fp32 arithmetic).
//   pcm_convert_kernel      fsnp_debug_pcm_convert: exactly pcm_store<FMT> - the output conversion of the overlap-add kernels - on a
//                           caller's float buffer, because a test cannot make the model produce a tie or an overflow on demand.
// One workgroup works on one row (blockIdx.y), as in stft.hip.
#include "fsnp_common.h"
#include "pcm.h"

namespace fsnp {

__global__ __launch_bounds__(256) void pcm_peak_scale_kernel(const float* __restrict__ stage, long stage_stride,
                                                             const unsigned* __restrict__ peak, PcmOut out, int n) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    if (j >= n) return;
    static_cast<int16_t*>(out.p)[(long)b * out.stride + (long)j * out.step] =
        pcm_peak_quantise(stage[(long)b * stage_stride + j], __uint_as_float(peak[b]));
}

void launch_pcm_peak_scale(const float* stage, long stage_stride, const unsigned* peak, const PcmOut& out, int rows, int n, hipStream_t s) {
    for_row_chunks(rows, nullptr, n, [&](int b0, int r, auto) {      // (the chunks only: the grid's y extent)
        hipLaunchKernelGGL(pcm_peak_scale_kernel, dim3((unsigned)((n + 255) / 256), r), dim3(256), 0, s, stage + (long)b0 * stage_stride,
                           stage_stride, peak + b0, pcm_rows(out, b0), n);
    });
}

template <int FMT, typename LEN>
__global__ __launch_bounds__(256) void pcm_convert_kernel(const float* __restrict__ in, long in_stride, PcmOut out, int n, LEN len) {
    const int b = blockIdx.y, j = blockIdx.x * 256 + threadIdx.x;
    float v = 0.0f;
    if (j < row_len(len, b)) v = in[(long)b * in_stride + j];   // (row_len <= n)
    pcm_store<FMT>(out, b, j, v, j < n);
}

void launch_pcm_convert(const float* in, long in_stride, const PcmOut& out, int rows, int n, const int* samples, hipStream_t s) {
    for_row_chunks(rows, samples, n, [&](int b0, int r, auto len) {
        const dim3 grid((unsigned)((n + 255) / 256), r);
        if (out.fmt == kPcmPeak)
            hipLaunchKernelGGL((pcm_convert_kernel<kPcmPeak, decltype(len)>), grid, dim3(256), 0, s, in + (long)b0 * in_stride, in_stride, pcm_rows(out, b0), n, len);
        else
            hipLaunchKernelGGL((pcm_convert_kernel<kPcmS16, decltype(len)>), grid, dim3(256), 0, s, in + (long)b0 * in_stride, in_stride, pcm_rows(out, b0), n, len);
    });
}

}  // namespace fsnp
