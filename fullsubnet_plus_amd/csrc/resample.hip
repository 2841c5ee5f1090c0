// resample.hip - the free-standing kernel of include/fsnp_resample.h and the host side of its filter.
//   resample_kernel      one thread per output sample, one workgroup per kResampleBlock outputs of ONE row (blockIdx.y), as in stft.hip,
//                        so that a wave's clipped count and peak belong to one row.  Samples come in through pcm_load<FMT> and go out
//                        through pcm_store<FMT> (pcm.h); the sum itself is resample_sample (resample.h), shared with the resampling
//                        pad kernel of stft.hip.  Tap rows are read from global memory: a table is at most 170 KB ([up][tpp] floats),
//                        every workgroup of a launch walks the same rows, so they stay in L2 and the per-CU vector cache; consecutive
//                        outputs of a decimating pair (up = 1) read one row at consecutive columns.
//   taps / table         the closed formula in double, rounded once to fp32.
#include <cmath>

#include "fsnp_common.h"
#include "resample.h"

namespace fsnp {

template <int IFMT, int OFMT, bool BACK, bool COPY, typename LEN>
__global__ __launch_bounds__(kResampleBlock) void resample_kernel(PcmIn in, PcmOut out, ResampleTable t, int cols, LEN len) {
    const int b = blockIdx.y;
    const long m = (long)blockIdx.x * kResampleBlock + threadIdx.x;
    const long nb = row_len(len, b);
    float v = 0.0f;
    if constexpr (COPY) {
        if (m < nb) v = pcm_load<IFMT>(in, b, m);
    } else {
        const long n_in = BACK ? (nb * t.down + t.up - 1) / t.up : nb;
        const long n_out = BACK ? nb : (nb * t.up + t.down - 1) / t.down;
        if (m < n_out) v = resample_sample<IFMT>(in, b, m, n_in, t);
    }
    pcm_store<OFMT>(out, b, m, v, m < cols);
}

void launch_resample(const PcmIn& in, const PcmOut& out, const ResampleTable& t, int B, const int* samples, int uniform, int cols, bool back,
                     hipStream_t s) {
    for_row_chunks(B, samples, uniform, [&](int b0, int rows, auto len) {
        const dim3 grid((unsigned)((cols + kResampleBlock - 1) / kResampleBlock), rows);
#define FSNP_LAUNCH(I, O, BK, CP) \
    hipLaunchKernelGGL((resample_kernel<I, O, BK, CP, decltype(len)>), grid, dim3(kResampleBlock), 0, s, pcm_rows(in, b0), pcm_rows(out, b0), t, cols, len)
#define FSNP_OUT(O)                                                       \
    do {                                                                  \
        if (in.fmt == kPcmS16) {                                          \
            if (!t.taps) FSNP_LAUNCH(kPcmS16, O, false, true);            \
            else if (back) FSNP_LAUNCH(kPcmS16, O, true, false);          \
            else FSNP_LAUNCH(kPcmS16, O, false, false);                   \
        } else {                                                          \
            if (!t.taps) FSNP_LAUNCH(kPcmF32, O, false, true);            \
            else if (back) FSNP_LAUNCH(kPcmF32, O, true, false);          \
            else FSNP_LAUNCH(kPcmF32, O, false, false);                   \
        }                                                                 \
    } while (0)
        FSNP_PCM_SWITCH3(out.fmt, FSNP_OUT);
#undef FSNP_OUT
#undef FSNP_LAUNCH
    });
}

// ---------------------------------------------------------------------------------------------- host: the filter
namespace {
double bessel_i0(double x) {              // power series sum ((x / 2)^k / k!)^2: converges for every x, 30 terms at x = 8.6
    const double y = 0.25 * x * x;
    double term = 1.0, sum = 1.0;
    for (int k = 1; k < 500; ++k) {
        term *= y / ((double)k * (double)k);
        sum += term;
        if (term < 1e-18 * sum) break;
    }
    return sum;
}
}  // namespace

void resample_build_taps(const ResamplePlan& p, float* taps) {
    const double pi = 3.14159265358979323846264338327950288;
    const int M = p.up > p.down ? p.up : p.down;
    const double i0b = bessel_i0(kResampleBeta);
    for (int i = 0; i <= p.half; ++i) {
        const double x = kResampleRho * (double)i / (double)M;
        const double sinc = i == 0 ? 1.0 : sin(pi * x) / (pi * x);
        const double r = (double)i / (double)p.half;
        const double w = bessel_i0(kResampleBeta * sqrt(1.0 - r * r > 0.0 ? 1.0 - r * r : 0.0)) / i0b;
        const float t = (float)((double)p.up * ((kResampleRho / (double)M) * sinc * w));
        taps[p.half + i] = t;
        taps[p.half - i] = t;
    }
}

void resample_build_table(const ResamplePlan& p, float* table) {
    std::vector<float> taps(2 * (size_t)p.half + 1);
    resample_build_taps(p, taps.data());
    for (int ph = 0; ph < p.up; ++ph)
        for (int col = 0; col < p.tpp; ++col) {
            const long i = ph + (long)(p.J - col) * p.up;
            table[(size_t)ph * p.tpp + col] = (i < -p.half || i > p.half) ? 0.0f : taps[(size_t)(p.half + i)];
        }
}

}  // namespace fsnp
