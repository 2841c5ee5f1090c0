// stft.hip - SURVEY.md 8(f-3), second half: the STFT / iSTFT around the model, so that the reference inferencer's
// whole inner loop (speech_enhance/fullsubnet_plus/inferencer/inferencer.py:142-158: torch_stft -> model -> cIRM ->
// torch_istft) is ONE C-ABI call on device buffers (fsnp_enhance_wave).
//
// Replaces audio_zen/acoustics/feature.py:10-31 (torch.stft(y, n_fft, hop, win, window=hann, return_complex=True), i.e.
// center=True, pad_mode="reflect", onesided, not normalised) and :34-56 (torch.istft(..., length=L)).
// With n_fft = 512 a DFT is a [frames x 512] x [512 x 514] fp32 GEMM - 66 MFLOP per 2 s clip, nothing next to the model -
// so both transforms run on the MFMA GEMM of tcn.hip with the (periodic hann) window folded into the DFT matrices:
//   STFT : xp = reflect-pad(wav, n_fft/2);  X[t][2f + {0,1}] = sum_n xp[t*hop + n] * w[n] * {cos, -sin}(2 pi f n / N)
//          (the A operand is the padded signal itself read with row stride hop: frames overlap in memory, no copy);
//          the output IS torch.stft's memory layout ([B][T][F] complex64).
//   iSTFT: fr[t][n] = w[n]/N * sum_f c_f (Re X cos - Im X sin),  c_0 = c_{N/2} = 1, else 2 (C2R semantics);
//          wav[i] = (sum_t fr[t][i + N/2 - t*hop]) / (sum_t w^2[i + N/2 - t*hop])   (torch.istft's envelope division).
// Geometry (include/fsnp_stft_geometry.h): n_fft = 2 (F - 1), window = periodic hann(n_fft), N/8 <= hop <= N/2 with hop % 4 == 0 (the A
// rows above are read as float4); T = 1 + L / hop frames, the reflect padding is N/2 whatever the hop.
// Samples come in and go out in the formats of include/fsnp_pcm.h (pcm.h): fp32 or int16, at any sample step, converted in the
// pad kernel's loads and the overlap-add kernel's stores.  One workgroup works on one row (blockIdx.y), so that a wave's clipped
// count and peak belong to one row.
#include <cmath>
#include <type_traits>

#include "fsnp_common.h"
#include "pcm.h"
#include "resample.h"

namespace fsnp {

// Clips of different lengths in one batch: row b is its own row_len(len, b) samples long.  The counts travel as a kernel argument (LEN =
// RowLengths: no copy to the device, nothing to synchronise), kLenRows rows per launch; a batch of equal clips is the same kernel with
// the one count every row has (LEN = int).

// reflect padding at each row's own end (torch.stft of the clip alone), zeros behind it
template <int FMT, typename LEN>
__global__ __launch_bounds__(256) void stft_pad_kernel(PcmIn wav, float* __restrict__ xp, long xp_stride, int half, LEN len) {
    const int b = blockIdx.y;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;      // index into row b of [B][L + 2 half (+ tail)]
    if (p >= xp_stride) return;
    const int L = row_len(len, b);
    float v = 0.0f;
    if (p < L + 2 * half) {
        int j = (int)p - half;                                 // torch "reflect": no edge repeat
        if (j < 0) j = -j;
        if (j >= L) j = 2 * (L - 1) - j;
        v = pcm_load<FMT>(wav, b, j);
    }
    xp[(long)b * xp_stride + p] = v;
}

void launch_stft_pad(const PcmIn& wav, float* xp, long xp_stride, int B, int L, const int* samples, int n_fft, hipStream_t s) {
    for_row_chunks(B, samples, L, [&](int b0, int rows, auto len) {
        const dim3 grid((unsigned)((xp_stride + 255) / 256), rows);
#define FSNP_CALL(F) hipLaunchKernelGGL((stft_pad_kernel<F, decltype(len)>), grid, dim3(256), 0, s, pcm_rows(wav, b0), xp + (long)b0 * xp_stride, xp_stride, n_fft / 2, len)
        FSNP_PCM_SWITCH2(wav.fmt, FSNP_CALL);
#undef FSNP_CALL
    });
}

// The resampling variant (include/fsnp_resample.h): the clip arrives at another rate, and the padded sample at model-rate index j - after
// the reflect rule - is the FIR sum resample_sample taken straight from the caller's buffer.  No model-rate copy of the clip is written.
// `len` counts samples at the caller's rate; row b is ceil(n_b up / down) model-rate samples long.
template <int FMT, typename LEN>
__global__ __launch_bounds__(256) void stft_pad_resample_kernel(PcmIn wav, float* __restrict__ xp, long xp_stride, int half, LEN len,
                                                                ResampleTable t) {
    const int b = blockIdx.y;
    const long p = (long)blockIdx.x * 256 + threadIdx.x;
    if (p >= xp_stride) return;
    const long n = row_len(len, b);
    const long L = (n * t.up + t.down - 1) / t.down;
    float v = 0.0f;
    if (p < L + 2 * half) {
        long j = p - half;
        if (j < 0) j = -j;
        if (j >= L) j = 2 * (L - 1) - j;
        v = resample_sample<FMT>(wav, b, j, n, t);
    }
    xp[(long)b * xp_stride + p] = v;
}

void launch_stft_pad_resample(const PcmIn& wav, float* xp, long xp_stride, int B, const int* samples, int uniform, int n_fft,
                              const ResampleTable& t, hipStream_t s) {
    for_row_chunks(B, samples, uniform, [&](int b0, int rows, auto len) {
        const dim3 grid((unsigned)((xp_stride + 255) / 256), rows);
#define FSNP_CALL(F) hipLaunchKernelGGL((stft_pad_resample_kernel<F, decltype(len)>), grid, dim3(256), 0, s, pcm_rows(wav, b0), xp + (long)b0 * xp_stride, xp_stride, n_fft / 2, len, t)
        FSNP_PCM_SWITCH2(wav.fmt, FSNP_CALL);
#undef FSNP_CALL
    });
}

// One output sample: overlap-add and envelope division over the frames t < T that cover it, t * hop - n_fft / 2 <= n < t * hop + n_fft / 2
// (up to ceil(n_fft / hop) <= 8 of them), divided by the same frames' w^2 with torch.istft's guard.  HALF (hop = n_fft / 2): at most two
// frames cover a sample; the arithmetic the default geometry has always had, kept as it was so that its results stay bit-identical.
template <bool HALF>
__device__ __forceinline__ float istft_ola_sample(const float* __restrict__ frames /*[T][n_fft] of one clip*/,
                                                  const float* __restrict__ window, int n, int T, int n_fft, int hop) {
    const int p = n + n_fft / 2;                               // position in the centre-padded signal
    float num = 0.0f, den = 0.0f;
    if constexpr (HALF) {
        const int t1 = p / hop, t0 = t1 - 1;
        if (t1 < T) {
            const int k = p - t1 * hop;
            num += frames[(long)t1 * n_fft + k];
            den += window[k] * window[k];
        }
        if (t0 >= 0 && t0 < T) {
            const int k = p - t0 * hop;
            num += frames[(long)t0 * n_fft + k];
            den += window[k] * window[k];
        }
    } else {
        const int thi = p / hop < T ? p / hop : T - 1;         // newest frame that starts at or before p
        const int tlo = p < n_fft ? 0 : (p - n_fft) / hop + 1; // oldest frame that still reaches p
        for (int t = thi; t >= tlo; --t) {
            const int k = p - t * hop;                         // 0 <= k < n_fft by the two bounds
            num += frames[(long)t * n_fft + k];
            den += window[k] * window[k];
        }
    }
    return den > 1e-11f ? num / den : 0.0f;
}

// Row b's samples n < L_b = row_len(len, b), samples past them written as 0 (up to the L columns of the batch).  The frames a row sums
// are a fact of their own, not a function of its sample count.  Clips of different lengths (LEN = RowLengths): row b sums its own
// 1 + L_b / hop frames (torch.istft(..., length=) of the clip alone: frame T_b, which still overlaps the clip's last samples, is not
// part of it).  Equal clips (LEN = int): every row sums all T frames the caller gave, which may be more than 1 + L / hop (fsnp_istft)
// and then reach into the clip's last samples.
template <bool HALF, int FMT, typename LEN>
__global__ __launch_bounds__(256) void istft_ola_kernel(const float* __restrict__ frames, const float* __restrict__ window, PcmOut wav,
                                                        int T, int L, int n_fft, int hop, LEN len) {
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;      // (row, sample)
    const int Lb = row_len(len, b), Tb = std::is_same<LEN, RowLengths>::value ? 1 + Lb / hop : T;
    float v = 0.0f;
    if (n < Lb) v = istft_ola_sample<HALF>(frames + (long)b * T * n_fft, window, n, Tb, n_fft, hop);
    pcm_store<FMT>(wav, b, n, v, n < L);
}

void launch_istft_ola(const float* frames, const float* window, const PcmOut& wav, int B, int T, int L, const int* samples, int n_fft,
                      int hop, hipStream_t s) {
    for_row_chunks(B, samples, L, [&](int b0, int rows, auto len) {
        const dim3 grid((unsigned)((L + 255) / 256), rows);
        const float* fr = frames + (long)b0 * T * n_fft;
#define FSNP_CALL(F)                                                                                                                     \
    if (2 * hop == n_fft) hipLaunchKernelGGL((istft_ola_kernel<true, F, decltype(len)>), grid, dim3(256), 0, s, fr, window, pcm_rows(wav, b0), T, L, n_fft, hop, len); \
    else hipLaunchKernelGGL((istft_ola_kernel<false, F, decltype(len)>), grid, dim3(256), 0, s, fr, window, pcm_rows(wav, b0), T, L, n_fft, hop, len)
        FSNP_PCM_SWITCH3(wav.fmt, FSNP_CALL);
#undef FSNP_CALL
    });
}

// Host: GEMM operands (zero padded as tcn_gemm_kernel expects: rows to a multiple of 384, K to a multiple of 16).  They depend on n_fft
// only, not on the hop.
//   fwd [2F pad 384][n_fft pad 16]: row 2f = w[n] cos(2 pi f n / N), row 2f+1 = -w[n] sin(2 pi f n / N)
//   inv [n_fft pad 384][2F pad 16]: row n, column 2f = c_f w[n] cos(2 pi f n / N) / N, column 2f+1 = -c_f w[n] sin(...) / N
void stft_build_matrices(int n_fft, float* fwd, float* inv, float* window) {
    const int F = n_fft / 2 + 1, N2 = 2 * F;
    const int kp = (N2 + 15) / 16 * 16, np = (n_fft + 15) / 16 * 16;
    const double two_pi = 6.283185307179586476925286766559;
    for (int n = 0; n < n_fft; ++n) window[n] = (float)(0.5 - 0.5 * cos(two_pi * n / n_fft));   // torch.hann_window (periodic)
    for (int f = 0; f < F; ++f)
        for (int n = 0; n < n_fft; ++n) {
            const long ph = ((long)f * n) % n_fft;             // exact phase reduction
            const double c = cos(two_pi * ph / n_fft), sn = sin(two_pi * ph / n_fft);
            const double w = 0.5 - 0.5 * cos(two_pi * n / n_fft);
            fwd[(size_t)(2 * f) * np + n] = (float)(w * c);
            fwd[(size_t)(2 * f + 1) * np + n] = (float)(-w * sn);
            const double cf = (f == 0 || f == n_fft / 2) ? 1.0 : 2.0;
            inv[(size_t)n * kp + 2 * f] = (float)(cf * w * c / n_fft);
            inv[(size_t)n * kp + 2 * f + 1] = (float)(-cf * w * sn / n_fft);
        }
}

}  // namespace fsnp
