// stft_stream.hip - the streaming halves of stft.hip (include/fsnp_wave_stream.h): samples in, samples out around one ring push.
//
// torch.stft(center=True, reflect) / torch.istft(length=L) of a clip that arrives in blocks, hop = n_fft / 2.  Frame t is centred at
// t * hop and covers samples [(t - 1) hop, (t + 1) hop): it is complete once (t + 1) hop samples have arrived (frame 0 reflects
// wav[1 .. hop] and needs hop + 1).  Output sample i = (fr[i / hop][hop + i % hop] + fr[i / hop + 1][i % hop]) / (the two w^2), so it
// needs the ENHANCED frames i / hop and i / hop + 1, and the mask of frame t is the model's output of step t + look_ahead: the push that
// brings input sample i + D, D = (2 + look_ahead) hop, always has them.  The two DFTs are the GEMMs of the whole-clip path
// (launch_linear_act with the handle's matrices) and what lies between them is a spectrum session's push (spec_push_body: |X|, the mag
// push, cIRM times the waiting spectrum); the two kernels here gather the frame rows in front of it and overlap-add behind it, and carry
// what a later push needs (layout: fsnp_common.h, WaveArgs).  {P, c} of every slot: c as a kernel argument, P from the slot's record
// (WaveMeta).
#include "fsnp_common.h"

namespace fsnp {

__device__ __forceinline__ unsigned char* wave_rec(const WaveArgs& a, int b) { return a.state + (size_t)b * a.stride; }

// one workgroup per slot; dynamic LDS: the old carry, n_fft + 1 floats (the carry is rewritten in place)
__global__ __launch_bounds__(256) void wave_gather_kernel(WaveArgs a, SlotCounts cnt, int fin_call, const float* __restrict__ wav,
                                                          long wav_stride, float* __restrict__ xfr) {
    extern __shared__ float old[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hop = a.hop, N = 2 * hop;
    float* carry = reinterpret_cast<float*>(wave_rec(a, b));
    long long* pc = reinterpret_cast<long long*>(wave_rec(a, b) + a.o_count);
    const long long P = *pc;
    const int c = fin_call ? 0 : cnt.v[b], fin = fin_call ? cnt.v[b] : 0;
    for (int i = tid; i <= N; i += 256) old[i] = carry[i];
    __syncthreads();
    if (tid == 0) {
        a.meta[b] = WaveMeta{P, c, fin};
        if (c > 0) *pc = P + c;
    }
    const WaveStep w = wave_step(P, c, fin, hop, a.LA);
    const long long total = P + c;
    const float* in = wav ? wav + (long)b * wav_stride : nullptr;
    // sample i of the clip, P - (n_fft + 1) <= i < P + c
    auto sample = [&](long long i) { return i < P ? old[(int)(i - P) + N + 1] : in[i - P]; };
    for (int idx = tid; idx < a.nrow * N; idx += 256) {
        const int j = idx / N, k = idx - j * N;
        float v = 0.0f;
        if (j < w.ks) {
            long long i = (w.nf + j - 1) * hop + k;
            if (i < 0) i = -i;                                         // torch "reflect": no edge repeat
            if (fin && i >= total) i = 2 * (total - 1) - i;            // (only the clip's last frame reaches past its end)
            v = sample(i);
        }
        xfr[((long)b * a.nrow + j) * N + k] = v;
    }
    if (c > 0)
        for (int i = tid; i <= N; i += 256) {
            const long long at = total - (N + 1) + i;
            carry[i] = at < 0 ? 0.0f : sample(at);
        }
}

void launch_wave_gather(const WaveArgs& a, const SlotCounts& c, int fin, const float* wav, long wav_stride, float* xfr, hipStream_t s) {
    hipLaunchKernelGGL(wave_gather_kernel, dim3(a.S), dim3(256), (size_t)(2 * a.hop + 1) * sizeof(float), s, a, c, fin, wav, wav_stride, xfr);
}

// one workgroup per slot; dynamic LDS: the old tail and the old fifo, hop floats each (both are rewritten in place).  The arithmetic of
// istft_ola_lengths_kernel: both frames' terms where the second frame exists, the last frame alone behind (T_b - 1) hop, den > 1e-11
__global__ __launch_bounds__(256) void wave_ola_kernel(WaveArgs a, const float* __restrict__ fr, const float* __restrict__ window,
                                                       float* __restrict__ out, long out_stride, int ncols) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hop = a.hop, N = 2 * hop;
    float* s_tail = lds;
    float* s_fifo = lds + hop;
    float* tail = reinterpret_cast<float*>(wave_rec(a, b) + a.o_tail);
    float* fifo = reinterpret_cast<float*>(wave_rec(a, b) + a.o_fifo);
    const WaveMeta m = a.meta[b];
    const WaveStep w = wave_step(m.p, m.c, m.fin, hop, a.LA);
    const long long D = (long long)(2 + a.LA) * hop;
    const long long e_old = w.e_old, e_new = e_old + w.ke;
    const long long done_old = e_old > 0 ? (e_old - 1) * hop : 0;      // samples finished before this call
    const long long sent_old = m.p > D ? m.p - D : 0;                  // samples emitted before this call: the fifo holds [sent_old, done_old)
    for (int i = tid; i < hop; i += 256) { s_tail[i] = tail[i]; s_fifo[i] = fifo[i]; }
    __syncthreads();
    auto frame = [&](long long e) { return fr + ((long)b * a.nrow + (e - e_old + w.j0)) * N; };      // row j = step j = frame nf + j - LA
    auto sample = [&](long long i) -> float {                          // sent_old <= i < (finish: L, else) (e_new - 1) hop
        if (i < done_old) return s_fifo[(int)(i - sent_old)];
        const long long t0 = i / hop, t1 = t0 + 1;
        const int r = (int)(i - t0 * hop);
        float num = 0.0f, den = 0.0f;
        if (t1 < e_new) {
            num += frame(t1)[r];
            den += window[r] * window[r];
        }
        num += t0 < e_old ? s_tail[r] : frame(t0)[hop + r];
        den += window[hop + r] * window[hop + r];
        return den > 1e-11f ? num / den : 0.0f;
    };
    const int valid = m.fin ? (int)D : m.c;
    const long long first = m.p - D;
    for (int j = tid; j < ncols; j += 256) {
        float v = 0.0f;
        if (j < valid && first + j >= 0) v = sample(first + j);
        out[(long)b * out_stride + j] = v;
    }
    if (m.c > 0) {
        const long long sent_new = m.p + m.c > D ? m.p + m.c - D : 0;
        const long long done_new = e_new > 0 ? (e_new - 1) * hop : 0;
        for (int q = tid; q < hop; q += 256) {
            fifo[q] = sent_new + q < done_new ? sample(sent_new + q) : 0.0f;
            if (w.ke > 0) tail[q] = frame(e_new - 1)[hop + q];
        }
    }
}

void launch_wave_ola(const WaveArgs& a, const float* fr, const float* window, float* out, long out_stride, int ncols, hipStream_t s) {
    hipLaunchKernelGGL(wave_ola_kernel, dim3(a.S), dim3(256), (size_t)2 * a.hop * sizeof(float), s, a, fr, window, out, out_stride, ncols);
}

}  // namespace fsnp
