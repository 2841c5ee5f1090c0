// stft_stream.hip - the streaming halves of stft.hip (include/fsnp_wave_stream.h): samples in, samples out around one ring push.
//
// torch.stft(center=True, reflect) / torch.istft(length=L) of a clip that arrives in blocks, for the geometries of
// include/fsnp_stft_geometry.h: hop between frames, half = n_fft / 2.  Frame t is centred at t * hop and covers samples
// [t hop - half, t hop + half): it is complete once t hop + half samples have arrived (frame 0 reflects wav[1 .. half] and needs
// half + 1).  Output sample i is the sum of the ENHANCED frames that cover it, the newest of them frame (i + half) / hop, over the sum of
// their w^2; and the mask of frame t is the model's output of step t + look_ahead: the push that brings input sample i + D,
// D = n_fft + look_ahead * hop, always has them ((2 + look_ahead) hop in the default geometry).  With e enhanced frames the samples
// below e hop - half are finished, and the n_fft - hop samples behind them hold partial sums.  The two DFTs are the GEMMs of the
// whole-clip path (launch_linear_act with the handle's matrices) and what lies between them is a spectrum session's push
// (spec_push_body: |X|, the mag push, cIRM times the waiting spectrum); the two kernels here gather the frame rows in front of it and
// overlap-add behind it, and carry what a later push needs (layout: fsnp_common.h, WaveArgs).  {P, c} of every slot: c as a kernel
// argument, P from the slot's record (WaveMeta).  The caller's samples are read and written in the formats of include/fsnp_pcm.h
// (pcm.h), converted in the gather's loads and the overlap-add's stores; the records (carry, partial sums, fifo) are fp32 whatever the format.
#include "fsnp_common.h"
#include "pcm.h"

namespace fsnp {

__device__ __forceinline__ unsigned char* wave_rec(const WaveArgs& a, int b) { return a.state + (size_t)b * a.stride; }

// one workgroup per slot; dynamic LDS: the old carry, n_fft + 1 floats (the carry is rewritten in place)
template <int FMT>
__global__ __launch_bounds__(256) void wave_gather_kernel(WaveArgs a, SlotCounts cnt, int fin_call, PcmIn wav, float* __restrict__ xfr) {
    extern __shared__ float old[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hop = a.hop, half = a.half, N = 2 * half;
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
    const WaveStep w = wave_step(P, c, fin, hop, half, a.LA);
    const long long total = P + c;
    // sample i of the clip, P - (n_fft + 1) <= i < P + c (a finish has no input and c = 0)
    auto sample = [&](long long i) { return i < P ? old[(int)(i - P) + N + 1] : pcm_load<FMT>(wav, b, (long)(i - P)); };
    for (int idx = tid; idx < a.nrow * N; idx += 256) {
        const int j = idx / N, k = idx - j * N;
        float v = 0.0f;
        if (j < w.ks) {
            long long i = (w.nf + j) * hop - half + k;
            if (i < 0) i = -i;                                         // torch "reflect": no edge repeat
            if (fin && i >= total) i = 2 * (total - 1) - i;            // (only the frames a finish adds reach past the clip's end)
            v = sample(i);
        }
        xfr[((long)b * a.nrow + j) * a.xl + k] = v;
    }
    if (c > 0)
        for (int i = tid; i <= N; i += 256) {
            const long long at = total - (N + 1) + i;
            carry[i] = at < 0 ? 0.0f : sample(at);
        }
}

void launch_wave_gather(const WaveArgs& a, const SlotCounts& c, int fin, const PcmIn& wav, float* xfr, hipStream_t s) {
#define FSNP_CALL(F) hipLaunchKernelGGL(wave_gather_kernel<F>, dim3(a.S), dim3(256), (size_t)(2 * a.half + 1) * sizeof(float), s, a, c, fin, wav, xfr)
    FSNP_PCM_SWITCH2(wav.fmt, FSNP_CALL);
#undef FSNP_CALL
}

// one workgroup per slot; dynamic LDS: the old tail (n_fft - hop floats) and the old fifo (hop floats), both rewritten in place.  The
// arithmetic of istft_ola_sample: the covering frames from the newest to the oldest, the ones of earlier calls through the tail's partial
// sum, over the same frames' w^2, den > 1e-11.  At hop = half that is the two-frame sum the default geometry has always had, term by term.
template <int FMT>
__global__ __launch_bounds__(256) void wave_ola_kernel(WaveArgs a, const float* __restrict__ fr, const float* __restrict__ window,
                                                       PcmOut out /*no clipped count: every thread stores on its own*/, int ncols) {
    extern __shared__ float lds[];
    const int b = blockIdx.x, tid = threadIdx.x;
    const int hop = a.hop, half = a.half, N = 2 * half, NT = N - hop;
    float* s_tail = lds;
    float* s_fifo = lds + NT;
    float* tail = reinterpret_cast<float*>(wave_rec(a, b) + a.o_tail);
    float* fifo = reinterpret_cast<float*>(wave_rec(a, b) + a.o_fifo);
    const WaveMeta m = a.meta[b];
    const WaveStep w = wave_step(m.p, m.c, m.fin, hop, half, a.LA);
    const long long D = N + (long long)a.LA * hop;
    const long long e_old = w.e_old, e_new = e_old + w.ke;
    const long long tb_old = e_old * hop - half, tb_new = e_new * hop - half;      // first sample of the partial sums (< 0: nothing finished)
    const long long done_old = tb_old > 0 ? tb_old : 0;                // samples finished before this call
    const long long sent_old = m.p > D ? m.p - D : 0;                  // samples emitted before this call: the fifo holds [sent_old, done_old)
    for (int i = tid; i < NT; i += 256) s_tail[i] = tail[i];
    for (int i = tid; i < hop; i += 256) s_fifo[i] = fifo[i];
    __syncthreads();
    auto frame = [&](long long e) { return fr + ((long)b * a.nrow + (e - e_old + w.j0)) * N; };      // row j = step j = frame nf + j - LA
    // the oldest frame that reaches position p = i + half of the centre-padded clip
    auto oldest = [&](long long p) -> long long { return p < N ? 0 : (p - N) / hop + 1; };
    auto sample = [&](long long i) -> float {                          // sent_old <= i < (finish: L, else) tb_new
        if (i < done_old) return s_fifo[(int)(i - sent_old)];
        const long long p = i + half;
        const long long thi = p / hop < e_new ? p / hop : e_new - 1, tlo = oldest(p);
        float num = 0.0f, den = 0.0f;
        for (long long t = thi; t >= tlo; --t) {
            const int k = (int)(p - t * hop);                          // 0 <= k < n_fft by the two bounds
            if (t >= e_old) num += frame(t)[k];
            den += window[k] * window[k];
        }
        if (e_old > 0 && i - tb_old < NT) num += s_tail[(int)(i - tb_old)];      // the frames < e_old that reach i
        return den > 1e-11f ? num / den : 0.0f;
    };
    const int valid = m.fin ? (int)D : m.c;
    const long long first = m.p - D;
    for (int j = tid; j < ncols; j += 256) {
        float v = 0.0f;
        if (j < valid && first + j >= 0) v = sample(first + j);
        pcm_store<FMT>(out, b, j, v, true);
    }
    if (m.c > 0) {
        const long long sent_new = m.p + m.c > D ? m.p + m.c - D : 0;
        const long long done_new = tb_new > 0 ? tb_new : 0;
        for (int q = tid; q < hop; q += 256) fifo[q] = sent_new + q < done_new ? sample(sent_new + q) : 0.0f;
        if (w.ke > 0)
            for (int q = tid; q < NT; q += 256) {                      // sample tb_new + q: frame e_new - 1 always reaches it
                const long long i = tb_new + q, p = i + half;
                const long long tlo = oldest(p) > e_old ? oldest(p) : e_old;
                float num = frame(e_new - 1)[hop + q];
                for (long long t = e_new - 2; t >= tlo; --t) num += frame(t)[(int)(p - t * hop)];
                if (e_old > 0 && i - tb_old < NT) num += s_tail[(int)(i - tb_old)];
                tail[q] = num;
            }
    }
}

void launch_wave_ola(const WaveArgs& a, const float* fr, const float* window, const PcmOut& out, int ncols, hipStream_t s) {
#define FSNP_CALL(F) hipLaunchKernelGGL(wave_ola_kernel<F>, dim3(a.S), dim3(256), (size_t)2 * a.half * sizeof(float), s, a, fr, window, out, ncols)
    FSNP_PCM_SWITCH2(out.fmt, FSNP_CALL);
#undef FSNP_CALL
}

}  // namespace fsnp
