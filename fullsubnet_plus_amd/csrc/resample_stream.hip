// resample_stream.hip - the two streaming converters of a rate session (include/fsnp_wave_rate_stream.h): samples at the caller's rate R
// in front of a wave session at the model's rate M, and behind it.  The arithmetic of which samples are ready is resample.h's
// (resample_ready, resample_total); every output is resample_sum, the one summing function of the whole-clip converter, over the SAME
// k range a whole-clip call has - only that its samples lie in the slot's carried history and in this call's new ones.
//
// One workgroup owns a slot, as in stft_stream.hip: every output of a slot reads the slot's history, and the same call rewrites it, so
// the rewrite stands behind a __syncthreads() of the one workgroup that read it - no counter, no second launch.  A 10 ms block is a few
// hundred outputs of 65 .. 193 taps each: one thread per output, 256 threads, and the slots of a session side by side on the chip.
// Histories and new samples are read where they lie (global memory: at most a few KB per slot, in the vector cache after the first
// touch) rather than staged in LDS: the history of a steep pair (1 : 640 keeps 40960 samples) would not fit, and one code path serves
// every pair.  Tap rows come from the handle's cached table, as in resample.hip.
//   rate_in_kernel    history + PcmIn -> fp32 model-rate rows (the inner push's input); history, count and pair advanced; meta written
//   rate_out_kernel   enhanced history + the inner push's output (+ the inner finish's) -> PcmOut at rate R, zeros where the contract
//                     says so; enhanced history advanced
#include "fsnp_common.h"
#include "pcm.h"
#include "resample.h"

namespace fsnp {

__device__ __forceinline__ unsigned char* rate_rec(const RateArgs& a, int b) { return a.state + (size_t)b * a.stride; }

// hist[i] = load(n - H + i) for 0 <= i < H (0 where that index is negative), in place: `load` may read hist itself.  Chunk t reads
// positions >= its own, writes only its own, and a barrier separates the two; every thread of the workgroup gets here.
template <typename LOAD>
__device__ __forceinline__ void rate_advance(float* hist, int H, long long n, LOAD&& load) {
    for (int i0 = 0; i0 < H; i0 += 256) {
        const int i = i0 + (int)threadIdx.x;
        const long long k = n - H + i;
        float v = 0.0f;
        if (i < H && k >= 0) v = load((long)k);
        __syncthreads();
        if (i < H) hist[i] = v;
    }
}

template <int FMT>
__global__ __launch_bounds__(256) void rate_in_kernel(RateArgs a, SlotCounts cnt, int fin_call, PcmIn wav, ResampleTable t, float* __restrict__ xin,
                                                      long xs) {
    const int b = blockIdx.x, tid = threadIdx.x;
    float* hist = reinterpret_cast<float*>(rate_rec(a, b));
    long long* pc = reinterpret_cast<long long*>(rate_rec(a, b) + a.o_count);
    const long long P = *pc;
    const int c = fin_call ? 0 : cnt.v[b], fin = fin_call ? cnt.v[b] : 0;
    const long long Pn = P + c;
    // input sample k of the clip, P - HI <= k < P + c
    auto sample = [&](long k) { return k < P ? hist[(int)(k - (P - a.HI))] : pcm_load<FMT>(wav, b, (long)(k - P)); };
    const long long r0 = resample_ready(a.up, a.down, a.half, P);
    const long long r1 = fin ? resample_total(a.up, a.down, P) : resample_ready(a.up, a.down, a.half, Pn);
    const int cm = (int)(r1 - r0);
    for (int j = tid; j < cm; j += 256) xin[(long)b * xs + j] = resample_sum(sample, (long)(r0 + j), (long)Pn, t);
    __syncthreads();                                           // every read of the old history and count is done
    if (tid == 0) {
        a.meta[b] = RateMeta{P, c, fin};
        if (c > 0) {
            *pc = Pn;
            int* pair = reinterpret_cast<int*>(pc + 1);
            pair[0] = a.up; pair[1] = a.down;
        }
    }
    if (c > 0) rate_advance(hist, a.HI, Pn, sample);
}

template <int FMT>
__global__ __launch_bounds__(256) void rate_out_kernel(RateArgs a, ResampleTable t, const float* __restrict__ xout, long xs,
                                                       const float* __restrict__ xfin, long fs,
                                                       PcmOut out /*no clipped count: every thread stores on its own*/, int ncols) {
    const int b = blockIdx.x, tid = threadIdx.x;
    float* he = reinterpret_cast<float*>(rate_rec(a, b) + a.o_he);
    const RateMeta m = a.meta[b];
    const long long r0 = resample_ready(a.up, a.down, a.half, m.p);
    const long long r1 = m.fin ? resample_total(a.up, a.down, m.p) : resample_ready(a.up, a.down, a.half, m.p + m.c);
    // enhanced model-rate sample k is the inner session's output sample k + DM: E0 of them were carried (the newest HE), this call's
    // inner push brought [E0, E1), and a finish the last DM of the clip's r1
    const long long E0 = r0 > a.DM ? r0 - a.DM : 0, E1 = r1 > a.DM ? r1 - a.DM : 0;
    const long long n = m.fin ? r1 : E1;
    auto sample = [&](long k) -> float {
        if (k < E0) return he[(int)(k - (E0 - a.HE))];
        if (k < r1 - a.DM) return xout[(long)b * xs + (k + a.DM - r0)];
        return xfin[(long)b * fs + (k + a.DM - r1)];           // (finish only: a push sums below E1)
    };
    const int valid = m.fin ? (int)a.DR : m.c;
    const long long first = m.p - a.DR;
    for (int j = tid; j < ncols; j += 256) {
        float v = 0.0f;
        if (j < valid && first + j >= 0) v = resample_sum(sample, (long)(first + j), (long)n, t);
        pcm_store<FMT>(out, b, j, v, true);
    }
    __syncthreads();                                           // every read of the old history is done
    if (m.c > 0 && E1 > 0) rate_advance(he, a.HE, E1, sample);
}

void launch_rate_in(const RateArgs& a, const SlotCounts& c, int fin, const PcmIn& wav, const ResampleTable& t, float* xin, long xs,
                    hipStream_t s) {
#define FSNP_CALL(F) hipLaunchKernelGGL(rate_in_kernel<F>, dim3(a.S), dim3(256), 0, s, a, c, fin, wav, t, xin, xs)
    FSNP_PCM_SWITCH2(wav.fmt, FSNP_CALL);
#undef FSNP_CALL
}

void launch_rate_out(const RateArgs& a, const ResampleTable& t, const float* xout, long xs, const float* xfin, long fs, const PcmOut& out,
                     int ncols, hipStream_t s) {
#define FSNP_CALL(F) hipLaunchKernelGGL(rate_out_kernel<F>, dim3(a.S), dim3(256), 0, s, a, t, xout, xs, xfin, fs, out, ncols)
    FSNP_PCM_SWITCH2(out.fmt, FSNP_CALL);
#undef FSNP_CALL
}

}  // namespace fsnp
