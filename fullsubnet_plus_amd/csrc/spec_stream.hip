// spec_stream.hip - the two short launches of a ring push (fsnp_stream_abi.hip, spec_push_body) around one mag push.
//
// Noisy complex64 spectra come in with strides (slot, f, frame) in complex elements, enhanced spectra go out the same way: the caller's
// tensors for a spectrum session (include/fsnp_spec_stream.h), the workspace rows between the two DFT GEMMs for a wave session
// (include/fsnp_wave_stream.h).  The mask of frame t is the model's output of step t + look_ahead, so the noisy spectra of the newest
// look_ahead frames wait in a per-slot ring (frame g in row g % look_ahead).  The ring's position is the mag record's own frame count,
// which the mag push's prologue kernel publishes as StreamMeta.p together with the slot's steps of this push: the host mirrors nothing.
// A slot brings as many spectra as it steps, except a wave slot that is finished: one spectrum, 1 + look_ahead steps.
#include "fsnp_common.h"

namespace fsnp {

// hypotf as fe_repack_complex_kernel takes the magnitude of a complex forward's input; one thread per (slot, frame, padded bin)
__global__ __launch_bounds__(256) void spec_mag_kernel(SpecArgs a, SlotCounts cnt, const float2* __restrict__ spec, long sb, long sf, long st,
                                                       float* __restrict__ mag, long total) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int f = (int)(i % a.FP), j = (int)((i / a.FP) % a.n), b = (int)(i / ((long)a.FP * a.n));
    float v = 0.0f;
    if (j < cnt.v[b] && f < a.F) {
        const float2 x = spec[b * sb + f * sf + j * st];
        v = hypotf(x.x, x.y);
    }
    mag[i] = v;
}

void launch_spec_mag(const SpecArgs& a, const SlotCounts& c, const float* spec, const int64_t strides[3], float* mag, hipStream_t s) {
    const long total = (long)a.S * a.n * a.FP;
    hipLaunchKernelGGL(spec_mag_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a, c, reinterpret_cast<const float2*>(spec),
                       (long)strides[0], (long)strides[1], (long)strides[2], mag, total);
}

// one thread per (slot, f): it alone touches bin f of the slot's ring, so reading the waiting spectra and replacing them needs no barrier
// (spec and out carry no __restrict__: both may be the caller's).  m.cnt = the slot's steps, cnt.v = its spectra: the ring takes what
// came in, never the zero frames behind a finished clip's last one
__global__ __launch_bounds__(256) void spec_apply_kernel(SpecArgs a, SlotCounts cnt, const float* __restrict__ mask, const float2* spec, long sb,
                                                         long sf, long st, float2* out, long ob, long of, long ot) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.S * a.F) return;
    const int b = i / a.F, f = i - b * a.F;
    const StreamMeta m = a.meta[b];
    float2* ring = reinterpret_cast<float2*>(a.ring + (size_t)b * a.ring_stride);
    const float2* in = spec + b * sb + f * sf;
    float2* o = out + b * ob + f * of;
    for (int j = 0; j < a.n; ++j) {
        float2 y = make_float2(0.0f, 0.0f);
        if (j < m.cnt && m.p + j >= a.LA) {
            const long long g = m.p + j - a.LA;                            // the frame whose mask step P + j is
            const float2 x = g < m.p ? ring[(int)(g % a.LA) * a.F + f] : in[(g - m.p) * st];
            y = cirm_times(mask, ((long)b * 2 * a.F + f) * a.n + j, (long)a.F * a.n, x);
        }
        o[j * ot] = y;
    }
    const int ks = cnt.v[b];
    if (a.LA > 0)
        for (int j = ks > a.LA ? ks - a.LA : 0; j < ks; ++j) ring[(int)((m.p + j) % a.LA) * a.F + f] = in[j * st];
}

void launch_spec_apply(const SpecArgs& a, const SlotCounts& c, const float* mask, const float* spec, const int64_t strides[3], float* out,
                       const int64_t out_strides[3], hipStream_t s) {
    hipLaunchKernelGGL(spec_apply_kernel, dim3(cdiv(a.S * a.F, 256)), dim3(256), 0, s, a, c, mask, reinterpret_cast<const float2*>(spec),
                       (long)strides[0], (long)strides[1], (long)strides[2], reinterpret_cast<float2*>(out), (long)out_strides[0],
                       (long)out_strides[1], (long)out_strides[2]);
}

}  // namespace fsnp
