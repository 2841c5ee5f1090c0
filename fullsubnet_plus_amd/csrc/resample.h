// resample.h - the sample-rate converter of include/fsnp_resample.h: one rational polyphase FIR, defined by a closed formula, and the ONE
// device function that sums it.  The free-standing kernel (resample.hip) and the resampling pad kernel in front of the STFT (stft.hip)
// both call resample_sample, so that a fused call and the same conversion run on its own agree bit for bit whatever the compiler
// contracts elsewhere.  The rules are the header's, restated in DESIGN.md ("Sample rates").
//
//   g = gcd(from, to), up = to / g, down = from / g, M = max(up, down), half = kResampleZ * M
//   h[i] = (rho / M) sinc(rho i / M) I0(beta sqrt(1 - (i / half)^2)) / I0(beta),  |i| <= half;   t[i] = fp32(up h[i])
//   y[m] = sum over 0 <= k < n with |m down - k up| <= half of t[m down - k up] x[k],   m < ceil(n up / down)
//
// Tap rows per phase.  With c = m down, q = c / up and p = c % up the tap of sample k is t[p + (q - k) up]: output m walks ONE row of
//   table[p][col] = t[p + (J - col) up]  (0 where that index lies outside [-half, half]),   J = half / up,  0 <= col < tpp,
// at ascending columns col = J - q + k, i.e. in ascending k.  The zero entries are never read: the k range below is exactly the
// formula's, so a NaN or an infinity spreads as far as the formula says and no further.
#pragma once
#include <vector>

#include "pcm.h"

namespace fsnp {

constexpr int kResampleZ = 32;             // zero crossings of the sinc on either side of the centre tap
constexpr double kResampleRho = 0.91;      // cut-off as a share of the lower rate's Nyquist
constexpr double kResampleBeta = 8.6;      // Kaiser window
constexpr int kResampleMaxRatio = 640;     // max(up, down): 44.1 k <-> 192 k is 147 : 640, 16 k <-> 44.1 k is 160 : 441
constexpr int kResampleMaxPairs = 8;       // tables one handle keeps; they are never evicted (launches in flight read them)

struct ResamplePlan {
    int up, down, half;
    int J, tpp;                            // per-phase layout: column of tap index p is J, columns per phase
};
// what a kernel needs of one cached table; taps == nullptr: equal rates, a format-converting copy
struct ResampleTable {
    const float* taps;                     // device [up][tpp]
    int up, down, half, J, tpp;
};
// one cached pair of a handle: the host copy stays where it is until the handle goes (the upload reads it in stream order)
struct ResampleCached {
    ResamplePlan plan{};
    std::vector<float> host;               // [up][tpp]
    float* dev = nullptr;
};

// host arithmetic (fsnp_resample_abi.hip).  0, or 2 with the error set: a rate <= 0, max(up, down) > kResampleMaxRatio
int resample_plan(const char* where, int from_rate, int to_rate, ResamplePlan& plan);
inline long long resample_length(const ResamplePlan& p, long long n) { return (n * p.up + p.down - 1) / p.down; }
// t[i + half] for |i| <= half: the formula in double, I0 from its power series, rounded once to fp32; exactly symmetric
void resample_build_taps(const ResamplePlan& p, float* taps);
void resample_build_table(const ResamplePlan& p, float* table /*[up][tpp]*/);

#ifdef __HIPCC__
// Output sample m of a row of n input samples, sample k of the row being load(k).  Starts from 0.0f, ascending k, every step an explicit
// fmaf(t, x, acc); samples outside [0, n) are zeros and never loaded.  Where the samples lie is the caller's: one buffer (resample_sample),
// or a slot's carried history in front of a push's new samples (resample_stream.hip).
template <typename LOAD>
__device__ __forceinline__ float resample_sum(LOAD&& load, long m, long n, const ResampleTable& r) {
    const long c = m * r.down;                                 // the output's position on the grid of rate from * up
    const long q = c / r.up;
    const long at = (c - q * r.up) * r.tpp + r.J - q;          // table index of sample k: at + k
    long k = c - r.half <= 0 ? 0 : (c - r.half + r.up - 1) / r.up;     // first k with c - k up <= half
    long k1 = (c + r.half) / r.up;                             // last k with c - k up >= -half
    if (k1 > n - 1) k1 = n - 1;
    float acc = 0.0f;
    for (; k <= k1; ++k) acc = fmaf(r.taps[at + k], load(k), acc);
    return acc;
}
template <int FMT>
__device__ __forceinline__ float resample_sample(const PcmIn& in, long b, long m, long n, const ResampleTable& r) {
    return resample_sum([&](long k) { return pcm_load<FMT>(in, b, k); }, m, n, r);
}
#endif

// ---- streaming conversion (include/fsnp_wave_rate_stream.h; kernels: resample_stream.hip).  `p` is the plan of the caller's rate R ->
// the model's rate M; the way back is (down, up, half).  All of it 64-bit host-and-device arithmetic on the slot's sample count.
// model-rate samples whose whole window lies inside the first P input samples: sample j needs input up to floor((j down + half) / up)
__host__ __device__ inline long long resample_ready(int up, int down, int half, long long P) {
    return P * up <= half ? 0 : (P * up - half - 1) / down + 1;
}
__host__ __device__ inline long long resample_total(int up, int down, long long L) { return (L * up + down - 1) / down; }
// the smallest delay at rate R at which every push can return as many samples as it took, the inner session being DM samples late
inline long long resample_stream_delay(const ResamplePlan& p, long long DM) { return (DM * p.down + 2LL * p.half + 1 + p.up - 1) / p.up - 1; }
// carried samples: the input ones below P that sample ready(P) still reads, the enhanced ones a push's first output still reads
inline int resample_hist_in(const ResamplePlan& p) { return 2 * p.half / p.up; }
inline int resample_hist_out(const ResamplePlan& p) { return (2 * p.half + p.down - 1) / p.down; }
// most model-rate samples one push of c input samples completes, and a finish adds (total(L) - ready(L))
inline long long resample_push_max(const ResamplePlan& p, long long c) { return c * p.up / p.down + 1; }
inline int resample_finish_max(const ResamplePlan& p) { return (p.half + p.down - 1) / p.down; }

struct RateMeta { long long p; int c, fin; };      // samples (rate R) the slot had before this call, samples it gets now, 1 = it is finished now
struct RateArgs {
    unsigned char* state;                          // rate record of slot 0: [ input history fp32 [HI] | enhanced history fp32 [HE] | count int64 | up, down int32 ]
    size_t stride, o_he, o_count;                  // bytes between slots, byte offsets inside a record (the input history is at 0)
    RateMeta* meta;                                // [S], written by the in kernel for the out kernel behind it
    int S, HI, HE;
    int up, down, half;                            // the plan R -> M
    long long DM, DR;                              // the inner session's delay (rate M), the rate session's (rate R)
};
struct SlotCounts;
// c.v[slot]: samples of a push, or (fin) 1 = finish this slot.  xin [S][xs] fp32: the model-rate samples ready(P) .. ready(P + c) - 1
// (finish: .. total(L) - 1, the input clamped at L - 1) of every slot from its history and wav; history, count and pair advanced; meta written
void launch_rate_in(const RateArgs& a, const SlotCounts& c, int fin, const PcmIn& wav /*finish: p = NULL*/, const ResampleTable& t, float* xin,
                    long xs, hipStream_t s);
// out [S][ncols]: column j < c (finish: < DR) is sample P + j - DR (finish: L - DR + j) at rate R summed from the enhanced history, xout
// (the inner push's output, its column i = inner sample ready(P) + i - DM) and, at finish, xfin (the inner finish's DM columns); exactly 0
// where that index is negative and in every other column; the enhanced history advanced (push)
void launch_rate_out(const RateArgs& a, const ResampleTable& t /*M -> R*/, const float* xout, long xs, const float* xfin, long fs,
                     const PcmOut& out, int ncols, hipStream_t s);

// resample.hip
// out[b][m] = y_b[m] for m < the row's output count, exactly 0 from there to `cols`; one launch per kLenRows rows.
//   back = false: `samples` (NULL: `uniform` for every row) are INPUT counts n_b; row b has ceil(n_b up / down) outputs.
//   back = true : they are OUTPUT counts; row b reads ceil(n_b down / up) inputs - the way back of enhance_wave, whose caller takes
//                 the first n_b samples of what the model-rate clip converts to.
//   t.taps == nullptr: out[b][m] = in[b][m] for m < n_b (a format-converting copy).
// out.fmt kPcmF32 / kPcmS16 (out.clipped zeroed in front by the caller) / kPcmPeak (the first pass: fp32 rows and out.peak)
void launch_resample(const PcmIn& in, const PcmOut& out, const ResampleTable& t, int B, const int* samples, int uniform, int cols, bool back,
                     hipStream_t s);
constexpr int kResampleBlock = 256;        // outputs per workgroup
// stft.hip: launch_stft_pad of the clip CONVERTED by t, straight from the caller's buffer (samples / uniform: counts at the caller's
// rate; row b holds ceil(n_b up / down) model-rate samples, reflect-padded by n_fft / 2 at its own ends, zeros behind)
void launch_stft_pad_resample(const PcmIn& wav, float* xp, long xp_stride, int B, const int* samples, int uniform, int n_fft,
                              const ResampleTable& t, hipStream_t s);

}  // namespace fsnp
