// lstm_step.hip - live stream sessions (include/fsnp_stream_live.h): ONE launch per LSTM layer and time step, cut by columns over
// the whole chip.
//
// A live push is short (one hop is the point of it), so there is no time loop to stay resident for: one step of one layer is a plain
// GEMM plus cells, [rows x (inputs + H)] x [(inputs + H) x 4H] with h_{t-1} read from memory, and the order layer 0 -> layer 1 ->
// next step is the order of the launches on the stream.  No workgroup waits for another one: no counters, no polling, no cooperative
// launch.  Every kernel reads h_{t-1} from the buffer of parity t & 1 and writes h_t to the other one (nobody of the same launch reads
// it) and, with c_t, in place into the slot records: a (row, unit) of a record is touched by exactly one thread of a launch, and no
// step kernel ever READS h from a record (live_load_kernel copies it into the parity-0 buffers in front of the first step), so the
// records are up to date after every step and nothing is left to do at the end of a push.
//
//   sub-band    grid (row tiles of 32) x (H / 16): a workgroup owns 16 hidden units = 64 gate columns = two 32 x 32 fp32 MFMA tiles
//               (gates i|f and g|o) and splits K over its 4 waves; the weight image is the one the K-split column-split kernel
//               already has (LstmWeights::wpack_coop[1], weight_layouts.h PK_KSPLIT at 16 units: [slice][wave][k-group][tile][lane][4],
//               local group i of wave w = global k-group 4 i + w) - nothing is packed for this file.  h travels between the launches
//               as per-tile images in MFMA A-fragment order (a_frag_index), so a wave's operand load is one coalesced 1 KiB read per
//               k-group; x_t is gathered (sb_feature_offset) and normalised (md_row) into an LDS image of the same order.  The four
//               waves' partial tiles meet in LDS and are summed in wave order 0..3: no float atomics, one order for every row.
//   full-band   a GEMV over 15 MB of weights: grid (CH / 8) x (rows / 8), 512 threads = 32 gate columns x 16 k-parts on plain FMAs
//               over the transposed image of the runtime-sized kernel (LstmWeights::wgen), so the weight read is spread over CH / 8
//               CUs once per step; the k-parts are summed in order 0..15.  A row's arithmetic does not depend on the rows beside it.
//   Linear(H, 2) + sb_act + output store: a wave per row, fixed summation order (live_sb_out_kernel).
// rows[].valid is the row's step count of this push: at step t a row with valid <= t keeps its state and writes nothing.
#include "fsnp_common.h"
#include "lstm_common.h"
#include "lstm_launch.h"

namespace fsnp {

namespace {

constexpr int kStepKgxp = 8;           // x k-groups of the 16-unit K-split image: KX = 40 and 64 both pad to 8 groups (64 columns)
constexpr int kPartLd = 17;            // floats per lane of a partial tile in LDS (16 + 1: lane-strided stores without bank conflicts)

}  // namespace

// ------------------------------------------------------------------------------------------------ state -> parity-0 h buffers
// blocks [0, 2 tiles): sub-band h0 / h1 of one row tile, record [f][layer][h|c][H] -> A-fragment image; blocks behind: full-band rows
__global__ __launch_bounds__(256) void live_load_kernel(LiveSbArgs sb, LiveFbArgs fb, int H, int CH) {
    const int tid = threadIdx.x;
    if ((int)blockIdx.x < 2 * sb.tiles) {
        const int tile = blockIdx.x >> 1, which = blockIdx.x & 1, KGH = H / 8;
        float4* img = reinterpret_cast<float4*>(which ? sb.h1[0] : sb.h0[0]) + (size_t)tile * KGH * 64;
        for (int e = tid; e < KGH * 64; e += 256) {
            const int g = e >> 6, kh = (e >> 5) & 1, row = e & 31;
            const RowDesc rd = sb.rows[tile * 32 + row];
            float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
            if (rd.valid > 0) {
                const float* p = sb.st + (size_t)rd.b * sb.st_stride + (size_t)rd.f * 4 * H + which * 2 * H + 8 * g + kh;
                v = make_float4(p[0], p[2], p[4], p[6]);
            }
            img[e] = v;
        }
        return;
    }
    const long idx = ((long)blockIdx.x - 2 * sb.tiles) * 256 + tid;
    if (idx >= (long)fb.num_rows * 2 * CH) return;
    const int i = (int)(idx / (2 * CH)), which = (int)(idx / CH) & 1, u = (int)(idx % CH);
    const RowDesc rd = fb.rows[i];
    if (rd.valid <= 0) return;
    (which ? fb.h1[0] : fb.h0[0])[(size_t)rd.b * CH + u] = fb.st[(size_t)rd.b * fb.st_stride + which * 2 * CH + u];
}

// ------------------------------------------------------------------------------------------------ sub-band: one layer, one step
template <int HID, int LAYER>
__global__ __launch_bounds__(256) void live_sb_step_kernel(LstmWeights w, LiveSbArgs a) {
    constexpr int KGH = HID / 8, KGXP = kStepKgxp;
    constexpr int G0W = (KGXP + KGH) / 4, G1W = KGH / 2, GW = G0W + G1W;     // k-groups per wave: layer 0, layer 1, both
    static_assert(KGH % 4 == 0, "k-groups split over 4 waves");
    __shared__ float4 Xs[LAYER == 0 ? KGXP * 64 : 1];                         // A image of x_t (layer 0)
    __shared__ float part[4 * 2 * 64 * kPartLd];                              // [wave][tile][lane][16 + 1]
    __shared__ RowDesc rows_s[32];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int tile = blockIdx.x, cs = blockIdx.y, t = a.t, par = a.par;
    int live = 0;
    if (tid < 32) {
        const RowDesc rd = a.rows[tile * 32 + tid];
        rows_s[tid] = rd;
        live = t < rd.valid;
    }
    if (!__syncthreads_or(live)) return;                                      // every row of this tile has had its steps

    if constexpr (LAYER == 0) {       // x_t: row = tid & 31, features j = (tid >> 5) + 8 i over all 64 columns of the image
        const int row = tid & 31;
        const RowDesc rd = rows_s[row];
        const bool on = t < rd.valid;
        NormMD md = {0.0f, 1.0f};
        if (on) md = a.md_row[(size_t)(tile * 32 + row) * a.Tp + t];
        float* Xf = reinterpret_cast<float*>(Xs);
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            const int j = (tid >> 5) + 8 * i;
            float v = 0.0f;
            if (on && j < w.NIN) {
                const int off = sb_feature_offset(j, rd.f, rd.b * a.Tp * a.FP, a.F, a.NSBN, a.NFBN, a.fb_rel, a.fb_branch_stride);
                v = (a.att_mag[off + t * a.FP] - md.m) / md.d;
            }
            Xf[a_frag_index(row, j)] = v;
        }
        __syncthreads();
    }

    // ---- this wave's quarter of K over the workgroup's two tiles
    const float4* __restrict__ Wp = reinterpret_cast<const float4*>(w.wpack_coop[1]) +
                                    (((size_t)cs * 4 + wave) * GW + (LAYER ? G0W : 0)) * 2 * 64 + lane;
    const float4* __restrict__ h0p = reinterpret_cast<const float4*>(a.h0[LAYER ? par ^ 1 : par]) + (size_t)tile * KGH * 64 + wave * 64 + lane;
    const float4* __restrict__ h1p = reinterpret_cast<const float4*>(a.h1[par]) + (size_t)tile * KGH * 64 + wave * 64 + lane;
    f32x16 acc0, acc1;
#pragma unroll
    for (int r = 0; r < 16; ++r) { acc0[r] = 0.0f; acc1[r] = 0.0f; }
    auto mm = [&](const float4 av, const float4 b0, const float4 b1) {
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b0.x, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.x, b1.x, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b0.y, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.y, b1.y, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b0.z, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.z, b1.z, acc1, 0, 0, 0);
        acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b0.w, acc0, 0, 0, 0);
        acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av.w, b1.w, acc1, 0, 0, 0);
    };
    // local k-group i of this wave is global k-group 4 i + wave.  layer 0: [x_t (the first 8 groups, LDS) | h0_{t-1}], layer 1:
    // [h1_{t-1} | h0_t].  Operands travel L2 -> registers in batches of NB groups, the next batch in flight while this one multiplies
    // (left to itself hipcc loads a group right in front of its MFMAs and every group waits out an L2 round trip).
    constexpr int NG = LAYER ? G1W : G0W, NB = HID == 384 ? 6 : 4, NX = LAYER ? KGH / 4 : KGXP / 4;
    float4 av[2][NB], b0[2][NB], b1[2][NB];
    auto load = [&](int buf, int i0) {
#pragma unroll
        for (int j = 0; j < NB; ++j) {
            const int i = i0 + j;
            if (i >= NG) continue;
            if (LAYER == 0) av[buf][j] = i < NX ? Xs[(4 * i + wave) * 64 + lane] : h0p[(i - NX) * 256];
            else av[buf][j] = i < NX ? h1p[i * 256] : h0p[(i - NX) * 256];
            b0[buf][j] = Wp[i * 128];
            b1[buf][j] = Wp[i * 128 + 64];
        }
    };
    load(0, 0);
#pragma unroll
    for (int i0 = 0; i0 < NG; i0 += NB) {
        const int cur = (i0 / NB) & 1;
        if (i0 + NB < NG) load(cur ^ 1, i0 + NB);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < NB; ++j)
            if (i0 + j < NG) mm(av[cur][j], b0[cur][j], b1[cur][j]);
        __builtin_amdgcn_sched_barrier(0);
    }
    {
        float* p0 = part + ((wave * 2 + 0) * 64 + lane) * kPartLd;
        float* p1 = part + ((wave * 2 + 1) * 64 + lane) * kPartLd;
#pragma unroll
        for (int r = 0; r < 16; ++r) { p0[r] = acc0[r]; p1[r] = acc1[r]; }
    }
    __syncthreads();

    // ---- cells: thread = (row, a pair of units that are neighbours in the A image): units u, u + 2 = 8 ua + 2 p + kh, p = 2 ph, 2 ph + 1
    const int row = tid & 31, q = tid >> 5;
    const RowDesc rd = rows_s[row];
    if (t >= rd.valid) return;
    const int ua = q >> 2, kh = (q >> 1) & 1, ph = q & 1;
    const int u0 = 8 * ua + 4 * ph + kh;
    // element (row, column c) of a 32 x 32 accumulator tile: lane c + 32 ((row >> 2) & 1), register (row & 3) + 4 (row >> 3)
    const int plane = 32 * ((row >> 2) & 1), preg = (row & 3) + 4 * (row >> 3);
    auto pre = [&](int gate, int u) {
        const int n = gate >> 1, c = (gate & 1) * 16 + u;
        const float* p = part + (n * 64 + plane + c) * kPartLd + preg;
        float s = p[0];                                                       // waves 0, 1, 2, 3 in this order, then the bias
        s += p[1 * 2 * 64 * kPartLd];
        s += p[2 * 2 * 64 * kPartLd];
        s += p[3 * 2 * 64 * kPartLd];
        return s + w.bias[LAYER * 4 * HID + gate * HID + cs * 16 + u];
    };
    float* __restrict__ rec = a.st + (size_t)rd.b * a.st_stride + (size_t)rd.f * 4 * HID + LAYER * 2 * HID + cs * 16 + u0;
    f32x2 c = f32x2{rec[HID], rec[HID + 2]};
    const f32x2 h = lstm_cell_pair(f32x2{pre(0, u0), pre(0, u0 + 2)}, f32x2{pre(1, u0), pre(1, u0 + 2)},
                                   f32x2{pre(2, u0), pre(2, u0 + 2)}, f32x2{pre(3, u0), pre(3, u0 + 2)}, c);
    rec[HID] = c.x; rec[HID + 2] = c.y;
    rec[0] = h.x; rec[2] = h.y;
    float* hn = (LAYER ? a.h1[par ^ 1] : a.h0[par ^ 1]) + ((size_t)tile * KGH * 64 + (2 * cs + ua) * 64 + kh * 32 + row) * 4 + 2 * ph;
    *reinterpret_cast<float2*>(hn) = make_float2(h.x, h.y);
}

// Linear(H, 2) + activation + store of step t: a wave per row, output o = lane >> 5, k = (lane & 31) + 32 i, then a fixed butterfly
template <int HID>
__global__ __launch_bounds__(256) void live_sb_out_kernel(LstmWeights w, LiveSbArgs a) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= a.tiles * 32) return;
    const RowDesc rd = a.rows[r];
    if (a.t >= rd.valid) return;
    const float* img = a.h1[a.par ^ 1] + (size_t)(r >> 5) * (HID / 8) * 256;
    const int o = lane >> 5;
    float s = 0.0f;
#pragma unroll 4
    for (int i = 0; i < HID / 32; ++i) {
        const int k = (lane & 31) + 32 * i;
        s = fmaf(img[a_frag_index(r & 31, k)], w.wfc[o * HID + k], s);
    }
#pragma unroll
    for (int m = 16; m > 0; m >>= 1) s += __shfl_xor(s, m);
    if ((lane & 31) == 0) a.out[(size_t)rd.out_off + (size_t)o * a.out_stride_o + a.t] = apply_act(s + w.bfc[o], a.act);
}

// ------------------------------------------------------------------------------------------------ full-band: one layer, one step
constexpr int kFbUnits = 8, kFbKParts = 16, kFbThreads = 32 * kFbKParts;
static size_t live_fb_smem(int RB, int H, int NIN) {
    const size_t KP = (size_t)cdiv(NIN > H ? NIN + H : 2 * H, 64) * 64;      // the larger K of the two layers, padded to the k-loop's stride
    return ((size_t)RB * KP + (size_t)kFbKParts * RB * 32) * 4;
}

template <int LAYER, int RB>
__global__ __launch_bounds__(kFbThreads) void live_fb_step_kernel(LstmWeights w, LiveFbArgs a) {
    extern __shared__ __attribute__((aligned(16))) float fsm[];
    __shared__ RowDesc rows_s[RB];
    const int H = w.H, NIN = w.NIN, G4 = 4 * H;
    const int KA = LAYER ? H : NIN, K = KA + H, KP = cdiv(K, 64) * 64;
    float* op = fsm;                                   // [RB][KP]  layer 0: [x_t | h0_{t-1}], layer 1: [h0_t | h1_{t-1}], zero padded
    float* red = fsm + RB * KP;                        // [k-part][RB][32 columns]
    const int tid = threadIdx.x, t = a.t, par = a.par;
    const int u0 = blockIdx.x * kFbUnits, r0 = blockIdx.y * RB;
    int live = 0;
    if (tid < RB) {
        const bool have = r0 + tid < a.num_rows;
        const int i = have ? r0 + tid : 0;
        rows_s[tid].b = a.rows[i].b;
        rows_s[tid].valid = have ? a.rows[i].valid : 0;
        live = have && t < a.rows[i].valid;
    }
    if (!__syncthreads_or(live)) return;

    const float* __restrict__ hA = LAYER ? a.h0[par ^ 1] : a.h0[par];        // the H values next to the input: h0_{t-1} / h0_t
    for (int idx = tid; idx < RB * KP; idx += kFbThreads) {
        const int r = idx / KP, k = idx % KP;
        const RowDesc rd = rows_s[r];
        float v = 0.0f;
        if (t < rd.valid && k < K) {
            if (LAYER == 0) {
                if (k < NIN) {
                    const NormMD md = a.md_seq[(size_t)rd.b * a.Tp + t];
                    v = (a.dense[((size_t)rd.b * a.Tp + t) * a.dense_stride + k] - md.m) / md.d;
                } else v = hA[(size_t)rd.b * H + (k - NIN)];
            } else v = k < H ? hA[(size_t)rd.b * H + k] : a.h1[par][(size_t)rd.b * H + (k - H)];
        }
        op[idx] = v;
    }
    __syncthreads();

    // thread = (gate column, k-part): k = 64 i + 4 kp + j
    const int col = tid & 31, kp = tid >> 5;
    const int u = u0 + (col & 7);
    const bool cvalid = u < H;
    const float* __restrict__ wT = w.wgen + (LAYER ? (size_t)(NIN + H) * G4 : 0) + (cvalid ? (col >> 3) * H + u : 0);
    float acc[RB];
#pragma unroll
    for (int r = 0; r < RB; ++r) acc[r] = 0.0f;
#pragma unroll 4
    for (int kb = 4 * kp; kb < KP; kb += 64) {
        float wv[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) wv[j] = (cvalid && kb + j < K) ? wT[(size_t)(kb + j) * G4] : 0.0f;
#pragma unroll
        for (int r = 0; r < RB; ++r) {
            const float4 v = *reinterpret_cast<const float4*>(op + r * KP + kb);
            float s = acc[r];
            s = fmaf(wv[0], v.x, s); s = fmaf(wv[1], v.y, s); s = fmaf(wv[2], v.z, s); s = fmaf(wv[3], v.w, s);
            acc[r] = s;
        }
    }
#pragma unroll
    for (int r = 0; r < RB; ++r) red[(kp * RB + r) * 32 + col] = acc[r];
    __syncthreads();

    if (tid >= RB * kFbUnits) return;
    const int r = tid / kFbUnits, uu = tid % kFbUnits, cu = u0 + uu;
    const RowDesc rd = rows_s[r];
    if (cu >= H || t >= rd.valid) return;
    float g4[4];
#pragma unroll
    for (int g = 0; g < 4; ++g) {
        float s = 0.0f;
        for (int p = 0; p < kFbKParts; ++p) s += red[(p * RB + r) * 32 + g * 8 + uu];      // k-parts 0 .. 15 in this order
        g4[g] = s + w.bias[LAYER * G4 + g * H + cu];
    }
    float* __restrict__ rec = a.st + (size_t)rd.b * a.st_stride + LAYER * 2 * H + cu;
    const float cn = exact_sigmoid(g4[1]) * rec[H] + exact_sigmoid(g4[0]) * exact_tanh(g4[2]);
    const float hv = exact_sigmoid(g4[3]) * exact_tanh(cn);
    rec[H] = cn;
    rec[0] = hv;
    (LAYER ? a.h1[par ^ 1] : a.h0[par ^ 1])[(size_t)rd.b * H + cu] = hv;
    if (LAYER == 1) a.seq_out[((size_t)rd.b * a.Tp + t) * a.seq_stride + cu] = hv;
}

// ------------------------------------------------------------------------------------------------ host
bool live_sb_available(const LstmWeights& w) {
    return !w.gru && w.OUT == 2 && (w.H == 384 || w.H == 256) && (w.KX == 40 || w.KX == 64) && w.wpack_coop[1] != nullptr;
}

// floats of the session's h buffers: 2 layers x 2 parities of per-tile A images / of [slot][CH] vectors
size_t live_sb_h_floats(int H, int tiles) { return (size_t)tiles * (H / 8) * 256; }

// LDS opt-in + residency check of one instantiation (smem == 0: opt-in only): lds_opt_in, lstm_launch.h
template <int LAYER, int RB>
static hipError_t live_fb_prepare(size_t smem) { return lds_opt_in<live_fb_step_kernel<LAYER, RB>>(152 * 1024, kFbThreads, smem); }

// rows per workgroup of the full-band step kernel: 8, or 1 where 8 operand rows do not fit a CU's LDS; 0 = not even one
int live_fb_rows_per_group(int H, int NIN) {
    if (live_fb_smem(8, H, NIN) <= (size_t)150 * 1024) return 8;
    return live_fb_smem(1, H, NIN) <= (size_t)150 * 1024 ? 1 : 0;
}

// session-creation check (as lstm_generic_stream_check): LDS opt-in + residency of the instantiations a live push launches
int live_fb_check(int H, int NIN) {
    const int rb = live_fb_rows_per_group(H, NIN);
    if (rb == 0) { set_error("live full-band step kernel (hidden %d, %d inputs): one operand row does not fit a CU's LDS", H, NIN); return 2; }
    const size_t smem = live_fb_smem(rb, H, NIN);
    hipError_t e = rb == 8 ? live_fb_prepare<0, 8>(smem) : live_fb_prepare<0, 1>(smem);
    if (e == hipSuccess) e = rb == 8 ? live_fb_prepare<1, 8>(smem) : live_fb_prepare<1, 1>(smem);
    if (e != hipSuccess) {
        set_error("live full-band step kernel (hidden %d, %d inputs): a 512-thread workgroup with its LDS does not fit a CU of this device: %s",
                  H, NIN, hipGetErrorString(e));
        return 2;
    }
    return 0;
}

void launch_live_load(const LiveSbArgs& sb, const LiveFbArgs& fb, int H, int CH, hipStream_t s) {
    const int blocks = 2 * sb.tiles + cdiv(fb.num_rows * 2 * CH, 256);
    if (blocks <= 0) return;
    hipLaunchKernelGGL(live_load_kernel, dim3(blocks), dim3(256), 0, s, sb, fb, H, CH);
}

void launch_live_sb_step(const LstmWeights& w, const LiveSbArgs& a, int layer, hipStream_t s) {
    if (a.tiles <= 0) return;
    const dim3 grid(a.tiles, w.H / 16);
    if (w.H == 256) {
        if (layer) hipLaunchKernelGGL((live_sb_step_kernel<256, 1>), grid, dim3(256), 0, s, w, a);
        else hipLaunchKernelGGL((live_sb_step_kernel<256, 0>), grid, dim3(256), 0, s, w, a);
    } else {
        if (layer) hipLaunchKernelGGL((live_sb_step_kernel<384, 1>), grid, dim3(256), 0, s, w, a);
        else hipLaunchKernelGGL((live_sb_step_kernel<384, 0>), grid, dim3(256), 0, s, w, a);
    }
}

void launch_live_sb_out(const LstmWeights& w, const LiveSbArgs& a, hipStream_t s) {
    if (a.tiles <= 0) return;
    if (w.H == 256) hipLaunchKernelGGL((live_sb_out_kernel<256>), dim3(a.tiles * 8), dim3(256), 0, s, w, a);
    else hipLaunchKernelGGL((live_sb_out_kernel<384>), dim3(a.tiles * 8), dim3(256), 0, s, w, a);
}

void launch_live_fb_step(const LstmWeights& w, const LiveFbArgs& a, int layer, hipStream_t s) {
    if (a.num_rows <= 0) return;
    const int rb = live_fb_rows_per_group(w.H, w.NIN);
    const size_t smem = live_fb_smem(rb, w.H, w.NIN);
    const dim3 grid(cdiv(w.H, kFbUnits), cdiv(a.num_rows, rb));
    // (a failed LDS opt-in makes the launch itself fail: the push's hipGetLastError reports it)
    if (rb == 8) {
        if (layer) { (void)live_fb_prepare<1, 8>(0); hipLaunchKernelGGL((live_fb_step_kernel<1, 8>), grid, dim3(kFbThreads), smem, s, w, a); }
        else { (void)live_fb_prepare<0, 8>(0); hipLaunchKernelGGL((live_fb_step_kernel<0, 8>), grid, dim3(kFbThreads), smem, s, w, a); }
    } else {
        if (layer) { (void)live_fb_prepare<1, 1>(0); hipLaunchKernelGGL((live_fb_step_kernel<1, 1>), grid, dim3(kFbThreads), smem, s, w, a); }
        else { (void)live_fb_prepare<0, 1>(0); hipLaunchKernelGGL((live_fb_step_kernel<0, 1>), grid, dim3(kFbThreads), smem, s, w, a); }
    }
}

}  // namespace fsnp
