// rowtile.h - what the one-tile-per-CU recurrent kernels (lstm.hip: lstm2_fc_kernel, lstm2_fc_stream_kernel; lstm_gru.hip:
// gru2_fc_kernel; lstm16.hip: lstm2_fc16_kernel) share around their k-group loops and cells: the dynamic-LDS image, the table fills of
// the prologue, the per-step gather of x_t and the Linear epilogue.  Everything here is resolved at compile time: a kernel names its
// differences as template arguments and keeps its own k-group loops, cell and store condition.  A kernel uses a helper only where
// hipcc's code for every instantiation keeps its registers, spills and loops (tools/asm_diff.py, profiles/rowtile_shared.md).
#pragma once
#include "fsnp_common.h"
#include "lstm_common.h"
#include "lstm_launch.h"

namespace fsnp {

// ---- the dynamic-LDS image of a tile of ROWS (32 or 16) MFMA rows + EX VALU rows, NW waves: byte offset of every region, in the
// order they lie.  An A image is 64 float4 per k-group (8 k of 32 rows, or 16 k of 16 rows).  The kernels take their pointers as
// smem + offset, the launchers their dynamic LDS size from bytes().
template <int ROWS, int HID, int KX, int EX, int NW, bool BF>
struct RowTileLds {
    static_assert(ROWS == 32 || ROWS == 16, "MFMA rows per tile");
    static constexpr int KG = ROWS == 32 ? 8 : 16;                       // k per k-group
    static constexpr int KGX = (KX + KG - 1) / KG, KGH = HID / KG;      // k-groups of x_t (zero padded) and of h
    static constexpr int KSB = HID / (2 * KG);                           // bf16 k-steps of the layer-1 ih segment (BF only)
    static constexpr int BL = (BF && ROWS == 32) ? 1 : 2;                // bias layers: the 32-row BF kernel folds layer 0's into its weights
    static constexpr int HB = !BF ? 0 : (ROWS == 32 && EX > 0) ? 1 : 2;  // bf16 images of h0_t: hi + lo; hi only where E images take the room
    static constexpr int state_f4 = (KGX + 2 * KGH) * (64 + 2 * EX);     // float4 from x on that start as zero: the A and E images
    static constexpr size_t x = 0;                                       // [KGX][64] float4       A image of x_t
    static constexpr size_t h0 = x + (size_t)KGX * 64 * 16;              // [KGH][64]              h0
    static constexpr size_t h1 = h0 + (size_t)KGH * 64 * 16;             // [KGH][64]              h1
    static constexpr size_t xe = h1 + (size_t)KGH * 64 * 16;             // [KGX][2][EX]           E image of x_t (extra rows)
    static constexpr size_t he0 = xe + (size_t)KGX * 2 * EX * 16;        // [KGH][2][EX]
    static constexpr size_t he1 = he0 + (size_t)KGH * 2 * EX * 16;       // [KGH][2][EX]
    static constexpr size_t fc = he1 + (size_t)KGH * 2 * EX * 16;        // [2][HID] float         Linear weights (32 rows: as [2][HID / 8][2] float4)
    static constexpr size_t rows = fc + (size_t)2 * HID * 4;             // [ROWS + EX] RowDesc
    static constexpr size_t bias = rows + (ROWS + EX) * sizeof(RowDesc); // [BL][NW][tiles per wave][ROWS columns] = [BL][4 HID] float
    static constexpr size_t h0b = bias + (size_t)BL * 4 * HID * 4;       // [HB][KSB][64] float4   bf16 A images of h0_t (h = hi + lo)
    static constexpr size_t bytes() { return h0b + (size_t)HB * KSB * 64 * 16; }
    static constexpr bool fits(size_t static_lds) { return bytes() + static_lds <= (size_t)kCuLds; }   // next to the kernel's static LDS
};

// Linear weights [2][HID] as Wfc4[o][k-group][k parity] = the 4 weights a float4 of a 32-row A image multiplies
template <int HID, int NTHR>
__device__ __forceinline__ void rowtile_fill_fc(float4* __restrict__ Wfc4, const float* __restrict__ wfc, int tid) {
    constexpr int KGH = HID / 8;
    for (int i = tid; i < 2 * KGH * 2; i += NTHR) {
        const int o = i / (KGH * 2), kg = (i >> 1) % KGH, kh = i & 1;
        const float* wr = wfc + (size_t)o * HID + kg * 8 + kh;
        Wfc4[i] = make_float4(wr[0], wr[2], wr[4], wr[6]);
    }
}

// bias[2][4 HID] (gate-major) as Bs[((layer * NW + wave) * NT + n) * COLS + col], tile n = gate * ST + s.  LAYERS == 1: layer 1 only.
template <int COLS, int LAYERS, int HID, int NW, int NTHR>
__device__ __forceinline__ void rowtile_fill_bias(float* __restrict__ Bs, const float* __restrict__ bias, int tid) {
    constexpr int UW = HID / NW, ST = UW / COLS, NT = 4 * ST, SH = COLS == 32 ? 5 : 4;
    static_assert(COLS == 32 || COLS == 16, "columns per tile");
    for (int i = tid; i < LAYERS * NW * NT * COLS; i += NTHR) {
        const int col = i & (COLS - 1), n = (i >> SH) % NT, wv = (i / (COLS * NT)) % NW, layer = LAYERS == 1 ? 1 : i / (COLS * NT * NW);
        Bs[i] = bias[layer * 4 * HID + (n / ST) * HID + wv * UW + (n % ST) * COLS + col];
    }
}

// accumulator tiles that start as their column's bias (bias already offset by the lane's column, tile n at bias[n * STRIDE])
template <int STRIDE, typename V, int NT>
__device__ __forceinline__ void acc_from_bias(V (&acc)[NT], const float* __restrict__ bias) {
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
        for (int r = 0; r < (int)(sizeof(V) / sizeof(float)); ++r) acc[n][r] = bias[n * STRIDE];
}

// ---- the gather of x_t: thread tid owns row = tid % ROWS of the tile and features j = tid / ROWS + JSTEP i of its input frame; every
// step it loads x(t + 1) early (prefetch), and normalises and stores it into the A image once layer 0 has consumed x(t) (store_next).
// goff: 32-bit float offset of the element at t = 0 from one uniform base (att_mag, or the dense input); -1 = zero; -2 = no element i.
//   IDX    float index of (row, k) inside the A image (a_frag_index / a16_index)
//   KXP    features of the image (KX, zero padded to whole k-groups)
//   STREAM rows[].valid is a step count, the per-row norm table is always there, no dense mode
template <int (*IDX)(int, int), int ROWS, int NTHR, int KXP, bool STREAM>
struct RowTileGather {
    static constexpr int JSTEP = NTHR / ROWS, NG = (KXP + JSTEP - 1) / JSTEP;
    static constexpr bool HOLES = ROWS == 32 || NG * JSTEP != KXP;   // test for -2 (the 32-row kernels always did, and keep their code)

    const float* __restrict__ gbase;
    int gstep;
    bool dense;
    float* Xf;
    int goff[NG], xdst[NG];
    NormMD md; const NormMD* md_row;
    const RowDesc* rd_s;                                             // the thread's row (LDS)
    // offset(): of feature j of row rd at t = 0, or -1.  norms(): of row rd, one {mean, deviation} for all steps or a table entry per step
    __device__ __forceinline__ int offset(const LstmWeights& w, const LstmArgs& a, const RowDesc& rd, int j) const {
        if (!(STREAM ? rd.valid > 0 : rd.valid != 0) || j >= w.NIN) return -1;
        if (dense) return rd.b * a.Tp * w.NIN + j;           // rd.b = sequence index in dense mode
        return sb_feature_offset(j, rd.f, rd.b * a.Tp * a.FP, a.F, a.NSBN, a.NFBN, a.fb_rel, a.fb_branch_stride);
    }
    __device__ __forceinline__ void norms(const LstmArgs& a, const RowDesc& rd, int slot, NormMD& m, const NormMD*& m_row) const {
        m.m = 0.0f; m.d = 1.0f; m_row = nullptr;
        if constexpr (STREAM) { m_row = a.md_row + (size_t)slot * a.Tp; return; }     // (rows without steps: never dereferenced)
        if (dense || !rd.valid) return;
        if (a.md_row != nullptr) m_row = a.md_row + (size_t)slot * a.Tp;
        else m = a.md_utt[rd.b];
    }
    __device__ __forceinline__ void plan(const LstmWeights& w, const LstmArgs& a, const RowDesc* rows_s, int slot0, int tid, float* Xf_) {
        dense = !STREAM && a.dense != nullptr;
        gbase = dense ? a.dense : a.att_mag;
        gstep = dense ? w.NIN : a.FP;
        Xf = Xf_;
        const int grow = tid & (ROWS - 1);
        rd_s = rows_s + grow;
        const RowDesc rd = rows_s[grow];
#pragma unroll
        for (int i = 0; i < NG; ++i) {
            const int j = (tid >> (ROWS == 32 ? 5 : 4)) + JSTEP * i;
            goff[i] = (!HOLES || j < KXP) ? offset(w, a, rd, j) : -2;
            xdst[i] = IDX(grow, !HOLES || j < KXP ? j : 0);
        }
        norms(a, rd, slot0 + grow, md, md_row);
    }
    __device__ __forceinline__ bool has_row_norm() const { return STREAM ? rd_s->valid > 0 : md_row != nullptr; }   // a table entry per step?
    __device__ __forceinline__ void store_first() const {           // x(0)
        const NormMD m0 = has_row_norm() ? md_row[0] : md;
#pragma unroll
        for (int i = 0; i < NG; ++i)
            if (!HOLES || goff[i] != -2) Xf[xdst[i]] = goff[i] >= 0 ? (gbase[goff[i]] - m0.m) / m0.d : 0.0f;
    }
    __device__ __forceinline__ void prefetch(int t, float (&xr)[NG], NormMD& mdn) const {      // loads of x(t) and its norm (mdn comes in as md)
        if (has_row_norm()) mdn = md_row[t];
#pragma unroll
        for (int i = 0; i < NG; ++i) xr[i] = goff[i] >= 0 ? gbase[goff[i] + t * gstep] : 0.0f;
    }
    __device__ __forceinline__ void store_next(const float (&xr)[NG], const NormMD& mdn) const {
#pragma unroll
        for (int i = 0; i < NG; ++i)
            if (!HOLES || goff[i] != -2) Xf[xdst[i]] = goff[i] >= 0 ? (xr[i] - mdn.m) / mdn.d : 0.0f;
    }
};

// ---- Linear epilogue of the 32-row kernels: waves 0..3 each sum 8 rows x 2 outputs x 4 k-parts of Wfc . h1 (rows 0..31)
template <int HID>
struct RowTileFc {
    int row, o, kp;                   // sum(): the sum for (row, o), in every lane of its 4 k-parts; store(): out[row's plane o][col] = act(sum + bias)
    __device__ __forceinline__ RowTileFc(int wave, int lane) : row((wave & 3) * 8 + (lane & 7)), o((lane >> 3) & 1), kp(lane >> 4) {}
    __device__ __forceinline__ float sum(const float4* __restrict__ H1s, const float4* __restrict__ Wfc4) const {
        constexpr int KGH = HID / 8, KGP = KGH / 4;
        static_assert(KGH % 4 == 0, "FC k-split");
        float s = 0.0f;
#pragma unroll 4
        for (int kk = 0; kk < KGP; ++kk) {
            const int kg = kp * KGP + kk;
#pragma unroll
            for (int kh = 0; kh < 2; ++kh) {
                const float4 h4 = H1s[kg * 64 + kh * 32 + row];
                const float4 w4 = Wfc4[(o * KGH + kg) * 2 + kh];
                s += h4.x * w4.x + h4.y * w4.y + h4.z * w4.z + h4.w * w4.w;
            }
        }
        s += __shfl_xor(s, 16);
        s += __shfl_xor(s, 32);
        return s;
    }
    __device__ __forceinline__ void store(const LstmWeights& w, const LstmArgs& a, const RowDesc& rd, float s, int col) const {
        a.out[(size_t)rd.out_off + (size_t)o * a.out_stride_o + col] = apply_act(s + w.bfc[o], a.act);
    }
};

}  // namespace fsnp
