// weight_layouts.h - every layout of the packed weight blob, stated once.  pack_ref() maps a position of an image to where its value
// comes from: an element of a source tensor, the sum or product of two, or zero.  The host packer (pack_image_host, behind
// fsnp_commit_weights and the fsnp_debug_*_pack hooks), the device packer (weight_pack.hip, behind fsnp_commit_weights_on) and
// fsnp_debug_pack_emulate all walk an image through this one function, so they cannot disagree about a layout.
//
// Sources are addressed inside ONE arena (all parameters of a handle, back to back in fsnp_weight_info order; host copy or device
// copy): PackJob::s[i] is the arena offset of source i.  Recurrent images take the reference's own tensors: s[0..3] = weight_ih_l0,
// weight_hh_l0, weight_ih_l1, weight_hh_l1 ([G H][cols], G = 4 gates of an LSTM or 3 of a GRU), s[4..7] = bias_ih_l0, bias_hh_l0,
// bias_ih_l1, bias_hh_l1.  The kernels see FOUR column slots per hidden unit: LSTM i, f, g, o; GRU r, z, n_x, n_h with W_in only in
// the input matrices and W_hn only in the hidden ones (zero blocks elsewhere), biases b_ir + b_hr, b_iz + b_hz, b_in, b_hn - rnn_w /
// rnn_bias below are that spread.
#pragma once
#include <cstdint>
#include <cstring>
#include <vector>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FSNP_HD __host__ __device__
#else
#define FSNP_HD
#endif

namespace fsnp {

constexpr int kFbvXP = 288;                 // lstm_fbv.hip: x part of layer 0's k range (num_freqs <= 288, zero padded)
constexpr int kFbvK0 = 100, kFbvK1 = 128;   // weights per thread: layer 0 (8 slices x 100 = 288 + 512), layer 1 (8 x 128 = 512 + 512)

enum PackKind : int {
    PK_ROWTILE = 0,   // lstm.hip         p = {H, NIN, KX, NW, gru}      [wave][k-group][tile][lane][k-pair]
    PK_ROWTILE_BF,    // lstm.hip         the same with W_ih1 as bf16 k-steps and b_ih0 + b_hh0 in input column k = NIN
    PK_HALF,          // lstm16.hip       p = {H, NIN, KX}               [wave][k-group of 16][tile][lane][q]
    PK_HALF_BF,       // lstm16.hip       W_ih1 as bf16 k-steps of 32
    PK_GRU,           // lstm_gru.hip     p = {H, NIN, KX, NW, 1}        [wave][k-group][live tile][lane][k-pair]
    PK_KSPLIT,        // lstm_coop.hip    p = {H, NIN, KX, units, gru}   [slice][wave][local k-group][tile][lane][k-pair]
    PK_COOPN,         // lstm_coopn.hip   p = {H, NIN, KX, 0, gru}       [32-unit block][k-group][gate][lane][k-pair]
    PK_HP,            // lstm_hp.hip      p = {H, NIN, KX}               [slice][gate][fragment][lane][4]
    PK_HPW,           // lstm_hpw.hip     p = {H, NIN, KX}               [participant][fragment][lane][4]
    PK_COOPW,         // lstm_coopw.hip   p = {H, NIN, KX}               [k-group][8-unit block][lane][k-pair]
    PK_FBV,           // lstm_fbv.hip     p = {H, NIN}                   [slice][fragment][thread][4]
    PK_GENERIC,       // lstm_generic.hip p = {H, NIN, 0, 0, gru}        [layer][k][4H]
    PK_BIAS,          // summed biases    p = {H, 0, 0, 0, gru}          [layer][4H]
    PK_SPREAD,        // four-slot matrix p = {H, NIN, 0, m, gru}        [4H][cols] of source m (what the kernels' images are cut from)
    PK_PADMAT,        // s[0] [R][C] -> [NP][KP], zero padded            p = {R, C, NP, KP}   (R = NP = 1: a plain copy)
    PK_TRANSPOSE,     // s[0] [R][C] -> [C][R]                            p = {R, C}
    PK_FOLDW,         // s[0] W [R][C] times s[1] gamma [C] -> [NP][KP]   p = {R, C, NP, KP}   (GroupNorm 2 folded into the sconv GEMM)
    PK_FOLDC,         // its two per-row constants, fp64 sums over C      p = {R, C, NP, which} s = {W, gamma, beta, bias}
    PK_COUNT
};

// One image of the blob.  `n` floats at blob offset `out`; the first nsub * sub of them are nsub sub-images of one layout whose
// sources sit at a regular distance in the arena (TCN blocks inside a model: stride_in, models: stride_out), the rest is zero.
struct PackJob {
    int kind;
    int p[8];
    long long s[8];
    long long out, n, sub;
    int nsub, nb;
    long long stride_in, stride_out;
};

enum PackOp : int { OP_ONE = 0, OP_ADD = 1, OP_DMUL = 2 };
struct PackRef {
    int a; long long ia;      // source index into PackJob::s and element offset; a < 0: the value is zero
    int b; long long ib;      // second operand of OP_ADD / OP_DMUL
    int op;
};
FSNP_HD inline PackRef ref_zero() { return PackRef{-1, 0, -1, 0, OP_ONE}; }
FSNP_HD inline PackRef ref_one(int a, long long ia) { return PackRef{a, ia, -1, 0, OP_ONE}; }

// element (row, k) of the four-slot matrix of source m (0 W_ih0, 1 W_hh0, 2 W_ih1, 3 W_hh1); row in [0, 4H)
FSNP_HD inline PackRef rnn_w(const int* p, int m, long long row, long long k) {
    const int H = p[0], cols = m == 0 ? p[1] : H;
    if (p[4]) {
        const int slot = (int)(row / H);
        const bool hidden = (m & 1) != 0;
        if (slot == 2 && hidden) return ref_zero();
        if (slot == 3) { if (!hidden) return ref_zero(); row -= H; }
    }
    return ref_one(m, row * cols + k);
}
// element i in [0, 4H) of the summed bias of layer l
FSNP_HD inline PackRef rnn_bias(const int* p, int l, long long i) {
    const int H = p[0];
    if (!p[4] || i < 2 * H) return PackRef{4 + 2 * l, i, 5 + 2 * l, i, OP_ADD};
    if (i < 3 * H) return ref_one(4 + 2 * l, i);
    return ref_one(5 + 2 * l, i - H);
}

FSNP_HD inline int coop_kgxp(int KX) { return (KX / 8 + 3) / 4 * 4; }
FSNP_HD inline int gx16(int KX) { return (KX + 15) / 16; }

// floats of one (sub-)image
FSNP_HD inline long long pack_floats(int kind, const int* p) {
    const long long H = p[0], KX = p[2], P = p[3];
    switch (kind) {
    case PK_ROWTILE: return P * (KX / 8 + 3 * (H / 8)) * (4 * (H / P / 32)) * 256;
    case PK_ROWTILE_BF: return P * (KX / 8 + 2 * (H / 8) + H / 16) * (4 * (H / P / 32)) * 256;
    case PK_HALF: return 4 * (gx16((int)KX) + 3 * (H / 16)) * (4 * (H / 4 / 16)) * 256;
    case PK_HALF_BF: return 4 * (gx16((int)KX) + 2 * (H / 16) + H / 32) * (4 * (H / 4 / 16)) * 256;
    case PK_GRU: return P * (KX / 8 + 3 * (H / 8)) * (3 * (H / P / 32)) * 256;
    case PK_KSPLIT: return (H / P) * 4 * ((coop_kgxp((int)KX) + H / 8) / 4 + H / 16) * (P / 8) * 256;
    case PK_COOPN: return (H / 32) * (KX / 8 + 3 * (H / 8)) * 4 * 256;
    case PK_HP: case PK_HPW: return (H / 16) * 4 * (gx16((int)KX) + 3 * (H / 16)) * 256;
    case PK_COOPW: return (KX / 8 + 3 * (H / 8)) * (H / 8) * 256;
    case PK_FBV: return (H / 8) * (kFbvK0 + kFbvK1) * 256;
    case PK_GENERIC: return ((long long)p[1] + H) * 4 * H + 2 * H * 4 * H;
    case PK_BIAS: return 8 * H;
    case PK_SPREAD: return 4 * H * (p[3] == 0 ? p[1] : H);
    case PK_PADMAT: case PK_FOLDW: return (long long)p[2] * p[3];
    case PK_TRANSPOSE: return (long long)p[0] * p[1];
    case PK_FOLDC: return p[2];
    default: return 0;
    }
}

// the 16-byte unit u of the image holds 8 bf16 values instead of 4 floats
FSNP_HD inline bool pack_unit_bf16(const PackJob& J, long long u) {
    const int H = J.p[0], KX = J.p[2];
    if (J.kind == PK_ROWTILE_BF) {
        const int NW = J.p[3], NT = 4 * (H / NW / 32), KGH = H / 8, KG0 = KX / 8 + KGH, KGT = KG0 + KGH + H / 16;
        return u < J.n / 4 && (int)((u / 64 / NT) % KGT) >= KG0 + KGH;
    }
    if (J.kind == PK_HALF_BF) {
        const int NT = 4 * (H / 4 / 16), KGH = H / 16, KG0 = gx16(KX) + KGH, KGT = KG0 + KGH + H / 32;
        return u < J.n / 4 && (int)((u / 64 / NT) % KGT) >= KG0 + KGH;
    }
    return false;
}

// Where component j of unit u comes from (j in [0, 4): float 4 u + j of the image; a bf16 unit: j in [0, 8)).  *shift: what to add
// to the source offsets (the sub-image's distance from the first one in the arena).
FSNP_HD inline PackRef pack_ref(const PackJob& J, long long u, int j, long long* shift) {
    *shift = 0;
    const int* p = J.p;
    const int H = p[0], NIN = p[1], KX = p[2], P = p[3];
    const bool bf = pack_unit_bf16(J, u);
    long long pos = bf ? 4 * u : 4 * u + j;
    if (pos >= J.sub * J.nsub) return ref_zero();
    if (J.nsub > 1 || J.sub != J.n) {
        const long long bi = pos / J.sub;
        pos -= bi * J.sub;
        *shift = (bi / J.nb) * J.stride_out + (bi % J.nb) * J.stride_in;
    }
    const int c4 = (int)(pos & 3), lane = (int)((pos >> 2) & 63);
    const long long t = pos >> 8;          // index of the 64-lane fragment
    switch (J.kind) {
    case PK_ROWTILE: case PK_ROWTILE_BF: case PK_COOPN: case PK_COOPW: {
        // K order: layer 0 = [x (KX, zero padded) | h0], layer 1 = [h1 | h0]; k = 8 g + 2 p + (lane >> 5)
        const int KGX = KX / 8, KGH = H / 8, KG0 = KGX + KGH;
        long long wrow; int g;
        if (J.kind == PK_COOPN) {          // [ub][g][gate][lane][p]
            const int KGT = KG0 + 2 * KGH, gate = (int)(t % 4);
            g = (int)((t / 4) % KGT);
            wrow = (long long)gate * H + (t / 4 / KGT) * 32 + (lane & 31);
        } else if (J.kind == PK_COOPW) {   // [g][ub][lane][p]: column c = lane & 31 is gate c & 3 of unit 8 ub + (c >> 2)
            const int NUB = H / 8, c = lane & 31;
            g = (int)(t / NUB);
            wrow = (long long)(c & 3) * H + (t % NUB) * 8 + (c >> 2);
        } else {                           // [wv][g][n][lane][p]: tile n = gate * ST + s holds units wv UW + 32 s + (lane & 31)
            const int UW = H / P, ST = UW / 32, NT = 4 * ST;
            const int KGT = J.kind == PK_ROWTILE ? KG0 + 2 * KGH : KG0 + KGH + H / 16;
            const int n = (int)(t % NT), wv = (int)(t / NT / KGT);
            g = (int)((t / NT) % KGT);
            wrow = (long long)(n / ST) * H + wv * UW + (n % ST) * 32 + (lane & 31);
        }
        if (g < KG0) {
            const int k = 8 * g + 2 * c4 + (lane >> 5);
            if (k >= KX) return rnn_w(p, 1, wrow, k - KX);
            if (k < NIN) return rnn_w(p, 0, wrow, k);
            if (J.kind == PK_ROWTILE_BF && k == NIN) return rnn_bias(p, 0, wrow);    // the kernel feeds input slot NIN with the constant 1
            return ref_zero();
        }
        if (bf) return rnn_w(p, 2, wrow, 16 * (g - KG0 - KGH) + 8 * (lane >> 5) + j);
        const int k = 8 * (g - KG0) + 2 * c4 + (lane >> 5);
        return k < H ? rnn_w(p, 3, wrow, k) : rnn_w(p, 2, wrow, k - H);
    }
    case PK_HALF: case PK_HALF_BF: {       // [wv][g][n][lane][q]: tile n = gate * SB + s, units wv UW + 16 s + (lane & 15); k = 16 g + 4 q + (lane >> 4)
        const int UW = H / 4, SB = UW / 16, NT = 4 * SB, KGX = gx16(KX), KGH = H / 16, KG0 = KGX + KGH;
        const int KGT = J.kind == PK_HALF ? KG0 + 2 * KGH : KG0 + KGH + H / 32;
        const int n = (int)(t % NT), g = (int)((t / NT) % KGT), wv = (int)(t / NT / KGT);
        const long long wrow = (long long)(n / SB) * H + wv * UW + (n % SB) * 16 + (lane & 15);
        if (bf) return rnn_w(p, 2, wrow, 32 * (g - KG0 - KGH) + 8 * (lane >> 4) + j);
        const int kk = 4 * c4 + (lane >> 4);
        if (g < KGX) { const int k = 16 * g + kk; return k < NIN ? rnn_w(p, 0, wrow, k) : ref_zero(); }
        if (g < KG0) return rnn_w(p, 1, wrow, 16 * (g - KGX) + kk);
        if (g < KG0 + KGH) return rnn_w(p, 3, wrow, 16 * (g - KG0) + kk);
        return rnn_w(p, 2, wrow, 16 * (g - KG0 - KGH) + kk);
    }
    case PK_GRU: {                         // live tile n: slot n / ST for n < 2 ST, else slot 2 in an input segment, 3 in a hidden one
        const int UW = H / P, ST = UW / 32, NL = 3 * ST, KGX = KX / 8, KGH = H / 8, KG0 = KGX + KGH, KGT = KG0 + 2 * KGH;
        const int n = (int)(t % NL), g = (int)((t / NL) % KGT), wv = (int)(t / NL / KGT);
        const bool l0 = g < KG0, hidden = l0 ? g >= KGX : g < KG0 + KGH;
        const int m = l0 ? (hidden ? 1 : 0) : (hidden ? 3 : 2);
        const int cols = m == 0 ? NIN : H;
        const int g0 = l0 ? (hidden ? KGX : 0) : (hidden ? KG0 : KG0 + KGH);
        const int slot = n < 2 * ST ? n / ST : (hidden ? 3 : 2);
        const long long wrow = (long long)slot * H + wv * UW + (n % ST) * 32 + (lane & 31);
        const int k = 8 * (g - g0) + 2 * c4 + (lane >> 5);
        return k < cols ? rnn_w(p, m, wrow, k) : ref_zero();
    }
    case PK_KSPLIT: {                      // local group i of wave w is global k-group 4 i + w of its layer; column j = n 32 + (lane & 31) is gate j / units
        const int units = P, NT = units / 8, KGXP = coop_kgxp(KX), KGH = H / 8, G0W = (KGXP + KGH) / 4, GW = G0W + KGH / 2;
        const int n = (int)(t % NT), i = (int)((t / NT) % GW), wave = (int)((t / NT / GW) % 4), cs = (int)(t / NT / GW / 4);
        const int col = n * 32 + (lane & 31);
        const long long wrow = (long long)(col / units) * H + cs * units + col % units;
        if (i < G0W) {
            const int g = 4 * i + wave;
            if (g < KGXP) { const int k = 8 * g + 2 * c4 + (lane >> 5); return k < NIN ? rnn_w(p, 0, wrow, k) : ref_zero(); }
            return rnn_w(p, 1, wrow, 8 * (g - KGXP) + 2 * c4 + (lane >> 5));
        }
        const int k = 8 * (4 * (i - G0W) + wave) + 2 * c4 + (lane >> 5);
        return k < H ? rnn_w(p, 3, wrow, k) : rnn_w(p, 2, wrow, k - H);
    }
    case PK_HP: case PK_HPW: {             // fragments: x k-groups | W_hh0 | W_hh1 | W_ih1; k = 16 g + 4 j + (lane >> 4)
        const int GX = gx16(KX), GH = H / 16, NF = GX + 3 * GH;
        const int f = (int)(t % NF);
        long long wrow;
        if (J.kind == PK_HP) {             // [cs][gate][f]: column lane & 15 of slice cs
            const long long cg = t / NF;
            wrow = (cg % 4) * H + (cg / 4) * 16 + (lane & 15);
        } else {                           // [part = 4 cs + w][f]: M row m = lane & 15 = 4 jj + gate, unit 16 cs + w + 4 jj
            const long long part = t / NF;
            const int m = lane & 15;
            wrow = (long long)(m & 3) * H + (part >> 2) * 16 + (part & 3) + 4 * (m >> 2);
        }
        const int kk = 4 * c4 + (lane >> 4);
        if (f < GX) { const int k = 16 * f + kk; return k < NIN ? rnn_w(p, 0, wrow, k) : ref_zero(); }
        if (f < GX + GH) return rnn_w(p, 1, wrow, 16 * (f - GX) + kk);
        if (f < GX + 2 * GH) return rnn_w(p, 3, wrow, 16 * (f - GX - GH) + kk);
        return rnn_w(p, 2, wrow, 16 * (f - GX - 2 * GH) + kk);
    }
    case PK_FBV: {                         // thread (c = tid & 31, ks = tid >> 5): gate c & 3 of unit 8 cs + (c >> 2); layer 0 k = 100 ks + j over
        const int NF = (kFbvK0 + kFbvK1) / 4;      // [x (288) | h0], layer 1 k = 128 ks + j over [h0 | h1]
        const int tid = (int)((pos >> 2) & 255), f = (int)((pos >> 10) % NF), cs = (int)((pos >> 10) / NF);
        const int c = tid & 31, ks = tid >> 5, jj = 4 * f + c4;
        const long long wrow = (long long)(c & 3) * H + cs * 8 + (c >> 2);
        if (jj < kFbvK0) {
            const int k = kFbvK0 * ks + jj;
            if (k >= kFbvXP) return rnn_w(p, 1, wrow, k - kFbvXP);
            return k < NIN ? rnn_w(p, 0, wrow, k) : ref_zero();
        }
        const int k = kFbvK1 * ks + (jj - kFbvK0);
        return k < H ? rnn_w(p, 2, wrow, k) : rnn_w(p, 3, wrow, k - H);
    }
    case PK_GENERIC: {                     // transposed: layer 0 k = [x | h0], layer 1 k = [h0 | h1]
        const long long G4 = 4LL * H, L0 = (NIN + (long long)H) * G4;
        if (pos < L0) { const long long k = pos / G4, c = pos % G4; return k < NIN ? rnn_w(p, 0, c, k) : rnn_w(p, 1, c, k - NIN); }
        const long long k = (pos - L0) / G4, c = (pos - L0) % G4;
        return k < H ? rnn_w(p, 2, c, k) : rnn_w(p, 3, c, k - H);
    }
    case PK_BIAS: return rnn_bias(p, (int)(pos / (4LL * H)), pos % (4LL * H));
    case PK_SPREAD: { const int cols = P == 0 ? NIN : H; return rnn_w(p, P, pos / cols, pos % cols); }
    case PK_PADMAT: case PK_FOLDW: {
        const long long n = pos / p[3], k = pos % p[3];
        if (n >= p[0] || k >= p[1]) return ref_zero();
        if (J.kind == PK_PADMAT) return ref_one(0, n * p[1] + k);
        return PackRef{0, n * p[1] + k, 1, k, OP_DMUL};
    }
    case PK_TRANSPOSE: return ref_one(0, (pos % p[0]) * p[1] + pos / p[0]);
    default: return ref_zero();
    }
}

// float -> bf16, round to nearest even (the bf16-ih images)
FSNP_HD inline unsigned short bf16_rne(float v) {
    unsigned u;
#if defined(__HIP_DEVICE_COMPILE__)
    u = __float_as_uint(v);
#else
    memcpy(&u, &v, 4);
#endif
    return (unsigned short)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}

// fp64 product and sum that no compiler contracts into an FMA: host and device then round alike
FSNP_HD inline double mul_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dmul_rn(a, b);
#else
    volatile double r = a * b;
    return r;
#endif
}
FSNP_HD inline double add_rn(double a, double b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __dadd_rn(a, b);
#else
    volatile double r = a + b;
    return r;
#endif
}

FSNP_HD inline float pack_value(const PackJob& J, const float* arena, const PackRef& r, long long shift) {
    if (r.a < 0) return 0.0f;
    const float x = arena[J.s[r.a] + shift + r.ia];
    if (r.op == OP_ONE) return x;
    const float y = arena[J.s[r.b] + shift + r.ib];
    if (r.op == OP_ADD) return x + y;
    return (float)mul_rn((double)x, (double)y);
}

// unit u of the image -> 16 bytes at dst
FSNP_HD inline void pack_unit(const PackJob& J, const float* arena, long long u, float* dst) {
    long long shift;
    if (pack_unit_bf16(J, u)) {
        unsigned short* d16 = reinterpret_cast<unsigned short*>(dst);
        for (int j = 0; j < 8; ++j) { const PackRef r = pack_ref(J, u, j, &shift); d16[j] = bf16_rne(pack_value(J, arena, r, shift)); }
        return;
    }
    for (int j = 0; j < 4; ++j) { const PackRef r = pack_ref(J, u, j, &shift); dst[j] = pack_value(J, arena, r, shift); }
}

// PK_FOLDC, output row `row` of the padded vector: sum_k ((a - m) r g_k + b_k) W[n][k] = r sum_k a g_k W[n][k] + c1[n] - r m c2[n];
// c1 = bias[n] + sum_k beta_k W[n][k] (which = 0), c2 = sum_k gamma_k W[n][k] (which = 1), in fp64 and in k order
FSNP_HD inline float fold_row(const PackJob& J, const float* arena, long long row) {
    if (row >= J.sub * J.nsub) return 0.0f;
    const long long bi = row / J.sub, n = row % J.sub;
    const long long shift = (bi / J.nb) * J.stride_out + (bi % J.nb) * J.stride_in;
    const int R = J.p[0], C = J.p[1], which = J.p[3];
    if (n >= R) return 0.0f;
    const float* w = arena + J.s[0] + shift + n * C;
    const float* v = arena + J.s[which ? 1 : 2] + shift;
    double acc = which ? 0.0 : (double)arena[J.s[3] + shift + n];
    for (int k = 0; k < C; ++k) acc = add_rn(acc, mul_rn((double)v[k], (double)w[k]));
    return (float)acc;
}

// ---- host side ---------------------------------------------------------------------------------------------------------------
inline PackJob make_job(int kind, int p0, int p1 = 0, int p2 = 0, int p3 = 0, int p4 = 0) {
    PackJob J{};
    J.kind = kind;
    J.p[0] = p0; J.p[1] = p1; J.p[2] = p2; J.p[3] = p3; J.p[4] = p4;
    J.sub = J.n = pack_floats(kind, J.p);
    J.nsub = 1; J.nb = 1;
    return J;
}

// `count` floats of the image (from its start) into out
inline void pack_image_host(const PackJob& J, const float* arena, float* out, long long count) {
    if (J.kind == PK_FOLDC) {
        for (long long r = 0; r < count; ++r) out[r] = fold_row(J, arena, r);
        return;
    }
    for (long long u = 0; 4 * u < count; ++u) {
        if (4 * u + 4 <= count) { pack_unit(J, arena, u, out + 4 * u); continue; }
        float tmp[4];
        pack_unit(J, arena, u, tmp);
        memcpy(out + 4 * u, tmp, (size_t)(count - 4 * u) * 4);
    }
}

// the recurrent images as the fsnp_debug_*_pack hooks take them: four matrices that already have four slots ([4H][cols]), no biases
inline long long rnn_image_floats(int kind, int H, int NIN, int KX, int P) { return make_job(kind, H, NIN, KX, P, 0).n; }
inline void pack_rnn_host(int kind, int H, int NIN, int KX, int P, const float* wih0, const float* whh0, const float* wih1, const float* whh1,
                          float* out) {
    PackJob J = make_job(kind, H, NIN, KX, P, 0);
    const float* src[4] = {wih0, whh0, wih1, whh1};
    std::vector<float> arena;
    for (int i = 0; i < 4; ++i) {
        J.s[i] = (long long)arena.size();
        arena.insert(arena.end(), src[i], src[i] + (size_t)4 * H * (i == 0 ? NIN : H));
    }
    pack_image_host(J, arena.data(), out, J.n);
}

// device side (weight_pack.hip): one launch on the stream for `count` floats of the image
int launch_pack_image(const PackJob& J, const float* d_arena, long long arena_floats, float* d_blob, long long count, void* hip_stream);

}  // namespace fsnp
