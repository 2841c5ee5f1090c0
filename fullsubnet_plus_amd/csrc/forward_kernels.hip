// forward_kernels.hip - the small kernels of the forward's orchestration (fsnp_abi.hip) and their launchers: the row descriptors of
// the sub-band problem, the prologue that zeroes the workspace and describes the rows in one launch, and the per-utterance lengths.
#include <algorithm>

#include "fsnp_common.h"
#include "fsnp_handle.h"
#include "weight_watch.h"

namespace fsnp {

// Row slots of the sub-band problem.  Tile i owns `rt` slots (32 MFMA rows + ex VALU rows) and gets
// base (+1 for the first rem tiles) consecutive sequences; slot -> (utterance, frequency, output offset).
__device__ __forceinline__ void build_rows_slot(RowDesc* rows, int slot, int num_rows, int num_tiles, int rt, int F, int T, int mode,
                                                int batch_offset, int global_batch, int dense_out, int n_base, int groups, int OC) {
    const int tile = slot / rt, sl = slot % rt;
    const int base = num_rows / num_tiles, rem = num_rows % num_tiles;
    const int cnt = base + (tile < rem ? 1 : 0);
    const int n = n_base + tile * base + (tile < rem ? tile : rem) + sl;      // n_base: first sequence of this chunk
    RowDesc r{0, 0, 0, 0};
    if (sl < cnt) {
        r.valid = 1;
        if (dense_out) {               // fsnp_lstm2_fc: x[n][t][:] -> out[n][o][t], o < OC = output_size (fullsubnet_plus.py:104,206)
            r.b = n; r.f = 0; r.out_off = n * OC * T;
        } else if (mode == FSNP_MODE_FULL) {
            r.b = n / F; r.f = n % F;
            r.out_off = ((r.b * OC) * F + r.f) * T;
        } else {                       // drop_band (feature.py:254-285) with G = num_groups_in_drop_band groups:
            // global sample s keeps bins p + G i (p = s % G, i < (F - F % G) / G); output rows = group 0's samples, group 1's, ...
            const int G = groups, Fh = F / G;
            r.b = n / Fh;
            const int i = n % Fh;
            const int s = batch_offset + r.b, p = s % G;
            int orow = s / G;
            for (int q = 0; q < p; ++q) orow += (global_batch - q + G - 1) / G;     // samples of the groups in front
            r.f = p + G * i;
            r.out_off = ((orow * OC) * Fh + i) * T;
        }
    }
    rows[slot] = r;
}
__global__ void build_rows_kernel(RowDesc* rows, int num_rows, int num_tiles, int rt, int F, int T, int mode,
                                  int batch_offset, int global_batch, int dense_out, int n_base, int groups, int OC) {
    const int slot = blockIdx.x * blockDim.x + threadIdx.x;
    if (slot >= num_tiles * rt) return;
    build_rows_slot(rows, slot, num_rows, num_tiles, rt, F, T, mode, batch_offset, global_batch, dense_out, n_base, groups, OC);
}
void launch_build_rows(RowDesc* rows, const RowTiles& t, const RowLayout& l, hipStream_t s) {
    hipLaunchKernelGGL(build_rows_kernel, dim3(cdiv(t.num_tiles * t.rows_per_tile, 256)), dim3(256), 0, s, rows, t.num_rows, t.num_tiles,
                       t.rows_per_tile, l.F, l.T, l.mode, l.batch_offset, l.global_batch, l.dense_out, t.row0, l.groups, l.OC);
}
void launch_build_rows(const SbPlan& plan, RowDesc* rows, const RowLayout& l, hipStream_t s) {
    for (const SbChunk& c : plan.chunks) launch_build_rows(rows + c.slot0, {c.nrows, c.num_tiles, c.rps, c.row0}, l, s);
}

// Zeroes the accumulator / exchange / barrier region of the workspace.  A kernel rather than hipMemsetAsync: a memset
// node captured into the hipGraph was NOT re-executed reliably on replay (ROCm 7.2: stale barrier counters and
// accumulators after the first launch - tests/test_gpu_parity.py::test_b32_batch_independence caught it).
__global__ __launch_bounds__(256) void zero_region_kernel(uint4* __restrict__ p, size_t n16) {
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n16; i += stride) p[i] = make_uint4(0u, 0u, 0u, 0u);
}
void launch_zero_region(void* p, size_t bytes, hipStream_t s) {      // bytes is a multiple of 256
    const size_t n16 = bytes / 16;
    if (n16 == 0) return;
    const int blocks = (int)((n16 + 255) / 256 < 2048 ? (n16 + 255) / 256 : 2048);
    hipLaunchKernelGGL(zero_region_kernel, dim3(blocks), dim3(256), 0, s, reinterpret_cast<uint4*>(p), n16);
}

// ---- the forward's prologue as ONE launch (round 5; it used to be a zeroing kernel, a build_rows launch per chunk and, with a weight
// watch, the fingerprint kernel - three to six dependent launches of ~5 us each in front of a 250 us full-band stage at B = 1):
// blocks [0, zb) zero the accumulator / exchange / counter region, [zb, zb + rb) describe the sub-band rows of every chunk, the rest
// fingerprint the watched source tensors (fsnp_watch_weights).
struct PrologueChunk { int slot0, nrows, tiles, rt, row0, blocks; };
struct PrologueArgs {
    uint4* zero; size_t n16; int zero_blocks;
    RowDesc* rows; PrologueChunk chunk[kPrologueChunks]; int nchunks, rows_blocks;
    int F, T, mode, batch_offset, global_batch, groups, OC;
    const WatchSeg* segs; int nseg, watch_blocks; unsigned long long* watch_acc; unsigned* err_host;
};
__global__ __launch_bounds__(256) void prologue_kernel(PrologueArgs a) {
    const int b = blockIdx.x;
    if (b < a.zero_blocks) {
        const size_t stride = (size_t)a.zero_blocks * 256;
        for (size_t i = (size_t)b * 256 + threadIdx.x; i < a.n16; i += stride) a.zero[i] = make_uint4(0u, 0u, 0u, 0u);
        return;
    }
    int rb = b - a.zero_blocks;
    if (rb < a.rows_blocks) {
        for (int c = 0; c < a.nchunks; ++c) {
            const PrologueChunk k = a.chunk[c];
            if (rb < k.blocks) {
                const int slot = rb * 256 + threadIdx.x;
                if (slot < k.tiles * k.rt)
                    build_rows_slot(a.rows + k.slot0, slot, k.nrows, k.tiles, k.rt, a.F, a.T, a.mode, a.batch_offset, a.global_batch, 0, k.row0, a.groups, a.OC);
                return;
            }
            rb -= k.blocks;
        }
        return;
    }
    weight_watch_block(a.segs, a.nseg, a.watch_acc, 0, a.err_host, b - a.zero_blocks - a.rows_blocks, a.watch_blocks);
}
void launch_prologue_kernel(const fsnp_handle* h, const SbPlan& plan, RowDesc* rows, const RowLayout& l, void* zero, size_t zero_bytes,
                            bool watch, hipStream_t s) {
    PrologueArgs pa{};
    pa.zero = reinterpret_cast<uint4*>(zero);
    pa.n16 = zero_bytes / 16;
    pa.zero_blocks = (int)std::min<size_t>((pa.n16 + 255) / 256, 2048);
    pa.rows = rows;
    for (const SbChunk& c : plan.chunks) {
        PrologueChunk& k = pa.chunk[pa.nchunks++];
        k.slot0 = c.slot0; k.nrows = c.nrows; k.tiles = c.num_tiles; k.rt = c.rps; k.row0 = c.row0; k.blocks = cdiv(c.num_tiles * c.rps, 256);
        pa.rows_blocks += k.blocks;
    }
    pa.F = l.F; pa.T = l.T; pa.mode = l.mode; pa.batch_offset = l.batch_offset; pa.global_batch = l.global_batch;
    pa.groups = l.groups; pa.OC = l.OC;
    pa.segs = static_cast<const WatchSeg*>(h->watch_segs); pa.nseg = watch ? h->watch_nseg : 0;
    pa.watch_blocks = watch ? std::min(h->watch_nseg, kWatchBlocks) : 0;
    pa.watch_acc = h->watch_acc; pa.err_host = h->d_err;
    hipLaunchKernelGGL(prologue_kernel, dim3(pa.zero_blocks + pa.rows_blocks + pa.watch_blocks), dim3(256), 0, s, pa);
}

// ---- clips of different lengths (fsnp_forward_lengths).  The host's lengths reach the workspace as kernel arguments - no copy from
// pageable memory, nothing to synchronise, the caller may reuse its buffer when the call returns - 256 utterances per launch:
// lens[b] = lengths[b], tpb[b] = lengths[b] + look_ahead (Dims::lens / Dims::tpb)
constexpr int kLengthsPerLaunch = 256;
struct LengthArgs { int* lens; int* tpb; int b0, n, LA; int v[kLengthsPerLaunch]; };
__global__ __launch_bounds__(kLengthsPerLaunch) void set_lengths_kernel(LengthArgs a) {
    const int i = threadIdx.x;
    if (i < a.n) { a.lens[a.b0 + i] = a.v[i]; a.tpb[a.b0 + i] = a.v[i] + a.LA; }
}
void launch_set_lengths(const int32_t* lengths, int B, int LA, int* lens, int* tpb, hipStream_t s) {
    for (int b0 = 0; b0 < B; b0 += kLengthsPerLaunch) {
        LengthArgs a{};
        a.lens = lens; a.tpb = tpb; a.b0 = b0; a.n = std::min(kLengthsPerLaunch, B - b0); a.LA = LA;
        for (int i = 0; i < a.n; ++i) a.v[i] = lengths[b0 + i];
        hipLaunchKernelGGL(set_lengths_kernel, dim3(1), dim3(kLengthsPerLaunch), 0, s, a);
    }
}
// frames [lengths[b], T) of every row of utterance b of the [B][rows_per_utt][T] mask are written as 0 (the sub-band model ran over
// them: causal, so the frames before lengths[b] never saw them, but what it wrote there is no part of the clip)
__global__ __launch_bounds__(256) void zero_tails_kernel(float* __restrict__ out, const int* __restrict__ lens, int rows_per_utt, int T,
                                                         long total) {
    for (long i = (long)blockIdx.x * 256 + threadIdx.x; i < total; i += (long)gridDim.x * 256) {
        const long row = i / T;
        const int t = (int)(i - row * T);
        if (t >= lens[row / rows_per_utt]) out[i] = 0.0f;
    }
}
void launch_zero_tails(float* out, const int* lens, int B, int rows_per_utt, int T, hipStream_t s) {
    const long total = (long)B * rows_per_utt * T;
    const int blocks = (int)std::min<long>((total + 255) / 256, 4096);
    hipLaunchKernelGGL(zero_tails_kernel, dim3(blocks), dim3(256), 0, s, out, lens, rows_per_utt, T, total);
}

}  // namespace fsnp
