// weight_pack.hip - the packed weight blob built on the device (fsnp_commit_weights_on): one kernel per image kind, every thread
// writes one 16-byte unit of its image (coalesced; zero padding written explicitly - the blob's allocation is not assumed to be zero)
// and gathers the unit's sources from the handle's device arena through pack_ref (weight_layouts.h), the function the host packer
// walks too.  The folded GroupNorm constants are fp64 sums: one thread per output row, in the host's term order.
#include "fsnp_common.h"
#include "weight_layouts.h"

namespace fsnp {

// (KIND is a template parameter so that each image kind is a kernel of its own with the other layouts compiled out)
template <int KIND>
__global__ __launch_bounds__(256) void pack_image_kernel(PackJob J, const float* __restrict__ arena, long long arena_floats,
                                                         float* __restrict__ blob, long long units) {
    const long long u = (long long)blockIdx.x * 256 + threadIdx.x;
    if (u >= units) return;
    J.kind = KIND;
    long long shift;
    // a source offset outside the arena reads as zero: the image is then wrong (and its test says so), the device is not harmed
    auto value = [&](int j) {
        const PackRef r = pack_ref(J, u, j, &shift);
        if (r.a < 0) return 0.0f;
        const long long ia = J.s[r.a] + shift + r.ia;
        if (ia < 0 || ia >= arena_floats) return 0.0f;
        const float x = arena[ia];
        if (r.op == OP_ONE) return x;
        const long long ib = J.s[r.b] + shift + r.ib;
        if (ib < 0 || ib >= arena_floats) return 0.0f;
        const float y = arena[ib];
        return r.op == OP_ADD ? x + y : (float)mul_rn((double)x, (double)y);
    };
    uint4 o;
    if ((KIND == PK_ROWTILE_BF || KIND == PK_HALF_BF) && pack_unit_bf16(J, u)) {
        unsigned w[4];
        for (int q = 0; q < 4; ++q) w[q] = (unsigned)bf16_rne(value(2 * q)) | ((unsigned)bf16_rne(value(2 * q + 1)) << 16);
        o = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        o = make_uint4(__float_as_uint(value(0)), __float_as_uint(value(1)), __float_as_uint(value(2)), __float_as_uint(value(3)));
    }
    reinterpret_cast<uint4*>(blob + J.out)[u] = o;
}

__global__ __launch_bounds__(64) void pack_fold_kernel(PackJob J, const float* __restrict__ arena, float* __restrict__ blob, long long rows) {
    const long long r = (long long)blockIdx.x * 64 + threadIdx.x;
    if (r < rows) blob[J.out + r] = fold_row(J, arena, r);
}

template <int KIND>
static void launch_kind(const PackJob& J, const float* arena, long long arena_floats, float* blob, long long units, hipStream_t s) {
    hipLaunchKernelGGL(pack_image_kernel<KIND>, dim3((unsigned)((units + 255) / 256)), dim3(256), 0, s, J, arena, arena_floats, blob, units);
}

// `count` floats (a multiple of 4) of image J, from blob + J.out; every source of J lies inside [arena, arena + arena_floats)
int launch_pack_image(const PackJob& J, const float* d_arena, long long arena_floats, float* d_blob, long long count, void* hip_stream) {
    hipStream_t s = static_cast<hipStream_t>(hip_stream);
    if (count <= 0) return 0;
    if (count % 4 != 0 || J.out % 4 != 0) { set_error("weight pack: image of kind %d is not a whole number of 16-byte units", J.kind); return 3; }
    if (J.kind == PK_FOLDC) {
        // (the rows read [R][C] matrices of the arena: checked here once instead of per element)
        const long long last = (long long)(J.nsub - 1) / J.nb * J.stride_out + (long long)(J.nsub - 1) % J.nb * J.stride_in;
        if (J.nsub > 0 && (J.s[0] + last + (long long)J.p[0] * J.p[1] > arena_floats || J.s[1] + last + J.p[1] > arena_floats ||
                           J.s[2] + last + J.p[1] > arena_floats || J.s[3] + last + J.p[0] > arena_floats)) {
            set_error("weight pack: a GroupNorm fold reads outside the arena"); return 3;
        }
        hipLaunchKernelGGL(pack_fold_kernel, dim3((unsigned)((count + 63) / 64)), dim3(64), 0, s, J, d_arena, d_blob, count);
        FSNP_HIP_CHECK(hipGetLastError());
        return 0;
    }
    const long long units = count / 4;
    switch (J.kind) {
    case PK_ROWTILE: launch_kind<PK_ROWTILE>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_ROWTILE_BF: launch_kind<PK_ROWTILE_BF>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_HALF: launch_kind<PK_HALF>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_HALF_BF: launch_kind<PK_HALF_BF>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_GRU: launch_kind<PK_GRU>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_KSPLIT: launch_kind<PK_KSPLIT>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_COOPN: launch_kind<PK_COOPN>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_HP: launch_kind<PK_HP>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_HPW: launch_kind<PK_HPW>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_COOPW: launch_kind<PK_COOPW>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_FBV: launch_kind<PK_FBV>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_GENERIC: launch_kind<PK_GENERIC>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_BIAS: launch_kind<PK_BIAS>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_SPREAD: launch_kind<PK_SPREAD>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_PADMAT: launch_kind<PK_PADMAT>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_TRANSPOSE: launch_kind<PK_TRANSPOSE>(J, d_arena, arena_floats, d_blob, units, s); break;
    case PK_FOLDW: launch_kind<PK_FOLDW>(J, d_arena, arena_floats, d_blob, units, s); break;
    default: set_error("weight pack: unknown image kind %d", J.kind); return 3;
    }
    FSNP_HIP_CHECK(hipGetLastError());
    return 0;
}

}  // namespace fsnp
