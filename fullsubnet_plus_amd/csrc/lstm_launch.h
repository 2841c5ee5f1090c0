// lstm_launch.h - host launch glue shared by the recurrent kernel files (lstm*.hip): LDS opt-in + residency check, the launch of a
// column-split kernel, runtime -> template-parameter dispatch.  Device helpers: lstm_common.h.
#pragma once
#include <type_traits>

#include "lstm_common.h"

namespace fsnp {

// LDS opt-in of kernel KERN (per device) + a residency check: a workgroup of `threads` threads with `smem` bytes of dynamic LDS must
// fit a CU.  smem == 0: the opt-in only.  Returns hipSuccess, or the error of the attribute call (kept per device: a failure on one
// GPU is that GPU's alone) / hipErrorLaunchOutOfResources when no workgroup fits.
template <auto KERN>
hipError_t lds_opt_in(int max_dyn, int threads, size_t smem) {
    const void* k = reinterpret_cast<const void*>(KERN);
    static PerDeviceOnce once;
    static hipError_t attr_err[64] = {};
    int dev = 0;
    (void)hipGetDevice(&dev);
    const int di = dev >= 0 && dev < 64 ? dev : 0;
    once.run([&] { attr_err[di] = hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, max_dyn); });
    if (attr_err[di] != hipSuccess) return attr_err[di];
    if (smem == 0) return hipSuccess;
    int blocks = 0;
    const hipError_t e = hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, k, threads, smem);
    if (e != hipSuccess) return e;
    return blocks >= 1 ? hipSuccess : hipErrorLaunchOutOfResources;
}

constexpr int kCuLds = 160 * 1024;      // LDS of one CU; a kernel may opt in to all of it minus its static __shared__ words

// Launch of column-split kernel KERN: `tiles` row tiles (or groups of them) x S workgroups of 256 threads, all co-resident, placed
// XCD-locally with a.coop_xcd (lstm_common.h).  occ != nullptr: do not launch; report how many workgroups with smem_need bytes of
// dynamic LDS fit one CU at once (0 = unknown).  LstmArgs::coop_own_cu claims the rest of the CU's LDS as (unused) dynamic LDS so
// that no LDS-using workgroup of a concurrent kernel shares the CU (pipelined loop: the next forward's full-band GEMMs).  Two rules:
//   STATIC_LDS = false: the kernel's static LDS counts as 256 bytes; a.coop_own_cu is the dynamic size to launch with
//   STATIC_LDS = true : the kernel's static LDS is looked up; a.coop_own_cu is the workgroup's whole LDS (lstm_coopn.hip)
// EVERY_CALL: the opt-in is repeated at every launch (the phase-profile variants).
template <auto KERN, bool STATIC_LDS = false, bool EVERY_CALL = false>
void launch_column_split(const LstmWeights& w, const LstmArgs& a, hipStream_t s, int S, int tiles, size_t smem_need, int* occ) {
    const void* k = reinterpret_cast<const void*>(KERN);
    static PerDeviceOnce once;                 // the attribute is per device: one process may drive several GPUs
    static int static_lds = 0;
    auto opt_in = [&] {
        if constexpr (STATIC_LDS) {
            hipFuncAttributes fa{};
            if (hipFuncGetAttributes(&fa, k) == hipSuccess) static_lds = (int)fa.sharedSizeBytes;
        }
        (void)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, kCuLds - (STATIC_LDS ? static_lds : 256));
    };
    if constexpr (EVERY_CALL) opt_in(); else once.run(opt_in);
    if (occ) {
        if (hipOccupancyMaxActiveBlocksPerMultiprocessor(occ, k, 256, smem_need) != hipSuccess) *occ = 0;
        return;
    }
    const int own = a.coop_own_cu > 0 ? a.coop_own_cu - static_lds : 0;
    const size_t smem = own > 0 && (size_t)own > smem_need ? (size_t)own : smem_need;
    const int grid = a.coop_xcd ? 8 * xcd_local_blocks_per_xcd(S, tiles, a.coop_xcd) : tiles * S;
    hipLaunchKernelGGL(KERN, dim3(grid), dim3(256), smem, s, w, a);
}

// Runtime value -> template parameter: f(integral_constant<int, V>) for the first listed V == v; the LAST one listed also takes
// every other v.  A file states its instantiated sizes once, for its launch entry and its occupancy entry alike.
template <int V, int... Rest, typename F>
void dispatch_int(int v, F&& f) {
    if constexpr (sizeof...(Rest) == 0) f(std::integral_constant<int, V>{});
    else if (v == V) f(std::integral_constant<int, V>{});
    else dispatch_int<Rest...>(v, f);
}
template <typename F>
void dispatch_bool(bool v, F&& f) {
    if (v) f(std::true_type{}); else f(std::false_type{});
}

}  // namespace fsnp
