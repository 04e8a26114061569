// launch.h -- host-only helpers shared by the launchers: the per-device LDS opt-in, the dtype ladders, the dropout constants.
// Grids, streams and hipLaunchKernelGGL stay with the caller.
#pragma once
#include "common.h"

namespace amds {

// More than 64 KB of dynamic LDS needs hipFuncAttributeMaxDynamicSharedMemorySize, and the attribute belongs to a (kernel, device) pair: a process
// that drives several cards has to opt in on each.  Applied once per pair: one bit per device in a mask that lives with the kernel instantiation;
// two threads that race on a first launch both set the same value.  `bytes` is the largest request the kernel will ever see (it limits, it does
// not reserve), so a launcher whose request varies passes its bound.
template <auto Kernel>
inline hipError_t lds_opt_in(int bytes) {
    static std::atomic<uint64_t> done{0};
    int dev = -1;
    const hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    if (dev < 0 || dev >= MAX_DEV) return hipErrorInvalidDevice;
    const uint64_t bit = uint64_t(1) << dev;
    if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
    const hipError_t s = hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
    if (s == hipSuccess) done.fetch_or(bit, std::memory_order_release);
    return s;
}

// dtype ladders: f(Tag<T>{}) for the element type of an AMDS_* code, false for any other code -- the caller keeps its own message and AMDS_ERR_INVALID.
// Kernels with several independent dtypes nest the calls; a pair that has no kernel is refused before the dispatch or by `if constexpr` on the tags.
template <typename T> struct Tag { typedef T type; };
template <typename F>
inline bool dispatch_16(int dtype, F&& f) {
    if (dtype == AMDS_F16) f(Tag<f16>{});
    else if (dtype == AMDS_BF16) f(Tag<bf16>{});
    else return false;
    return true;
}
template <typename F>
inline bool dispatch_16_32(int dtype, F&& f) {
    if (dtype == AMDS_F32) f(Tag<float>{});
    else return dispatch_16(dtype, f);
    return true;
}
// the first ladder for a lambda that can fail (an LDS opt-in in front of its launch): *rc receives the status it returns
template <typename F>
inline bool dispatch_16(int dtype, int* rc, F&& f) {
    return dispatch_16(dtype, [&](auto t) { *rc = f(t); });
}
#define AMDS_TAG_T(tag) typename decltype(tag)::type

// threshold and keep scale of a dropout rate (common.h, "dropout bits"); p = 0 gives {0, 1}: nothing dropped, nothing scaled
struct DropParams {
    uint32_t thr;
    float scale;
    explicit DropParams(float p) : thr(drop_thr16(p)), scale(drop_scale(thr)) {}
};

}  // namespace amds
