// Shared host/device helpers for libpulsarutils_hip (gfx950).  What needs no HIP
// (set_error, PU_REQUIRE, elem_size, the tuning knobs) is in pu_host.h.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <utility>

#include "pu_host.h"
#include "pulsarutils_hip.h"

namespace pu {

// Map a HIP status to PU_EHIP with a message; returns PU_OK on success.
inline int hip_check(hipError_t e, const char *what)
{
    if (e == hipSuccess) return PU_OK;
    set_error("%s: %s", what, hipGetErrorString(e));
    return e == hipErrorOutOfMemory ? PU_ENOMEM : PU_EHIP;
}

#define PU_TRY_HIP(expr)                                  \
    do {                                                  \
        int _rc = ::pu::hip_check((expr), #expr);         \
        if (_rc != PU_OK) return _rc;                     \
    } while (0)

// Launch-error check after a kernel launch.
inline int launch_check(const char *name)
{
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) return PU_OK;
    set_error("launch %s: %s", name, hipGetErrorString(e));
    return PU_EHIP;
}

inline hipStream_t as_stream(void *s) { return reinterpret_cast<hipStream_t>(s); }

// Raise a kernel's dynamic LDS limit (ensure_lds, and the one caller that raises it once per
// device for every later launch).
template <typename Kern>
int raise_lds(Kern kern, size_t bytes)
{
    return hip_check(hipFuncSetAttribute(reinterpret_cast<const void *>(kern),
                                         hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes),
                     "hipFuncSetAttribute(MaxDynamicSharedMemorySize)");
}

// Dynamic LDS above 64 KiB needs the kernel's attribute raised before its launch.
template <typename Kern>
int ensure_lds(Kern kern, size_t bytes)
{
    return bytes <= 64 * 1024 ? PU_OK : raise_lds(kern, bytes);
}

// One launch with its own check: raise the LDS attribute where needed, launch, report.
// Launches that share one launch_check stay hipLaunchKernelGGL.
template <typename... P, typename... A>
int launch(const char *name, void (*kern)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream,
           A &&...args)
{
    if (int rc = ensure_lds(kern, lds_bytes)) return rc;
    hipLaunchKernelGGL(kern, grid, block, lds_bytes, stream, std::forward<A>(args)...);
    return launch_check(name);
}

// The element type a dtype code names, as a tag a generic lambda can take:
//     [&](auto tag) { using T = typename decltype(tag)::type; ... }
template <typename T>
struct type_tag {
    using type = T;
};
template <typename T>
constexpr int dtype_of = -1;
template <>
inline constexpr int dtype_of<uint8_t> = PU_U8;
template <>
inline constexpr int dtype_of<float> = PU_F32;
template <>
inline constexpr int dtype_of<double> = PU_F64;
template <>
inline constexpr int dtype_of<int64_t> = PU_I64;

// f(type_tag<T>{}) for the T among Ts... that dtype names; PU_EUNSUPPORTED for any other.
template <typename... Ts, typename F>
int with_dtype(const char *who, int dtype, F &&f)
{
    int rc = PU_EUNSUPPORTED;
    const bool known = ((dtype == dtype_of<Ts> && ((rc = f(type_tag<Ts>{})), true)) || ...);
    if (!known) set_error("%s: unsupported dtype %d", who, dtype);
    return rc;
}

// XCD-aware bijective block remap (cdna_hip_programming.md §5 "XCD swizzle must be
// bijective"): consecutive logical ids land on one XCD (blocks b, b+8 share one).
__device__ __forceinline__ int xcd_remap(int bid, int nblk)
{
    const int xcd = bid & 7, q = nblk >> 3, r = nblk & 7;
    return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);
}

}  // namespace pu
