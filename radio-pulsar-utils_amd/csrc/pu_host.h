// Host-only helpers of libpulsarutils_hip: the error state, argument checks and tuning
// knobs.  Plain C++ (no HIP): the planner's translation units include this, the device
// units get it through pu_common.h.
#pragma once
#include <cstddef>
#include <cstdlib>

#include "pulsarutils_hip.h"

namespace pu {

void set_error(const char *fmt, ...);

#define PU_REQUIRE(cond, ...)                             \
    do {                                                  \
        if (!(cond)) {                                    \
            ::pu::set_error(__VA_ARGS__);                 \
            return PU_EINVAL;                             \
        }                                                 \
    } while (0)

inline size_t elem_size(int dtype)
{
    switch (dtype) {
    case PU_U8: return 1;
    case PU_F32: return 4;
    case PU_F64: return 8;
    case PU_I64: return 8;
    default: return 0;
    }
}

// Tuning knobs for A/B experiments (group size, workgroup shape, batch sizes ...): read
// from the environment ONLY in the diagnostic build (make stamps: -DPU_STAMPS,
// libpulsarutils_hip_stamps.so).  The production library ignores the environment and
// always runs its defaults or the explicit plan-create arguments, so a stray PU_* in a
// user's environment cannot change a kernel (the reference is configured by kwargs only).
inline bool knob_set(const char *name)
{
#ifdef PU_STAMPS
    return getenv(name) != nullptr;
#else
    (void)name;
    return false;
#endif
}

inline int knob(const char *name, int dflt)
{
#ifdef PU_STAMPS
    if (const char *e = getenv(name)) return atoi(e);
#endif
    (void)name;
    return dflt;
}

}  // namespace pu
