// Host-only helpers of libpulsarutils_hip: the error state, argument checks, workspace
// layout and tuning knobs.  Plain C++ (no HIP): the planner's translation units include
// this, the device units get it through pu_common.h.
#pragma once
#include <cstddef>
#include <cstdint>
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

// Workspace pieces start on 256-byte boundaries.
inline size_t up256(size_t b) { return (b + 255) & ~size_t(255); }

// The one workspace check of an entry point: non-null, large enough, aligned.
inline int check_workspace(const char *who, const void *ptr, size_t got, size_t need, size_t align)
{
    PU_REQUIRE(ptr && got >= need && reinterpret_cast<uintptr_t>(ptr) % align == 0,
               "%s: workspace of %zu bytes (%zu-byte aligned) needed, got %zu", who, need, align, got);
    return PU_OK;
}

// A workspace layout, written once: a function takes its pieces from a Carver in order.
// On the caller's pointer that yields the pieces; on a null base nothing is dereferenced
// and used() is the size the *_workspace_bytes function reports.  A piece starts at the
// next multiple of align from the base and occupies exactly its bytes.
class Carver {
    char *base_;
    size_t off_ = 0;

public:
    explicit Carver(void *base = nullptr) : base_(static_cast<char *>(base)) {}
    template <class T>
    T *take(size_t bytes, size_t align = 256)
    {
        off_ = (off_ + align - 1) & ~(align - 1);
        T *p = base_ ? reinterpret_cast<T *>(base_ + off_) : nullptr;
        off_ += bytes;
        return p;
    }
    size_t used() const { return off_; }
};

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
