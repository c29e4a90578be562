// What crosses the dedispersion translation units: the plan object with its device
// tables and certification state (dedisp_host.hip owns them and the C ABI), and the
// launchers of the kernel units - dedisperse.hip (subband), dedisp_chan.hip (channel
// order, float32 rows), dedisp_f64.hip (channel order, float64 rows) and
// dedisp_finalize.hip.  Included by both sides of every such call.
//
// Structs shared as types live in namespace pu (as PlanTables does).  DedispArgs is a
// kernel argument and stays each unit's own type (dedisp_common.h): the launchers take it
// as bytes and check its size, dedisp_f64.hip's plain-types convention.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <mutex>
#include <utility>
#include <vector>

#include "dedisp_common.h"
#include "dedisp_plan.h"

namespace pu {

// Certification state at the workspace tail (pu_plan_workspace_bytes), then the list
// of the trials to recompute (int32 each).
struct CertState {
    int32_t nflag;       // trials the fast path could not certify (listed after the state)
    int32_t nnonfinite;  // of which: a non-finite partial (NaN / inf in the series)
    int32_t scan;        // non-finite input scan (pu::nonfinite_any_async)
    int32_t why[3];      // flagged by: std not above its bound, S/N sign, S/N tie
    int32_t pad[58];
};
static_assert(sizeof(CertState) == 256, "CertState");

// An owning device pointer (move-only): the one place a plan table is freed.
template <typename T>
struct DevicePtr {
    T *ptr = nullptr;
    DevicePtr() = default;
    DevicePtr(DevicePtr &&o) noexcept : ptr(o.ptr) { o.ptr = nullptr; }
    DevicePtr &operator=(DevicePtr &&o) noexcept
    {
        std::swap(ptr, o.ptr);
        return *this;
    }
    ~DevicePtr() { (void)hipFree(ptr); }
    operator T *() const { return ptr; }
};

// the planner fills these records as plain structs; DeviceTables::upload copies their bytes
static_assert(sizeof(PlanU32x4) == sizeof(u32x4) && sizeof(PlanI32x4) == sizeof(i32x4) &&
                  sizeof(PlanI32x2) == sizeof(i32x2),
              "plan table records");

// The plan's tables in device memory.
struct DeviceTables {
    DevicePtr<int32_t> first, count, rowlen, base, slots;
    DevicePtr<u32x4> rec;
    DevicePtr<uint32_t> rec8, recs;
    DevicePtr<i32x4> tiles, stages;
    DevicePtr<i32x2> tile_stages;

    // Uploads every table the plan's mode fills, the padded slot records included, and
    // releases each host copy.
    int upload(PlanTables &t);
};

}  // namespace pu

// A plan: the problem, what the planner made of it, the device tables and the per-call
// state (timing events and the launch counter, the pinned certification copy and the last
// call's certification outcome).  Cached plans are shared across threads (ctypes releases
// the GIL): every entry point that launches or reads the per-call state holds the lock
// for the whole call.
struct pu_plan {
    mutable std::mutex lock;
    pu::PlanProblem pb;
    pu::PlanTables t;
    pu::DeviceTables d;
    // optional kernel timing: events before the first and after the last launch of
    // each dispatch
    std::vector<hipEvent_t> ev_start, ev_stop;
    int64_t launches = 0;
    uint64_t *d_stamps = nullptr;  // diagnostic build (PU_STAMPS): phase-cycle totals
    // certification: the shift table (host) for exact recomputation of
    // flagged trials, a pinned copy of the device CertState, the last call's outcome
    std::vector<int64_t> shifts;
    pu::CertState *h_cert = nullptr;
    int64_t cert_rechecked = 0, cert_nan = 0, cert_why[3] = {0, 0, 0}, cert_us = 0;
};

namespace pu {

// the plan's partial records (part_elem: dedisp_plan.h), in whole 256-byte pieces; the
// certification state follows them in the workspace
static inline size_t part_bytes(const pu_plan *p)
{
    return up256((size_t)p->pb.ndm * p->t.ntt * kPartStride * part_elem(p->pb));
}

}  // namespace pu

// ---- the launchers.  args / args_bytes: the caller's DedispArgs.

// dedisp_f64.hip (waves: dedisp_plan.h's kF64Waves, checked against the kernel's)
int pu_dd_launch_f64(bool tin_f32, bool plane, const void *args, size_t args_bytes, size_t lds_bytes,
                     const int32_t *first, const int32_t *count, const int32_t *rowlen, const int32_t *base,
                     const void *rec8, const void *first_off, void *stream, int waves);
// dedisp_chan.hip: dedisp_kernel for the plan's variant (the three with float32 rows)
int pu_dd_launch_chan(const pu_plan *p, const void *args, size_t args_bytes, bool plane, void *stream);
// dedisperse.hip: dedisp_sub_kernel for the plan's input type, shape, group and slot kind
int pu_dd_launch_sub(const pu_plan *p, const void *args, size_t args_bytes, bool plane, void *stream);

// ---- dedisp_finalize.hip

// pu_finalize_kernel over trials [first, first + count), outputs indexed by plan trial.
// cleared: the caller already zeroed the certification state earlier in the stream.
int pu_dd_launch_finalize(pu_plan *p, const void *part, double *mx, double *sd, double *snr, int32_t *win, char *ws,
                          void *stream, bool cleared, int64_t first, int64_t count);
// After the finalize kernel: wait for it, then settle the flagged trials of that range.
int pu_dd_resolve_flagged(pu_plan *p, const void *data, int64_t ld, double *mx, double *sd, double *snr,
                          int32_t *win, char *ws, void *stream, int64_t first, int64_t count);
