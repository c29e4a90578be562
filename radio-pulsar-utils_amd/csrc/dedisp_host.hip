// The host side of dedispersion: the plan object (pu_plan: planner output, device tables,
// timing events, certification state) and every extern "C" entry point of the plan API.
// No kernel lives here: the launches go through the launchers of the kernel units
// (dedisp_units.h), the planning through plan.cpp (dedisp_plan.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <mutex>
#include <type_traits>
#include <vector>

#include "exact.h"
#include "pu_common.h"

#include "dedisp_units.h"

// The planner (plan.cpp, plain C++): its functions are found through these types.
using pu::CertState;
using pu::PlanProblem;
using pu::PlanTables;

int pu::DeviceTables::upload(PlanTables &t)
{
    pad_slots(t);
    int rc = PU_OK;
    auto put = [&rc](auto &dst, auto &vec) {
        if (rc || vec.empty()) return;
        const size_t bytes = vec.size() * sizeof vec[0];
        rc = pu::hip_check(hipMalloc((void **)&dst.ptr, std::max<size_t>(bytes, 16)), "hipMalloc(plan)");
        if (rc) return;
        rc = pu::hip_check(hipMemcpy(dst.ptr, vec.data(), bytes, hipMemcpyHostToDevice), "hipMemcpy(plan)");
        std::remove_reference_t<decltype(vec)>().swap(vec);
    };
    put(first, t.first);
    put(count, t.count);
    put(rowlen, t.rowlen);
    put(tiles, t.tiles);
    put(tile_stages, t.tile_stages);
    put(stages, t.stages);
    put(slots, t.slots);
    put(recs, t.recs);
    put(base, t.base);
    put(rec, t.rec);
    put(rec8, t.rec8);
    return rc;
}

namespace {

// The kernel for the plan: subband (dedisperse.hip), or in channel order with float64 rows
// (dedisp_f64.hip, its own code-generation options) or float32 rows (dedisp_chan.hip);
// between the plan's timing events when timing is enabled.
int dispatch(pu_plan *p, const DedispArgs &a, bool plane, hipStream_t s)
{
    const size_t nslot = p->ev_start.size();
    const size_t slot = nslot ? (size_t)(p->launches % (int64_t)nslot) : 0;
    if (nslot) PU_TRY_HIP(hipEventRecord(p->ev_start[slot], s));
    int rc;
    if (p->t.group > 1) {
        rc = pu_dd_launch_sub(p, &a, sizeof a, plane, s);
    } else if (kVariants[p->pb.variant].fsm) {
        // records, then the first-window table (planner: one upload)
        const uint32_t *first_off = p->d.rec8 + (size_t)p->t.ndt * p->pb.nchan * kTPT / 2;
        rc = pu_dd_launch_f64(p->pb.variant == V_F32_F64, plane, &a, sizeof a, p->t.lds_bytes, p->d.first, p->d.count,
                              p->d.rowlen, p->d.base, p->d.rec8, first_off, s, kF64Waves);
    } else {
        rc = pu_dd_launch_chan(p, &a, sizeof a, plane, s);
    }
    if (rc) return rc;
    if (nslot) PU_TRY_HIP(hipEventRecord(p->ev_stop[slot], s));
    ++p->launches;
    return PU_OK;
}

void destroy_events(pu_plan *p)
{
    for (auto *v : {&p->ev_start, &p->ev_stop}) {
        for (auto e : *v) (void)hipEventDestroy(e);
        v->clear();
    }
}

void free_plan(pu_plan *p)
{
    if (!p) return;
    destroy_events(p);
    (void)hipFree(p->d_stamps);
    if (p->h_cert) (void)hipHostFree(p->h_cert);
    delete p;  // the device tables: ~DeviceTables
}

// The plan keeps its shift table (host) for the exact recomputation of flagged trials,
// and a pinned copy of the certification state.
int finish_plan(pu_plan *p, const int64_t *shifts)
{
    p->shifts.assign(shifts, shifts + p->pb.ndm * p->pb.nchan);
    return pu::hip_check(hipHostMalloc((void **)&p->h_cert, sizeof(CertState), hipHostMallocDefault),
                         "hipHostMalloc(cert)");
}

}  // namespace

extern "C" {

int pu_plan_create_ex(pu_plan **out, int dtype, int acc, int64_t nchan, int64_t n, const int64_t *shifts,
                      int64_t ndm, const pu_plan_opts *opts)
{
    PU_REQUIRE(out != nullptr, "pu_plan_create: out is NULL");
    *out = nullptr;
    PlanProblem pb;
    int rc = check_plan_args(dtype, acc, nchan, n, shifts, ndm, opts, pb);
    if (rc) return rc;
    pu_plan *p = new pu_plan();
    p->pb = pb;
    rc = choose_plan(p->pb, shifts, *opts, p->t);
    if (!rc) rc = p->d.upload(p->t);
    if (!rc) rc = finish_plan(p, shifts);
    if (rc) {
        free_plan(p);
        return rc;
    }
    *out = p;
    return PU_OK;
}

int pu_plan_create_grouped(pu_plan **out, int dtype, int acc, int64_t nchan, int64_t n, const int64_t *shifts,
                           int64_t ndm, int group)
{
    pu_plan_opts o{};
    o.group = group;
    o.shape = -1;
    o.u8_dma = -1;
    o.dt_major = -1;
    return pu_plan_create_ex(out, dtype, acc, nchan, n, shifts, ndm, &o);
}

int pu_plan_create(pu_plan **out, int dtype, int acc, int64_t nchan, int64_t n, const int64_t *shifts, int64_t ndm)
{
    return pu_plan_create_grouped(out, dtype, acc, nchan, n, shifts, ndm, 0);
}

void pu_plan_destroy(pu_plan *p) { free_plan(p); }

int pu_plan_enable_timing(pu_plan *p, int nslots)
{
    PU_REQUIRE(p != nullptr && nslots >= 0 && nslots <= 65536, "pu_plan_enable_timing: bad arguments");
    std::lock_guard<std::mutex> guard(p->lock);
    destroy_events(p);
    for (auto *v : {&p->ev_start, &p->ev_stop}) {
        v->assign((size_t)nslots, nullptr);
        for (int i = 0; i < nslots; ++i) PU_TRY_HIP(hipEventCreate(&(*v)[i]));
    }
    p->launches = 0;
    return PU_OK;
}

int pu_plan_stamps(pu_plan *p, int64_t *out, int n)
{
    PU_REQUIRE(p != nullptr && out != nullptr, "pu_plan_stamps: bad arguments");
    std::lock_guard<std::mutex> guard(p->lock);
#ifdef PU_STAMPS
    constexpr int kStamps = 16;  // 2 roles (other waves, DMA-issuing waves) x 8 phases
    if (!p->d_stamps) {
        PU_TRY_HIP(hipMalloc((void **)&p->d_stamps, kStamps * sizeof(uint64_t)));
        PU_TRY_HIP(hipMemset(p->d_stamps, 0, kStamps * sizeof(uint64_t)));
        return 0;  // armed: the next launches accumulate
    }
    uint64_t h[kStamps];
    PU_TRY_HIP(hipDeviceSynchronize());
    PU_TRY_HIP(hipMemcpy(h, p->d_stamps, sizeof h, hipMemcpyDeviceToHost));
    PU_TRY_HIP(hipMemset(p->d_stamps, 0, kStamps * sizeof(uint64_t)));
    const int m = std::min(n, kStamps);
    for (int i = 0; i < m; ++i) out[i] = (int64_t)h[i];
    return m;
#else
    (void)n;
    return 0;
#endif
}

int pu_plan_kernel_times(pu_plan *p, float *ms, int n)
{
    PU_REQUIRE(p != nullptr && ms != nullptr, "pu_plan_kernel_times: bad arguments");
    std::lock_guard<std::mutex> guard(p->lock);
    const int64_t have = std::min<int64_t>(p->launches, (int64_t)p->ev_start.size());
    const int m = (int)std::min<int64_t>(n, have);
    for (int i = 0; i < m; ++i) {
        PU_TRY_HIP(hipEventSynchronize(p->ev_stop[i]));
        PU_TRY_HIP(hipEventElapsedTime(&ms[i], p->ev_start[i], p->ev_stop[i]));
    }
    return m;
}

size_t pu_plan_workspace_bytes(const pu_plan *p)
{
    if (!p) return 0;
    // per-(trial, time tile) partial records | CertState | flagged-trial list
    return pu::part_bytes(p) + sizeof(CertState) + (size_t)p->pb.ndm * sizeof(int32_t);
}

int pu_plan_info(const pu_plan *p, int64_t *info, int n)
{
    if (!p || !info) return 0;
    std::lock_guard<std::mutex> guard(p->lock);
    const int64_t cert[6] = {p->cert_rechecked, p->cert_nan, p->cert_why[0], p->cert_why[1], p->cert_why[2], p->cert_us};
    return fill_info(p->pb, p->t, cert, info, n);
}

static int check_data(const pu_plan *p, const void *data, int64_t ld)
{
    PU_REQUIRE(p != nullptr, "plan is NULL");
    PU_REQUIRE(data != nullptr, "data is NULL");
    PU_REQUIRE(ld >= p->pb.n, "ld %lld < nsamples %lld", (long long)ld, (long long)p->pb.n);
    PU_REQUIRE(!p->t.dma8 || (reinterpret_cast<uintptr_t>(data) % 4 == 0 && ld % 4 == 0),
               "8-bit subband plan: rows must start on 4-byte boundaries (data %% 4 == 0, ld %% 4 == 0)");
    return PU_OK;
}

static DedispArgs make_args(const pu_plan *p, const void *data, int64_t ld)
{
    DedispArgs a{};
    a.data = data;
    a.ld = ld;
    a.nchan = (int32_t)p->pb.nchan;
    a.n = (int32_t)p->pb.n;
    a.ndt = p->t.ndt;
    a.ntt = p->t.ntt;
    a.tt0 = 0;
    a.ntt_run = p->t.ntt;
    a.ncc = p->t.ncc;
    a.row_stride = p->t.row_stride;
    a.small_n = p->t.small_n;
    return a;
}

int pu_plan_search_tiles(pu_plan *p, const void *data, int64_t ld, int64_t tt_begin, int64_t tt_end,
                         void *workspace, size_t ws_bytes, void *stream)
{
    int rc = check_data(p, data, ld);
    if (rc) return rc;
    std::lock_guard<std::mutex> guard(p->lock);
    PU_REQUIRE(0 <= tt_begin && tt_begin <= tt_end && tt_end <= p->t.ntt,
               "pu_plan_search_tiles: tile range [%lld, %lld) outside [0, %d)", (long long)tt_begin,
               (long long)tt_end, p->t.ntt);
    if ((rc = pu::check_workspace("pu_plan_search_tiles", workspace, ws_bytes, pu_plan_workspace_bytes(p), 1))) return rc;
    if (tt_begin == tt_end) return PU_OK;
    DedispArgs a = make_args(p, data, ld);
    a.partials = workspace;
    a.tt0 = (int32_t)tt_begin;
    a.ntt_run = (int32_t)(tt_end - tt_begin);
    return dispatch(p, a, false, pu::as_stream(stream));
}

// What pu_plan_finalize, _range and _range_flagged share: their checks (the error texts
// name `who`, the entry point that was called; outputs: its other output pointers are set)
// and pu_finalize_kernel over trials [begin, end).  The caller holds the plan's lock.
static int finalize_range(const char *who, pu_plan *p, int64_t begin, int64_t end, bool outputs, double *max_out,
                          double *std_out, double *snr_out, int32_t *rebin_out, void *workspace, size_t ws_bytes,
                          void *stream)
{
    PU_REQUIRE(0 <= begin && begin <= end && end <= p->pb.ndm, "%s: trial range [%lld, %lld) outside [0, %lld)", who,
               (long long)begin, (long long)end, (long long)p->pb.ndm);
    PU_REQUIRE(outputs && max_out && std_out && snr_out && rebin_out, "%s: NULL output", who);
    if (int rc = pu::check_workspace(who, workspace, ws_bytes, pu_plan_workspace_bytes(p), 8)) return rc;
    char *ws = reinterpret_cast<char *>(workspace);
    return pu_dd_launch_finalize(p, ws, max_out, std_out, snr_out, rebin_out, ws, stream, false, begin, end - begin);
}

// finalize_range, then its flagged trials settled from the data
static int finalize_resolved(const char *who, pu_plan *p, const void *data, int64_t ld, int64_t begin, int64_t end,
                             double *max_out, double *std_out, double *snr_out, int32_t *rebin_out, void *workspace,
                             size_t ws_bytes, void *stream)
{
    int rc = check_data(p, data, ld);
    if (rc) return rc;
    std::lock_guard<std::mutex> guard(p->lock);
    rc = finalize_range(who, p, begin, end, true, max_out, std_out, snr_out, rebin_out, workspace, ws_bytes, stream);
    if (rc) return rc;
    return pu_dd_resolve_flagged(p, data, ld, max_out, std_out, snr_out, rebin_out, reinterpret_cast<char *>(workspace),
                                 stream, begin, end - begin);
}

int pu_plan_finalize(pu_plan *p, const void *data, int64_t ld, double *max_out, double *std_out, double *snr_out,
                     int32_t *rebin_out, void *workspace, size_t ws_bytes, void *stream)
{
    return finalize_resolved("pu_plan_finalize", p, data, ld, 0, p ? p->pb.ndm : 0, max_out, std_out, snr_out,
                             rebin_out, workspace, ws_bytes, stream);
}

int pu_plan_finalize_range(pu_plan *p, const void *data, int64_t ld, int64_t trial_begin, int64_t trial_end,
                           double *max_out, double *std_out, double *snr_out, int32_t *rebin_out, void *workspace,
                           size_t ws_bytes, void *stream)
{
    return finalize_resolved("pu_plan_finalize_range", p, data, ld, trial_begin, trial_end, max_out, std_out, snr_out,
                             rebin_out, workspace, ws_bytes, stream);
}

int pu_plan_finalize_range_flagged(pu_plan *p, int64_t trial_begin, int64_t trial_end, double *max_out,
                                   double *std_out, double *snr_out, int32_t *rebin_out, void *workspace,
                                   size_t ws_bytes, int32_t *flagged, int64_t cap, int64_t *counts, void *stream)
{
    PU_REQUIRE(p != nullptr, "plan is NULL");
    std::lock_guard<std::mutex> guard(p->lock);
    int rc = finalize_range("pu_plan_finalize_range_flagged", p, trial_begin, trial_end,
                            counts && (flagged || cap == 0), max_out, std_out, snr_out, rebin_out, workspace, ws_bytes,
                            stream);
    if (rc) return rc;
    hipStream_t s = pu::as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    CertState *cert = reinterpret_cast<CertState *>(ws + pu::part_bytes(p));
    const int32_t *list = reinterpret_cast<const int32_t *>(cert + 1);
    PU_TRY_HIP(hipMemcpyAsync(p->h_cert, cert, sizeof(CertState), hipMemcpyDeviceToHost, s));
    PU_TRY_HIP(hipStreamSynchronize(s));
    const int64_t nflag = p->h_cert->nflag;
    counts[0] = nflag;
    counts[1] = p->h_cert->nnonfinite;
    for (int k = 0; k < 3; ++k) p->cert_why[k] = p->h_cert->why[k];
    p->cert_rechecked = 0;
    p->cert_nan = 0;
    p->cert_us = 0;
    const int64_t m = std::min(nflag, cap);
    if (m > 0) {
        PU_TRY_HIP(hipMemcpyAsync(flagged, list, (size_t)m * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        PU_TRY_HIP(hipStreamSynchronize(s));
        std::sort(flagged, flagged + m);
    }
    return PU_OK;
}

int pu_plan_exact_series(pu_plan *p, const void *data, int64_t ld, const int32_t *trials, int64_t m, int64_t t_begin,
                         int64_t t_end, double *out, void *stream)
{
    int rc = check_data(p, data, ld);
    if (rc) return rc;
    std::lock_guard<std::mutex> guard(p->lock);
    PU_REQUIRE(0 <= t_begin && t_begin <= t_end && t_end <= p->pb.n, "pu_plan_exact_series: samples [%lld, %lld) outside [0, %lld)",
               (long long)t_begin, (long long)t_end, (long long)p->pb.n);
    PU_REQUIRE(m >= 0, "pu_plan_exact_series: m < 0");
    if (m == 0 || t_end == t_begin) return PU_OK;
    PU_REQUIRE(trials && out, "pu_plan_exact_series: NULL trials / out");
    const int64_t n = p->pb.n, nchan = p->pb.nchan;
    std::vector<int64_t> sh((size_t)(m * nchan));
    for (int64_t k = 0; k < m; ++k) {
        PU_REQUIRE(0 <= trials[k] && trials[k] < p->pb.ndm, "pu_plan_exact_series: trial %d outside [0, %lld)",
                   trials[k], (long long)p->pb.ndm);
        std::copy_n(p->shifts.data() + (size_t)trials[k] * nchan, nchan, sh.data() + k * nchan);
    }
    for (auto &v : sh) v = ((v % n) + n) % n;
    hipStream_t s = pu::as_stream(stream);
    void *d_sh = nullptr;
    PU_TRY_HIP(hipMallocAsync(&d_sh, sh.size() * sizeof(int64_t), s));
    rc = pu::hip_check(hipMemcpyAsync(d_sh, sh.data(), sh.size() * sizeof(int64_t), hipMemcpyHostToDevice, s),
                       "hipMemcpyAsync(exact series shifts)");
    if (!rc)
        rc = pu::exact_series(data, p->pb.dtype, nchan, n, ld, reinterpret_cast<const int64_t *>(d_sh), m, out, s, t_begin,
                              t_end - t_begin);
    (void)hipFreeAsync(d_sh, s);
    const int rs = pu::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(exact series)");
    return rc ? rc : rs;
}

int pu_nonfinite_any(const void *data, int dtype, int64_t nrows, int64_t ncols, int64_t ld, int32_t *flag, void *stream)
{
    PU_REQUIRE(flag, "pu_nonfinite_any: NULL pointer");
    PU_REQUIRE(nrows >= 0 && ncols >= 0 && ld >= ncols, "pu_nonfinite_any: bad shape");
    hipStream_t s = pu::as_stream(stream);
    if (nrows == 0 || ncols == 0) {  // nothing to read: data may be NULL (an empty torch view's pointer is)
        PU_TRY_HIP(hipMemsetAsync(flag, 0, sizeof(int32_t), s));
        return PU_OK;
    }
    PU_REQUIRE(data, "pu_nonfinite_any: NULL pointer");
    return pu::nonfinite_any_async(data, dtype, nrows, ncols, ld, flag, s);
}

int pu_plan_search(pu_plan *p, const void *data, int64_t ld, double *max_out, double *std_out,
                   double *snr_out, int32_t *rebin_out, void *workspace, size_t ws_bytes, void *stream)
{
    int rc = check_data(p, data, ld);
    if (rc) return rc;
    std::lock_guard<std::mutex> guard(p->lock);
    PU_REQUIRE(max_out && std_out && snr_out && rebin_out, "pu_plan_search: NULL output");
    if ((rc = pu::check_workspace("pu_plan_search", workspace, ws_bytes, pu_plan_workspace_bytes(p), 8))) return rc;
    DedispArgs a = make_args(p, data, ld);
    a.partials = workspace;
    hipStream_t s = pu::as_stream(stream);
    char *ws = reinterpret_cast<char *>(workspace);
    // the certification state is cleared BEFORE the search kernel: the fill then runs while
    // the stream is idle after the previous call's host read, instead of between the search
    // and finalize kernels (C5: ~10 us of fill + dispatch gap on the step)
    PU_TRY_HIP(hipMemsetAsync(ws + pu::part_bytes(p), 0, sizeof(CertState), s));
    rc = dispatch(p, a, false, s);
    if (rc) return rc;
    rc = pu_dd_launch_finalize(p, a.partials, max_out, std_out, snr_out, rebin_out, ws, s, true, 0, p->pb.ndm);
    if (rc) return rc;
    return pu_dd_resolve_flagged(p, data, ld, max_out, std_out, snr_out, rebin_out, ws, s, 0, p->pb.ndm);
}

int pu_plan_dedisperse(pu_plan *p, const void *data, int64_t ld, void *plane, int64_t ld_plane, void *stream)
{
    int rc = check_data(p, data, ld);
    if (rc) return rc;
    std::lock_guard<std::mutex> guard(p->lock);
    PU_REQUIRE(plane != nullptr, "pu_plan_dedisperse: plane is NULL");
    PU_REQUIRE(ld_plane >= p->pb.n, "pu_plan_dedisperse: ld_plane < nsamples");
    DedispArgs a = make_args(p, data, ld);
    a.plane = plane;
    a.ld_plane = ld_plane;
    return dispatch(p, a, true, pu::as_stream(stream));
}

int pu_plan_dm_tiles(const pu_plan *p, int32_t *first, int32_t *count, int n)
{
    if (!p) return 0;
    std::lock_guard<std::mutex> guard(p->lock);
    const int ndt = (int)p->t.tile_first.size();
    for (int t = 0; t < std::min(n, ndt); ++t) {
        if (first) first[t] = p->t.tile_first[t];
        if (count) count[t] = p->t.tile_count[t];
    }
    return ndt;
}

int pu_plan_dedisperse_dm_tile(pu_plan *p, const void *data, int64_t ld, int64_t dt, void *plane, int64_t ld_plane,
                               void *stream)
{
    int rc = check_data(p, data, ld);
    if (rc) return rc;
    std::lock_guard<std::mutex> guard(p->lock);
    PU_REQUIRE(plane != nullptr, "pu_plan_dedisperse_dm_tile: plane is NULL");
    PU_REQUIRE(ld_plane >= p->pb.n, "pu_plan_dedisperse_dm_tile: ld_plane < nsamples");
    PU_REQUIRE(0 <= dt && dt < (int64_t)p->t.tile_first.size(), "pu_plan_dedisperse_dm_tile: DM tile %lld outside [0, %d)",
               (long long)dt, (int)p->t.tile_first.size());
    DedispArgs a = make_args(p, data, ld);
    a.dt0 = (int32_t)dt;
    a.ndt = 1;
    // the kernels write trial row (first + i) at plane + (first + i) ld_plane: shift the base
    // so that the tile's rows land at rows 0 .. count - 1 of the caller's plane
    const size_t elem = kVariants[p->pb.variant].acc_f64 ? sizeof(double) : sizeof(float);
    a.plane = reinterpret_cast<void *>(reinterpret_cast<uintptr_t>(plane) -
                                       (uintptr_t)((size_t)p->t.tile_first[(size_t)dt] * (size_t)ld_plane * elem));
    a.ld_plane = ld_plane;
    return dispatch(p, a, true, pu::as_stream(stream));
}

}  // extern "C"
