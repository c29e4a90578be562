// The finalize step of a search: pu_finalize_kernel combines the per-tile
// partial statistics the dedispersion kernels wrote into each trial's max / std / S/N and
// best rebin width, and flags the trials whose decisions the fast path's rounding could
// change; resolve_flagged recomputes those exactly (exact.hip).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <type_traits>
#include <vector>

#include "exact.h"
#include "pu_common.h"

#include "dedisp_units.h"

using pu::CertState;

namespace {

// Rounding model of one plan's fast statistics.
struct CertModel {
    int32_t tie_check;  // the series is exact (u8 with exact f32 sums, any f64 accumulation)
    double e_rel;       // per-sample series error bound / (|mean| + 4 std + |max|)
    double gamma;       // relative rounding of the epilogue's sums of (shifted) squares
};

// One workgroup per trial: combine the per-time-tile partials in a fixed order
// (thread-strided then an LDS tree: deterministic), then the reference's S/N logic
// (dedispersion.py:186-201): snr_w = max(reb_w)/std(reb_w), first strict best.
// Certification: a trial whose statistics or S/N decisions the fast path's summation
// order could change is appended to the list in ``cert`` (the host recomputes it
// exactly).  Bounds: the epilogue's sums of squares carry relative error gamma of
// Q = their magnitude (tile-local second moments + recentring terms), so
// |d var| <= 4 gamma Q; a per-sample series error E moves a width-w std by <= w E and
// max - w mean by <= 2 w E.  A trial is flagged when a partial is non-finite, when
// std is not > 4 x its bound (zero or rounding-level std: constant inputs), when
// max - w mean is within its bound of 0 (the S/N sign decision), and - for plans whose
// series is exact - when two S/N values of the strict first-best chain are within the
// sum of their bounds (ties).
template <typename PT>
__global__ void __launch_bounds__(256)
pu_finalize_kernel(const PT *__restrict__ part, int ntt, int n, int tt_len,
                   double *max_out, double *std_out, double *snr_out, int32_t *win_out,
                   CertModel cm, CertState *cert, int32_t *list, int first)
{
    __shared__ double red[4][4][256];
    const int trial = first + (int)blockIdx.x;  // trials [first, first + gridDim.x) of the plan
    const int tid = threadIdx.x;
    const PT *p = part + (size_t)trial * ntt * kPartStride;
    const double mu = p[0];
    double S1[4] = {0, 0, 0, 0}, S2[4] = {0, 0, 0, 0}, MX[4] = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};
    double A2[4] = {0, 0, 0, 0};
    for (int i = tid; i < ntt; i += 256) {
        const PT *q = p + (size_t)i * kPartStride;
        const double dk = q[0] - mu;
        for (int w = 0; w < 4; ++w) {
            const int width = 1 << w;
            const long lo = (long)i * tt_len / width;
            const long hi = min((long)(i + 1) * tt_len / width, (long)(n / width));
            const double cntb = (double)max(0L, hi - lo);
            if (cntb <= 0) continue;
            const double s1 = q[2 + 3 * w], s2 = q[3 + 3 * w];
            const double wd = width * dk;
            S1[w] += s1 + cntb * wd;
            S2[w] += s2 + 2.0 * wd * s1 + cntb * wd * wd;
            // magnitude the rounding bound scales with: the tile's sum of squares (relative
            // error gamma), its recentring term through s1 (|d s1| <= gamma sum|y| <=
            // gamma sqrt(cnt s2)), and 2^-30 of the float64 recentring square
            A2[w] += fabs(s2) + 2.0 * fabs(wd) * sqrt(cntb * fabs(s2)) + 0x1p-30 * cntb * wd * wd;
            // NaN-propagating (a NaN partial max makes the trial non-finite below)
            MX[w] = (q[1 + 3 * w] > MX[w] || q[1 + 3 * w] != q[1 + 3 * w]) ? q[1 + 3 * w] : MX[w];
        }
    }
    for (int w = 0; w < 4; ++w) {
        red[0][w][tid] = S1[w];
        red[1][w][tid] = S2[w];
        red[2][w][tid] = MX[w];
        red[3][w][tid] = A2[w];
    }
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (tid < s) {
            for (int w = 0; w < 4; ++w) {
                red[0][w][tid] += red[0][w][tid + s];
                red[1][w][tid] += red[1][w][tid + s];
                const double a = red[2][w][tid], b = red[2][w][tid + s];
                red[2][w][tid] = (b > a || b != b) ? b : a;
                red[3][w][tid] += red[3][w][tid + s];
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        const double mean = mu + red[0][0][0] / n;  // mean of the dedispersed series
        double best = 0.0;
        int bestw = 0;
        double sdw[4] = {0, 0, 0, 0}, Qw[4] = {0, 0, 0, 0};
        bool nonfinite = !isfinite(mu) || !isfinite(mean);
        for (int w = 0; w < 4; ++w) {
            const int width = 1 << w;
            const long nb = n / width;
            if (nb <= 0) continue;
            const double m1 = red[0][w][0] / nb;
            const double var = red[1][w][0] / nb - m1 * m1;
            const double sd = sqrt(var > 0 ? var : 0.0);
            sdw[w] = sd;
            Qw[w] = red[3][w][0] / nb;
            nonfinite = nonfinite || !isfinite(red[0][w][0]) || !isfinite(red[1][w][0]) ||
                        !isfinite(red[2][w][0]) || !isfinite(red[3][w][0]);
            const double snr = (red[2][w][0] - width * mean) / sd;
            if (snr > best) {
                best = snr;
                bestw = width;
            }
        }
        bool uncertain = false;
        int why = -1;
        if (!nonfinite) {
            const double E = cm.e_rel * (fabs(mean) + 4.0 * sdw[0] + fabs(red[2][0][0]));
            double b = 0.0, eb = 0.0;  // the reference's (best_snr, its bound) chain
            for (int w = 0; w < 4 && !uncertain; ++w) {
                const int width = 1 << w;
                if (n / width <= 0) continue;
                const double sd = sdw[w], MXw = red[2][w][0];
                const double e_var = 4.0 * cm.gamma * Qw[w];
                const double e_sd = sd > 0 ? e_var / sd + width * E : INFINITY;
                const double num = MXw - width * mean;
                // max - w mean: the series error, the mean's rounding (through S1), the
                // float64 combination, and - unless the rebinned sums are exact (exact-series
                // plans: integers < 2^24 or float64) - their float32 rounding
                const double e_num = 2.0 * width * E + cm.gamma * width * sqrt(Qw[0]) +
                                     (cm.tie_check ? 0.0 : cm.gamma * fabs(MXw)) +
                                     0x1p-50 * (fabs(MXw) + width * fabs(mean));
                if (!(e_sd <= 0.25 * sd) || !(fabs(num) > e_num)) {
                    uncertain = true;
                    why = !(e_sd <= 0.25 * sd) ? 0 : 1;
                    break;
                }
                const double snr = num / sd;
                const double e_snr = (e_num + fabs(snr) * e_sd) / (sd - e_sd) + 0x1p-44 * fabs(snr);
                if (cm.tie_check) {
                    const double d = snr - b;
                    if (!(fabs(d) > e_snr + eb)) {
                        uncertain = true;
                        why = 2;
                    } else if (d > 0) {
                        b = snr;
                        eb = e_snr;
                    }
                }
            }
        }
        if (nonfinite || uncertain) {
            list[atomicAdd(&cert->nflag, 1)] = trial;
            if (nonfinite) atomicAdd(&cert->nnonfinite, 1);
            if (why >= 0) atomicAdd(&cert->why[why], 1);
        }
        max_out[trial] = red[2][0][0] - mean;
        std_out[trial] = sdw[0];
        snr_out[trial] = best;
        win_out[trial] = bestw;
    }
}

// Rounding model of the plan's fast statistics (pu_finalize_kernel).
CertModel cert_model(const pu_plan *p)
{
    CertModel m{};
    if (kVariants[p->pb.variant].acc_f64) {
        m.tie_check = 1;  // float64 channel order: the reference's series bit for bit
        m.e_rel = 0x1p-50;
        m.gamma = 0x1p-44;
    } else if (p->pb.dtype == PU_U8 && 8 * 255 * p->pb.nchan < (int64_t(1) << 24)) {
        // integer sums (and their 8-sample rebins) below 2^24: exact in float32.  The
        // epilogue's sums of squares: <= 14 float32 roundings of nonnegative terms (the
        // shifted value, the square-and-add, 4 lane-local adds, the pair add, 2 permlane
        // and 4 row-reduction adds, the float record) = 14 x 2^-24 < 2^-20
        m.tie_check = 1;
        m.e_rel = 0.0;
        m.gamma = 0x1p-20;
    } else {
        // float32 sums of float data: the typical (random-walk) rounding of nchan terms
        // with an 8x margin, relative to the series' magnitude; S/N ties within the
        // float32 tolerance are not recomputed (the stated tolerance covers them)
        m.tie_check = 0;
        m.e_rel = 8.0 * 0x1p-24 * std::sqrt((double)p->pb.nchan);
        m.gamma = 0x1p-19;
    }
    return m;
}

}  // namespace

int pu_dd_launch_finalize(pu_plan *p, const void *part, double *mx, double *sd, double *snr, int32_t *win, char *ws,
                          void *stream, bool cleared, int64_t first, int64_t count)
{
    hipStream_t s = pu::as_stream(stream);
    CertState *cert = reinterpret_cast<CertState *>(ws + pu::part_bytes(p));
    int32_t *list = reinterpret_cast<int32_t *>(cert + 1);
    if (!cleared) PU_TRY_HIP(hipMemsetAsync(cert, 0, sizeof(CertState), s));
    if (count == 0) return PU_OK;
    auto go = [&](auto *rec) {
        using PT = std::remove_const_t<std::remove_pointer_t<decltype(rec)>>;
        hipLaunchKernelGGL(pu_finalize_kernel<PT>, dim3((unsigned)count), dim3(256), 0, s, rec, p->t.ntt, (int)p->pb.n,
                           p->t.TT, mx, sd, snr, win, cert_model(p), cert, list, (int)first);
    };
    if (part_elem(p->pb) == sizeof(float))
        go(reinterpret_cast<const float *>(part));
    else
        go(reinterpret_cast<const double *>(part));
    return pu::launch_check("pu_finalize_kernel");
}

// After the finalize kernel: wait for it, then settle the flagged trials.  An input
// holding NaN / inf (found by a scan, run only when some trial saw a non-finite value)
// gives every trial the reference's NaN result; other flagged trials are recomputed
// exactly - their float64 channel-order series (the reference's bit for bit, by a direct
// gather: ~1 ms per trial at C3, far below a channel-mode sub-plan's cost for the
// few trials a search flags) + pu_series_stats - in batches that fit ~1 GiB of
// stream-ordered scratch allocated for the call.
int pu_dd_resolve_flagged(pu_plan *p, const void *data, int64_t ld, double *mx, double *sd, double *snr,
                          int32_t *win, char *ws, void *stream, int64_t first, int64_t count)
{
    hipStream_t s = pu::as_stream(stream);
    CertState *cert = reinterpret_cast<CertState *>(ws + pu::part_bytes(p));
    const int32_t *list = reinterpret_cast<const int32_t *>(cert + 1);
    p->cert_rechecked = 0;
    p->cert_nan = 0;
    PU_TRY_HIP(hipMemcpyAsync(p->h_cert, cert, sizeof(CertState), hipMemcpyDeviceToHost, s));
    PU_TRY_HIP(hipStreamSynchronize(s));
    const int64_t nflag = p->h_cert->nflag;
    for (int k = 0; k < 3; ++k) p->cert_why[k] = p->h_cert->why[k];
    p->cert_us = 0;
    if (nflag == 0) return PU_OK;
    const auto t_start = std::chrono::steady_clock::now();
    struct Timer {  // host time spent settling the flagged trials (pu_plan_info cert_us)
        pu_plan *p;
        std::chrono::steady_clock::time_point t0;
        ~Timer()
        {
            p->cert_us = std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0)
                             .count();
        }
    } timer{p, t_start};
    if (p->h_cert->nnonfinite > 0 && p->pb.dtype != PU_U8) {
        int rc = pu::nonfinite_any_async(data, p->pb.dtype, p->pb.nchan, p->pb.n, ld, &cert->scan, s);
        if (rc) return rc;
        PU_TRY_HIP(hipMemcpyAsync(p->h_cert, cert, sizeof(CertState), hipMemcpyDeviceToHost, s));
        PU_TRY_HIP(hipStreamSynchronize(s));
        if (p->h_cert->scan) {
            // every trial's series holds every input sample once (circular shift-and-sum),
            // so a NaN / inf anywhere reaches every trial: np.mean -> NaN or inf, the
            // shifted series -> NaN, max = std = NaN, no S/N beats 0 (dedispersion.py:186-201)
            p->cert_nan = 1;
            int rc2 = pu::nan_rule(count, mx + first, sd + first, snr + first, win + first, s);
            if (rc2) return rc2;
            PU_TRY_HIP(hipStreamSynchronize(s));
            return PU_OK;
        }
    }
    std::vector<int32_t> idx((size_t)nflag);
    PU_TRY_HIP(hipMemcpyAsync(idx.data(), list, (size_t)nflag * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    PU_TRY_HIP(hipStreamSynchronize(s));
    std::sort(idx.begin(), idx.end());
    const int64_t n = p->pb.n, nchan = p->pb.nchan;
    const int64_t per_row = n * 8 + (int64_t)pu_series_stats_workspace_bytes(1, n) + nchan * 8;
    const int64_t B = std::max<int64_t>(1, std::min<int64_t>(nflag, (int64_t(1) << 30) / per_row));
    // the scratch of a batch: its series, pu_series_stats' workspace, its shifts and trial numbers
    const size_t sws_b = pu_series_stats_workspace_bytes(B, n);
    double *plane = nullptr;
    void *sws = nullptr;
    int64_t *d_sh = nullptr;
    int32_t *d_idx = nullptr;
    auto carve = [&](pu::Carver c) {
        plane = c.take<double>((size_t)B * n * sizeof(double));
        sws = c.take<char>(sws_b);
        d_sh = c.take<int64_t>((size_t)B * nchan * sizeof(int64_t));
        d_idx = c.take<int32_t>((size_t)B * sizeof(int32_t));
        return c.used();
    };
    const size_t need = carve(pu::Carver());
    // per-call scratch, stream-ordered (no device-wide synchronisation, nothing held
    // with the plan between calls); freed on every return path
    void *rc_buf = nullptr;
    PU_TRY_HIP(hipMallocAsync(&rc_buf, need, s));
    struct Scratch {
        void *b;
        hipStream_t s;
        ~Scratch()
        {
            (void)hipFreeAsync(b, s);
            (void)hipStreamSynchronize(s);
        }
    } scratch{rc_buf, s};
    carve(pu::Carver(rc_buf));
    std::vector<int64_t> sh;
    int rc = PU_OK;
    for (int64_t i0 = 0; !rc && i0 < nflag; i0 += B) {
        const int64_t m = std::min(B, nflag - i0);
        sh.resize((size_t)(m * nchan));
        for (int64_t k = 0; k < m; ++k)
            std::copy_n(p->shifts.data() + (size_t)idx[(size_t)(i0 + k)] * nchan, nchan, sh.data() + k * nchan);
        for (auto &v : sh) v = ((v % n) + n) % n;  // row index (t + shift) mod n
        rc = pu::hip_check(hipMemcpyAsync(d_sh, sh.data(), sh.size() * sizeof(int64_t), hipMemcpyHostToDevice, s),
                           "hipMemcpyAsync(recheck shifts)");
        if (!rc) rc = pu::exact_series(data, p->pb.dtype, nchan, n, ld, d_sh, m, plane, s);
        if (!rc)
            rc = pu::hip_check(hipMemcpyAsync(d_idx, idx.data() + i0, (size_t)m * sizeof(int32_t),
                                              hipMemcpyHostToDevice, s), "hipMemcpyAsync(recheck index)");
        if (!rc) rc = pu_series_stats(plane, m, n, n, d_idx, mx, sd, snr, win, sws, sws_b, s);
        const int rs = pu::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(recheck)");
        if (!rc) rc = rs;
    }
    if (!rc) p->cert_rechecked = nflag;
    return rc;
}
