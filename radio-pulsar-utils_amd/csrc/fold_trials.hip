// Folding dedispersed series at many trial frequencies and the epoch-folding chi^2, for gfx950.
//
//   pu_fold_trials   no reference counterpart: the pulse-frequency search the reference leaves
//                    to other packages (its PulseInfo takes pulse_freq as given)
//   pu_profile_chi2  Leahy et al. 1983, the chi^2 of a folded profile against a constant
//
// pu_fold_trials.  pu_fold (fold.hip) shares the bins b(t) of ONE period among many channels;
// this is the transpose: one or a few rows, thousands of periods, so nothing but the samples is
// shared.  A workgroup of W waves owns one row, one segment of FT_SEG samples counted from the
// chunk's start, and a tile of 64 W trials: LANE = TRIAL.  The workgroup stages the segment in
// sub-blocks of FT_SUB samples into LDS, converted to float64 once; every lane then walks the
// sub-block in time order.  All lanes read the same LDS address per step (a broadcast), compute
// their own bin by the three-step rule of the header, and keep the running sum of the current
// run of equal bins in a register; when the bin changes the run sum is added to the lane's own
// LDS accumulator, laid out [bin][lane] (lanes l and l + 32 fall on one bank but in different
// halves of the wave: conflict-free for any mix of bins).  No lane ever touches another lane's
// accumulator: no race, no atomic, no cross-lane step.
//
// Order of a (row, trial, bin) sum, fixed by (n, first_sample, phase0[k], dphase[k], nbin) alone:
//   1. the chunk is cut in segments of FT_SEG = 16384 samples from its start;
//   2. inside a segment the samples are cut in maximal runs of consecutive samples of one bin (a
//      run ends at the segment's end; sub-blocks do not cut it); a run is summed left to right,
//      starting from its first sample;
//   3. the segment's partial of a bin is 0.0 + its runs' sums, in time order;
//   4. ft_combine_kernel adds the partials of a bin in segment order, starting from segment 0's,
//      and adds that total to ``sums``.
// W (waves per workgroup) only selects which lane of which workgroup handles a trial, and a
// partial last tile is masked, never reshaped, so trial k's bits depend neither on ntrials, on
// k's place in the list, on rows nor on the device.
//
// LDS: FT_SUB x 8 = 16 KiB of staged samples + W x 64 x nbin x 8 bytes of accumulators within
// 144 KiB (the CU has 160 KiB): W = 4 up to nbin 64 (at nbin <= 32: 80 KiB, two workgroups per
// CU), W = 2 up to 128, W = 1 up to FT_MAX_NBIN = 256; above that PU_EUNSUPPORTED.
//
// counts: ft_counts_kernel walks the same bins once per call (not per row) with uint32 LDS
// counters per lane, then integer atomics to counts (exact, order-free).
//
// A trial with a non-finite phase0 / dphase or |p| >= 2^52 at either end of the chunk (ft_bad:
// the test pu_fold makes on the host) is masked in both kernels; ft_combine_kernel stores NaN
// over its sums.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pu_common.h"

namespace {

constexpr int FT_SEG = 16384;     // samples of a segment (one partial per row, trial and bin)
constexpr int FT_SUB = 2048;      // samples staged in LDS at a time (float64: 16 KiB)
constexpr int FT_BATCH = 8;       // staged samples a lane reads ahead of its accumulator updates
constexpr int FT_MAX_NBIN = 256;  // 64 lanes x 256 bins x 8 bytes = 128 KiB: one wave's accumulators
constexpr size_t FT_ACC_BUDGET = 144 * 1024;
static_assert(FT_SEG % FT_SUB == 0 && FT_SUB % FT_BATCH == 0 && FT_SUB * 8 + FT_ACC_BUDGET <= 160 * 1024, "fold_trials tiling");

// waves per workgroup: the most of 4, 2, 1 whose accumulators fit FT_ACC_BUDGET
int ft_waves(int64_t nbin)
{
    for (int w : {4, 2, 1})
        if ((size_t)w * 64 * (size_t)nbin * 8 <= FT_ACC_BUDGET) return w;
    return 0;
}

// the bin rule of the header at the float64 sample index td: every step one IEEE operation
__device__ __forceinline__ int ft_bin(double td, double phase0, double dphase, double nbin_d, int nbin)
{
    const double p = phase0 + td * dphase;
    const double f = p - floor(p);
    const int b = (int)(f * nbin_d);  // f in [0, 1]: the product fits an int
    return b < nbin - 1 ? b : nbin - 1;
}

// the trials pu_fold would reject on the host: no fraction left to bin
__device__ __forceinline__ bool ft_bad(double phase0, double dphase, int64_t first_sample, int64_t n)
{
    const double lim = 4503599627370496.0;  // 2^52
    const double pa = phase0 + (double)first_sample * dphase;
    const double pb = phase0 + (double)(first_sample + (n > 0 ? n - 1 : 0)) * dphase;
    // (a NaN or an infinity fails the comparisons)
    return !(fabs(phase0) < INFINITY && fabs(dphase) < INFINITY && fabs(pa) < lim && fabs(pb) < lim);
}

// INC: every sample index of the chunk is below 2^53 in magnitude, so the float64 index is kept
// by adding 1.0 (exact); otherwise it is converted from the int64 index at every sample
template <bool INC>
__device__ __forceinline__ double ft_index(double td, int64_t next)
{
    return INC ? td + 1.0 : (double)next;
}

template <typename T, bool INC>
__global__ void __launch_bounds__(256) ft_fold_kernel(const T *__restrict__ x, int64_t n, int64_t ld, int64_t first_sample,
                                                      const double *__restrict__ phase0, const double *__restrict__ dphase,
                                                      int64_t ntrials, int nbin, int64_t nkt, int64_t nseg,
                                                      double *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ft_smem[];
    double *stage = reinterpret_cast<double *>(ft_smem);  // [FT_SUB]
    double *acc = stage + FT_SUB;                         // [nbin][tl]
    const int tid = threadIdx.x, tl = blockDim.x;
    const int64_t kt = blockIdx.x % nkt, rs = blockIdx.x / nkt;  // rs = row * nseg + seg
    const int64_t seg = rs % nseg, r = rs / nseg;
    const int64_t k = kt * tl + tid;
    double ph = 0.0, dp = 0.0;
    bool active = k < ntrials;
    if (active) {
        ph = phase0 ? phase0[k] : 0.0;
        dp = dphase[k];
        active = !ft_bad(ph, dp, first_sample, n);
    }
    for (int b = 0; b < nbin; ++b) acc[b * tl + tid] = 0.0;
    const T *row = x + r * ld;
    const int64_t s0 = seg * FT_SEG, send = s0 + FT_SEG < n ? s0 + FT_SEG : n;
    const double nbin_d = (double)nbin;
    int cur = -1;
    double run = 0.0;
    for (int64_t t0 = s0; t0 < send; t0 += FT_SUB) {
        __syncthreads();  // the previous sub-block's readers of stage
        for (int i = tid; i < FT_SUB; i += tl) {
            const int64_t t = t0 + i;
            stage[i] = t < send ? static_cast<double>(row[t]) : 0.0;
        }
        __syncthreads();
        if (!active) continue;
        const int cnt = (int)(send - t0 < FT_SUB ? send - t0 : FT_SUB);
        const int64_t base = first_sample + t0;
        double td = (double)base;
        for (int i0 = 0; i0 < cnt; i0 += FT_BATCH) {
            // the batch's samples and bins first (independent of the accumulators), then the adds
            double v[FT_BATCH];
            int bn[FT_BATCH];
#pragma unroll
            for (int u = 0; u < FT_BATCH; u += 2) {
                const double2 w = *reinterpret_cast<const double2 *>(&stage[i0 + u]);
                v[u] = w.x, v[u + 1] = w.y;
            }
#pragma unroll
            for (int u = 0; u < FT_BATCH; ++u) {
                bn[u] = ft_bin(td, ph, dp, nbin_d, nbin);
                td = ft_index<INC>(td, base + i0 + u + 1);
            }
#pragma unroll
            for (int u = 0; u < FT_BATCH; ++u) {
                if (i0 + u >= cnt) break;  // (uniform: the samples staged beyond the end)
                if (bn[u] != cur) {
                    if (cur >= 0) acc[cur * tl + tid] += run;
                    cur = bn[u];
                    run = v[u];
                } else {
                    run += v[u];
                }
            }
        }
    }
    if (cur >= 0) acc[cur * tl + tid] += run;
    __syncthreads();
    // the tile's partials, trial-major: consecutive threads write consecutive bins
    double *dst = part + (rs * ntrials + kt * tl) * nbin;
    const int64_t left = ntrials - kt * tl;
    const int nk = (int)(left < tl ? left : tl);
    for (int i = tid; i < nk * nbin; i += tl) dst[i] = acc[(i % nbin) * tl + i / nbin];
}

// sums[r][k][b] += the partials of (r, k, b) added in segment order; NaN for a masked trial
__global__ void ft_combine_kernel(const double *__restrict__ part, int64_t nseg, int64_t rows, int64_t ntrials, int nbin,
                                  int64_t n, int64_t first_sample, const double *__restrict__ phase0,
                                  const double *__restrict__ dphase, double *__restrict__ sums, int64_t ld_trial,
                                  int64_t ld_row)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ntrials * nbin) return;
    const int64_t b = i % nbin, rk = i / nbin, k = rk % ntrials, r = rk / ntrials;
    double *out = sums + r * ld_row + k * ld_trial + b;
    if (ft_bad(phase0 ? phase0[k] : 0.0, dphase[k], first_sample, n)) {
        *out = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const int64_t step = ntrials * nbin;
    const double *p = part + (r * nseg * ntrials + k) * nbin + b;
    double total = p[0];
    for (int64_t s = 1; s < nseg; ++s) total += p[s * step];
    *out += total;
}

// counts[k][b] += the samples of the call in bin b of trial k: lane = trial, run lengths in a
// register, uint32 LDS counters [bin][lane] per segment, then integer atomics
template <bool INC>
__global__ void __launch_bounds__(256) ft_counts_kernel(int64_t n, int64_t first_sample, const double *__restrict__ phase0,
                                                        const double *__restrict__ dphase, int64_t ntrials, int nbin,
                                                        int64_t nkt, int64_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ft_smem[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(ft_smem);  // [nbin][tl]
    const int tid = threadIdx.x, tl = blockDim.x;
    const int64_t kt = blockIdx.x % nkt, seg = blockIdx.x / nkt;
    const int64_t k = kt * tl + tid;
    if (k >= ntrials) return;  // (no barrier in this kernel: a lane owns its counters)
    const double ph = phase0 ? phase0[k] : 0.0, dp = dphase[k];
    if (ft_bad(ph, dp, first_sample, n)) return;
    for (int b = 0; b < nbin; ++b) hist[b * tl + tid] = 0;
    const int64_t s0 = seg * FT_SEG, send = s0 + FT_SEG < n ? s0 + FT_SEG : n;
    const double nbin_d = (double)nbin;
    int cur = -1;
    uint32_t len = 0;
    double td = (double)(first_sample + s0);
    for (int64_t t = s0; t < send; ++t) {
        const int b = ft_bin(td, ph, dp, nbin_d, nbin);
        td = ft_index<INC>(td, first_sample + t + 1);
        if (b != cur) {
            if (cur >= 0) hist[cur * tl + tid] += len;
            cur = b;
            len = 0;
        }
        ++len;
    }
    if (cur >= 0) hist[cur * tl + tid] += len;
    unsigned long long *out = reinterpret_cast<unsigned long long *>(counts) + k * nbin;
    for (int b = 0; b < nbin; ++b) {
        const uint32_t c = hist[b * tl + tid];
        if (c) atomicAdd(out + b, (unsigned long long)c);
    }
}

// one thread per (row, trial): the sum over the bins in bin order
__global__ void chi2_kernel(const double *__restrict__ sums, int64_t ld_trial, int64_t ld_row,
                            const int64_t *__restrict__ counts, int64_t rows, int64_t ntrials, int nbin,
                            const double *__restrict__ mean, const double *__restrict__ var, double *__restrict__ chi2,
                            int32_t *__restrict__ dof)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= rows * ntrials) return;
    const int64_t k = i % ntrials, r = i / ntrials;
    const double *s = sums + r * ld_row + k * ld_trial;
    const int64_t *c = counts + k * nbin;
    const double mu = mean[r], vr = var[r];
    double total = 0.0;
    int32_t hit = 0;
    bool ok = vr > 0.0;
    for (int b = 0; b < nbin; ++b) {
        const double sb = s[b];
        ok = ok && fabs(sb) < INFINITY;  // (in an empty bin too: a masked trial's NaN sums give NaN)
        if (c[b] <= 0) continue;
        const double cd = (double)c[b];
        const double d = sb - cd * mu;
        total += d * d / (cd * vr);
        ++hit;
    }
    chi2[i] = ok ? total : __longlong_as_double(0x7ff8000000000000ll);
    if (r == 0) dof[k] = hit - 1;
}

// the partials of rows x segments x trials x bins, in elements; -1 when they overflow
int64_t ft_partials(int64_t rows, int64_t n, int64_t ntrials, int64_t nbin)
{
    const int64_t nseg = (n + FT_SEG - 1) / FT_SEG, lim = INT64_MAX / 8;
    if (nseg > lim / rows || nseg * rows > lim / ntrials || nseg * rows * ntrials > lim / nbin) return -1;
    return nseg * rows * ntrials * nbin;
}

}  // namespace

extern "C" {

size_t pu_fold_trials_workspace_bytes(int64_t rows, int64_t n, int64_t ntrials, int64_t nbin)
{
    if (rows <= 0 || n <= 0 || ntrials <= 0 || nbin <= 0) return 0;
    const int64_t el = ft_partials(rows, n, ntrials, nbin);
    return el < 0 ? SIZE_MAX : (size_t)el * 8;
}

int pu_fold_trials(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, int64_t first_sample,
                   const double *phase0, const double *dphase, int64_t ntrials, int64_t nbin, double *sums,
                   int64_t ld_trial, int64_t ld_row, int64_t *counts, void *workspace, size_t workspace_bytes,
                   void *stream)
{
    // (a dedispersed series is float32 or float64)
    return pu::with_dtype<float, double>("pu_fold_trials", dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        PU_REQUIRE(nbin >= 2, "pu_fold_trials: nbin %lld < 2", (long long)nbin);
        PU_REQUIRE(n >= 0 && rows >= 0 && ntrials >= 0, "pu_fold_trials: negative size (rows %lld, n %lld, ntrials %lld)",
                   (long long)rows, (long long)n, (long long)ntrials);
        PU_REQUIRE(ld >= n && ld_trial >= nbin && ntrials <= INT64_MAX / ld_trial && ld_row >= ntrials * ld_trial,
                   "pu_fold_trials: leading dimension too small (ld %lld < n %lld, ld_trial %lld < nbin %lld or ld_row %lld "
                   "< ntrials x ld_trial)", (long long)ld, (long long)n, (long long)ld_trial, (long long)nbin,
                   (long long)ld_row);
        PU_REQUIRE(first_sample <= INT64_MAX - n, "pu_fold_trials: first_sample + n overflows");
        if (nbin > FT_MAX_NBIN) {
            pu::set_error("pu_fold_trials: nbin %lld above %d (a lane's bins are LDS accumulators: 64 x nbin x 8 bytes per "
                          "wave within 144 KiB)", (long long)nbin, FT_MAX_NBIN);
            return PU_EUNSUPPORTED;
        }
        if (n == 0 || rows == 0 || ntrials == 0) return PU_OK;
        const int64_t el = ft_partials(rows, n, ntrials, nbin);
        PU_REQUIRE(el >= 0, "pu_fold_trials: the partials of %lld x %lld x %lld x %lld overflow", (long long)rows,
                   (long long)n, (long long)ntrials, (long long)nbin);
        const size_t need = (size_t)el * 8;
        if (int rc = pu::check_workspace("pu_fold_trials", workspace, workspace_bytes, need, 8)) return rc;
        PU_REQUIRE(x && dphase && sums && counts, "pu_fold_trials: null pointer");
        PU_REQUIRE(reinterpret_cast<uintptr_t>(x) % sizeof(T) == 0, "pu_fold_trials: x is not aligned to its element type");
        const int w = ft_waves(nbin), tl = 64 * w;
        const int64_t nseg = (n + FT_SEG - 1) / FT_SEG, nkt = (ntrials + tl - 1) / tl;
        PU_REQUIRE(nseg <= INT32_MAX / nkt && nseg * nkt <= INT32_MAX / rows && el / nseg <= INT32_MAX * (int64_t)128,
                   "pu_fold_trials: %lld rows x %lld segments x %lld trial tiles exceed the grid limit", (long long)rows,
                   (long long)nseg, (long long)nkt);
        // float64 sample indices by adding 1.0 while every index of the chunk is below 2^53
        const int64_t big = (int64_t)1 << 53;
        const bool inc = first_sample > -big && first_sample + n < big;
        const size_t lds = (size_t)FT_SUB * 8 + (size_t)tl * nbin * 8, clds = (size_t)tl * nbin * 4;
        hipStream_t s = pu::as_stream(stream);
        const dim3 grid((unsigned)(rows * nseg * nkt)), block(tl);
        double *part = static_cast<double *>(workspace);
        const int nb = (int)nbin;
        const T *xs = static_cast<const T *>(x);
        // (either instance, then one check)
        if (inc) {
            if (int rc = pu::ensure_lds(ft_fold_kernel<T, true>, lds)) return rc;
            hipLaunchKernelGGL((ft_fold_kernel<T, true>), grid, block, lds, s, xs, n, ld, first_sample, phase0, dphase, ntrials, nb, nkt, nseg, part);
        } else {
            if (int rc = pu::ensure_lds(ft_fold_kernel<T, false>, lds)) return rc;
            hipLaunchKernelGGL((ft_fold_kernel<T, false>), grid, block, lds, s, xs, n, ld, first_sample, phase0, dphase, ntrials, nb, nkt, nseg, part);
        }
        if (int rc = pu::launch_check("ft_fold_kernel")) return rc;
        const unsigned cgrid = (unsigned)((rows * ntrials * nbin + 255) / 256);
        if (int rc = pu::launch("ft_combine_kernel", ft_combine_kernel, dim3(cgrid), dim3(256), 0, s, part, nseg, rows, ntrials, nb,
                                n, first_sample, phase0, dphase, sums, ld_trial, ld_row))
            return rc;
        const dim3 hgrid((unsigned)(nseg * nkt));
        if (inc) {
            if (int rc = pu::ensure_lds(ft_counts_kernel<true>, clds)) return rc;
            hipLaunchKernelGGL(ft_counts_kernel<true>, hgrid, block, clds, s, n, first_sample, phase0, dphase, ntrials, nb, nkt, counts);
        } else {
            if (int rc = pu::ensure_lds(ft_counts_kernel<false>, clds)) return rc;
            hipLaunchKernelGGL(ft_counts_kernel<false>, hgrid, block, clds, s, n, first_sample, phase0, dphase, ntrials, nb, nkt, counts);
        }
        return pu::launch_check("ft_counts_kernel");
    });
}

int pu_profile_chi2(const double *sums, int64_t ld_trial, int64_t ld_row, const int64_t *counts, int64_t rows,
                    int64_t ntrials, int64_t nbin, const double *mean, const double *var, double *chi2, int32_t *dof,
                    void *stream)
{
    PU_REQUIRE(nbin >= 2, "pu_profile_chi2: nbin %lld < 2", (long long)nbin);
    PU_REQUIRE(rows >= 0 && ntrials >= 0, "pu_profile_chi2: negative size (rows %lld, ntrials %lld)", (long long)rows,
               (long long)ntrials);
    PU_REQUIRE(ld_trial >= nbin && ntrials <= INT64_MAX / ld_trial && ld_row >= ntrials * ld_trial,
               "pu_profile_chi2: leading dimension too small (ld_trial %lld < nbin %lld or ld_row %lld < ntrials x "
               "ld_trial)", (long long)ld_trial, (long long)nbin, (long long)ld_row);
    PU_REQUIRE(nbin <= INT32_MAX, "pu_profile_chi2: nbin %lld above the int32 range of dof", (long long)nbin);
    if (rows == 0 || ntrials == 0) return PU_OK;
    PU_REQUIRE(sums && counts && mean && var && chi2 && dof, "pu_profile_chi2: null pointer");
    PU_REQUIRE(rows <= INT32_MAX * (int64_t)256 / ntrials, "pu_profile_chi2: %lld rows x %lld trials exceed the grid limit",
               (long long)rows, (long long)ntrials);
    return pu::launch("chi2_kernel", chi2_kernel, dim3((unsigned)((rows * ntrials + 255) / 256)), dim3(256), 0,
                      pu::as_stream(stream), sums, ld_trial, ld_row, counts, rows, ntrials, (int)nbin, mean, var, chi2, dof);
}

}  // extern "C"
