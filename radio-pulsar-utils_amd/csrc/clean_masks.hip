// The channel-mask decisions of the RFI cleaning for gfx950 (MI355X), each one workgroup:
// get_noisier_channels (clean.py:58-67) and measure_channel_variability's certified
// decision (:114-133) from the row means and shifted moments of clean_rows.hip, in numpy's
// dtypes and operation order (compiled with -ffp-contract=off: clean_common.h).
//
// Kernels
//   noisy_channels_kernel    medfilt(spec, 7) and the MAD of diff(spec): two sorts, a 7-window rank.
//   variability_cert_kernel  std bounds per channel, quartile intervals by two sorts.
//   channel_masks_kernel     both for n <= 1024 in one launch, the sorts in registers
//                            (sort_regs_1024: DPP / permlane exchanges inside a wave).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "clean_common.h"

namespace {

// ---------------------------------------------------------------- noisy channels
// get_noisier_channels' decision on the device (clean.py:58-67, stats.py:11-32): one
// workgroup, spec of n <= kNoisyMax channel means in T (float32 for float32 input, else
// float64: numpy's mean dtype).  The host path it replaces did medfilt + ref_mad in numpy
// after a read-back of spec; every step here keeps numpy's dtypes (NEP 50) and order:
//   smooth = medfilt(spec, 7)           rank 3 of the zero-padded 7-window (T, exact)
//   d = diff(spec)                      T, then float64: statsmodels 0.12.2's mad starts with
//                                       array_like(a, dtype=np.double) (robust/scale.py:49)
//   m = median(d)                       float64: the middle element, or (a + b) / 2
//   e = |d - m| / c                     float64
//   rm = median(e) / sqrt(2)            float64
//   mask = spec > smooth + 5 rm         float64
// A non-finite spec (NaN / inf: medfilt's and median's handling of them is left to
// numpy / scipy) sets *flag and leaves mask unwritten: the caller then takes the host path.
constexpr int kNoisyMax = 4096;

template <typename T>
__device__ void bitonic_sort_lds(T *v, int m)  // m: power of two, 1024 threads
{
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < m; i += 1024) {
                const int l = i ^ j;
                if (l > i) {
                    const T a = v[i], b = v[l];
                    const bool up = (i & k) == 0;
                    if (up ? (b < a) : (a < b)) {
                        v[i] = b;
                        v[l] = a;
                    }
                }
            }
            __syncthreads();
        }
}

// x of lane (lane ^ J) within the wave, on the VALU (no LDS round trip): DPP quad
// permutes for J = 1, 2, row rotations for 4, 8 (J = 4: rotations by 4 and 12, the one
// whose source is lane ^ 4 picked per lane - sel4, computed once by the caller from the
// same rotation of the lane ids), the gfx950 permlane swaps for 16, 32 (the pair returns
// rows / halves exchanged: lanes in the upper row / half take the first result).
template <int J>
__device__ __forceinline__ double lane_xor(double x, int lane, bool sel4)
{
    const uint64_t u = __builtin_bit_cast(uint64_t, x);
    uint32_t w[2] = {(uint32_t)u, (uint32_t)(u >> 32)};
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int v = (int)w[h];
        if constexpr (J == 1) {
            w[h] = (uint32_t)__builtin_amdgcn_mov_dpp(v, 0xB1, 0xf, 0xf, false);  // quad_perm [1,0,3,2]
        } else if constexpr (J == 2) {
            w[h] = (uint32_t)__builtin_amdgcn_mov_dpp(v, 0x4E, 0xf, 0xf, false);  // quad_perm [2,3,0,1]
        } else if constexpr (J == 4) {
            const int a = __builtin_amdgcn_mov_dpp(v, 0x124, 0xf, 0xf, false);  // row_ror:4
            const int b = __builtin_amdgcn_mov_dpp(v, 0x12C, 0xf, 0xf, false);  // row_ror:12
            w[h] = (uint32_t)(sel4 ? a : b);
        } else if constexpr (J == 8) {
            w[h] = (uint32_t)__builtin_amdgcn_mov_dpp(v, 0x128, 0xf, 0xf, false);  // row_ror:8
        } else if constexpr (J == 16) {
            const auto r = __builtin_amdgcn_permlane16_swap((unsigned)v, (unsigned)v, false, false);
            w[h] = (lane & 16) ? (uint32_t)r[0] : (uint32_t)r[1];
        } else {
            static_assert(J == 32, "lane_xor: J = 1 .. 32");
            const auto r = __builtin_amdgcn_permlane32_swap((unsigned)v, (unsigned)v, false, false);
            w[h] = (lane & 32) ? (uint32_t)r[0] : (uint32_t)r[1];
        }
    }
    return __builtin_bit_cast(double, (uint64_t)w[0] | ((uint64_t)w[1] << 32));
}

// min / max of two doubles that are never NaN (the sorts' callers check: __syncthreads_or) in
// one instruction each (a compare + two selects per 32-bit half otherwise)
__device__ __forceinline__ double min_nn(double a, double b)
{
    double r;
    asm("v_min_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}
__device__ __forceinline__ double max_nn(double a, double b)
{
    double r;
    asm("v_max_f64 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

// the bitonic compare-exchange of x with its partner y: the smaller value stays when
// keep_min (exact: min / max of non-NaN values)
__device__ __forceinline__ double bitonic_keep(double x, double y, bool keep_min)
{
    const double lo = min_nn(x, y), hi = max_nn(x, y);
    return keep_min ? lo : hi;
}

// the in-wave bitonic steps j = J, J/2, .., 1 of merge size k (lane_xor exchanges)
template <int J>
__device__ __forceinline__ void bitonic_wave_steps(double &x, int i, int k, int lane, bool sel4)
{
    const double y = lane_xor<J>(x, lane, sel4);
    x = bitonic_keep(x, y, ((i & J) == 0) == ((i & k) == 0));
    if constexpr (J > 1) bitonic_wave_steps<J / 2>(x, i, k, lane, sel4);
}

// NV independent ascending sorts over the 1024 threads of the workgroup, one value of each
// per thread in x[q] (thread i ends with the i-th smallest of sort q), the sorts sharing
// every barrier.  Bitonic: the 45 of the 55 steps whose partner is in the same wave
// exchange on the VALU (lane_xor: DPP and permlane swaps, no barrier; round 5 first:
// __shfl_xor, an LDS permute per step), the 10 with a partner in another wave through ex
// (NV x 2048 doubles of LDS, two alternating halves per sort: one barrier per step).  ex
// must be free on entry; the caller synchronises before reusing it.  No value is NaN (each
// caller tests that first and hands the decision to the host), so min / max are exact.
template <int NV>
__device__ void sort_regs_1024(double (&x)[NV], double *ex)
{
    const int i = threadIdx.x;
    const int lane = i & 63;
    // the lane whose value row_ror:4 brings (whatever the rotation's direction)
    const bool sel4 = __builtin_amdgcn_mov_dpp(lane, 0x124, 0xf, 0xf, false) == (lane ^ 4);
    // merge sizes 2 .. 64 inside each wave
#pragma unroll
    for (int q = 0; q < NV; ++q) {
        bitonic_wave_steps<1>(x[q], i, 2, lane, sel4);
        bitonic_wave_steps<2>(x[q], i, 4, lane, sel4);
        bitonic_wave_steps<4>(x[q], i, 8, lane, sel4);
        bitonic_wave_steps<8>(x[q], i, 16, lane, sel4);
        bitonic_wave_steps<16>(x[q], i, 32, lane, sel4);
        bitonic_wave_steps<32>(x[q], i, 64, lane, sel4);
    }
    int half = 0;
    for (int k = 128; k <= 1024; k <<= 1) {
        for (int j = k >> 1; j >= 64; j >>= 1) {
            double *e = ex + 1024 * half;
#pragma unroll
            for (int q = 0; q < NV; ++q) e[2048 * q + i] = x[q];
            __syncthreads();
            half ^= 1;  // the next exchange writes the other half: no second barrier
            const bool keep_min = ((i & j) == 0) == ((i & k) == 0);
#pragma unroll
            for (int q = 0; q < NV; ++q) x[q] = bitonic_keep(x[q], e[2048 * q + (i ^ j)], keep_min);
        }
#pragma unroll
        for (int q = 0; q < NV; ++q) bitonic_wave_steps<32>(x[q], i, k, lane, sel4);
    }
}

// Ascending sort of v[0, m) (m a power of two) by 1024 threads.  m <= 1024: one element per
// thread, +inf padding to 1024, sort_regs_1024 with v itself as the exchange (v must hold
// 2048 elements).  Larger m: bitonic_sort_lds.
__device__ void sort_1024(double *v, int m)
{
    if (m > 1024) {
        bitonic_sort_lds(v, m);
        return;
    }
    const int i = threadIdx.x;
    double x[1] = {i < m ? v[i] : INFINITY};
    __syncthreads();  // every thread has its element before v is reused as the exchange
    sort_regs_1024<1>(x, v);
    __syncthreads();  // every exchange read is done
    if (i < m) v[i] = x[0];
    __syncthreads();
}

template <typename T>
__device__ T median_sorted(const T *v, int cnt)  // numpy: middle element / mean of the two
{
    if (cnt & 1) return v[cnt / 2];
    const T s = v[cnt / 2 - 1] + v[cnt / 2];
    return s / T(2);
}

template <typename T>
__global__ void __launch_bounds__(1024)
noisy_channels_kernel(const T *__restrict__ spec, int n, double c, uint8_t *__restrict__ mask,
                      int32_t *__restrict__ flag)
{
    __shared__ T sp[kNoisyMax];
    __shared__ double ev[kNoisyMax];  // the sorted differences, then the sorted e (float64)
    const int tid = threadIdx.x;
    int nonfinite = 0;
    for (int i = tid; i < n; i += 1024) {
        const T v = spec[i];
        sp[i] = v;
        nonfinite |= !isfinite((double)v);
    }
    if (__syncthreads_or(nonfinite)) {
        if (tid == 0) flag[0] = 1;
        return;
    }
    int m = 1;
    while (m < n - 1) m <<= 1;
    // the differences in T (np.diff of the T spectrum), then exactly widened to float64
    for (int i = tid; i < m; i += 1024) ev[i] = i < n - 1 ? (double)T(sp[i + 1] - sp[i]) : INFINITY;
    __syncthreads();
    sort_1024(ev, m);
    const double med = median_sorted(ev, n - 1);
    __syncthreads();  // every thread has read the median before ev is overwritten
    int nan_e = 0;
    for (int i = tid; i < m; i += 1024) {
        ev[i] = i < n - 1 ? fabs((double)T(sp[i + 1] - sp[i]) - med) / c : INFINITY;
        nan_e |= isnan(ev[i]);
    }
    // a NaN (inf - inf after a float32 difference overflowed) would be dropped by the
    // register sort's min / max: the host decides
    if (__syncthreads_or(nan_e)) {
        if (tid == 0) flag[0] = 1;
        return;
    }
    sort_1024(ev, m);
    const double rm = median_sorted(ev, n - 1) / 1.4142135623730951;  // np.sqrt(2)
    const double thr = 5.0 * rm;
    for (int i = tid; i < n; i += 1024) {
        T w[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int k = i + j - 3;
            w[j] = (k >= 0 && k < n) ? sp[k] : T(0);
        }
        // rank 3 of 7 (a full insertion sort of the window: exact selection)
#pragma unroll
        for (int a = 1; a < 7; ++a)
#pragma unroll
            for (int b = a; b > 0; --b)
                if (w[b] < w[b - 1]) {
                    const T t = w[b];
                    w[b] = w[b - 1];
                    w[b - 1] = t;
                }
        mask[i] = (double)sp[i] > (double)w[3] + thr ? 1 : 0;
    }
    if (tid == 0) flag[0] = 0;
}

// ---------------------------------------------------------------- variability mask
// measure_channel_variability's certified decision (clean.py:114-133) on the device: the
// host restatement clean._certified_variability, step for step in float64 (same operation
// order), from the means pass's numpy means (T) and shifted moments (c, s1, s2) per row:
//   V = s2 - 2 dm s1 + n dm^2, dm = m - c;  eV = (s2 + 2 |dm| sqrt(n s2) + n dm^2) mef
//   s_lo / s_hi = numpy's std bounds;  q1..q3 intervals = the k-th smallest s_lo / s_hi of
//   the good channels (k = nrows/4, nrows/2, 3 nrows/4: the reference's indices);
//   the limit intervals; a channel is decided when it is clear of both.
// One workgroup, nrows <= kNoisyMax: bad channels' bounds are +inf in the two bitonic
// sorts, so the k-th smallest of all is the k-th smallest good one.  *flag = 1 (mask not
// written) for non-finite statistics, too few good channels, or any undecided channel:
// the caller then runs the exact second pass.
__device__ __forceinline__ void variability_bounds(double m, const double *mom, double nd, double mef, double gam,
                                                   double u, double &lo, double &hi)
{
    const double c = mom[0], s1 = mom[1], s2 = mom[2];
    const double dm = m - c;
    const double V = (s2 - (2.0 * dm) * s1) + (nd * dm) * dm;
    const double eV = ((s2 + (2.0 * fabs(dm)) * sqrt(nd * s2)) + (nd * dm) * dm) * mef + 1e-300;
    lo = sqrt(fmax(V - eV, 0.0) * (1.0 - gam) / nd * (1.0 - u)) * (1.0 - u);
    hi = sqrt((V + eV) * (1.0 + gam) / nd * (1.0 + u)) * (1.0 + u);
}

template <typename T>
__global__ void __launch_bounds__(1024)
variability_cert_kernel(const T *__restrict__ means, const double *__restrict__ mom, int nrows, double nd,
                        double mef, double gam, double u, const uint8_t *__restrict__ bad,
                        uint8_t *__restrict__ mask, int32_t *__restrict__ flag)
{
    __shared__ double lo[kNoisyMax], hi[kNoisyMax];
    __shared__ int gsum;
    const int tid = threadIdx.x;
    if (tid == 0) gsum = 0;
    __syncthreads();
    int nonfinite = 0, good = 0;
    for (int i = tid; i < nrows; i += 1024) {
        const double m = (double)means[i];
        nonfinite |= !isfinite(m) || !isfinite(mom[3 * i]) || !isfinite(mom[3 * i + 1]) || !isfinite(mom[3 * i + 2]);
        good += bad[i] == 0;
    }
    if (good) atomicAdd(&gsum, good);
    const int any_nf = __syncthreads_or(nonfinite);  // (also orders the LDS adds before the read)
    const int ngood = gsum;
    if (any_nf || nrows / 4 * 3 >= ngood) {
        if (tid == 0) flag[0] = 1;
        return;
    }
    int m2 = 1;
    while (m2 < nrows) m2 <<= 1;
    for (int i = tid; i < m2; i += 1024) {
        double a = INFINITY, b = INFINITY;
        if (i < nrows && bad[i] == 0) variability_bounds((double)means[i], mom + 3 * i, nd, mef, gam, u, a, b);
        lo[i] = a;
        hi[i] = b;
    }
    __syncthreads();
    sort_1024(lo, m2);
    sort_1024(hi, m2);
    const double a1 = lo[nrows / 4], b1 = hi[nrows / 4];
    const double a2 = lo[nrows / 2], b2 = hi[nrows / 2];
    const double a3 = lo[nrows / 4 * 3], b3 = hi[nrows / 4 * 3];
    const double r = 4.0 * u * (b2 + 2.0 * (b3 - a1)) + 1e-300;
    const double low_lo = (2.0 * a1 - b2) - r, low_hi = (2.0 * b1 - a2) + r;
    const double hi_lo = (2.0 * a3 - b2) - r, hi_hi = (2.0 * b3 - a2) + r;
    int unsure = 0;
    for (int i = tid; i < nrows; i += 1024) {
        double sl, sh;
        variability_bounds((double)means[i], mom + 3 * i, nd, mef, gam, u, sl, sh);
        const bool below = sh < low_lo, above = sl > hi_hi;
        const bool sure = (below || sl >= low_hi) && (above || sh <= hi_lo);
        const bool b = bad[i] != 0;
        unsure |= !b && !sure;
        mask[i] = (below || above || b) ? 1 : 0;
    }
    const int any_unsure = __syncthreads_or(unsure);
    if (tid == 0) flag[0] = any_unsure ? 1 : 0;
}

// get_noisier_channels' decision and then measure_channel_variability's for that mask, in
// ONE workgroup and one launch (n <= 1024; round 5: the two kernels above back to back).
// Thread i owns channel i: the noisy-channel steps of noisy_channels_kernel (the two sorts
// of the differences, the 7-window rank), the mask kept in a register as the variability
// certification's bad mask (variability_cert_kernel's steps, the channel's std bounds
// computed once, the lower- and upper-bound sorts sharing their barriers).  spec = the
// row means (numpy's mean dtype T), mom their shifted moments (pu_row_moments).
constexpr int kMasksMax = 1024;

template <typename T>
__global__ void __launch_bounds__(1024)
channel_masks_kernel(const T *__restrict__ spec, const double *__restrict__ mom, int n, double c, double nd,
                     double mef, double gam, double u, uint8_t *__restrict__ nmask, int32_t *__restrict__ nflag,
                     uint8_t *__restrict__ vmask, int32_t *__restrict__ vflag)
{
    __shared__ double ex[2 * 2048];
    __shared__ T sp[kMasksMax];
    __shared__ double ord[8];  // order statistics handed between threads
    const int tid = threadIdx.x;
    const bool in = tid < n;
    const T sv = in ? spec[tid] : T(0);
    if (in) sp[tid] = sv;
    if (__syncthreads_or(in && !isfinite((double)sv))) {
        if (tid == 0) {
            nflag[0] = 1;  // the host decides both masks
            vflag[0] = 1;
        }
        return;
    }
    // ---- noisy channels (clean.py:58-67; noisy_channels_kernel)
    const int nd1 = n - 1;
    const double d = tid < nd1 ? (double)T(sp[tid + 1] - sp[tid]) : INFINITY;
    auto median_of_sorted = [&](double v) {  // numpy's median of the nd1 sorted values
        if (nd1 & 1) {
            if (tid == nd1 / 2) ord[0] = v;
        } else {
            if (tid == nd1 / 2 - 1) ord[0] = v;
            if (tid == nd1 / 2) ord[1] = v;
        }
        __syncthreads();
        const double r = (nd1 & 1) ? ord[0] : (ord[0] + ord[1]) / 2.0;
        __syncthreads();  // ord read by every thread before its next use
        return r;
    };
    double x1[1] = {d};
    sort_regs_1024<1>(x1, ex);
    const double med = median_of_sorted(x1[0]);  // (its barriers also free ex)
    x1[0] = tid < nd1 ? fabs(d - med) / c : INFINITY;
    // the register sorts' v_min_f64 / v_max_f64 drop a NaN operand: a NaN here (a float32
    // difference that overflowed to inf, then inf - inf) hands both decisions to the host
    if (__syncthreads_or(isnan(x1[0]))) {
        if (tid == 0) {
            nflag[0] = 1;
            vflag[0] = 1;
        }
        return;
    }
    sort_regs_1024<1>(x1, ex);
    const double rm = median_of_sorted(x1[0]) / 1.4142135623730951;  // np.sqrt(2)
    const double thr = 5.0 * rm;
    bool bad = false;
    if (in) {
        T w[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int k = tid + j - 3;
            w[j] = (k >= 0 && k < n) ? sp[k] : T(0);
        }
#pragma unroll
        for (int a = 1; a < 7; ++a)
#pragma unroll
            for (int b = a; b > 0; --b)
                if (w[b] < w[b - 1]) {
                    const T t = w[b];
                    w[b] = w[b - 1];
                    w[b - 1] = t;
                }
        bad = (double)sv > (double)w[3] + thr;
        nmask[tid] = bad ? 1 : 0;
    }
    if (tid == 0) nflag[0] = 0;
    // ---- variability (clean.py:114-133; variability_cert_kernel) with bad = the noisy mask
    const double *mr = mom + 3 * (in ? tid : 0);
    const bool nf = in && (!isfinite(mr[0]) || !isfinite(mr[1]) || !isfinite(mr[2]));
    const int any_nf = __syncthreads_or(nf);
    const int ngood = __syncthreads_count(in && !bad);
    if (any_nf || n / 4 * 3 >= ngood) {
        if (tid == 0) vflag[0] = 1;
        return;
    }
    double sl = INFINITY, sh = INFINITY;
    if (in) variability_bounds((double)sv, mr, nd, mef, gam, u, sl, sh);
    double x2[2] = {in && !bad ? sl : INFINITY, in && !bad ? sh : INFINITY};
    if (__syncthreads_or(isnan(x2[0]) || isnan(x2[1]))) {  // (NaN bounds: the host decides)
        if (tid == 0) vflag[0] = 1;
        return;
    }
    sort_regs_1024<2>(x2, ex);
    const int k1 = n / 4, k2 = n / 2, k3 = n / 4 * 3;
    if (tid == k1) { ord[2] = x2[0]; ord[3] = x2[1]; }
    if (tid == k2) { ord[4] = x2[0]; ord[5] = x2[1]; }
    if (tid == k3) { ord[6] = x2[0]; ord[7] = x2[1]; }
    __syncthreads();
    const double a1 = ord[2], b1 = ord[3], a2 = ord[4], b2 = ord[5], a3 = ord[6], b3 = ord[7];
    const double r = 4.0 * u * (b2 + 2.0 * (b3 - a1)) + 1e-300;
    const double low_lo = (2.0 * a1 - b2) - r, low_hi = (2.0 * b1 - a2) + r;
    const double hi_lo = (2.0 * a3 - b2) - r, hi_hi = (2.0 * b3 - a2) + r;
    int unsure = 0;
    if (in) {
        const bool below = sh < low_lo, above = sl > hi_hi;
        const bool sure = (below || sl >= low_hi) && (above || sh <= hi_lo);
        unsure = !bad && !sure;
        vmask[tid] = (below || above || bad) ? 1 : 0;
    }
    const int any_unsure = __syncthreads_or(unsure);
    if (tid == 0) vflag[0] = any_unsure ? 1 : 0;
}

}  // namespace

extern "C" {

int pu_variability_cert(const void *means, int dtype, const double *moments, int64_t nrows, int64_t n, double mef,
                        double gam, double u, const uint8_t *bad, uint8_t *mask, int32_t *flag, void *stream)
{
    PU_REQUIRE(means && moments && bad && mask && flag, "pu_variability_cert: NULL pointer");
    PU_REQUIRE(nrows >= 1 && nrows <= kNoisyMax, "pu_variability_cert: nrows = %lld outside [1, %d]",
               (long long)nrows, kNoisyMax);
    PU_REQUIRE(n >= 1, "pu_variability_cert: n must be positive");
    PU_REQUIRE(dtype == PU_F32 || dtype == PU_F64, "pu_variability_cert: means must be float32 or float64");
    return pu::with_dtype<float, double>("pu_variability_cert", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return pu::launch("variability_cert_kernel", variability_cert_kernel<T>, dim3(1), dim3(1024), 0,
                          pu::as_stream(stream), reinterpret_cast<const T *>(means), moments, (int)nrows, (double)n, mef,
                          gam, u, bad, mask, flag);
    });
}

int pu_noisy_channels(const void *spec, int dtype, int64_t n, double mad_c, uint8_t *mask, int32_t *flag,
                      void *stream)
{
    PU_REQUIRE(spec && mask && flag, "pu_noisy_channels: NULL pointer");
    PU_REQUIRE(n >= 2 && n <= kNoisyMax, "pu_noisy_channels: n = %lld outside [2, %d]", (long long)n, kNoisyMax);
    PU_REQUIRE(dtype == PU_F32 || dtype == PU_F64, "pu_noisy_channels: spec must be float32 or float64");
    return pu::with_dtype<float, double>("pu_noisy_channels", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return pu::launch("noisy_channels_kernel", noisy_channels_kernel<T>, dim3(1), dim3(1024), 0, pu::as_stream(stream),
                          reinterpret_cast<const T *>(spec), (int)n, mad_c, mask, flag);
    });
}

int pu_channel_masks(const void *means, int dtype, const double *moments, int64_t nrows, int64_t n, double mad_c,
                     double mef, double gam, double u, uint8_t *noisy, int32_t *noisy_flag, uint8_t *var,
                     int32_t *var_flag, void *stream)
{
    PU_REQUIRE(means && moments && noisy && noisy_flag && var && var_flag, "pu_channel_masks: NULL pointer");
    PU_REQUIRE(nrows >= 2 && nrows <= kMasksMax, "pu_channel_masks: nrows = %lld outside [2, %d]", (long long)nrows,
               kMasksMax);
    PU_REQUIRE(n >= 1, "pu_channel_masks: n must be positive");
    PU_REQUIRE(dtype == PU_F32 || dtype == PU_F64, "pu_channel_masks: means must be float32 or float64");
    return pu::with_dtype<float, double>("pu_channel_masks", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return pu::launch("channel_masks_kernel", channel_masks_kernel<T>, dim3(1), dim3(1024), 0, pu::as_stream(stream),
                          reinterpret_cast<const T *>(means), moments, (int)nrows, mad_c, (double)n, mef, gam, u, noisy,
                          noisy_flag, var, var_flag);
    });
}

}  // extern "C"
