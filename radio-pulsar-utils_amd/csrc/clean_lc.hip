// The light-curve chain of the RFI cleaning for gfx950 (MI355X): the zero-DM series
// smoothed, its median, the renormalisation factor, and cut_outliers (clean.py:77-105),
// each bit for bit with scipy / numpy (order and -ffp-contract=off: clean_common.h).
//
// Kernels
//   gauss_quad_kernel    scipy correlate1d symmetric order, mode 'reflect' (:79): four
//                        adjacent outputs per thread from an LDS window (gauss_kernel:
//                        direct form for huge radii).
//   median_*_kernel      np.median by radix select over order-preserving keys (:80).
//   ratio_kernel, ratio_dev_kernel   median / smoothed series (:81).
//   outlier_*_kernel     cut_outliers (:93-105): certified decisions on directly summed
//                        window means, launch by launch or in one launch behind grid
//                        barriers (outlier_fused_kernel), and the reference's own running
//                        sum when a decision is ambiguous (outlier_exact_kernel).
#include <atomic>
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "clean_common.h"

namespace {

// Direct form (radius too large for the LDS window).
__global__ void gauss_kernel(const double *__restrict__ x, int64_t n, const double *__restrict__ w,
                             int64_t r, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double acc = x[i] * w[r];
    for (int64_t jj = -r; jj < 0; ++jj)
        acc += (x[reflect_index(i + jj, n)] + x[reflect_index(i - jj, n)]) * w[r + jj];
    out[i] = acc;
}

// LDS form (r <= kGaussMaxR): a workgroup stages its outputs' window (reflected once, at
// staging, kGaussPad extra samples at either end) and the r+1 weights.
constexpr int kGaussMaxR = 2048;
constexpr int kGaussPad = 2;
typedef double f64x2 __attribute__((ext_vector_type(2)));

// Quad form (round 4): each thread computes FOUR adjacent outputs i..i+3 from two sliding
// register windows, left x[i+j .. i+j+3] and right x[i-j .. i-j+3]; per two taps one new
// 16-B pair enters each window, so the LDS traffic per output-tap is 4 B plus a broadcast
// weight pair (the two-output form it replaced: 12 B).  The next two
// taps' pairs are read one iteration ahead.  1024 outputs per workgroup (one workgroup per CU
// at n = 2^18, one wave per SIMD: the f64 adds, not LDS, set the pace).  Per output the
// order is scipy's: acc = x[i] w[r], then acc += (x[i+j] + x[i-j]) w[r+j], j = -r..-1.
constexpr int kGaussQuadThreads = 256;

// One workgroup's 4 T outputs [i0, i0 + 4 T) into a[4] (thread t: outputs i0 + 4 t + q),
// T = kGaussQuadThreads.
// gsm4: LDS of ((r + 2) & ~1) + 4 T + 2 r + 2 kGaussPad doubles.  Returns after the last
// LDS read of the workgroup's staging only once every thread has passed the staging barrier
// (callers that restage must __syncthreads() first).
__device__ __forceinline__ void gauss_quad_segment(const double *__restrict__ x, int64_t n, const double *__restrict__ w,
                                                   int r, int64_t i0, double *gsm4, double (&a)[4])
{
    constexpr int T = kGaussQuadThreads;
    const int wn = (r + 2) & ~1;  // weights padded to an even count: the window stays 16-B aligned
    double *ws = gsm4;
    double *xs = gsm4 + wn;       // x[i0 - r - pad, i0 + 1024 + r + pad), reflected at staging
    const int span = (4 * T) + 2 * r + 2 * kGaussPad;
    for (int k = threadIdx.x; k < wn; k += T) ws[k] = k <= r ? w[k] : 0.0;
    const int64_t g0 = i0 - r - kGaussPad;
    if (g0 >= 0 && g0 + span <= n) {  // interior workgroup (uniform): no reflection
        for (int k = threadIdx.x; k < span; k += T) xs[k] = x[g0 + k];
    } else {
        for (int k = threadIdx.x; k < span; k += T) {
            const int64_t g = g0 + k;
            xs[k] = x[(g >= 0 && g < n) ? g : reflect_index(g, n)];
        }
    }
    __syncthreads();
    const int t4 = 4 * (int)threadIdx.x;
    // xc[q] = x[i + q]; xc + m is 16-B aligned whenever m + r is even (pad even, t4 even)
    const double *xc = xs + t4 + r + kGaussPad;
    auto pair = [&](int m) { return *reinterpret_cast<const f64x2 *>(xc + m); };
    auto wpair = [&](int m) { return *reinterpret_cast<const f64x2 *>(ws + r + m); };  // w[r+m], w[r+m+1]
    const double wr = ws[r];
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] = xc[q] * wr;
    int j = -r;
    f64x2 l01 = pair(j), l23 = pair(j + 2);    // left  window xc[j .. j+3]
    f64x2 r01 = pair(-j), r23 = pair(-j + 2);  // right window xc[-j .. -j+3]
    // the next two taps' window and weight pairs are read one iteration ahead (one wave per
    // SIMD: nothing else covers the LDS latency)
    f64x2 p = {0.0, 0.0}, s = {0.0, 0.0}, wp = {0.0, 0.0};
    if (r >= 2) {
        p = pair(j + 4);   // xc[j+4], xc[j+5]
        s = pair(-j - 2);  // xc[-j-2], xc[-j-1]
        wp = wpair(j);
    }
#pragma unroll 2
    for (; j + 1 < 0; j += 2) {
        const int jn = j + 3 < 0 ? j + 2 : j;  // the last iteration reloads its own (in bounds)
        const f64x2 pn = pair(jn + 4), sn = pair(-jn - 2), wpn = wpair(jn);
        const double w0 = wp.x, w1 = wp.y;
        // tap j: left xc[j+q], right xc[q-j]
        a[0] += (l01.x + r01.x) * w0;
        a[1] += (l01.y + r01.y) * w0;
        a[2] += (l23.x + r23.x) * w0;
        a[3] += (l23.y + r23.y) * w0;
        // tap j+1: left xc[j+1+q], right xc[q-j-1]
        a[0] += (l01.y + s.y) * w1;
        a[1] += (l23.x + r01.x) * w1;
        a[2] += (l23.y + r01.y) * w1;
        a[3] += (p.x + r23.x) * w1;
        l01 = l23;
        l23 = p;
        r23 = r01;
        r01 = s;
        p = pn;
        s = sn;
        wp = wpn;
    }
    if (j < 0) {  // odd r: the last tap, j = -1
        const double w0 = ws[r - 1];
        a[0] += (l01.x + r01.x) * w0;
        a[1] += (l01.y + r01.y) * w0;
        a[2] += (l23.x + r23.x) * w0;
        a[3] += (l23.y + r23.y) * w0;
    }
}

__global__ void __launch_bounds__(kGaussQuadThreads)
gauss_quad_kernel(const double *__restrict__ x, int64_t n, const double *__restrict__ w, int r,
                  double *__restrict__ out)
{
    extern __shared__ __attribute__((aligned(16))) double gsm4[];
    const int64_t i0 = (int64_t)blockIdx.x * (4 * kGaussQuadThreads);
    double a[4];
    gauss_quad_segment(x, n, w, r, i0, gsm4, a);
    const int64_t i = i0 + 4 * (int)threadIdx.x;
    if (i + 3 < n && (reinterpret_cast<uintptr_t>(out) & 15) == 0) {
        *reinterpret_cast<f64x2 *>(out + i) = f64x2{a[0], a[1]};
        *reinterpret_cast<f64x2 *>(out + i + 2) = f64x2{a[2], a[3]};
    } else {
#pragma unroll
        for (int q = 0; q < 4; ++q)
            if (i + q < n) out[i + q] = a[q];
    }
}

__global__ void ratio_kernel(double num, const double *__restrict__ x, int64_t n, double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = num / x[i];
}

__global__ void ratio_dev_kernel(const double *__restrict__ num, const double *__restrict__ x, int64_t n,
                                 double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = num[0] / x[i];
}

// ---------------------------------------------------------------- cut_outliers
// clean.py:93-105 on the device.  Only the last window (16) of the reference loop
// survives: lc_rebin = uniform_filter1d(lc, 16) (mode reflect: window [i-8, i+7]),
// sd = np.std(lc_rebin[::16]), bad = lc_rebin > 5 sd | lc_rebin < -3 sd.
//
// scipy evaluates lc_rebin as a sequential running sum (tmp += (x[i+7] - x[i-9]) / 16),
// a chain no parallel order reproduces bit for bit.  The kernels instead compute each
// window sum directly (u[i]) and CERTIFY every decision: with L = max |lc|, both the
// chain value v[i] and u[i] lie within (2n + 64) 2^-53 L of the exact windowed mean
// (per-step rounding of the chain <= 1.5 2^-53 L, of the 16-term sum <= 16 2^-53 L),
// and |std(u) - std(v)| <= max |u - v| plus rounding.  A comparison is decided only
// when u is farther than that bound from the threshold; otherwise (or on NaN) the
// state's flag is raised and outlier_exact_kernel, on the same stream, recomputes the
// mask with scipy's running sum and numpy's std order (ws[0:4] then only reports that
// the exact path ran).  So the mask equals the reference's bit for bit either way.
struct OutlierState {
    uint32_t flag;             // 1: a decision was ambiguous or a value NaN (ABI: bytes 0-3)
    uint32_t nbad;             // bad time bins (ABI: bytes 4-7)
    unsigned long long lbits;  // max |lc| as ordered bits (non-negative doubles)
    double sd;
    double up, down;           // 5 sd, -3 sd
    double margin_up, margin_down;
};

__device__ __forceinline__ int64_t reflect_small(int64_t i, int64_t n)
{
    // scipy 'reflect' for |offset| <= n (windows of 16 at the ends)
    if (i < 0) i = -i - 1;
    if (i >= n) i = 2 * n - 1 - i;
    return i < 0 ? 0 : (i >= n ? n - 1 : i);
}

// The certified decision, stated once for the launch-by-launch kernels and for
// outlier_fused_kernel: the window mean, the thresholds with their margins, the decision.

// u[i]: the mean of the reflected 16-sample window [i - 8, i + 7], summed left to right
__device__ __forceinline__ double outlier_window_mean(const double *__restrict__ lc, int64_t i, int64_t n)
{
    double s = 0.0;
    for (int j = -8; j < 8; ++j) s += lc[(i + j >= 0 && i + j < n) ? i + j : reflect_small(i + j, n)];
    return s / 16.0;
}

// Thresholds 5 sd and -3 sd, and how far from each a window mean u must lie for the
// comparison to be decided without the exact path (sd = std(u[::16]), L = max |lc|).
struct OutlierThresholds {
    double up, down;
    double margin_up, margin_down;
};

__device__ __forceinline__ OutlierThresholds outlier_thresholds(double sd, double L, int64_t n)
{
    const double E = ((double)(2 * n + 64) * 0x1p-53) * L + 1e-300;  // |u - v| bound
    const double Es = E + 1e-12 * sd;                                  // |std(u) - std(v)| bound
    OutlierThresholds th;
    th.up = 5.0 * sd;
    th.down = -3.0 * sd;
    th.margin_up = E + 5.0 * Es + 1e-15 * (L + 5.0 * sd);
    th.margin_down = E + 3.0 * Es + 1e-15 * (L + 3.0 * sd);
    return th;
}

// One lane's certified decision on the window mean v of time bin i (in: i < n; every lane
// of the wave calls): the mask, the flag (an ambiguous comparison raises it) and the bin
// appended to the bad list (one atomic per wave that has any, lanes in column order).
__device__ __forceinline__ void outlier_decide(bool in, double v, int64_t i, const OutlierThresholds &th,
                                               OutlierState *st, uint8_t *__restrict__ mask,
                                               int32_t *__restrict__ list)
{
    uint8_t b = 0;
    if (in) {
        const double du = v - th.up, dd = v - th.down;
        const bool amb = !(fabs(du) > th.margin_up) || !(fabs(dd) > th.margin_down);
        if (amb) atomicOr(&st->flag, 1u);
        b = (du > 0.0 || dd < 0.0) ? 1 : 0;
        mask[i] = b;
    }
    const uint64_t bal = __ballot(b != 0);
    if (!bal) return;
    const int lane = threadIdx.x & 63;
    uint32_t base = 0;
    if (lane == __ffsll((unsigned long long)bal) - 1) base = atomicAdd(&st->nbad, (uint32_t)__popcll(bal));
    base = __shfl(base, __ffsll((unsigned long long)bal) - 1, 64);
    if (b) list[base + __popcll(bal & ((uint64_t(1) << lane) - 1))] = (int32_t)i;
}

__global__ void __launch_bounds__(256)
outlier_window_kernel(const double *__restrict__ lc, int64_t n, double *__restrict__ u, double *__restrict__ u16,
                      OutlierState *st)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    double a = 0.0;
    bool nan = false;
    if (i < n) {
        const double w = outlier_window_mean(lc, i, n);
        u[i] = w;
        if ((i & 15) == 0) u16[i >> 4] = w;  // u[::16], compact for the std pass
        const double x = lc[i];
        nan = x != x;
        a = fabs(x);
    }
    // block max of |lc| (non-negative doubles order like their bit patterns)
    unsigned long long b = nan ? ~0ull : (unsigned long long)__double_as_longlong(a);
    for (int off = 32; off > 0; off >>= 1) {
        const unsigned long long o = __shfl_xor(b, off, 64);
        b = o > b ? o : b;
    }
    __shared__ unsigned long long wm[4];
    if ((threadIdx.x & 63) == 0) wm[threadIdx.x >> 6] = b;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long m = wm[0];
        for (int w = 1; w < 4; ++w) m = wm[w] > m ? wm[w] : m;
        if (m == ~0ull) atomicOr(&st->flag, 1u);
        else atomicMax(&st->lbits, m);
    }
}

// Block-wide sum (1024 threads): wave sums by xor shuffles, then the 16 wave totals.
__device__ __forceinline__ double block_sum_1024(double v, double *red)
{
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    const int t = threadIdx.x;
    __syncthreads();  // red is reused between calls
    if ((t & 63) == 0) red[t >> 6] = v;
    __syncthreads();
    double tot = 0.0;
#pragma unroll
    for (int w = 0; w < 16; ++w) tot += red[w];
    return tot;
}

// One workgroup: sd = std(u[::16]) (two passes over the compact copy), thresholds and
// certification margins.  (Any summation order: the margins bound the difference.)
__global__ void __launch_bounds__(1024) outlier_std_kernel(const double *__restrict__ u16, int64_t n, OutlierState *st)
{
    __shared__ double red[16];
    const int t = threadIdx.x;
    const int64_t m = (n + 15) / 16;
    double s = 0.0;
    for (int64_t k = t; k < m; k += 1024) s += u16[k];
    const double mean = block_sum_1024(s, red) / (double)m;
    s = 0.0;
    for (int64_t k = t; k < m; k += 1024) {
        const double d = u16[k] - mean;
        s += d * d;
    }
    const double ss = block_sum_1024(s, red);
    if (t == 0) {
        const double sd = sqrt(ss / (double)m);
        const double L = __longlong_as_double((long long)st->lbits);
        const OutlierThresholds th = outlier_thresholds(sd, L, n);
        st->sd = sd;
        st->up = th.up;
        st->down = th.down;
        st->margin_up = th.margin_up;
        st->margin_down = th.margin_down;
        if (sd != sd) st->flag |= 1u;
    }
}

// Certified decisions, one lane per time bin (outlier_decide; outlier_exact_kernel redoes
// the mask when the flag is raised), st->nbad entries in the list of the bad bins.
__global__ void __launch_bounds__(256)
outlier_mask_kernel(const double *__restrict__ u, int64_t n, OutlierState *st, uint8_t *__restrict__ mask,
                    int32_t *__restrict__ list)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const OutlierThresholds th = {st->up, st->down, st->margin_up, st->margin_down};
    outlier_decide(i < n, i < n ? u[i] : 0.0, i, th, st, mask, list);
}

// numpy add.reduce of a contiguous double vector (0 + pairwise sums of 8192-element
// blocks) by one lane; each block is staged in LDS by the whole workgroup first.
__device__ double reduce_sum_staged(const double *__restrict__ a, int64_t m, double *stage)
{
    double acc = 0.0;
    for (int64_t b = 0; b < m; b += kBlock) {
        const int len = (int)(m - b < kBlock ? m - b : kBlock);
        __syncthreads();
        for (int k = threadIdx.x; k < len; k += blockDim.x) stage[k] = a[b + k];
        __syncthreads();
        if (threadIdx.x == 0) acc += pairwise_lane<double, double, 0, 10>(stage, 0, len, 0.0, nullptr);
    }
    return acc;  // valid in lane 0
}

// The reference's own arithmetic for the rare case (the flag is set: a certified decision
// was ambiguous, or the light curve holds NaN / inf), on the device so that the common
// path needs no host round trip (round 4; the host used to rerun scipy).  One
// workgroup:
//  * scipy.ndimage.uniform_filter1d(lc, 16) (mode 'reflect', origin 0): the running sum
//    tmp = (sum of the first window) / 16, then tmp += (x[i + 7] - x[i - 9]) / 16 - the
//    differences of a chunk by all lanes into LDS (each is scipy's single rounding),
//    the chain by lane 0 (its order is the whole point);
//  * np.std(lc_rebin[::16]): numpy's add.reduce order for the mean and for the squared
//    deviations (a compact copy in tmp);
//  * bad = lc_rebin > 5 sd | lc_rebin < -3 sd (NaN compares false, as in numpy).
// Restatement checked bit for bit against scipy / numpy on CPU
// (tests/test_oracle.py::test_cut_outliers_exact_restatement).
__device__ void outlier_exact_body(const double *__restrict__ lc, int64_t n, OutlierState *st, double *__restrict__ v,
                                   double *__restrict__ tmp, uint8_t *__restrict__ mask, int32_t *__restrict__ list)
{
    __shared__ double stage[kBlock];
    __shared__ double thr[2];
    constexpr int kSize = 16, kOrig = kSize / 2;  // window [i - 8, i + 7]
    const int t = threadIdx.x;
    auto ext = [&](int64_t k) { return lc[reflect_small(k - kOrig, n)]; };  // scipy's extended line
    double s = 0.0;
    if (t == 0) {
        for (int j = 0; j < kSize; ++j) s += ext(j);
        s /= (double)kSize;
        v[0] = s;
    }
    for (int64_t c0 = 1; c0 < n; c0 += kBlock) {
        const int len = (int)(n - c0 < kBlock ? n - c0 : kBlock);
        __syncthreads();
        for (int k = t; k < len; k += 256) stage[k] = (ext(c0 + k + kSize - 1) - ext(c0 + k - 1)) / (double)kSize;
        __syncthreads();
        if (t == 0)
            for (int k = 0; k < len; ++k) {
                s += stage[k];
                v[c0 + k] = s;
            }
    }
    __syncthreads();
    __threadfence_block();
    const int64_t m = (n + 15) / 16;
    for (int64_t k = t; k < m; k += 256) tmp[k] = v[16 * k];
    __threadfence_block();
    const double mean = reduce_sum_staged(tmp, m, stage) / (double)m;  // lane 0
    __syncthreads();
    if (t == 0) thr[0] = mean;
    __syncthreads();
    for (int64_t k = t; k < m; k += 256) {
        const double d = tmp[k] - thr[0];
        tmp[k] = d * d;
    }
    __threadfence_block();
    const double ss = reduce_sum_staged(tmp, m, stage);
    __syncthreads();
    if (t == 0) {
        const double sd = sqrt(ss / (double)m);
        thr[0] = 5.0 * sd;
        thr[1] = -3.0 * sd;
        st->sd = sd;
        st->up = thr[0];
        st->down = thr[1];
        st->nbad = 0;
        st->flag = 1;
    }
    __syncthreads();
    __threadfence_block();
    for (int64_t i = t; i < n; i += 256) {
        const double x = v[i];
        const uint8_t b = (x > thr[0] || x < thr[1]) ? 1 : 0;
        mask[i] = b;
        if (b) list[atomicAdd(&st->nbad, 1u)] = (int32_t)i;  // any order: the zeroing is idempotent
    }
}

__global__ void __launch_bounds__(256)
outlier_exact_kernel(const double *__restrict__ lc, int64_t n, OutlierState *st, double *__restrict__ v,
                     double *__restrict__ tmp, uint8_t *__restrict__ mask, int32_t *__restrict__ list, int force)
{
    if (!force && st->flag == 0) return;
    outlier_exact_body(lc, n, st, v, tmp, mask, list);
}

// Zero the plane's bad columns (the final list): one workgroup per row, the list's
// entries over the lanes (entries of a wave are consecutive columns of a burst, so the
// stores coalesce).  Row-major: each row's 2 MiB page is touched by one workgroup instead
// of once per 64-column block of bad bins (15 us -> a few at C4).
__global__ void __launch_bounds__(256)
outlier_zero_kernel(const int32_t *__restrict__ list, const OutlierState *st, double *__restrict__ out,
                    int64_t nrows, int64_t ld)
{
    const uint32_t nbad = st->nbad;
    double *row = out + (int64_t)blockIdx.x * ld;
    for (uint32_t k = threadIdx.x; k < nbad; k += 256) row[list[k]] = 0.0;
}

// ---------------------------------------------------------------- median
// np.median of a float64 series on the device (clean.py:80), so the factor pass
// does not wait on a host round trip.  Radix select over order-preserving 64-bit
// keys: six digit passes (11,11,11,11,11,9 bits, high to low) narrow the key
// prefixes of the two order statistics numpy averages (k = n/2-1 and n/2 for even
// n, n/2 twice for odd n).  Each pass is ONE histogram kernel (LDS bins, one global
// atomic add per non-empty bin and workgroup): its workgroups first select the
// previous pass's bin from that pass's global histogram themselves (every workgroup
// computes the same prefix; workgroup 0 records it), and clear the buffer the next
// pass will fill (three rotating buffers).  A one-workgroup final kernel selects the
// last digit.  The result is numpy's mean of the two values, add.reduce order:
// (0 + ((0 + a) + b)) / 2; any NaN gives NaN.  8 launches (was 14).
constexpr int kMedBitsMax = 11;
constexpr int kMedBins = 1 << kMedBitsMax;
constexpr int kMedPasses = 6;
constexpr int kMedBufs = 3;

struct MedState {
    uint64_t prefix[kMedPasses + 1][2];  // key prefix of each target before pass p
    int64_t k[kMedPasses + 1][2];        // its rank among the keys with that prefix
    uint32_t nan;
    uint32_t pad;
};

__host__ __device__ constexpr int med_shift(int p) { return 64 - kMedBitsMax * (p + 1) > 0 ? 64 - kMedBitsMax * (p + 1) : 0; }
__host__ __device__ constexpr int med_bits(int p) { return 64 - kMedBitsMax * p - med_shift(p); }

__device__ __forceinline__ uint64_t order_key(double d)
{
    const uint64_t u = static_cast<uint64_t>(__double_as_longlong(d));
    return (u >> 63) ? ~u : (u | (uint64_t(1) << 63));
}

__device__ __forceinline__ double key_value(uint64_t k)
{
    const uint64_t u = (k >> 63) ? (k & ~(uint64_t(1) << 63)) : ~k;
    return __longlong_as_double(static_cast<long long>(u));
}

__global__ void median_init_kernel(MedState *st, uint32_t *hist, int64_t n)
{
    const int t = threadIdx.x;
    if (t == 0) {
        st->prefix[0][0] = st->prefix[0][1] = 0;
        st->k[0][0] = (n % 2 == 0) ? n / 2 - 1 : n / 2;
        st->k[0][1] = n / 2;
        st->nan = 0;
    }
    for (int i = t; i < kMedBufs * 2 * kMedBins; i += blockDim.x) hist[i] = 0;
}

// Block-wide selection (256 threads): the bin of ``hj`` holding rank k; thread t owns
// bins [8t, 8t+8).  Returns (bin, rank inside the bin) to every thread.
__device__ void med_select_block(const uint32_t *hj, int64_t k, uint32_t *scan, int64_t *res, int &bin,
                                 int64_t &rem)
{
    const int t = threadIdx.x;
    uint32_t c[8], sum = 0;
#pragma unroll
    for (int b = 0; b < 8; ++b) {
        c[b] = hj[8 * t + b];
        sum += c[b];
    }
    scan[t] = sum;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        const uint32_t v = t >= off ? scan[t - off] : 0;
        __syncthreads();
        scan[t] += v;
        __syncthreads();
    }
    const int64_t before = (int64_t)scan[t] - sum;
    if (k >= before && k < before + (int64_t)sum) {
        int64_t r = k - before;
        int b = 0;
        while (r >= (int64_t)c[b]) r -= c[b++];
        res[0] = 8 * t + b;
        res[1] = r;
    }
    __syncthreads();
    bin = (int)res[0];
    rem = res[1];
    __syncthreads();
}

// Prefix and rank of both targets before pass ``pass`` (pass >= 1), from the previous
// pass's histogram.
__device__ void med_prefix(const MedState *st, const uint32_t *hist, int pass, uint32_t *scan, int64_t *res,
                           uint64_t (&pfx)[2], int64_t (&kk)[2])
{
    const uint32_t *hp = hist + (size_t)((pass - 1) % kMedBufs) * 2 * kMedBins;
    for (int j = 0; j < 2; ++j) {
        int bin;
        int64_t rem;
        med_select_block(hp + j * kMedBins, st->k[pass - 1][j], scan, res, bin, rem);
        pfx[j] = st->prefix[pass - 1][j] | ((uint64_t)bin << med_shift(pass - 1));
        kk[j] = rem;
    }
}

__global__ void __launch_bounds__(256)
median_hist_kernel(const double *__restrict__ x, int64_t n, MedState *st, uint32_t *hist, int pass)
{
    __shared__ uint32_t h[2][kMedBins];
    __shared__ uint32_t scan[256];
    __shared__ int64_t res[2];
    uint64_t pfx[2] = {0, 0};
    int64_t kk[2] = {st->k[0][0], st->k[0][1]};
    if (pass > 0) {
        med_prefix(st, hist, pass, scan, res, pfx, kk);
        if (blockIdx.x == 0 && threadIdx.x == 0) {
            st->prefix[pass][0] = pfx[0];
            st->prefix[pass][1] = pfx[1];
            st->k[pass][0] = kk[0];
            st->k[pass][1] = kk[1];
        }
    }
    // clear the buffer the NEXT pass accumulates into (nobody reads it during this pass)
    uint32_t *nxt = hist + (size_t)((pass + 1) % kMedBufs) * 2 * kMedBins;
    for (int i = blockIdx.x * 256 + threadIdx.x; i < 2 * kMedBins; i += gridDim.x * 256) nxt[i] = 0;
    for (int i = threadIdx.x; i < 2 * kMedBins; i += 256) (&h[0][0])[i] = 0;
    __syncthreads();
    const int shift = med_shift(pass), bits = med_bits(pass);
    const uint64_t dmask = (uint64_t(1) << bits) - 1;
    const int hs = shift + bits;  // bits above the digit must match the prefix
    uint32_t nans = 0;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
        const double d = x[i];
        if (d != d) {
            ++nans;
            continue;
        }
        const uint64_t k = order_key(d);
        const uint32_t dig = (uint32_t)((k >> shift) & dmask);
        if (hs >= 64 || (k >> hs) == (pfx[0] >> hs)) atomicAdd(&h[0][dig], 1u);
        if (hs >= 64 || (k >> hs) == (pfx[1] >> hs)) atomicAdd(&h[1][dig], 1u);
    }
    if (pass == 0 && nans) atomicAdd(&st->nan, nans);
    __syncthreads();
    uint32_t *cur = hist + (size_t)(pass % kMedBufs) * 2 * kMedBins;
    for (int i = threadIdx.x; i < 2 * kMedBins; i += 256) {
        const uint32_t c = (&h[0][0])[i];
        if (c) atomicAdd(&cur[i], c);
    }
}

// One workgroup: the last digit, then numpy's mean of the two order statistics.
__global__ void __launch_bounds__(256) median_final_kernel(MedState *st, const uint32_t *hist, int64_t n,
                                                           double *out)
{
    __shared__ uint32_t scan[256];
    __shared__ int64_t res[2];
    uint64_t pfx[2];
    int64_t kk[2];
    med_prefix(st, hist, kMedPasses, scan, res, pfx, kk);
    if (threadIdx.x != 0) return;
    if (st->nan) {
        out[0] = __longlong_as_double(0x7ff8000000000000ll);
        return;
    }
    const double a = key_value(pfx[0]);
    if (n % 2 == 0) {
        const double b = key_value(pfx[1]);
        out[0] = (0.0 + ((0.0 + a) + b)) / 2.0;
    } else {
        out[0] = (0.0 + (0.0 + a)) / 1.0;
    }
}

// ---------------------------------------------------------------- grid barrier
// A monotonic arrival counter for the one-launch cut_outliers (every wave's vmcnt(0), the
// workgroup barrier, lane 0's agent release, the arrival, a relaxed poll with s_sleep, the
// agent acquire - MI355X_MICROARCH.md, inter-workgroup visibility).  Round 5 also tried it
// for renormalize_data's light-curve chain (Gaussian + six radix-select passes + ratio in one
// launch, smoothed values kept in LDS): 103 us with this barrier, 123 us with the fenced form
// of every pass, against 79 us for the ten launches (scripts/bench_lc.py, n = 2^18, sigma
// 101): at 256 workgroups a barrier costs ~7 us, a kernel boundary ~1.5 us, so the chain
// stays launch-by-launch (pu_lc_factor).
// arrive: the launch's arrival counter (zero at launch); target: workgroups x barriers so far.
__device__ __forceinline__ void lc_grid_barrier(unsigned *arrive, unsigned target)
{
    asm volatile("s_waitcnt vmcnt(0)" : : : "memory");  // this wave's atomics done
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        __hip_atomic_fetch_add(arrive, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        while (__hip_atomic_load(arrive, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < target)
            __builtin_amdgcn_s_sleep(2);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
    }
    __syncthreads();
}

// ---------------------------------------------------------------- cut_outliers, one launch
// pu_cut_outliers' window means, std, certified decisions, exact fallback and column zeroing
// (clean.py:93-105) in ONE launch (round 5; until round 4: a state fill + five kernels).
// Phases separated by grid barriers (lc_grid_barrier; the counters sit in the workspace
// head cleared by the call's one 128-byte fill):
//   1. each workgroup: u = the 16-window means of its segments (kept in LDS and stored for
//      the exact path), the partial sum of u[::16], max |lc| and the NaN flag;
//   2. mean of u[::16] -> the partial sum of squared deviations;
//   3. sd, thresholds and certification margins (every workgroup computes the same values
//      from the same totals) -> the mask, the ambiguity flag, the bad-bin list;
//   4. only when the flag is set: workgroup 0 redoes the mask with the reference's own
//      arithmetic (outlier_exact_body), the others wait;
//   5. the bad columns of the plane zeroed, rows dealt over the workgroups.
// The sums in phases 1-2 are float64 atomics (any order: the certification margins bound
// the difference from scipy's chain, as in outlier_std_kernel).
struct OutlierBar {
    unsigned arrive, leave;
    double sum_u16, sum_sq;
};

__global__ void __launch_bounds__(256)
outlier_fused_kernel(const double *__restrict__ lc, int64_t n, OutlierState *st, OutlierBar *ob,
                     double *__restrict__ u, double *__restrict__ u16, uint8_t *__restrict__ mask,
                     int32_t *__restrict__ list, double *__restrict__ out, int64_t nrows, int64_t ld_out, int segs)
{
    extern __shared__ __attribute__((aligned(16))) double usm[];  // [segs][1024] window means
    __shared__ double red[4];
    __shared__ unsigned long long wm[4];
    const int t = threadIdx.x;
    const unsigned G = gridDim.x;
    auto block_sum = [&](double v) {
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        __syncthreads();
        if ((t & 63) == 0) red[t >> 6] = v;
        __syncthreads();
        return (red[0] + red[1]) + (red[2] + red[3]);
    };
    // 1. window means, sum of u[::16], max |lc|, NaN
    double s16 = 0.0;
    unsigned long long lb = 0;
    bool nan = false;
    for (int sg = 0; sg < segs; ++sg) {
        const int64_t i0 = ((int64_t)blockIdx.x + (int64_t)G * sg) * 1024;
        if (i0 >= n) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + q * 256 + t;
            double w = 0.0;
            if (i < n) {
                w = outlier_window_mean(lc, i, n);
                u[i] = w;
                if ((i & 15) == 0) {
                    u16[i >> 4] = w;
                    s16 += w;
                }
                const double x = lc[i];
                nan = nan || x != x;
                const unsigned long long ab = (unsigned long long)__double_as_longlong(fabs(x));
                lb = ab > lb ? ab : lb;
            }
            usm[sg * 1024 + q * 256 + t] = w;
        }
    }
    {
        const double tot = block_sum(s16);
        unsigned long long b = nan ? ~0ull : lb;
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned long long o = __shfl_xor(b, off, 64);
            b = o > b ? o : b;
        }
        if ((t & 63) == 0) wm[t >> 6] = b;
        __syncthreads();
        if (t == 0) {
            unsigned long long m = wm[0];
            for (int w = 1; w < 4; ++w) m = wm[w] > m ? wm[w] : m;
            if (m == ~0ull) atomicOr(&st->flag, 1u);
            else atomicMax(&st->lbits, m);
            atomicAdd(&ob->sum_u16, tot);
        }
    }
    lc_grid_barrier(&ob->arrive, G);
    // 2. squared deviations of u[::16] from their mean
    const int64_t m = (n + 15) / 16;
    const double mean = __hip_atomic_load(&ob->sum_u16, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) / (double)m;
    double ssq = 0.0;
    for (int sg = 0; sg < segs; ++sg) {
        const int64_t i0 = ((int64_t)blockIdx.x + (int64_t)G * sg) * 1024;
        if (i0 >= n) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + q * 256 + t;
            if (i < n && (i & 15) == 0) {
                const double d = usm[sg * 1024 + q * 256 + t] - mean;
                ssq += d * d;
            }
        }
    }
    {
        const double tot = block_sum(ssq);
        if (t == 0) atomicAdd(&ob->sum_sq, tot);
    }
    lc_grid_barrier(&ob->arrive, 2 * G);
    // 3. thresholds, margins, decisions, the bad-bin list
    const double ss = __hip_atomic_load(&ob->sum_sq, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const double sd = sqrt(ss / (double)m);
    const double L = __longlong_as_double(
        (long long)__hip_atomic_load(&st->lbits, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    const OutlierThresholds th = outlier_thresholds(sd, L, n);
    if (blockIdx.x == 0 && t == 0) {
        st->sd = sd;
        st->up = th.up;
        st->down = th.down;
        st->margin_up = th.margin_up;
        st->margin_down = th.margin_down;
        if (sd != sd) atomicOr(&st->flag, 1u);
    }
    for (int sg = 0; sg < segs; ++sg) {
        const int64_t i0 = ((int64_t)blockIdx.x + (int64_t)G * sg) * 1024;
        if (i0 >= n) break;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t i = i0 + q * 256 + t;
            outlier_decide(i < n, usm[sg * 1024 + q * 256 + t], i, th, st, mask, list);
        }
    }
    lc_grid_barrier(&ob->arrive, 3 * G);
    // 4. the rare exact path (uniform: every workgroup reads the same flag)
    if (__hip_atomic_load(&st->flag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0) {
        if (blockIdx.x == 0) outlier_exact_body(lc, n, st, u, u16, mask, list);
        lc_grid_barrier(&ob->arrive, 4 * G);
    }
    // 5. zero the bad columns, rows over the workgroups
    const uint32_t nbad = __hip_atomic_load(&st->nbad, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (int64_t r = blockIdx.x; r < nrows; r += G) {
        double *row = out + r * ld_out;
        for (uint32_t k = t; k < nbad; k += 256) row[list[k]] = 0.0;
    }
}

}  // namespace

extern "C" {

int pu_gaussian_filter1d(const double *x, int64_t n, const double *w, int64_t r, double *out, void *stream)
{
    PU_REQUIRE(x && w && out && n > 0 && r >= 0, "pu_gaussian_filter1d: bad arguments");
    if (r <= kGaussMaxR) {
        constexpr int T = kGaussQuadThreads;  // 4 outputs per thread
        const size_t lds = (size_t)(((r + 2) & ~int64_t(1)) + 4 * T + 2 * r + 2 * kGaussPad) * sizeof(double);
        return pu::launch("gauss_quad_kernel", gauss_quad_kernel, dim3(blocks_for(n, 4 * T)), dim3(T), lds,
                          pu::as_stream(stream), x, n, w, (int)r, out);
    }
    return pu::launch("gauss_kernel", gauss_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, pu::as_stream(stream), x, n, w,
                      r, out);
}

int pu_ratio(double num, const double *x, int64_t n, double *out, void *stream)
{
    PU_REQUIRE(x && out && n > 0, "pu_ratio: bad arguments");
    return pu::launch("ratio_kernel", ratio_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, pu::as_stream(stream), num, x,
                      n, out);
}

size_t pu_cut_outliers_workspace_bytes(int64_t n)
{
    const size_t m = (size_t)(n > 0 ? n : 0);
    return 256 + (m + (m + 15) / 16) * sizeof(double) + m * sizeof(int32_t);  // state | window means | every 16th | bad list
}

namespace {
// CUs a launch on stream s may use: the current device's, or the stream's CU mask's when it
// has one (pu_stream_create_cu_masked); 0 if they cannot be counted.
int usable_cus(hipStream_t s)
{
    int dev = 0, cus = 0;
    if (hipGetDevice(&dev) != hipSuccess) return 0;
    static std::atomic<int> ncu[64];
    cus = dev < 64 ? ncu[dev].load() : 0;
    if (cus <= 0) {
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess) return 0;
        if (dev < 64) ncu[dev].store(cus);
    }
    if (s) {
        uint32_t m[32] = {};
        if (hipExtStreamGetCUMask(s, 32, m) == hipSuccess) {
            int c = 0;
            for (uint32_t w : m) c += __builtin_popcount(w);
            if (c > 0 && c < cus) cus = c;
        } else {
            (void)hipGetLastError();
        }
    }
    return cus;
}

int cut_outliers(const double *lc, int64_t n, double *out, int64_t nrows, int64_t ld_out, uint8_t *mask, void *ws,
                 size_t ws_bytes, void *stream, bool exact_only)
{
    PU_REQUIRE(lc && out && mask && n >= 64 && nrows > 0 && ld_out >= n, "pu_cut_outliers: bad arguments");
    if (int rc = pu::check_workspace("pu_cut_outliers", ws, ws_bytes, pu_cut_outliers_workspace_bytes(n), 8)) return rc;
    hipStream_t s = pu::as_stream(stream);
    OutlierState *st = reinterpret_cast<OutlierState *>(ws);
    double *u = reinterpret_cast<double *>(reinterpret_cast<char *>(ws) + 256);
    double *u16 = u + n;
    int32_t *list = reinterpret_cast<int32_t *>(u16 + (n + 15) / 16);
    PU_REQUIRE(nrows < (int64_t(1) << 31), "pu_cut_outliers: too many rows");
    // one 16-byte-multiple fill (the runtime splits a 56-byte memset into two kernels)
    static_assert(sizeof(OutlierState) <= 64, "OutlierState fits the cleared 64 bytes");
    static_assert(sizeof(OutlierBar) <= 64, "OutlierBar fits the cleared 64 bytes after the state");
    bool resident = false;
    if (!exact_only) {
        // one launch with grid barriers (outlier_fused_kernel): at most one workgroup per two
        // CUs the stream may use, each with <= 64 KB of window means in LDS, and never more
        // than the occupancy calculator says can be resident on them together - so every
        // workgroup of the grid is resident and the spinning barrier cannot wait on one that
        // never starts.  Counted per call on the current device and the stream's CU mask (a
        // CU-masked stream, pu_stream_create_cu_masked, sees only its CUs); a grid that would
        // not be resident takes the launch-by-launch path below.
        const int64_t nseg = (n + 1023) / 1024;
        const int cus = usable_cus(s);
        const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(nseg, std::max(1, cus / 2)));
        const int segs = (int)((nseg + grid - 1) / grid);
        if (cus > 0 && segs <= 8 && nrows < (int64_t(1) << 31)) {
            int dev = 0;
            PU_TRY_HIP(hipGetDevice(&dev));
            static std::atomic<uint64_t> attr_set{0};  // per device: 64 KB static (the exact
                                                      // path's staging) + the window means
            if (dev < 64 && !(attr_set.load() >> dev & 1)) {
                if (int rc = pu::raise_lds(outlier_fused_kernel, 8 * 1024 * sizeof(double))) return rc;
                attr_set.fetch_or(uint64_t(1) << dev);
            }
            // resident workgroups per CU at this LDS size (cached per device and size)
            static std::atomic<int> occ[64][9];
            int per_cu = dev < 64 ? occ[dev][segs].load() : 0;
            if (per_cu <= 0) {
                PU_TRY_HIP(hipOccupancyMaxActiveBlocksPerMultiprocessor(
                    &per_cu, reinterpret_cast<const void *>(outlier_fused_kernel), 256, (size_t)segs * 1024 * sizeof(double)));
                if (dev < 64) occ[dev][segs].store(per_cu);
            }
            resident = (int64_t)per_cu * cus >= grid;
        }
        if (resident) {
            PU_TRY_HIP(hipMemsetAsync(st, 0, 128, s));
            OutlierBar *ob = reinterpret_cast<OutlierBar *>(reinterpret_cast<char *>(ws) + 64);
            // (at most the 64 KiB raised above: pu::launch raises nothing here)
            return pu::launch("outlier_fused_kernel", outlier_fused_kernel, dim3(grid), dim3(256),
                              (size_t)segs * 1024 * sizeof(double), s, lc, n, st, ob, u, u16, mask, list, out, nrows, ld_out,
                              segs);
        }
    }
    PU_TRY_HIP(hipMemsetAsync(st, 0, 64, s));
    if (!exact_only) {
        hipLaunchKernelGGL(outlier_window_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, lc, n, u, u16, st);
        hipLaunchKernelGGL(outlier_std_kernel, dim3(1), dim3(1024), 0, s, u16, n, st);
        hipLaunchKernelGGL(outlier_mask_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, u, n, st, mask, list);
    }
    // returns at once unless the flag is set (or exact_only)
    hipLaunchKernelGGL(outlier_exact_kernel, dim3(1), dim3(256), 0, s, lc, n, st, u, u16, mask, list,
                       exact_only ? 1 : 0);
    hipLaunchKernelGGL(outlier_zero_kernel, dim3((unsigned)nrows), dim3(256), 0, s, list, st, out, nrows, ld_out);
    return pu::launch_check("outlier kernels");
}
}  // namespace

int pu_cut_outliers(const double *lc, int64_t n, double *out, int64_t nrows, int64_t ld_out, uint8_t *mask,
                    void *ws, size_t ws_bytes, void *stream)
{
    return cut_outliers(lc, n, out, nrows, ld_out, mask, ws, ws_bytes, stream, false);
}

int pu_cut_outliers_exact(const double *lc, int64_t n, double *out, int64_t nrows, int64_t ld_out, uint8_t *mask,
                          void *ws, size_t ws_bytes, void *stream)
{
    return cut_outliers(lc, n, out, nrows, ld_out, mask, ws, ws_bytes, stream, true);
}

size_t pu_median_workspace_bytes(void) { return sizeof(MedState) + kMedBufs * 2 * kMedBins * sizeof(uint32_t); }

int pu_median(const double *x, int64_t n, double *out, void *ws, size_t ws_bytes, void *stream)
{
    PU_REQUIRE(x && out && n > 0, "pu_median: bad arguments");
    if (int rc = pu::check_workspace("pu_median", ws, ws_bytes, pu_median_workspace_bytes(), 8)) return rc;
    hipStream_t s = pu::as_stream(stream);
    MedState *st = reinterpret_cast<MedState *>(ws);
    uint32_t *hist = reinterpret_cast<uint32_t *>(st + 1);
    hipLaunchKernelGGL(median_init_kernel, dim3(1), dim3(256), 0, s, st, hist, n);
    // a few elements per thread and at most 256 workgroups per pass: fewer workgroups to
    // flush LDS bins to the global histogram
    const unsigned grid = std::min<int64_t>(256, std::max<int64_t>(1, (n + 1023) / 1024));
    for (int p = 0; p < kMedPasses; ++p)
        hipLaunchKernelGGL(median_hist_kernel, dim3(grid), dim3(256), 0, s, x, n, st, hist, p);
    hipLaunchKernelGGL(median_final_kernel, dim3(1), dim3(256), 0, s, st, hist, n, out);
    return pu::launch_check("median_kernels");
}

int pu_ratio_dev(const double *numerator, const double *x, int64_t n, double *out, void *stream)
{
    PU_REQUIRE(numerator && x && out && n > 0, "pu_ratio_dev: bad arguments");
    return pu::launch("ratio_dev_kernel", ratio_dev_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, pu::as_stream(stream),
                      numerator, x, n, out);
}

namespace {
// pu_lc_factor's workspace: the smoothed series, pu_median's workspace and the median
struct LcFactorWs {
    double *smooth, *med;
    void *mws;
    size_t bytes;
};

LcFactorWs lc_factor_carve(pu::Carver c, int64_t n)
{
    LcFactorWs w;
    w.smooth = c.take<double>((size_t)std::max<int64_t>(n, 0) * 8);
    w.mws = c.take<char>(pu_median_workspace_bytes());
    w.med = c.take<double>(64, 8);
    w.bytes = c.used();
    return w;
}
}  // namespace

size_t pu_lc_factor_workspace_bytes(int64_t n) { return lc_factor_carve(pu::Carver(), n).bytes; }

int pu_lc_factor(const double *lc, int64_t n, const double *w, int64_t r, double *factor, double *median_out, void *ws,
                 size_t ws_bytes, void *stream)
{
    PU_REQUIRE(lc && w && factor && n > 0 && r >= 0, "pu_lc_factor: bad arguments");
    const LcFactorWs p = lc_factor_carve(pu::Carver(ws), n);
    if (int rc = pu::check_workspace("pu_lc_factor", ws, ws_bytes, p.bytes, 256)) return rc;
    // Gaussian, median, ratio, launch by launch (a one-launch form with grid barriers measured
    // slower: see the grid-barrier note above)
    double *med = median_out ? median_out : p.med;
    int rc = pu_gaussian_filter1d(lc, n, w, r, p.smooth, stream);
    if (!rc) rc = pu_median(p.smooth, n, med, p.mws, pu_median_workspace_bytes(), stream);
    if (!rc) rc = pu_ratio_dev(med, p.smooth, n, factor, stream);
    return rc;
}

}  // extern "C"
