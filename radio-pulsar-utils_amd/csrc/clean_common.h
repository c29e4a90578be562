// What more than one of the RFI-cleaning units (clean_rows.hip, clean_cols.hip,
// clean_lc.hip, clean_masks.hip) uses: numpy's pairwise sum by one lane, the vector
// loads and the in-order row walk of the column passes, scipy's 'reflect' index and the
// host helpers that pick a launch shape.
//
// The cleaning units replace the 2-D array passes of the reference cleaning path
// (pulsarutils/clean.py:58-111, 114-133) with bit-exact HIP kernels.  The masks the
// reference derives are threshold comparisons on these reductions, so every sum is
// reproduced in numpy's exact order (SURVEY.md §8 a-R; oracle/numpy_order.py):
//
//   add.reduce over a contiguous row  = 0 + pw(block_0) + pw(block_1) + ...,
//       blocks of 8192 elements, pw = numpy pairwise_sum (8 strided accumulators
//       over 128-element leaves, halving splits at n/2 - (n/2)%8)
//   mean(0) / zero-DM light curve      = sequential over rows
//
// Everything is compiled with -ffp-contract=off: a fused multiply-add would change
// the rounding of x*f - mu and of the squared deviations.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "pu_common.h"

namespace {

constexpr int kBlock = 8192;   // numpy ufunc buffer size
constexpr int kLeaf = 128;     // numpy PW_BLOCKSIZE

template <typename Tin, typename Ta, int MODE>
__device__ __forceinline__ Ta load_val(const Tin *row, int64_t t, Ta center, const double *scale)
{
    if constexpr (MODE == 0) {
        return static_cast<Ta>(row[t]);
    } else if constexpr (MODE == 1) {
        const Ta d = static_cast<Ta>(row[t]) - center;
        return d * d;
    } else if constexpr (MODE == 4) {
        const Ta v = static_cast<Ta>(row[t]);
        return v * v;
    } else {
        return static_cast<Ta>(static_cast<double>(row[t]) * scale[t]);
    }
}

// numpy pairwise_sum over [off, off+n) of a row, one lane.  DEPTH bounds the
// recursion at compile time (n <= 8192 needs < 10 levels).
template <typename Tin, typename Ta, int MODE, int DEPTH>
__device__ Ta pairwise_lane(const Tin *row, int64_t off, int64_t n, Ta center, const double *scale)
{
    if (n < 8) {
        Ta r = Ta(0);
        for (int64_t i = 0; i < n; ++i) r += load_val<Tin, Ta, MODE>(row, off + i, center, scale);
        return r;
    }
    if constexpr (DEPTH > 0) {
        if (n > kLeaf) {
            int64_t n2 = n / 2;
            n2 -= n2 % 8;
            const Ta l = pairwise_lane<Tin, Ta, MODE, DEPTH - 1>(row, off, n2, center, scale);
            const Ta r = pairwise_lane<Tin, Ta, MODE, DEPTH - 1>(row, off + n2, n - n2, center, scale);
            return l + r;
        }
    }
    Ta r[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) r[j] = load_val<Tin, Ta, MODE>(row, off + j, center, scale);
    int64_t i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int j = 0; j < 8; ++j) r[j] += load_val<Tin, Ta, MODE>(row, off + i + j, center, scale);
    Ta res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res += load_val<Tin, Ta, MODE>(row, off + i, center, scale);
    return res;
}

// V consecutive elements moved by one global load / store instruction.
template <typename T, int V>
struct alignas(sizeof(T) * V) Vec {
    T v[V];
};

template <typename T, int V>
__device__ __forceinline__ Vec<T, V> load_vec(const T *p)
{
    return *reinterpret_cast<const Vec<T, V> *>(p);
}

// Column passes: a lane owns V adjacent columns and walks the rows in order (the
// numpy order of mean(0) and of the row loop of clean.py:81-94).  Per-row scalars
// (skip flag, channel mean) are staged in LDS per chunk of kRowChunk rows.
constexpr int kRowChunk = 4096;
constexpr int kBatchBytes = 128;  // per lane and register buffer: U = kBatchBytes / (V * elem)
constexpr int kMaxBatchRows = 32;

// Rows [0, rn) of a column strip, in order: batches of U rows alternate between two
// register buffers, the next batch's loads issued before the current batch is
// consumed (no register copies, so a wait never covers the batch in flight).
template <typename Tin, int V, typename Body, int BB = kBatchBytes>
__device__ __forceinline__ void walk_rows(const Tin *p, int64_t ld, int rn, Body &&body)
{
    constexpr int U = std::max(1, std::min(kMaxBatchRows, BB / (V * (int)sizeof(Tin))));
    Vec<Tin, V> a[U], b[U];
    auto load = [&](Vec<Tin, V>(&dst)[U], int i0) {
        if (i0 + U <= rn) {
#pragma unroll
            for (int k = 0; k < U; ++k) dst[k] = load_vec<Tin, V>(p + (int64_t)(i0 + k) * ld);
        } else {
#pragma unroll
            for (int k = 0; k < U; ++k)
                if (i0 + k < rn) dst[k] = load_vec<Tin, V>(p + (int64_t)(i0 + k) * ld);
        }
    };
    auto run = [&](Vec<Tin, V>(&src)[U], int i0) {
        if (i0 + U <= rn) {
#pragma unroll
            for (int k = 0; k < U; ++k) body(i0 + k, src[k]);
        } else {
#pragma unroll
            for (int k = 0; k < U; ++k)
                if (i0 + k < rn) body(i0 + k, src[k]);
        }
    };
    load(a, 0);
    for (int i0 = 0; i0 < rn; i0 += 2 * U) {
        if (i0 + U < rn) load(b, i0 + U);
        run(a, i0);
        if (i0 + 2 * U < rn) load(a, i0 + 2 * U);
        if (i0 + U < rn) run(b, i0 + U);
    }
}

__device__ __forceinline__ int64_t reflect_index(int64_t i, int64_t n)
{
    // scipy 'reflect' (d c b a | a b c d | d c b a): period 2n, half-sample symmetric
    const int64_t p = 2 * n;
    int64_t m = i % p;
    if (m < 0) m += p;
    return m >= n ? p - 1 - m : m;
}

inline unsigned blocks_for(int64_t n, int threads) { return (unsigned)((n + threads - 1) / threads); }

// Widest V in {vmax, .., 2} with every row start of p (stride ld elements) aligned
// to V elements; 1 otherwise.
template <typename T>
int pick_vec(const void *p, int64_t ld, int vmax)
{
    for (int v = vmax; v > 1; v >>= 1)
        if (reinterpret_cast<uintptr_t>(p) % (v * sizeof(T)) == 0 && ld % v == 0) return v;
    return 1;
}

// Columns [0, n - n%V) with V-wide lanes (v <= VMAX: wider lanes are not instantiated),
// the rest with scalar lanes.
template <int VMAX, typename Launch>
int column_launches(int v, int64_t n, Launch &&launch)
{
    const int64_t nv = n - n % v;
    if (nv > 0) {
        if constexpr (VMAX >= 4)
            if (v == 4) launch(std::integral_constant<int, 4>{}, 0, nv);
        if constexpr (VMAX >= 2)
            if (v == 2) launch(std::integral_constant<int, 2>{}, 0, nv);
        if (v == 1) launch(std::integral_constant<int, 1>{}, 0, nv);
    }
    if (n > nv) launch(std::integral_constant<int, 1>{}, nv, n - nv);
    return PU_OK;
}

}  // namespace
