// Running-median detrending for gfx950: a sliding-window median (pu_running_median) and the
// subtraction of the baseline interpolated between block medians (pu_detrend_apply).  The
// definitions are in include/pulsarutils_hip.h ("running-median detrending"); tests/detrend_oracle.py
// restates them in numpy, bit for bit.
//
// running_median_kernel: a workgroup of 256 threads makes RMED_TILE = 1024 consecutive outputs of
// one row.  It stages the tile plus the 2h halo (indices clamped to the row) in LDS as unsigned
// keys whose integer order is the order of the values (-0 before +0; every NaN becomes the largest
// key), then each thread selects its four outputs (tile offsets tid, tid + 256 ..) by a radix
// descent: for every key bit from the top, count the window's keys that continue the prefix found
// so far with a 0 bit; the wanted rank is among them or, lowered by their count, among the others.
// That is `bits` passes over the window, w LDS reads each, branch-free, and every read has the 64
// lanes of a wave on 64 consecutive keys (lane l reads key o + k + l): no bank conflict, no
// divergence, no sorting network whose size depends on w.  LDS: (1024 + 2h) keys, at most 3070:
// 12 KiB (float32) or 24 KiB (float64), so several workgroups share a CU.
//
// detrend_apply_kernel: one read and one write per sample, 16 bytes per lane where the pointers
// and strides allow; the medians (nblk per row, read twice per sample) come from the caches.
#include <hip/hip_runtime.h>

#include "pu_common.h"

namespace {

constexpr int RMED_TILE = 1024, RMED_THREADS = 256, RMED_PER_THREAD = RMED_TILE / RMED_THREADS;
constexpr int RMED_MAX_W = 2047;
constexpr int RMED_NINFO = 3;

template <typename T> struct rmed_key;
template <> struct rmed_key<float> {
    using type = uint32_t;
    static constexpr uint32_t quiet_nan = 0x7fc00000u;
};
template <> struct rmed_key<double> {
    using type = uint64_t;
    static constexpr uint64_t quiet_nan = 0x7ff8000000000000ull;
};

// The bits of v as a key: negative values have all bits flipped, the others the sign bit set, so
// keys compare as the values do with -0 below +0; a NaN of either sign is the all-ones key, which
// no other value has (it would be the positive NaN of largest payload).
template <typename T>
__device__ __forceinline__ typename rmed_key<T>::type to_key(T v)
{
    using K = typename rmed_key<T>::type;
    constexpr int B = 8 * sizeof(K);
    K b;
    __builtin_memcpy(&b, &v, sizeof(K));
    const K k = (b >> (B - 1)) ? ~b : (b | (K(1) << (B - 1)));
    return v != v ? ~K(0) : k;
}

template <typename T>
__device__ __forceinline__ T from_key(typename rmed_key<T>::type k)
{
    using K = typename rmed_key<T>::type;
    constexpr int B = 8 * sizeof(K);
    const K b = (k >> (B - 1)) ? (k ^ (K(1) << (B - 1))) : ~k;
    T v;
    __builtin_memcpy(&v, &b, sizeof(K));
    return v;
}

template <typename T>
__global__ void __launch_bounds__(RMED_THREADS) running_median_kernel(const T *__restrict__ x, int64_t n, int64_t ld, int h,
                                                                      int64_t ntiles, T *__restrict__ out, int64_t ld_out)
{
    using K = typename rmed_key<T>::type;
    constexpr int B = 8 * sizeof(K);
    extern __shared__ __attribute__((aligned(16))) unsigned char rmed_lds[];
    K *keys = reinterpret_cast<K *>(rmed_lds);
    const int64_t bid = blockIdx.x, r = bid / ntiles, t0 = (bid % ntiles) * RMED_TILE;
    const int tid = threadIdx.x, w = 2 * h + 1;
    const int count = (int)(n - t0 < RMED_TILE ? n - t0 : RMED_TILE);  // outputs of this tile, >= 1
    const T *xr = x + r * ld;

    // key j is sample clip(t0 - h + j, 0, n - 1): output o of the tile reads keys o .. o + 2h
    for (int j = tid; j < count + 2 * h; j += RMED_THREADS) {
        int64_t i = t0 - h + j;
        i = i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
        keys[j] = to_key(xr[i]);
    }
    __syncthreads();

    // a thread past the tile's end repeats the last output and stores nothing: no key beyond
    // count - 1 + 2h is read
    int o[RMED_PER_THREAD];
#pragma unroll
    for (int q = 0; q < RMED_PER_THREAD; ++q) {
        const int oq = tid + q * RMED_THREADS;
        o[q] = oq < count ? oq : count - 1;
    }
    K prefix[RMED_PER_THREAD];
    int rank[RMED_PER_THREAD], nans[RMED_PER_THREAD];
#pragma unroll
    for (int q = 0; q < RMED_PER_THREAD; ++q) prefix[q] = 0, rank[q] = h, nans[q] = 0;
    for (int k = 0; k < w; ++k) {
#pragma unroll
        for (int q = 0; q < RMED_PER_THREAD; ++q) nans[q] += keys[o[q] + k] == ~K(0);
    }
    for (int b = B - 1; b >= 0; --b) {
        const K mask = ~K(0) << b;  // bit b and the bits above it
        int c[RMED_PER_THREAD];
#pragma unroll
        for (int q = 0; q < RMED_PER_THREAD; ++q) c[q] = 0;
        for (int k = 0; k < w; ++k) {
#pragma unroll
            for (int q = 0; q < RMED_PER_THREAD; ++q) c[q] += ((keys[o[q] + k] ^ prefix[q]) & mask) == 0;
        }
#pragma unroll
        for (int q = 0; q < RMED_PER_THREAD; ++q) {
            const bool one = rank[q] >= c[q];
            rank[q] -= one ? c[q] : 0;
            prefix[q] |= one ? (K(1) << b) : K(0);
        }
    }
    T *outr = out + r * ld_out + t0;
#pragma unroll
    for (int q = 0; q < RMED_PER_THREAD; ++q) {
        const int oq = tid + q * RMED_THREADS;
        T v = from_key<T>(prefix[q]);
        if (nans[q]) {
            const K qn = rmed_key<T>::quiet_nan;
            __builtin_memcpy(&v, &qn, sizeof(K));
        }
        if (oq < count) outr[oq] = v;
    }
}

template <typename T, int V> struct alignas(sizeof(T) * V) dt_piece { T v[V]; };

// base of sample i (header: "Baseline"); every step one float64 operation (-ffp-contract=off)
__device__ __forceinline__ double detrend_base(const double *__restrict__ med, int64_t nblk, int64_t d, double two_d, int64_t i)
{
    if (nblk == 1) return med[0];
    const double u = (double)(2 * i - d + 1) / two_d;
    int64_t b0 = (int64_t)floor(u);
    b0 = b0 < 0 ? 0 : (b0 > nblk - 2 ? nblk - 2 : b0);
    double t = u - (double)b0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double m0 = med[b0], m1 = med[b0 + 1];
    return t == 0.0 ? m0 : (t == 1.0 ? m1 : m0 + t * (m1 - m0));
}

template <typename T, int V>
__global__ void __launch_bounds__(256) detrend_apply_kernel(const T *x, int64_t n, int64_t ld, const double *__restrict__ med,
                                                            int64_t ld_med, int64_t nblk, int64_t d, T *out, int64_t ld_out,
                                                            int64_t nchunk)
{
    const int64_t bid = blockIdx.x, r = bid / nchunk;
    const int64_t i0 = ((bid % nchunk) * 256 + threadIdx.x) * V;
    if (i0 >= n) return;
    const T *xr = x + r * ld + i0;
    T *outr = out + r * ld_out + i0;
    const double *mr = med + r * ld_med;
    const double two_d = (double)(2 * d);
    const bool whole = V > 1 && i0 + V <= n;
    dt_piece<T, V> p;
    if (whole) {
        p = *reinterpret_cast<const dt_piece<T, V> *>(xr);
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k) p.v[k] = i0 + k < n ? xr[k] : T(0);
    }
#pragma unroll
    for (int k = 0; k < V; ++k) {
        const int64_t i = i0 + k < n ? i0 + k : n - 1;
        p.v[k] = static_cast<T>(static_cast<double>(p.v[k]) - detrend_base(mr, nblk, d, two_d, i));
    }
    if (whole) {
        *reinterpret_cast<dt_piece<T, V> *>(outr) = p;
    } else {
#pragma unroll
        for (int k = 0; k < V; ++k)
            if (i0 + k < n) outr[k] = p.v[k];
    }
}

// dtype and w of pu_running_median and its describe; *esize = the element's bytes
int rmed_check(const char *who, int dtype, int64_t w, size_t *esize)
{
    if (int rc = pu::with_dtype<float, double>(who, dtype, [&](auto tag) {
            *esize = sizeof(typename decltype(tag)::type);
            return PU_OK;
        }))
        return rc;
    PU_REQUIRE(w >= 1 && (w & 1), "%s: w %lld is not an odd width >= 1", who, (long long)w);
    if (w > RMED_MAX_W) {
        pu::set_error("%s: w %lld above %d (the tile's halo is staged in LDS)", who, (long long)w, RMED_MAX_W);
        return PU_EUNSUPPORTED;
    }
    return PU_OK;
}

// *end = one past the last byte of rows of n elements, ld elements apart, from base; false when
// that is beyond the address space (an absurd ld)
bool rows_end(uintptr_t base, int64_t rows, int64_t ld, int64_t n, size_t esize, uintptr_t *end)
{
    const unsigned __int128 e = (unsigned __int128)base + ((unsigned __int128)(rows - 1) * (uint64_t)ld + (uint64_t)n) * esize;
    *end = (uintptr_t)e;
    return e <= (unsigned __int128)UINTPTR_MAX;
}

size_t rmed_lds_bytes(size_t esize, int64_t w) { return (size_t)(RMED_TILE + (w - 1)) * esize; }

}  // namespace

extern "C" {

int pu_running_median_describe(int dtype, int64_t w, int64_t *info, int n)
{
    size_t esize = 0;
    if (int rc = rmed_check("pu_running_median_describe", dtype, w, &esize)) return rc;
    PU_REQUIRE(info && n >= 0, "pu_running_median_describe: null info");
    const int64_t v[RMED_NINFO] = {RMED_TILE, (int64_t)rmed_lds_bytes(esize, w), RMED_MAX_W};
    for (int i = 0; i < n && i < RMED_NINFO; ++i) info[i] = v[i];
    return PU_OK;
}

int pu_running_median(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, int64_t w, void *out, int64_t ld_out,
                      void *stream)
{
    size_t esize = 0;
    if (int rc = rmed_check("pu_running_median", dtype, w, &esize)) return rc;
    PU_REQUIRE(rows >= 0, "pu_running_median: rows %lld < 0", (long long)rows);
    PU_REQUIRE(n >= 1, "pu_running_median: n %lld < 1", (long long)n);
    PU_REQUIRE(ld >= n && ld_out >= n, "pu_running_median: ld %lld or ld_out %lld < n = %lld", (long long)ld, (long long)ld_out,
               (long long)n);
    const int64_t ntiles = (n + RMED_TILE - 1) / RMED_TILE;
    if (rows > 0 && ntiles > INT32_MAX / rows) {
        pu::set_error("pu_running_median: rows %lld x %lld tiles above 2^31 - 1 (the grid of one call)", (long long)rows,
                      (long long)ntiles);
        return PU_EUNSUPPORTED;
    }
    if (rows == 0) return PU_OK;
    PU_REQUIRE(x && out, "pu_running_median: x or out is NULL");
    const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
    PU_REQUIRE(xa % esize == 0 && oa % esize == 0, "pu_running_median: a pointer is not aligned to its element type");
    uintptr_t xe, oe;
    PU_REQUIRE(rows_end(xa, rows, ld, n, esize, &xe) && rows_end(oa, rows, ld_out, n, esize, &oe),
               "pu_running_median: rows %lld x ld %lld or ld_out %lld beyond the address space", (long long)rows, (long long)ld,
               (long long)ld_out);
    PU_REQUIRE(xe <= oa || oe <= xa, "pu_running_median: x and out overlap");
    const int h = (int)((w - 1) / 2);
    return pu::with_dtype<float, double>("pu_running_median", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return pu::launch("running_median_kernel", running_median_kernel<T>, dim3((unsigned)(rows * ntiles)), dim3(RMED_THREADS),
                          rmed_lds_bytes(sizeof(T), w), pu::as_stream(stream), (const T *)x, n, ld, h, ntiles, (T *)out, ld_out);
    });
}

int pu_detrend_apply(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, const double *med, int64_t ld_med,
                     int64_t nblk, int64_t d, void *out, int64_t ld_out, void *stream)
{
    return pu::with_dtype<float, double>("pu_detrend_apply", dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        constexpr int V = 16 / sizeof(T);
        PU_REQUIRE(rows >= 0, "pu_detrend_apply: rows %lld < 0", (long long)rows);
        PU_REQUIRE(n >= 1, "pu_detrend_apply: n %lld < 1", (long long)n);
        PU_REQUIRE(d >= 1, "pu_detrend_apply: d %lld < 1", (long long)d);
        PU_REQUIRE(nblk >= 1 && nblk == n / d, "pu_detrend_apply: nblk %lld is not n / d = %lld (at least 1)", (long long)nblk,
                   (long long)(n / d));
        PU_REQUIRE(ld >= n && ld_out >= n && ld_med >= nblk,
                   "pu_detrend_apply: ld %lld or ld_out %lld < n = %lld, or ld_med %lld < nblk = %lld", (long long)ld,
                   (long long)ld_out, (long long)n, (long long)ld_med, (long long)nblk);
        // 2 i - d + 1 must convert to float64 exactly; the grid is at most one workgroup per 256 samples
        const int64_t nchunk1 = (n + 255) / 256, nchunk = (n + 256 * V - 1) / (256 * V);
        if (n > (int64_t(1) << 51) || (rows > 0 && nchunk1 > INT32_MAX / rows)) {
            pu::set_error("pu_detrend_apply: rows %lld x n %lld too large for one call", (long long)rows, (long long)n);
            return PU_EUNSUPPORTED;
        }
        if (rows == 0) return PU_OK;
        PU_REQUIRE(x && med && out, "pu_detrend_apply: x, med or out is NULL");
        const uintptr_t xa = reinterpret_cast<uintptr_t>(x), oa = reinterpret_cast<uintptr_t>(out);
        PU_REQUIRE(xa % sizeof(T) == 0 && oa % sizeof(T) == 0 && reinterpret_cast<uintptr_t>(med) % 8 == 0,
                   "pu_detrend_apply: a pointer is not aligned to its element type");
        uintptr_t xe, oe;
        PU_REQUIRE(rows_end(xa, rows, ld, n, sizeof(T), &xe) && rows_end(oa, rows, ld_out, n, sizeof(T), &oe),
                   "pu_detrend_apply: rows %lld x ld %lld or ld_out %lld beyond the address space", (long long)rows, (long long)ld,
                   (long long)ld_out);
        // in place (a sample is read and written by one lane) or apart: anything between would read what another
        // workgroup has written
        PU_REQUIRE((xa == oa && ld == ld_out) || xe <= oa || oe <= xa,
                   "pu_detrend_apply: out overlaps x without being x itself (the same pointer and ld_out == ld)");
        const dim3 grid((unsigned)(rows * nchunk)), block(256);
        hipStream_t s = pu::as_stream(stream);
        // 16-byte pieces where x, out and every row start are aligned to them
        const uintptr_t a = xa | oa | ((uintptr_t)ld * sizeof(T)) | ((uintptr_t)ld_out * sizeof(T));
        if (a % 16 == 0)
            return pu::launch("detrend_apply_kernel<vec>", detrend_apply_kernel<T, V>, grid, block, 0, s, (const T *)x, n, ld, med,
                              ld_med, nblk, d, (T *)out, ld_out, nchunk);
        // element by element otherwise
        return pu::launch("detrend_apply_kernel", detrend_apply_kernel<T, 1>, dim3((unsigned)(rows * nchunk1)), block, 0, s,
                          (const T *)x, n, ld, med, ld_med, nblk, d, (T *)out, ld_out, nchunk1);
    });
}

}  // extern "C"
