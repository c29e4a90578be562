// Row reductions of the RFI cleaning for gfx950 (MI355X): numpy's add.reduce over a
// contiguous row, bit for bit (order and -ffp-contract=off: clean_common.h).
//
// Kernels
//   rowsum_chunk_kernel  one workgroup per (row, full 8192 block): leaves read straight
//                        into registers, 8-accumulator leaf sums, in-order pairwise
//                        tree by xor-shuffles.
//   rowsum_tail_kernel   one lane per row for the trailing partial block (irregular
//                        pairwise tree; compile-time-bounded recursion).
//   rowsum_combine       sequential 0 + block sums (+ true_divide by the count).
//   row_moments_combine  the same, with the rows' shifted moments (pu_row_moments).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "clean_common.h"

namespace {

constexpr int kScaleRows = 16;  // rows per workgroup of the scaled (MODE 2) row sums
                                // (C4 sweep: f32 191 vs 206 us at 4; u8 73 vs 86 us)

// load_val on an element already in registers (s = scale[t] for MODE 2).
template <typename Tin, typename Ta, int MODE>
__device__ __forceinline__ Ta elem_val(Tin x, Ta center, double s)
{
    if constexpr (MODE == 0) {
        return static_cast<Ta>(x);
    } else if constexpr (MODE == 1) {
        const Ta d = static_cast<Ta>(x) - center;
        return d * d;
    } else if constexpr (MODE == 4) {
        const Ta v = static_cast<Ta>(x);
        return v * v;
    } else {
        return static_cast<Ta>(static_cast<double>(x) * s);
    }
}

// Full 8192-element blocks: 64 leaves of 128, read straight into registers.
// Thread (b = tid/4, q = tid%4) owns accumulators r[2q], r[2q+1] of leaf b and loads
// its 16 element pairs (stride 8) with all loads in flight; the leaf total is
// ((r0+r1)+(r2+r3))+((r4+r5)+(r6+r7)) via two xor-shuffles.  The 64 leaves combine
// as the perfect binary tree pairwise_sum builds for n = 8192: leaf distances 1..8
// are lane distances 4..32 inside a wave (left + right at the even lane), the last
// two levels are (W0+W1)+(W2+W3) over the four waves.  PAIR: element pairs (and
// the scale pairs of MODE 2) are single 2-element vector loads.  A workgroup sums
// the same block of R consecutive rows, so MODE 2 reads its scale pairs once per R
// rows instead of once per row.
//
// MOM (MODE 0, pu_row_moments): the same pass also sums, in float64 and in any order,
// d = x - c and d^2 with c = the row's first element - the shifted moments from which
// measure_channel_variability's std is certified without a second pass (clean.py).
template <typename Tin, typename Ta, int MODE, bool PAIR, int R, bool MOM = false>
__global__ void __launch_bounds__(256)
rowsum_chunk_kernel(const Tin *__restrict__ x, int64_t ld, int64_t nrows, int64_t nfull, int64_t nblk_row,
                    const Ta *__restrict__ centers, const double *__restrict__ scale,
                    Ta *__restrict__ block_sums, double *__restrict__ moments = nullptr)
{
    // mom_tot has one slot per wave, not per row, and only row0's moments are stored
    static_assert(!MOM || R == 1, "rowsum_chunk_kernel: MOM needs R == 1");
    __shared__ Ta wave_tot[R][4];
    __shared__ double mom_tot[2][4];
    const int64_t row0 = (blockIdx.x / nfull) * R;
    const int64_t blk = blockIdx.x % nfull;
    const int tid = threadIdx.x;
    const int b = tid >> 2, q = tid & 3;
    const int64_t e0 = blk * kBlock + b * kLeaf + 2 * q;
    double sa[16], sc[16];
#pragma unroll
    for (int m = 0; m < 16; ++m) {
        if constexpr (MODE == 2 && PAIR) {
            const Vec<double, 2> s = load_vec<double, 2>(scale + e0 + 8 * m);
            sa[m] = s.v[0];
            sc[m] = s.v[1];
        } else if constexpr (MODE == 2) {
            sa[m] = scale[e0 + 8 * m];
            sc[m] = scale[e0 + 8 * m + 1];
        } else {
            sa[m] = sc[m] = 0.0;
        }
    }
#pragma unroll
    for (int rr = 0; rr < R; ++rr) {
        const int64_t row = row0 + rr;
        if (row >= nrows) break;
        const Tin *rp = x + row * ld + e0;
        const Ta center = MODE == 1 ? centers[row] : Ta(0);
        Tin a[16], c[16];
#pragma unroll
        for (int m = 0; m < 16; ++m) {
            if constexpr (PAIR) {
                const Vec<Tin, 2> p = load_vec<Tin, 2>(rp + 8 * m);
                a[m] = p.v[0];
                c[m] = p.v[1];
            } else {
                a[m] = rp[8 * m];
                c[m] = rp[8 * m + 1];
            }
        }
        if constexpr (sizeof(Tin) == 1 && MODE == 0) {
            // 8-bit sums (round 5): every partial sum of bytes - and of (x - c) and (x - c)^2 -
            // is an integer far below 2^53, so the float64 sums are exact in ANY order and
            // integer adds give the same values bit for bit, at a fraction of the float64
            // work (the moments pass was bound by it: 3.3 TB/s of its 8-bit reads)
            uint32_t si = 0;
#pragma unroll
            for (int m = 0; m < 16; ++m) si += (uint32_t)a[m] + (uint32_t)c[m];
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) si += __shfl_xor(si, s, 64);  // <= 64 * 32 * 255
            if ((tid & 63) == 0) wave_tot[rr][tid >> 6] = static_cast<Ta>(si);
            if constexpr (MOM) {
                const int cs = (int)x[row * ld];
                int m1 = 0;
                uint32_t m2 = 0;
#pragma unroll
                for (int m = 0; m < 16; ++m) {
                    const int da = (int)a[m] - cs, dc = (int)c[m] - cs;
                    m1 += da + dc;
                    m2 += (uint32_t)(da * da) + (uint32_t)(dc * dc);
                }
#pragma unroll
                for (int s = 1; s < 64; s <<= 1) {  // |m1| <= 64 * 32 * 255, m2 <= 64 * 32 * 255^2 < 2^32
                    m1 += __shfl_xor(m1, s, 64);
                    m2 += __shfl_xor(m2, s, 64);
                }
                if ((tid & 63) == 0) {
                    mom_tot[0][tid >> 6] = static_cast<double>(m1);
                    mom_tot[1][tid >> 6] = static_cast<double>(m2);
                }
            }
            continue;
        }
        Ta r0 = elem_val<Tin, Ta, MODE>(a[0], center, sa[0]);
        Ta r1 = elem_val<Tin, Ta, MODE>(c[0], center, sc[0]);
#pragma unroll
        for (int m = 1; m < 16; ++m) {
            r0 += elem_val<Tin, Ta, MODE>(a[m], center, sa[m]);
            r1 += elem_val<Tin, Ta, MODE>(c[m], center, sc[m]);
        }
        Ta t = r0 + r1;
#pragma unroll
        for (int s = 1; s < 64; s <<= 1) t += __shfl_xor(t, s, 64);
        if ((tid & 63) == 0) wave_tot[rr][tid >> 6] = t;
        if constexpr (MOM) {
            const double cs = static_cast<double>(x[row * ld]);
            double m1 = 0.0, m2 = 0.0;
#pragma unroll
            for (int m = 0; m < 16; ++m) {
                const double da = static_cast<double>(a[m]) - cs, dc = static_cast<double>(c[m]) - cs;
                m1 += da + dc;
                m2 += da * da + dc * dc;
            }
#pragma unroll
            for (int s = 1; s < 64; s <<= 1) {
                m1 += __shfl_xor(m1, s, 64);
                m2 += __shfl_xor(m2, s, 64);
            }
            if ((tid & 63) == 0) {
                mom_tot[0][tid >> 6] = m1;
                mom_tot[1][tid >> 6] = m2;
            }
        }
    }
    __syncthreads();
    if (tid < R && row0 + tid < nrows)
        block_sums[(row0 + tid) * nblk_row + blk] =
            (wave_tot[tid][0] + wave_tot[tid][1]) + (wave_tot[tid][2] + wave_tot[tid][3]);
    if constexpr (MOM) {
        if (tid < 2 && row0 < nrows)
            moments[(row0 * nblk_row + blk) * 2 + tid] =
                (mom_tot[tid][0] + mom_tot[tid][1]) + (mom_tot[tid][2] + mom_tot[tid][3]);
    }
}

template <typename Tin, typename Ta, int MODE, bool MOM = false>
__global__ void __launch_bounds__(64)
rowsum_tail_kernel(const Tin *__restrict__ x, int64_t ld, int64_t nrows, int64_t n, int64_t nfull,
                   int64_t nblk_row, const Ta *__restrict__ centers, const double *__restrict__ scale,
                   Ta *__restrict__ block_sums, double *__restrict__ moments = nullptr)
{
    const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
    if (row >= nrows) return;
    const Ta center = MODE == 1 ? centers[row] : Ta(0);
    const int64_t off = nfull * kBlock;
    block_sums[row * nblk_row + nfull] =
        pairwise_lane<Tin, Ta, MODE, 10>(x + row * ld, off, n - off, center, scale);
    if constexpr (MOM) {
        const double cs = static_cast<double>(x[row * ld]);
        double m1 = 0.0, m2 = 0.0;
        for (int64_t i = off; i < n; ++i) {
            const double d = static_cast<double>(x[row * ld + i]) - cs;
            m1 += d;
            m2 += d * d;
        }
        moments[(row * nblk_row + nfull) * 2] = m1;
        moments[(row * nblk_row + nfull) * 2 + 1] = m2;
    }
}

// pu_row_moments' combine, one launch (round 5: two before): per row the block sums in
// block order into the mean (rowsum_combine's arithmetic) and (c, sum(x - c),
// sum((x - c)^2)), c = the row's first element, from the per-block moment pairs (float64).
template <typename Tin, typename Ta>
__global__ void row_moments_combine(const Ta *__restrict__ block_sums, const double *__restrict__ blk,
                                    const Tin *__restrict__ x, int64_t ld, int64_t nrows, int64_t nblk_row,
                                    double divisor, Ta *__restrict__ means, double *__restrict__ out)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    Ta acc = Ta(0);
    double m1 = 0.0, m2 = 0.0;
    // unrolled: 24 independent loads in flight per step (one at a time, the dependent adds
    // put every load's latency in series: 13 us for C4's 1024 rows x 32 blocks)
#pragma unroll 8
    for (int64_t k = 0; k < nblk_row; ++k) {
        acc += block_sums[row * nblk_row + k];
        m1 += blk[(row * nblk_row + k) * 2];
        m2 += blk[(row * nblk_row + k) * 2 + 1];
    }
    means[row] = static_cast<Ta>(static_cast<double>(acc) / divisor);
    out[row * 3] = static_cast<double>(x[row * ld]);
    out[row * 3 + 1] = m1;
    out[row * 3 + 2] = m2;
}

template <typename Ta>
__global__ void rowsum_combine(const Ta *__restrict__ block_sums, int64_t nrows, int64_t nblk_row,
                               double divisor, Ta *__restrict__ out)
{
    const int64_t row = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (row >= nrows) return;
    Ta acc = Ta(0);
#pragma unroll 8
    for (int64_t k = 0; k < nblk_row; ++k) acc += block_sums[row * nblk_row + k];
    if (divisor > 0) acc = static_cast<Ta>(static_cast<double>(acc) / divisor);
    out[row] = acc;
}

template <typename Tin, typename Ta, int MODE>
int row_sums_t(const void *x, int64_t nrows, int64_t n, int64_t ld, const void *center, const double *scale,
               double divisor, void *out, void *ws, hipStream_t s)
{
    const int64_t nfull = n / kBlock;
    const int64_t tail = n % kBlock;
    const int64_t nblk_row = nfull + (tail ? 1 : 0);
    Ta *bs = reinterpret_cast<Ta *>(ws);
    const Tin *xp = reinterpret_cast<const Tin *>(x);
    const Ta *cp = reinterpret_cast<const Ta *>(center);
    if (nfull > 0) {
        // pair loads need 2-element alignment of every row (and of the scale vector)
        const bool pair = reinterpret_cast<uintptr_t>(x) % (2 * sizeof(Tin)) == 0 && ld % 2 == 0 &&
                          (MODE != 2 || reinterpret_cast<uintptr_t>(scale) % 16 == 0);
        // MODE 2: R rows per workgroup share the scale pairs
        constexpr int R = MODE == 2 ? kScaleRows : 1;
        const int64_t ngroups = (nrows + R - 1) / R;
        PU_REQUIRE(ngroups * nfull < (int64_t(1) << 31), "pu_row_sums: too many blocks");
        if (pair)
            hipLaunchKernelGGL((rowsum_chunk_kernel<Tin, Ta, MODE, true, R>), dim3((unsigned)(ngroups * nfull)),
                               dim3(256), 0, s, xp, ld, nrows, nfull, nblk_row, cp, scale, bs);
        else
            hipLaunchKernelGGL((rowsum_chunk_kernel<Tin, Ta, MODE, false, R>), dim3((unsigned)(ngroups * nfull)),
                               dim3(256), 0, s, xp, ld, nrows, nfull, nblk_row, cp, scale, bs);
        int rc = pu::launch_check("rowsum_chunk_kernel");
        if (rc) return rc;
    }
    if (tail) {
        int rc = pu::launch("rowsum_tail_kernel", rowsum_tail_kernel<Tin, Ta, MODE>, dim3((unsigned)((nrows + 63) / 64)),
                            dim3(64), 0, s, xp, ld, nrows, n, nfull, nblk_row, cp, scale, bs, nullptr);
        if (rc) return rc;
    }
    return pu::launch("rowsum_combine", rowsum_combine<Ta>, dim3((unsigned)((nrows + 255) / 256)), dim3(256), 0, s, bs,
                      nrows, nblk_row, divisor, reinterpret_cast<Ta *>(out));
}

// pu_row_moments' workspace: a sum per block (of rows x blocks per row), then 2 doubles per block
struct MomentsWs {
    void *bs;
    double *mb;
    size_t bytes;
};

MomentsWs moments_carve(pu::Carver c, int64_t nrows, int64_t n)
{
    const int64_t nblk = (n + kBlock - 1) / kBlock;
    const size_t nb = (size_t)(nrows > 0 ? nrows : 0) * (size_t)(nblk > 0 ? nblk : 1);
    MomentsWs w;
    w.bs = c.take<char>(nb * sizeof(double), 8);
    w.mb = c.take<double>(nb * 2 * sizeof(double));
    w.bytes = c.used();
    return w;
}

// numpy's row means (MODE 0 order, divided by n) and, in the same pass, the shifted
// moments of every row (pu_row_moments).
template <typename Tin, typename Ta>
int row_moments_t(const void *x, int64_t nrows, int64_t n, int64_t ld, void *means, double *moments,
                  const MomentsWs &w, hipStream_t s)
{
    const int64_t nfull = n / kBlock;
    const int64_t tail = n % kBlock;
    const int64_t nblk_row = nfull + (tail ? 1 : 0);
    Ta *bs = reinterpret_cast<Ta *>(w.bs);
    double *mb = w.mb;
    const Tin *xp = reinterpret_cast<const Tin *>(x);
    if (nfull > 0) {
        PU_REQUIRE(nrows * nfull < (int64_t(1) << 31), "pu_row_moments: too many blocks");
        const bool pair = reinterpret_cast<uintptr_t>(x) % (2 * sizeof(Tin)) == 0 && ld % 2 == 0;
        if (pair)
            hipLaunchKernelGGL((rowsum_chunk_kernel<Tin, Ta, 0, true, 1, true>), dim3((unsigned)(nrows * nfull)),
                               dim3(256), 0, s, xp, ld, nrows, nfull, nblk_row, nullptr, nullptr, bs, mb);
        else
            hipLaunchKernelGGL((rowsum_chunk_kernel<Tin, Ta, 0, false, 1, true>), dim3((unsigned)(nrows * nfull)),
                               dim3(256), 0, s, xp, ld, nrows, nfull, nblk_row, nullptr, nullptr, bs, mb);
        int rc = pu::launch_check("rowsum_chunk_kernel");
        if (rc) return rc;
    }
    if (tail) {
        int rc = pu::launch("rowsum_tail_kernel", rowsum_tail_kernel<Tin, Ta, 0, true>, dim3((unsigned)((nrows + 63) / 64)),
                            dim3(64), 0, s, xp, ld, nrows, n, nfull, nblk_row, nullptr, nullptr, bs, mb);
        if (rc) return rc;
    }
    return pu::launch("row_moments_combine", row_moments_combine<Tin, Ta>, dim3((unsigned)((nrows + 255) / 256)), dim3(256),
                      0, s, bs, mb, xp, ld, nrows, nblk_row, (double)n, reinterpret_cast<Ta *>(means), moments);
}

template <typename Tin>
int row_sums_in(int mode, bool f32acc, const void *x, int64_t nrows, int64_t n, int64_t ld, const void *center,
                const double *scale, double divisor, void *out, void *ws, hipStream_t s)
{
    if (mode == 2) return row_sums_t<Tin, double, 2>(x, nrows, n, ld, center, scale, divisor, out, ws, s);
    if (mode == 3) return row_sums_t<Tin, double, 0>(x, nrows, n, ld, center, scale, divisor, out, ws, s);
    if (mode == 4) return row_sums_t<Tin, double, 4>(x, nrows, n, ld, center, scale, divisor, out, ws, s);
    if (f32acc) {
        if (mode == 0) return row_sums_t<Tin, float, 0>(x, nrows, n, ld, center, scale, divisor, out, ws, s);
        return row_sums_t<Tin, float, 1>(x, nrows, n, ld, center, scale, divisor, out, ws, s);
    }
    if (mode == 0) return row_sums_t<Tin, double, 0>(x, nrows, n, ld, center, scale, divisor, out, ws, s);
    return row_sums_t<Tin, double, 1>(x, nrows, n, ld, center, scale, divisor, out, ws, s);
}

}  // namespace

extern "C" {

size_t pu_row_sums_workspace_bytes(int64_t nrows, int64_t n)
{
    const int64_t nblk = (n + kBlock - 1) / kBlock;
    return (size_t)(nrows > 0 ? nrows : 0) * (size_t)(nblk > 0 ? nblk : 1) * sizeof(double);
}

int pu_row_sums(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, int mode, const void *center,
                const double *scale, double divisor, void *out, void *ws, size_t ws_bytes, void *stream)
{
    PU_REQUIRE(x && out, "pu_row_sums: NULL pointer");
    PU_REQUIRE(nrows > 0 && n > 0 && ld >= n, "pu_row_sums: bad shape");
    PU_REQUIRE(mode >= 0 && mode <= 4, "pu_row_sums: bad mode %d", mode);
    PU_REQUIRE(mode != 1 || center, "pu_row_sums: mode 1 needs center");
    PU_REQUIRE(mode != 2 || scale, "pu_row_sums: mode 2 needs scale");
    if (int rc = pu::check_workspace("pu_row_sums", ws, ws_bytes, pu_row_sums_workspace_bytes(nrows, n), 1)) return rc;
    hipStream_t s = pu::as_stream(stream);
    return pu::with_dtype<uint8_t, float, double>("pu_row_sums", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        // float32 input accumulates in float32 (modes 0 and 1)
        return row_sums_in<T>(mode, std::is_same_v<T, float>, x, nrows, n, ld, center, scale, divisor, out, ws, s);
    });
}

size_t pu_row_moments_workspace_bytes(int64_t nrows, int64_t n)
{
    return moments_carve(pu::Carver(), nrows, n).bytes;
}

int pu_row_moments(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, void *means, double *moments,
                   void *ws, size_t ws_bytes, void *stream)
{
    PU_REQUIRE(x && means && moments, "pu_row_moments: NULL pointer");
    PU_REQUIRE(nrows > 0 && n > 0 && ld >= n, "pu_row_moments: bad shape");
    const MomentsWs w = moments_carve(pu::Carver(ws), nrows, n);
    if (int rc = pu::check_workspace("pu_row_moments", ws, ws_bytes, w.bytes, 8)) return rc;
    hipStream_t s = pu::as_stream(stream);
    return pu::with_dtype<uint8_t, float, double>("pu_row_moments", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        // the accumulator: float32 for float32 input, float64 otherwise
        using Ta = std::conditional_t<std::is_same_v<T, float>, float, double>;
        return row_moments_t<T, Ta>(x, nrows, n, ld, means, moments, w, s);
    });
}

}  // extern "C"
