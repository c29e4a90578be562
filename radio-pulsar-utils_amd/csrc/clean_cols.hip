// Column passes of the RFI cleaning for gfx950 (MI355X): the sums over channels run
// sequentially over the rows, numpy's order for mean(0) and the zero-DM light curve
// (order and -ffp-contract=off: clean_common.h).
//
// Kernels
//   colmean_kernel           V adjacent columns per lane, rows in order (clean.py:77).
//   colsum_u8_seg_kernel,    8-bit input: exact integer column sums by row segments,
//   colsum_u8_finish_kernel  added and divided in place.
//   apply_kernel             (x*f - mu)/mu, bad rows zeroed, optional column mean (:81-94),
//                            V adjacent columns per lane.
//   zero_cols_kernel         listed columns of the plane zeroed.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <type_traits>

#include "clean_common.h"

namespace {

// colmean_kernel's bytes of rows in flight per lane and register buffer (C4 sweep,
// profiles/r02_clean/: f32 V=4 190 us vs 212 us at walk_rows' default of 128 B)
constexpr int kColmeanBatchBytes = 256;

// Skipped rows add +0.0 (a select, not a branch): acc starts at +0.0 and never
// becomes -0.0 under round-to-nearest, so acc + 0.0 == acc bit for bit, and NaN or
// Inf in a skipped row never reaches the sum.
template <typename Tin, int V>
__global__ void __launch_bounds__(256)
colmean_kernel(const Tin *__restrict__ x, int64_t nrows, int64_t col0, int64_t ncols, int64_t ld,
               const uint8_t *__restrict__ skip, double *__restrict__ out)
{
    __shared__ uint8_t sk[kRowChunk];
    const int64_t c = col0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    const bool active = c < col0 + ncols;
    double acc[V];
#pragma unroll
    for (int j = 0; j < V; ++j) acc[j] = 0.0;
    int64_t ngood = 0;
    auto body_fn = [&](int i, const Vec<Tin, V> &v) {
        const bool s = sk[i] != 0;
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] += s ? 0.0 : static_cast<double>(v.v[j]);
    };
    for (int64_t r0 = 0; r0 < nrows; r0 += kRowChunk) {
        const int rn = (int)(nrows - r0 < kRowChunk ? nrows - r0 : kRowChunk);
        __syncthreads();
        for (int i = threadIdx.x; i < rn; i += 256) sk[i] = skip ? skip[r0 + i] : 0;
        __syncthreads();
        for (int i = 0; i < rn; ++i) ngood += sk[i] ? 0 : 1;
        if (!active) continue;
        walk_rows<Tin, V, decltype(body_fn) &, kColmeanBatchBytes>(x + r0 * ld + c, ld, rn, body_fn);
    }
    if (!active) return;
#pragma unroll
    for (int j = 0; j < V; ++j) out[c + j] = acc[j] / static_cast<double>(ngood);
}

// 8-bit column sums by row segments.  Every partial sum of 8-bit values is an integer
// (< 2^53), so float64 accumulation is exact in any order: the sequential chain of
// colmean_kernel and a sum of per-segment integer sums give the same bits.  Segments of
// kColSegRows rows fit u16 (256 x 255 = 65280), two columns per dword lane half
// (bytes 0/2 and 1/3 masked with 0x00ff00ff: the halves never carry into each other), so a
// row of 8 columns costs one 8-byte load and four adds.  The (up to 4) u16 segment sums of
// column c are written into out[c]'s 8 bytes; colsum_u8_finish_kernel adds them and divides
// in place.  4 x the lanes of the row-sequential kernel for the same bytes.
constexpr int kColSegRows = 256;
constexpr int kColSegMax = 4;

__global__ void __launch_bounds__(256)
colsum_u8_seg_kernel(const uint8_t *__restrict__ x, int64_t nrows, int64_t ncols, int64_t ld,
                     const uint8_t *__restrict__ skip, uint16_t *__restrict__ part)
{
    __shared__ uint8_t sk[kColSegRows];
    const int seg = blockIdx.y;
    const int64_t r0 = (int64_t)seg * kColSegRows;
    const int rn = (int)(nrows - r0 < kColSegRows ? nrows - r0 : kColSegRows);
    if ((int)threadIdx.x < rn) sk[threadIdx.x] = skip ? skip[r0 + threadIdx.x] : 0;
    __syncthreads();
    const int64_t c = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 8;
    if (c >= ncols) return;
    const uint8_t *p = x + r0 * ld + c;
    uint32_t a02 = 0, a13 = 0, a46 = 0, a57 = 0;  // u16 pairs: columns (0,2), (1,3), (4,6), (5,7)
    constexpr int B = 16;                          // rows in flight per lane
    for (int i0 = 0; i0 < rn; i0 += B) {
        uint2 v[B];
#pragma unroll
        for (int k = 0; k < B; ++k)
            if (i0 + k < rn) v[k] = *reinterpret_cast<const uint2 *>(p + (int64_t)(i0 + k) * ld);
#pragma unroll
        for (int k = 0; k < B; ++k) {
            if (i0 + k < rn && !sk[i0 + k]) {
                a02 += v[k].x & 0x00ff00ffu;
                a13 += (v[k].x >> 8) & 0x00ff00ffu;
                a46 += v[k].y & 0x00ff00ffu;
                a57 += (v[k].y >> 8) & 0x00ff00ffu;
            }
        }
    }
    uint16_t *q = part + c * kColSegMax + seg;  // out[c] viewed as 4 x u16
    const uint32_t s[8] = {a02 & 0xffffu, a13 & 0xffffu, a02 >> 16, a13 >> 16,
                           a46 & 0xffffu, a57 & 0xffffu, a46 >> 16, a57 >> 16};
#pragma unroll
    for (int j = 0; j < 8; ++j) q[j * kColSegMax] = (uint16_t)s[j];
}

__global__ void __launch_bounds__(256)
colsum_u8_finish_kernel(double *__restrict__ out, int64_t ncols, int nseg, int64_t nrows,
                        const uint8_t *__restrict__ skip)
{
    __shared__ int cnt[256];
    int good = 0;
    for (int64_t r = threadIdx.x; r < nrows; r += 256) good += (skip && skip[r]) ? 0 : 1;
    cnt[threadIdx.x] = good;
    __syncthreads();
    for (int off = 128; off > 0; off >>= 1) {
        if ((int)threadIdx.x < off) cnt[threadIdx.x] += cnt[threadIdx.x + off];
        __syncthreads();
    }
    const double ngood = (double)cnt[0];
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (c >= ncols) return;
    const uint64_t w = reinterpret_cast<const uint64_t *>(out)[c];
    uint32_t tot = 0;
    for (int k = 0; k < nseg; ++k) tot += (uint32_t)((w >> (16 * k)) & 0xffffu);
    out[c] = (double)tot / ngood;
}

// (x*f - mu)/mu per element, bad channels written as 0.0, column mean of the result
// accumulated over channels in order.  Same column layout as colmean_kernel; the
// channel means and bad flags are staged in LDS per row chunk.
//
// ZDM (opt-in zero-DM subtraction, no reference counterpart: clean.py:77-82 only
// divides by the smoothed zero-DM series): the strip is walked twice.  The first walk
// sums the normalised values over channels in order (bad channels add +0.0, so the sum
// is the good channels' sum bit for bit); the second writes e - S[t]/ngood for good
// channels and 0.0 for bad ones.  col_means (the cut_outliers series) is S[t]/nchan of
// the normalised data BEFORE the subtraction, as without ZDM.
template <typename Tin, int V, bool NT, bool ZDM>
__global__ void __launch_bounds__(256)
apply_kernel(const Tin *__restrict__ x, int64_t nchan, int64_t col0, int64_t ncols, int64_t ld,
             const double *__restrict__ factor, const double *__restrict__ spec,
             const uint8_t *__restrict__ bad, double *__restrict__ out, int64_t ld_out,
             double *__restrict__ col_means, int64_t ngood)
{
    __shared__ double mus[kRowChunk];
    __shared__ uint8_t bads[kRowChunk];
    const int64_t c = col0 + ((int64_t)blockIdx.x * 256 + threadIdx.x) * V;
    const bool active = c < col0 + ncols;
    double f[V], acc[V], zsub[V];
#pragma unroll
    for (int j = 0; j < V; ++j) {
        f[j] = active ? factor[c + j] : 0.0;
        acc[j] = 0.0;
        zsub[j] = 0.0;
    }
    auto stage = [&](int64_t r0, int rn) {
        __syncthreads();
        for (int i = threadIdx.x; i < rn; i += 256) {
            mus[i] = spec[r0 + i];
            bads[i] = bad ? bad[r0 + i] : 0;
        }
        __syncthreads();
    };
    if constexpr (ZDM) {
        for (int64_t r0 = 0; r0 < nchan; r0 += kRowChunk) {
            const int rn = (int)(nchan - r0 < kRowChunk ? nchan - r0 : kRowChunk);
            stage(r0, rn);
            if (!active) continue;
            auto sum_fn = [&](int i, const Vec<Tin, V> &v) {
                const double mu = mus[i];
                const bool b = bads[i] != 0;
#pragma unroll
                for (int j = 0; j < V; ++j) {
                    double e = static_cast<double>(v.v[j]) * f[j];
                    e = (e - mu) / mu;
                    acc[j] += b ? 0.0 : e;
                }
            };
            walk_rows<Tin, V>(x + r0 * ld + c, ld, rn, sum_fn);
        }
#pragma unroll
        for (int j = 0; j < V; ++j) zsub[j] = ngood > 0 ? acc[j] / static_cast<double>(ngood) : 0.0;
    }
    for (int64_t r0 = 0; r0 < nchan; r0 += kRowChunk) {
        const int rn = (int)(nchan - r0 < kRowChunk ? nchan - r0 : kRowChunk);
        stage(r0, rn);
        if (!active) continue;
        double *o = out + r0 * ld_out + c;
        auto apply_fn = [&](int i, const Vec<Tin, V> &v) {
            const double mu = mus[i];
            const bool b = bads[i] != 0;
            Vec<double, V> res;
#pragma unroll
            for (int j = 0; j < V; ++j) {
                double e = static_cast<double>(v.v[j]) * f[j];
                e = (e - mu) / mu;
                if constexpr (ZDM) {
                    res.v[j] = b ? 0.0 : e - zsub[j];
                } else {
                    res.v[j] = b ? 0.0 : e;
                    acc[j] += res.v[j];
                }
            }
            if constexpr (NT && V % 2 == 0) {
                // 16-byte non-temporal stores (round 3: one 8-byte store per column)
                typedef double f64x2 __attribute__((ext_vector_type(2)));
#pragma unroll
                for (int j = 0; j < V; j += 2)
                    __builtin_nontemporal_store(f64x2{res.v[j], res.v[j + 1]},
                                                reinterpret_cast<f64x2 *>(o + (int64_t)i * ld_out + j));
            } else if constexpr (NT) {
#pragma unroll
                for (int j = 0; j < V; ++j) __builtin_nontemporal_store(res.v[j], o + (int64_t)i * ld_out + j);
            } else {
                *reinterpret_cast<Vec<double, V> *>(o + (int64_t)i * ld_out) = res;
            }
        };
        walk_rows<Tin, V>(x + r0 * ld + c, ld, rn, apply_fn);
    }
    if (!active || !col_means) return;
#pragma unroll
    for (int j = 0; j < V; ++j) col_means[c + j] = acc[j] / static_cast<double>(nchan);
}

__global__ void zero_cols_kernel(double *out, int64_t nrows, int64_t ld, const int64_t *__restrict__ cols,
                                 int64_t ncols)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    for (int64_t rr = r; rr < nrows; rr += gridDim.y)
        if (k < ncols) out[rr * ld + cols[k]] = 0.0;
}

// Column lanes: V adjacent columns per lane (16-byte loads at most), the widest V the
// alignment allows up to a per-pass, per-type maximum.  Measured on C4 (1024 x 2^18,
// DESIGN.md section 4.4): the read-only mean pass is fastest with wide lanes (V=4).
template <typename Tin>
int col_means_t(const void *x, int64_t nrows, int64_t n, int64_t ld, const uint8_t *skip, double *out, hipStream_t s)
{
    if constexpr (sizeof(Tin) == 1) {
        // 8-bit input: exact integer sums by row segments
        const int nseg = (int)((nrows + kColSegRows - 1) / kColSegRows);
        if (nseg <= kColSegMax && n % 8 == 0 && ld % 8 == 0 && reinterpret_cast<uintptr_t>(x) % 8 == 0) {
            hipLaunchKernelGGL(colsum_u8_seg_kernel, dim3(blocks_for(n / 8, 256), nseg), dim3(256), 0, s,
                               reinterpret_cast<const uint8_t *>(x), nrows, n, ld, skip,
                               reinterpret_cast<uint16_t *>(out));
            hipLaunchKernelGGL(colsum_u8_finish_kernel, dim3(blocks_for(n, 256)), dim3(256), 0, s, out, n, nseg,
                               nrows, skip);
            return PU_OK;
        }
    }
    constexpr int VMAX = sizeof(Tin) >= 8 ? 2 : 4;
    const int v = pick_vec<Tin>(x, ld, VMAX);
    return column_launches<VMAX>(v, n, [&](auto vc, int64_t col0, int64_t ncols) {
        constexpr int V = decltype(vc)::value;
        hipLaunchKernelGGL((colmean_kernel<Tin, V>), dim3(blocks_for(ncols / V, 256)), dim3(256), 0, s,
                           reinterpret_cast<const Tin *>(x), nrows, col0, ncols, ld, skip, out);
    });
}

template <typename Tin>
int renorm_apply_t(const void *x, int64_t nchan, int64_t n, int64_t ld, const double *factor, const double *spec,
                   const uint8_t *bad, double *out, int64_t ld_out, double *col_means, int64_t ngood_zdm,
                   hipStream_t s)
{
    // C4 sweep (profiles/r02_clean/): f32 V=4 615 us (V=1 640), u8 V=2 + nt stores 480 us
    constexpr int VMAX = sizeof(Tin) == 4 ? 4 : sizeof(Tin) == 1 ? 2 : 1;
    // Output plane written with non-temporal stores: on for 8-bit input (C4 u8 apply
    // 542 -> 481 us), off for float input (606 vs 623 us)
    constexpr bool NT = sizeof(Tin) == 1;
    const int v = std::min(pick_vec<Tin>(x, ld, VMAX), pick_vec<double>(out, ld_out, VMAX));
    const bool zdm = ngood_zdm >= 0;
    return column_launches<VMAX>(v, n, [&](auto vc, int64_t col0, int64_t ncols) {
        constexpr int V = decltype(vc)::value;
        auto go = [&](auto kern) {
            hipLaunchKernelGGL(kern, dim3(blocks_for(ncols / V, 256)), dim3(256), 0, s,
                               reinterpret_cast<const Tin *>(x), nchan, col0, ncols, ld, factor, spec, bad, out,
                               ld_out, col_means, ngood_zdm);
        };
        if (zdm)
            go(apply_kernel<Tin, V, NT, true>);
        else
            go(apply_kernel<Tin, V, NT, false>);
    });
}

}  // namespace

extern "C" {

int pu_col_means(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, const uint8_t *skip, double *out,
                 void *stream)
{
    PU_REQUIRE(x && out, "pu_col_means: NULL pointer");
    PU_REQUIRE(nrows > 0 && n > 0 && ld >= n, "pu_col_means: bad shape");
    hipStream_t s = pu::as_stream(stream);
    // (one check after the launches of every column range)
    int rc = pu::with_dtype<uint8_t, float, double>("pu_col_means", dtype, [&](auto tag) {
        return col_means_t<typename decltype(tag)::type>(x, nrows, n, ld, skip, out, s);
    });
    return rc ? rc : pu::launch_check("colmean_kernel");
}

static int renorm_apply_any(const void *x, int dtype, int64_t nchan, int64_t n, int64_t ld, const double *factor,
                            const double *spec, const uint8_t *bad, double *out, int64_t ld_out, double *col_means,
                            int64_t ngood_zdm, void *stream)
{
    PU_REQUIRE(x && factor && spec && out, "pu_renorm_apply: NULL pointer");
    PU_REQUIRE(nchan > 0 && n > 0 && ld >= n && ld_out >= n, "pu_renorm_apply: bad shape");
    hipStream_t s = pu::as_stream(stream);
    // (one check after the launches of every column range)
    int rc = pu::with_dtype<uint8_t, float, double>("pu_renorm_apply", dtype, [&](auto tag) {
        return renorm_apply_t<typename decltype(tag)::type>(x, nchan, n, ld, factor, spec, bad, out, ld_out, col_means,
                                                            ngood_zdm, s);
    });
    return rc ? rc : pu::launch_check("apply_kernel");
}

int pu_renorm_apply(const void *x, int dtype, int64_t nchan, int64_t n, int64_t ld, const double *factor,
                    const double *spec, const uint8_t *bad, double *out, int64_t ld_out, double *col_means,
                    void *stream)
{
    return renorm_apply_any(x, dtype, nchan, n, ld, factor, spec, bad, out, ld_out, col_means, -1, stream);
}

int pu_renorm_apply_zero_dm(const void *x, int dtype, int64_t nchan, int64_t n, int64_t ld, const double *factor,
                            const double *spec, const uint8_t *bad, int64_t ngood, double *out, int64_t ld_out,
                            double *col_means, void *stream)
{
    PU_REQUIRE(ngood >= 0 && ngood <= nchan, "pu_renorm_apply_zero_dm: ngood %lld outside [0, nchan]",
               (long long)ngood);
    return renorm_apply_any(x, dtype, nchan, n, ld, factor, spec, bad, out, ld_out, col_means, ngood, stream);
}

int pu_zero_columns(double *out, int64_t nrows, int64_t ld, const int64_t *cols, int64_t ncols, void *stream)
{
    PU_REQUIRE(out && nrows > 0 && ld > 0, "pu_zero_columns: bad arguments");
    if (ncols <= 0) return PU_OK;
    PU_REQUIRE(cols != nullptr, "pu_zero_columns: cols is NULL");
    const unsigned gy = (unsigned)(nrows < 1024 ? nrows : 1024);
    return pu::launch("zero_cols_kernel", zero_cols_kernel, dim3(blocks_for(ncols, 256), gy), dim3(256), 0,
                      pu::as_stream(stream), out, nrows, ld, cols, ncols);
}

}  // extern "C"
