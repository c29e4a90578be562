// Rebinning and roll helpers (HBM-streaming kernels) for gfx950.
//
//   pu_rebin_time   <- quick_resample           pulsarutils/dedispersion.py:38-57
//   pu_rebin_chan   <- quick_chan_rebin         :15-35
//   pu_roll_rows    <- apply_dm_shifts_to_data  :254-258
//   pu_roll_and_sum <- roll_and_sum             :60-83
//   pu_transpose    <- the (nsamps, nchans) -> (nchans, nsamps) transpose sigpyproc's
//                      readBlock performs (clean.py:327, stats.py:45)
//   pu_unpack_transpose <- the same for 1/2/4-bit files: sigpyproc's unpack + transpose
// Each output element is produced by one lane in the reference's add order, so
// results are bit-identical to the reference for every supported dtype.
#include <hip/hip_runtime.h>

#include "pu_common.h"

namespace {

unsigned nblocks(int64_t n, int t) { return (unsigned)((n + t - 1) / t); }

template <typename Tin>
__global__ void rebin_time_kernel(const Tin *__restrict__ x, int64_t nrows, int64_t nout, int64_t ld, int64_t w,
                                  double *__restrict__ out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (i >= nout) return;
    const Tin *p = x + r * ld + i * w;
    double acc = 0.0;
    for (int64_t j = 0; j < w; ++j) acc += static_cast<double>(p[j]);
    out[r * nout + i] = acc;
}

template <typename Tin, typename Tout>
__global__ void rebin_chan_kernel(const Tin *__restrict__ x, int64_t n, int64_t ld, int64_t rb,
                                  Tout *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t g = blockIdx.y;
    if (t >= n) return;
    const Tin *p = x + g * rb * ld + t;
    Tout acc = static_cast<Tout>(p[0]);
    for (int64_t j = 1; j < rb; ++j) acc += static_cast<Tout>(p[j * ld]);
    out[g * n + t] = acc;
}

template <typename T>
__global__ void roll_rows_kernel(const T *__restrict__ x, int64_t n, int64_t ld, const int64_t *__restrict__ shifts,
                                 T *__restrict__ out)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t r = blockIdx.y;
    if (t >= n) return;
    int64_t s = shifts[r] % n;
    if (s < 0) s += n;
    int64_t idx = t + s;
    if (idx >= n) idx -= n;
    out[r * n + t] = x[r * ld + idx];
}

template <typename Tin>
__global__ void roll_and_sum_kernel(const Tin *__restrict__ x, int64_t n, int64_t roll, double *__restrict__ sum)
{
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) return;
    int64_t idx = t - roll;
    if (idx < 0) idx += n;
    sum[t] += static_cast<double>(x[idx]);
}

// 64x64 tiles through LDS (+1 element pad against bank conflicts); coalesced reads of
// ``src`` rows and coalesced writes of ``dst`` rows.
template <typename T>
__global__ void __launch_bounds__(256) transpose_kernel(const T *__restrict__ src, int64_t rows, int64_t cols,
                                                        int64_t ld_src, T *__restrict__ dst, int64_t ld_dst)
{
    __shared__ T tile[64][65];
    const int64_t r0 = (int64_t)blockIdx.y * 64, c0 = (int64_t)blockIdx.x * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    for (int i = ty; i < 64; i += 4) {
        const int64_t r = r0 + i, c = c0 + tx;
        if (r < rows && c < cols) tile[i][tx] = src[r * ld_src + c];
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int64_t c = c0 + i, r = r0 + tx;
        if (r < rows && c < cols) dst[c * ld_dst + r] = tile[tx][i];
    }
}

// Packed 1/2/4-bit samples -> channel-major bytes.  One workgroup makes a tile of UT_TC
// channels x UT_TT samples (32 KiB of dst) from UT_TT rows of PB = UT_TC * NBITS / 8 packed
// bytes.  The kernel is bound by the dst write (one byte per sample against NBITS / 8 read),
// so the tile is laid out for the store:
//   1. the packed bytes are read in W-byte pieces (W = the largest of 16/8/4/2/1 dividing
//      src and ld_src; a piece that crosses the row's end is read byte by byte) and stored
//      to LDS byte-transposed, pk[byte][time] - the LDS holds the PACKED tile (4-17 KiB);
//   2. a lane reads 16 consecutive samples of one packed byte column with one ds_read_b128
//      (the 8 / NBITS channels of a byte read the same address: a broadcast), extracts its
//      channel from the four dwords in registers ((w >> sh) & mask, 4 samples per op) and
//      stores 16 bytes along time: 16 lanes cover the tile's 256 contiguous bytes of a
//      channel row, a wave four such rows.  Rows of dst start at any address (ld_dst is the
//      sample count of the block), so the 16-byte store is an unaligned one.
// The row pitch of pk is UT_TT + 16 bytes: 16-byte aligned for the b128 reads, and 4 banks
// off per row so the byte columns of one read group land on different banks.
constexpr int UT_TT = 256, UT_TC = 128, UT_PITCH = UT_TT + 16;

template <int W> struct ut_piece;
template <> struct ut_piece<16> { using type = uint4; };
template <> struct ut_piece<8> { using type = uint2; };
template <> struct ut_piece<4> { using type = uint32_t; };
template <> struct ut_piece<2> { using type = uint16_t; };
template <> struct ut_piece<1> { using type = uint8_t; };

template <int NBITS, int W>
__global__ void __launch_bounds__(256) unpack_transpose_kernel(const uint8_t *__restrict__ src, int64_t nsamps,
                                                               int64_t nchans, int64_t row_bytes, int64_t ld_src,
                                                               uint8_t *__restrict__ dst, int64_t ld_dst, int64_t nct)
{
    constexpr int PB = UT_TC * NBITS / 8;  // packed bytes of a tile row: 16 / 32 / 64
    constexpr int PPR = PB / W;            // pieces per tile row
    using piece_t = typename ut_piece<W>::type;
    __shared__ __attribute__((aligned(16))) uint8_t pk[PB * UT_PITCH];
    const int64_t bid = blockIdx.x, ct = bid % nct;
    const int64_t t0 = (bid / nct) * UT_TT, b0 = ct * PB, c0 = ct * UT_TC;

    for (int item = threadIdx.x; item < UT_TT * PPR; item += 256) {
        const int tl = item / PPR, bl = (item % PPR) * W;
        const int64_t t = t0 + tl, b = b0 + bl;
        if (t >= nsamps || b >= row_bytes) continue;
        const uint8_t *p = src + t * ld_src + b;
        uint8_t v[W];
        if (b + W <= row_bytes) {
            const piece_t w = *reinterpret_cast<const piece_t *>(p);
            __builtin_memcpy(v, &w, W);
        } else {
#pragma unroll
            for (int k = 0; k < W; ++k) v[k] = b + k < row_bytes ? p[k] : (uint8_t)0;
        }
#pragma unroll
        for (int k = 0; k < W; ++k) pk[(bl + k) * UT_PITCH + tl] = v[k];
    }
    __syncthreads();

    constexpr uint32_t MASK = ((1u << NBITS) - 1u) * 0x01010101u;
    for (int item = threadIdx.x; item < UT_TC * (UT_TT / 16); item += 256) {
        const int cl = item / (UT_TT / 16), q = item % (UT_TT / 16);
        const int64_t c = c0 + cl, t = t0 + q * 16;
        if (c >= nchans || t >= nsamps) continue;
        const uint4 w = *reinterpret_cast<const uint4 *>(&pk[(cl * NBITS / 8) * UT_PITCH + q * 16]);
        // sh + NBITS <= 8: the bits shifted in from the next byte fall outside the mask
        const int sh = (cl * NBITS) % 8;
        const uint4 o = make_uint4((w.x >> sh) & MASK, (w.y >> sh) & MASK, (w.z >> sh) & MASK, (w.w >> sh) & MASK);
        uint8_t *d = dst + c * ld_dst + t;
        if (t + 16 <= nsamps) {
            __builtin_memcpy(d, &o, 16);
        } else {
            uint8_t ob[16];
            __builtin_memcpy(ob, &o, 16);
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (t + k < nsamps) d[k] = ob[k];
        }
    }
}

template <int NBITS>
void launch_unpack_transpose(int w, unsigned grid, hipStream_t s, const uint8_t *src, int64_t nsamps, int64_t nchans,
                             int64_t row_bytes, int64_t ld_src, uint8_t *dst, int64_t ld_dst, int64_t nct)
{
    const dim3 g(grid), b(256);
    switch (w) {
    case 16: hipLaunchKernelGGL((unpack_transpose_kernel<NBITS, 16>), g, b, 0, s, src, nsamps, nchans, row_bytes, ld_src, dst, ld_dst, nct); break;
    case 8: hipLaunchKernelGGL((unpack_transpose_kernel<NBITS, 8>), g, b, 0, s, src, nsamps, nchans, row_bytes, ld_src, dst, ld_dst, nct); break;
    case 4: hipLaunchKernelGGL((unpack_transpose_kernel<NBITS, 4>), g, b, 0, s, src, nsamps, nchans, row_bytes, ld_src, dst, ld_dst, nct); break;
    case 2: hipLaunchKernelGGL((unpack_transpose_kernel<NBITS, 2>), g, b, 0, s, src, nsamps, nchans, row_bytes, ld_src, dst, ld_dst, nct); break;
    default: hipLaunchKernelGGL((unpack_transpose_kernel<NBITS, 1>), g, b, 0, s, src, nsamps, nchans, row_bytes, ld_src, dst, ld_dst, nct); break;
    }
}

}  // namespace

extern "C" {

int pu_unpack_transpose(const void *src, int nbits, int64_t nsamps, int64_t nchans, int64_t ld_src, uint8_t *dst,
                        int64_t ld_dst, void *stream)
{
    if (nbits != 1 && nbits != 2 && nbits != 4) {
        pu::set_error("pu_unpack_transpose: nbits %d unsupported (1, 2, 4)", nbits);
        return PU_EUNSUPPORTED;
    }
    PU_REQUIRE(src && dst && nsamps >= 0 && nchans >= 0 && nchans <= INT64_MAX / 8,
               "pu_unpack_transpose: bad arguments");
    PU_REQUIRE(nchans * nbits % 8 == 0, "pu_unpack_transpose: nchans %lld x nbits %d is not a whole number of bytes",
               (long long)nchans, nbits);
    const int64_t row_bytes = nchans * nbits / 8;
    PU_REQUIRE(ld_src >= row_bytes && ld_dst >= nsamps,
               "pu_unpack_transpose: leading dimension too small (ld_src %lld < %lld row bytes or ld_dst %lld < %lld "
               "samples)", (long long)ld_src, (long long)row_bytes, (long long)ld_dst, (long long)nsamps);
    if (nsamps == 0 || nchans == 0) return PU_OK;
    const int64_t nct = (nchans + UT_TC - 1) / UT_TC, ntt = (nsamps + UT_TT - 1) / UT_TT;
    PU_REQUIRE(ntt <= INT32_MAX / nct, "pu_unpack_transpose: %lld x %lld tiles exceed the grid limit",
               (long long)ntt, (long long)nct);
    // the widest piece that src and every row start are aligned to
    const uintptr_t a = reinterpret_cast<uintptr_t>(src) | static_cast<uintptr_t>(ld_src);
    const int w = a % 16 == 0 ? 16 : a % 8 == 0 ? 8 : a % 4 == 0 ? 4 : a % 2 == 0 ? 2 : 1;
    const unsigned grid = (unsigned)(nct * ntt);
    hipStream_t s = pu::as_stream(stream);
    const uint8_t *p = static_cast<const uint8_t *>(src);
    switch (nbits) {
    case 1: launch_unpack_transpose<1>(w, grid, s, p, nsamps, nchans, row_bytes, ld_src, dst, ld_dst, nct); break;
    case 2: launch_unpack_transpose<2>(w, grid, s, p, nsamps, nchans, row_bytes, ld_src, dst, ld_dst, nct); break;
    default: launch_unpack_transpose<4>(w, grid, s, p, nsamps, nchans, row_bytes, ld_src, dst, ld_dst, nct); break;
    }
    return pu::launch_check("unpack_transpose_kernel");
}

int pu_transpose(const void *src, int elem_bytes, int64_t rows, int64_t cols, int64_t ld_src, void *dst,
                 int64_t ld_dst, void *stream)
{
    PU_REQUIRE(src && dst && rows >= 0 && cols >= 0 && ld_src >= cols && ld_dst >= rows,
               "pu_transpose: bad arguments");
    if (rows == 0 || cols == 0) return PU_OK;
    PU_REQUIRE((rows + 63) / 64 < 65536, "pu_transpose: too many rows");
    const dim3 g((unsigned)((cols + 63) / 64), (unsigned)((rows + 63) / 64)), b(256);
    hipStream_t s = pu::as_stream(stream);
    switch (elem_bytes) {
    case 1: hipLaunchKernelGGL(transpose_kernel<uint8_t>, g, b, 0, s, (const uint8_t *)src, rows, cols, ld_src, (uint8_t *)dst, ld_dst); break;
    case 2: hipLaunchKernelGGL(transpose_kernel<uint16_t>, g, b, 0, s, (const uint16_t *)src, rows, cols, ld_src, (uint16_t *)dst, ld_dst); break;
    case 4: hipLaunchKernelGGL(transpose_kernel<uint32_t>, g, b, 0, s, (const uint32_t *)src, rows, cols, ld_src, (uint32_t *)dst, ld_dst); break;
    case 8: hipLaunchKernelGGL(transpose_kernel<uint64_t>, g, b, 0, s, (const uint64_t *)src, rows, cols, ld_src, (uint64_t *)dst, ld_dst); break;
    default: pu::set_error("pu_transpose: element size %d unsupported", elem_bytes); return PU_EUNSUPPORTED;
    }
    return pu::launch_check("transpose_kernel");
}


int pu_rebin_time(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, int64_t w, double *out,
                  void *stream)
{
    PU_REQUIRE(x && out && nrows > 0 && n > 0 && ld >= n && w > 0, "pu_rebin_time: bad arguments");
    PU_REQUIRE(nrows < 65536, "pu_rebin_time: at most 65535 rows");
    const int64_t nout = n / w;
    if (nout == 0) return PU_OK;
    const dim3 g(nblocks(nout, 256), (unsigned)nrows), b(256);
    hipStream_t s = pu::as_stream(stream);
    switch (dtype) {
    case PU_U8: hipLaunchKernelGGL(rebin_time_kernel<uint8_t>, g, b, 0, s, (const uint8_t *)x, nrows, nout, ld, w, out); break;
    case PU_F32: hipLaunchKernelGGL(rebin_time_kernel<float>, g, b, 0, s, (const float *)x, nrows, nout, ld, w, out); break;
    case PU_F64: hipLaunchKernelGGL(rebin_time_kernel<double>, g, b, 0, s, (const double *)x, nrows, nout, ld, w, out); break;
    case PU_I64: hipLaunchKernelGGL(rebin_time_kernel<int64_t>, g, b, 0, s, (const int64_t *)x, nrows, nout, ld, w, out); break;
    default: pu::set_error("pu_rebin_time: unsupported dtype %d", dtype); return PU_EUNSUPPORTED;
    }
    return pu::launch_check("rebin_time_kernel");
}

int pu_rebin_chan(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, int64_t rb, void *out, void *stream)
{
    PU_REQUIRE(x && out && nrows > 0 && n > 0 && ld >= n && rb > 0, "pu_rebin_chan: bad arguments");
    const int64_t ng = nrows / rb;
    if (ng == 0) return PU_OK;
    PU_REQUIRE(ng < 65536, "pu_rebin_chan: at most 65535 output rows");
    const dim3 g(nblocks(n, 256), (unsigned)ng), b(256);
    hipStream_t s = pu::as_stream(stream);
    switch (dtype) {
    case PU_U8: hipLaunchKernelGGL((rebin_chan_kernel<uint8_t, uint64_t>), g, b, 0, s, (const uint8_t *)x, n, ld, rb, (uint64_t *)out); break;
    case PU_F32: hipLaunchKernelGGL((rebin_chan_kernel<float, float>), g, b, 0, s, (const float *)x, n, ld, rb, (float *)out); break;
    case PU_F64: hipLaunchKernelGGL((rebin_chan_kernel<double, double>), g, b, 0, s, (const double *)x, n, ld, rb, (double *)out); break;
    case PU_I64: hipLaunchKernelGGL((rebin_chan_kernel<int64_t, int64_t>), g, b, 0, s, (const int64_t *)x, n, ld, rb, (int64_t *)out); break;
    default: pu::set_error("pu_rebin_chan: unsupported dtype %d", dtype); return PU_EUNSUPPORTED;
    }
    return pu::launch_check("rebin_chan_kernel");
}

int pu_roll_rows(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, const int64_t *shifts, void *out,
                 void *stream)
{
    PU_REQUIRE(x && out && shifts && nrows > 0 && n > 0 && ld >= n, "pu_roll_rows: bad arguments");
    PU_REQUIRE(nrows < 65536, "pu_roll_rows: at most 65535 rows");
    const dim3 g(nblocks(n, 256), (unsigned)nrows), b(256);
    hipStream_t s = pu::as_stream(stream);
    switch (pu::elem_size(dtype)) {
    case 1: hipLaunchKernelGGL(roll_rows_kernel<uint8_t>, g, b, 0, s, (const uint8_t *)x, n, ld, shifts, (uint8_t *)out); break;
    case 4: hipLaunchKernelGGL(roll_rows_kernel<uint32_t>, g, b, 0, s, (const uint32_t *)x, n, ld, shifts, (uint32_t *)out); break;
    case 8: hipLaunchKernelGGL(roll_rows_kernel<uint64_t>, g, b, 0, s, (const uint64_t *)x, n, ld, shifts, (uint64_t *)out); break;
    default: pu::set_error("pu_roll_rows: unsupported dtype %d", dtype); return PU_EUNSUPPORTED;
    }
    return pu::launch_check("roll_rows_kernel");
}

int pu_roll_and_sum(const void *x, int dtype, int64_t n, int64_t roll, double *sum, void *stream)
{
    PU_REQUIRE(x && sum && n > 0, "pu_roll_and_sum: bad arguments");
    PU_REQUIRE(roll >= 0 && roll < n, "pu_roll_and_sum: roll %lld outside [0, %lld)", (long long)roll, (long long)n);
    const dim3 g(nblocks(n, 256)), b(256);
    hipStream_t s = pu::as_stream(stream);
    switch (dtype) {
    case PU_U8: hipLaunchKernelGGL(roll_and_sum_kernel<uint8_t>, g, b, 0, s, (const uint8_t *)x, n, roll, sum); break;
    case PU_F32: hipLaunchKernelGGL(roll_and_sum_kernel<float>, g, b, 0, s, (const float *)x, n, roll, sum); break;
    case PU_F64: hipLaunchKernelGGL(roll_and_sum_kernel<double>, g, b, 0, s, (const double *)x, n, roll, sum); break;
    case PU_I64: hipLaunchKernelGGL(roll_and_sum_kernel<int64_t>, g, b, 0, s, (const int64_t *)x, n, roll, sum); break;
    default: pu::set_error("pu_roll_and_sum: unsupported dtype %d", dtype); return PU_EUNSUPPORTED;
    }
    return pu::launch_check("roll_and_sum_kernel");
}

}  // extern "C"
