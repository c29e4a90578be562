// Rebinning and roll helpers (HBM-streaming kernels) for gfx950.
//
//   pu_rebin_time   <- quick_resample           pulsarutils/dedispersion.py:38-57
//   pu_rebin_chan   <- quick_chan_rebin         :15-35
//   pu_roll_rows    <- apply_dm_shifts_to_data  :254-258
//   pu_roll_and_sum <- roll_and_sum             :60-83
//   pu_transpose    <- the (nsamps, nchans) -> (nchans, nsamps) transpose sigpyproc's
//                      readBlock performs (clean.py:327, stats.py:45)
//   pu_unpack_transpose <- the same for 1/2/4-bit files: sigpyproc's unpack + transpose
//   pu_quantize_pack_transpose <- the array step of cleanup_data (clean.py:354-356, a stub
//                      in the reference): requantise + transpose + pack, the way back
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

// Channel-major samples -> quantised, packed, time-major rows: the mirror image of
// unpack_transpose_kernel.  One workgroup makes QP_TT rows of QP_TC * nbits / 8 packed bytes
// from a tile of QP_TC channels x QP_TT samples.  The kernel is bound by the src read (8, 4
// or 1 bytes per sample against nbits / 8 written), so the tile is laid out for the load:
//   1. a lane reads E consecutive samples (one 16-byte piece: 2 doubles, 4 floats, 16 bytes,
//      when src and ld_src allow it; narrower pieces otherwise) of each of 4 consecutive
//      channel rows - four independent loads, and the lanes of a wave walk along time, so
//      for float64 one wave-instruction reads the tile's whole 1 KiB of a channel row - and
//      quantises them in registers (float64 multiply, add, rint, clamp: ~1.25 samples per
//      clock and CU at the HBM rate, an eighth of the float64 rate).  The four channels'
//      bytes of one sample make one dword, stored to LDS time-major, q[time][channel]: the
//      LDS holds the QUANTISED tile (16.5 KiB, so 8 workgroups fit a CU and the load of one
//      hides the packing of another) and takes a quarter of the stores byte writes would;
//   2. a lane reads the 16 channel bytes of one sample as four dwords, folds each dword's
//      four values into 4 * nbits bits with two shift-or-mask steps, and stores the
//      2 * nbits bytes along the dst row with one store when dst and ld_dst are aligned to
//      it (byte by byte otherwise, or where the row ends inside the piece): 8 lanes cover
//      the tile's 16 * nbits contiguous bytes of a dst row.  Tiles are numbered channel-tile
//      first, so the workgroups that complete a dst row run together.
// The row pitch of q is QP_TC + 4 bytes: one bank off per sample.  The dword stores of a
// wave's 32-lane half then hit 32 / E banks E-fold (E = 2, float64: free on ds_write_b32;
// E = 4, float32: twice the cycles, against half the HBM bytes; 8-bit input pays 16-fold and
// is bound by these stores, not by its 1-byte reads), and the dword reads of step 2 (4
// samples x 8 channel groups per half) are conflict-free.  The pitch is no multiple of 16,
// so step 2 reads dwords, not b128: 64 wave-reads per tile, nothing beside the loads.
// The scale and offset of the tile's channels are staged in LDS once (a broadcast read per
// channel quad instead of two more global loads per row).
constexpr int QP_TT = 128, QP_TC = 128, QP_PITCH = QP_TC + 4;

template <typename T, int E> struct alignas(sizeof(T) * E) qp_piece { T v[E]; };

template <typename T>
__device__ __forceinline__ double qp_value(T x, double s, double o, bool ident)
{
    const double v = static_cast<double>(x);
    return ident ? v : v * s + o;  // (two roundings: the build has no FMA contraction)
}

// min(max(rint(v), 0), top) with a NaN replaced by ``nanv`` first (fmax drops a NaN nanv to 0)
__device__ __forceinline__ uint32_t qp_quant(double v, double nanv, double top)
{
    if (v != v) v = nanv;
    return static_cast<uint32_t>(fmin(fmax(rint(v), 0.0), top));
}

// the four values (< 2^NBITS) in the bytes of w, lowest first -> 4 * NBITS bits
template <int NBITS>
__device__ __forceinline__ uint32_t qp_fold(uint32_t w)
{
    if (NBITS == 8) return w;
    const uint32_t y = (w | (w >> (8 - NBITS))) & (((1u << (2 * NBITS)) - 1u) * 0x00010001u);
    return (y | (y >> (16 - 2 * NBITS))) & ((1u << (4 * NBITS)) - 1u);
}

template <int NBITS>
__device__ __forceinline__ void qp_pack_store(const uint8_t *q, int64_t t0, int64_t nsamps, int64_t b0,
                                              int64_t row_bytes, uint8_t *__restrict__ dst, int64_t ld_dst, int dalign)
{
    constexpr int S = 2 * NBITS;  // packed bytes of 16 channels
    for (int item = threadIdx.x; item < QP_TT * (QP_TC / 16); item += 256) {
        const int cg = item % (QP_TC / 16), tl = item / (QP_TC / 16);
        const int64_t t = t0 + tl, b = b0 + cg * S;
        if (t >= nsamps || b >= row_bytes) continue;
        const uint32_t *r = reinterpret_cast<const uint32_t *>(q + tl * QP_PITCH + cg * 16);
        uint32_t o[4];
        if (NBITS == 8) {
            o[0] = r[0], o[1] = r[1], o[2] = r[2], o[3] = r[3];
        } else {
            const uint64_t acc = (uint64_t)qp_fold<NBITS>(r[0]) | ((uint64_t)qp_fold<NBITS>(r[1]) << (4 * NBITS))
                                 | ((uint64_t)qp_fold<NBITS>(r[2]) << (8 * NBITS))
                                 | ((uint64_t)qp_fold<NBITS>(r[3]) << (12 * NBITS));
            o[0] = (uint32_t)acc, o[1] = (uint32_t)(acc >> 32), o[2] = o[3] = 0;
        }
        uint8_t *d = dst + t * ld_dst + b;
        if (b + S <= row_bytes && dalign >= S) {
            if (S == 16) *reinterpret_cast<uint4 *>(d) = make_uint4(o[0], o[1], o[2], o[3]);
            else if (S == 8) *reinterpret_cast<uint2 *>(d) = make_uint2(o[0], o[1]);
            else if (S == 4) *reinterpret_cast<uint32_t *>(d) = o[0];
            else *reinterpret_cast<uint16_t *>(d) = (uint16_t)o[0];
        } else {
#pragma unroll
            for (int k = 0; k < S; ++k)
                if (b + k < row_bytes) d[k] = (uint8_t)(o[k / 4] >> (8 * (k % 4)));
        }
    }
}

template <typename T, int E>
__global__ void __launch_bounds__(256) quantize_pack_kernel(const T *__restrict__ src, int64_t nchans, int64_t nsamps,
                                                            int64_t ld_src, const double *__restrict__ scale,
                                                            const double *__restrict__ offset, int nbits,
                                                            uint8_t *__restrict__ dst, int64_t ld_dst, int64_t row_bytes,
                                                            int64_t nct, int dalign)
{
    constexpr int PPR = QP_TT / E;  // pieces per tile row
    __shared__ __attribute__((aligned(16))) uint8_t q[QP_TT * QP_PITCH];
    __shared__ double sc[QP_TC], of[QP_TC];
    const int64_t bid = blockIdx.x, ct = bid % nct;
    const int64_t t0 = (bid / nct) * QP_TT, c0 = ct * QP_TC;
    const bool ident = scale == nullptr;
    const double top = (double)((1u << nbits) - 1u);

    if (threadIdx.x < QP_TC) {
        const int64_t c = c0 + threadIdx.x;
        const bool ok = !ident && c < nchans;
        sc[threadIdx.x] = ok ? scale[c] : 1.0;
        of[threadIdx.x] = ok ? offset[c] : 0.0;
    }
    __syncthreads();

    uint32_t *qw = reinterpret_cast<uint32_t *>(q);
    if (c0 + QP_TC <= nchans && t0 + QP_TT <= nsamps) {
#pragma unroll 4
        for (int item = threadIdx.x; item < (QP_TC / 4) * PPR; item += 256) {
            const int cq = item / PPR, tl = (item % PPR) * E;
            const T *p = src + (c0 + 4 * cq) * ld_src + t0 + tl;
            qp_piece<T, E> v[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) v[j] = *reinterpret_cast<const qp_piece<T, E> *>(p + j * ld_src);
            uint32_t w[E];
#pragma unroll
            for (int k = 0; k < E; ++k) w[k] = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const double s = sc[4 * cq + j], o = of[4 * cq + j];
#pragma unroll
                for (int k = 0; k < E; ++k) w[k] |= qp_quant(qp_value(v[j].v[k], s, o, ident), o, top) << (8 * j);
            }
#pragma unroll
            for (int k = 0; k < E; ++k) qw[((tl + k) * QP_PITCH) / 4 + cq] = w[k];
        }
    } else {
        // a tile on the edge: element by element, zeros outside (never stored to dst)
        for (int item = threadIdx.x; item < (QP_TC / 4) * QP_TT; item += 256) {
            const int cq = item / QP_TT, tl = item % QP_TT;
            const int64_t t = t0 + tl;
            uint32_t w = 0;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int64_t c = c0 + 4 * cq + j;
                if (c < nchans && t < nsamps) {
                    const double o = of[4 * cq + j];
                    w |= qp_quant(qp_value(src[c * ld_src + t], sc[4 * cq + j], o, ident), o, top) << (8 * j);
                }
            }
            qw[(tl * QP_PITCH) / 4 + cq] = w;
        }
    }
    __syncthreads();

    const int64_t b0 = ct * (QP_TC / 8) * nbits;
    switch (nbits) {
    case 1: qp_pack_store<1>(q, t0, nsamps, b0, row_bytes, dst, ld_dst, dalign); break;
    case 2: qp_pack_store<2>(q, t0, nsamps, b0, row_bytes, dst, ld_dst, dalign); break;
    case 4: qp_pack_store<4>(q, t0, nsamps, b0, row_bytes, dst, ld_dst, dalign); break;
    default: qp_pack_store<8>(q, t0, nsamps, b0, row_bytes, dst, ld_dst, dalign); break;
    }
}

// nbits 32: dst[t][c] = (float)v, 64x64 tiles through LDS as transpose_kernel (rows of dst
// are ld_dst BYTES apart).
template <typename T>
__global__ void __launch_bounds__(256) scale_transpose_f32_kernel(const T *__restrict__ src, int64_t nchans,
                                                                  int64_t nsamps, int64_t ld_src,
                                                                  const double *__restrict__ scale,
                                                                  const double *__restrict__ offset,
                                                                  uint8_t *__restrict__ dst, int64_t ld_dst, int64_t nct)
{
    __shared__ float tile[64][65];
    const int64_t bid = blockIdx.x;
    const int64_t c0 = (bid % nct) * 64, t0 = (bid / nct) * 64;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;
    const bool ident = scale == nullptr;
    for (int i = ty; i < 64; i += 4) {
        const int64_t c = c0 + i, t = t0 + tx;
        if (c < nchans && t < nsamps)
            tile[i][tx] = static_cast<float>(qp_value(src[c * ld_src + t], ident ? 1.0 : scale[c],
                                                      ident ? 0.0 : offset[c], ident));
    }
    __syncthreads();
    for (int i = ty; i < 64; i += 4) {
        const int64_t t = t0 + i, c = c0 + tx;
        if (c < nchans && t < nsamps) *reinterpret_cast<float *>(dst + t * ld_dst + 4 * c) = tile[tx][i];
    }
}

}  // namespace

extern "C" {

int pu_quantize_pack_transpose(const void *src, int dtype, int64_t nchans, int64_t nsamps, int64_t ld_src,
                               const double *scale, const double *offset, int nbits, void *dst, int64_t ld_dst,
                               void *stream)
{
    if (nbits != 1 && nbits != 2 && nbits != 4 && nbits != 8 && nbits != 32) {
        pu::set_error("pu_quantize_pack_transpose: nbits %d unsupported (1, 2, 4, 8, 32)", nbits);
        return PU_EUNSUPPORTED;
    }
    return pu::with_dtype<uint8_t, float, double>("pu_quantize_pack_transpose", dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        PU_REQUIRE(src && dst && nsamps >= 0 && nchans >= 0 && nchans <= INT64_MAX / 32,
                   "pu_quantize_pack_transpose: bad arguments");
        PU_REQUIRE((scale == nullptr) == (offset == nullptr),
                   "pu_quantize_pack_transpose: scale and offset go together (both, or both NULL for identity)");
        PU_REQUIRE(nchans * nbits % 8 == 0,
                   "pu_quantize_pack_transpose: nchans %lld x nbits %d is not a whole number of bytes", (long long)nchans,
                   nbits);
        const int64_t row_bytes = nchans * nbits / 8;
        PU_REQUIRE(ld_src >= nsamps && ld_dst >= row_bytes,
                   "pu_quantize_pack_transpose: leading dimension too small (ld_src %lld < %lld samples or ld_dst %lld < "
                   "%lld row bytes)", (long long)ld_src, (long long)nsamps, (long long)ld_dst, (long long)row_bytes);
        const uintptr_t esize = sizeof(T);
        const uintptr_t sa = reinterpret_cast<uintptr_t>(src), da = reinterpret_cast<uintptr_t>(dst);
        PU_REQUIRE(sa % esize == 0, "pu_quantize_pack_transpose: src is not aligned to its element type");
        PU_REQUIRE(nbits != 32 || ((da | static_cast<uintptr_t>(ld_dst)) % 4 == 0),
                   "pu_quantize_pack_transpose: float32 rows need dst and ld_dst in multiples of 4 bytes");
        if (nsamps == 0 || nchans == 0) return PU_OK;
        const int tc = nbits == 32 ? 64 : QP_TC, tt = nbits == 32 ? 64 : QP_TT;
        const int64_t nct = (nchans + tc - 1) / tc, ntt = (nsamps + tt - 1) / tt;
        PU_REQUIRE(ntt <= INT32_MAX / nct, "pu_quantize_pack_transpose: %lld x %lld tiles exceed the grid limit",
                   (long long)ntt, (long long)nct);
        const unsigned grid = (unsigned)(nct * ntt);
        hipStream_t s = pu::as_stream(stream);
        const T *p = static_cast<const T *>(src);
        uint8_t *d = static_cast<uint8_t *>(dst);
        if (nbits == 32)
            return pu::launch("scale_transpose_f32_kernel", scale_transpose_f32_kernel<T>, dim3(grid), dim3(256), 0, s, p, nchans,
                              nsamps, ld_src, scale, offset, d, ld_dst, nct);
        // the widest piece that src and every row start are aligned to; the widest store dst allows
        const uintptr_t a = sa | (static_cast<uintptr_t>(ld_src) * esize);
        const int w = a % 16 == 0 ? 16 : a % 4 == 0 ? 4 : 1;
        const uintptr_t ad = da | static_cast<uintptr_t>(ld_dst);
        const int dalign = ad % 16 == 0 ? 16 : ad % 8 == 0 ? 8 : ad % 4 == 0 ? 4 : ad % 2 == 0 ? 2 : 1;
        // E elements per piece: 16 bytes' worth, for 8-bit input 4 bytes' worth too, else 1
        auto go = [&](auto e) {
            return pu::launch("quantize_pack_kernel", quantize_pack_kernel<T, decltype(e)::value>, dim3(grid), dim3(256), 0, s, p,
                              nchans, nsamps, ld_src, scale, offset, nbits, d, ld_dst, row_bytes, nct, dalign);
        };
        if (w == 16) return go(std::integral_constant<int, 16 / sizeof(T)>{});
        if constexpr (sizeof(T) == 1)
            if (w == 4) return go(std::integral_constant<int, 4>{});
        return go(std::integral_constant<int, 1>{});
    });
}

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
    return pu::with_dtype<uint8_t, float, double, int64_t>("pu_rebin_time", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return pu::launch("rebin_time_kernel", rebin_time_kernel<T>, g, b, 0, s, (const T *)x, nrows, nout, ld, w, out);
    });
}

int pu_rebin_chan(const void *x, int dtype, int64_t nrows, int64_t n, int64_t ld, int64_t rb, void *out, void *stream)
{
    PU_REQUIRE(x && out && nrows > 0 && n > 0 && ld >= n && rb > 0, "pu_rebin_chan: bad arguments");
    const int64_t ng = nrows / rb;
    if (ng == 0) return PU_OK;
    PU_REQUIRE(ng < 65536, "pu_rebin_chan: at most 65535 output rows");
    const dim3 g(nblocks(n, 256), (unsigned)ng), b(256);
    hipStream_t s = pu::as_stream(stream);
    return pu::with_dtype<uint8_t, float, double, int64_t>("pu_rebin_chan", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        // 8-bit rows sum to uint64, every other type to itself
        using To = std::conditional_t<std::is_same_v<T, uint8_t>, uint64_t, T>;
        return pu::launch("rebin_chan_kernel", rebin_chan_kernel<T, To>, g, b, 0, s, (const T *)x, n, ld, rb, (To *)out);
    });
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
    return pu::with_dtype<uint8_t, float, double, int64_t>("pu_roll_and_sum", dtype, [&](auto tag) {
        using T = typename decltype(tag)::type;
        return pu::launch("roll_and_sum_kernel", roll_and_sum_kernel<T>, g, b, 0, s, (const T *)x, n, roll, sum);
    });
}

}  // extern "C"
