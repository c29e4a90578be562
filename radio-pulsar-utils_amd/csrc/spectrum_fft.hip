// Real-to-complex FFT of dedispersed series for gfx950: pu_rfft, and the acceleration search's
// pu_resample_accel and pu_rfft_accel (include/pulsarutils_hip.h).
//
// A row of nfft real samples is packed as M = nfft / 2 complex ones, z[j] = y[2j] + i y[2j+1]; the
// complex transform Z of length M runs in LDS and a split step turns Z into the real-input
// spectrum.  The mean subtraction, the float64 -> float32 rounding and the zero padding happen
// where the first pass loads its samples.
//
//   M <= 4096 (nfft <= 2^13): one pass.  A workgroup loads the row, transforms it, and writes Z in
//       natural order into the output row.
//   above: four-step, M = N1 x N2 with N1 = 2^floor(log2 M / 2) <= N2 <= 4096, j = j1 N2 + j2,
//       k = k1 + N1 k2:
//         pass 1 (rfft_cols_kernel): a workgroup owns C = 8192 / N1 consecutive columns j2, laid
//           out in LDS [j1][c] (c fastest: a butterfly's lanes are contiguous, no bank conflict
//           while C h >= 32); transforms over j1, multiplies by W_M^(j2 k1) and writes
//           T[k1][j2] to the workspace (segments of C x 8 bytes);
//         pass 2 (rfft_rows_kernel): a workgroup owns R = 8192 / N2 consecutive rows k1 of T, laid
//           out [r][N2 + 1] (the odd pitch spreads the transposing read-out over the banks);
//           transforms over j2 and writes Z[k1 + N1 k2] into the output row (segments of R x 8
//           bytes).
//   split (rfft_split_kernel), in place in the output row: thread j <= M / 2 reads Z[j] and
//       Z[M - j] and writes X[j] and X[M - j];  X[k] = E + W^k O with E = (Z[k] + conj Z[M-k]) / 2,
//       O = -i (Z[k] - conj Z[M-k]) / 2, W = e^(-2 pi i / nfft), Z[M] = Z[0].
//
// The LDS transform is radix-2 decimation in frequency, in place, natural order in and
// bit-reversed order out (the write-out undoes it): log2 N stages with a barrier each.  Stage
// twiddles come from an LDS copy of W_N^j (j < N / 2), itself read from the table W_nfft^k
// (k < nfft / 2) that rfft_twiddle_kernel makes at the start of the workspace with float64
// sincospi rounded once to float32.  No fused multiply-add (-ffp-contract=off), no atomics, and
// every operation's order is fixed by nfft: a row's bits depend on nothing but its samples.
//
// Acceleration trials: pu_rfft_accel transforms nacc x rows virtual rows, v = a rows + r, that
// exist nowhere in memory.  The kernels that load samples take a map (RfPlain, RfAccel) that says
// which row of x a virtual row reads and where in it sample t lies: accel_src(t, n, afac[a]), the
// nearest-neighbour index of the time-domain resampling.  Everything after the load is the code
// above, so the spectrum has the bits of pu_rfft on the series pu_resample_accel writes (the same
// accel_src, as a plain gather).  The map is near the identity (|src - t| <= n / 4 over a whole
// row, a step of one now and then), so a wave's loads stay contiguous but for those steps.
//
// LDS per workgroup: 8192 complex64 of data (64 KiB, + R pads) + N / 2 twiddles (<= 16 KiB):
// at most 82 KiB of the CU's 160 KiB.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pu_common.h"

namespace {

constexpr int RF_TILE = 8192;    // complex elements of a workgroup's LDS tile
constexpr int RF_THREADS = 512;  // 8 waves
constexpr int RF_MAX_LOG = 12;   // longest LDS transform: 4096

struct RfShape {
    int lm, l1, l2;  // log2 of M, N1, N2 (l1 = 0: one pass)
    int lc, lr;      // log2 of the columns (pass 1) / rows (pass 2) of a workgroup
};

RfShape rf_shape(int64_t nfft)
{
    RfShape s{};
    int lg = 0;
    while (((int64_t)1 << lg) < nfft) ++lg;
    s.lm = lg - 1;
    if (s.lm <= RF_MAX_LOG) {
        s.l1 = 0, s.l2 = s.lm, s.lc = 0, s.lr = 0;
    } else {
        s.l1 = s.lm / 2, s.l2 = s.lm - s.l1;
        s.lc = 13 - s.l1, s.lr = 13 - s.l2;
    }
    return s;
}

__device__ __forceinline__ float2 cmul(float2 a, float2 w)
{
    return make_float2(a.x * w.x - a.y * w.y, a.x * w.y + a.y * w.x);
}

// tbl[k] = e^(-2 pi i k / nfft), k < nfft / 2: float64 sincospi, rounded once
__global__ void rfft_twiddle_kernel(float2 *__restrict__ tbl, int64_t nfft)
{
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nfft / 2) return;
    double sn, cs;
    sincospi(2.0 * (double)k / (double)nfft, &sn, &cs);  // 2 k / nfft is exact
    tbl[k] = make_float2((float)cs, (float)-sn);
}

// W_nfft^e for 0 <= e < nfft from the half table
__device__ __forceinline__ float2 rf_tw(const float2 *__restrict__ tbl, int e, int half)
{
    if (e < half) return tbl[e];
    const float2 w = tbl[e - half];
    return make_float2(-w.x, -w.y);
}

// In-place radix-2 DIF of 2^lv vectors of 2^ln elements in LDS.  COLS: element i of vector c at
// s[(i << lv) + c]; otherwise at s[c * ((1 << ln) + 1) + i].  tw[j] = W_N^j, j < N / 2.
template <bool COLS>
__device__ __forceinline__ void rf_lds_fft(float2 *s, const float2 *tw, int ln, int lv)
{
    const int half = 1 << (ln - 1), work = half << lv, pitch = (1 << ln) + 1;
    for (int st = 0; st < ln; ++st) {
        const int lh = ln - 1 - st, h = 1 << lh;
        __syncthreads();
        for (int w = threadIdx.x; w < work; w += blockDim.x) {
            const int c = COLS ? w & ((1 << lv) - 1) : w >> (ln - 1);
            const int b = COLS ? w >> lv : w & (half - 1);
            const int p = b & (h - 1), i0 = ((b >> lh) << (lh + 1)) + p, i1 = i0 + h;
            const int a0 = COLS ? (i0 << lv) + c : c * pitch + i0;
            const int a1 = COLS ? (i1 << lv) + c : c * pitch + i1;
            const float2 u = s[a0], v = s[a1];
            s[a0] = make_float2(u.x + v.x, u.y + v.y);
            s[a1] = cmul(make_float2(u.x - v.x, u.y - v.y), tw[p << st]);
        }
    }
    __syncthreads();
}

// Sample i of a series of n resampled at the factor af = accel * sample_time / (2 c) is sample
// i + s of the input: s = rint(af i (i - n)) (ties to even), clamped so that 0 <= i + s <= n - 1
// for every af (fmax and fmin drop a NaN: src = 0).  i (i - n) is exact in int64 and in float64
// for n <= 2^24; one float64 product (no FMA: there is nothing to fuse), one rint.
__device__ __forceinline__ int64_t accel_src(int64_t i, int64_t n, double af)
{
    const double q = af * (double)(i * (i - n));
    const double s = fmin(fmax(rint(q), -(double)i), (double)(n - 1 - i));
    return i + (int64_t)s;
}

// Where the first pass finds sample t of its row v.  RfPlain (pu_rfft): row v of x, sample t.
struct RfPlain {
    struct Row {
        int64_t r;
        __device__ __forceinline__ int64_t src(int64_t t) const { return t; }
    };
    __device__ __forceinline__ Row row(int64_t v, int64_t) const { return Row{v}; }
};

// RfAccel (pu_rfft_accel): virtual row v = a rows + r reads row r of x at accel_src(t, n, afac[a])
struct RfAccel {
    const double *afac;
    int64_t rows;
    struct Row {
        int64_t r, n;
        double af;
        __device__ __forceinline__ int64_t src(int64_t t) const { return accel_src(t, n, af); }
    };
    __device__ __forceinline__ Row row(int64_t v, int64_t n) const { return Row{v % rows, n, afac[v / rows]}; }
};

// z[j] of a row: the packed, mean-subtracted, float32-rounded, zero-padded samples 2j, 2j + 1
template <typename T, typename ROW>
__device__ __forceinline__ float2 rf_sample(const T *__restrict__ row, int64_t n, double mu, int64_t j, const ROW &m)
{
    const int64_t t = 2 * j;
    const float a = t < n ? (float)((double)row[m.src(t)] - mu) : 0.0f;
    const float b = t + 1 < n ? (float)((double)row[m.src(t + 1)] - mu) : 0.0f;
    return make_float2(a, b);
}

__device__ __forceinline__ int rf_brev(int i, int ln) { return (int)(__brev((unsigned)i) >> (32 - ln)); }

// pass 1 of the four-step: columns j2 of z (N1 x N2) -> T[k1][j2] W_M^(j2 k1)
template <typename T, typename MAP>
__global__ void __launch_bounds__(RF_THREADS)
rfft_cols_kernel(const T *__restrict__ x, int64_t n, int64_t ld, const double *__restrict__ mean, RfShape sh,
                 const float2 *__restrict__ tbl, float2 *__restrict__ tws, MAP map)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rf_smem[];
    float2 *s = reinterpret_cast<float2 *>(rf_smem);  // [N1][C]
    float2 *tw = s + RF_TILE;                          // [N1 / 2]
    const int n1 = 1 << sh.l1, n2 = 1 << sh.l2, cmask = (1 << sh.lc) - 1, half = 1 << sh.lm;
    const int groups = n2 >> sh.lc;
    const int64_t r = blockIdx.x / groups;
    const int j20 = (int)(blockIdx.x % groups) << sh.lc;
    const auto m = map.row(r, n);
    const T *row = x + m.r * ld;
    const double mu = mean ? mean[m.r] : 0.0;
    for (int j = threadIdx.x; j < n1 / 2; j += blockDim.x) tw[j] = tbl[(int64_t)j << (sh.lm + 1 - sh.l1)];
    for (int w = threadIdx.x; w < RF_TILE; w += blockDim.x) {
        const int c = w & cmask, j1 = w >> sh.lc;
        s[w] = rf_sample(row, n, mu, (int64_t)j1 * n2 + j20 + c, m);
    }
    rf_lds_fft<true>(s, tw, sh.l1, sh.lc);
    float2 *dst = tws + r * (int64_t)half;
    for (int w = threadIdx.x; w < RF_TILE; w += blockDim.x) {
        const int c = w & cmask, k1 = rf_brev(w >> sh.lc, sh.l1), j2 = j20 + c;
        dst[(int64_t)k1 * n2 + j2] = cmul(s[w], rf_tw(tbl, 2 * j2 * k1, half));  // 2 j2 k1 < nfft <= 2^24
    }
}

// pass 2 of the four-step (rows k1 of T -> Z[k1 + N1 k2]), or the whole transform of a short row
// (FROM_X: N1 = 1, one row of z per workgroup)
template <typename T, typename MAP, bool FROM_X>
__global__ void __launch_bounds__(RF_THREADS)
rfft_rows_kernel(const T *__restrict__ x, int64_t n, int64_t ld, const double *__restrict__ mean, RfShape sh,
                 const float2 *__restrict__ tbl, const float2 *__restrict__ tws, float2 *__restrict__ spec,
                 int64_t ld_spec, MAP map)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char rf_smem[];
    const int n1 = 1 << sh.l1, n2 = 1 << sh.l2, pitch = n2 + 1, nr = 1 << sh.lr, half = 1 << sh.lm;
    float2 *s = reinterpret_cast<float2 *>(rf_smem);  // [R][N2 + 1]
    float2 *tw = s + nr * pitch;                       // [N2 / 2]
    const int groups = n1 >> sh.lr;
    const int64_t r = blockIdx.x / groups;
    const int k10 = (int)(blockIdx.x % groups) << sh.lr;
    for (int j = threadIdx.x; j < n2 / 2; j += blockDim.x) tw[j] = tbl[(int64_t)j << (sh.lm + 1 - sh.l2)];
    const int total = nr << sh.l2;
    if (FROM_X) {
        const auto m = map.row(r, n);
        const T *row = x + m.r * ld;
        const double mu = mean ? mean[m.r] : 0.0;
        for (int w = threadIdx.x; w < total; w += blockDim.x) s[w] = rf_sample(row, n, mu, w, m);
    } else {
        const float2 *src = tws + r * (int64_t)half + (int64_t)k10 * n2;
        for (int w = threadIdx.x; w < total; w += blockDim.x) s[(w >> sh.l2) * pitch + (w & (n2 - 1))] = src[w];
    }
    rf_lds_fft<false>(s, tw, sh.l2, sh.lr);
    float2 *dst = spec + r * ld_spec;
    for (int w = threadIdx.x; w < total; w += blockDim.x) {
        const int rr = w & (nr - 1), i = w >> sh.lr;
        dst[k10 + rr + (int64_t)n1 * rf_brev(i, sh.l2)] = s[rr * pitch + i];
    }
}

// Z (M values at the start of each output row) -> the nfft / 2 + 1 bins of the real transform
__global__ void __launch_bounds__(256)
rfft_split_kernel(float2 *__restrict__ spec, int64_t ld_spec, int64_t m, const float2 *__restrict__ tbl)
{
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j > m / 2) return;
    float2 *row = spec + (int64_t)blockIdx.y * ld_spec;
    const float2 za = row[j], zb = row[j ? m - j : 0];
    // bin j: Zk = za, Zm = conj(zb); bin m - j: Zk = zb, Zm = conj(za)
    const float2 ea = make_float2(0.5f * (za.x + zb.x), 0.5f * (za.y - zb.y));
    const float2 oa = make_float2(0.5f * (za.y + zb.y), -0.5f * (za.x - zb.x));
    if (j == 0) {
        row[0] = make_float2(ea.x + oa.x, ea.y + oa.y);
        row[m] = make_float2(ea.x - oa.x, ea.y - oa.y);
        return;
    }
    const float2 wa = tbl[j], pa = cmul(oa, wa);
    const float2 xa = make_float2(ea.x + pa.x, ea.y + pa.y);
    if (2 * j == m) {
        row[j] = xa;
        return;
    }
    // W^(m - j) = -conj(W^j)
    const float2 eb = make_float2(ea.x, -ea.y);
    const float2 ob = make_float2(oa.x, -oa.y);
    const float2 pb = cmul(ob, make_float2(-wa.x, wa.y));
    row[j] = xa;
    row[m - j] = make_float2(eb.x + pb.x, eb.y + pb.y);
}

// out[v][i] = x[v % rows][accel_src(i, n, afac[v / rows])]: the resampled series written out.
// grid.y strides over the virtual rows v.
template <typename T>
__global__ void __launch_bounds__(256)
resample_accel_kernel(const T *__restrict__ x, int64_t rows, int64_t n, int64_t ld, const double *__restrict__ afac,
                      int64_t vrows, T *__restrict__ out, int64_t ld_out)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int64_t v = blockIdx.y; v < vrows; v += gridDim.y)
        out[v * ld_out + i] = x[(v % rows) * ld + accel_src(i, n, afac[v / rows])];
}

bool rf_valid_nfft(int64_t nfft) { return nfft >= 256 && nfft <= ((int64_t)1 << 24) && (nfft & (nfft - 1)) == 0; }

// The workspace: the twiddle table of nfft / 2 entries, then (four-step lengths only) the
// first pass's columns, nfft / 2 per row.
struct RfWs {
    float2 *tbl, *tws;
    size_t bytes;
};

RfWs rf_carve(pu::Carver c, int64_t rows, int64_t nfft)
{
    const size_t half = (size_t)(nfft / 2) * sizeof(float2);
    RfWs w;
    w.tbl = c.take<float2>(half);
    w.tws = c.take<float2>(rf_shape(nfft).l1 ? (size_t)rows * half : 0);
    w.bytes = c.used();
    return w;
}

// pu_rfft (MAP = RfPlain) and pu_rfft_accel (RfAccel) over vrows output rows: every check, then
// the launches.  ``who`` names the entry point in the messages.
template <typename MAP>
int rf_transform(const char *who, const void *x, int dtype, int64_t vrows, int64_t n, int64_t ld, const double *mean,
                 int64_t nfft, void *spec, int64_t ld_spec, void *workspace, size_t workspace_bytes, void *stream, MAP map)
{
    // (a dedispersed series is float32 or float64)
    return pu::with_dtype<float, double>(who, dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        PU_REQUIRE(rf_valid_nfft(nfft), "%s: nfft %lld is not a power of two in [2^8, 2^24]", who, (long long)nfft);
        PU_REQUIRE(vrows >= 0 && n >= 0 && n <= nfft, "%s: bad size (rows %lld, n %lld, nfft %lld)", who, (long long)vrows,
                   (long long)n, (long long)nfft);
        PU_REQUIRE(ld >= n && ld_spec >= nfft / 2 + 1, "%s: leading dimension too small (ld %lld < n %lld or ld_spec "
                   "%lld < nfft / 2 + 1)", who, (long long)ld, (long long)n, (long long)ld_spec);
        if (vrows == 0) return PU_OK;
        const RfShape sh = rf_shape(nfft);
        const int64_t m = nfft / 2;
        const int64_t groups = sh.l1 ? ((int64_t)1 << (sh.l1 - sh.lr)) : 1, cgroups = sh.l1 ? ((int64_t)1 << (sh.l2 - sh.lc)) : 1;
        PU_REQUIRE(vrows <= 65535 && vrows <= INT32_MAX / groups && vrows <= INT32_MAX / cgroups,
                   "%s: %lld rows exceed the grid limit (65535 per call)", who, (long long)vrows);
        if (int rc = pu::check_workspace(who, workspace, workspace_bytes, pu_rfft_workspace_bytes(vrows, nfft), 256)) return rc;
        PU_REQUIRE(x && spec, "%s: null pointer", who);
        PU_REQUIRE(reinterpret_cast<uintptr_t>(x) % sizeof(T) == 0 && reinterpret_cast<uintptr_t>(spec) % 8 == 0,
                   "%s: x or spec is not aligned to its element type", who);
        hipStream_t s = pu::as_stream(stream);
        const RfWs w = rf_carve(pu::Carver(workspace), vrows, nfft);
        const T *xs = static_cast<const T *>(x);
        float2 *out = static_cast<float2 *>(spec);
        if (int rc = pu::launch("rfft_twiddle_kernel", rfft_twiddle_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, s,
                                w.tbl, nfft))
            return rc;
        const int n2 = 1 << sh.l2, nr = 1 << sh.lr;
        const size_t lds_rows = ((size_t)nr * (n2 + 1) + n2 / 2) * sizeof(float2);
        if (sh.l1 == 0) {
            if (int rc = pu::launch("rfft_rows_kernel", rfft_rows_kernel<T, MAP, true>, dim3((unsigned)vrows), dim3(RF_THREADS),
                                    lds_rows, s, xs, n, ld, mean, sh, w.tbl, nullptr, out, ld_spec, map))
                return rc;
        } else {
            const size_t lds_cols = ((size_t)RF_TILE + ((size_t)1 << sh.l1) / 2) * sizeof(float2);
            const dim3 cgrid((unsigned)(vrows * cgroups)), rgrid((unsigned)(vrows * groups));
            if (int rc = pu::launch("rfft_cols_kernel", rfft_cols_kernel<T, MAP>, cgrid, dim3(RF_THREADS), lds_cols, s, xs, n, ld,
                                    mean, sh, w.tbl, w.tws, map))
                return rc;
            // the second pass reads the workspace, never x: one instance serves both entry points
            if (int rc = pu::launch("rfft_rows_kernel", rfft_rows_kernel<float, RfPlain, false>, rgrid, dim3(RF_THREADS), lds_rows,
                                    s, nullptr, n, ld, mean, sh, w.tbl, w.tws, out, ld_spec, RfPlain{}))
                return rc;
        }
        return pu::launch("rfft_split_kernel", rfft_split_kernel, dim3((unsigned)((m / 2 + 1 + 255) / 256), (unsigned)vrows),
                          dim3(256), 0, s, out, ld_spec, m, w.tbl);
    });
}

// rows and nacc of an acceleration call: both in [0, 2^31), so that their product is an int64
bool rf_valid_trials(int64_t rows, int64_t nacc) { return rows >= 0 && nacc >= 0 && rows <= INT32_MAX && nacc <= INT32_MAX; }

}  // namespace

extern "C" {

size_t pu_rfft_workspace_bytes(int64_t rows, int64_t nfft)
{
    if (rows <= 0 || !rf_valid_nfft(nfft)) return 0;
    const size_t half = (size_t)(nfft / 2) * sizeof(float2);
    if (rf_shape(nfft).l1 && (size_t)rows > (SIZE_MAX - pu::up256(half)) / half) return SIZE_MAX;
    return rf_carve(pu::Carver(), rows, nfft).bytes;
}

int pu_rfft(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, const double *mean, int64_t nfft, void *spec,
            int64_t ld_spec, void *workspace, size_t workspace_bytes, void *stream)
{
    return rf_transform("pu_rfft", x, dtype, rows, n, ld, mean, nfft, spec, ld_spec, workspace, workspace_bytes, stream,
                        RfPlain{});
}

size_t pu_rfft_accel_workspace_bytes(int64_t rows, int64_t nacc, int64_t nfft)
{
    if (!rf_valid_trials(rows, nacc)) return 0;
    return pu_rfft_workspace_bytes(rows * nacc, nfft);
}

int pu_rfft_accel(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, const double *mean, const double *afac,
                  int64_t nacc, int64_t nfft, void *spec, int64_t ld_spec, void *workspace, size_t workspace_bytes,
                  void *stream)
{
    PU_REQUIRE(rf_valid_trials(rows, nacc), "pu_rfft_accel: bad size (rows %lld, nacc %lld)", (long long)rows,
               (long long)nacc);
    PU_REQUIRE(rows * nacc <= 65535, "pu_rfft_accel: nacc %lld x rows %lld exceed the grid limit (65535 per call)",
               (long long)nacc, (long long)rows);
    PU_REQUIRE(afac || rows * nacc == 0, "pu_rfft_accel: null pointer (afac)");
    PU_REQUIRE(reinterpret_cast<uintptr_t>(afac) % 8 == 0, "pu_rfft_accel: afac is not aligned to its element type");
    return rf_transform("pu_rfft_accel", x, dtype, rows * nacc, n, ld, mean, nfft, spec, ld_spec, workspace,
                        workspace_bytes, stream, RfAccel{afac, rows});
}

int pu_resample_accel(const void *x, int dtype, int64_t rows, int64_t n, int64_t ld, const double *afac, int64_t nacc,
                      void *out, int64_t ld_out, void *stream)
{
    return pu::with_dtype<float, double>("pu_resample_accel", dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        PU_REQUIRE(rf_valid_trials(rows, nacc) && n >= 0 && n <= ((int64_t)1 << 24),
                   "pu_resample_accel: bad size (rows %lld, nacc %lld, n %lld; n <= 2^24)", (long long)rows, (long long)nacc,
                   (long long)n);
        PU_REQUIRE(ld >= n && ld_out >= n, "pu_resample_accel: leading dimension too small (ld %lld or ld_out %lld < n %lld)",
                   (long long)ld, (long long)ld_out, (long long)n);
        const int64_t vrows = rows * nacc;
        if (vrows == 0 || n == 0) return PU_OK;
        PU_REQUIRE(x && afac && out && x != out, "pu_resample_accel: null pointer, or out is x (not in place)");
        PU_REQUIRE(reinterpret_cast<uintptr_t>(x) % sizeof(T) == 0 && reinterpret_cast<uintptr_t>(out) % sizeof(T) == 0 &&
                       reinterpret_cast<uintptr_t>(afac) % 8 == 0,
                   "pu_resample_accel: x, out or afac is not aligned to its element type");
        const dim3 grid((unsigned)((n + 255) / 256), (unsigned)(vrows < 65535 ? vrows : 65535));
        return pu::launch("resample_accel_kernel", resample_accel_kernel<T>, grid, dim3(256), 0, pu::as_stream(stream),
                          static_cast<const T *>(x), rows, n, ld, afac, vrows, static_cast<T *>(out), ld_out);
    });
}

}  // extern "C"
