// Folding at a pulse period and the binned Z^2_n / H-test, for gfx950.
//
//   pu_fold    no reference counterpart: the reference's PulseInfo (clean.py:27-55) holds a
//              folded profile but nothing in it makes one from a filterbank
//   pu_h_test  <- hendrics' h_test on a binned profile, as plot_diagnostics calls it per DM
//              row (clean.py:252-253)
//
// pu_fold.  Sample t of the call falls in bin b(t) (header: three float64 steps, no FMA - this
// unit is built with -ffp-contract=off like the rest).  b(t) is the same for every channel,
// so a workgroup owns FOLD_SEG consecutive samples x TC channels, walks the segment in
// sub-blocks of FOLD_SUB samples whose bins it computes ONCE into LDS, and keeps TC x nbin
// accumulators in LDS.  It writes them as the segment's partial to the workspace;
// fold_combine_kernel adds the partials of a (channel, bin) in segment order into ``sums``.
// FOLD_SEG, FOLD_SUB and the 64-sample group below are compile-time constants and TC only
// selects which workgroup handles a channel, so the order in which a (channel, bin) sum is
// formed depends on the arguments alone: not on the grid, TC or the device.  No
// floating-point atomic anywhere.
//
//   8-bit input (fold_u8_kernel): uint32 LDS accumulators and integer ds_add, exact and
//   order-free.  A lane takes 16 consecutive samples (one 16-byte load when x and ld allow
//   it) and adds each run of equal bins once, so wide bins cost one LDS atomic per lane
//   and piece instead of sixteen 64-way conflicting ones.
//
//   float32 / float64 (fold_float_kernel): a wave owns whole channels of the tile, so no two
//   waves touch one accumulator.  Lane l of a wave holds sample 64 g + l of group g.  The
//   lanes of a maximal run of equal bins are summed by a segmented scan (DPP row shifts inside
//   rows of 16 lanes, then the carries across rows: a fixed tree and no LDS traffic), and the
//   run's last lane adds the run sum to its LDS bin with a plain read-modify-write.  Two runs of ONE group can share a bin only when the phase
//   wraps inside 64 samples (bins narrower than a sample, periods below 64 samples): those
//   runs are ranked in time order and added in rank order, one round per rank (LDS
//   operations of a wave execute in order).  Run starts, last-lane flags and ranks depend on
//   the bins alone, so they are worked out once per sub-block (fold_group_meta) and shared
//   by the tile's channels.
//
// LDS: TC x nbin x 8 bytes (8-bit input: 4 bytes, one pad dword per 32 bins) + 8.1 KiB of tables;
// the choice of TC is fold_tile's (nbin 4096, float: TC = 4, 136 KiB, one workgroup per CU).
// nbin above FOLD_MAX_NBIN = 8192 is PU_EUNSUPPORTED (13 bits of the packed group table).
// Workspace traffic is nseg x nchan x nbin partials, i.e. nbin x 8 / (FOLD_SEG x element
// bytes) of the input: 1/8 at nbin 256 for 8-bit input (uint32 partials: 1/16), which is why
// the segment is long.
//
// pu_h_test.  A table of (cos, sin)(2 pi r / n), r = 0 .. n - 1, by sincospi (workspace), one
// wave per harmonic k summing p[j] cos / sin at the exact integer phase r = k j mod n (kept
// by addition mod n), the powers C_k^2 + S_k^2 to the workspace, then one workgroup per row:
// P, the finite check, and the sequential cumulative sum over k with the running maximum.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pu_common.h"

namespace {

constexpr int FOLD_SEG = 16384;      // samples of a segment (one partial per channel and bin)
constexpr int FOLD_SUB = 2048;       // samples whose bins are staged in LDS at a time
constexpr int FOLD_GROUP = 64;       // samples of a wave's group (float path)
constexpr int FOLD_MAX_NBIN = 8192;  // 13 bits of the packed group table
constexpr int FOLD_NG = FOLD_SUB / FOLD_GROUP;
constexpr int FOLD_BATCH = 8;        // groups a wave loads and scans together
constexpr size_t FOLD_TABLE_BYTES = FOLD_SUB * 4 + FOLD_NG * 4;
constexpr size_t FOLD_LDS_FULL = 20 * 1024, FOLD_LDS_SMALL = 64 * 1024, FOLD_LDS_MAX = 160 * 1024;
static_assert(FOLD_TABLE_BYTES % 16 == 0 && FOLD_SEG % FOLD_SUB == 0 && FOLD_SUB % 16 == 0 && FOLD_SUB % FOLD_GROUP == 0 && FOLD_NG % FOLD_BATCH == 0, "fold tiling");

// the bin rule of the header: every step one IEEE float64 operation (no contraction)
__device__ __forceinline__ int fold_bin(int64_t sample, double phase0, double dphase, int64_t nbin)
{
    const double p = phase0 + (double)sample * dphase;
    const double f = p - floor(p);
    const int64_t b = (int64_t)(f * (double)nbin);
    return (int)(b < nbin - 1 ? b : nbin - 1);
}

// bins of sub-block samples [t0, t0 + FOLD_SUB) of the call into tab; -1 at and beyond tend
__device__ __forceinline__ void fold_stage_bins(int *tab, int64_t t0, int64_t tend, int64_t first_sample, double phase0,
                                                double dphase, int64_t nbin)
{
    for (int i = threadIdx.x; i < FOLD_SUB; i += 256) {
        const int64_t t = t0 + i;
        tab[i] = t < tend ? fold_bin(first_sample + t, phase0, dphase, nbin) : -1;
    }
}

// 8-bit accumulators are padded by one dword per 32 bins: with a power-of-two number of bins
// per 16-sample piece (0.5 samples per bin: 32) the lanes of a wave would otherwise add to
// bins a multiple of 32 dwords apart - one LDS bank, a 64-way conflict
__host__ __device__ __forceinline__ int fold_pad(int b) { return b + (b >> 5); }

template <bool VEC>
__global__ void __launch_bounds__(256) fold_u8_kernel(const uint8_t *__restrict__ x, int64_t nchan, int64_t n, int64_t ld,
                                                      int64_t first_sample, double phase0, double dphase, int64_t nbin,
                                                      int tc, int64_t nct, uint32_t *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fold_smem[];
    int *bins = reinterpret_cast<int *>(fold_smem);                               // [FOLD_SUB]
    uint32_t *acc = reinterpret_cast<uint32_t *>(fold_smem + FOLD_TABLE_BYTES);  // [tc][fold_pad(nbin)]
    const int64_t seg = blockIdx.x / nct, c0 = (blockIdx.x % nct) * tc;
    const int64_t s0 = seg * FOLD_SEG, send = s0 + FOLD_SEG < n ? s0 + FOLD_SEG : n;
    const int pitch = fold_pad((int)nbin), nacc = tc * pitch;
    for (int i = threadIdx.x; i < nacc; i += 256) acc[i] = 0;
    constexpr int PIECES = FOLD_SUB / 16, BATCH = 4;
    const int nitems = tc * PIECES;
    for (int64_t t0 = s0; t0 < send; t0 += FOLD_SUB) {
        __syncthreads();  // the zeroing; the previous sub-block's readers of bins
        fold_stage_bins(bins, t0, send, first_sample, phase0, dphase, nbin);
        __syncthreads();
        for (int base = threadIdx.x; base < nitems; base += 256 * BATCH) {
            // the loads of BATCH pieces first (independent: one latency), then their adds
            uint4 w[BATCH];
            bool ok[BATCH];
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                const int item = base + u * 256;
                const int cl = item / PIECES, q = item % PIECES;
                const int64_t c = c0 + cl, t = t0 + q * 16;
                ok[u] = item < nitems && c < nchan && t < send;
                w[u] = make_uint4(0, 0, 0, 0);
                if (!ok[u]) continue;
                const uint8_t *p = x + c * ld + t;
                if (VEC && t + 16 <= send) {
                    w[u] = *reinterpret_cast<const uint4 *>(p);
                } else {
                    uint8_t v[16];
#pragma unroll
                    for (int k = 0; k < 16; ++k) v[k] = t + k < send ? p[k] : (uint8_t)0;
                    __builtin_memcpy(&w[u], v, 16);
                }
            }
#pragma unroll
            for (int u = 0; u < BATCH; ++u) {
                if (!ok[u]) continue;
                const int item = base + u * 256;
                const int cl = item / PIECES, q = item % PIECES;
                uint8_t v[16];
                __builtin_memcpy(v, &w[u], 16);
                int b[16];
#pragma unroll
                for (int k = 0; k < 16; k += 4) {
                    const int4 bw = *reinterpret_cast<const int4 *>(&bins[q * 16 + k]);
                    b[k] = bw.x, b[k + 1] = bw.y, b[k + 2] = bw.z, b[k + 3] = bw.w;
                }
                uint32_t *a = acc + cl * pitch;
                int cur = b[0];  // (a sample beyond the end has bin -1 and value 0)
                uint32_t s = v[0];
#pragma unroll
                for (int k = 1; k < 16; ++k) {
                    if (b[k] != cur) {
                        if (cur >= 0) atomicAdd(&a[fold_pad(cur)], s);
                        cur = b[k], s = 0;
                    }
                    s += v[k];
                }
                if (cur >= 0) atomicAdd(&a[fold_pad(cur)], s);
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < tc * (int)nbin; i += 256) {
        const int cl = i / (int)nbin, bb = i % (int)nbin;
        if (c0 + cl < nchan) part[(seg * nchan + c0 + cl) * nbin + bb] = acc[cl * pitch + fold_pad(bb)];
    }
}

// packed group table entry: bin [0, 13), run start lane [13, 19), rank [19, 25), "valid last
// lane of a run" bit 25
__device__ __forceinline__ void fold_group_meta(uint32_t *meta, int *gmax, int g, int lane)
{
    const int key = reinterpret_cast<const int *>(meta)[g * FOLD_GROUP + lane];  // bin, or -1 past the end
    const bool valid = key >= 0;
    const unsigned long long vmask = __ballot(valid);
    if (vmask == 0) {  // (wave-uniform)
        meta[g * FOLD_GROUP + lane] = 0;
        if (lane == 0) gmax[g] = -1;
        return;
    }
    const int prev = __shfl_up(key, 1), next = __shfl_down(key, 1);
    const bool hf = lane == 0 || key != prev;
    const bool vt = valid && (lane == 63 || key != next);
    int hd = hf ? lane : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int o = __shfl_up(hd, d);
        if (lane >= d && o > hd) hd = o;
    }
    // the invalid lanes trail the valid ones: lanes 0 .. nv - 1 are valid
    const int nv = __popcll(vmask);
    const unsigned long long desc = __ballot(valid && lane >= 1 && key < prev);
    const int firstkey = __shfl(key, 0), lastkey = __shfl(key, nv - 1);
    int rank = 0, gm = 0;
    // non-decreasing bins with at most one wrap that ends below where it began: the runs'
    // bins are all different.  Anything else: rank the runs of each bin in lane order.
    if (!(desc == 0 || (__popcll(desc) == 1 && lastkey < firstkey))) {
        unsigned long long rem = __ballot(vt);
        while (rem) {
            const int leader = __ffsll((long long)rem) - 1;
            const int kb = __shfl(key, leader);
            const bool mine = vt && key == kb;
            const unsigned long long m = __ballot(mine);
            if (mine) rank = __popcll(m & ((1ull << lane) - 1ull));
            const int cnt = __popcll(m) - 1;
            gm = cnt > gm ? cnt : gm;
            rem &= ~m;
        }
    }
    meta[g * FOLD_GROUP + lane] = (valid ? (uint32_t)key : 0u) | ((uint32_t)hd << 13) | ((uint32_t)rank << 19)
                                  | ((uint32_t)vt << 25);
    if (lane == 0) gmax[g] = gm;
}

// Inclusive sums of ``v`` over the lanes [max(hd, ...), lane] of each lane's run (hd = the
// run's first lane): a Hillis-Steele scan inside each row of 16 lanes by DPP row shifts (no
// LDS traffic), then the carry of a run that crosses a row boundary, row by row, from the
// row's last lane.  A fixed tree: the order depends on the lane layout alone.
template <int CTRL>
__device__ __forceinline__ double fold_dpp(double x)
{
    const int lo = __builtin_amdgcn_update_dpp(0, __double2loint(x), CTRL, 0xF, 0xF, false);
    const int hi = __builtin_amdgcn_update_dpp(0, __double2hiint(x), CTRL, 0xF, 0xF, false);
    return __hiloint2double(hi, lo);
}

__device__ __forceinline__ double fold_lane(double x, int l)
{
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(x), l),
                            __builtin_amdgcn_readlane(__double2loint(x), l));
}

__device__ __forceinline__ double fold_run_scan(double v, int hd, int lane)
{
    const int inrow = lane & 15;
    double u;
    u = fold_dpp<0x111>(v);  // row_shr:1
    if (inrow >= 1 && lane - 1 >= hd) v += u;
    u = fold_dpp<0x112>(v);  // row_shr:2
    if (inrow >= 2 && lane - 2 >= hd) v += u;
    u = fold_dpp<0x114>(v);  // row_shr:4
    if (inrow >= 4 && lane - 4 >= hd) v += u;
    u = fold_dpp<0x118>(v);  // row_shr:8
    if (inrow >= 8 && lane - 8 >= hd) v += u;
    u = fold_lane(v, 15);
    if (lane >= 16 && lane < 32 && hd <= 15) v += u;
    u = fold_lane(v, 31);
    if (lane >= 32 && lane < 48 && hd <= 31) v += u;
    u = fold_lane(v, 47);
    if (lane >= 48 && hd <= 47) v += u;
    return v;
}

template <typename T>
__global__ void __launch_bounds__(256) fold_float_kernel(const T *__restrict__ x, int64_t nchan, int64_t n, int64_t ld,
                                                         int64_t first_sample, double phase0, double dphase,
                                                         int64_t nbin, int tc, int64_t nct, double *__restrict__ part)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fold_smem[];
    uint32_t *meta = reinterpret_cast<uint32_t *>(fold_smem);                 // [FOLD_SUB]
    int *gmax = reinterpret_cast<int *>(meta + FOLD_SUB);                     // [FOLD_NG]
    double *acc = reinterpret_cast<double *>(fold_smem + FOLD_TABLE_BYTES);  // [tc][nbin]
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t seg = blockIdx.x / nct, c0 = (blockIdx.x % nct) * tc;
    const int64_t s0 = seg * FOLD_SEG, send = s0 + FOLD_SEG < n ? s0 + FOLD_SEG : n;
    const int nacc = tc * (int)nbin;
    for (int i = threadIdx.x; i < nacc; i += 256) acc[i] = 0.0;
    for (int64_t t0 = s0; t0 < send; t0 += FOLD_SUB) {
        __syncthreads();  // the zeroing; the previous sub-block's readers of meta
        fold_stage_bins(reinterpret_cast<int *>(meta), t0, send, first_sample, phase0, dphase, nbin);
        __syncthreads();
        for (int g = wave; g < FOLD_NG; g += 4) fold_group_meta(meta, gmax, g, lane);
        __syncthreads();
        for (int cl = wave; cl < tc; cl += 4) {
            const int64_t c = c0 + cl;
            if (c >= nchan) break;
            const T *row = x + c * ld;
            // volatile: a later round or group reads what another lane of this wave stored
            volatile double *a = acc + cl * (int)nbin;
            // FOLD_BATCH groups at a time: their loads and their scans are independent (one
            // latency for all), and the next batch's loads are issued before this batch's
            // scans and adds; the adds to the bins stay in group order
            T nv[FOLD_BATCH];  // (raw: converted at use, so nothing waits for a prefetched load early)
#pragma unroll
            for (int k = 0; k < FOLD_BATCH; ++k) {
                const int64_t t = t0 + k * FOLD_GROUP + lane;
                nv[k] = t < send ? row[t] : T(0);
            }
            for (int g0 = 0; g0 < FOLD_NG; g0 += FOLD_BATCH) {
                if (gmax[g0] < 0) break;  // no sample of the segment in this group or a later one
                double v[FOLD_BATCH];
                uint32_t mt[FOLD_BATCH];
#pragma unroll
                for (int k = 0; k < FOLD_BATCH; ++k) {
                    v[k] = static_cast<double>(nv[k]);
                    mt[k] = meta[(g0 + k) * FOLD_GROUP + lane];
                }
#pragma unroll
                for (int k = 0; k < FOLD_BATCH; ++k) {
                    const int64_t t = t0 + (g0 + FOLD_BATCH + k) * FOLD_GROUP + lane;
                    nv[k] = g0 + FOLD_BATCH < FOLD_NG && t < send ? row[t] : T(0);
                }
#pragma unroll
                for (int k = 0; k < FOLD_BATCH; ++k) v[k] = fold_run_scan(v[k], (int)((mt[k] >> 13) & 63), lane);
#pragma unroll
                for (int k = 0; k < FOLD_BATCH; ++k) {
                    const int gm = gmax[g0 + k];  // (-1: a group past the end, no add)
                    const int bin = mt[k] & 0x1FFF, rank = (mt[k] >> 19) & 63;
                    const bool vt = (mt[k] >> 25) & 1;
                    for (int r = 0; r <= gm; ++r)
                        if (vt && rank == r) a[bin] = a[bin] + v[k];
                }
            }
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < nacc; i += 256) {
        const int64_t c = c0 + i / (int)nbin;
        if (c < nchan) part[(seg * nchan + c) * nbin + i % (int)nbin] = acc[i];
    }
}

// sums[c][b] += the partials of (c, b) added in segment order
template <typename P>
__global__ void fold_combine_kernel(const P *__restrict__ part, int64_t nseg, int64_t nchan, int64_t nbin,
                                    double *__restrict__ sums, int64_t ld_sums)
{
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nchan * nbin) return;
    const int64_t c = i / nbin, b = i % nbin;
    double total;
    if (sizeof(P) == 4) {  // integer partials: exact
        uint64_t s = 0;
        for (int64_t k = 0; k < nseg; ++k) s += (uint64_t)part[k * nchan * nbin + i];
        total = (double)s;
    } else {
        total = (double)part[i];
        for (int64_t k = 1; k < nseg; ++k) total += (double)part[k * nchan * nbin + i];
    }
    sums[c * ld_sums + b] += total;
}

// counts[b] += the samples of the call in bin b: an LDS histogram per segment, then integer
// atomics (exact, order-free)
__global__ void __launch_bounds__(256) fold_counts_kernel(int64_t n, int64_t first_sample, double phase0, double dphase,
                                                          int64_t nbin, int64_t *__restrict__ counts)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char fold_smem[];
    uint32_t *hist = reinterpret_cast<uint32_t *>(fold_smem);
    for (int i = threadIdx.x; i < nbin; i += 256) hist[i] = 0;
    __syncthreads();
    const int64_t s0 = (int64_t)blockIdx.x * FOLD_SEG, send = s0 + FOLD_SEG < n ? s0 + FOLD_SEG : n;
    for (int64_t t = s0 + threadIdx.x; t < send; t += 256)
        atomicAdd(&hist[fold_bin(first_sample + t, phase0, dphase, nbin)], 1u);
    __syncthreads();
    for (int i = threadIdx.x; i < nbin; i += 256)
        if (hist[i]) atomicAdd(reinterpret_cast<unsigned long long *>(counts) + i, (unsigned long long)hist[i]);
}

// the channel tile: for float input (``full``) 16, 8 or 4 channels within 20 KiB of LDS (eight
// workgroups, i.e. every wave slot of a CU: the per-wave chains of load, scan and LDS add are
// latency-bound; measured 1.64 -> 0.83 ms on 1024 x 2^18 float32 at nbin 256), else within
// 64 KiB (8-bit input starts here: its LDS atomics gain nothing from more waves), else 4, 2 or 1 within 160 KiB; 0 = not even one channel fits (not reached for nbin <=
// FOLD_MAX_NBIN)
int fold_tile(int64_t pitch, size_t acc_bytes, bool full, size_t *lds)
{
    static const int small[] = {16, 8, 4}, large[] = {4, 2, 1};
    for (size_t budget : {full ? FOLD_LDS_FULL : FOLD_LDS_SMALL, FOLD_LDS_SMALL})
        for (int tc : small) {
            *lds = (size_t)tc * pitch * acc_bytes + FOLD_TABLE_BYTES;
            if (*lds <= budget) return tc;
        }
    for (int tc : large) {
        *lds = (size_t)tc * pitch * acc_bytes + FOLD_TABLE_BYTES;
        if (*lds <= FOLD_LDS_MAX) return tc;
    }
    return 0;
}

// ------------------------------------------------------------------ H-test

constexpr int HT_MAX_N = 8192;

__global__ void htest_table_kernel(int64_t n, double2 *__restrict__ tab)
{
    const int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    double s, c;
    sincospi(2.0 * (double)r / (double)n, &s, &c);
    tab[r] = make_double2(c, s);
}

// one wave per (row, harmonic k): pw[row][k - 1] = C_k^2 + S_k^2
__global__ void __launch_bounds__(256) htest_power_kernel(const double *__restrict__ prof, int64_t n, int64_t ld,
                                                          int64_t nmax, int64_t kblocks,
                                                          const double2 *__restrict__ tab, double *__restrict__ pw)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t row = blockIdx.x / kblocks, k = (blockIdx.x % kblocks) * 4 + wave + 1;
    if (k > nmax) return;
    const double *p = prof + row * ld;
    int64_t r = (k * lane) % n;
    const int64_t step = (k * 64) % n;
    double cs = 0.0, sn = 0.0;
    for (int64_t j = lane; j < n; j += 64) {
        const double v = p[j];
        const double2 w = tab[r];
        cs += v * w.x;
        sn += v * w.y;
        r += step;
        if (r >= n) r -= n;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        cs += __shfl_down(cs, d);
        sn += __shfl_down(sn, d);
    }
    if (lane == 0) pw[row * nmax + k - 1] = cs * cs + sn * sn;
}

// one workgroup per row: P and the finite check, then Z^2_m = (2 / P) sum_{k <= m} pw[k] by a
// sequential cumulative sum, H = max_m (Z^2_m - 4 m + 4) and the first m that attains it
__global__ void __launch_bounds__(256) htest_final_kernel(const double *__restrict__ prof, int64_t n, int64_t ld,
                                                          int64_t nmax, const double *__restrict__ pw,
                                                          double *__restrict__ h, int32_t *__restrict__ mo,
                                                          double *__restrict__ zs, int64_t ld_zs)
{
    __shared__ double buf[1024];
    __shared__ double red[4];
    __shared__ int bad[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t row = blockIdx.x;
    const double *p = prof + row * ld;
    double s = 0.0;
    int nf = 0;
    for (int64_t j = tid; j < n; j += 256) {
        const double v = p[j];
        nf |= !(fabs(v) <= 1.79769313486231570815e308);  // NaN or +-inf
        s += v;
    }
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        s += __shfl_down(s, d);
        nf |= __shfl_down(nf, d);
    }
    if (lane == 0) red[wave] = s, bad[wave] = nf;
    __syncthreads();
    const double P = ((red[0] + red[1]) + red[2]) + red[3];
    const bool ok = !(bad[0] | bad[1] | bad[2] | bad[3]) && P > 0.0;
    if (!ok) {  // (uniform over the workgroup)
        const double qnan = __longlong_as_double(0x7ff8000000000000ll);
        if (tid == 0) h[row] = qnan, mo[row] = 0;
        if (zs)
            for (int64_t k = tid; k < nmax; k += 256) zs[row * ld_zs + k] = qnan;
        return;
    }
    const double scale = 2.0 / P;
    double cum = 0.0, best = 0.0;
    int32_t bestm = 0;
    for (int64_t k0 = 0; k0 < nmax; k0 += 1024) {
        const int cnt = (int)(nmax - k0 < 1024 ? nmax - k0 : 1024);
        for (int i = tid; i < cnt; i += 256) buf[i] = pw[row * nmax + k0 + i];
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < cnt; ++i) {
                cum += buf[i];
                const double z = scale * cum;
                const int32_t m = (int32_t)(k0 + i + 1);
                const double hm = z - 4.0 * (double)m + 4.0;
                if (bestm == 0 || hm > best) best = hm, bestm = m;
                buf[i] = z;
            }
        }
        __syncthreads();
        if (zs)
            for (int i = tid; i < cnt; i += 256) zs[row * ld_zs + k0 + i] = buf[i];
        __syncthreads();
    }
    if (tid == 0) h[row] = best, mo[row] = bestm;
}

// pu_h_test's workspace: the table of n (cos, sin) pairs, then rows x nmax harmonic powers
struct HtestWs {
    double2 *tab;
    double *pw;
    size_t bytes;
};

HtestWs htest_carve(pu::Carver c, int64_t rows, int64_t n, int64_t nmax)
{
    HtestWs w;
    w.tab = c.take<double2>((size_t)n * sizeof(double2), 16);
    w.pw = c.take<double>((size_t)rows * (size_t)nmax * sizeof(double));
    w.bytes = c.used();
    return w;
}

}  // namespace

extern "C" {

size_t pu_fold_workspace_bytes(int64_t nchan, int64_t n, int64_t nbin)
{
    if (nchan <= 0 || n <= 0 || nbin <= 0) return 0;
    const int64_t nseg = (n + FOLD_SEG - 1) / FOLD_SEG;
    if (nseg > INT64_MAX / 8 / nchan || nseg * nchan > INT64_MAX / 8 / nbin) return SIZE_MAX;
    return (size_t)(nseg * nchan * nbin) * 8;
}

int pu_fold(const void *x, int dtype, int64_t nchan, int64_t n, int64_t ld, int64_t first_sample, double phase0,
            double dphase, int64_t nbin, double *sums, int64_t ld_sums, int64_t *counts, void *workspace,
            size_t workspace_bytes, void *stream)
{
    return pu::with_dtype<uint8_t, float, double>("pu_fold", dtype, [&](auto tag) -> int {
        using T = typename decltype(tag)::type;
        constexpr bool u8 = std::is_same_v<T, uint8_t>;
        PU_REQUIRE(nbin >= 1, "pu_fold: nbin %lld < 1", (long long)nbin);
        PU_REQUIRE(n >= 0 && nchan >= 0, "pu_fold: negative size (nchan %lld, n %lld)", (long long)nchan, (long long)n);
        PU_REQUIRE(ld >= n && ld_sums >= nbin,
                   "pu_fold: leading dimension too small (ld %lld < n %lld or ld_sums %lld < nbin %lld)", (long long)ld,
                   (long long)n, (long long)ld_sums, (long long)nbin);
        PU_REQUIRE(std::isfinite(phase0) && std::isfinite(dphase), "pu_fold: phase0 and dphase must be finite");
        PU_REQUIRE(first_sample <= INT64_MAX - n, "pu_fold: first_sample + n overflows");
        {
            const double lim = 4503599627370496.0;  // 2^52: beyond it a phase has no fraction
            const double pa = phase0 + (double)first_sample * dphase;
            const double pb = phase0 + (double)(first_sample + (n > 0 ? n - 1 : 0)) * dphase;
            PU_REQUIRE(std::fabs(pa) < lim && std::fabs(pb) < lim,
                       "pu_fold: the phase reaches 2^52 in this chunk (%g .. %g): no fraction left to bin", pa, pb);
        }
        if (nbin > FOLD_MAX_NBIN) {
            pu::set_error("pu_fold: nbin %lld above %d (the bins of a channel tile are LDS accumulators)", (long long)nbin,
                          FOLD_MAX_NBIN);
            return PU_EUNSUPPORTED;
        }
        if (n == 0 || nchan == 0) return PU_OK;
        PU_REQUIRE(x && sums && counts, "pu_fold: null pointer");
        const size_t need = pu_fold_workspace_bytes(nchan, n, nbin);
        PU_REQUIRE(need != SIZE_MAX, "pu_fold: the partials of %lld x %lld x %lld overflow", (long long)nchan,
                   (long long)n, (long long)nbin);
        if (int rc = pu::check_workspace("pu_fold", workspace, workspace_bytes, need, 8)) return rc;
        PU_REQUIRE(reinterpret_cast<uintptr_t>(x) % sizeof(T) == 0, "pu_fold: x is not aligned to its element type");
        size_t lds = 0;
        const int tc = u8 ? fold_tile(fold_pad((int)nbin), 4, false, &lds) : fold_tile(nbin, 8, true, &lds);
        PU_REQUIRE(tc > 0, "pu_fold: nbin %lld does not fit the LDS", (long long)nbin);
        const int64_t nseg = (n + FOLD_SEG - 1) / FOLD_SEG, nct = (nchan + tc - 1) / tc;
        PU_REQUIRE(nseg <= INT32_MAX / nct && nchan <= INT32_MAX / nbin,
                   "pu_fold: %lld segments x %lld channel tiles exceed the grid limit", (long long)nseg, (long long)nct);
        hipStream_t s = pu::as_stream(stream);
        const dim3 grid((unsigned)(nseg * nct)), block(256);
        const T *p = static_cast<const T *>(x);
        // the partial sums: exact integers for 8-bit input, float64 otherwise
        using P = std::conditional_t<u8, uint32_t, double>;
        P *part = static_cast<P *>(workspace);
        if constexpr (u8) {
            // (either instance, then one check)
            const bool vec = (reinterpret_cast<uintptr_t>(x) | static_cast<uintptr_t>(ld)) % 16 == 0;
            if (vec) {
                if (int rc = pu::ensure_lds(fold_u8_kernel<true>, lds)) return rc;
                hipLaunchKernelGGL(fold_u8_kernel<true>, grid, block, lds, s, p, nchan, n, ld, first_sample, phase0, dphase, nbin, tc, nct, part);
            } else {
                if (int rc = pu::ensure_lds(fold_u8_kernel<false>, lds)) return rc;
                hipLaunchKernelGGL(fold_u8_kernel<false>, grid, block, lds, s, p, nchan, n, ld, first_sample, phase0, dphase, nbin, tc, nct, part);
            }
            if (int rc = pu::launch_check("fold_u8_kernel")) return rc;
        } else {
            if (int rc = pu::launch("fold_float_kernel", fold_float_kernel<T>, grid, block, lds, s, p, nchan, n, ld, first_sample,
                                    phase0, dphase, nbin, tc, nct, part))
                return rc;
        }
        if (int rc = pu::launch("fold_combine_kernel", fold_combine_kernel<P>, dim3((unsigned)((nchan * nbin + 255) / 256)), block,
                                0, s, part, nseg, nchan, nbin, sums, ld_sums))
            return rc;
        return pu::launch("fold_counts_kernel", fold_counts_kernel, dim3((unsigned)nseg), block, (size_t)nbin * 4, s, n,
                          first_sample, phase0, dphase, nbin, counts);
    });
}

size_t pu_h_test_workspace_bytes(int64_t rows, int64_t n, int64_t nmax)
{
    if (rows <= 0 || n <= 0 || nmax <= 0 || n > HT_MAX_N || nmax > n) return 0;
    return htest_carve(pu::Carver(), rows, n, nmax).bytes;
}

int pu_h_test(const double *profiles, int64_t rows, int64_t n, int64_t ld, int64_t nmax, double *h, int32_t *m,
              double *zs, int64_t ld_zs, void *workspace, size_t workspace_bytes, void *stream)
{
    PU_REQUIRE(rows >= 0 && n >= 2, "pu_h_test: rows %lld, n %lld (a profile has at least 2 bins)", (long long)rows,
               (long long)n);
    if (n > HT_MAX_N) {
        pu::set_error("pu_h_test: n %lld above %d: the direct sum is for folded profiles; the H curve of an unfolded "
                      "chunk (n ~ 1e5, nmax = n / 10) needs an FFT, which this library does not have",
                      (long long)n, HT_MAX_N);
        return PU_EUNSUPPORTED;
    }
    PU_REQUIRE(nmax >= 1 && nmax <= n - 1, "pu_h_test: nmax %lld outside [1, n - 1 = %lld]", (long long)nmax,
               (long long)(n - 1));
    PU_REQUIRE(ld >= n && (!zs || ld_zs >= nmax), "pu_h_test: leading dimension too small (ld %lld < n %lld or ld_zs "
               "%lld < nmax %lld)", (long long)ld, (long long)n, (long long)ld_zs, (long long)nmax);
    if (rows == 0) return PU_OK;
    PU_REQUIRE(profiles && h && m, "pu_h_test: null pointer");
    const int64_t kblocks = (nmax + 3) / 4;
    PU_REQUIRE(rows <= INT32_MAX / kblocks, "pu_h_test: %lld rows x %lld harmonics exceed the grid limit",
               (long long)rows, (long long)nmax);
    const HtestWs w = htest_carve(pu::Carver(workspace), rows, n, nmax);
    if (int rc = pu::check_workspace("pu_h_test", workspace, workspace_bytes, w.bytes, 16)) return rc;
    hipStream_t s = pu::as_stream(stream);
    if (int rc = pu::launch("htest_table_kernel", htest_table_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, n,
                            w.tab))
        return rc;
    if (int rc = pu::launch("htest_power_kernel", htest_power_kernel, dim3((unsigned)(rows * kblocks)), dim3(256), 0, s,
                            profiles, n, ld, nmax, kblocks, w.tab, w.pw))
        return rc;
    return pu::launch("htest_final_kernel", htest_final_kernel, dim3((unsigned)rows), dim3(256), 0, s, profiles, n, ld, nmax,
                      w.pw, h, m, zs, ld_zs);
}

}  // extern "C"
