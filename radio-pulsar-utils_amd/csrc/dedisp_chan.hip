// Incoherent (brute-force) shift-and-sum dedispersion for gfx950 (MI355X) in channel
// order with float32 rows in LDS: dedisp_kernel (group-1 plans with float32 accumulation,
// and 8-bit input with float64 accumulation) and its launcher.  The subband kernel is
// dedisperse.hip, the float64-row kernel dedisp_f64.hip.
//
// Replaces the reference hot loop (pulsarutils/dedispersion.py):
//   _dedispersion_search :174-202  (prange over trials -> workgroups over DM tiles)
//   dedisperse/_dedisperse/roll_and_sum :60-98 (circular shift-and-sum, channel order)
//
// out_d[t] = sum_c x[c][(t + s[d][c]) mod N]   (s = dedispersion_shifts, any sign)
//
// Mapping:
//   * one workgroup = 8 waves = one DM tile (64 trials) x one time tile; each wave
//     owns D = 8 trials, lane l owns K samples (float: t0 + 2l + 128j + e, j<4, e<2)
//     -> D*K accumulators in VGPRs.
//   * channel rows are staged in LDS, ncc channels per chunk, each row covering
//     [t0 + smin_c, t0 + TT + smax_c) mod N: the tile's modular halo.  Rows arrive by
//     LDS-DMA (global_load_lds, 1 KiB pieces, per-lane modular addresses only for
//     the rare windows that wrap) into a two-buffer ring: chunk k+1 lands while chunk
//     k is summed.  Converting inputs (u8, f64 -> f32 LDS) use register staging.
//   * per (tile, channel, wave) the host precomputes 8 x u16 "window records": the LDS
//     byte offset of each trial's K-sample window (alignment copy included) and, in
//     bit 15, whether it differs from the previous trial's.  One scalar load per
//     channel; per trial one s_bitcmp1 + branch; the window is re-read (in place, 4 x
//     ds_read_b64) only when it changes -- adjacent plan trials differ by <= 1 sample
//     per channel, so most v_add_f32 reuse registers.  The first window of the next
//     channel is prefetched into the other window buffer while this one is summed.
//   * accumulation in channel order 0..nchan-1 (reference order: with a float64
//     accumulator the series is bit-identical).
//   * epilogue: the dedispersed plane, or per-tile partial statistics of the
//     1/2/4/8-sample rebinned series reduced by pu_finalize_kernel in a fixed order.
//   * blockIdx is remapped XCD-aware so all DM tiles of a time tile run on one XCD.
#include <hip/hip_runtime.h>

#include <type_traits>

#include "pu_common.h"

#include "dedisp_common.h"
#include "dedisp_units.h"

namespace {

// float32 sample k of a window (J x 8 bytes: pairs)
__device__ __forceinline__ float window_elem(const double (&w)[4], int k)
{
    const uint64_t b = __builtin_bit_cast(uint64_t, w[k >> 1]);
    return __builtin_bit_cast(float, (uint32_t)((k & 1) ? (b >> 32) : b));
}

// Add one channel's contribution to all D trials of this wave.  ``rec`` = 8 u16 window
// records (byte offset | reload flag << 15); ``w`` holds trial 0's window (raw LDS
// elements).  The window's K samples are taken into the accumulation type once per
// window (``wv``: a float32 -> float64 conversion per changed window, not per trial and
// sample: round 3 converted on every add, two VALU ops per float64 add at C2 acc='f64');
// a trial whose window differs from the previous trial's re-reads it in place.
template <typename Ta, int K, int J>
__device__ __forceinline__ void channel_trials(Ta (&acc)[kD][K], double (&w)[4], const u32x4 rec, uint32_t cbase)
{
    Ta wv[K];
#pragma unroll
    for (int k = 0; k < K; ++k) wv[k] = static_cast<Ta>(window_elem(w, k));
#pragma unroll
    for (int d = 0; d < kD; ++d) {
        if (d > 0) {
            const uint32_t word = rec[d >> 1] >> (16 * (d & 1));
            if (word & 0x8000u) {
                read_window<J>(w, cbase + (word & 0x7fffu));
#pragma unroll
                for (int k = 0; k < K; ++k) wv[k] = static_cast<Ta>(window_elem(w, k));
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) acc[d][k] += wv[k];
        pin_accumulators(acc[d]);
    }
}

template <typename Tin, typename Ta, bool PLANE, bool STATS>
// 4 waves per SIMD (2 workgroups per CU): <= 128 VGPRs, enforced (the float64 epilogue
// left alone took 130, i.e. 3 waves per SIMD)
__global__ void __launch_bounds__(kThreads) __attribute__((amdgpu_waves_per_eu(4)))
dedisp_kernel(DedispArgs a, const int32_t *__restrict__ tile_first, const int32_t *__restrict__ tile_count,
              const int32_t *__restrict__ tile_rowlen, const int32_t *__restrict__ base_tab,
              const u32x4 *__restrict__ rec_tab)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool kDma = std::is_same<Tin, float>::value;  // float32 rows: LDS-DMA, else converted
    constexpr int E = 2;          // float32 samples per 8-byte LDS read
    // reads per window: 4, or 2 when float32 rows feed float64 accumulators (8 trials x 8
    // float64 samples per lane would take 164 VGPRs: 3 waves per SIMD)
    constexpr int J = sizeof(Ta) == 8 ? 2 : 4;
    constexpr int K = E * J;      // samples per lane
    constexpr int TT = 64 * K;    // samples per time tile
    constexpr int D = kD;

    const int wg = pu::xcd_remap(blockIdx.x, gridDim.x);
    const int dt = a.dt0 + wg % a.ndt;
    const int tt = a.tt0 + wg / a.ndt;
    const int t0 = tt * TT;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int first = ld_uniform(tile_first + dt);
    const int cnt = ld_uniform(tile_count + dt);
    const int rowlen = ld_uniform(tile_rowlen + dt);
    const int slot0 = wave * D;
    const bool active = slot0 < cnt;
    const int n = a.n;
    const int stride = a.row_stride;           // elements per row copy
    const int copy_bytes = stride * 4;
    const int chan_bytes = E * copy_bytes;
    const int buf_bytes = a.ncc * chan_bytes;
    // LDS byte address of the dynamic region (local-address-space pointer -> 32-bit offset)
    const uint32_t smem_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;

    Ta acc[D][K];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int k = 0; k < K; ++k) acc[d][k] = Ta(0);

    const int32_t *base = base_tab + (size_t)dt * a.nchan;
    const u32x4 *recs = rec_tab + (size_t)dt * a.nchan * kWaves + wave;
    const Tin *data = reinterpret_cast<const Tin *>(a.data);
    const int nchunks = (a.nchan + a.ncc - 1) / a.ncc;
    // bytes of a row copy actually moved (whole 256-byte pieces)
    const int cover_bytes = (rowlen * 4 + 255) & ~255;

    // ---- LDS-DMA of chunk k into ring buffer b: each wave moves whole row copies (copy q of
    // a channel's row starts q samples later)
    auto issue_dma = [&](int k, int b) {
        const int c0 = k * a.ncc;
        const int nc = min(a.ncc, a.nchan - c0);
        const uint32_t bufo = (uint32_t)(b * buf_bytes);
        for (int r = wave; r < nc * E; r += kWaves) {
            const int ci = r / E, q = r % E;
            const int c = c0 + ci;
            int start = ld_uniform(base + c) + t0 + q;
            if (start >= n) start -= n;
            if (start >= n) start -= n;
            dma_row_f32(smem + bufo + ci * chan_bytes + q * copy_bytes,
                        reinterpret_cast<const float *>(a.data) + (size_t)c * (size_t)a.ld, start, cover_bytes, n,
                        a.small_n != 0, lane);
        }
    };

    // ---- register staging for converting inputs (u8 -> f32, f64 -> f32)
    auto stage_regs = [&](int k) {
        const int c0 = k * a.ncc;
        const int nc = min(a.ncc, a.nchan - c0);
        for (int ci = 0; ci < nc; ++ci) {
            const int c = c0 + ci;
            const Tin *row = data + (size_t)c * (size_t)a.ld;
            int start = ld_uniform(base + c) + t0;
            if (start >= n) start -= n;
            float *dst = reinterpret_cast<float *>(smem + ci * chan_bytes);
            const int len = rowlen + 1;  // + the alignment copy's last element
            for (int j = tid; j < len; j += kThreads) {
                int idx = start + j;
                if (!a.small_n) {
                    if (idx >= n) idx -= n;
                } else {
                    idx %= n;
                }
                const float v = static_cast<float>(row[idx]);
                if (j < rowlen) dst[j] = v;
                if (j >= 1) dst[stride + j - 1] = v;
            }
        }
    };

    if constexpr (kDma) issue_dma(0, 0);
    for (int k = 0; k < nchunks; ++k) {
        const int c0 = k * a.ncc;
        const int nc = min(a.ncc, a.nchan - c0);
        const int b = kDma ? (k & 1) : 0;
        if constexpr (kDma) asm volatile("s_waitcnt vmcnt(0)" : : : "memory");  // explicit (see dedisp_sub_kernel)
        __syncthreads();  // this wave's DMA landed and every wave left the other buffer
        if constexpr (kDma) {
            if (k + 1 < nchunks) issue_dma(k + 1, b ^ 1);
        } else {
            stage_regs(k);
            __syncthreads();
        }
        if (!active) continue;
        // ---- accumulate the chunk: channel pairs alternate window buffers so the next
        // channel's first window is read while this one is summed.  (Round 4 tried reads
        // one trial ahead of the adds instead, with a copy per changed window: C1 0.076
        // vs 0.068 ms.)
        const uint32_t rows_lane = smem_addr + (uint32_t)(b * buf_bytes) + 8u * lane;
        double w0[4], w1[4];
        const u32x4 *rc = recs + (size_t)c0 * kWaves;
        u32x4 rec0 = ld_uniform(rc);
        u32x4 rec1 = nc > 1 ? ld_uniform(rc + kWaves) : rec0;
        read_window<J>(w0, rows_lane + (rec0[0] & 0x7fffu));
        for (int ci = 0; ci < nc; ci += 2) {
            const uint32_t cb0 = rows_lane + (uint32_t)(ci * chan_bytes);
            const bool has1 = ci + 1 < nc, has2 = ci + 2 < nc, has3 = ci + 3 < nc;
            u32x4 rec2 = rec0, rec3 = rec1;
            if (has2) rec2 = ld_uniform(rc + (size_t)(ci + 2) * kWaves);  // two channels ahead
            if (has1) prefetch_window<J>(w1, cb0 + chan_bytes + (rec1[0] & 0x7fffu));
            channel_trials<Ta, K, J>(acc, w0, rec0, cb0);
            if (!has1) break;
            wait_window<J>(w1);
            if (has3) rec3 = ld_uniform(rc + (size_t)(ci + 3) * kWaves);
            if (has2) prefetch_window<J>(w0, cb0 + 2 * chan_bytes + (rec2[0] & 0x7fffu));
            channel_trials<Ta, K, J>(acc, w1, rec1, cb0 + chan_bytes);
            if (has2) wait_window<J>(w0);
            rec0 = rec2;
            rec1 = rec3;
        }
    }
    if (!active) return;

    if constexpr (STATS && !PLANE && sizeof(Ta) == 8) {
        if (t0 + TT <= n) {  // full tile: the permlane epilogue
            stats_full_f64<E, K>(acc, a, first, slot0, cnt, tt, lane);
            return;
        }
    }
    write_outputs<float, Ta, K, kD, PLANE, STATS>(acc, a, first, slot0, cnt, t0, tt, lane);
}

template <typename Tin, typename Ta>
int launch_variant(const pu_plan *p, const DedispArgs &a, bool plane, hipStream_t s)
{
    const dim3 grid((unsigned)((int64_t)a.ndt * a.ntt_run)), block(kThreads);
    auto go = [&](auto kern) {
        int rc = pu::ensure_lds(kern, p->t.lds_bytes);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, grid, block, p->t.lds_bytes, s, a, p->d.first, p->d.count, p->d.rowlen, p->d.base,
                           p->d.rec);
        return pu::launch_check("dedisp_kernel");
    };
    return plane ? go(dedisp_kernel<Tin, Ta, true, false>) : go(dedisp_kernel<Tin, Ta, false, true>);
}

}  // namespace

int pu_dd_launch_chan(const pu_plan *p, const void *args, size_t args_bytes, bool plane, void *stream)
{
    PU_REQUIRE(args_bytes == sizeof(DedispArgs), "pu_dd_launch_chan: argument block size mismatch");
    const DedispArgs &a = *reinterpret_cast<const DedispArgs *>(args);
    hipStream_t s = pu::as_stream(stream);
    switch (p->pb.variant) {
    case V_U8_F32: return launch_variant<uint8_t, float>(p, a, plane, s);
    case V_F32_F32: return launch_variant<float, float>(p, a, plane, s);
    case V_U8_F64: return launch_variant<uint8_t, double>(p, a, plane, s);
    case V_F64_F32: return launch_variant<double, float>(p, a, plane, s);
    }
    pu::set_error("pu_dd_launch_chan: plan variant %d has no float32-row kernel", p->pb.variant);
    return PU_EINVAL;
}
