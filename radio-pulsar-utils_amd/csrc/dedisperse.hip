// Incoherent (brute-force) shift-and-sum dedispersion for gfx950 (MI355X): the subband
// kernel (float32 accumulation of u8 / f32 / f64 inputs) and its launch
// code.  The channel-order kernels are dedisp_chan.hip and dedisp_f64.hip, the finalize
// kernel dedisp_finalize.hip, the plan object and the C ABI dedisp_host.hip.
//
// Replaces the reference hot loop (pulsarutils/dedispersion.py):
//   _dedispersion_search :174-202  (prange over trials -> workgroups over DM tiles)
//   dedisperse/_dedisperse/roll_and_sum :60-98 (circular shift-and-sum, channel order)
//
// out_d[t] = sum_c x[c][(t + s[d][c]) mod N]   (s = dedispersion_shifts, any sign)
//
// Channels are taken in groups of G adjacent channels.  For trial d and group g the
// shifts are s_{d,c0+k} = b_d + v_k, with b_d the group's first-channel shift and v the
// group's relative-shift VECTOR.  Plan trials share a handful of vectors per group
// (channels of a group drift apart by ~G/nchan sample per trial; the floor() of each
// channel's delay jitters by one), so a DM tile of 128 trials needs ~4 distinct vectors
// per group.  Per (DM tile, time tile) workgroup, stage by stage (a stage = a few
// consecutive groups):
//   1. build: for every distinct vector v of the tile in the stage's groups -- a "slot"
//      -- the exact partial sum  R[i] = sum_{k<G} x[c0+k][(t0 + lo + v_k + i) mod N]
//      into LDS (two alignment copies: R[i] and R[i+1] at the same offset), from the
//      stage's channel rows staged in LDS by DMA (f32) or straight from global memory
//      (u8 / f64, converted to f32).  One slot per wave at a time, U 64-element chunks
//      per pass with all their reads in flight;
//   2. sum: every trial adds ONE window of its slot per group:
//      out_d[t0 + i] += R_{v(d)}[i + b_d - lo].
// The gathered elements are the reference's (circular shift-and-sum; u8 exact), with
// G x fewer adds than channel mode.
//
// Lane l of a wave owns samples t0 + 2l + 128j + e (j < K/2, e < 2) of D trials.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <type_traits>

#include "pu_common.h"

#include "dedisp_common.h"
#include "dedisp_units.h"

namespace {

#ifdef PU_STAMPS
// Diagnostic build only: a shader-clock stamp with the LDS queue drained, fenced
// against scheduling (cdna_hip_programming.md §7, In-kernel stamps).  s_memtime is a
// scalar-cache READ of the clock; the totals leave the kernel through vector atomics.
__device__ __forceinline__ uint64_t stamp()
{
    uint64_t t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#endif

// max(v, v of the DPP source lane) in one v_max_f32_dpp (rows outside ROW_MASK keep v).
// IEEE-mode v_max_f32 returns the non-NaN operand, as fmax does; hipcc's fmax would
// add canonicalising maxes and could not fold the DPP move.
#define PU_MAX_DPP(NAME, CTRL)                                                                  \
    __device__ __forceinline__ float NAME(float v)                                              \
    {                                                                                           \
        float r = v;                                                                            \
        asm volatile("v_max_f32_dpp %0, %1, %0 " CTRL " bank_mask:0xf" : "+v"(r) : "v"(v));     \
        return r;                                                                               \
    }
PU_MAX_DPP(max_qp1032, "quad_perm:[1,0,3,2] row_mask:0xf")
PU_MAX_DPP(max_qp2301, "quad_perm:[2,3,0,1] row_mask:0xf")
PU_MAX_DPP(max_ror4, "row_ror:4 row_mask:0xf")
PU_MAX_DPP(max_ror8, "row_ror:8 row_mask:0xf")
#undef PU_MAX_DPP

__device__ __forceinline__ float vmax(float a, float b)
{
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));  // pure: may be computed unconditionally
    return r;
}

// v_max3_f32 (IEEE mode: a NaN operand is skipped, as by v_max_f32)
__device__ __forceinline__ float vmax3(float a, float b, float c)
{
    float r;
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "v"(c));
    return r;
}

// Cross-lane combines by the gfx950 permlane swaps (VALU, no LDS): one instruction
// exchanges half of two registers, so one swap + one op reduces TWO values by a factor
// of two in lanes.  swap32: lanes 0-31 of the result = op(a[l], a[l + 32]), lanes 32-63
// = op(b[l - 32], b[l]).  swap16 (rows of 16 lanes): [op(a.r0, a.r1), op(b.r0, b.r1),
// op(a.r2, a.r3), op(b.r2, b.r3)].
template <class Op>
__device__ __forceinline__ float swap32_combine(float a, float b, Op op)
{
    const auto r = __builtin_amdgcn_permlane32_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b),
                                                    false, false);
    return op(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
}
template <class Op>
__device__ __forceinline__ float swap16_combine(float a, float b, Op op)
{
    const auto r = __builtin_amdgcn_permlane16_swap(__builtin_bit_cast(unsigned, a), __builtin_bit_cast(unsigned, b),
                                                    false, false);
    return op(__builtin_bit_cast(float, (unsigned)r[0]), __builtin_bit_cast(float, (unsigned)r[1]));
}

// Row of 16 lanes: every lane gets the row's sum / max (fused DPP ops).
__device__ __forceinline__ float row_allsum(float v)
{
    v += dpp_undef<0xB1>(v);
    v += dpp_undef<0x4E>(v);
    v += dpp_undef<0x124>(v);
    v += dpp_undef<0x128>(v);
    return v;
}
__device__ __forceinline__ float row_allmax(float v)
{
    v = max_qp1032(v);
    v = max_qp2301(v);
    v = max_ror4(v);
    return max_ror8(v);
}

// Search-mode outputs of a wave of the subband kernel for a FULL time tile (every width's
// windows inside the series): the statistics of write_outputs (same partial record) from
// the packed accumulator pairs, without per-sample bounds tests.
//  * Per lane and trial: width 1 on the pairs (v_pk_*), widths 2/4/8 on scalars (the 4-
//    and 8-sample sums are fused v_add_f32_dpp row shifts) accumulated on every lane and
//    kept only on lanes where they are aligned windows, by one select after the loop (a
//    conditional v_max in inline asm became an EXEC-mask branch); squares accumulated by
//    FMA (one rounding), maxima by v_max3_f32 / v_max_f32.
//  * Across the wave, 8 trials at once: permlane32 swaps pair trial k with k + 4 (half
//    the lanes each), permlane16 swaps pair those with k + 2, so each of 2 registers
//    holds 4 trials' partials in its 4 rows; 4 DPP steps finish every row.
//    Per 8 trials and statistic: 6 swaps, 6 ops and 8 DPP steps instead of 6 DPP steps
//    per trial (the previous epilogue: ~10 % of the kernel's wave cycles at C2).
//  * Sums in float32 throughout: <= 14 float32 roundings per term (the shifted value, the
//    4-term lane chain, the pair, 2 swaps, 4 row steps, the square), within the gamma =
//    2^-20 the finalize kernel's certification assumes.
//  * Stores: lane 16 r + i writes field i (< 13) of the record of row r's trial - one
//    store instruction per 4 trials' records instead of one per field and trial.
template <int D, int J>
__device__ __forceinline__ void stats_full_pairs(const f32x2 (&acc)[D][J], const DedispArgs &a, int first, int slot0,
                                                 int cnt, int tt, int lane)
{
    static_assert(D % 8 == 0, "trials per wave");
    constexpr int NV = 9;  // per trial: sum y, sum of squares w = 1,2,4,8, max w = 1,2,4,8
    const bool even = (lane & 1) == 0;
    // The shift (recorded as the partial's center): the tile mean of the wave's first
    // trial.  The wave's D trials are a few DM steps apart, so their tile means differ by
    // a small fraction of the std: the shifted squares stay near the variance and their
    // float32 sums stay accurate, which keeps the finalize's certification bound tight
    // (lane 0's first sample as the shift inflated them by w^2 var).
    float kt;
    {
        f32x2 s0 = acc[0][0];
#pragma unroll
        for (int j = 1; j < J; ++j) s0 += acc[0][j];
        const float v = wave_sum_to63(s0.x + s0.y);
        kt = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), 63)) *
             (1.0f / (128.0f * J));
    }
    const f32x2 k1 = {kt, kt};
    const float k2 = 2.0f * kt, k4 = 4.0f * kt, k8 = 8.0f * kt;
    static_assert(J % 2 == 0, "sample pairs are taken two blocks at a time");
    const bool lo2 = (lane & 2) == 0;
    auto lane_stats = [&](int d, float (&v)[NV]) {
        f32x2 s1 = {0.0f, 0.0f}, q1 = s1;
        float q2 = 0.0f, q4 = 0.0f, q8 = 0.0f;
        float m1 = -INFINITY, m2 = -INFINITY, m4 = -INFINITY, m8 = -INFINITY;
#pragma unroll
        for (int j = 0; j < J; j += 2) {
            float r2[2];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const f32x2 x = acc[d][j + h];
                const f32x2 y = x - k1;
                s1 += y;
                q1 = __builtin_elementwise_fma(y, y, q1);
                m1 = vmax3(m1, x.x, x.y);
                r2[h] = x.x + x.y;  // width 2 (every lane)
                const float y2 = r2[h] - k2;
                q2 = __builtin_fmaf(y2, y2, q2);
                m2 = vmax(m2, r2[h]);
            }
            // widths 4 and 8 of the two blocks j, j + 1 packed into one register (every
            // lane useful, round 4): even lanes hold block j's width-4 sums (r2 of lanes l,
            // l + 1), odd lanes block j + 1's (lanes l - 1, l) - one quad_perm [1,0,3,2] add
            // of the parity-swapped r2; then quad_perm [2,3,0,1] pairs them into width 8 on
            // lanes 4k (block j) and 4k + 1 (block j + 1), the other two lanes of each quad
            // holding copies (dropped after the loop).  (Round 3: both widths on every lane
            // of every block, half / three quarters of them dropped.)
            const float a4 = even ? r2[0] : r2[1];
            const float c4 = even ? r2[1] : r2[0];
            const float r4 = a4 + dpp<0xB1>(0.0f, c4);
            const float y4 = r4 - k4;
            q4 = __builtin_fmaf(y4, y4, q4);
            m4 = vmax(m4, r4);
            const float r8 = r4 + dpp<0x4E>(0.0f, r4);
            const float y8 = r8 - k8;
            q8 = __builtin_fmaf(y8, y8, q8);
            m8 = vmax(m8, r8);
        }
        v[0] = s1.x + s1.y;
        v[1] = q1.x + q1.y;
        v[2] = q2;
        v[3] = q4;
        v[4] = lo2 ? q8 : 0.0f;
        v[5] = m1;
        v[6] = m2;
        v[7] = m4;
        v[8] = lo2 ? m8 : -INFINITY;
    };
    auto add = [](float x, float y) { return x + y; };
    auto mx = [](float x, float y) { return vmax(x, y); };
    // record field f = lane & 15 (< 13): kt | max w, sum, sum of squares w (w = 1, 2, 4, 8)
    const int f = lane & 15, row = lane >> 4;
    const int fw = (f - 1) / 3, fk = (f - 1) % 3;  // f >= 1: width index, 0 max / 1 sum / 2 squares
    // 8 trials at a time (b0 .. b0 + 7): the register footprint of the 16-trial shapes'
    // two passes is that of one
#pragma unroll
    for (int b0 = 0; b0 < D; b0 += 8) {
        // trials k and k + 4 -> U[k] (lanes 0-31: k, 32-63: k + 4)
        float U[4][NV];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            float va[NV], vb[NV];
            lane_stats(b0 + k, va);
            lane_stats(b0 + k + 4, vb);
#pragma unroll
            for (int i = 0; i < NV; ++i)
                U[k][i] = i < 5 ? swap32_combine(va[i], vb[i], add) : swap32_combine(va[i], vb[i], mx);
        }
        // U[j] and U[j + 2] -> W[j]: row r holds trial j + 2 r
        float W[2][NV];
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int i = 0; i < NV; ++i)
                W[j][i] = i < 5 ? row_allsum(swap16_combine(U[j][i], U[j + 2][i], add))
                                : row_allmax(swap16_combine(U[j][i], U[j + 2][i], mx));
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            float v = kt;
#pragma unroll
            for (int w = 0; w < 4; ++w) {
                v = (f >= 1 && fw == w && fk == 0) ? W[j][5 + w] : v;
                v = (f >= 1 && fw == w && fk == 1) ? W[j][0] : v;
                v = (f >= 1 && fw == w && fk == 2) ? W[j][1 + w] : v;
            }
            const int trial = b0 + j + 2 * row;
            if (f < 13 && slot0 + trial < cnt)
                reinterpret_cast<float *>(a.partials)[((size_t)(first + slot0 + trial) * a.ntt + tt) * kPartStride + f] = v;
        }
    }
}

struct SubArgs {
    DedispArgs o;           // data, ld, nchan, n, ndt, ntt, small_n; plane / partials
    int32_t ngroups;
    int32_t raw_stride;     // elements per staged channel row (DMA mode; bytes for 8-bit rows)
    int32_t zero_len;       // floats of the zero row at LDS offset 0 (DMA mode, partial groups)
    int32_t lds_bytes;      // dynamic LDS size: a stage's raw rows end here
    int32_t skip;           // diagnostic build only (PU_SUB_SKIP; results invalid): 1 build, 2 sum, 4 DMA, 8 epilogue
    int32_t dma_waves;      // waves that issue the LDS-DMA rows (the last ones of the workgroup)
    int32_t nitems;         // work items (DM tiles x time tiles of this launch)
    int32_t base_bits;      // DMA row words: base = word & (2^base_bits - 1), cover = (word >> base_bits) x 256 B
    int32_t dt_major;       // item order: 0 = time tile major (DM tiles of a time tile share L2), 1 = DM tile major
    void *stamps;           // diagnostic build (PU_STAMPS): 2 roles x 8 u64 phase-cycle totals
};

// Counted LDS wait, s_waitcnt lgkmcnt(N), that also "defines" the register it guards, so
// the instructions that read it cannot be hoisted above it.  lgkmcnt counts the inline-asm
// reads in issue order; an LDS op issued earlier or an outstanding scalar load only makes
// the wait longer, never shorter.
template <int N, typename T>
__device__ __forceinline__ void wait_lgkm(T &v)
{
    static_assert(N >= 0 && N <= 15, "lgkmcnt");
    asm volatile("s_waitcnt lgkmcnt(%1)" : "+v"(v) : "n"(N) : "memory");
}

// the same for the J registers of a window
template <int N, int J>
__device__ __forceinline__ void wait_lgkm(double (&w)[J])
{
    static_assert(J == 2 || J == 4, "window reads");
    static_assert(N >= 0 && N <= 15, "lgkmcnt");
    if constexpr (J == 4)
        asm volatile("s_waitcnt lgkmcnt(%4)" : "+v"(w[0]), "+v"(w[1]), "+v"(w[2]), "+v"(w[3]) : "n"(N) : "memory");
    else
        asm volatile("s_waitcnt lgkmcnt(%2)" : "+v"(w[0]), "+v"(w[1]) : "n"(N) : "memory");
}

// One group's contribution to the wave's D trials: rec[d] = LDS byte offset (slot area
// relative) of trial d's window; reads run 3 trials ahead of the adds.  Accumulators are
// float pairs (samples 2l + 128 j + {0, 1}): one window read is one pair, added by one
// v_pk_add_f32 - two IEEE adds, the same bits as two v_add_f32, at half the VALU issue
// (the sum's 8 v_add_f32 per trial took as many CU cycles as its 4 ds_read_b64).
// (Skipping the reads of windows that repeat the previous trial's - a third of them at
// C2 - was tried: 32 compile-time read patterns chosen per (group, wave) spilled at the
// switch's joins; an EXEC = 0 ds_read_b64 or a ds_nop costs about as much as a real
// read, scripts/lds_probe.hip.)

template <class C, typename RecT>
__device__ __forceinline__ void group_trials(f32x2 (&acc)[C::D][C::J], const RecT rec, uint32_t base)
{
    constexpr int D = C::D, J = C::J;
    double w[4][J];
    prefetch_window<J>(w[0], base + rec[0]);
    prefetch_window<J>(w[1], base + rec[1]);
    prefetch_window<J>(w[2], base + rec[2]);
#pragma unroll
    for (int d = 0; d < D; ++d) {
        if (d + 3 < D) prefetch_window<J>(w[(d + 3) & 3], base + rec[d + 3]);
        double(&wd)[J] = w[d & 3];
        const int ahead = D - 1 - d < 3 ? D - 1 - d : 3;
        if (ahead == 3)
            wait_lgkm<3 * J>(wd);
        else if (ahead == 2)
            wait_lgkm<2 * J>(wd);
        else if (ahead == 1)
            wait_lgkm<J>(wd);
        else
            wait_lgkm<0>(wd);
#pragma unroll
        for (int m = 0; m < J; ++m) acc[d][m] += __builtin_bit_cast(f32x2, wd[m]);
        pin_accumulators(acc[d]);
    }
}

// ---- 16-bit integer slots (8-bit input, time tile 256: DESIGN.md §4.1b).  A slot of an
// 8-bit group is a sum of <= G bytes, an integer <= G x 255, kept as u16 in four alignment
// copies (copy s holds R[i + s] at element i), so every window - 256 samples, four per
// lane - is ONE ds_read_b64 at an 8-byte-aligned address: half the sum's LDS reads of the
// float32 slots (two ds_read_b64 per window).  Lane l owns samples 4 l .. 4 l + 3 of its D
// trials in packed u16 accumulators `lo` (every add exact while the total since the last
// flush stays < 2^16) and `hi` (units of 256): every <= F groups (F G 255 + 255 < 2^16)
// `hi += lo >> 8, lo &= 255` - then hi 256 + lo is the exact integer sum (< nchan 255 <
// 2^24), converted to float32 once per item.  The u16 pairs are added as plain 32-bit words
// (v_add_u32): each half stays below 2^16, so no carry crosses into the high half.

// 16-bit slot build, one chunk of 128 elements: lane l's two elements 128 c + 2 l (+ 1) as
// the byte sums of the G channels (addresses ad[q], reads rb in flight).
// 16-bit slot build, P = 8 / G chunks of 128 elements in flight (2 G P = 16 byte reads,
// all the lgkmcnt field can count): register set C % P holds chunk C's reads.
template <int G, int P, int C>
__device__ __forceinline__ void s16_issue(uint32_t (&rb)[P][G][2], const uint32_t (&ad)[G])
{
#pragma unroll
    for (int q = 0; q < G; ++q) {
        asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(rb[C % P][q][0]) : "v"(ad[q]), "i"(128 * C) : "memory");
        asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(rb[C % P][q][1]) : "v"(ad[q]), "i"(128 * C + 1) : "memory");
    }
}

template <int G, int Q>
__device__ __forceinline__ void s16_quad_step(u32x2 (&d)[G], const uint32_t (&src)[G], uint32_t &acc02, uint32_t &acc13)
{
    if constexpr (Q < G) {
        wait_lgkm<G - 1 - Q>(d[Q]);
        const uint32_t t = __builtin_amdgcn_alignbyte(d[Q].y, d[Q].x, src[Q]);  // bytes src .. src + 3
        acc02 += t & 0x00ff00ffu;
        acc13 += (t >> 8) & 0x00ff00ffu;
        s16_quad_step<G, Q + 1>(d, src, acc02, acc13);
    }
}

// 16-bit slot build, the first 256 elements with four per lane: one ds_read2_b32 per
// channel (the lane's two aligned dwords around its 4 bytes: 4 LDS cycles for 256
// positions, where two ds_read_u8 per 128 positions take 8), the 4 bytes by v_alignbyte
// (src mod 4, uniform per channel), even and odd bytes summed as u16 pairs (no carry
// crosses: each half <= G 255).  ea / eb = the lane's (R[4l], R[4l+1]) / (R[4l+2], R[4l+3]).
template <int G>
__device__ __forceinline__ void s16_quad(const uint32_t (&src)[G], uint32_t smem_addr, int lane, uint32_t &ea,
                                         uint32_t &eb)
{
    u32x2 d[G];
#pragma unroll
    for (int q = 0; q < G; ++q) {
        const uint32_t a = smem_addr + (src[q] & ~3u) + 4u * (uint32_t)lane;
        asm volatile("ds_read2_b32 %0, %1 offset1:1" : "=&v"(d[q]) : "v"(a) : "memory");
    }
    uint32_t acc02 = 0, acc13 = 0;
    s16_quad_step<G, 0>(d, src, acc02, acc13);
    ea = __builtin_amdgcn_perm(acc13, acc02, 0x05040100u);
    eb = __builtin_amdgcn_perm(acc13, acc02, 0x07060302u);
}

// chunks C .. CEND - 1 of the 128-element build, issued ahead as s16_run expects
template <int G, int P, int C, int CEND>
__device__ __forceinline__ void s16_issue_range(uint32_t (&rb)[P][G][2], const uint32_t (&ad)[G])
{
    if constexpr (C < CEND) {
        s16_issue<G, P, C>(rb, ad);
        s16_issue_range<G, P, C + 1, CEND>(rb, ad);
    }
}

template <int G, int P, int C, int NCH>
__device__ __forceinline__ void s16_issue_first(uint32_t (&rb)[P][G][2], const uint32_t (&ad)[G])
{
    if constexpr (C < P && C < NCH) {
        s16_issue<G, P, C>(rb, ad);
        s16_issue_first<G, P, C + 1, NCH>(rb, ad);
    }
}

// Read i of chunk C (channel i / 2, byte i % 2): wait until it landed - the reads complete
// in issue order, so the wait allows every read issued after it to be outstanding: the rest
// of chunk C, the chunks after C already issued and (NEXT) the i already re-issued for chunk
// C + P: lgkmcnt(2 G P - 1) in steady state (an outstanding scalar load only lengthens the
// wait) - add it, and (NEXT) re-issue its register for chunk C + P.
template <int G, int P, int C, int NCH, int I>
__device__ __forceinline__ void s16_step(uint32_t (&rb)[P][G][2], const uint32_t (&ad)[G], uint32_t &s0, uint32_t &s1)
{
    if constexpr (I < 2 * G) {
        constexpr int q = I >> 1, e = I & 1;
        constexpr bool NEXT = C + P < NCH;
        constexpr int L = (C + P <= NCH ? P : NCH - C) - 1;  // later chunks already in flight
        constexpr int N = NEXT ? 2 * G * P - 1 : 2 * G - 1 - I + 2 * G * L;
        static_assert(N >= 0 && N <= 15, "lgkmcnt");
        uint32_t &r = rb[C % P][q][e];
        wait_lgkm<N>(r);
        if constexpr (e == 0)
            s0 += r;
        else
            s1 += r;
        if constexpr (NEXT)
            asm volatile("ds_read_u8 %0, %1 offset:%2" : "=v"(r) : "v"(ad[q]), "i"(128 * (C + P) + e) : "memory");
        s16_step<G, P, C, NCH, I + 1>(rb, ad, s0, s1);
    }
}

// chunks C .. NCH - 1: e[c] = lane l's elements 128 c + 2 l (+ 1) as a u16 pair
template <int G, int P, int C, int NCH>
__device__ __forceinline__ void s16_run(uint32_t (&rb)[P][G][2], const uint32_t (&ad)[G], uint32_t (&e)[4])
{
    if constexpr (C < NCH) {
        uint32_t s0 = 0, s1 = 0;
        s16_step<G, P, C, NCH, 0>(rb, ad, s0, s1);
        e[C] = s0 | (s1 << 16);
        s16_run<G, P, C + 1, NCH>(rb, ad, e);
    }
}


// The next lane's value (DPP wave_shl:1; lane 63 takes lane 0 of `next` by wave_rol:1).
__device__ __forceinline__ uint32_t s16_nextlane(uint32_t v, uint32_t next)
{
    const uint32_t x = (uint32_t)__builtin_amdgcn_mov_dpp((int)next, 0x134, 0xf, 0xf, false);
    return (uint32_t)__builtin_amdgcn_update_dpp((int)x, (int)v, 0x130, 0xf, 0xf, false);
}

// The odd-shifted u16 pair (R[2k + 1], R[2k + 2]) of lane k: the high half of its pair e =
// (R[2k], R[2k + 1]) with the low half of the next lane's (lane 63: of enext's lane 0).
__device__ __forceinline__ uint32_t s16_odd(uint32_t e, uint32_t enext)
{
    return __builtin_amdgcn_alignbit(s16_nextlane(e, enext), e, 16);
}

__device__ __forceinline__ void issue_window1(u32x2 &w, uint32_t addr)
{
    asm volatile("ds_read_b64 %0, %1" : "=&v"(w) : "v"(addr) : "memory");
}

// One group's contribution to the wave's D trials from 16-bit slots: one window read per
// trial, issued A trials ahead of its two v_pk_add_u16.
template <int D, int A, int I, typename RecT>
__device__ __forceinline__ void trials16_step(uint32_t (&lo)[D][2], u32x2 (&w)[A + 1], const RecT &rec, uint32_t base)
{
    if constexpr (I < D) {
        if constexpr (I + A < D) issue_window1(w[(I + A) % (A + 1)], base + rec[I + A]);
        constexpr int ahead = D - 1 - I < A ? D - 1 - I : A;
        u32x2 &wd = w[I % (A + 1)];
        wait_lgkm<ahead>(wd);
        lo[I][0] += wd.x;  // two u16 sums per dword: no carry crosses (each half < 2^16)
        lo[I][1] += wd.y;
        asm volatile("" : "+v"(lo[I][0]), "+v"(lo[I][1]));
        trials16_step<D, A, I + 1>(lo, w, rec, base);
    }
}

template <class C, typename RecT>
__device__ __forceinline__ void group_trials16(uint32_t (&lo)[C::D][2], const RecT rec, uint32_t base)
{
    constexpr int D = C::D, A = 5;
    u32x2 w[A + 1];
#pragma unroll
    for (int d = 0; d < A && d < D; ++d) issue_window1(w[d], base + rec[d]);
    trials16_step<D, A, 0>(lo, w, rec, base);
}

// per 16-bit half: hi += lo >> 8, lo &= 255 (exact: lo < 2^16; hi counts 256s of a sum of at
// most nchan x 255 <= 2^24 - 1 - the planner's nchan <= 65793 check - so hi < 2^16 and
// neither 32-bit add carries across the halves)
template <int D>
__device__ __forceinline__ void flush16(uint32_t (&lo)[D][2], uint32_t (&hi)[D][2])
{
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            hi[d][k] += (lo[d][k] >> 8) & 0x00ff00ffu;
            lo[d][k] &= 0x00ff00ffu;
        }
}

// The exact sums as float32 in the float slots' lane layout (lane l: samples 128 j + 2 l +
// e), which the epilogues and write_outputs take: sample 128 j + 2 l + e lives in lane
// 32 j + l / 2, element 2 (l & 1) + e - four ds_bpermute per (trial, j) and a select.
template <int D>
__device__ __forceinline__ void s16_to_pairs(const uint32_t (&lo)[D][2], const uint32_t (&hi)[D][2], f32x2 (&acc)[D][2],
                                             int lane)
{
    const bool odd = lane & 1;
#pragma unroll
    for (int d = 0; d < D; ++d) {
        float v[4];
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            v[2 * k] = (float)((hi[d][k] & 0xffffu) * 256u + (lo[d][k] & 0xffffu));
            v[2 * k + 1] = (float)((hi[d][k] >> 16) * 256u + (lo[d][k] >> 16));
        }
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int src = 4 * (32 * j + (lane >> 1));
            float g[4];
#pragma unroll
            for (int e = 0; e < 4; ++e)
                g[e] = __builtin_bit_cast(float, __builtin_amdgcn_ds_bpermute(src, __builtin_bit_cast(int, v[e])));
            acc[d][j] = odd ? f32x2{g[2], g[3]} : f32x2{g[0], g[1]};
        }
    }
}

// LDS-DMA of one 8-bit channel-row window [start, start + cover) mod n into dst, start
// and n multiples of 4 (the planner folds each row's misalignment into the slot
// sources): 1 KiB pieces while contiguous, per-lane modular dwords if it wraps.
__device__ __forceinline__ void dma_row_u8(unsigned char *dst, const unsigned char *row, int start, int cover_bytes,
                                           int n, bool small_n, int lane)
{
    if (!small_n && start + cover_bytes <= n) {
        const unsigned char *src = row + start;
        int off = 0;
        for (; off + 1024 <= cover_bytes; off += 1024)
            __builtin_amdgcn_global_load_lds((const void *)(src + off + 16 * lane),
                                             (__attribute__((address_space(3))) void *)(dst + off), 16, 0, 0);
        if (off < cover_bytes && lane < (cover_bytes - off) / 16)  // tail: one partial piece
            __builtin_amdgcn_global_load_lds((const void *)(src + off + 16 * lane),
                                             (__attribute__((address_space(3))) void *)(dst + off), 16, 0, 0);
    } else {
        const int nd = n >> 2;
        for (int off = 0; off < cover_bytes; off += 256) {
            int idx = (start >> 2) + (off >> 2) + lane;
            if (small_n) {
                idx %= nd;
            } else {
                idx = idx >= nd ? idx - nd : idx;
            }
            __builtin_amdgcn_global_load_lds((const void *)(row + 4 * idx),
                                             (__attribute__((address_space(3))) void *)(dst + off), 4, 0, 0);
        }
    }
}

// DMA8: 8-bit rows staged by LDS-DMA as bytes (plans with n % 4 == 0); otherwise 8-bit
// and float64 builds read global memory.
// One (DM tile, time tile) work item of the subband kernel: logical index wg; first =
// this workgroup's first item (it writes the zero row, which no item overwrites).
template <class C, typename Tin, int G, bool PLANE, bool STATS, bool DMA8, bool S16>
__device__ __forceinline__ void sub_item(SubArgs &a, const i32x4 *__restrict__ tiles,
                                         const i32x2 *__restrict__ tile_stages, const i32x4 *__restrict__ stages,
                                         const int32_t *__restrict__ slots, const int32_t *__restrict__ base_tab,
                                         const uint32_t *__restrict__ rec_tab, const int wg, const bool first_item)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr bool kDma = std::is_same<Tin, float>::value || (DMA8 && std::is_same<Tin, uint8_t>::value);
    constexpr int EB = std::is_same<Tin, float>::value ? 4 : 1;  // bytes per staged raw element
    constexpr int W = C::W, D = C::D, K = C::K, TT = C::TT;
    constexpr int MS = slot_stride(G);
    // chunks of 64 per build pass: one pass at a plan grid's spread when G x U values fit
    constexpr int U = std::min((TT + 80 + 63) / 64, (sizeof(Tin) == 8 ? 20 : 40) / G);
    typedef int32_t meta_t __attribute__((ext_vector_type(MS)));
    typedef uint32_t rec_t __attribute__((ext_vector_type(D)));
    const DedispArgs &o = a.o;
    const int ndt = o.ndt;
    // Items in dispatch order.  The planner sorts the DM tiles by decreasing cost, so
    // DM-tile-major order dispatches the longest items first (LPT: the short ones fill
    // the tail), for grids of few items per CU; time-tile-major order keeps the DM tiles
    // of one time tile together (one XCD, its L2 serving their overlapping rows).
    const int dt = o.dt0 + (a.dt_major ? wg / o.ntt_run : wg % ndt);
    const int tt = o.tt0 + (a.dt_major ? wg % o.ntt_run : wg / ndt);
    const int t0 = tt * TT;
    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const i32x4 tile = ld_uniform(tiles + dt);        // {first trial, count, raw row length, copy bytes}
    const i32x2 ts = ld_uniform(tile_stages + dt);    // {first stage, stage count}
    const int first = tile.x, cnt = tile.y;
    // alignment-copy bytes: float32 slots share the tile's (its widest span: whole build
    // passes need no store guards, C2's 2560 B at UP = 10); a 16-bit slot's follow from its
    // own length (the planner sizes it by its own span: (len + 2) u16, 64-rounded)
    const int tile_copy_bytes = tile.w;
    auto copy_bytes_of = [&](int len) {
        if constexpr (S16) return ((len + 65) & ~63) * 2;
        // float32: whole build passes (64 U elements: no store guards), at most the tile's
        const int whole = (len + 64 * U) / (64 * U) * (64 * U) * 4;
        return whole < tile_copy_bytes ? whole : tile_copy_bytes;
    };
    const int slot0 = wave * D;
    const bool active = slot0 < cnt;
    const int n = o.n;
    const bool small_n = o.small_n != 0;
    const Tin *data = reinterpret_cast<const Tin *>(o.data);
    const uint32_t smem_addr = (uint32_t)(uintptr_t)(__attribute__((address_space(3))) unsigned char *)smem;
    const uint32_t lds_base = smem_addr;  // slot records hold absolute LDS offsets
    const float *raw_lds = reinterpret_cast<const float *>(smem);
    const unsigned char *raw_lds8 = smem;

    static_assert(!S16 || (kDma && EB == 1 && C::K == 4), "16-bit slots: 8-bit DMA rows, 256-sample tiles");
    f32x2 acc2[D][C::J];
    if constexpr (!S16) {
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int m = 0; m < C::J; ++m) acc2[d][m] = f32x2{0.0f, 0.0f};
    }
    // 16-bit slots: packed u16 accumulators, flushed every <= F16 groups (see flush16)
    constexpr int F16 = (65535 - 255) / (G * 255);
    uint32_t lo16[S16 ? D : 1][2], hi16[S16 ? D : 1][2];  // u16 pairs: (sample 4 l + 2 k, + 1)
    if constexpr (S16) {
#pragma unroll
        for (int d = 0; d < D; ++d)
#pragma unroll
            for (int k = 0; k < 2; ++k) lo16[d][k] = hi16[d][k] = 0u;
    }
    int gc16 = 0;  // groups added since the last flush

    const rec_t *recs = reinterpret_cast<const rec_t *>(rec_tab) + (size_t)dt * a.ngroups * W + wave;
    if constexpr (kDma) {
        // zero row (partial groups' missing channels) between the raw rows and the slots
        if (first_item) {
            float *zero = reinterpret_cast<float *>(smem);
            for (int i = tid; i < a.zero_len; i += C::THREADS) zero[i] = 0.0f;
        }
    }

    // ---- DMA mode: the channel rows of stage st into the raw area.  vb = this wave's row
    // bases, lane k holding row wave + W k (one vector load per stage, issued a phase
    // ahead: a scalar load per row put its latency in series with every row's DMA issue,
    // ~10 % of the kernel's wave cycles at C2)
    // Only the last NDW waves issue the DMA (rows dw + NDW k, dw = wave - (W - NDW)): the
    // other waves go straight from the barrier to the sum instead of queueing their DMA
    // instructions behind everyone's on the CU's one texture-address path.
    const int32_t *base_t = base_tab + (size_t)dt * o.nchan;
    const int NDW = a.dma_waves;
#ifdef PU_STAMPS
    int skip = a.skip;  // diagnostic build only: PU_SUB_SKIP ablation (results invalid)
#else
    constexpr int skip = 0;  // the production kernel always does all of its work
#endif
    const int dw = wave - (W - NDW);  // < 0: this wave issues no DMA
    auto bases_of = [&](const i32x4 st) -> int {
        const int c = st.x * G + dw + NDW * lane;
        return dw >= 0 && c < min(st.y * G, o.nchan) ? base_t[c] : 0;
    };
    // this wave's rows of stage st: dw + NDW k for k < rows_of(st)
    auto rows_of = [&](const i32x4 st) {
        return dw < 0 ? 0 : (min(st.y * G, o.nchan) - st.x * G - dw + NDW - 1) / NDW;
    };
    // rows k in [kb, ke) of this wave
    auto issue_raw = [&](const i32x4 st, int vb, int kb, int ke) {
        const int c0 = st.x * G;
        const int nc = min(st.y * G, o.nchan) - c0;
        // the stage's rows end at the top of LDS (the host packs stages so that they never
        // overlap the previous stage's slots, which are summed while these rows land)
        unsigned char *raw = smem + a.lds_bytes - ((nc * a.raw_stride * EB + 255) & ~255);
        const int cover_tile = (tile.z * EB + 255) & ~255;
        const uint32_t base_mask = (1u << a.base_bits) - 1u;
        // row pointers by increments (one 64-bit add per row instead of a 64-bit multiply)
        const size_t row_step = (size_t)NDW * (size_t)o.ld;
        const Tin *rowp = data + (size_t)(c0 + dw + NDW * kb) * (size_t)o.ld;
        for (int k = kb; k < ke; ++k, rowp += row_step) {
            const int ci = dw + NDW * k;
            const int c = c0 + ci;
            // the row word: its base mod N and, in the top bits, this channel's own cover
            // (TT + its shift spread over the tile, in 256-B units; 0 = the tile's)
            const uint32_t word = (uint32_t)(k < 64 ? __builtin_amdgcn_readlane(vb, k) : ld_uniform(base_t + c));
            const uint32_t cu = word >> a.base_bits;
            const int cover_bytes = cu ? (int)(cu << 8) : cover_tile;
            int start = (int)(word & base_mask) + t0;
            if (start >= n) start -= n;
            if constexpr (EB == 4)
                dma_row_f32(raw + ci * a.raw_stride * 4, reinterpret_cast<const float *>(rowp), start, cover_bytes, n,
                            small_n, lane);
            else
                dma_row_u8(raw + ci * a.raw_stride, reinterpret_cast<const unsigned char *>(rowp), start, cover_bytes,
                           n, small_n, lane);
        }
    };

    auto load = [&](const meta_t &m, int q, int i) -> float {
        if constexpr (kDma && EB == 1) {
            return static_cast<float>(raw_lds8[m[4 + q] + i]);  // ds_read_u8
        } else if constexpr (kDma) {
            return raw_lds[m[4 + q] + i];  // past the slot only for masked lanes (row padding)
        } else {
            int pos = m[4 + q] + t0 + i;
            if (small_n) {
                pos %= n;
            } else {
                if (pos >= n) pos -= n;
                if (pos >= n) pos -= n;
            }
            const int ch = min(m[2] + q, o.nchan - 1);  // partial groups: in-bounds, discarded
            return static_cast<float>(data[(size_t)ch * (size_t)o.ld + pos]);
        }
    };

    // ---- one build pass: chunks [i0, i0 + 64 UP) of a slot, written while < lim (whole
    // chunks: lanes past len write row padding).  All G x UP reads in flight.  Reads of
    // chunks past lim are not clamped: their results are discarded, and an LDS read past
    // the allocation returns 0 (clamping them costs a VALU add per read - the reads then
    // cannot fold 256 u into the ds_read offset field - and was measured 1.8 ms slower at
    // C2, 20.2 vs 18.4 ms).
    // A pass of a width matched to the slot (exact: all its chunks < lim, see slot()) has no
    // guarded store path at all.
    auto build_pass = [&](auto upc, auto exact, const meta_t &m, int gs, int i0, int lim, bool whole_cb,
                          int copy_bytes) {
        constexpr int UP = decltype(upc)::value;
        const bool whole = decltype(exact)::value || whole_cb;
        auto at = [&](int u) { return i0 + 64 * u + lane; };
        float r[UP];
        if constexpr (kDma && EB == 1) {
            // 8-bit rows: the bytes summed as integers (v_add3_u32), one convert per element
            // - the same float32 value as the float sum (every partial sum < 2^24 is exact),
            // a third of the VALU work of a convert + add per byte
            uint32_t w[UP][G];
#pragma unroll
            for (int u = 0; u < UP; ++u)
#pragma unroll
                for (int q = 0; q < G; ++q) w[u][q] = raw_lds8[m[4 + q] + at(u)];  // ds_read_u8
#pragma unroll
            for (int u = 0; u < UP; ++u) {
                uint32_t s = 0;
#pragma unroll
                for (int q = 0; q < G; ++q) s += w[u][q];
                r[u] = static_cast<float>(s);
            }
        } else {
            float v[UP][G];
            if (kDma || gs == G) {  // branch-free, all G x UP reads in flight (DMA mode: a
                                    // partial group's missing channels read the zero row)
#pragma unroll
                for (int u = 0; u < UP; ++u)
#pragma unroll
                    for (int q = 0; q < G; ++q) v[u][q] = load(m, q, at(u));
            } else {        // the last, partial group of a band
#pragma unroll
                for (int u = 0; u < UP; ++u)
#pragma unroll
                    for (int q = 0; q < G; ++q) v[u][q] = q < gs ? load(m, q, at(u)) : 0.0f;
            }
#pragma unroll
            for (int u = 0; u < UP; ++u) {
                r[u] = 0.0f;
#pragma unroll
                for (int q = 0; q < G; ++q) r[u] += v[u][q];
            }
        }
        // all sums before the first (chunk-uniform) write branch: keeps every read
        // of the pass in flight together
#pragma unroll
        for (int u = 0; u < UP; ++u) asm volatile("" : "+v"(r[u]));
        // copy 0 at element i, copy 1 at element i - 1: lane-contiguous dwords, so
        // ds_write_addtid_b32 (address = M0 + offset + 4 lane, no address VGPR):
        // twice the LDS store rate of ds_write_b32 (MI355X_MICROARCH.md §LDS)
        const uint32_t w0 = lds_base + (uint32_t)m[1] + 4u * (uint32_t)i0;
        const uint32_t w1 = w0 + (uint32_t)copy_bytes - 4u;
        // M0 set twice per pass (copy 0, then copy 1) and not restored: hipcc sets M0 afresh
        // in the basic block of every LDS-DMA it emits (checked on the generated code by
        // scripts/check_m0.py; an "m0" clobber would be ignored - hipcc treats M0 as
        // reserved); nothing between these volatile statements uses M0.  (Saving and
        // restoring it cost two scalar instructions per pass: C2 15.78 vs 15.65 ms.)  Setting it around every
        // chunk's two stores instead cost ~7 scalar issue slots per chunk on the CU's shared
        // scalar unit (C2 19.97 -> 19.20 ms, C3 625 trials 156.5 -> 150.9 ms).  When a copy
        // spans whole passes (copy_bytes a multiple of 256 UP: C2's 2560 B at UP = 10) the
        // chunks past len only write the slot's own padding, so the stores need no guards;
        // so does any pass whose UP chunks end inside the copy (4 i0 + 256 UP <= copy_bytes:
        // copy 1's stores end 4 bytes earlier than copy 0's) - round 5: C3's single pass per
        // slot (272 elements, UP = 5) no longer guards each store by a scalar compare + branch
        // when its copy is 6 chunks long.  (whole: pass_whole(i0), decided by the caller - for
        // the first pass once per tile.)
        asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(w0) : "memory");
        if (whole) {
#pragma unroll
            for (int u = 0; u < UP; ++u)
                asm volatile("ds_write_addtid_b32 %0 offset:%1" : : "v"(r[u]), "i"(256 * u) : "memory");
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(w1) : "memory");
#pragma unroll
            for (int u = 0; u < UP; ++u)
                asm volatile("ds_write_addtid_b32 %0 offset:%1" : : "v"(r[u]), "i"(256 * u) : "memory");
        } else {
#pragma unroll
            for (int u = 0; u < UP; ++u)
                if (i0 + 64 * u < lim)
                    asm volatile("ds_write_addtid_b32 %0 offset:%1" : : "v"(r[u]), "i"(256 * u) : "memory");
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(w1) : "memory");
#pragma unroll
            for (int u = 0; u < UP; ++u)
                if (i0 + 64 * u < lim)
                    asm volatile("ds_write_addtid_b32 %0 offset:%1" : : "v"(r[u]), "i"(256 * u) : "memory");
        }
    };

    // ---- 16-bit slots (S16): one slot in chunks of 128 elements, lane l building elements
    // 128 u + 2 l and + 1 of chunk u (two byte reads per channel, summed as integers) packed
    // as one u16 pair E_u; the odd-shifted pair (R[2k + 1], R[2k + 2]) is E_u's high half
    // with the next lane's low half (DPP wave_shl:1; lane 63 takes chunk u + 1's lane 0 by
    // wave_rol:1).  Stores by ds_write_addtid_b32: E_u to copy 0 and, 4 bytes down, copy 2;
    // O_u to copy 1 and, 4 bytes down, copy 3 (element i of copy s is R[i + s]).  Chunks
    // 0-2 always (len <= 512; a chunk past the copy's end stores only its lanes inside it),
    // chunk 3 when len > 384; the reads of the next 8 / G chunks in flight while a chunk is
    // summed.
    auto slot16_pairs = [&](const meta_t &m) {
        const bool four = m[0] > 384;
        const int copy_bytes = copy_bytes_of(m[0]);
        // per channel the lane's byte address; 2 G byte reads per chunk (ds_read_u8 in inline
        // asm: the order kept by s16_run holds ~15 in flight in 16 registers - each value is
        // added, then its register takes the read of chunk c + 8 / G, same channel and byte)
        uint32_t ad[G];
#pragma unroll
        for (int q = 0; q < G; ++q) ad[q] = smem_addr + (uint32_t)m[4 + q] + 2u * (uint32_t)lane;
        constexpr int P = 8 / G;
        uint32_t rb[P][G][2];
        uint32_t e[4] = {0u, 0u, 0u, 0u};
        if (four) {
            s16_issue_first<G, P, 0, 4>(rb, ad);
            s16_run<G, P, 0, 4>(rb, ad, e);
        } else {
            s16_issue_first<G, P, 0, 3>(rb, ad);
            s16_run<G, P, 0, 3>(rb, ad, e);
        }
        const uint32_t e0 = e[0], e1 = e[1], e2 = e[2], e3 = e[3];
        uint32_t o0 = s16_odd(e0, e1), o1 = s16_odd(e1, e2), o2 = s16_odd(e2, e3), o3 = four ? s16_odd(e3, e3) : 0u;
        asm volatile("" : "+v"(o0), "+v"(o1), "+v"(o2), "+v"(o3));
        const uint32_t c0 = lds_base + (uint32_t)m[1];
        const uint32_t cbu = (uint32_t)copy_bytes;
        // a chunk reaching past its copy (copies hold TT + span + 2 elements rounded to 64)
        // stores only its lanes inside it (elements 128 c + 2 l <= copy - 2; copies 2 / 3 give
        // up their last dword, beyond every window)
        const bool fit2 = 768u <= cbu, fit3 = 1024u <= cbu;
        const bool in2 = 512 + 4 * lane <= (int)cbu - 4, in3 = 768 + 4 * lane <= (int)cbu - 4;
        auto store = [&](uint32_t base, uint32_t v0, uint32_t v1, uint32_t v2, uint32_t v3) {
            asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(base) : "memory");
            asm volatile("ds_write_addtid_b32 %0 offset:0" : : "v"(v0) : "memory");
            asm volatile("ds_write_addtid_b32 %0 offset:256" : : "v"(v1) : "memory");
            if (fit2 || in2) asm volatile("ds_write_addtid_b32 %0 offset:512" : : "v"(v2) : "memory");
            if (four && (fit3 || in3)) asm volatile("ds_write_addtid_b32 %0 offset:768" : : "v"(v3) : "memory");
        };
        store(c0, e0, e1, e2, e3);
        store(c0 + 2u * cbu - 4u, e0, e1, e2, e3);
        store(c0 + cbu, o0, o1, o2, o3);
        store(c0 + 3u * cbu - 4u, o0, o1, o2, o3);
    };

    auto slot16_quad = [&](const meta_t &m) {
        const int len = m[0];  // 256 (= TT) .. 510
        const int copy_bytes = copy_bytes_of(len);
        // elements 0 .. 255: four per lane (s16_quad)
        uint32_t src[G];
#pragma unroll
        for (int q = 0; q < G; ++q) src[q] = (uint32_t)m[4 + q];
        uint32_t ea, eb;
        s16_quad<G>(src, smem_addr, lane, ea, eb);
        // elements 256 .. len - 1 (<= 2 chunks of 128): two per lane, as chunks 2 and 3 of the
        // 128-element build (its reads in flight per s16_run)
        uint32_t ad[G];
#pragma unroll
        for (int q = 0; q < G; ++q) ad[q] = smem_addr + src[q] + 2u * (uint32_t)lane;
        constexpr int P = 8 / G;
        uint32_t rb[P][G][2];
        uint32_t e[4] = {0u, 0u, 0u, 0u};
        const bool t2 = len > 256, t3 = len > 384;
        if (t3) {
            s16_issue_range<G, P, 2, (2 + P < 4 ? 2 + P : 4)>(rb, ad);
            s16_run<G, P, 2, 4>(rb, ad, e);
        } else if (t2) {
            s16_issue_range<G, P, 2, 3>(rb, ad);
            s16_run<G, P, 2, 3>(rb, ad, e);
        }
        // dword j of copy s: copy 0 E[j], copy 1 O[j], copy 2 E[j + 1], copy 3 O[j + 1]
        // (E[k] = (R[2k], R[2k+1]), O[k] = (R[2k+1], R[2k+2])); lane l of the first 256
        // elements owns dwords 2l and 2l + 1: E[2l] = ea, E[2l+1] = eb
        const uint32_t nea = s16_nextlane(ea, e[2]);  // E[2l + 2] (lane 63: the tail's first pair)
        const uint32_t neb = s16_nextlane(eb, e[2]);  // E[2l + 3] (lane 63's is rewritten by the tail)
        u32x2 w0 = {ea, eb}, w2 = {eb, nea};
        u32x2 w1 = {__builtin_amdgcn_alignbit(eb, ea, 16), __builtin_amdgcn_alignbit(nea, eb, 16)};
        u32x2 w3 = {w1.y, __builtin_amdgcn_alignbit(neb, nea, 16)};
        const uint32_t c0 = lds_base + (uint32_t)m[1];
        const uint32_t cbu = (uint32_t)copy_bytes;
        const uint32_t a0 = c0 + 8u * (uint32_t)lane;
        asm volatile("ds_write_b64 %0, %1" : : "v"(a0), "v"(w0) : "memory");
        asm volatile("ds_write_b64 %0, %1" : : "v"(a0 + cbu), "v"(w1) : "memory");
        asm volatile("ds_write_b64 %0, %1" : : "v"(a0 + 2u * cbu), "v"(w2) : "memory");
        asm volatile("ds_write_b64 %0, %1" : : "v"(a0 + 3u * cbu), "v"(w3) : "memory");
        if (t2) {
            // the tail chunks by ds_write_addtid_b32 (copies 2 / 3 4 bytes down, after the
            // first part's stores: its copy-3 dword 127 is rewritten here); a chunk reaching
            // past its copy (copies hold TT + span + 2 elements rounded to 64) stores only its
            // lanes inside it (elements 128 c + 2 l <= copy - 2)
            const uint32_t o2 = s16_odd(e[2], e[3]), o3 = s16_odd(e[3], e[3]);
            const bool in2 = 768u <= cbu || 512 + 4 * lane <= (int)cbu - 4;
            const bool in3 = t3 && (1024u <= cbu || 768 + 4 * lane <= (int)cbu - 4);
            auto store = [&](uint32_t base, uint32_t v2, uint32_t v3) {
                asm volatile("s_mov_b32 m0, %0\n\ts_nop 0" : : "s"(base) : "memory");
                if (in2) asm volatile("ds_write_addtid_b32 %0 offset:512" : : "v"(v2) : "memory");
                if (in3) asm volatile("ds_write_addtid_b32 %0 offset:768" : : "v"(v3) : "memory");
            };
            store(c0, e[2], e[3]);
            store(c0 + 2u * cbu - 4u, e[2], e[3]);
            store(c0 + cbu, o2, o3);
            store(c0 + 3u * cbu - 4u, o2, o3);
        }
    };

    // G = 8: the first 256 elements four per lane (s16_quad: half the build's LDS read cycles;
    // round 6 A/B: C3 625 trials 115.5 -> 113.5 ms, 5000 958 -> 936 ms); G <= 4: two per lane
    // throughout, which measured faster there (5000 trials G = 4: 858 vs 901 ms) - with 2 G
    // byte reads per chunk, 8 / G chunks stay in flight
    auto slot16 = [&](const meta_t &m) {
        if constexpr (G == 8)
            slot16_quad(m);
        else
            slot16_pairs(m);
    };

    // ---- build the stage's slots, one per wave at a time: R[i] (i < len) at copy 0 [i]
    // and copy 1 [i - 1] (copy 1's element -1 lands in copy 0's padding).  (Splitting a
    // slot over waves to balance the ~20 slots of a stage over 16 waves was measured
    // slower: 22.1 / 25.6 vs 20.2 ms for halves / thirds - fewer reads in flight per
    // pass, and the extra pass code spilled registers.)
    auto pass_whole = [&](int i0, int copy_bytes) {
        return copy_bytes % (256 * U) == 0 || 4 * i0 + 256 * U <= copy_bytes;
    };
    auto build = [&](const i32x4 st, const meta_t m0) {
        // the next slot's record is loaded a slot ahead (round 5: loaded on demand, its
        // scalar-load latency stood in front of every slot after a wave's first), through a
        // pointer stepped by W records: past the stage's last slot it reads the next stage's
        // records or the table's padding (pad_slots: W records of zeros), never used.
        // Every slot has a first pass (len >= TT): peeled, with the tile's whole0.
        // Two slots per iteration with ping-pong records (rotating one record through a copy
        // cost a dozen scalar moves per slot).
        // The first pass is U chunks wide or, for a slot that needs fewer, UN = U - 1 (picked
        // by a wave-uniform test on lim): a fixed U read, summed and stored a chunk no window
        // reads, past lim, into the copy's padding - 73 % of C2's slots, nearly all of C5's
        // and all of C4's.  len > TT, so lim >= 64 UN: neither first pass
        // runs past lim, both end inside the copy (4 lim <= copy_bytes) and store without
        // guards.  Plans whose U is already the shortest slot's chunk count (UN = U: G = 8,
        // float64 G >= 4) keep the one first pass.  Trailing passes are full-width, guarded
        // where they end past the copy (C2: 40 of 5109 slots have one; a 1-chunk pass for
        // them cost the wide float G = 4 kernel register spills).
        constexpr int UN = TT / 64 + 1 < U ? U - 1 : U;
        auto slot = [&](const meta_t &m) {
            const int len = m[0], gs = m[3];
            const int lim = (len + 63) & ~63;
            const int cb = copy_bytes_of(len);
            if constexpr (UN < U) {
                if (lim < 64 * U)
                    build_pass(std::integral_constant<int, UN>{}, std::true_type{}, m, gs, 0, lim, true, cb);
                else
                    build_pass(std::integral_constant<int, U>{}, std::true_type{}, m, gs, 0, lim, true, cb);
            } else {
                build_pass(std::integral_constant<int, U>{}, std::false_type{}, m, gs, 0, lim, pass_whole(0, cb), cb);
            }
            for (int i0 = 64 * U; i0 < len; i0 += 64 * U)
                build_pass(std::integral_constant<int, U>{}, std::false_type{}, m, gs, i0, lim, pass_whole(i0, cb),
                           cb);
        };
        meta_t ma = m0;
        const meta_t *mp = reinterpret_cast<const meta_t *>(slots) + (size_t)(st.z + wave + W);
        for (int s = st.z + wave; s < st.w; s += 2 * W, mp += 2 * W) {
            meta_t mb = ld_uniform(mp);
            if constexpr (S16)
                slot16(ma);
            else
                slot(ma);
            if (s + W >= st.w) break;
            ma = ld_uniform(mp + W);
            if constexpr (S16)
                slot16(mb);
            else
                slot(mb);
        }
    };

    // ---- stage loop.  Scalar metadata is loaded one step ahead (the stage records of k+1
    // and k+2, this wave's first DMA row base, slot record and window records), so the
    // loads' latency overlaps a phase of work (kAhead, below) or at least the barrier waits.
    const int ns = ts.y;
    auto stage_at = [&](int k) { return ld_uniform(stages + ts.x + min(k, ns - 1)); };
    auto meta_of = [&](const i32x4 st) {
        return ld_uniform(reinterpret_cast<const meta_t *>(slots + (size_t)min(st.z + wave, st.w - 1) * MS));
    };
    i32x4 st = stage_at(0), st1 = stage_at(1);
    if constexpr (kDma) issue_raw(st, bases_of(st), 0, rows_of(st));
#ifdef PU_STAMPS
    // diagnostic build only (make stamps): per-wave cycles per phase, summed over stages.
    // No stamp stands between the loop-top loads and barrier 1 (a stamp drains lgkmcnt:
    // it would expose their latency before the barrier, on every wave): phase 1 runs from
    // the end of the sum through the wave's own DMA wait and barrier 1; phase 0 is what the
    // wave then waits for its scalar metadata (the clock is read before the wait, so two
    // stamps back to back cost one scalar-cache round trip: the floor of phase 0).
    uint64_t ph[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tp = stamp(), tq;
#define PU_PHASE(i) (tq = stamp(), ph[i] += tq - tp, tp = tq)
#else
#define PU_PHASE(i) ((void)0)
#endif
    // The scalar metadata a stage consumes right after barrier 1 is loaded a phase ahead and
    // not just before that barrier, where the wave that arrives last (and releases it) has
    // nothing to hide the latency behind before its first slot().  Measured: C2 13.52 ->
    // 13.22 ms; the stamps do not show that stall on its own:
    //  * rec0, the stage's first window record, is the record the previous stage's sum
    //    loaded during its last group - the stages of a tile are consecutive in groups
    //    (plan_sub; asserted by plan_check), so the row after a stage's last group is the
    //    next stage's first.  Only the tile's first stage loads it here.
    //  * m0, this wave's first slot record, and the stage record of k + 2 are loaded
    //    right after barrier 2 of the previous stage, with its DMA issue: a whole sum ahead.
    //    (Loading them at the sum's last group instead, m0 live across one group only, put
    //    the loads on three paths of the group loop and spilled 40 more SGPRs: C2 13.98 vs
    //    13.20 ms, parent 13.49; profiles/stage_metadata/.)
    // kAhead: the G = 8 and the 16-bit-slot instantiations keep all three loads at the loop
    // top, as before - their 16-word slot records / packed accumulators leave no room: loading
    // ahead cost them SGPR spills (profiles/stage_metadata/code_object_metadata.txt).
    constexpr bool kAhead = G < 8 && !S16;
    rec_t rec0;
    meta_t m0;
    if constexpr (kAhead) {
        rec0 = ld_uniform(recs + (size_t)st.x * W);
        m0 = meta_of(st);
    }
    const int glt = a.ngroups - 1;  // the tile's last group: the last row of its records
    for (int k = 0; k < ns; ++k) {
        i32x4 st2;
        meta_t m1;
        if constexpr (!kAhead) {
            st2 = stage_at(k + 2);
            m0 = meta_of(st);
            rec0 = ld_uniform(recs + (size_t)st.x * W);
        }
        // This wave's LDS-DMA rows have landed before it arrives at the barrier.  Explicit:
        // a workgroup-scope __syncthreads does not wait for vmcnt on gfx950, and the
        // compiler's own LDS-DMA tracking puts its wait before this wave's first LDS read,
        // after the barrier - too late for the other waves that read these rows.
        asm volatile("s_waitcnt vmcnt(0)" : : : "memory");
        __syncthreads();  // raw rows of stage k landed; every wave left the slot area
        PU_PHASE(1);
        PU_PHASE(0);  // the stall on this stage's scalar metadata after the barrier
        const int vb1 = kDma && k + 1 < ns ? bases_of(st1) : 0;  // lands during the build
        if (!(skip & 1)) build(st, m0);
        PU_PHASE(2);
        __syncthreads();  // slots built; every wave left the raw rows
        PU_PHASE(3);
        if constexpr (kAhead) {
            m1 = meta_of(st1);  // past the tile's last stage: the clamped stage's, never used
            st2 = stage_at(k + 2);
        }
        if constexpr (kDma) {
            // the next stage's rows land while this stage is summed.  (Spreading these DMAs
            // over the sum's groups instead was measured slower, 20.6 vs 18.5 ms at C2: the
            // issue inside the sum breaks its read pipelining.)
            // The row-base load is waited for HERE, on every path, while no DMA is in
            // flight: left to the compiler, the wait for it lands at the head of the sum
            // loop as vmcnt(0) (its register is reused there), which also waits for all
            // the DMAs just issued - every DMA wave then summed only after its rows landed.
            int vb = vb1;
            asm volatile("" : "+v"(vb));
            if (k + 1 < ns && !(skip & 4)) issue_raw(st1, vb, 0, rows_of(st1));
        }
        PU_PHASE(4);
        // The DMA waves start summing last (their LDS-DMA issue holds them ~10 % of the
        // stage), so they sum at raised priority: the other waves fill the LDS queue
        // around them instead of reaching the barrier first and leaving it half idle
        // (C2 17.3 -> 16.9 ms; raising it for the DMA issue too: 17.6).
        if (dw >= 0) __builtin_amdgcn_s_setprio(1);
        if (active && !(skip & 2)) {
            const uint32_t sb = smem_addr + 8u * lane;  // window records: absolute LDS offsets
            // two groups per iteration with ping-pong records (no per-group record copy).
            // A record is consumed only after the previous group's last lgkmcnt(0) (the empty
            // asm): hoisted into the trial loop, its scalar-load wait drained the LDS reads.
            // kAhead: the row past the stage's last group is the next stage's first record
            // (rec0 of the next iteration, in ra or rb by the parity of the stage's group
            // count); the index is clamped to the tile's last group, whose successor would be
            // the next tile's row or, in the last tile, lie past the table.  Otherwise clamped
            // to the stage's last group.  The clamped row is loaded again, never used.
            rec_t ra = rec0, rb;
            if constexpr (kAhead) rb = ra;  // read after the loop (a stage has >= 1 group: set there)
            const int gl = st.y - 1;
            const int gc = kAhead ? glt : gl;
            for (int g = st.x; g < st.y; g += 2) {
                rb = ld_uniform(recs + (size_t)min(g + 1, gc) * W);
                if constexpr (S16) {
                    if (gc16 + 2 > F16) {
                        flush16<D>(lo16, hi16);
                        gc16 = 0;
                    }
                    gc16 += 2;
                    group_trials16<C>(lo16, ra, sb);
                } else {
                    group_trials<C>(acc2, ra, sb);
                }
                asm volatile("" : "+s"(rb));
                if (g + 1 > gl) break;
                ra = ld_uniform(recs + (size_t)min(g + 2, gc) * W);
                if constexpr (S16)
                    group_trials16<C>(lo16, rb, sb);
                else
                    group_trials<C>(acc2, rb, sb);
                asm volatile("" : "+s"(ra));
            }
            if constexpr (kAhead) rec0 = ((st.y - st.x) & 1) ? rb : ra;
        }
        // (a wave without trials sums nothing and uses no window record: its rec0 stays the
        // tile's first, unused)
        if (dw >= 0) __builtin_amdgcn_s_setprio(0);
        PU_PHASE(5);
        st = st1;
        st1 = st2;
        if constexpr (kAhead) m0 = m1;
    }
    if constexpr (S16) {
        if (active) s16_to_pairs<D>(lo16, hi16, acc2, lane);
    }
    if constexpr (STATS && !PLANE) {
        if (active && !(skip & 8) && t0 + TT <= n) {
            stats_full_pairs<D, C::J>(acc2, o, first, slot0, cnt, tt, lane);
#ifndef PU_STAMPS
            return;
#else
            skip |= 8;  // stamps build: the epilogue is done, only the stamps remain
#endif
        }
    }
    float acc[D][K];
#pragma unroll
    for (int d = 0; d < D; ++d)
#pragma unroll
        for (int m = 0; m < C::J; ++m) {
            acc[d][2 * m] = acc2[d][m].x;
            acc[d][2 * m + 1] = acc2[d][m].y;
        }
#ifdef PU_STAMPS
    if (active && !(skip & 8)) write_outputs<float, float, K, D, PLANE, STATS>(acc, o, first, slot0, cnt, t0, tt, lane);
    PU_PHASE(6);
    if (lane == 0 && a.stamps) {
        // two sets of totals by role: the DMA-issuing waves after the others
        const int role = dw >= 0 ? 8 : 0;
        for (int i = 0; i < 8; ++i) atomicAdd(reinterpret_cast<unsigned long long *>(a.stamps) + role + i,
                                              (unsigned long long)ph[i]);
    }
#undef PU_PHASE
#else
#undef PU_PHASE
    if (!active || (skip & 8)) return;
    write_outputs<float, float, K, D, PLANE, STATS>(acc, o, first, slot0, cnt, t0, tt, lane);
#endif
}

// One workgroup per work item.  (A persistent grid - one workgroup per CU looping over
// items b, b + grid, ... - measured slower at C2, 16.68 vs 16.19 ms: the hardware's
// dynamic dispatch of the next workgroup to whichever CU frees first beats a static
// round-robin; and its loop state cost the C3 instantiation scratch spills.)
template <class C, typename Tin, int G, bool PLANE, bool STATS, bool DMA8, bool S16 = false>
__global__ void __launch_bounds__(C::THREADS, 4)
dedisp_sub_kernel(SubArgs a, const i32x4 *__restrict__ tiles, const i32x2 *__restrict__ tile_stages,
                  const i32x4 *__restrict__ stages, const int32_t *__restrict__ slots,
                  const int32_t *__restrict__ base_tab, const uint32_t *__restrict__ rec_tab)
{
    sub_item<C, Tin, G, PLANE, STATS, DMA8, S16>(a, tiles, tile_stages, stages, slots, base_tab, rec_tab,
                                            pu::xcd_remap(blockIdx.x, gridDim.x), true);
}

template <class C, typename Tin, int G>
int launch_sub(const pu_plan *p, const DedispArgs &a, bool plane, hipStream_t s)
{
    SubArgs sa{};
    sa.o = a;
    sa.ngroups = p->t.ngroups;
    sa.raw_stride = p->t.raw_stride;
    sa.zero_len = (int32_t)p->t.zero_len;
    sa.lds_bytes = (int32_t)p->t.lds_bytes;
    sa.stamps = p->d_stamps;
    sa.dma_waves = std::min<int>(8, C::W);  // C2 17.6 vs 18.95 ms with all 16 waves, C3 141 vs 150 (625 trials)
#ifdef PU_STAMPS
    // diagnostic build only (make stamps): ablation and DMA-wave tuning knobs
    if (const char *env = getenv("PU_SUB_SKIP")) sa.skip = atoi(env);
    if (const char *env = getenv("PU_DMA_WAVES")) sa.dma_waves = std::clamp(atoi(env), 1, (int)C::W);
#endif

    const int64_t nitems = (int64_t)a.ndt * a.ntt_run;
    sa.nitems = (int32_t)nitems;
    sa.base_bits = p->t.base_bits;
    sa.dt_major = p->t.dt_major;
    const int64_t nblk = nitems;
    const dim3 grid((unsigned)nblk), block(C::THREADS);
    auto go = [&](auto kern) {
        int rc = pu::ensure_lds(kern, p->t.lds_bytes);
        if (rc) return rc;
        hipLaunchKernelGGL(kern, grid, block, p->t.lds_bytes, s, sa, p->d.tiles, p->d.tile_stages, p->d.stages,
                           p->d.slots, p->d.base, p->d.recs);
        return pu::launch_check("dedisp_sub_kernel");
    };
    if constexpr (std::is_same<Tin, uint8_t>::value) {
        if constexpr (C::K == 4) {
            if (p->t.slot16)
                return plane ? go(dedisp_sub_kernel<C, Tin, G, true, false, true, true>)
                             : go(dedisp_sub_kernel<C, Tin, G, false, true, true, true>);
        }
        if (p->t.dma8)
            return plane ? go(dedisp_sub_kernel<C, Tin, G, true, false, true>)
                         : go(dedisp_sub_kernel<C, Tin, G, false, true, true>);
    }
    return plane ? go(dedisp_sub_kernel<C, Tin, G, true, false, false>)
                 : go(dedisp_sub_kernel<C, Tin, G, false, true, false>);
}

template <class C, typename Tin>
int launch_sub_g(const pu_plan *p, const DedispArgs &a, bool plane, hipStream_t s)
{
    switch (p->t.group) {
    case 2: return launch_sub<C, Tin, 2>(p, a, plane, s);
    case 4: return launch_sub<C, Tin, 4>(p, a, plane, s);
    case 8: return launch_sub<C, Tin, 8>(p, a, plane, s);
    }
    pu::set_error("bad plan group %d", p->t.group);
    return PU_EINVAL;
}

template <typename Tin>
int launch_sub_shape(const pu_plan *p, const DedispArgs &a, bool plane, hipStream_t s)
{
    return with_shape(p->t.shape, [&](auto c) { return launch_sub_g<decltype(c), Tin>(p, a, plane, s); });
}

}  // namespace

int pu_dd_launch_sub(const pu_plan *p, const void *args, size_t args_bytes, bool plane, void *stream)
{
    PU_REQUIRE(args_bytes == sizeof(DedispArgs), "pu_dd_launch_sub: argument block size mismatch");
    const DedispArgs &a = *reinterpret_cast<const DedispArgs *>(args);
    hipStream_t s = pu::as_stream(stream);
    switch (p->pb.dtype) {
    case PU_U8: return launch_sub_shape<uint8_t>(p, a, plane, s);
    case PU_F32: return launch_sub_shape<float>(p, a, plane, s);
    case PU_F64: return launch_sub_shape<double>(p, a, plane, s);
    }
    pu::set_error("bad plan dtype");
    return PU_EINVAL;
}
