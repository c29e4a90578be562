// The Fourier-domain periodicity search after pu_rfft, for gfx950: pu_spectrum_normalize and
// pu_harmonic_search (the definitions are in include/pulsarutils_hip.h).
//
// pu_spectrum_normalize.  A workgroup of 256 owns a tile of up to 1024 consecutive bins of one
// row: the powers go to LDS twice (values and a copy to sort), a bitonic network whose merges stop
// at the block size B sorts every aligned block of B on its own, and each bin is scaled by its
// block's LN2 / median.  Only values are sorted, so ties cannot change a result.
//
// pu_harmonic_search.  A workgroup owns 1024 consecutive top-harmonic bins k of one row, plus one
// bin on either side.  A thread computes S_0 .. S_(nlev-1) of its bins in a register (ascending
// level, ascending m: the order of the header) and leaves them in LDS [level][bin]; nothing but
// the optional ``sums`` goes back to HBM.  Wave w then walks the tile for levels w, w + 4 in bin
// order, 64 bins at a time: a ballot of the candidate test gives the count (first launch) or,
// with the offsets of the scan, each candidate's place (second launch).  The counts are laid out
// [row][level][tile], which is the delivery order, so one exclusive scan over them is all the
// ordering there is: no atomics, nothing depends on scheduling.  The second launch skips a tile
// whose counts are all zero before it computes anything.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pu_common.h"

namespace {

constexpr int SN_TILE = 1024;  // bins of a normalise workgroup (the largest block)
constexpr int HS_TILE = 1024;  // top-harmonic bins of a search workgroup
constexpr int HS_MAX_LEV = 6;
constexpr float SN_LN2 = 0.6931472f;

__global__ void __launch_bounds__(256)
spec_normalize_kernel(const float2 *__restrict__ spec, int64_t ld_spec, int64_t nb, int lb, float *__restrict__ out,
                      int64_t ld_out)
{
    __shared__ float pw[SN_TILE], srt[SN_TILE];
    __shared__ int bad[SN_TILE / 16];
    const int64_t r = blockIdx.y, k0 = (int64_t)blockIdx.x * SN_TILE;
    const int tile = (int)(nb - k0 < SN_TILE ? nb - k0 : SN_TILE);  // a power of two >= B (nb is one)
    const int bsz = 1 << lb;
    const float inf = __int_as_float(0x7f800000);
    const float2 *row = spec + r * ld_spec;
    if (threadIdx.x < SN_TILE / 16) bad[threadIdx.x] = 0;
    __syncthreads();
    for (int i = threadIdx.x; i < tile; i += blockDim.x) {
        const float2 z = row[k0 + i];
        const float a = z.x * z.x, b = z.y * z.y;
        const float p = a + b;
        const bool first = k0 + i == 0;
        pw[i] = p;
        srt[i] = first ? inf : p;
        if (!first && !(fabsf(p) < inf)) bad[i >> lb] = 1;
    }
    // bitonic sort of every aligned block of B: merges of size 2 .. B
    for (int k = 2; k <= bsz; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            __syncthreads();
            for (int i = threadIdx.x; i < tile; i += blockDim.x) {
                const int l = i ^ j;
                if (l > i) {
                    const float a = srt[i], b = srt[l];
                    const bool up = (i & k) == 0 || k == bsz;  // the last merge of a block ascends
                    if (up ? a > b : a < b) {
                        srt[i] = b;
                        srt[l] = a;
                    }
                }
            }
        }
    }
    __syncthreads();
    float *dst = out + r * ld_out;
    for (int i = threadIdx.x; i < tile; i += blockDim.x) {
        const int blk = i >> lb, base = blk << lb;
        const bool zero_blk = k0 + base == 0;
        const float lo = srt[base + bsz / 2 - 1], hi = srt[base + bsz / 2];
        const float med = zero_blk ? lo : 0.5f * (lo + hi);
        float v;
        if (bad[blk]) {
            v = __int_as_float(0x7fc00000);
        } else if (!(med > 0.0f)) {
            v = 0.0f;
        } else {
            const float scale = SN_LN2 / med;
            v = pw[i] * scale;
        }
        if (k0 + i == 0) v = 0.0f;
        dst[k0 + i] = v;
    }
}

struct HsLevels {
    float thr[HS_MAX_LEV];
    int64_t kmin[HS_MAX_LEV], kmax[HS_MAX_LEV];
};

// In place: blk[i] (counts, m of them) -> their exclusive prefix sum; *total = the sum.  One
// workgroup of 1024, 8 consecutive entries per thread and step (exact.hip's event scan).
__global__ void __launch_bounds__(1024) hs_scan_kernel(int64_t *__restrict__ blk, int64_t m, int64_t *total)
{
    __shared__ int64_t wsum[16];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t c0 = 0; c0 < m; c0 += 8 * 1024) {
        const int64_t i0 = c0 + (int64_t)threadIdx.x * 8;
        int64_t v[8], sum = 0;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            v[j] = i0 + j < m ? blk[i0 + j] : 0;
            sum += v[j];
        }
        int64_t inc = sum;
        for (int d = 1; d < 64; d <<= 1) {
            const int64_t o = __shfl_up(inc, d);
            if (lane >= d) inc += o;
        }
        if (lane == 63) wsum[wave] = inc;
        __syncthreads();
        int64_t before = 0, all = 0;
        for (int w = 0; w < 16; ++w) {
            if (w < wave) before += wsum[w];
            all += wsum[w];
        }
        int64_t run = carry + before + inc - sum;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i0 + j < m) {
                blk[i0 + j] = run;
                run += v[j];
            }
        carry += all;
        __syncthreads();
    }
    if (threadIdx.x == 0) *total = carry;
}

// EMIT false: sums (if asked for) and the candidate counts of every (row, level, tile); EMIT true:
// the candidates themselves at the scanned offsets.
template <bool EMIT>
__global__ void __launch_bounds__(256)
hs_search_kernel(const float *__restrict__ norm, int64_t nb, int64_t ld, int nlev, float *__restrict__ sums,
                 int64_t ld_level, int64_t ld_row, HsLevels lv, int64_t *__restrict__ blk, int64_t ntile,
                 const int64_t *__restrict__ total, pu_spec_cand *__restrict__ cands, int64_t cap)
{
    __shared__ float sm[HS_MAX_LEV][HS_TILE + 2];  // [level][bin - k0 + 1]
    const int64_t r = blockIdx.y, k0 = (int64_t)blockIdx.x * HS_TILE;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t slot = (r * nlev) * ntile + blockIdx.x;  // level l: slot + l * ntile
    if (EMIT) {
        // nothing to deliver from this tile: at every level its offset equals the next slot's (the
        // slots are in delivery order), or lies beyond cap
        const int64_t slots = (int64_t)gridDim.y * nlev * ntile;
        bool any = false;
        for (int l = 0; l < nlev; ++l) {
            const int64_t i = slot + l * ntile, at = blk[i];
            const int64_t nxt = i + 1 < slots ? blk[i + 1] : *total;
            any = any || (nxt > at && at < cap);
        }
        if (!any) return;
    }
    const float ninf = __int_as_float(0xff800000);
    const float *row = norm + r * ld;
    for (int i = threadIdx.x; i < HS_TILE + 2; i += blockDim.x) {
        const int64_t k = k0 - 1 + i;
        if (k < 0 || k >= nb) {
            for (int l = 0; l < nlev; ++l) sm[l][i] = ninf;
            continue;
        }
        float s = row[k];
        sm[0][i] = s;
        for (int l = 0; l + 1 < nlev; ++l) {
            const int64_t h = (int64_t)1 << l;
            for (int64_t m = 1; m < 2 * h; m += 2) s += row[(k * m + h) / (2 * h)];
            sm[l + 1][i] = s;
        }
        if (!EMIT && sums && i >= 1 && i <= HS_TILE)
            for (int l = 0; l < nlev; ++l) sums[l * ld_level + r * ld_row + k] = sm[l][i];
    }
    __syncthreads();
    for (int l = wave; l < nlev; l += 4) {
        const float thr = lv.thr[l];
        const int64_t kmin = lv.kmin[l], kmax = lv.kmax[l];
        int64_t pos = EMIT ? blk[slot + l * ntile] : 0;
        for (int i0 = 0; i0 < HS_TILE; i0 += 64) {
            const int i = i0 + lane + 1;
            const int64_t k = k0 + i0 + lane;
            const float v = sm[l][i];
            const bool c = k < nb && k >= kmin && k < kmax && v > thr && v > sm[l][i - 1] && v >= sm[l][i + 1];
            const uint64_t m = __ballot(c);
            if (EMIT) {
                const int64_t at = pos + __popcll(m & ((1ull << lane) - 1ull));
                if (c && at < cap) {
                    pu_spec_cand e;
                    e.row = (int32_t)r;
                    e.level = l;
                    e.bin = k;
                    e.power = v;
                    e.pad = 0.0f;
                    cands[at] = e;
                }
            }
            pos += __popcll(m);
        }
        if (!EMIT && lane == 0) blk[slot + l * ntile] = pos;
    }
}

// pu_harmonic_search's workspace: a count (then offset) per (row, level, tile), then the total
struct HsWs {
    int64_t *blk, *total;
    size_t bytes;
};

HsWs hs_carve(pu::Carver c, int64_t slots)
{
    HsWs w;
    w.blk = c.take<int64_t>((size_t)slots * 8);
    w.total = c.take<int64_t>(256);
    w.bytes = c.used();
    return w;
}

}  // namespace

extern "C" {

int pu_spectrum_normalize(const void *spec, int64_t rows, int64_t nb, int64_t ld_spec, int64_t block, float *out,
                          int64_t ld_out, void *stream)
{
    PU_REQUIRE(nb >= 128 && nb <= ((int64_t)1 << 23) && (nb & (nb - 1)) == 0,
               "pu_spectrum_normalize: nb %lld is not a power of two in [2^7, 2^23]", (long long)nb);
    PU_REQUIRE(block >= 16 && block <= 1024 && block <= nb && (block & (block - 1)) == 0,
               "pu_spectrum_normalize: block %lld is not a power of two in [16, min(1024, nb)]", (long long)block);
    PU_REQUIRE(rows >= 0 && rows <= 65535, "pu_spectrum_normalize: rows %lld outside [0, 65535]", (long long)rows);
    PU_REQUIRE(ld_spec >= nb && ld_out >= nb, "pu_spectrum_normalize: leading dimension too small (ld_spec %lld, ld_out "
               "%lld < nb %lld)", (long long)ld_spec, (long long)ld_out, (long long)nb);
    if (rows == 0) return PU_OK;
    PU_REQUIRE(spec && out, "pu_spectrum_normalize: null pointer");
    PU_REQUIRE(reinterpret_cast<uintptr_t>(spec) % 8 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0,
               "pu_spectrum_normalize: spec or out is not aligned to its element type");
    int lb = 0;
    while (((int64_t)1 << lb) < block) ++lb;
    const dim3 grid((unsigned)((nb + SN_TILE - 1) / SN_TILE), (unsigned)rows);
    return pu::launch("spec_normalize_kernel", spec_normalize_kernel, grid, dim3(256), 0, pu::as_stream(stream),
                      static_cast<const float2 *>(spec), ld_spec, nb, lb, out, ld_out);
}

size_t pu_harmonic_search_workspace_bytes(int64_t rows, int64_t nb, int64_t nlev)
{
    if (rows <= 0 || nb <= 0 || nlev <= 0) return 0;
    return hs_carve(pu::Carver(), rows * nlev * ((nb + HS_TILE - 1) / HS_TILE)).bytes;
}

int pu_harmonic_search(const float *norm, int64_t rows, int64_t nb, int64_t ld, int64_t nlev, float *sums,
                       int64_t ld_level, int64_t ld_row, const float *thr, const int64_t *kmin, const int64_t *kmax,
                       pu_spec_cand *cands, int64_t cap, int64_t *count, void *workspace, size_t workspace_bytes,
                       void *stream)
{
    PU_REQUIRE(nlev >= 1 && nlev <= HS_MAX_LEV, "pu_harmonic_search: nlev %lld outside [1, 6]", (long long)nlev);
    PU_REQUIRE(rows >= 0 && rows <= 65535, "pu_harmonic_search: rows %lld outside [0, 65535]", (long long)rows);
    PU_REQUIRE(nb >= 1 && nb <= ((int64_t)1 << 23) && ld >= nb, "pu_harmonic_search: bad shape (nb %lld, ld %lld)",
               (long long)nb, (long long)ld);
    PU_REQUIRE(!sums || (ld_row >= nb && rows <= INT64_MAX / (ld_row > 0 ? ld_row : 1) && ld_level >= rows * ld_row),
               "pu_harmonic_search: strides of sums too small (ld_row %lld < nb, or ld_level %lld < rows x ld_row)",
               (long long)ld_row, (long long)ld_level);
    PU_REQUIRE(cap >= 0 && (cands || cap == 0), "pu_harmonic_search: cap < 0, or cands NULL with cap > 0");
    PU_REQUIRE(thr && kmin && kmax && count, "pu_harmonic_search: null pointer");
    *count = 0;
    if (rows == 0) return PU_OK;
    PU_REQUIRE(norm, "pu_harmonic_search: null pointer");
    HsLevels lv{};
    for (int l = 0; l < nlev; ++l) lv.thr[l] = thr[l], lv.kmin[l] = kmin[l], lv.kmax[l] = kmax[l];
    const int64_t ntile = (nb + HS_TILE - 1) / HS_TILE, slots = rows * nlev * ntile;
    const HsWs w = hs_carve(pu::Carver(workspace), slots);
    if (int rc = pu::check_workspace("pu_harmonic_search", workspace, workspace_bytes, w.bytes, 256)) return rc;
    hipStream_t s = pu::as_stream(stream);
    const dim3 grid((unsigned)ntile, (unsigned)rows);
    // run on after an error, then synchronise, then report the first one
    int rc = pu::launch("hs_search_kernel<count>", hs_search_kernel<false>, grid, dim3(256), 0, s, norm, nb, ld, (int)nlev,
                        sums, ld_level, ld_row, lv, w.blk, ntile, w.total, cands, cap);
    if (!rc) rc = pu::launch("hs_scan_kernel", hs_scan_kernel, dim3(1), dim3(1024), 0, s, w.blk, slots, w.total);
    if (!rc && cap > 0)
        rc = pu::launch("hs_search_kernel<emit>", hs_search_kernel<true>, grid, dim3(256), 0, s, norm, nb, ld, (int)nlev,
                        nullptr, ld_level, ld_row, lv, w.blk, ntile, w.total, cands, cap);
    if (!rc)
        rc = pu::hip_check(hipMemcpyAsync(count, w.total, sizeof(int64_t), hipMemcpyDeviceToHost, s),
                           "hipMemcpyAsync(candidate count)");
    const int rs = pu::hip_check(hipStreamSynchronize(s), "hipStreamSynchronize(harmonic search)");
    return rc ? rc : rs;
}

}  // extern "C"
