// The fast folding algorithm (FFA) and the boxcar S/N of its folded profiles, for gfx950.
//
//   pu_ffa_describe  the level split and workspace of a call, on the host alone
//   pu_ffa           the transform of rows series of m x p bins and / or its S/N table
//
// No reference counterpart: the definition is this project's (include/pulsarutils_hip.h has it in
// full, tests/ffa_oracle.py restates it in numpy).  In short, with rdiv(a, b) = (2a + b) / (2b):
//
//   F(x) = x for one row; otherwise nh = m / 2, nt = m - nh, H = F(x[:nh]), T = F(x[nh:]),
//   F[s][j] = H[rdiv(s (nh-1), m-1)][j] + T[t][(j + s - t) mod p],  t = rdiv(s (nt-1), m-1).
//
// The tree.  The blocks of recursion depth d are the top-down halvings of [0, m): 2^d blocks of
// floor or ceil(m / 2^d) rows, stored where their rows are (the head's result in the block's first
// nh rows, the tail's behind it), so a level is a pass from one (m, p) plane to another and the
// entry (head row, tail row, rotation) of an output row follows from (m, level, row) alone by a walk
// of `level` halvings.  Every kernel does that walk itself (ffa_entry): there is no table in memory
// and nothing to upload.  The depth is D = ceil(log2 m); blocks of one row occur at depth D - 1
// only (the sizes there are 1 and 2) and are copied, so -0.0 and NaN payloads survive.
//
// The split.  ffa_lds_kernel: one workgroup owns a block of depth D - L, at most B = 2^L rows, loads
// its rows once into one of two ping-pong LDS buffers of B x p floats and runs the L bottom levels
// there; B = the largest power of two with B p <= 16384 (2 x 64 KiB of buffers + 8 KiB of packed
// entries = 136 KiB of the CU's 160), at most 256.  All LDS accesses are 4-byte: the rotated operand
// starts at any bin, and an unaligned 8-byte LDS read is replayed.  ffa_pass_kernel: one level above
// that per launch, a workgroup forms FFA_PASS_ELEMS / p consecutive output rows, whose heads and
// tails are about half as many consecutive rows each: every input row is used by two neighbouring
// output rows of one workgroup, so the level moves one plane in and one plane out of HBM.
// ffa_score_kernel: a wave per profile.  Lane l holds bins l, l + 64 ..; a wave scan per 64 bins
// in float64 builds the prefix sums P[0 .. p] in LDS, P[p] is the total, and the best window of each
// width is max_b (b + w <= p ? P[b + w] - P[b] : (P[p] - P[b]) + P[b + w - p]), the lowest b on
// ties.  With FUSED the profile is the top level's row, formed in registers from the two planes
// below it and never written: the call stores nothing but snr and peak.  Both forms score the same
// float32 profile with the same code, so their results are equal bit for bit.
//
// Every float32 add is the definition's, head operand on the left, nothing fused or reassociated:
// the bits of F depend on (m, p) and the row's samples alone.  No atomics.
#include <hip/hip_runtime.h>

#include <cmath>

#include "pu_common.h"

namespace {

constexpr int FFA_MAX_P = 2048;          // B >= 8 rows of an LDS block
constexpr int FFA_LDS_ELEMS = 16384;     // floats of one ping-pong buffer (64 KiB)
constexpr int FFA_MAX_BLOCK = 256;       // rows of an LDS block: entries pack 8-bit local rows
constexpr int FFA_MAX_LDS_LEVELS = 8;    // log2(FFA_MAX_BLOCK)
constexpr int FFA_PASS_ELEMS = 4096;     // elements a workgroup of a global pass forms
constexpr int FFA_PASS_ROWS = 256;       // ... in at most this many rows
constexpr int FFA_MAX_WIDTHS = 16;
constexpr int FFA_SCORE_WAVES = 4;       // waves (profiles in flight) of a scoring workgroup
constexpr int FFA_SCORE_ROWS = 4;        // profiles a wave scores one after the other
constexpr int FFA_NINFO = 8;
static_assert(2 * FFA_LDS_ELEMS * 4 + FFA_MAX_BLOCK * FFA_MAX_LDS_LEVELS * 4 <= 160 * 1024, "ffa LDS budget");
static_assert(FFA_LDS_ELEMS / FFA_MAX_P >= 2 && (1 << FFA_MAX_LDS_LEVELS) == FFA_MAX_BLOCK, "ffa tiling");

struct ffa_widths {
    int w[FFA_MAX_WIDTHS];
};

// (2a + b) / (2b): a / b rounded half up
__host__ __device__ __forceinline__ int64_t ffa_rdiv(int64_t a, int64_t b) { return (2 * a + b) / (2 * b); }

// The entry of row g (0 <= g < m) at `level`: the block of that depth holding g, then the
// definition's h, t, b inside it.  head, tail: rows of the plane below; tail = -1: copy head.
struct ffa_ent {
    int head, tail, rot;
};
__host__ __device__ __forceinline__ ffa_ent ffa_entry(int m, int level, int g)
{
    int start = 0, size = m;
    for (int d = 0; d < level; ++d) {
        const int nh = size >> 1;
        if (g - start < nh) {
            size = nh;
        } else {
            start += nh;
            size -= nh;
        }
    }
    if (size == 1) return {g, -1, 0};
    const int nh = size >> 1, nt = size - nh, s = g - start;
    const int h = (int)ffa_rdiv((int64_t)s * (nh - 1), size - 1);
    const int t = (int)ffa_rdiv((int64_t)s * (nt - 1), size - 1);
    return {start + h, start + nh + t, s - t};
}

struct ffa_split {
    int depth, lds_levels, block_rows, global_levels;
};
ffa_split ffa_levels(int64_t m, int64_t p)
{
    ffa_split sp{0, 0, 1, 0};
    while (((int64_t)1 << sp.depth) < m) ++sp.depth;
    while (sp.block_rows * 2 <= FFA_MAX_BLOCK && (int64_t)sp.block_rows * 2 * p <= FFA_LDS_ELEMS) sp.block_rows *= 2;
    int cap = 0;
    while ((1 << (cap + 1)) <= sp.block_rows) ++cap;
    sp.lds_levels = sp.depth < cap ? sp.depth : cap;
    sp.global_levels = sp.depth - sp.lds_levels;
    return sp;
}

// The bottom `nlev` levels of one block of depth `depth - nlev` per workgroup, in LDS.
__global__ void __launch_bounds__(1024) ffa_lds_kernel(const float *__restrict__ x, int64_t ld, int m, int p, int depth, int nlev,
                                                       int cap, float *__restrict__ dst, int64_t ld_dst)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ffa_smem[];
    float *cur = reinterpret_cast<float *>(ffa_smem);  // [cap * p]
    float *nxt = cur + (size_t)cap * p;                // [cap * p]
    uint32_t *tab = reinterpret_cast<uint32_t *>(nxt + (size_t)cap * p);  // [nlev][cap]: head | tail << 8 | rot << 16, bit 31 copy
    const int tid = threadIdx.x, nth = blockDim.x;
    const int dl = depth - nlev;
    const int q = (int)(blockIdx.x & ((1u << dl) - 1));
    const int64_t r = blockIdx.x >> dl;
    // block q of depth dl: its bits, most significant first, are the path (0 = head)
    int start = 0, size = m;
    for (int d = 0; d < dl; ++d) {
        const int nh = size >> 1;
        if ((q >> (dl - 1 - d)) & 1) {
            start += nh;
            size -= nh;
        } else {
            size = nh;
        }
    }
    // the block's own sub-tree: level lv of it (0 = the bottom one) has depth nlev - 1 - lv inside it
    for (int e = tid; e < nlev * size; e += nth) {
        const int lv = e / size, i = e - lv * size;
        const ffa_ent en = ffa_entry(size, nlev - 1 - lv, i);
        tab[lv * cap + i] = en.tail < 0 ? (0x80000000u | (uint32_t)en.head)
                                        : ((uint32_t)en.head | (uint32_t)en.tail << 8 | (uint32_t)(en.rot % p) << 16);
    }
    const int total = size * p;  // <= cap * p <= FFA_LDS_ELEMS
    const float *src = x + r * ld + (int64_t)start * p;
    for (int e = tid; e < total; e += nth) cur[e] = src[e];
    __syncthreads();
    const int dq = nth / p, dr = nth - dq * p;  // a thread's step of nth elements as (rows, bins)
    for (int lv = 0; lv < nlev; ++lv) {
        int i = tid / p, j = tid - i * p;
        for (int e = tid; e < total; e += nth) {
            const uint32_t en = tab[lv * cap + i];
            const int h = en & 255;
            float v = cur[h * p + j];
            if (!(en >> 31)) {
                const int t = (en >> 8) & 255;
                int jj = j + (int)((en >> 16) & 0x7fff);
                if (jj >= p) jj -= p;
                v = v + cur[t * p + jj];
            }
            nxt[e] = v;
            i += dq;
            j += dr;
            if (j >= p) {
                j -= p;
                ++i;
            }
        }
        __syncthreads();
        float *sw = cur;
        cur = nxt;
        nxt = sw;
    }
    float *out = dst + r * ld_dst + (int64_t)start * p;
    for (int e = tid; e < total; e += nth) out[e] = cur[e];
}

// One level above the LDS ones: dst rows [g0, g0 + nrow) of series r from the plane below.
__global__ void __launch_bounds__(256) ffa_pass_kernel(const float *__restrict__ src, int64_t ld_src, int m, int p, int level,
                                                       int nrow, int nchunk, float *__restrict__ dst, int64_t ld_dst)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ffa_smem[];
    int *ent = reinterpret_cast<int *>(ffa_smem);  // [nrow][3]
    const int tid = threadIdx.x, nth = blockDim.x;
    const int c = (int)(blockIdx.x % (unsigned)nchunk);
    const int64_t r = blockIdx.x / (unsigned)nchunk;
    const int g0 = c * nrow, left = m - g0, rows = left < nrow ? left : nrow;
    for (int i = tid; i < rows; i += nth) {
        // (levels above the LDS ones have blocks of 2 rows and more: never a copy)
        const ffa_ent en = ffa_entry(m, level, g0 + i);
        ent[3 * i] = en.head;
        ent[3 * i + 1] = en.tail;
        ent[3 * i + 2] = en.rot % p;
    }
    __syncthreads();
    const float *in = src + r * ld_src;
    float *out = dst + r * ld_dst + (int64_t)g0 * p;
    const int total = rows * p, dq = nth / p, dr = nth - dq * p;
    int i = tid / p, j = tid - i * p;
    for (int e = tid; e < total; e += nth) {
        int jj = j + ent[3 * i + 2];
        if (jj >= p) jj -= p;
        out[e] = in[(int64_t)ent[3 * i] * p + j] + in[(int64_t)ent[3 * i + 1] * p + jj];
        i += dq;
        j += dr;
        if (j >= p) {
            j -= p;
            ++i;
        }
    }
}

// The S/N of profiles, a wave per profile.  FUSED: profile s is the top level's row s, formed from
// the plane below (src); otherwise it is row s of src.
template <bool FUSED>
__global__ void __launch_bounds__(64 * FFA_SCORE_WAVES) ffa_score_kernel(const float *__restrict__ src, int64_t ld_src, int m, int p,
                                                                          int nchunk, ffa_widths widths, int nw,
                                                                          const double *__restrict__ sigma,
                                                                          float *__restrict__ snr, int32_t *__restrict__ peak)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ffa_smem[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    double *P = reinterpret_cast<double *>(ffa_smem) + (size_t)wave * (p + 1);  // [p + 1] prefix sums
    const int c = (int)(blockIdx.x % (unsigned)nchunk);
    const int64_t r = blockIdx.x / (unsigned)nchunk;
    const float *in = src + r * ld_src;
    const double sig = sigma ? sigma[r] : 1.0;
    const int nround = (p + 63) >> 6;
    for (int it = 0; it < FFA_SCORE_ROWS; ++it) {  // (uniform over the workgroup: the barriers below)
        const int s = (c * FFA_SCORE_WAVES + wave) * FFA_SCORE_ROWS + it;
        const bool live = s < m;
        const float *head = in, *tail = in;
        int rot = 0;
        if (live) {
            if (FUSED) {
                const ffa_ent en = ffa_entry(m, 0, s);  // (m >= 2 here: a fused level exists)
                head = in + (int64_t)en.head * p;
                tail = in + (int64_t)en.tail * p;
                rot = en.rot % p;
            } else {
                head = in + (int64_t)s * p;
            }
        }
        double carry = 0.0;
        if (lane == 0) P[0] = 0.0;
        for (int k = 0; k < nround; ++k) {
            const int j = k * 64 + lane;
            double v = 0.0;
            if (live && j < p) {
                float f = head[j];
                if (FUSED) {
                    int jj = j + rot;
                    if (jj >= p) jj -= p;
                    f = f + tail[jj];
                }
                v = (double)f;
            }
            // inclusive scan of the wave's 64 bins, then the bins before them
            for (int d = 1; d < 64; d <<= 1) {
                const double up = __shfl_up(v, d, 64);
                if (lane >= d) v += up;
            }
            v += carry;
            if (j < p) P[j + 1] = v;
            carry = __shfl(v, 63, 64);
        }
        __syncthreads();
        const double total = P[p];
        // lane k keeps width k's window; the quotient is then formed once, by all widths' lanes at once
        double my_best = 0.0;
        int my_peak = 0, my_w = 1;
        for (int k = 0; k < nw; ++k) {
            const int w = widths.w[k];
            double best = -INFINITY;
            int bb = 0;
            for (int b = lane; b < p; b += 64) {
                const int e = b + w;
                const double sum = e <= p ? P[e] - P[b] : (total - P[b]) + P[e - p];
                if (sum > best) {
                    best = sum;
                    bb = b;
                }
            }
            for (int d = 32; d >= 1; d >>= 1) {
                const double ob = __shfl_xor(best, d, 64);
                const int obb = __shfl_xor(bb, d, 64);
                if (ob > best || (ob == best && obb < bb)) {
                    best = ob;
                    bb = obb;
                }
            }
            if (lane == k) {
                my_best = best;
                my_peak = bb;
                my_w = w;
            }
        }
        const double wd = (double)my_w, pd = (double)p;
        const double num = my_best - wd * total / pd;
        const double den = sqrt((double)m * wd * (1.0 - wd / pd)) * sig;
        const float my_snr = (float)(num / den);
        if (live && lane < nw) {
            const int64_t o = (r * m + s) * nw + lane;
            snr[o] = my_snr;
            if (peak) peak[o] = my_peak;
        }
        __syncthreads();  // the next profile overwrites P
    }
}

// The buffers of rows x m x p floats a call carves from its workspace (0, 1 or 2).
int ffa_buffers(const ffa_split &sp, bool want_out)
{
    if (want_out) return sp.global_levels >= 1 ? 1 : 0;
    return sp.global_levels >= 2 ? 2 : 1;
}

// Argument checks shared by pu_ffa_describe and pu_ffa.
int ffa_check_shape(const char *who, int64_t rows, int64_t m, int64_t p)
{
    PU_REQUIRE(p >= 2, "%s: p %lld < 2", who, (long long)p);
    PU_REQUIRE(m >= 1, "%s: m %lld < 1", who, (long long)m);
    PU_REQUIRE(rows >= 0, "%s: rows %lld < 0", who, (long long)rows);
    if (p > FFA_MAX_P) {
        pu::set_error("%s: p %lld above %d (an LDS block holds at least 8 rows of p bins twice within 128 KiB)", who, (long long)p,
                      FFA_MAX_P);
        return PU_EUNSUPPORTED;
    }
    if (m > INT32_MAX || (rows > 0 && m > INT32_MAX / rows)) {
        pu::set_error("%s: rows %lld x m %lld above 2^31 - 1 (the grid of one call; larger batches go in several)", who,
                      (long long)rows, (long long)m);
        return PU_EUNSUPPORTED;
    }
    return PU_OK;
}

}  // namespace

extern "C" {

int pu_ffa_describe(int64_t rows, int64_t m, int64_t p, int64_t nwidths, int want_out, int64_t *info, int n)
{
    if (int rc = ffa_check_shape("pu_ffa_describe", rows, m, p)) return rc;
    PU_REQUIRE(nwidths >= 0 && nwidths <= FFA_MAX_WIDTHS, "pu_ffa_describe: nwidths %lld outside 0 .. %d", (long long)nwidths,
               FFA_MAX_WIDTHS);
    PU_REQUIRE(want_out || nwidths >= 1, "pu_ffa_describe: neither the transform nor any width wanted");
    PU_REQUIRE(info && n >= 0, "pu_ffa_describe: null info");
    const ffa_split sp = ffa_levels(m, p);
    const int nbuf = ffa_buffers(sp, want_out != 0);
    const int64_t plane = rows * m * p * 4;  // (rows m < 2^31, p <= 2048: no overflow)
    pu::Carver ws;
    for (int b = 0; b < nbuf; ++b) ws.take<float>((size_t)plane);
    // planes through HBM: the LDS kernel reads x and writes one; every global level reads one and
    // writes one, but a fused top level writes none; an unfused score reads one
    const bool fused = !want_out && sp.global_levels >= 1;
    int64_t planes = 2 + 2 * (int64_t)sp.global_levels;
    if (fused) planes -= 1;
    if (nwidths >= 1 && !fused) planes += 1;
    const int64_t lds_bytes = (int64_t)2 * sp.block_rows * p * 4 + (int64_t)sp.block_rows * FFA_MAX_LDS_LEVELS * 4;
    const int64_t v[FFA_NINFO] = {sp.depth, sp.lds_levels, sp.block_rows, (int64_t)ws.used(), sp.global_levels, FFA_MAX_P,
                                  lds_bytes, planes * plane + (nwidths >= 1 ? rows * m * nwidths * 8 : 0)};
    for (int i = 0; i < n && i < FFA_NINFO; ++i) info[i] = v[i];
    return PU_OK;
}

int pu_ffa(const float *x, int64_t rows, int64_t ld, int64_t m, int64_t p, float *out, int64_t ld_out_row,
           const int32_t *widths, int64_t nwidths, const double *sigma, float *snr, int32_t *peak, void *workspace,
           size_t workspace_bytes, void *stream)
{
    if (int rc = ffa_check_shape("pu_ffa", rows, m, p)) return rc;
    const int64_t mp = m * p;
    PU_REQUIRE(ld >= mp, "pu_ffa: ld %lld < m x p = %lld", (long long)ld, (long long)mp);
    PU_REQUIRE(out || snr, "pu_ffa: both out and snr are NULL");
    PU_REQUIRE(!out || ld_out_row >= mp, "pu_ffa: ld_out_row %lld < m x p = %lld", (long long)ld_out_row, (long long)mp);
    PU_REQUIRE(snr || !peak, "pu_ffa: peak without snr");
    ffa_widths wv{};
    if (snr) {
        PU_REQUIRE(nwidths >= 1 && nwidths <= FFA_MAX_WIDTHS, "pu_ffa: nwidths %lld outside 1 .. %d", (long long)nwidths,
                   FFA_MAX_WIDTHS);
        PU_REQUIRE(widths, "pu_ffa: widths is NULL");
        for (int64_t k = 0; k < nwidths; ++k) {
            PU_REQUIRE(widths[k] >= 1 && widths[k] < p, "pu_ffa: widths[%lld] = %d outside 1 .. p - 1 = %lld", (long long)k,
                       (int)widths[k], (long long)(p - 1));
            wv.w[k] = widths[k];
        }
    }
    const ffa_split sp = ffa_levels(m, p);
    const int nbuf = ffa_buffers(sp, out != nullptr);
    const size_t plane = (size_t)rows * (size_t)mp * 4;
    pu::Carver need;
    for (int b = 0; b < nbuf; ++b) need.take<float>(plane);
    if (rows == 0) return PU_OK;
    if (need.used() > 0)
        if (int rc = pu::check_workspace("pu_ffa", workspace, workspace_bytes, need.used(), 256)) return rc;
    PU_REQUIRE(x, "pu_ffa: x is NULL");
    PU_REQUIRE(reinterpret_cast<uintptr_t>(x) % 4 == 0 && reinterpret_cast<uintptr_t>(out) % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(snr) % 4 == 0 && reinterpret_cast<uintptr_t>(peak) % 4 == 0 &&
                   reinterpret_cast<uintptr_t>(sigma) % 8 == 0,
               "pu_ffa: a pointer is not aligned to its element type");
    pu::Carver ws(workspace);
    float *buf[2] = {nullptr, nullptr};
    for (int b = 0; b < nbuf; ++b) buf[b] = ws.take<float>(plane);
    hipStream_t st = pu::as_stream(stream);
    const int mi = (int)m, pi = (int)p;
    const bool fused = !out && sp.global_levels >= 1;
    const int writes = 1 + sp.global_levels - (fused ? 1 : 0);  // planes written: the LDS kernel's, then one per pass

    // plane i of `writes` alternates between two places: with out, out itself and the one buffer,
    // so that the last plane lands in out (a pass writes the m x p bins of a row only: out's
    // padding stays as it is); without, the two buffers
    auto target = [&](int i, float **ptr, int64_t *ldp) {
        const bool odd = out ? ((writes - 1 - i) & 1) : (i & 1);
        if (out && !odd) {
            *ptr = out;
            *ldp = ld_out_row;
        } else {
            *ptr = out ? buf[0] : buf[odd ? 1 : 0];
            *ldp = mp;
        }
    };
    float *cur;
    int64_t ld_cur;
    target(0, &cur, &ld_cur);
    {
        const int dl = sp.depth - sp.lds_levels;
        const size_t lds = (size_t)2 * sp.block_rows * pi * 4 + (size_t)sp.block_rows * FFA_MAX_LDS_LEVELS * 4;
        const int64_t per_block = (int64_t)(mi < sp.block_rows ? mi : sp.block_rows) * pi;
        const int nth = per_block >= 8192 ? 1024 : 256;
        if (int rc = pu::launch("ffa_lds_kernel", ffa_lds_kernel, dim3((unsigned)(rows << dl)), dim3(nth), lds, st, x, ld, mi, pi,
                                sp.depth, sp.lds_levels, sp.block_rows, cur, ld_cur))
            return rc;
    }
    int nrow = FFA_PASS_ELEMS / pi;
    nrow = nrow < 1 ? 1 : (nrow > FFA_PASS_ROWS ? FFA_PASS_ROWS : nrow);
    const int nchunk = (mi + nrow - 1) / nrow;
    for (int i = 1; i < writes; ++i) {
        float *nxt;
        int64_t ld_nxt;
        target(i, &nxt, &ld_nxt);
        const int level = sp.global_levels - i;
        if (int rc = pu::launch("ffa_pass_kernel", ffa_pass_kernel, dim3((unsigned)(rows * nchunk)), dim3(256), (size_t)nrow * 12, st,
                                (const float *)cur, ld_cur, mi, pi, level, nrow, nchunk, nxt, ld_nxt))
            return rc;
        cur = nxt;
        ld_cur = ld_nxt;
    }
    if (!snr) return PU_OK;
    const int per_wg = FFA_SCORE_WAVES * FFA_SCORE_ROWS, schunk = (mi + per_wg - 1) / per_wg;
    const size_t slds = (size_t)FFA_SCORE_WAVES * (pi + 1) * 8;
    const dim3 sgrid((unsigned)(rows * schunk)), sblock(64 * FFA_SCORE_WAVES);
    if (fused)
        return pu::launch("ffa_score_kernel<fused>", ffa_score_kernel<true>, sgrid, sblock, slds, st, (const float *)cur, ld_cur, mi,
                          pi, schunk, wv, (int)nwidths, sigma, snr, peak);
    return pu::launch("ffa_score_kernel", ffa_score_kernel<false>, sgrid, sblock, slds, st, (const float *)cur, ld_cur, mi, pi, schunk,
                      wv, (int)nwidths, sigma, snr, peak);
}

}  // extern "C"
