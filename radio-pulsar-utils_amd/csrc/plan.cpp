// The dedispersion planner of libpulsarutils_hip: host arithmetic from (problem, shifts,
// options) to the launch geometry and the tables the kernels of dedisperse.hip,
// dedisp_chan.hip and dedisp_f64.hip read.  Compiled by g++ (not hipcc),
// like planner.cpp: no HIP header is in reach, so nothing here can touch a device.
// -ffp-contract=off: the cost model compares float64 sums.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "dedisp_plan.h"
#include "pu_host.h"

namespace pu {

// the table records under the names the kernels know them by
using u32x4 = PlanU32x4;
using i32x4 = PlanI32x4;
using i32x2 = PlanI32x2;

// W (<= 16) records of padding after the slot records: the kernel's build loads each wave's
// next slot record a slot ahead without clamping the index
void pad_slots(PlanTables &t)
{
    if (t.group > 1) t.slots.resize(t.slots.size() + (size_t)16 * slot_stride(8), 0);
}

// FNV-1a (64 bits) over the tables as uploaded (pad_slots applied): each table's name,
// element count and bytes, in the order of the names - not the upload's
uint64_t digest_tables(const PlanTables &t)
{
    uint64_t h = 0xcbf29ce484222325ull;
    auto bytes = [&h](const void *p, size_t n) {
        const unsigned char *b = static_cast<const unsigned char *>(p);
        for (size_t i = 0; i < n; ++i) {
            h ^= b[i];
            h *= 0x100000001b3ull;
        }
    };
    auto table = [&](const char *name, const auto &v) {
        const uint64_t count = v.size();
        bytes(name, strlen(name));
        bytes(&count, sizeof count);
        bytes(v.data(), v.size() * sizeof v[0]);
    };
    table("base", t.base);
    table("count", t.count);
    table("first", t.first);
    table("rec", t.rec);
    table("rec8", t.rec8);
    table("recs", t.recs);
    table("rowlen", t.rowlen);
    table("slots", t.slots);
    table("stages", t.stages);
    table("tile_stages", t.tile_stages);
    table("tiles", t.tiles);
    return h;
}

namespace {

// ---- The planner: plan_channels, plan_sub and choose_plan are host arithmetic from
// (problem, shifts, options) to a PlanTables value; no device is touched (pu_plan_describe
// runs them on a machine without one).

// ---- channel mode (every variant): DM tiles of <= kTPT trials with per-channel shift
// spread <= kMaxSpread; per (tile, channel) the modular row base; u16 window records.
int plan_channels(const PlanProblem &pb, const int64_t *shifts, size_t budget, PlanTables &out)
{
    const int64_t nchan = pb.nchan, n = pb.n, ndm = pb.ndm;
    const int esz = kVariants[pb.variant].lds_elem;
    const int E = 8 / esz;
    out = PlanTables{};
    out.K = E * (kVariants[pb.variant].acc_f64 && esz == 4 ? 2 : 4);  // dedisp_kernel's J
    out.TT = 64 * out.K;
    out.ntt = (int)((n + out.TT - 1) / out.TT);
    std::vector<int32_t> first, count;
    {
        std::vector<int64_t> mn((size_t)nchan), mx((size_t)nchan);
        int64_t i = 0;
        while (i < ndm) {
            const int64_t *s0 = shifts + i * nchan;
            for (int64_t c = 0; c < nchan; ++c) mn[c] = mx[c] = s0[c];
            int64_t j = i + 1;
            while (j < ndm && j - i < kTPT) {
                const int64_t *sj = shifts + j * nchan;
                bool ok = true;
                for (int64_t c = 0; c < nchan && ok; ++c)
                    ok = std::max(mx[c], sj[c]) - std::min(mn[c], sj[c]) <= kMaxSpread;
                if (!ok) break;
                for (int64_t c = 0; c < nchan; ++c) {
                    mn[c] = std::min(mn[c], sj[c]);
                    mx[c] = std::max(mx[c], sj[c]);
                }
                ++j;
            }
            first.push_back((int32_t)i);
            count.push_back((int32_t)(j - i));
            i = j;
        }
    }
    // Balance the tiles: the greedy pass leaves a short last tile (C1: 64 + 36 trials), and
    // a launch of few workgroups per CU runs as long as its busiest CU.  Same tile count,
    // trials dealt in whole waves (kD) as evenly as possible; kept only if every balanced
    // tile still meets the spread limit.
    if (first.size() > 1) {
        const int64_t nt = (int64_t)first.size();
        const int64_t blocks = (ndm + kD - 1) / kD;
        std::vector<int32_t> bf, bc;
        bool ok = true;
        int64_t t0 = 0;
        for (int64_t t = 0; t < nt && ok; ++t) {
            const int64_t nb = blocks / nt + (t < blocks % nt ? 1 : 0);
            const int64_t t1 = std::min<int64_t>(ndm, t0 + nb * kD);
            for (int64_t c = 0; c < nchan && ok; ++c) {
                int64_t m0 = INT64_MAX, m1 = INT64_MIN;
                for (int64_t d = t0; d < t1; ++d) {
                    m0 = std::min(m0, shifts[d * nchan + c]);
                    m1 = std::max(m1, shifts[d * nchan + c]);
                }
                ok = t1 > t0 && m1 - m0 <= kMaxSpread;
            }
            bf.push_back((int32_t)t0);
            bc.push_back((int32_t)(t1 - t0));
            t0 = t1;
        }
        if (ok && t0 == ndm) {
            first.swap(bf);
            count.swap(bc);
        }
    }
    const int ndt = (int)first.size();
    std::vector<int32_t> rowlen(ndt), base((size_t)ndt * nchan);
    std::vector<int32_t> rel((size_t)ndt * nchan * kTPT);  // window shift relative to the row base
    int max_rowlen = 0, max_spread = 0;
    for (int t = 0; t < ndt; ++t) {
        const int64_t i0 = first[t];
        const int cntt = count[t];
        int spread = 0;
        for (int64_t c = 0; c < nchan; ++c) {
            int64_t m0 = INT64_MAX, m1 = INT64_MIN;
            for (int d = 0; d < cntt; ++d) {
                m0 = std::min(m0, shifts[(i0 + d) * nchan + c]);
                m1 = std::max(m1, shifts[(i0 + d) * nchan + c]);
            }
            int64_t b0 = m0 % n;
            if (b0 < 0) b0 += n;
            base[(size_t)t * nchan + c] = (int32_t)b0;
            for (int d = 0; d < kTPT; ++d) {
                const int dd = d < cntt ? d : cntt - 1;  // padding slots repeat the last trial
                rel[((size_t)t * nchan + c) * kTPT + d] = (int32_t)((shifts[(i0 + dd) * nchan + c] - m0) % n);
            }
            spread = std::max(spread, (int)std::min<int64_t>(m1 - m0, n - 1));
        }
        max_spread = std::max(max_spread, spread);
        rowlen[t] = out.TT + spread;
        max_rowlen = std::max(max_rowlen, rowlen[t]);
    }
    const int epp = 256 / esz;
    const bool fsm = kVariants[pb.variant].fsm != 0;
    out.row_stride = (max_rowlen + E + epp - 1) / epp * epp;
    out.small_n = (int64_t)out.row_stride + 2 > n ? 1 : 0;
    const int nbuf = kVariants[pb.variant].dma ? 2 : 1;
    const int64_t chan_bytes = (int64_t)E * out.row_stride * esz;
    if (chan_bytes > 32768) {
        pu::set_error("pu_plan_create: LDS row of %d elements does not fit", out.row_stride);
        return PU_EUNSUPPORTED;
    }
    out.ndt = ndt;
    out.max_spread = max_spread;
    // dedisp_f64_kernel: two float64 row buffers, plus one raw float32 row per channel for
    // float32 inputs (whole 256-byte DMA pieces)
    // (its stride: the row_stride's, as the kernel computes it), and two slots of window
    // records (one 256-byte DMA per channel, + 2 channels of read-ahead each)
    const int64_t raw_bytes = fsm && pb.dtype == PU_F32 ? ((int64_t)out.row_stride * 4 + 255) / 256 * 256 : 0;
    constexpr int64_t kRecChan = 2 * kTPT;  // u16 words
    const int64_t per_chan = nbuf * chan_bytes + raw_bytes + (fsm ? 2 * kRecChan : 0);
    const int64_t fixed = fsm ? 2 * 2 * kRecChan : 0;
    out.ncc = (int)std::max<int64_t>(1, std::min<int64_t>(nchan, (int64_t)((budget - fixed) / per_chan)));
    out.lds_bytes = (size_t)out.ncc * per_chan + fixed;
    if (out.lds_bytes > 160 * 1024) {
        pu::set_error("pu_plan_create: LDS row of %d elements does not fit", out.row_stride);
        return PU_EUNSUPPORTED;
    }
    // window records: per (tile, channel, wave) 8 x u16 = LDS byte offset of each
    // trial's window inside the row slot | (differs from the previous trial) << 15
    // (dedisp_kernel); dedisp_f64_kernel: kF64Trials u16 per (tile, channel, wave), word
    // d = 0 if trial d reads the window of trial d - 1, else 1 + the offset in float64
    // elements, from the chunk's row base, of the window to PREFETCH when trial d's becomes
    // current (the next reloading trial's, after the channel's last reload the next
    // channel's first, 0 + 1 past the chunk: a harmless read of the row base); the reload
    // count of every channel pair the kernel walks (see below) is made even (trial 0 always
    // reloads; an odd count gets a non-reloading trial reloaded too, re-reading its
    // predecessor's window) so that each pair starts and ends in the kernel's state 0.
    // After the records: per (tile, channel, wave) the byte offset of the channel's first
    // window (read at chunk starts).
    const size_t copy_bytes = (size_t)out.row_stride * esz;
    std::vector<u32x4> rec(fsm ? 0 : (size_t)ndt * nchan * kWaves);
    std::vector<uint32_t> rec8(fsm ? (size_t)ndt * nchan * kTPT / 2 + (size_t)ndt * nchan * kF64Waves : 0);
    int64_t f64_reads = 0;  // window reads of dedisp_f64_kernel, per launch and time tile
    if (fsm) {
        if (out.ncc * chan_bytes / 8 + 1 >= (int64_t(1) << 16)) {
            pu::set_error("pu_plan_create: float64 window records overflow");
            return PU_EUNSUPPORTED;
        }
        constexpr int FD = kF64Trials;
        uint32_t *first8 = rec8.data() + (size_t)ndt * nchan * kTPT / 2;
        auto reloads = [&](size_t t, int64_t c, int w, bool (&re)[FD]) {
            const int32_t *rr = rel.data() + (t * nchan + c) * kTPT + w * FD;
            int nre = 0;
            for (int d = 0; d < FD; ++d) {
                re[d] = d == 0 || rr[d] != rr[d - 1];
                nre += re[d];
            }
            return nre;
        };
        auto add_reload = [](bool (&re)[FD]) {  // the last non-reloading trial re-reads
            for (int d = FD - 1; d > 0; --d)
                if (!re[d]) {
                    re[d] = true;
                    return true;
                }
            return false;
        };
        auto emit = [&](size_t t, int64_t c, int w, const bool (&re)[FD]) {
            const int32_t *rr = rel.data() + (t * nchan + c) * kTPT + w * FD;
            const uint32_t cb = (uint32_t)((c % out.ncc) * chan_bytes);
            first8[(t * nchan + c) * kF64Waves + w] = cb + 8u * (uint32_t)rr[0];
            const bool nxt_ok = c + 1 < nchan && (c + 1) % out.ncc != 0;
            const uint32_t nxt_off =
                nxt_ok ? (uint32_t)(cb + chan_bytes + 8u * (uint32_t)rel[((t * nchan + c + 1) * kTPT) + w * FD]) : 0u;
            uint32_t *r = rec8.data() + ((t * nchan + c) * kF64Waves + w) * (FD / 2);
            for (int d = 0; d < FD; ++d) {
                int e = d + 1;
                while (e < FD && !re[e]) ++e;
                const uint32_t off = e < FD ? cb + 8u * (uint32_t)rr[e] : nxt_off;
                const uint32_t word = re[d] ? off / 8u + 1u : 0u;
                r[d / 2] = d % 2 ? r[d / 2] | word << 16 : word;
                if (re[d] && w * FD < count[t]) f64_reads += 1;
            }
        };
        // the kernel walks each chunk's channels in pairs (a lone last one when the chunk's
        // count is odd): a pair's reload count - a lone channel's - is made even, so every
        // pair starts and ends in state 0 (the pair's second channel has an entry for each)
        for (size_t t = 0; t < (size_t)ndt; ++t)
            for (int64_t c0 = 0; c0 < nchan; c0 += out.ncc) {
                const int64_t nc = std::min<int64_t>(out.ncc, nchan - c0);
                for (int64_t ci = 0; ci < nc; ci += 2)
                    for (int w = 0; w < kF64Waves; ++w) {
                        bool ra[FD], rb[FD];
                        int tot = reloads(t, c0 + ci, w, ra);
                        const bool pair = ci + 1 < nc;
                        if (pair) tot += reloads(t, c0 + ci + 1, w, rb);
                        if (tot & 1) {
                            const bool ok = (pair && add_reload(rb)) || add_reload(ra);
                            if (!ok) {
                                pu::set_error("pu_plan_create: float64 reload parity");  // unreachable
                                return PU_EINVAL;
                            }
                        }
                        emit(t, c0 + ci, w, ra);
                        if (pair) emit(t, c0 + ci + 1, w, rb);
                    }
            }
    }
    for (size_t t = 0; t < (size_t)(fsm ? 0 : ndt); ++t)
        for (int64_t c = 0; c < nchan; ++c)
            for (int w = 0; w < kWaves; ++w) {
                const int32_t *rr = rel.data() + (t * nchan + c) * kTPT + w * kD;
                uint32_t words[kD];
                uint32_t prev = 0xffffffffu;
                for (int d = 0; d < kD; ++d) {
                    const uint32_t s = (uint32_t)rr[d];
                    const uint32_t off = E == 2 ? (uint32_t)((s & 1u) * copy_bytes + (s & ~1u) * 4u) : s * 8u;
                    words[d] = off | (off != prev ? 0x8000u : 0u);
                    prev = off;
                }
                uint32_t r[4];
                for (int u = 0; u < 4; ++u) r[u] = words[2 * u] | (words[2 * u + 1] << 16);
                rec[(t * nchan + c) * kWaves + w] = u32x4{r[0], r[1], r[2], r[3]};
            }
    if ((int64_t)out.ndt * out.ntt >= (int64_t(1) << 31)) {
        pu::set_error("pu_plan_create: grid too large");
        return PU_EINVAL;
    }
    out.exec_adds = ndm * nchan * (int64_t)out.ntt * out.TT;
    // LDS bytes per launch (bench.py roofline): per time tile, the staged rows (E copies of
    // row_stride elements per channel) and, per active wave and channel, one J x 8-byte
    // x 64-lane window read for the first trial and for every trial whose window differs
    // from the previous trial's (the reload flag); J = out.K / E reads per window
    {
        const int J = out.K / E;
        int64_t lds_tile = 0;
        for (size_t t = 0; t < (size_t)ndt; ++t) {
            // staged rows (dedisp_f64_kernel on float32: + the raw row's DMA write and the
            // converting pass's read)
            lds_tile += nchan * (int64_t)E * out.row_stride * esz + (raw_bytes ? nchan * 2 * raw_bytes : 0);
            if (fsm) continue;  // the float64 kernel's reads: f64_reads (records, below)
            for (int w = 0; w < kWaves && w * kD < count[t]; ++w)
                for (int64_t c = 0; c < nchan; ++c) {
                    const int32_t *rr = rel.data() + (t * nchan + c) * kTPT + w * kD;
                    int reads = 1;
                    for (int d = 1; d < kD; ++d) reads += rr[d] != rr[d - 1] ? 1 : 0;
                    lds_tile += (int64_t)reads * J * 64 * 8;
                }
        }
        lds_tile += f64_reads * J * 64 * 8;
        out.lds_traffic = lds_tile * out.ntt;
    }
    out.tile_first = first;
    out.tile_count = count;
    out.first = std::move(first);
    out.count = std::move(count);
    out.rowlen = std::move(rowlen);
    out.base = std::move(base);
    out.rec = std::move(rec);
    out.rec8 = std::move(rec8);
    return PU_OK;
}

// ---- subband mode planning (float32 accumulation).  Returns PU_EUNSUPPORTED when one
// trial's group does not fit the LDS budget (the caller then tries a smaller G, then
// channel mode).
constexpr int64_t kSubMaxSpread = 2048;
constexpr int64_t kS16Span = 254;  // 16-bit slots: TT + span + 2 <= 512 elements (four build chunks)
constexpr int64_t kDtMajorItems = 16 * 256;  // below this many items per launch: DM-tile-major order

struct SubSlot {
    int32_t vid;     // relative-shift vector id (per group)
    int64_t lo, hi;  // first-channel shift range of the tile's trials with this vector
    int64_t d0;      // one trial with this vector
};

// Fills ``out`` only on success.
int plan_sub(const PlanProblem &pb, const int64_t *shifts, int G, int shape, size_t budget, PlanTables &out)
{
    const int64_t nchan = pb.nchan, n = pb.n, ndm = pb.ndm;
    const int W = with_shape(shape, [](auto c) { return decltype(c)::W; });
    const int D = with_shape(shape, [](auto c) { return decltype(c)::D; });
    const int64_t TT = with_shape(shape, [](auto c) { return (int64_t)decltype(c)::TT; });
    const int64_t T = (int64_t)W * D;
    const int ngroups = (int)((nchan + G - 1) / G);
    // 8-bit rows are staged as bytes by LDS-DMA when every row window starts on a dword
    // (n % 4 == 0; the row's misalignment base % 4 is folded into the slot sources)
    bool dma8 = pb.dtype == PU_U8 && n % 4 == 0;
    dma8 = dma8 && pu::knob("PU_U8_DMA", pb.opt_u8_dma) != 0;
    const bool dma = pb.dtype == PU_F32 || dma8;
    const int64_t eb = dma8 ? 1 : 4;  // bytes per staged raw element
    // 16-bit integer slots: 8-bit DMA rows in 256-sample time tiles; four
    // alignment copies of >= 384 u16 elements, slots of <= 512 elements (span <= kS16Span)
    // Every G: with the four-per-lane build G = 8 is faster with 16-bit slots too (C3 625
    // trials 113.5 vs 114.3 ms, 5000: 936 vs 957 - DESIGN.md §4.1b, profiles/r06/experiments/
    // slot16/); the per-window cost term below makes the planner pick G per grid
    const int s16opt = pu::knob("PU_SLOT16", pb.opt_slot16);  // -1 auto (= on), 0 off, 1 on
    const bool s16 = dma8 && TT == 256 && s16opt != 0;
    // flush16's carry-free halves: a series sums to at most nchan x 255 <= 2^24 - 1
    if (s16 && nchan * 255 > (int64_t(1) << 24) - 1) {
        pu::set_error("pu_plan_create: 16-bit slots exact only for nchan <= 65793");
        return PU_EINVAL;
    }
    const int64_t ncopies = s16 ? 4 : 2;
    const bool pack_cover = n < (int64_t(1) << 24);  // row bases fit 24 bits: covers above them
    // a stage's raw rows (DMA mode) and its slots share the LDS budget; a stage holds
    // whole groups.  The zero row (DMA mode, partial last group) sits at the end.
    const bool partial = dma && nchan % G != 0;
    const int64_t lds_cap = (int64_t)budget;
    auto S = [&](int64_t d, int64_t c) { return shifts[d * nchan + c]; };
    // elements per staged row: whole 256-byte DMA pieces for 8-bit rows (+3 misalignment)
    auto raw_stride_of = [&](int64_t spread) {
        return dma8 ? (TT + spread + 1 + 3 + 255) / 256 * 256 : (TT + spread + 1 + 63) / 64 * 64;
    };
    // slot copy: len = TT + span + 1 elements + 1 padding float (copy 1's element -1);
    // 16-bit slots: TT + span + 2 u16 (copies 2 and 3 are written 4 bytes down), 64-rounded
    auto copy_of = [&](int64_t span) { return (TT + span + 2 + 63) / 64 * 64 * (s16 ? 2 : 4); };
    auto zero_bytes = [&](int64_t stride) { return partial ? ((stride + 64) * eb + 255) / 256 * 256 : 0; };
    auto raw_bytes = [&](int64_t chans, int64_t stride) { return dma ? (chans * stride * eb + 255) / 256 * 256 : 0; };
    // one group's rows, `slots` slots and the zero row fit the budget
    auto group_fits = [&](int64_t spread, int64_t slots, int64_t span) {
        const int64_t rs = raw_stride_of(spread);
        return raw_bytes(G, rs) + slots * ncopies * copy_of(span) + zero_bytes(rs) <= lds_cap;
    };
    if (!group_fits(0, 1, 0)) return PU_EUNSUPPORTED;

    // ---- relative-shift vector id per (trial, group): v_k = s[c0 + k] - s[c0], k < gs
    std::vector<int32_t> vid((size_t)(ndm * ngroups));
    {
        std::vector<int64_t> order((size_t)ndm);
        for (int g = 0; g < ngroups; ++g) {
            const int64_t c0 = (int64_t)g * G;
            const int gs = (int)std::min<int64_t>(G, nchan - c0);
            auto cmp = [&](int64_t x, int64_t y) {
                for (int k = 1; k < gs; ++k) {
                    const int64_t u = S(x, c0 + k) - S(x, c0), v = S(y, c0 + k) - S(y, c0);
                    if (u != v) return u < v ? -1 : 1;
                }
                return 0;
            };
            for (int64_t d = 0; d < ndm; ++d) order[d] = d;
            std::sort(order.begin(), order.end(), [&](int64_t x, int64_t y) {
                const int c = cmp(x, y);
                return c != 0 ? c < 0 : x < y;
            });
            int32_t id = -1;
            for (int64_t i = 0; i < ndm; ++i) {
                if (i == 0 || cmp(order[i], order[i - 1]) != 0) ++id;
                vid[(size_t)order[i] * ngroups + g] = id;
            }
        }
    }

    // ---- DM tiles: <= T consecutive trials whose channel rows (one group's worth)
    // fit the raw area and whose slots of any one group fit the slot area
    std::vector<int32_t> first, count;
    std::vector<int64_t> spread_t, span_t, smin_t, smax_t;  // smin_t / smax_t: per tile x channel
    std::vector<std::vector<SubSlot>> tslots;       // per tile x group
    {
        std::vector<int64_t> mn((size_t)nchan), mx((size_t)nchan);
        std::vector<std::vector<SubSlot>> cur((size_t)ngroups), nxt((size_t)ngroups);
        int64_t i = 0;
        while (i < ndm) {
            for (int64_t c = 0; c < nchan; ++c) mn[c] = mx[c] = S(i, c);
            for (int g = 0; g < ngroups; ++g) {
                const int64_t b = S(i, (int64_t)g * G);
                cur[g].assign(1, SubSlot{vid[(size_t)i * ngroups + g], b, b, i});
            }
            int64_t spread = 0, span = 0;
            int64_t j = i + 1;
            while (j < ndm && j - i < T) {
                int64_t sp = spread;
                for (int64_t c = 0; c < nchan; ++c)
                    sp = std::max(sp, std::max(mx[c], S(j, c)) - std::min(mn[c], S(j, c)));
                if (sp > kSubMaxSpread) break;
                if (!group_fits(sp, 1, 0)) break;
                int64_t spn = span;
                size_t maxslots = 0;
                for (int g = 0; g < ngroups; ++g) {
                    nxt[g] = cur[g];
                    const int32_t v = vid[(size_t)j * ngroups + g];
                    const int64_t b = S(j, (int64_t)g * G);
                    bool found = false;
                    for (auto &sl : nxt[g])
                        if (sl.vid == v) {
                            sl.lo = std::min(sl.lo, b);
                            sl.hi = std::max(sl.hi, b);
                            spn = std::max(spn, sl.hi - sl.lo);
                            found = true;
                            break;
                        }
                    if (!found) nxt[g].push_back(SubSlot{v, b, b, j});
                    maxslots = std::max(maxslots, nxt[g].size());
                }
                if (!group_fits(sp, (int64_t)maxslots, spn)) break;
                if (s16 && spn > kS16Span) break;  // a 16-bit slot holds <= 512 elements
                for (int64_t c = 0; c < nchan; ++c) {
                    mn[c] = std::min(mn[c], S(j, c));
                    mx[c] = std::max(mx[c], S(j, c));
                }
                std::swap(cur, nxt);
                spread = sp;
                span = spn;
                ++j;
            }
            first.push_back((int32_t)i);
            count.push_back((int32_t)(j - i));
            spread_t.push_back(spread);
            span_t.push_back(span);
            smin_t.insert(smin_t.end(), mn.begin(), mn.end());
            smax_t.insert(smax_t.end(), mx.begin(), mx.end());
            for (int g = 0; g < ngroups; ++g) tslots.push_back(cur[g]);
            i = j;
        }
    }
    const int ndt = (int)first.size();
    int64_t raw_stride = 64, max_spread = 0;
    for (int t = 0; t < ndt; ++t) {
        raw_stride = std::max(raw_stride, raw_stride_of(spread_t[t]));
        max_spread = std::max(max_spread, spread_t[t]);
    }
    // the plan-wide row stride may exceed a tile's own: every tile's largest group must
    // still fit with it
    const int64_t zr = zero_bytes(raw_stride);
    const int64_t stage_cap = lds_cap - zr;  // raw rows + slots of one stage (and of the
                                             // next stage's rows + this stage's slots)
    for (int t = 0; t < ndt; ++t) {
        size_t maxslots = 0;
        for (int g = 0; g < ngroups; ++g) maxslots = std::max(maxslots, tslots[(size_t)t * ngroups + g].size());
        if (raw_bytes(G, raw_stride) + (int64_t)maxslots * ncopies * copy_of(span_t[t]) > stage_cap) {
            pu::set_error("subband mode: a group does not fit the LDS budget");
            return PU_EUNSUPPORTED;
        }
    }

    // ---- stages, slot records, window records (D per wave and group), DMA row bases.
    // LDS layout (the budget): [zero row | slots of the stage ... | raw rows of the stage],
    // the raw rows ending at the top.  Slot and window records hold absolute LDS byte
    // offsets.  A stage's rows land (DMA) while the previous stage is summed, so they
    // must also clear the previous stage's slots.  DMA mode: the G - gs missing channels
    // of a partial last group read the zero row, so the build never branches on the
    // group size.
    const int ms = slot_stride(G);
    const int64_t zero_row_f = 0;
    std::vector<i32x4> tiles((size_t)ndt), stages;
    std::vector<i32x2> tile_stages((size_t)ndt);
    std::vector<int32_t> slotmeta, base;
    std::vector<uint32_t> rec((size_t)ndt * ngroups * W * D);
    std::vector<int64_t> slot_base((size_t)ngroups);
    std::vector<std::vector<int64_t>> slot_off((size_t)ngroups);  // per group: each slot's byte offset
    // 16-bit slots' alignment copies are sized by their own span (round 6; the tile's widest
    // span sized every slot before): more groups per stage
    // 16-bit slots by their own span; float32 slots by theirs rounded up to whole build passes
    // of 64 U elements (sub_item's U), at most the tile's size (sub_item's copy_bytes_of)
    const int64_t UP64 = 64 * std::min<int64_t>((TT + 80 + 63) / 64, (pb.dtype == PU_F64 ? 20 : 40) / G);
    auto slot_copy = [&](size_t t, const SubSlot &sl) {
        if (s16) return copy_of(sl.hi - sl.lo);
        const int64_t whole = (TT + (sl.hi - sl.lo) + 2 + UP64 - 1) / UP64 * UP64 * 4;
        return std::min(whole, copy_of(span_t[t]));
    };
    auto group_slot_bytes = [&](size_t t, int g) {
        int64_t b = 0;
        for (const auto &sl : tslots[t * ngroups + g]) b += ncopies * slot_copy(t, sl);
        return b;
    };
    int64_t prev_slots = 0;
    // element offset of a stage's first raw row: its rows end at the top of LDS
    auto raw_top_f = [&](int g0, int g1) {
        const int64_t nc = std::min<int64_t>((int64_t)g1 * G, nchan) - (int64_t)g0 * G;
        return (lds_cap - raw_bytes(nc, raw_stride)) / eb;
    };
    auto base_of = [&](int64_t smin_c) {
        int64_t b = smin_c % n;
        return b < 0 ? b + n : b;
    };
    int64_t slot_used = 0, max_stage_chans = 0;
    int64_t adds_tile = 0, lds_tile = 0;  // per time tile, summed over DM tiles
    int64_t win16_tile = 0;               // 16-bit-slot windows per time tile
    std::vector<double> tile_cost((size_t)ndt);  // per DM tile: LDS bytes + stage overhead (cost model)
    for (int t = 0; t < ndt; ++t) {
        const int64_t lds_before = lds_tile;
        const int64_t cb = copy_of(span_t[t]);
        const int64_t *smin = smin_t.data() + (size_t)t * nchan;
        const int64_t *smax = smax_t.data() + (size_t)t * nchan;
        const int64_t trials_run = (count[t] + D - 1) / D * D;  // active waves run all D trials
        adds_tile += trials_run * ngroups * TT;
        lds_tile += trials_run * ngroups * TT * (s16 ? 2 : 4);  // sum: one window read per trial and group
        if (s16) win16_tile += trials_run * ngroups;
        const int64_t row_len = TT + spread_t[t] + 1 + (dma8 ? 3 : 0);  // staged elements per row
        tiles[t] = i32x4{first[t], count[t], (int32_t)row_len, (int32_t)cb};
        if (dma)
            for (int64_t c = 0; c < nchan; ++c) {
                int64_t b = dma8 ? base_of(smin[c]) & ~int64_t(3) : base_of(smin[c]);
                if (pack_cover) {
                    // the channel's own DMA cover: its rows need TT + its spread + 1 (+3)
                    // elements, not the tile's widest (C2: 2304 vs 2560 B for most rows)
                    const int64_t len = TT + (smax[c] - smin[c]) + 1 + (dma8 ? 3 : 0);
                    const int64_t cu = (len * eb + 255) / 256;
                    if (cu < 128) b |= cu << 24;
                }
                base.push_back((int32_t)b);
            }
        tile_stages[t] = i32x2{(int32_t)stages.size(), 0};
        prev_slots = 0;
        int g = 0;
        while (g < ngroups) {
            const int32_t s_begin = (int32_t)(slotmeta.size() / ms);
            int64_t used = 0, chans = 0;
            int g_stop = g;  // pass 1: the stage's group range
            {
                int64_t u = 0, ch = 0;
                while (g_stop < ngroups) {
                    const int gs = (int)std::min<int64_t>(G, nchan - (int64_t)g_stop * G);
                    const int64_t nb = group_slot_bytes((size_t)t, g_stop);
                    const int64_t rb = raw_bytes(ch + gs, raw_stride);
                    if (g_stop > g && (rb + u + nb > stage_cap || rb + prev_slots > stage_cap)) break;
                    u += nb;
                    ch += gs;
                    ++g_stop;
                }
                if (raw_bytes(ch, raw_stride) + prev_slots > stage_cap) {
                    pu::set_error("subband mode: consecutive stages do not fit the LDS budget");
                    return PU_EUNSUPPORTED;
                }
                prev_slots = u;
            }
            int g_end = g;
            while (g_end < g_stop) {
                const int64_t c0 = (int64_t)g_end * G;
                const int gs = (int)std::min<int64_t>(G, nchan - c0);
                const auto &sls = tslots[(size_t)t * ngroups + g_end];
                slot_off[g_end].clear();
                for (const auto &sl : sls) {
                    const int64_t cbs = slot_copy((size_t)t, sl);
                    slot_off[g_end].push_back(used);
                    // 16-bit slots: len = the elements the windows read (the build's chunk count)
                    const int64_t len = TT + (sl.hi - sl.lo) + (s16 ? 0 : 1);
                    adds_tile += len * gs;
                    if (s16)  // chunks of 128: 2 G byte reads, 4 copies x 2 B
                        lds_tile += std::max<int64_t>(3, (len + 127) / 128) * 128 * (G + 8);
                    else
                        lds_tile += ((len + 63) / 64 * 64) * (dma ? eb * G + 8 : 8);  // build reads + 2 writes
                    slotmeta.push_back((int32_t)len);
                    slotmeta.push_back((int32_t)(zr + used));
                    slotmeta.push_back((int32_t)c0);
                    slotmeta.push_back(gs);
                    for (int k = 0; k < ms - 4; ++k) {
                        int64_t src = dma && k < G ? zero_row_f : 0;  // missing channel: zero row
                        if (k < gs) {
                            // smallest shift of channel c0+k over the slot's trials
                            const int64_t sk = sl.lo + S(sl.d0, c0 + k) - S(sl.d0, c0);
                            if (dma) {
                                src = raw_top_f(g, g_stop) + (chans + k) * raw_stride + (sk - smin[c0 + k]) +
                                      (dma8 ? (base_of(smin[c0 + k]) & 3) : 0);
                            } else {
                                src = sk % n;
                                if (src < 0) src += n;
                            }
                        }
                        slotmeta.push_back((int32_t)src);
                    }
                    used += ncopies * cbs;
                }
                chans += gs;
                ++g_end;
            }
            // The stages of a tile are consecutive, and dedisp_sub_kernel relies on it twice
            // (plan_check asserts both): in groups - the next stage begins at g_end (g =
            // g_end below), so the window record after a stage's last group is the next
            // stage's first, which the sum carries over instead of loading it again; and in
            // slots - the next stage's s_begin is this stage's end, so the build's slot
            // pointer, stepping past a stage's last slot, reads the next stage's records
            // (or pad_slots' padding).
            stages.push_back(i32x4{g, g_end, s_begin, (int32_t)(slotmeta.size() / ms)});
            tile_stages[t].y++;
            if (dma) lds_tile += chans * ((row_len * eb + 255) / 256 * 256);  // DMA writes
            slot_used = std::max(slot_used, zr + used);
            for (int gg = g; gg < g_end; ++gg) slot_base[gg] = zr;
            max_stage_chans = std::max(max_stage_chans, chans);
            g = g_end;
        }
        for (int gg = 0; gg < ngroups; ++gg) {
            const auto &sls = tslots[(size_t)t * ngroups + gg];
            for (int w = 0; w < W; ++w) {
                uint32_t *r = rec.data() + (((size_t)t * ngroups + gg) * W + w) * D;
                for (int d = 0; d < D; ++d) {
                    const int64_t tr = first[t] + std::min<int64_t>(w * D + d, count[t] - 1);  // padding repeats the last trial
                    const int32_t v = vid[(size_t)tr * ngroups + gg];
                    size_t si = 0;
                    while (sls[si].vid != v) ++si;
                    const int64_t rr = S(tr, (int64_t)gg * G) - sls[si].lo;
                    const int64_t cbs = slot_copy((size_t)t, sls[si]);
                    // copy rr mod 2 (float32) / rr mod 4 (u16), the aligned element below rr
                    r[d] = (uint32_t)(slot_base[gg] + slot_off[gg][si] +
                                      (s16 ? (rr & 3) * cbs + (rr & ~int64_t(3)) * 2 : (rr & 1) * cbs + (rr & ~int64_t(1)) * 4));
                }
            }
        }
        tile_cost[t] = (double)(lds_tile - lds_before) + 3.0e6 * tile_stages[t].y;
    }
    // Item order: DM-tile major (longest items first) when the launch gives the CUs only
    // a few items each, where the tail of unequal items weighs; time-tile major otherwise
    // (the DM tiles of one time tile together on one XCD, sharing L2).  PU_DT_MAJOR
    // overrides (tuning).  DM-tile major sorts the DM tiles by decreasing cost; a tile's
    // trials are named by its record, so the order changes nothing else.  (Sorting them
    // for the time-tile-major order too cost C3 1.1 % - 1109 vs 1122 ms.)
    const int64_t ntt_plan = (n + TT - 1) / TT;
    bool dt_major = (int64_t)ndt * ntt_plan < kDtMajorItems;
    if (pb.opt_dt_major >= 0) dt_major = pb.opt_dt_major != 0;
    dt_major = pu::knob("PU_DT_MAJOR", dt_major ? 1 : 0) != 0;
    if (dt_major) {
        std::vector<int> perm((size_t)ndt);
        for (int t = 0; t < ndt; ++t) perm[t] = t;
        std::stable_sort(perm.begin(), perm.end(), [&](int x, int y) { return tile_cost[x] > tile_cost[y]; });
        std::vector<i32x4> tiles2((size_t)ndt);
        std::vector<i32x2> tile_stages2((size_t)ndt);
        std::vector<int32_t> base2(base.size());
        std::vector<uint32_t> rec2(rec.size());
        const size_t rec_block = (size_t)ngroups * W * D;
        for (int i = 0; i < ndt; ++i) {
            const int t = perm[i];
            tiles2[i] = tiles[t];
            tile_stages2[i] = tile_stages[t];
            if (!base.empty())
                std::copy_n(base.begin() + (size_t)t * nchan, nchan, base2.begin() + (size_t)i * nchan);
            std::copy_n(rec.begin() + (size_t)t * rec_block, rec_block, rec2.begin() + (size_t)i * rec_block);
        }
        tiles.swap(tiles2);
        tile_stages.swap(tile_stages2);
        base.swap(base2);
        rec.swap(rec2);
    }
    const int64_t lds_total = lds_cap;
    if (lds_total > 160 * 1024) {
        pu::set_error("subband mode: %lld bytes of LDS", (long long)lds_total);
        return PU_EUNSUPPORTED;
    }
    const int64_t ntt = (n + TT - 1) / TT;
    if ((int64_t)ndt * ntt >= (int64_t(1) << 31) || (int64_t)slotmeta.size() >= (int64_t(1) << 31)) {
        pu::set_error("pu_plan_create: grid too large");
        return PU_EINVAL;
    }
    out = PlanTables{};
    out.group = G;
    out.ngroups = ngroups;
    out.ndt = ndt;
    out.shape = shape;
    out.K = (int)(TT / 64);
    out.TT = (int)TT;
    out.ntt = (int)ntt;
    out.ncc = (int)max_stage_chans;
    out.raw_stride = (int)raw_stride;
    out.row_stride = (int)raw_stride;
    out.max_spread = (int)max_spread;
    out.small_n = raw_stride + 2 > n ? 1 : 0;
    out.zero_len = zr ? (size_t)(((raw_stride + 64) * eb + 3) / 4) : 0;  // floats
    out.dma8 = dma8 ? 1 : 0;
    out.slot16 = s16 ? 1 : 0;
    out.base_bits = pack_cover ? 24 : 31;
    out.slot_bytes = (size_t)slot_used;
    out.lds_bytes = (size_t)lds_total;
    out.nslots_total = (int)(slotmeta.size() / ms);
    out.nstages = (int64_t)stages.size();
    out.dt_major = dt_major ? 1 : 0;
    out.exec_adds = adds_tile * ntt;
    out.lds_traffic = lds_tile * ntt;
    out.cost_windows16 = win16_tile * ntt;
    out.tile_first.resize((size_t)ndt);
    out.tile_count.resize((size_t)ndt);
    for (int t = 0; t < ndt; ++t) {
        out.tile_first[t] = tiles[t].x;
        out.tile_count[t] = tiles[t].y;
    }
    out.tiles = std::move(tiles);
    out.tile_stages = std::move(tile_stages);
    out.stages = std::move(stages);
    out.slots = std::move(slotmeta);
    out.recs = std::move(rec);
    if (dma) out.base = std::move(base);
    return PU_OK;
}

}  // namespace

// The argument checks of pu_plan_create_ex and pu_plan_describe; fills the problem.
int check_plan_args(int dtype, int acc, int64_t nchan, int64_t n, const int64_t *shifts, int64_t ndm,
                    const pu_plan_opts *opts, PlanProblem &pb)
{
    PU_REQUIRE(opts != nullptr, "pu_plan_create_ex: opts is NULL");
    const int group = opts->group;
    PU_REQUIRE(opts->shape >= -1 && opts->shape <= 2, "pu_plan_create_ex: shape %d not in {-1, 0, 1, 2}", opts->shape);
    PU_REQUIRE(opts->lds_budget_kb == 0 || (opts->lds_budget_kb >= 8 && opts->lds_budget_kb <= 160),
               "pu_plan_create_ex: lds_budget_kb %d not 0 or in [8, 160]", opts->lds_budget_kb);
    PU_REQUIRE(opts->u8_dma >= -1 && opts->u8_dma <= 1 && opts->dt_major >= -1 && opts->dt_major <= 1 &&
                   opts->slot16 >= -1 && opts->slot16 <= 1,
               "pu_plan_create_ex: u8_dma / dt_major / slot16 must be -1, 0 or 1");
    const int v = pick_variant(dtype, acc);
    PU_REQUIRE(v >= 0, "pu_plan_create: unsupported dtype %d", dtype);
    PU_REQUIRE(acc >= PU_ACC_NATIVE && acc <= PU_ACC_F64, "pu_plan_create: bad acc %d", acc);
    PU_REQUIRE(nchan > 0 && nchan < (1 << 30), "pu_plan_create: nchan %lld out of range", (long long)nchan);
    PU_REQUIRE(n > 0 && n < (int64_t(1) << 31) - 65536, "pu_plan_create: nsamples %lld out of range",
               (long long)n);
    PU_REQUIRE(ndm > 0 && ndm < (1 << 30), "pu_plan_create: ndm %lld out of range", (long long)ndm);
    PU_REQUIRE(shifts != nullptr, "pu_plan_create: shifts is NULL");
    PU_REQUIRE(group == 0 || group == 1 || group == 2 || group == 4 || group == 8,
               "pu_plan_create: group %d not in {0 (auto), 1, 2, 4, 8}", group);
    if (dtype == PU_U8 && acc != PU_ACC_F64)
        PU_REQUIRE(nchan <= 65793, "pu_plan_create: u8 f32 accumulation exact only for nchan <= 65793");
    pb.dtype = dtype;
    pb.acc = acc;
    pb.variant = v;
    pb.nchan = nchan;
    pb.n = n;
    pb.ndm = ndm;
    pb.opt_u8_dma = opts->u8_dma < 0 ? 1 : opts->u8_dma;
    pb.opt_dt_major = opts->dt_major;
    pb.opt_slot16 = opts->slot16;
    return PU_OK;
}

// The plan for a validated problem: subband mode with the explicit or automatic group size
// and shape, falling through to smaller groups and then channel mode where a candidate does
// not fit (PU_EUNSUPPORTED); any other error is returned as is.
int choose_plan(const PlanProblem &pb, const int64_t *shifts, const pu_plan_opts &opts, PlanTables &out)
{
    const int64_t nchan = pb.nchan, n = pb.n;
    const VariantInfo &vi = kVariants[pb.variant];
    // subband workgroup shape: 0 = wide (1 WG/CU), 1 = pair (2 WGs/CU), 2 = tall (256
    // trials x 256 samples, 1 WG/CU); -1 = the cost model's choice among wide and tall.
    // LDS budget per workgroup (channel / subband mode).  (Diagnostic build: PU_SUB_SHAPE,
    // PU_LDS_BUDGET_KB and PU_GROUP override the options, for A/B sweeps.)
    const int shape_opt = pu::knob("PU_SUB_SHAPE", opts.shape);
    const int budget_kb = pu::knob("PU_LDS_BUDGET_KB", opts.lds_budget_kb);
    const int shape = shape_opt < 0 ? SUB_WIDE : std::clamp(shape_opt, 0, 2);
    // dedisp_f64_kernel: 80 KiB (two workgroups per CU); dedisp_kernel: 64 KiB
    size_t budget = vi.fsm ? 80 * 1024 : kLdsBudget, sub_budget = shape == SUB_PAIR ? 80 * 1024 : 160 * 1024;
    if (budget_kb > 0) budget = sub_budget = (size_t)std::max(8, budget_kb) * 1024;
    // group size: explicit, else the automatic choice (G = 4 where it is not calibrated);
    // float32 accumulation only (the float64 modes keep the reference's sequential
    // channel order)
    int G = pu::knob("PU_GROUP", opts.group);
    bool auto_g = false;
    if (G == 0) {
        G = 4;
        auto_g = !vi.acc_f64 && nchan > 8;
    }
    G = std::min(G, 8);
    if (vi.acc_f64) G = 1;
    while (G > 1 && G >= nchan) G >>= 1;
    // The automatic choice is calibrated on the wide shape with DMA-staged rows (f32, or
    // u8 with n % 4 == 0); elsewhere the default stays G = 4.
    const bool dma_rows = pb.dtype == PU_F32 || (pb.dtype == PU_U8 && n % 4 == 0);
    if (auto_g && (shape != SUB_WIDE || !dma_rows || budget_kb > 0)) auto_g = false;
    if (auto_g) {
        // Default group size: plan G = 8 and G = 4 on the host and keep the cheaper by the
        // measured cost model: LDS bytes + 3.0e6 B-equivalent per (stage,
        // time tile).  G = 8 halves the LDS traffic at C3 (1240 vs 1328 ms) but its extra
        // stages cost more than that at C2 (22.7 vs 18.4 ms) and C5.  Only the winner's
        // tables are uploaded.  A candidate that does not fit (PU_EUNSUPPORTED) is not
        // viable; any other error is returned as is.
        // Round 6: a 16-bit-slot window costs more than its 512 LDS bytes say (its sum is not
        // LDS-bound: the u16 G = 4 plan lost 6 % to float32 G = 8 at C3's 625-trial shard
        // and won 10 % at its 5000 trials, which the byte model alone ranks the same way at
        // both): + 200 B-equivalent per window, the middle of the (88, 389) the two
        // measurements allow.
        auto cost = [](const PlanTables &q) {
            return (double)q.lds_traffic + 3.0e6 * (double)q.nstages * q.ntt + 200.0 * (double)q.cost_windows16;
        };
        // Round 6, per-slot copy sizes for 16-bit slots: fewer stages for both G, G = 8 most
        // (C3 5000 trials tall G = 4 855.9 -> 847.2 ms, G = 8 936.7 -> 885.3; the 625-trial
        // shard G = 8 114.1 -> 111.9), and the cost above then ranks tall G = 8 first at 5000
        // trials too - wrongly.  Between the two tall 16-bit-slot plans a stage costs 6e6
        // B-equivalents, inside the (4.5e6, 1.0e7) that ranks both measurements right; the
        // winner meets the other shapes under the cost above (6e6 for every plan would pick
        // the wide float32 plan at C3: 1066 vs 847 ms).
        auto cost_tall16 = [](const PlanTables &q) {
            return (double)q.lds_traffic + 6.0e6 * (double)q.nstages * q.ntt + 200.0 * (double)q.cost_windows16;
        };
        // Round 3: the tall shape (256 trials x 256 samples) competes too, with G = 4 and 8.
        // With the permlane epilogue the same cost model ranks every measured case right:
        // C2 tall G4 14.92 ms (wide G4 15.23, tall G8 20.19), C3 tall G8 1042 ms (wide G8
        // 1114; 625 trials 125.6 vs 132.4, tall G4 135.8), C5 tall G4 0.365 (wide 0.374),
        // C4 wide G4 0.581 (100 trials: tall 0.662).  PU_SUB_SHAPE pins the shape.
        const bool try_tall = shape_opt < 0;
        // candidates in the order a tie keeps the earlier: G = 4, G = 8, tall G = 4, tall G = 8
        enum { C4, C8, T4, T8, NCAND };
        PlanTables cand[NCAND];
        int rcs[NCAND] = {PU_EUNSUPPORTED, PU_EUNSUPPORTED, PU_EUNSUPPORTED, PU_EUNSUPPORTED};
        rcs[C8] = plan_sub(pb, shifts, 8, shape, sub_budget, cand[C8]);
        rcs[C4] = plan_sub(pb, shifts, 4, shape, sub_budget, cand[C4]);
        if (try_tall) rcs[T4] = plan_sub(pb, shifts, 4, SUB_TALL, 160 * 1024, cand[T4]);
        if (try_tall) rcs[T8] = plan_sub(pb, shifts, 8, SUB_TALL, 160 * 1024, cand[T8]);
        for (int k : {C8, C4, T4, T8})
            if (rcs[k] != PU_OK && rcs[k] != PU_EUNSUPPORTED) return rcs[k];
        // both tall plans with 16-bit slots: only the cheaper by cost_tall16 competes
        if (rcs[T4] == PU_OK && rcs[T8] == PU_OK && cand[T4].slot16 && cand[T8].slot16)
            rcs[cost_tall16(cand[T8]) < cost_tall16(cand[T4]) ? T4 : T8] = PU_EUNSUPPORTED;
        int keep = -1;
        for (int k = 0; k < NCAND; ++k)
            if (rcs[k] == PU_OK && (keep < 0 || cost(cand[k]) < cost(cand[keep]))) keep = k;
        if (keep >= 0) {
            out = std::move(cand[keep]);
            return PU_OK;
        }
        G = 2;  // 8 and 4 do not fit: continue with the smaller groups
    }
    int rc = PU_EUNSUPPORTED;
    for (; G > 1 && rc == PU_EUNSUPPORTED; G >>= 1) rc = plan_sub(pb, shifts, G, shape, sub_budget, out);
    if (rc == PU_EUNSUPPORTED) rc = plan_channels(pb, shifts, budget, out);
    return rc;
}

// pu_plan_info's fields; cert: {rechecked, nan, why[3], us} of the last call
int fill_info(const PlanProblem &pb, const PlanTables &t, const int64_t (&cert)[6], int64_t *info, int n)
{
    // which kernel a plan's searches launch: 0 dedisp_kernel (channel order), 1 dedisp_f64_kernel,
    // 2 dedisp_sub_kernel (float32 slots), 3 dedisp_sub_kernel with 16-bit integer slots
    const int64_t kernel = t.group > 1 ? (t.slot16 ? 3 : 2) : (kVariants[pb.variant].fsm ? 1 : 0);
    const int64_t v[] = {pb.ndm, t.ndt, t.ntt, t.group > 1 ? with_shape(t.shape, [](auto c) { return decltype(c)::T; }) : kTPT, t.TT, t.ncc,
                         t.row_stride, (int64_t)t.lds_bytes, kVariants[pb.variant].acc_f64, t.max_spread,
                         t.group, t.nslots_total, t.nstages, (int64_t)t.slot_bytes, t.raw_stride,
                         t.exec_adds, t.lds_traffic, cert[0], cert[1], cert[2],
                         cert[3], cert[4], cert[5], kernel, (int64_t)part_elem(pb),
                         kPartStride};
    const int m = std::min<int>(n, (int)(sizeof v / sizeof v[0]));
    for (int k = 0; k < m; ++k) info[k] = v[k];
    return m;
}

}  // namespace pu

extern "C" {

int pu_plan_describe(int dtype, int acc, int64_t nchan, int64_t n, const int64_t *shifts, int64_t ndm,
                     const pu_plan_opts *opts, int64_t *info, int ninfo, uint64_t *tables_digest)
{
    PU_REQUIRE(ninfo >= 0 && (info != nullptr || ninfo == 0), "pu_plan_describe: info is NULL");
    pu::PlanProblem pb;
    pu::PlanTables t;
    int rc = pu::check_plan_args(dtype, acc, nchan, n, shifts, ndm, opts, pb);
    if (!rc) rc = pu::choose_plan(pb, shifts, *opts, t);
    if (rc) return rc;
    pu::pad_slots(t);
    const int64_t no_cert[6] = {0, 0, 0, 0, 0, 0};
    pu::fill_info(pb, t, no_cert, info, ninfo);
    if (tables_digest) *tables_digest = pu::digest_tables(t);
    return PU_OK;
}

}  // extern "C"
