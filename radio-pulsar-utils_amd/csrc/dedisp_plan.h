// Dedispersion geometry shared by the kernel units (dedisperse.hip, dedisp_chan.hip,
// dedisp_f64.hip, dedisp_finalize.hip), the plan object's unit (dedisp_host.hip) and the
// host planner (plan.cpp), and the planner's interface.  Plain C++17: no HIP header, no
// device code, so the planner's unit cannot reach the device.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#include "pulsarutils_hip.h"

#ifdef __HIPCC__
#define PU_HOST_DEVICE __host__ __device__
#else
#define PU_HOST_DEVICE
#endif

// As in dedisp_common.h: each translation unit gets its own copy (the kernels' symbol
// names carry SubCfg).
namespace {

constexpr int kWaves = 8;                 // waves per workgroup (each owns D trials): 2 WGs = 4 waves/SIMD
constexpr int kThreads = kWaves * 64;
constexpr int kD = 8;                     // trials per wave
constexpr int kTPT = kWaves * kD;         // trials per tile
constexpr int kPartStride = 16;           // elements per (trial, time tile) partial record: the
                                          // accumulation type's (float: 64 B, double: 128 B)
constexpr size_t kLdsBudget = 64 * 1024;  // per workgroup: 2 workgroups / CU
constexpr int kMaxSpread = 2048;

// dedisp_f64_kernel's workgroup: 16 waves x 4 trials (= kTPT trials per DM tile)
constexpr int kF64Waves = 16, kF64Trials = 4;

// Workgroup shapes: W waves x D trials per wave, K samples per lane (time tile 64 K).
template <int W_, int D_, int K_>
struct SubCfg {
    static constexpr int W = W_, D = D_, K = K_, J = K_ / 2, TT = 64 * K_, T = W_ * D_, THREADS = 64 * W_;
};
using SubWide = SubCfg<16, 8, 8>;   // 128 trials x 512 samples, one workgroup per CU (160 KiB LDS)
using SubPair = SubCfg<8, 16, 4>;   // 128 trials x 256 samples, two workgroups per CU (80 KiB each)
using SubTall = SubCfg<16, 16, 4>;  // 256 trials x 256 samples, one workgroup per CU (160 KiB LDS)
enum SubShape { SUB_WIDE = 0, SUB_PAIR = 1, SUB_TALL = 2 };

template <class F>
auto with_shape(int shape, F &&f)
{
    if (shape == SUB_PAIR) return f(SubPair{});
    if (shape == SUB_TALL) return f(SubTall{});
    return f(SubWide{});
}

// Slot record (int32): slot length (elements, <= TT + spread + 1), copy-0 byte offset in
// the slot area, first channel, channels in the group, then the G sources of element
// 0 (raw-row float offsets in LDS, or sample indices mod N before adding t0).  Padded
// to a whole s_load.
PU_HOST_DEVICE constexpr int slot_stride(int G) { return G <= 4 ? 8 : 16; }

enum Variant { V_U8_F32, V_F32_F32, V_F64_F64, V_U8_F64, V_F32_F64, V_F64_F32, V_COUNT };

struct VariantInfo {
    int lds_elem, acc_f64, dma, fsm;  // fsm: dedisp_f64_kernel (prefetched windows, u32x8 records)
};

// K samples per lane = (8 / LDS element size) * 4 reads; D = 8 trials per wave
constexpr VariantInfo kVariants[V_COUNT] = {
    {4, 0, 0, 0},  // u8 in, f32 LDS (register staging), f32 acc (exact: sums < 2^24)
    {4, 0, 1, 0},  // f32 in, f32 LDS (DMA), f32 acc
    {8, 1, 1, 1},  // f64 in, f64 LDS (DMA), f64 acc (bit-exact vs reference)
    {4, 1, 0, 0},  // u8 in, f32 LDS, f64 acc
    {8, 1, 1, 1},  // f32 in, raw f32 DMA converted to f64 LDS rows, f64 acc (bit-exact vs reference)
    {4, 0, 0, 0},  // f64 in, f32 LDS (register staging), f32 acc
};

inline int pick_variant(int dtype, int acc)
{
    switch (dtype) {
    case PU_U8: return acc == PU_ACC_F64 ? V_U8_F64 : V_U8_F32;
    case PU_F32: return acc == PU_ACC_F64 ? V_F32_F64 : V_F32_F32;
    case PU_F64: return acc == PU_ACC_F32 ? V_F64_F32 : V_F64_F64;
    default: return -1;
    }
}

}  // namespace

namespace pu {

// Table records the kernels read as clang vector types (u32x4, i32x4, i32x2): the same
// layout as plain structs (dedisp_units.h asserts the sizes; the upload copies bytes).
struct PlanU32x4 {
    uint32_t x, y, z, w;
};
struct PlanI32x4 {
    int32_t x, y, z, w;
};
struct PlanI32x2 {
    int32_t x, y;
};

// The planner's input besides the shift table: the problem and the pu_plan_opts that reach
// plan_sub (group, shape and LDS budget are arguments of the planning functions).
struct PlanProblem {
    int dtype = 0, acc = 0, variant = 0;
    int64_t nchan = 0, n = 0, ndm = 0;
    int opt_u8_dma = -1, opt_dt_major = -1, opt_slot16 = -1;
};

// Everything the planner produces (plan_channels, plan_sub, choose_plan): the geometry the
// launch code reads and the host tables, which the kept plan uploads (DeviceTables) and
// then releases - all but tile_first / tile_count.
struct PlanTables {
    int K = 0, TT = 0;
    int ndt = 0, ntt = 0, ncc = 0, row_stride = 0, small_n = 0, max_spread = 0;
    size_t lds_bytes = 0;
    // subband mode (group > 1)
    int group = 1, ngroups = 0, nslots_total = 0, raw_stride = 0, shape = SUB_WIDE;
    int dma8 = 0;  // subband plan stages 8-bit rows by LDS-DMA (rows must be 4-byte aligned)
    int slot16 = 0;  // subband plan with 16-bit integer slots (8-bit rows)
    int base_bits = 31;  // subband DMA row words: base bits (24: per-channel cover above them)
    size_t slot_bytes = 0, zero_len = 0;
    int64_t exec_adds = 0, lds_traffic = 0;  // per launch (measurement: bench.py roofline)
    int64_t cost_windows16 = 0;  // 16-bit-slot windows per launch (the cost model's extra term)
    int64_t nstages = 0;
    int dt_major = 0;  // subband item order (SubArgs::dt_major)
    std::vector<int32_t> tile_first, tile_count;  // DM tiles in launch order (pu_plan_dm_tiles)
    // channel mode: per tile first trial, trial count and row length; per (tile, channel) the
    // row base (subband DMA mode: the DMA row words); window records (dedisp_kernel: rec,
    // dedisp_f64_kernel: rec8, kF64Trials words per channel and wave + the first-window table)
    std::vector<int32_t> first, count, rowlen, base;
    std::vector<PlanU32x4> rec;
    std::vector<uint32_t> rec8;
    // subband mode: per tile {first, count, raw row length, copy bytes} and {first stage,
    // stage count}, stages {group begin, group end, item begin, item end}, build items
    // (slot records), window records
    std::vector<PlanI32x4> tiles, stages;
    std::vector<PlanI32x2> tile_stages;
    std::vector<int32_t> slots;
    std::vector<uint32_t> recs;
};

// partial records in the plan's accumulation type (the epilogues' sums are float32
// for float32 accumulation: a float record stores them exactly).  static: it reads
// kVariants, which is each translation unit's own copy
static inline size_t part_elem(const PlanProblem &pb) { return kVariants[pb.variant].acc_f64 ? sizeof(double) : sizeof(float); }

// ---- plan.cpp: host arithmetic from (problem, shifts, options) to a PlanTables value

// The argument checks of pu_plan_create_ex and pu_plan_describe; fills the problem.
int check_plan_args(int dtype, int acc, int64_t nchan, int64_t n, const int64_t *shifts, int64_t ndm,
                    const pu_plan_opts *opts, PlanProblem &pb);
// The plan for a validated problem (subband mode, smaller groups, then channel mode).
int choose_plan(const PlanProblem &pb, const int64_t *shifts, const pu_plan_opts &opts, PlanTables &out);
// The padding the kernel's slot-record read-ahead needs; before upload and digest.
void pad_slots(PlanTables &t);
// FNV-1a (64 bits) over the tables as uploaded.
uint64_t digest_tables(const PlanTables &t);
// pu_plan_info's fields; cert: {rechecked, nan, why[3], us} of the last call
int fill_info(const PlanProblem &pb, const PlanTables &t, const int64_t (&cert)[6], int64_t *info, int n);

}  // namespace pu
