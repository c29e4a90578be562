// Stand-alone run of the host planner (pu_shift_table + pu_plan_describe) over small cases
// of every planning path: linked with the library's own planner objects (planner.o, plan.o)
// and no HIP library - `make plan_check`; the sources under AddressSanitizer and UBSan -
// `make sanitize-plan`.  Prints each case's plan and table digest; exits non-zero if a case
// fails to plan or a subband plan's stages break the order the kernel relies on
// (stages_consecutive).  A case named like a key of tests/golden/plan_tables.json is that
// case (tests/test_planner.py compares the digests).
#include <algorithm>
#include <cinttypes>
#include <cstdio>
#include <random>
#include <vector>

#include "dedisp_plan.h"
#include "pulsarutils_hip.h"

namespace {

int failures = 0;

// What dedisp_sub_kernel relies on in a subband plan (plan_sub states it where it pushes a
// stage): the stages of a DM tile partition its groups in order - stage k + 1 begins at the
// group where stage k ends, the first at group 0, the last ends at ngroups - so the window
// record after a stage's last group is the next stage's first; and likewise its slots -
// stage k + 1's slot records follow stage k's, so the build's read-ahead past a stage's
// last slot stays inside the (padded) table.  The window records are ngroups x W x D words
// per tile.  Returns the first violation, or nullptr.
const char *stages_consecutive(const pu::PlanTables &t)
{
    if (t.group <= 1) return nullptr;  // channel mode: no stages
    const int64_t wd = with_shape(t.shape, [](auto c) { return (int64_t) decltype(c)::W * decltype(c)::D; });
    if ((int64_t)t.recs.size() != (int64_t)t.ndt * t.ngroups * wd) return "window records: not ngroups x W x D per tile";
    if ((int64_t)t.tile_stages.size() != t.ndt) return "tile_stages: not one per tile";
    for (const auto &ts : t.tile_stages) {
        if (ts.y < 1 || ts.x < 0 || (int64_t)ts.x + ts.y > (int64_t)t.stages.size()) return "a tile's stage range";
        for (int k = 0; k < ts.y; ++k) {
            const auto &st = t.stages[(size_t)(ts.x + k)];
            if (st.x >= st.y || st.z >= st.w) return "an empty stage";
            if (st.w > t.nslots_total) return "a stage's slots past the table";
            if (k == 0 ? st.x != 0 : st.x != t.stages[(size_t)(ts.x + k - 1)].y)
                return "a stage does not begin at the group where the previous one ends";
            if (k > 0 && st.z != t.stages[(size_t)(ts.x + k - 1)].w)
                return "a stage's slots do not follow the previous stage's";
        }
        if (t.stages[(size_t)(ts.x + ts.y - 1)].y != t.ngroups) return "a tile's last stage does not end at ngroups";
    }
    return nullptr;
}

void run(const char *name, int dtype, int acc, int64_t nchan, int64_t n, const std::vector<int64_t> &shifts,
         pu_plan_opts opts)
{
    int64_t info[26] = {0};
    uint64_t digest = 0;
    const int64_t ndm = (int64_t)shifts.size() / nchan;
    const int rc = pu_plan_describe(dtype, acc, nchan, n, shifts.data(), ndm, &opts, info, 26, &digest);
    if (rc != PU_OK) {
        std::printf("%-28s FAILED rc %d: %s\n", name, rc, pu_last_error());
        ++failures;
        return;
    }
    {
        pu::PlanProblem pb;
        pu::PlanTables t;
        const char *bad = "planning again failed";
        if (pu::check_plan_args(dtype, acc, nchan, n, shifts.data(), ndm, &opts, pb) == PU_OK &&
            pu::choose_plan(pb, shifts.data(), opts, t) == PU_OK)
            bad = stages_consecutive(t);
        if (bad) {
            std::printf("%-28s FAILED stage order: %s\n", name, bad);
            ++failures;
            return;
        }
    }
    std::printf("%-28s kernel %" PRId64 " group %" PRId64 " dm_tiles %" PRId64 " stages %" PRId64 " lds %" PRId64
                " digest %016" PRIx64 "\n",
                name, info[23], info[10], info[1], info[12], info[7], digest);
}

// the reference's shifts for numpy.linspace(0, 50, ndm) pc cm^-3, 400-500 MHz, 1 ms samples
std::vector<int64_t> grid(int64_t nchan, int64_t ndm = 40)
{
    std::vector<double> dms((size_t)ndm);
    const double step = 50.0 / (double)(ndm - 1);
    for (int64_t d = 0; d < ndm; ++d) dms[(size_t)d] = (double)d * step;
    dms[(size_t)(ndm - 1)] = 50.0;
    std::vector<int64_t> sh((size_t)(ndm * nchan));
    if (pu_shift_table(nchan, dms.data(), ndm, 400.0, 100.0, 1e-3, sh.data()) != PU_OK) {
        std::printf("pu_shift_table failed: %s\n", pu_last_error());
        ++failures;
    }
    return sh;
}

// large random shifts of either sign, sorted per channel: windows that wrap modulo n
std::vector<int64_t> wrapping(int64_t nchan, int64_t ndm)
{
    std::mt19937_64 rng(9);
    std::uniform_int_distribution<int64_t> dist(-20000, 19999);
    std::vector<int64_t> sh((size_t)(ndm * nchan)), col((size_t)ndm);
    for (int64_t c = 0; c < nchan; ++c) {
        for (auto &v : col) v = dist(rng);
        std::sort(col.begin(), col.end());
        for (int64_t d = 0; d < ndm; ++d) sh[(size_t)(d * nchan + c)] = col[(size_t)d];
    }
    return sh;
}

pu_plan_opts opts(int group = 0, int shape = -1, int lds_kb = 0, int u8_dma = -1, int dt_major = -1, int slot16 = -1)
{
    pu_plan_opts o{};
    o.group = group;
    o.shape = shape;
    o.lds_budget_kb = lds_kb;
    o.u8_dma = u8_dma;
    o.dt_major = dt_major;
    o.slot16 = slot16;
    return o;
}

}  // namespace

int main()
{
    const auto g64 = grid(64), g50 = grid(50), g3 = grid(3), g1 = grid(1), wrap = wrapping(48, 70);
    for (int g : {0, 2, 4, 8})
        for (int s16 : {-1, 0}) {
            char name[64];
            std::snprintf(name, sizeof name, "u8_tall_g%d_slot16_%s", g, s16 < 0 ? "None" : "False");
            run(name, PU_U8, PU_ACC_NATIVE, 64, 4096, g64, opts(g, 2, 0, -1, -1, s16));
        }
    run("u8_pair_g4", PU_U8, PU_ACC_NATIVE, 64, 4096, g64, opts(4, 1));
    run("u8 wide g8", PU_U8, PU_ACC_NATIVE, 64, 4096, g64, opts(8, 0));
    run("u8 default", PU_U8, PU_ACC_NATIVE, 64, 4096, g64, opts());
    run("u8_n4099", PU_U8, PU_ACC_NATIVE, 64, 4099, g64, opts());
    run("u8_n4099_tall_g4", PU_U8, PU_ACC_NATIVE, 64, 4099, g64, opts(4, 2));
    run("u8_no_dma_tall_g4", PU_U8, PU_ACC_NATIVE, 64, 4096, g64, opts(4, 2, 0, 0));
    run("u8_acc_f64", PU_U8, PU_ACC_F64, 64, 4096, g64, opts());
    run("f32 default", PU_F32, PU_ACC_NATIVE, 64, 4096, g64, opts());
    run("f32_channel_mode", PU_F32, PU_ACC_NATIVE, 64, 4096, g64, opts(1));
    run("f32 acc f64", PU_F32, PU_ACC_F64, 64, 4096, g64, opts());
    run("f64", PU_F64, PU_ACC_NATIVE, 64, 4096, g64, opts());
    run("f64_acc_f32_g4", PU_F64, PU_ACC_F32, 64, 4096, g64, opts(4));
    run("u8_nchan50_g4", PU_U8, PU_ACC_NATIVE, 50, 4096, g50, opts(4));
    run("f32_nchan50_g4", PU_F32, PU_ACC_NATIVE, 50, 4096, g50, opts(4));
    for (int kb : {64, 8}) {
        char name[64];
        std::snprintf(name, sizeof name, "u8_tall_g4_lds%d", kb);
        run(name, PU_U8, PU_ACC_NATIVE, 64, 4096, g64, opts(4, 2, kb));
        std::snprintf(name, sizeof name, "f32_lds%d", kb);
        run(name, PU_F32, PU_ACC_NATIVE, 64, 4096, g64, opts(0, -1, kb));
    }
    run("u8 wrapping", PU_U8, PU_ACC_NATIVE, 48, 1024, wrap, opts(4, 2));
    run("u8 wrapping lds 64", PU_U8, PU_ACC_NATIVE, 48, 1024, wrap, opts(4, 2, 64));
    run("f32 wrapping", PU_F32, PU_ACC_NATIVE, 48, 1024, wrap, opts());
    run("f64 wrapping", PU_F64, PU_ACC_NATIVE, 48, 1024, wrap, opts());
    for (int dtm : {0, 1}) {
        char name[64];
        std::snprintf(name, sizeof name, "u8 wrapping dt_major %d", dtm);  // 50 DM tiles to order
        run(name, PU_U8, PU_ACC_NATIVE, 48, 1024, wrap, opts(4, 2, 0, -1, dtm));
        std::snprintf(name, sizeof name, "f32_lds64_dt_major_%s", dtm ? "True" : "False");  // 4 DM tiles
        run(name, PU_F32, PU_ACC_NATIVE, 64, 4096, g64, opts(0, -1, 64, -1, dtm));
    }
    run("f32_nchan3", PU_F32, PU_ACC_NATIVE, 3, 4096, g3, opts());
    run("u8_nchan3", PU_U8, PU_ACC_NATIVE, 3, 4096, g3, opts());
    run("f32_nchan1", PU_F32, PU_ACC_NATIVE, 1, 4096, g1, opts());
    run("u8_nchan1", PU_U8, PU_ACC_NATIVE, 1, 4096, g1, opts());
    std::printf("%d case(s) failed\n", failures);
    return failures ? 1 : 0;
}
