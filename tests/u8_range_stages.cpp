// Test-side helper of tests/test_u8_range_cpu.py: the stage partition of a subband plan.
//
// The 16-bit slots' flush counter runs across the stages of a DM tile and counts two groups
// per iteration, also when a stage with an odd group count ends on an iteration's first
// group - so how far a packed half climbs between two flushes depends on the stages' group
// counts, which pu_plan_info does not report.  This program plans on the host (the planner's
// own sources, no HIP) and prints, one line per DM tile, the group counts of its stages.
//
//   u8_range_stages NCHAN N NDM GROUP SHAPE LDS_KB SLOT16 SHIFTS_FILE
//
// SHIFTS_FILE: NDM x NCHAN int64, native byte order.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "dedisp_plan.h"
#include "pulsarutils_hip.h"

int main(int argc, char **argv)
{
    if (argc != 9) {
        std::fprintf(stderr, "usage: %s nchan n ndm group shape lds_kb slot16 shifts_file\n", argv[0]);
        return 2;
    }
    const int64_t nchan = std::atoll(argv[1]), n = std::atoll(argv[2]), ndm = std::atoll(argv[3]);
    pu_plan_opts opts{};
    opts.group = std::atoi(argv[4]);
    opts.shape = std::atoi(argv[5]);
    opts.lds_budget_kb = std::atoi(argv[6]);
    opts.u8_dma = -1;
    opts.dt_major = -1;
    opts.slot16 = std::atoi(argv[7]);
    std::vector<int64_t> shifts((size_t)(ndm * nchan));
    std::FILE *f = std::fopen(argv[8], "rb");
    if (!f || std::fread(shifts.data(), sizeof(int64_t), shifts.size(), f) != shifts.size()) {
        std::fprintf(stderr, "cannot read %s\n", argv[8]);
        return 2;
    }
    std::fclose(f);
    pu::PlanProblem pb;
    pu::PlanTables t;
    if (pu::check_plan_args(PU_U8, PU_ACC_NATIVE, nchan, n, shifts.data(), ndm, &opts, pb) != PU_OK ||
        pu::choose_plan(pb, shifts.data(), opts, t) != PU_OK) {
        std::fprintf(stderr, "planning failed: %s\n", pu_last_error());
        return 1;
    }
    std::printf("group %d slot16 %d ngroups %d tiles %d\n", t.group, t.slot16, t.ngroups, t.ndt);
    for (const auto &ts : t.tile_stages) {
        for (int k = 0; k < ts.y; ++k) {
            const auto &st = t.stages[(size_t)(ts.x + k)];
            std::printf("%s%d", k ? " " : "", st.y - st.x);
        }
        std::printf("\n");
    }
    return 0;
}
