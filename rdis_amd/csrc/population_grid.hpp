// population_grid.hpp -- the grid of the tiny-component solver's population launch (solver_quad_population.hpp), the members
// of a launch of the population's evaluation, and the replica of a population launch with point-major components
// (solver_ptm_population.hpp) with the members of a launch it allows, and a member's scratch in a launch of the population's
// value + gradient, pure host functions: no HIP call, no plan (tests/cpp/population_tiny_grid_test.cpp,
// tests/cpp/population_eval_members_test.cpp, tests/cpp/population_ptm_replica_test.cpp and
// tests/cpp/population_grad_members_test.cpp run them without a device).
#pragma once
#include <algorithm>
#include <cstdint>

namespace rdis_hip {

// Blocks per member of a launch of `members` members: every member's `ntiny` components are walked by its own persistent groups,
// groups_per_block to a block.  No more blocks than a member has first components for, and together about what the device holds
// at once (`resident_blocks`; 0 is taken as 1) -- at least one a member, so many members overfill the device and the later
// blocks start as earlier ones end.  `cap` > 0 bounds the result (the plan option tiny_max_blocks).  No bit of a result depends on it.
inline int tiny_population_blocks(int64_t ntiny, int groups_per_block, int resident_blocks, int64_t members, int cap) {
    const int64_t gpb = std::max(groups_per_block, 1), mem = std::max<int64_t>(members, 1), res = std::max(resident_blocks, 1);
    const int64_t need = std::max<int64_t>(1, (std::max<int64_t>(ntiny, 1) + gpb - 1) / gpb);
    int64_t gx = std::min(need, std::max<int64_t>(1, (res + mem - 1) / mem));
    if (cap > 0) gx = std::min<int64_t>(gx, cap);
    return (int)std::min<int64_t>(gx, INT32_MAX);
}

// Members of one launch of the population's evaluation (rdis_hip_population_eval): the member is the grid's second dimension
// (at most 65535), and every member of a launch has scratch of its own -- `partials_per_member` doubles (the chunks' or blocks'
// sums) and, where the launch reads rotation records (`records`), a replica of `nvars` doubles -- within `budget_bytes` (the
// population option eval_workspace_bytes).  At least one member a launch, whatever the budget.  No bit of a result depends on it.
inline int64_t eval_member_bytes(int64_t partials_per_member, int64_t nvars, bool records) {
    return 8 * (std::max<int64_t>(partials_per_member, 1) + (records ? std::max<int64_t>(nvars, 0) : 0));
}
inline int64_t eval_members_per_launch(int64_t members, int64_t budget_bytes, int64_t partials_per_member, int64_t nvars, bool records) {
    const int64_t fit = std::max<int64_t>(1, budget_bytes / eval_member_bytes(partials_per_member, nvars, records));
    return std::max<int64_t>(1, std::min(std::min<int64_t>(members, 65535), fit));
}

// Bytes of one replica of a population launch with point-major components (solver_ptm_population.hpp): the replica's pm_rec, pm_gh
// and pm_bex -- six doubles a point block each -- and its pm_cbox, eight floats per entry of pm_cptr; where the LDS-resident kernel
// runs in the same launch (`lds_part`) its ws and gfac too, 8 (5 nfree + ngfac).  A plan without point blocks has no such part.
inline int64_t ptm_population_replica_bytes(int64_t pm_blocks, int64_t pm_cptr_len, bool lds_part, int64_t nfree, int64_t ngfac) {
    const int64_t ptm = std::max<int64_t>(pm_blocks, 0) * (6 + 6 + 6) * 8 + (pm_blocks > 0 ? std::max<int64_t>(pm_cptr_len, 0) * 32 : 0);
    return ptm + (lds_part ? 8 * (5 * std::max<int64_t>(nfree, 0) + std::max<int64_t>(ngfac, 0)) : 0);
}
// Members of one launch of a population solve: the member is the grid's second dimension (at most 65535) and every member of a
// launch has a replica of `replica_bytes` within `budget_bytes` (the plan option starts_workspace_bytes) -- at least one member a
// launch, whatever the budget; a replica of nothing bounds nothing.  No bit of a result depends on it.
inline int64_t population_members_per_launch(int64_t members, int64_t budget_bytes, int64_t replica_bytes) {
    const int64_t fit = replica_bytes > 0 ? std::max<int64_t>(1, budget_bytes / replica_bytes) : members;
    return std::min(std::min(fit, members), (int64_t)65535);
}

// Bytes of one member's scratch in a launch of the population's value + gradient (rdis_hip_population_eval_grad), by the branch
// rdis_hip_eval_grad takes for the list (grad_branch; the info name of the same name reports it):
//   fused:    the member's camera records (GRAD_MEMBER_REC doubles a camera block), the list's camera and point staging arrays
//             (9 and 3 doubles a slot) and its chunk sums -- a count of zero allocates one, as the list's own arrays do;
//   short:    the per-factor partials gfac[nslots] and the one chunk's sum;
//   two-pass: gfac[nslots] and the blocks' sums.
enum GradBranch { GRAD_BRANCH_NONE = 0, GRAD_BRANCH_FUSED = 1, GRAD_BRANCH_SHORT = 2, GRAD_BRANCH_TWO_PASS = 3 };
constexpr int64_t GRAD_MEMBER_REC = 14;   // grad_fused.hpp: GRAD_REC (rdis_hip.hip asserts them equal)
struct GradMemberShape {
    int64_t ncam_blocks = 0, cstage_slots = 0, pstage_slots = 0, nchunks = 0;   // fused
    int64_t nslots = 0, blocks = 0;                                             // short (blocks not used), two-pass
};
inline int64_t grad_member_bytes(int branch, const GradMemberShape& s) {
    const auto pos = [](int64_t v) { return std::max<int64_t>(v, 0); };
    const auto one = [](int64_t v) { return std::max<int64_t>(v, 1); };
    switch (branch) {
    case GRAD_BRANCH_FUSED: return 8 * (GRAD_MEMBER_REC * pos(s.ncam_blocks) + 9 * one(s.cstage_slots) + 3 * one(s.pstage_slots) + one(s.nchunks));
    case GRAD_BRANCH_SHORT: return 8 * (pos(s.nslots) + 1);
    case GRAD_BRANCH_TWO_PASS: return 8 * (pos(s.nslots) + one(s.blocks));
    default: return 0;
    }
}
// Members of one launch of it: the member is the grid's second dimension (at most 65535) and every member of a launch has
// `member_bytes` of scratch within `budget_bytes` (the population option grad_workspace_bytes) -- at least one member a launch,
// whatever the budget.  No bit of a result depends on it.
inline int64_t grad_members_per_launch(int64_t count, int64_t budget_bytes, int64_t member_bytes) {
    const int64_t fit = std::max<int64_t>(1, budget_bytes / std::max<int64_t>(member_bytes, 1));
    return std::max<int64_t>(1, std::min(std::min<int64_t>(count, 65535), fit));
}

}  // namespace rdis_hip
