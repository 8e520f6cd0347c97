// population_grid.hpp -- the grid of the tiny-component solver's population launch (solver_quad_population.hpp) and the branch and
// shape of a member's scratch in a launch of the population's value + gradient, pure host functions: no HIP call, no plan.  The
// replicas themselves and the members of a launch are replica_layout.hpp's; the three sizes and the three *_members_per_launch
// below are one-line calls of it, under the names tests/cpp/population_eval_members_test.cpp,
// tests/cpp/population_ptm_replica_test.cpp and tests/cpp/population_grad_members_test.cpp check them by
// (tests/cpp/population_tiny_grid_test.cpp: the grid).
#pragma once
#include <algorithm>
#include <cstdint>
#include "replica_layout.hpp"

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

// What the population option eval_workspace_bytes is charged with for a member of one launch of the population's evaluation
// (rdis_hip_population_eval): replica_layout.hpp's two buffers, eval_partial and eval_xr, together.
inline int64_t eval_member_bytes(int64_t partials_per_member, int64_t nvars, bool records) {
    return population_eval_partial_layout(partials_per_member).member_bytes() + population_eval_xr_layout(records, nvars).member_bytes();
}
inline int64_t eval_members_per_launch(int64_t members, int64_t budget_bytes, int64_t partials_per_member, int64_t nvars, bool records) {
    return members_per_launch(members, budget_bytes, eval_member_bytes(partials_per_member, nvars, records));
}

// Bytes of one replica of a population launch with point-major components (ms_ptm) and, where the LDS-resident kernel runs in the
// same launch (`lds_part`), of its ws and gfac in ms_work too.
inline int64_t ptm_population_replica_bytes(int64_t pm_blocks, int64_t pm_cptr_len, bool lds_part, int64_t nfree, int64_t ngfac) {
    return population_ptm_layout(pm_blocks, pm_cptr_len).member_bytes() + population_work_layout(lds_part, nfree, ngfac, false, 0).member_bytes();
}
inline int64_t population_members_per_launch(int64_t members, int64_t budget_bytes, int64_t replica_bytes) {
    return members_per_launch(members, budget_bytes, replica_bytes);
}

// Bytes of one member's scratch in a launch of the population's value + gradient (rdis_hip_population_eval_grad), by the branch
// rdis_hip_eval_grad takes for the list (grad_branch; the info name of the same name reports it):
//   fused:    the member's camera records (GRAD_MEMBER_REC doubles a camera block), the list's camera and point staging arrays
//             (9 and 3 doubles a slot) and its chunk sums -- a count of zero allocates one, as the list's own arrays do;
//   short:    the per-factor partials gfac[nslots] and the one chunk's sum;
//   two-pass: gfac[nslots] and the blocks' sums.
enum GradBranch { GRAD_BRANCH_NONE = 0, GRAD_BRANCH_FUSED = 1, GRAD_BRANCH_SHORT = 2, GRAD_BRANCH_TWO_PASS = 3 };
struct GradMemberShape {
    int64_t ncam_blocks = 0, cstage_slots = 0, pstage_slots = 0, nchunks = 0;   // fused
    int64_t nslots = 0, blocks = 0;                                             // short (blocks not used), two-pass
};
inline ReplicaLayout grad_member_layout(int branch, const GradMemberShape& s) {
    switch (branch) {
    case GRAD_BRANCH_FUSED: return population_grad_fused_layout(s.ncam_blocks, s.cstage_slots, s.pstage_slots, s.nchunks);
    case GRAD_BRANCH_SHORT: return population_grad_list_layout(s.nslots, 1);
    case GRAD_BRANCH_TWO_PASS: return population_grad_list_layout(s.nslots, s.blocks);
    default: return ReplicaLayout();
    }
}
inline int64_t grad_member_bytes(int branch, const GradMemberShape& s) { return grad_member_layout(branch, s).member_bytes(); }
inline int64_t grad_members_per_launch(int64_t count, int64_t budget_bytes, int64_t member_bytes) {
    return members_per_launch(count, budget_bytes, member_bytes);
}

}  // namespace rdis_hip
