// population_grid.hpp -- the grid of the tiny-component solver's population launch (solver_quad_population.hpp), a pure host
// function: no HIP call, no plan (tests/cpp/population_tiny_grid_test.cpp runs it without a device).
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

}  // namespace rdis_hip
