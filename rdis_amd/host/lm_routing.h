// lm_routing.h -- which entry of include/rdis_hip.h solves a component that HipLMSubspaceOptimizer::optimizeBatch or the level
// driver (rdis_levels.h) is handed: a resident rdis_hip_lm_plan together with the other components of the call (one launch per
// class, the wide class included), or rdis_hip_lm_optimize on its own (its launches use the whole device).
// Pure host functions: nothing of HIP, no device, no function object -- tests/cpp/lm_routing_test.cpp runs them on the CPU.
#ifndef RDIS_LM_ROUTING_H_
#define RDIS_LM_ROUTING_H_

#include <cstddef>
#include <cstdint>

#include "../../include/rdis_hip.h"   // (plain C: RDIS_HIP_LM_WIDE_MAX_CAMERAS)

namespace rdis {

enum LmRoute { LM_ROUTE_PLAN = 0, LM_ROUTE_SINGLE = 1 };

// activeCameras: camera blocks that hold a free variable of the component (what rdis_hip_lm_plan_create counts against its
// limit); factors: the component's listed factors; singleMinFactors: the option LMsingleMinFactors, 0 (or less) = off.
//   * more than RDIS_HIP_LM_WIDE_MAX_CAMERAS active camera blocks: no plan takes the component -- the single call;
//   * singleMinFactors > 0 and at least that many factors: the single call too (one workgroup of a plan against the whole device);
//   * everything else: the plan.
inline LmRoute lmRoute(long long activeCameras, long long factors, long long singleMinFactors) {
    if (activeCameras > RDIS_HIP_LM_WIDE_MAX_CAMERAS) return LM_ROUTE_SINGLE;
    if (singleMinFactors > 0 && factors >= singleMinFactors) return LM_ROUTE_SINGLE;
    return LM_ROUTE_PLAN;
}

// Camera blocks with a free variable in a bundle adjustment function's free list: variable ids below 9 * ncams are camera
// parameters, nine a camera (BundleAdjustmentFunction::getCamVID).  The list need not be sorted; a camera counts once.
inline long long lmActiveCameras(const int64_t* vids, size_t n, long long ncams) {
    long long count = 0, last = -1;
    bool sorted = true;
    for (size_t i = 0; i < n && sorted; ++i) {
        if (vids[i] >= 9 * ncams) continue;
        const long long cam = vids[i] / 9;
        if (cam < last) sorted = false;
        else if (cam > last) { ++count; last = cam; }
    }
    if (sorted) return count;
    count = 0;   // (unsorted: every camera against the ones before it; lists this long are sorted in practice)
    for (size_t i = 0; i < n; ++i) {
        if (vids[i] >= 9 * ncams) continue;
        bool seen = false;
        for (size_t k = 0; k < i && !seen; ++k) seen = vids[k] < 9 * ncams && vids[k] / 9 == vids[i] / 9;
        if (!seen) ++count;
    }
    return count;
}

}  // namespace rdis
#endif  // RDIS_LM_ROUTING_H_
