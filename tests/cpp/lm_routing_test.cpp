// lm_routing_test.cpp -- rdis_amd/host/lm_routing.h without a device (tests/test_lm_levels_cpu.py compiles and runs it).
//   route:    stdin rows "activeCameras factors singleMinFactors", stdout one line per row: 0 (plan) or 1 (a call of its own);
//             the first line is the limit the rule uses (RDIS_HIP_LM_WIDE_MAX_CAMERAS)
//   cameras:  stdin "ncams n" then n variable ids, stdout the number of camera blocks among them
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rdis_amd/host/lm_routing.h"

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "route")) {
        std::printf("%d\n", (int)RDIS_HIP_LM_WIDE_MAX_CAMERAS);
        long long cams, factors, threshold;
        while (std::scanf("%lld %lld %lld", &cams, &factors, &threshold) == 3) std::printf("%d\n", (int)rdis::lmRoute(cams, factors, threshold));
        return 0;
    }
    if (!std::strcmp(argv[1], "cameras")) {
        long long ncams, n;
        if (std::scanf("%lld %lld", &ncams, &n) != 2 || n < 0) return 2;
        std::vector<int64_t> vids((size_t)n);
        for (auto& v : vids) { long long t; if (std::scanf("%lld", &t) != 1) return 2; v = t; }
        std::printf("%lld\n", rdis::lmActiveCameras(vids.data(), vids.size(), ncams));
        return 0;
    }
    return 2;
}
