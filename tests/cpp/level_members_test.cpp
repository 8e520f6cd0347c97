// level_members_test.cpp -- rdis_amd/host/level_members.h without a device (tests/test_level_population_cpu.py compiles and runs it).
//   stop:       stdin rows "before objective steptol" (%la hexadecimal or decimal doubles, "nan", "inf"), stdout 1 (the member
//               stops) or 0 per row
//   partition:  stdin "n k", then k rounds of active() flags (0 running / 1 stopped) for rows 0 .. active() - 1; stdout per round
//               one line "moved active | order[0..n) | rowToMember[0..n)", then one last line for restore(): "moved | order | map"
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../rdis_amd/host/level_members.h"

static void put(const std::vector<int64_t>& v) {
    std::printf(" |");
    for (int64_t x : v) std::printf(" %lld", (long long)x);
}

int main(int argc, char** argv) {
    if (argc < 2) return 2;
    if (!std::strcmp(argv[1], "stop")) {
        double before, objective, steptol;
        while (std::scanf("%lf %lf %lf", &before, &objective, &steptol) == 3) std::printf("%d\n", rdis::levelMemberStops(before, objective, steptol) ? 1 : 0);
        return 0;
    }
    if (!std::strcmp(argv[1], "partition")) {
        long long n, k;
        if (std::scanf("%lld %lld", &n, &k) != 2 || n < 0 || k < 0) return 2;
        rdis::LevelMembers rows(n);
        std::vector<int64_t> order;
        for (long long round = 0; round < k; ++round) {
            std::vector<char> stopped((size_t)rows.active());
            for (auto& s : stopped) { int t; if (std::scanf("%d", &t) != 1) return 2; s = (char)t; }
            const bool moved = rows.partition(stopped, order);
            std::printf("%d %lld", moved ? 1 : 0, (long long)rows.active());
            put(order); put(rows.rowToMember());
            std::printf("\n");
        }
        const bool moved = rows.restore(order);
        std::printf("%d", moved ? 1 : 0);
        put(order); put(rows.rowToMember());
        std::printf("\n");
        return 0;
    }
    return 2;
}
