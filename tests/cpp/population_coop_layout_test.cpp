// population_coop_layout_test.cpp -- what rdis_hip_plan_solve_population_cooperative takes from pure host functions, without a
// device: the replicas of a member of a cooperative population launch (replica_layout.hpp: population_coop_layout), the members
// of a launch under the budget AND the resident workgroups (coop_members_per_launch), and the entry's refusals
// (population_rules.hpp).  Reads commands from stdin, one a line, and prints one line each, then "ok"
// (tests/test_population_coop_layout_cpu.py restates every figure):
//   layout ngfac xi_doubles groups state_bytes R   -> member total off_gfac off_xi off_state stride_gfac stride_xi
//   members count budget member_bytes cap launch_wg -> R
//   refusal pipelined|grid|residency|hint who n     -> the message (residency: n workgroups a member, a cap of n / 2)
#include <cstdint>
#include <cstdio>
#include <iostream>
#include <sstream>
#include <string>
#include "../../rdis_amd/csrc/population_rules.hpp"
#include "../../rdis_amd/csrc/replica_layout.hpp"

using namespace rdis_hip;
typedef long long ll;

int main() {
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd;
        in >> cmd;
        if (cmd == "layout") {
            ll ngfac, xi, groups, state, R;
            in >> ngfac >> xi >> groups >> state >> R;
            const ReplicaLayout l = population_coop_layout(ngfac, xi, groups, state);
            if (l.nparts != 3) { std::fprintf(stderr, "population_coop_layout has %d parts\n", l.nparts); return 1; }
            std::printf("%lld %lld %lld %lld %lld %lld %lld\n", (ll)l.member_bytes(), (ll)l.total_bytes(R), (ll)l.offset(COOP_REPLICA_GFAC, R),
                        (ll)l.offset(COOP_REPLICA_XI, R), (ll)l.offset(COOP_REPLICA_STATE, R), l.doubles(COOP_REPLICA_GFAC), l.doubles(COOP_REPLICA_XI));
        } else if (cmd == "members") {
            ll count, budget, member, cap, wg;
            in >> count >> budget >> member >> cap >> wg;
            std::printf("%lld\n", (ll)coop_members_per_launch(count, budget, member, cap, wg));
        } else if (cmd == "refusal") {
            std::string which, who;
            ll n = 0;
            in >> which >> who >> n;
            const std::string m = which == "pipelined" ? population_coop_pipelined_refusal(who.c_str())
                                : which == "grid"      ? population_coop_grid_refusal(who.c_str(), n)
                                : which == "residency" ? population_coop_residency_refusal(who.c_str(), n, n / 2)
                                                       : population_coop_hint();
            std::printf("%s\n", m.c_str());
        } else {
            std::fprintf(stderr, "unknown command '%s'\n", cmd.c_str());
            return 1;
        }
    }
    std::printf("ok\n");
    return 0;
}
