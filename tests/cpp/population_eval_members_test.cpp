// population_eval_members_test.cpp -- rdis_amd/csrc/population_grid.hpp without a device: the members of one launch of the
// population's evaluation.  Checks the function's properties over a grid of arguments (exit code 1 and a line on stderr at the
// first one that fails), prints "case members budget partials nvars records result" for a few of them
// (tests/test_population_eval_cpu.py restates the rule) and then "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../rdis_amd/csrc/population_grid.hpp"

using rdis_hip::eval_member_bytes;
using rdis_hip::eval_members_per_launch;

static void fail(const char* what, int64_t mem, int64_t budget, int64_t part, int64_t nv, int rec, int64_t got) {
    std::fprintf(stderr, "%s: members %lld budget %lld partials %lld nvars %lld records %d -> %lld\n", what, (long long)mem, (long long)budget,
                 (long long)part, (long long)nv, rec, (long long)got);
    std::exit(1);
}

int main() {
    const int64_t members[] = {1, 2, 3, 5, 64, 255, 256, 1000, 65534, 65535, 65536, 1000000, 2147483647ll};
    const int64_t budgets[] = {0, 1, 7, 8, 9, 503, 504, 505, 190656, 381312, 1 << 20, 1ll << 30, 1ll << 40};   // (ascending)
    const int64_t partials[] = {1, 2, 3, 63, 2048, 4194304};
    const int64_t nvars[] = {0, 1, 135, 23769, 100000000};
    for (int64_t mem : members)
        for (int64_t part : partials)
            for (int64_t nv : nvars)
                for (int rec = 0; rec < 2; ++rec) {
                    const int64_t per = 8 * (part + (rec ? nv : 0));
                    if (eval_member_bytes(part, nv, rec != 0) != per) fail("bytes per member", mem, 0, part, nv, rec, eval_member_bytes(part, nv, rec != 0));
                    // the records term is counted only on the records branch
                    if (!rec && eval_member_bytes(part, nv, false) != 8 * part) fail("records counted off the records branch", mem, 0, part, nv, rec, 0);
                    int64_t before = -1;
                    for (int64_t budget : budgets) {
                        const int64_t R = eval_members_per_launch(mem, budget, part, nv, rec != 0);
                        if (R < 1) fail("fewer than one member", mem, budget, part, nv, rec, R);
                        if (R > mem) fail("more than the population", mem, budget, part, nv, rec, R);
                        if (R > 65535) fail("more than the grid's second dimension", mem, budget, part, nv, rec, R);
                        if (budget < per && R != 1) fail("a budget below one member's bytes does not give 1", mem, budget, part, nv, rec, R);
                        if (R > 1 && R * per > budget) fail("beyond the budget", mem, budget, part, nv, rec, R);
                        // everything that fits is taken
                        if (R < mem && R < 65535 && (R + 1) * per <= budget) fail("room left", mem, budget, part, nv, rec, R);
                        if (before >= 0 && R < before) fail("not monotone in the budget", mem, budget, part, nv, rec, R);
                        before = R;
                        // without records the number of variables does not matter
                        if (!rec && R != eval_members_per_launch(mem, budget, part, 0, false)) fail("nvars counted off the records branch", mem, budget, part, nv, rec, R);
                    }
                }
    const struct { int64_t mem, budget, part, nv; int rec; } shown[] = {
        {256, 1ll << 30, 1, 135, 1}, {64, 1ll << 30, 63, 23769, 1}, {5, 2 * 8 * (63 + 23769), 63, 23769, 1}, {5, 2 * 8 * (63 + 23769) - 1, 63, 23769, 1},
        {5, 1, 63, 23769, 1}, {5, 1024, 63, 23769, 0}, {5, 1023, 63, 23769, 0}, {1000000, 1ll << 30, 1, 135, 0}, {1000000, 1ll << 30, 1, 135, 1},
        {1, 0, 1, 0, 0}, {70000, 1ll << 40, 2048, 100000000, 1}, {3, 1ll << 30, 2048, 3600, 0}};
    for (const auto& s : shown)
        std::printf("case %lld %lld %lld %lld %d %lld\n", (long long)s.mem, (long long)s.budget, (long long)s.part, (long long)s.nv, s.rec,
                    (long long)eval_members_per_launch(s.mem, s.budget, s.part, s.nv, s.rec != 0));
    std::printf("ok\n");
    return 0;
}
