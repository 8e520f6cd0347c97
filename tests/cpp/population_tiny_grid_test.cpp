// population_tiny_grid_test.cpp -- rdis_amd/csrc/population_grid.hpp without a device: the blocks per member of the
// tiny-component solver's population launch.  Checks the function's properties over a grid of arguments (exit code 1 and a
// line on stderr at the first one that fails), prints "case ntiny groups_per_block resident members cap blocks" for a few
// of them (tests/test_population_tiny_cpu.py restates the rule) and then "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../rdis_amd/csrc/population_grid.hpp"

using rdis_hip::tiny_population_blocks;

static int64_t ceil_div(int64_t a, int64_t b) { return (a + b - 1) / b; }

static void fail(const char* what, int64_t ntiny, int gpb, int res, int64_t mem, int cap, int64_t got) {
    std::fprintf(stderr, "%s: ntiny %lld groups_per_block %d resident %d members %lld cap %d -> %lld\n", what, (long long)ntiny, gpb, res,
                 (long long)mem, cap, (long long)got);
    std::exit(1);
}

int main() {
    const int64_t ntinys[] = {1, 2, 3, 4, 5, 30, 63, 64, 65, 300, 4096, 7776, 31104, 500000, 2000000000ll};
    const int gpbs[] = {4, 64};                        // <16, 64>: four groups a block; <4, 256>: sixty-four
    const int resid[] = {0, 1, 2, 255, 256, 512, 2048};
    const int64_t members[] = {1, 2, 3, 4, 7, 64, 255, 256, 257, 2048, 4096, 65535};
    const int caps[] = {0, 1, 2, 100, 1 << 20};
    for (int64_t ntiny : ntinys)
        for (int gpb : gpbs)
            for (int res : resid)
                for (int cap : caps) {
                    int64_t before = -1;
                    for (int64_t mem : members) {
                        const int64_t gx = tiny_population_blocks(ntiny, gpb, res, mem, cap);
                        const int64_t need = ceil_div(ntiny, gpb), r1 = res > 0 ? res : 1;
                        if (gx < 1) fail("fewer than one block", ntiny, gpb, res, mem, cap, gx);
                        if (gx > need) fail("more blocks than first components", ntiny, gpb, res, mem, cap, gx);
                        if (cap > 0 && gx > cap) fail("beyond the cap", ntiny, gpb, res, mem, cap, gx);
                        // without a cap the device is filled when there is enough work
                        if (cap == 0 && gx * mem < (r1 < mem * need ? r1 : mem * need)) fail("the device is not filled", ntiny, gpb, res, mem, cap, gx);
                        // a resident count of 0 is taken as 1
                        if (res == 0 && gx != tiny_population_blocks(ntiny, gpb, 1, mem, cap)) fail("resident 0 is not resident 1", ntiny, gpb, res, mem, cap, gx);
                        // not increasing in the members of the launch (members[] ascends)
                        if (before >= 0 && gx > before) fail("more blocks for more members", ntiny, gpb, res, mem, cap, gx);
                        before = gx;
                    }
                }
    // edge cases, said out loud
    if (tiny_population_blocks(1, 64, 512, 1, 0) != 1) fail("one component", 1, 64, 512, 1, 0, tiny_population_blocks(1, 64, 512, 1, 0));
    if (tiny_population_blocks(7776, 4, 512, 65535, 0) != 1) fail("65535 members", 7776, 4, 512, 65535, 0, tiny_population_blocks(7776, 4, 512, 65535, 0));
    if (tiny_population_blocks(7776, 4, 0, 1, 0) != 1) fail("nothing resident", 7776, 4, 0, 1, 0, tiny_population_blocks(7776, 4, 0, 1, 0));
    const struct { int64_t ntiny; int gpb, res; int64_t mem; int cap; } shown[] = {
        {7776, 4, 4096, 1, 0}, {7776, 4, 4096, 64, 0}, {7776, 64, 256, 64, 0}, {7776, 64, 256, 1, 0}, {300, 64, 256, 2, 1}, {300, 4, 512, 2, 0},
        {300, 4, 512, 4, 0}, {30, 4, 512, 3, 0}, {500000, 64, 256, 3, 0}, {7776, 4, 4096, 256, 5}, {1, 4, 0, 65535, 0}};
    for (const auto& s : shown)
        std::printf("case %lld %d %d %lld %d %d\n", (long long)s.ntiny, s.gpb, s.res, (long long)s.mem, s.cap,
                    tiny_population_blocks(s.ntiny, s.gpb, s.res, s.mem, s.cap));
    std::printf("ok\n");
    return 0;
}
