// population_ptm_replica_test.cpp -- rdis_amd/csrc/population_grid.hpp without a device: the bytes of one replica of a population
// launch with point-major components, and the members of a launch under a budget.  Checks the functions' properties over a grid
// of arguments (exit code 1 and a line on stderr at the first one that fails), prints "replica blocks cptr_len lds nfree ngfac
// bytes" and "members members budget replica_bytes per_launch" for a few cases (tests/test_population_ptm_cpu.py restates the
// rules) and then "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../rdis_amd/csrc/population_grid.hpp"

using rdis_hip::population_members_per_launch;
using rdis_hip::ptm_population_replica_bytes;

static void fail(const char* what, long long a, long long b, long long c, long long got) {
    std::fprintf(stderr, "%s: %lld %lld %lld -> %lld\n", what, a, b, c, got);
    std::exit(1);
}

int main() {
    const int64_t blocks[] = {0, 1, 8, 63, 64, 65, 200, 7776, 2000000, 40000000};
    const int64_t nfrees[] = {0, 9, 663, 23769};
    const int64_t ngfacs[] = {0, 12, 382116};
    for (int64_t b : blocks) {
        const int64_t cptr = b > 0 ? (b + 63) / 64 + 1 : 0;
        const int64_t alone = ptm_population_replica_bytes(b, cptr, false, 0, 0);
        // the point-major part alone: three arrays of six doubles a block, eight floats per entry of the chunk table
        if (alone != b * 144 + cptr * 32) fail("the point-major part", b, cptr, 0, alone);
        if (alone % 16 != 0) fail("not a multiple of 16 bytes (a replica's exact bounds are read as 16-byte pairs)", b, cptr, 0, alone);
        for (int64_t nf : nfrees)
            for (int64_t ng : ngfacs) {
                // without the LDS-resident kernel its workspace does not count, whatever its size
                if (ptm_population_replica_bytes(b, cptr, false, nf, ng) != alone) fail("the LDS part counted without the kernel", b, nf, ng, alone);
                const int64_t both = ptm_population_replica_bytes(b, cptr, true, nf, ng);
                if (both != alone + 8 * (5 * nf + ng)) fail("the LDS part", b, nf, ng, both);
            }
    }
    // zero blocks: no point-major part, whatever the chunk table's length
    if (ptm_population_replica_bytes(0, 5, false, 0, 0) != 0) fail("zero blocks", 0, 5, 0, ptm_population_replica_bytes(0, 5, false, 0, 0));
    if (ptm_population_replica_bytes(0, 0, true, 100, 7) != 8 * 507) fail("zero blocks beside the LDS part", 0, 100, 7, ptm_population_replica_bytes(0, 0, true, 100, 7));

    const int64_t members[] = {1, 2, 3, 5, 64, 256, 65535, 65536, 1000000};
    const int64_t budgets[] = {0, 1, 28959, 28960, 72400, 1ll << 30, 1ll << 40};
    const int64_t reps[] = {0, 1, 28960, 1120000, 5ll << 30};
    for (int64_t m : members)
        for (int64_t bud : budgets)
            for (int64_t rep : reps) {
                const int64_t R = population_members_per_launch(m, bud, rep);
                if (R < 1) fail("fewer than one member a launch", m, bud, rep, R);
                if (R > m || R > 65535) fail("more members than there are, or than the grid takes", m, bud, rep, R);
                if (rep > 0 && R > 1 && R * rep > bud) fail("beyond the budget", m, bud, rep, R);
                if (rep > 0 && R < m && R < 65535 && (R + 1) * rep <= bud) fail("a member more would fit", m, bud, rep, R);
                if (rep == 0 && R != (m < 65535 ? m : 65535)) fail("a replica of nothing bounds nothing", m, bud, rep, R);
            }
    const struct { int64_t b, cptr; bool lds; int64_t nf, ng; } shown[] = {
        {200, 5, false, 0, 0}, {7776, 123, false, 0, 0}, {2400, 40, true, 501, 3120}, {0, 0, true, 45, 384}, {0, 0, false, 45, 384}, {1, 2, false, 0, 0}};
    for (const auto& s : shown)
        std::printf("replica %lld %lld %d %lld %lld %lld\n", (long long)s.b, (long long)s.cptr, s.lds ? 1 : 0, (long long)s.nf, (long long)s.ng,
                    (long long)ptm_population_replica_bytes(s.b, s.cptr, s.lds, s.nf, s.ng));
    const struct { int64_t m, bud, rep; } launches[] = {{5, 72400, 28960}, {5, 1, 28960}, {5, 1ll << 30, 28960}, {256, 1ll << 30, 1123680}, {256, 1ll << 28, 1123680},
                                                        {100000, 1ll << 30, 64}, {3, 0, 28960}, {7, 12345, 0}};
    for (const auto& s : launches)
        std::printf("members %lld %lld %lld %lld\n", (long long)s.m, (long long)s.bud, (long long)s.rep, (long long)population_members_per_launch(s.m, s.bud, s.rep));
    std::printf("ok\n");
    return 0;
}
