// population_grad_members_test.cpp -- rdis_amd/csrc/population_grid.hpp without a device: the bytes of one member's scratch in a
// launch of the population's value + gradient (grad_member_bytes, by branch) and the members of a launch under the budget
// grad_workspace_bytes (grad_members_per_launch).  Checks the functions' properties over a grid of arguments (exit code 1 and a
// line on stderr at the first one that fails), prints "bytes branch ncam_blocks cstage_slots pstage_slots nchunks nslots blocks
// bytes" and "members count budget member_bytes per_launch" for a few cases (tests/test_population_grad_cpu.py restates the
// rules) and then "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../rdis_amd/csrc/population_grid.hpp"

using namespace rdis_hip;

static void fail(const char* what, long long a, long long b, long long c, long long got) {
    std::fprintf(stderr, "%s: %lld %lld %lld -> %lld\n", what, a, b, c, got);
    std::exit(1);
}

static GradMemberShape shape(int64_t ncb, int64_t cs, int64_t ps, int64_t nch, int64_t nslots, int64_t blocks) {
    GradMemberShape s;
    s.ncam_blocks = ncb; s.cstage_slots = cs; s.pstage_slots = ps; s.nchunks = nch; s.nslots = nslots; s.blocks = blocks;
    return s;
}

int main() {
    const int64_t cams[] = {0, 1, 5, 49, 1000}, slots[] = {0, 1, 10, 20, 4000}, chunks[] = {0, 1, 63, 15626};
    for (int64_t ncb : cams)
        for (int64_t cs : slots)
            for (int64_t ps : slots)
                for (int64_t nch : chunks) {
                    // nslots and blocks do not count on the fused branch
                    const int64_t b = grad_member_bytes(GRAD_BRANCH_FUSED, shape(ncb, cs, ps, nch, 123456, 77));
                    const int64_t want = 8 * (14 * ncb + 9 * (cs > 1 ? cs : 1) + 3 * (ps > 1 ? ps : 1) + (nch > 1 ? nch : 1));
                    if (b != want) fail("the fused branch", ncb, cs, nch, b);
                    // zero slots are counted as one: the arrays of a list without staged blocks hold one slot
                    if (grad_member_bytes(GRAD_BRANCH_FUSED, shape(ncb, 0, 0, 0, 0, 0)) != grad_member_bytes(GRAD_BRANCH_FUSED, shape(ncb, 1, 1, 1, 0, 0)))
                        fail("zero slots counted as one", ncb, 0, 0, b);
                }
    const int64_t nslots[] = {0, 12, 4092, 382116, 96000000}, blocks[] = {0, 1, 125, 2048};
    for (int64_t ns : nslots)
        for (int64_t nb : blocks) {
            // the fused counts do not count on the other branches; the short branch has one value partial whatever `blocks`
            const int64_t s = grad_member_bytes(GRAD_BRANCH_SHORT, shape(49, 10, 20, 63, ns, nb));
            const int64_t t = grad_member_bytes(GRAD_BRANCH_TWO_PASS, shape(49, 10, 20, 63, ns, nb));
            if (s != 8 * (ns + 1)) fail("the short branch", ns, nb, 0, s);
            if (t != 8 * (ns + (nb > 1 ? nb : 1))) fail("the two-pass branch", ns, nb, 0, t);
        }
    if (grad_member_bytes(GRAD_BRANCH_NONE, shape(49, 10, 20, 63, 12, 1)) != 0) fail("an empty list needs no scratch", 0, 0, 0, 1);

    const int64_t counts[] = {1, 2, 3, 5, 64, 256, 65535, 65536, 1000000};
    const int64_t budgets[] = {0, 1, 7191, 7192, 17980, 1ll << 30, 1ll << 40};
    const int64_t per[] = {8, 7192, 3056936, 5ll << 30};
    for (int64_t m : counts)
        for (int64_t bud : budgets)
            for (int64_t mb : per) {
                const int64_t R = grad_members_per_launch(m, bud, mb);
                if (R < 1) fail("fewer than one member a launch", m, bud, mb, R);
                if (R > m || R > 65535) fail("more members than there are, or than the grid takes", m, bud, mb, R);
                if (R > 1 && R * mb > bud) fail("beyond the budget", m, bud, mb, R);
                if (R < m && R < 65535 && (R + 1) * mb <= bud) fail("a member more would fit", m, bud, mb, R);
            }
    const struct { int branch; int64_t ncb, cs, ps, nch, nslots, blocks; } shown[] = {
        {GRAD_BRANCH_FUSED, 49, 10, 20, 63, 0, 0},   {GRAD_BRANCH_FUSED, 5, 0, 0, 1, 0, 0},        {GRAD_BRANCH_FUSED, 49, 0, 3, 0, 382116, 125},
        {GRAD_BRANCH_SHORT, 49, 10, 20, 63, 4092, 9}, {GRAD_BRANCH_TWO_PASS, 0, 0, 0, 0, 382116, 125}, {GRAD_BRANCH_TWO_PASS, 0, 0, 0, 0, 30, 0},
        {GRAD_BRANCH_NONE, 49, 10, 20, 63, 12, 1}};
    for (const auto& s : shown)
        std::printf("bytes %d %lld %lld %lld %lld %lld %lld %lld\n", s.branch, (long long)s.ncb, (long long)s.cs, (long long)s.ps, (long long)s.nch,
                    (long long)s.nslots, (long long)s.blocks, (long long)grad_member_bytes(s.branch, shape(s.ncb, s.cs, s.ps, s.nch, s.nslots, s.blocks)));
    const struct { int64_t m, bud, mb; } launches[] = {{5, 17980, 7192}, {5, 1, 7192}, {3, 0, 7192}, {5, 1ll << 30, 7192}, {256, 1ll << 30, 3056936},
                                                       {1000, 1ll << 30, 3056936}, {100000, 1ll << 30, 8}, {70000, 1ll << 40, 7192}};
    for (const auto& s : launches)
        std::printf("members %lld %lld %lld %lld\n", (long long)s.m, (long long)s.bud, (long long)s.mb, (long long)grad_members_per_launch(s.m, s.bud, s.mb));
    std::printf("ok\n");
    return 0;
}
