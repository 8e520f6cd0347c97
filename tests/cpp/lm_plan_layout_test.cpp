// lm_plan_layout_test.cpp -- rdis_amd/csrc/replica_layout.hpp's lm_plan_layout without a device: the two buffers of a
// Levenberg-Marquardt plan's solve.  `out` holds, for every member of the solve, a result row of res_doubles doubles and hist_cap
// history records of four doubles per component, and the member's x[nfree]; `work` holds the workspace slices (ws_doubles doubles) of the members of one
// launch only.  Checked over a grid of arguments and member counts (exit code 1 and a line on stderr at the first check that
// fails): parts in declaration order, no overlap, no gap, every part at a multiple of 8 bytes, total = the sum of the parts, the
// strides the kernel is handed, and members_per_launch at budgets of nothing, just below / exactly / just above one member, and
// exactly `count` members.  Prints "lmplan ncomp res hist_cap nfree ws n r | out: member total, offsets of res hist x, their strides |
// work: total, stride" for the cases tests/test_lm_plan_cpu.py restates as literal arithmetic, then "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../rdis_amd/csrc/replica_layout.hpp"

using namespace rdis_hip;
typedef long long ll;

static void fail(const char* what, ll a, ll b, ll c, ll got) {
    std::fprintf(stderr, "%s: (%lld, %lld, %lld) -> %lld\n", what, a, b, c, got);
    std::exit(1);
}

static void check(const char* name, const ReplicaLayout& l, int64_t R) {
    int64_t sum = 0;
    for (int i = 0; i < l.nparts; ++i) sum += l.bytes[i];
    if (l.member_bytes() != sum) fail(name, 0, R, 0, l.member_bytes());
    if (l.offset(0, R) != 0) fail(name, 1, R, 0, l.offset(0, R));
    for (int i = 0; i < l.nparts; ++i) {
        const int64_t at = l.offset(i, R), end = at + R * l.bytes[i];
        const int64_t next = i + 1 < l.nparts ? l.offset(i + 1, R) : l.total_bytes(R);
        if (l.bytes[i] < 0 || at % 8 != 0) fail(name, 2, R, i, at);          // 8-byte alignment
        if (next != end) fail(name, 3, R, i, next);                          // order, no overlap, no gap; the last part ends the buffer
        if (l.doubles(i) * 8 != l.bytes[i]) fail(name, 4, R, i, l.doubles(i));
    }
    if (l.total_bytes(R) != R * sum) fail(name, 5, R, 0, l.total_bytes(R));    // total = parts
}

int main() {
    const int64_t ncomps[] = {0, 1, 2, 6, 49, 7776}, ress[] = {12}, caps[] = {0, 1, 8, 64}, wss[] = {0, 2, 86, 5050, 1306368}, nfrees[] = {0, 3, 135, 23328};
    const int64_t counts[] = {1, 2, 3, 4, 256, 65535, 70000};
    for (int64_t nc : ncomps)
        for (int64_t rd : ress)
            for (int64_t cap : caps)
                for (int64_t ws : wss)
                  for (int64_t nfr : nfrees) {
                    const LmPlanLayout L = lm_plan_layout(nc, rd, cap, nfr, ws);
                    if (L.out.nparts != 3 || L.work.nparts != 1) fail("part counts", nc, cap, ws, L.out.nparts);
                    if (L.out.bytes[LM_PLAN_RES] != 8 * rd * nc || L.out.bytes[LM_PLAN_HIST] != 32 * cap * nc || L.out.bytes[LM_PLAN_X] != 8 * nfr ||
                        L.work.bytes[LM_PLAN_WS] != 8 * ws)
                        fail("a part's bytes", nc, cap, ws, L.out.member_bytes());
                    for (int64_t count : counts) {
                        check("out", L.out, count);
                        // the history of all members lies behind the result rows of all members
                        if (L.out.offset(LM_PLAN_HIST, count) != count * 8 * rd * nc) fail("hist not behind res", nc, cap, count, L.out.offset(LM_PLAN_HIST, count));
                        if (L.out.offset(LM_PLAN_X, count) != count * (8 * rd * nc + 32 * cap * nc)) fail("x not behind hist", nc, cap, count, L.out.offset(LM_PLAN_X, count));
                        const int64_t mb = L.work.member_bytes();
                        // budgets: nothing, below one member, one member, count members, one byte less, more than enough
                        const int64_t budgets[] = {0, mb - 1, mb, mb + 1, 2 * mb, count * mb - 1, count * mb, (int64_t)1 << 40};
                        for (int64_t bud : budgets) {
                            if (bud < 0) continue;
                            const int64_t R = members_per_launch(count, bud, mb);
                            if (R < 1 || R > count || R > 65535) fail("members outside 1 ... min(count, 65535)", count, bud, mb, R);
                            if (mb > 0 && R > 1 && R * mb > bud) fail("members beyond the budget", count, bud, mb, R);
                            if (mb > 0 && R < count && R < 65535 && (R + 1) * mb <= bud) fail("a member more would fit", count, bud, mb, R);
                            if (mb == 0 && R != (count < 65535 ? count : 65535)) fail("a replica of nothing bounds nothing", count, bud, mb, R);
                            check("work", L.work, R);
                        }
                        if (mb > 0) {
                            if (members_per_launch(count, 0, mb) != 1 || members_per_launch(count, mb - 1, mb) != 1 || members_per_launch(count, mb, mb) != 1)
                                fail("a budget of at most one member: one member a launch", count, mb, 0, members_per_launch(count, mb, mb));
                            if (members_per_launch(count, count * mb, mb) != (count < 65535 ? count : 65535)) fail("a budget of count members: all of them", count, mb, 0, 0);
                            if (count > 1 && count <= 65535 && members_per_launch(count, count * mb - 1, mb) != count - 1) fail("one byte short of count members", count, mb, 0, 0);
                        }
                    }
                }
    // ncomp res hist_cap nfree ws_doubles R(out) R(work)
    const struct { int64_t nc, rd, cap, nfr, ws, n, r; } cases[] = {{1, 12, 64, 135, 5050, 4, 4}, {30, 12, 64, 90, 2580, 4, 2}, {7776, 12, 1, 23328, 1306368, 256, 102},
                                                                   {49, 12, 8, 441, 905520, 1, 1}, {2, 12, 0, 6, 86, 3, 1}, {0, 12, 64, 0, 0, 4, 4}};
    for (const auto& s : cases) {
        const LmPlanLayout L = lm_plan_layout(s.nc, s.rd, s.cap, s.nfr, s.ws);
        std::printf("lmplan %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld %lld\n", (ll)s.nc, (ll)s.rd, (ll)s.cap, (ll)s.nfr, (ll)s.ws,
                    (ll)s.n, (ll)s.r, (ll)L.out.member_bytes(), (ll)L.out.total_bytes(s.n), (ll)L.out.offset(LM_PLAN_RES, s.n), (ll)L.out.offset(LM_PLAN_HIST, s.n),
                    (ll)L.out.offset(LM_PLAN_X, s.n), L.out.doubles(LM_PLAN_RES), L.out.doubles(LM_PLAN_HIST), L.out.doubles(LM_PLAN_X), (ll)L.work.total_bytes(s.r),
                    L.work.doubles(LM_PLAN_WS));
    }
    std::printf("ok\n");
    return 0;
}
