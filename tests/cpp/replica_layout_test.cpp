// replica_layout_test.cpp -- rdis_amd/csrc/replica_layout.hpp without a device: the replicas of the five many-member entries.
// Checks over a grid of arguments (zeros for every count, both values of every flag, launches of 1, 2 and 65535 members; exit
// code 1 and a line on stderr at the first check that fails) that a layout's parts lie in declaration order, do not overlap,
// start at multiples of 8 bytes, end exactly at total_bytes(R) == R * member_bytes(), and that a part of zero bytes moves no other
// part; and that members_per_launch returns what each of the four rules it replaced returned over that rule's domain.  Prints a
// line per layout and case, "<layout> <arguments> <R> <sizes, offsets, strides>", and "members count budget member_bytes
// per_launch" (tests/test_replica_layout_cpu.py restates every figure from the expressions the entries had) and then "ok".
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include "../../rdis_amd/csrc/replica_layout.hpp"

using namespace rdis_hip;
typedef long long ll;

static void fail(const char* what, const char* layout, ll part, ll R, ll got) {
    std::fprintf(stderr, "%s: %s part %lld, %lld members -> %lld\n", what, layout, part, R, got);
    std::exit(1);
}

static const int64_t LAUNCHES[] = {1, 2, 65535};

static void check(const char* name, const ReplicaLayout& l) {
    if (l.nparts < 1 || l.nparts > ReplicaLayout::MAX_PARTS) fail("part count", name, l.nparts, 0, l.nparts);
    int64_t sum = 0;
    for (int i = 0; i < l.nparts; ++i) {
        if (l.bytes[i] < 0) fail("a part of negative size", name, i, 0, l.bytes[i]);
        sum += l.bytes[i];
    }
    if (l.member_bytes() != sum) fail("member_bytes is not the sum of the parts", name, 0, 0, l.member_bytes());
    for (int64_t R : LAUNCHES) {
        if (l.offset(0, R) != 0) fail("the first part does not start the buffer", name, 0, R, l.offset(0, R));
        for (int i = 0; i < l.nparts; ++i) {
            const int64_t at = l.offset(i, R), end = at + R * l.bytes[i];
            if (at % 8 != 0) fail("a part off a multiple of 8 bytes", name, i, R, at);
            // declaration order without overlap or gap: the next part starts where this one ends, the last ends the buffer
            const int64_t next = i + 1 < l.nparts ? l.offset(i + 1, R) : l.total_bytes(R);
            if (next < at) fail("parts out of declaration order", name, i, R, next);
            if (next < end) fail("parts overlap", name, i, R, next);
            if (next != end) fail("a gap behind a part", name, i, R, next);
            static char base[1 << 20];   // (pointers are formed where the whole launch fits it)
            if (l.total_bytes(R) <= (int64_t)sizeof base && reinterpret_cast<char*>(l.at<double>(base, i, R)) - base != at) fail("at() off offset()", name, i, R, at);
            if (l.doubles(i) * 8 != l.bytes[i]) fail("a stride in doubles off the part's bytes", name, i, R, l.doubles(i));
        }
        if (l.total_bytes(R) != R * l.member_bytes()) fail("total_bytes", name, 0, R, l.total_bytes(R));
        // a part of zero bytes takes no room: the layout without it has every other part where it was
        for (int z = 0; z < l.nparts; ++z) {
            if (l.bytes[z] != 0) continue;
            int64_t b[ReplicaLayout::MAX_PARTS + 1] = {0, 0, 0, 0, 0};
            int n = 0;
            for (int i = 0; i < l.nparts; ++i)
                if (i != z) b[n++] = l.bytes[i];
            if (n == 0) continue;
            const ReplicaLayout w(n, b[0], b[1], b[2], b[3]);
            for (int i = 0, j = 0; i < l.nparts; ++i) {
                if (i == z) continue;
                if (w.offset(j, R) != l.offset(i, R)) fail("a part of zero bytes moved another part", name, i, R, l.offset(i, R));
                ++j;
            }
            if (w.total_bytes(R) != l.total_bytes(R)) fail("a part of zero bytes changed the total", name, z, R, l.total_bytes(R));
        }
    }
}

// ---- the four rules members_per_launch replaced, as they stood ----
static int64_t rule_eval(int64_t members, int64_t budget, int64_t bytes) {
    const int64_t fit = std::max<int64_t>(1, budget / bytes);
    return std::max<int64_t>(1, std::min(std::min<int64_t>(members, 65535), fit));
}
static int64_t rule_population(int64_t members, int64_t budget, int64_t replica) {
    const int64_t fit = replica > 0 ? std::max<int64_t>(1, budget / replica) : members;
    return std::min(std::min(fit, members), (int64_t)65535);
}
static int64_t rule_grad(int64_t count, int64_t budget, int64_t bytes) {
    const int64_t fit = std::max<int64_t>(1, budget / std::max<int64_t>(bytes, 1));
    return std::max<int64_t>(1, std::min(std::min<int64_t>(count, 65535), fit));
}
static int64_t rule_starts(int64_t nstarts, int64_t budget, size_t rep_bytes) {
    int64_t R = rep_bytes ? std::max<int64_t>(1, budget / (int64_t)rep_bytes) : nstarts;
    R = std::min(std::min(R, nstarts), (int64_t)65535);
    return R;
}

static void print_offsets(const ReplicaLayout& l, int64_t R) {
    std::printf(" %lld %lld", (ll)l.member_bytes(), (ll)l.total_bytes(R));
    for (int i = 0; i < l.nparts; ++i) std::printf(" %lld", (ll)l.offset(i, R));
}

int main() {
    const int64_t nfrees[] = {0, 1, 9, 663, 23769}, ngfacs[] = {0, 12, 4092, 382116}, nvarss[] = {0, 1, 135, 23769};
    for (int64_t nf : nfrees)
        for (int64_t ng : ngfacs)
            for (int64_t nv : nvarss)
                for (int a = 0; a < 2; ++a) {
                    check("multi-start ms_work", starts_work_layout(nf, ng, a != 0, nv));
                    check("ms_dir", solve_dir_layout(a != 0, nv));
                    for (int b = 0; b < 2; ++b) check("population ms_work", population_work_layout(a != 0, nf, ng, b != 0, nv));
                }
    const int64_t blocks[] = {0, 1, 8, 63, 64, 65, 200, 7776, 2000000}, cptrs[] = {0, 1, 2, 5, 123, 31251};
    for (int64_t b : blocks)
        for (int64_t cp : cptrs) {
            const ReplicaLayout l = population_ptm_layout(b, cp);
            check("population ms_ptm", l);
            if (b == 0 && l.member_bytes() != 0) fail("a plan without point blocks has a point-major part", "population ms_ptm", 0, 0, l.member_bytes());
            // the float part lies behind three planes of doubles: a whole number of doubles from the base
            for (int64_t R : LAUNCHES)
                if (l.offset(PTM_REPLICA_CBOX, R) != 3 * R * 6 * b * 8) fail("cbox not behind the three planes", "population ms_ptm", 3, R, l.offset(PTM_REPLICA_CBOX, R));
        }
    const int64_t partials[] = {0, 1, 2, 63, 2048, 4194304};
    for (int64_t part : partials) {
        check("eval_partial", population_eval_partial_layout(part));
        for (int64_t nv : nvarss)
            for (int rec = 0; rec < 2; ++rec) check("eval_xr", population_eval_xr_layout(rec != 0, nv));
    }
    const int64_t cams[] = {0, 1, 5, 49, 1000}, slots[] = {0, 1, 10, 20, 4000}, chunks[] = {0, 1, 63, 15626};
    for (int64_t ncb : cams)
        for (int64_t cs : slots)
            for (int64_t ps : slots)
                for (int64_t nch : chunks) check("gradient, fused", population_grad_fused_layout(ncb, cs, ps, nch));
    const int64_t nslots[] = {0, 12, 4092, 382116, 96000000}, sums[] = {0, 1, 125, 2048};
    for (int64_t ns : nslots)
        for (int64_t nb : sums) check("gradient, short and two-pass", population_grad_list_layout(ns, nb));

    // members_per_launch against each rule it replaced, over what that rule's caller can pass: counts of at least 1, budgets of
    // at least 0; bytes of at least 8 for the evaluation and the gradient, of 0 too for the two solve entries
    const int64_t counts[] = {1, 2, 3, 5, 64, 255, 256, 1000, 65534, 65535, 65536, 1000000, 2147483647ll};
    const int64_t budgets[] = {0, 1, 7, 8, 9, 503, 504, 505, 7191, 7192, 17980, 28959, 28960, 72400, 190656, 381312, 1 << 20, 1ll << 30, 1ll << 40};
    const int64_t bytes[] = {0, 1, 8, 64, 504, 7192, 28960, 1120000, 3056936, 5ll << 30};
    for (int64_t m : counts)
        for (int64_t bud : budgets)
            for (int64_t mb : bytes) {
                const int64_t R = members_per_launch(m, bud, mb);
                if (R != rule_starts(m, bud, (size_t)mb)) fail("not the multi-start entry's rule", "members", m, bud, R);
                if (R != rule_population(m, bud, mb)) fail("not the population solve's rule", "members", m, bud, R);
                if (mb >= 8 && R != rule_eval(m, bud, mb)) fail("not the evaluation's rule", "members", m, bud, R);
                if (mb >= 8 && R != rule_grad(m, bud, mb)) fail("not the gradient's rule", "members", m, bud, R);
                if (R < 1 || R > m || R > 65535) fail("outside 1 ... min(count, 65535)", "members", m, bud, R);
                if (mb > 0 && R > 1 && R * mb > bud) fail("beyond the budget", "members", m, bud, R);
                if (mb > 0 && R < m && R < 65535 && (R + 1) * mb <= bud) fail("a member more would fit", "members", m, bud, R);
            }

    for (int64_t R : LAUNCHES) {
        // multi-start: nfree ngfac plain nvars R | ms_work: member total ws gfac x | ms_dir: member total | charged | strides ws gfac x
        const struct { int64_t nf, ng; int plain; int64_t nv; } starts[] = {{45, 384, 0, 135}, {121, 360, 1, 121}, {0, 0, 0, 0}, {0, 0, 1, 0}, {9, 0, 1, 7}, {663, 382116, 0, 23769}};
        for (const auto& s : starts) {
            const ReplicaLayout w = starts_work_layout(s.nf, s.ng, s.plain != 0, s.nv), d = solve_dir_layout(s.plain != 0, s.nv);
            std::printf("starts %lld %lld %d %lld %lld", (ll)s.nf, (ll)s.ng, s.plain, (ll)s.nv, (ll)R);
            print_offsets(w, R);
            std::printf(" %lld %lld %lld\n", (ll)d.member_bytes(), (ll)d.total_bytes(R), (ll)(w.member_bytes() + d.member_bytes()));
        }
        // population solve: listed nfree ngfac tiny_records plain nvars R | ms_work: member total ws gfac rot | ms_dir: member total
        const struct { int listed; int64_t nf, ng; int rec, plain; int64_t nv; } pops[] = {
            {1, 45, 384, 1, 0, 135}, {0, 45, 384, 0, 0, 135}, {1, 45, 384, 0, 0, 135}, {0, 23328, 382116, 1, 0, 23769}, {1, 120, 360, 0, 1, 121},
            {1, 100, 7, 0, 0, 0}, {1, 0, 0, 1, 0, 9}, {0, 0, 0, 0, 0, 0}};
        for (const auto& s : pops) {
            const ReplicaLayout w = population_work_layout(s.listed != 0, s.nf, s.ng, s.rec != 0, s.nv), d = solve_dir_layout(s.plain != 0, s.nv);
            std::printf("population %d %lld %lld %d %d %lld %lld", s.listed, (ll)s.nf, (ll)s.ng, s.rec, s.plain, (ll)s.nv, (ll)R);
            print_offsets(w, R);
            std::printf(" %lld %lld\n", (ll)d.member_bytes(), (ll)d.total_bytes(R));
        }
        // point-major: blocks cptr_len R | member total rec gh bex cbox
        const struct { int64_t b, cp; } ptms[] = {{200, 5}, {7776, 123}, {2400, 40}, {1, 2}, {0, 0}, {0, 5}, {8, 0}};
        for (const auto& s : ptms) {
            std::printf("ptm %lld %lld %lld", (ll)s.b, (ll)s.cp, (ll)R);
            print_offsets(population_ptm_layout(s.b, s.cp), R);
            std::printf("\n");
        }
        // evaluation: partials nvars records R | eval_partial: member total | eval_xr: member total | charged
        const struct { int64_t part, nv; int rec; } evals[] = {{63, 23769, 1}, {63, 23769, 0}, {1, 135, 1}, {2048, 3600, 0}, {1, 0, 1}, {1, 0, 0}};
        for (const auto& s : evals) {
            const ReplicaLayout a = population_eval_partial_layout(s.part), x = population_eval_xr_layout(s.rec != 0, s.nv);
            std::printf("eval %lld %lld %d %lld %lld %lld %lld %lld %lld\n", (ll)s.part, (ll)s.nv, s.rec, (ll)R, (ll)a.member_bytes(), (ll)a.total_bytes(R),
                        (ll)x.member_bytes(), (ll)x.total_bytes(R), (ll)(a.member_bytes() + x.member_bytes()));
        }
        // gradient, fused: ncam_blocks cstage_slots pstage_slots nchunks R | member total camrec cstage pstage partial | the four strides
        const struct { int64_t ncb, cs, ps, nch; } fused[] = {{49, 10, 20, 63}, {5, 0, 0, 1}, {49, 0, 3, 125}, {0, 0, 0, 1}, {1000, 4000, 4000, 15626}};
        for (const auto& s : fused) {
            const ReplicaLayout l = population_grad_fused_layout(s.ncb, s.cs, s.ps, s.nch);
            std::printf("gradf %lld %lld %lld %lld %lld", (ll)s.ncb, (ll)s.cs, (ll)s.ps, (ll)s.nch, (ll)R);
            print_offsets(l, R);
            std::printf(" %lld %lld %lld %lld\n", l.doubles(0), l.doubles(1), l.doubles(2), l.doubles(3));
        }
        // gradient, short (partials = 1) and two-pass: nslots partials R | member total gfac partial | gfac's stride
        const struct { int64_t ns, nb; } lists[] = {{382116, 125}, {4092, 1}, {30, 1}, {0, 1}, {12, 2048}};
        for (const auto& s : lists) {
            const ReplicaLayout l = population_grad_list_layout(s.ns, s.nb);
            std::printf("gradl %lld %lld %lld", (ll)s.ns, (ll)s.nb, (ll)R);
            print_offsets(l, R);
            std::printf(" %lld\n", l.doubles(GRAD_LIST_GFAC));
        }
    }
    // the cases the three programs beside this one print (population_eval_members_test: its bytes are 8 (partials + records))
    const struct { int64_t m, bud, mb; } launches[] = {
        {5, 17980, 7192}, {5, 1, 7192}, {3, 0, 7192}, {5, 1ll << 30, 7192}, {256, 1ll << 30, 3056936}, {1000, 1ll << 30, 3056936}, {100000, 1ll << 30, 8},
        {70000, 1ll << 40, 7192}, {5, 72400, 28960}, {5, 1, 28960}, {5, 1ll << 30, 28960}, {256, 1ll << 30, 1123680}, {256, 1ll << 28, 1123680},
        {100000, 1ll << 30, 64}, {3, 0, 28960}, {7, 12345, 0}, {256, 1ll << 30, 8 * 136}, {64, 1ll << 30, 8 * 23832}, {5, 2 * 8 * 23832, 8 * 23832},
        {5, 2 * 8 * 23832 - 1, 8 * 23832}, {5, 1, 8 * 23832}, {5, 1024, 504}, {5, 1023, 504}, {1000000, 1ll << 30, 8}, {1000000, 1ll << 30, 8 * 136},
        {1, 0, 8}, {70000, 1ll << 40, 8 * 100002048ll}, {3, 1ll << 30, 8 * 2048}};
    for (const auto& s : launches)
        std::printf("members %lld %lld %lld %lld\n", (ll)s.m, (ll)s.bud, (ll)s.mb, (ll)members_per_launch(s.m, s.bud, s.mb));
    std::printf("ok\n");
    return 0;
}
