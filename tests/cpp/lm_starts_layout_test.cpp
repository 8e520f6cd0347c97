// lm_starts_layout_test.cpp -- the host side of a Levenberg-Marquardt plan's multi-start solve without a device:
// rdis_amd/csrc/replica_layout.hpp's lm_starts_layout and rdis_amd/csrc/lm_starts.hpp's lm_starts_tables and lm_starts_best.
//   layout   checks over a grid of arguments and start counts (exit code 1 and a line on stderr at the first that fails): `out` is
//            lm_plan_layout's three fields in their order for nstarts + 1 rows, no overlap, no gap, every part at a multiple of 8
//            bytes, the winners' row behind the nstarts rows of every field, best[ncomp] behind the rows, the total; `work` charges
//            a start its workspace slices and a row of N doubles, and members_per_launch at budgets of nothing, one start and all
//            starts.  Prints "lmstarts ncomp res hist_cap nfree ws N nstarts per | out: offsets of res hist x, the winners' offsets
//            in them, best's offset, the total | work: a start's bytes, the offsets of ws and rows, the total" for the cases
//            tests/test_lm_starts_cpu.py restates as literal arithmetic, then "ok".
//   tables   reads "N ncomp", free_ptr[ncomp + 1] and free_vid[nfree] from stdin; prints pos[N] on one line, comp_of[nfree] on the next.
//   select   reads "nstarts ncomp" and fret[nstarts][ncomp] as the doubles' bit patterns (hexadecimal, so that NaNs and the sign of
//            zero arrive as they are) from stdin; prints best[ncomp]: the kernel's scan, lm_starts_best, with the kernel's strides.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../rdis_amd/csrc/lm_starts.hpp"
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

static int layout() {
    const int64_t ncomps[] = {1, 2, 5, 30, 7776}, rd = 12, caps[] = {0, 1, 64}, wss[] = {0, 86, 5050, 1306368}, nfrees[] = {0, 3, 135, 23328};
    const int64_t Ns[] = {1, 135, 23769}, counts[] = {1, 2, 5, 64, 65535, 70000};
    for (int64_t nc : ncomps)
        for (int64_t cap : caps)
            for (int64_t ws : wss)
                for (int64_t nfr : nfrees)
                    for (int64_t N : Ns) {
                        const LmStartsLayout Y = lm_starts_layout(nc, rd, cap, nfr, ws, N);
                        const LmPlanLayout P = lm_plan_layout(nc, rd, cap, nfr, ws);
                        if (Y.out.nparts != 3 || Y.work.nparts != 2) fail("part counts", nc, cap, ws, Y.out.nparts);
                        for (int i = 0; i < 3; ++i)
                            if (Y.out.bytes[i] != P.out.bytes[i]) fail("out's fields are the plan's", nc, cap, i, Y.out.bytes[i]);
                        if (Y.work.bytes[LM_STARTS_WS] != 8 * ws || Y.work.bytes[LM_STARTS_ROWS] != 8 * N) fail("work's parts", ws, N, 0, Y.work.member_bytes());
                        const int64_t mb = Y.work.member_bytes();
                        if (mb != 8 * (ws + N)) fail("a start's budget: its slices and its row of N doubles", ws, N, 0, mb);
                        for (int64_t S : counts) {
                            const int64_t R = Y.out_rows(S);
                            if (R != S + 1 || Y.winners_row(S) != S) fail("a row more than starts, the winners' the last", S, 0, 0, R);
                            check("out", Y.out, R);
                            for (int i = 0; i < 3; ++i) {   // the winners' row of field i: behind the S rows of the field, inside it
                                const int64_t w = Y.out.offset(i, R) + Y.winners_row(S) * Y.out.bytes[i];
                                const int64_t next = i + 1 < 3 ? Y.out.offset(i + 1, R) : Y.out.total_bytes(R);
                                if (w != Y.out.offset(i, R) + S * Y.out.bytes[i] || w + Y.out.bytes[i] != next) fail("the winners' row", S, i, 0, w);
                            }
                            if (Y.best_offset(S) != Y.out.total_bytes(R) || Y.best_offset(S) % 8 != 0) fail("best follows the rows", S, nc, 0, Y.best_offset(S));
                            if (Y.best_bytes() < 4 * nc || Y.best_bytes() % 8 != 0 || Y.best_bytes() >= 4 * nc + 8) fail("best: int32, padded to 8 bytes", nc, 0, 0, Y.best_bytes());
                            if (Y.out_bytes(S) != (S + 1) * P.out.member_bytes() + Y.best_bytes()) fail("out's total", S, nc, 0, Y.out_bytes(S));
                            // budgets: nothing, below one start, one start, two, all but a byte, all, more than enough
                            const int64_t budgets[] = {0, mb - 1, mb, mb + 1, 2 * mb, S * mb - 1, S * mb, (int64_t)1 << 40};
                            for (int64_t bud : budgets) {
                                if (bud < 0) continue;
                                const int64_t per = members_per_launch(S, bud, mb);
                                if (per < 1 || per > S || per > 65535) fail("starts outside 1 ... min(count, 65535)", S, bud, mb, per);
                                if (per > 1 && per * mb > bud) fail("starts beyond the budget", S, bud, mb, per);
                                if (per < S && per < 65535 && (per + 1) * mb <= bud) fail("a start more would fit", S, bud, mb, per);
                                check("work", Y.work, per);
                            }
                            if (members_per_launch(S, 0, mb) != 1 || members_per_launch(S, mb, mb) != 1) fail("a budget of nothing or of one start: one", S, mb, 0, 0);
                            if (members_per_launch(S, S * mb, mb) != (S < 65535 ? S : 65535)) fail("a budget of all starts: all of them", S, mb, 0, 0);
                            if (S > 1 && S <= 65535 && members_per_launch(S, S * mb - 1, mb) != S - 1) fail("one byte short of all starts", S, mb, 0, 0);
                            // the row of N doubles is in the budget: with the workspace slices alone one start more would seem to fit
                            if (S > 1 && ws > 0 && members_per_launch(S, 2 * 8 * ws + 8 * N, mb) != 1) fail("the row is charged", S, ws, N, 0);
                        }
                    }
    const struct { int64_t nc, cap, nfr, ws, N, S, per; } cases[] = {{30, 64, 90, 2580, 135, 6, 6}, {5, 64, 45, 40000, 135, 64, 3}, {7776, 1, 23328, 1306368, 23769, 16, 16},
                                                                       {2, 0, 6, 86, 300, 5, 2}, {1, 8, 0, 0, 1, 1, 1}};
    for (const auto& s : cases) {
        const LmStartsLayout Y = lm_starts_layout(s.nc, rd, s.cap, s.nfr, s.ws, s.N);
        const int64_t R = Y.out_rows(s.S);
        std::printf("lmstarts %lld %lld %lld %lld %lld %lld %lld %lld", (ll)s.nc, (ll)rd, (ll)s.cap, (ll)s.nfr, (ll)s.ws, (ll)s.N, (ll)s.S, (ll)s.per);
        for (int i = 0; i < 3; ++i) std::printf(" %lld", (ll)Y.out.offset(i, R));
        for (int i = 0; i < 3; ++i) std::printf(" %lld", (ll)(Y.out.offset(i, R) + Y.winners_row(s.S) * Y.out.bytes[i]));
        std::printf(" %lld %lld %lld %lld %lld %lld\n", (ll)Y.best_offset(s.S), (ll)Y.out_bytes(s.S), (ll)Y.work.member_bytes(), (ll)Y.work.offset(LM_STARTS_WS, s.per),
                    (ll)Y.work.offset(LM_STARTS_ROWS, s.per), (ll)Y.work.total_bytes(s.per));
    }
    std::printf("ok\n");
    return 0;
}

static int tables() {
    ll N, nc;
    if (std::scanf("%lld %lld", &N, &nc) != 2) return 2;
    std::vector<int64_t> fp((size_t)nc + 1);
    for (auto& v : fp) { ll t; if (std::scanf("%lld", &t) != 1) return 2; v = t; }
    std::vector<int64_t> fv((size_t)fp[(size_t)nc]);
    for (auto& v : fv) { ll t; if (std::scanf("%lld", &t) != 1) return 2; v = t; }
    std::vector<int32_t> pos, comp_of;
    lm_starts_tables(N, nc, fp.data(), fv.data(), pos, comp_of);
    if ((ll)pos.size() != N || comp_of.size() != fv.size()) return 1;
    for (int32_t v : pos) std::printf("%d ", (int)v);
    std::printf("\n");
    for (int32_t v : comp_of) std::printf("%d ", (int)v);
    std::printf("\n");
    return 0;
}

static int select() {
    ll S, nc;
    if (std::scanf("%lld %lld", &S, &nc) != 2 || S < 1) return 2;
    const ll rd = 12;                                   // a result row: fret is its first double, as on the device
    std::vector<double> res((size_t)(S * nc * rd), 0.0);
    for (ll s = 0; s < S; ++s)
        for (ll c = 0; c < nc; ++c) {
            unsigned long long bits;
            if (std::scanf("%llx", &bits) != 1) return 2;
            std::memcpy(&res[(size_t)((s * nc + c) * rd)], &bits, 8);
        }
    for (ll c = 0; c < nc; ++c) std::printf("%lld ", lm_starts_best(S, res.data() + c * rd, nc * rd));
    std::printf("\n");
    return 0;
}

int main(int argc, char** argv) {
    if (argc == 2 && !std::strcmp(argv[1], "layout")) return layout();
    if (argc == 2 && !std::strcmp(argv[1], "tables")) return tables();
    if (argc == 2 && !std::strcmp(argv[1], "select")) return select();
    std::fprintf(stderr, "usage: lm_starts_layout_test layout | tables | select\n");
    return 2;
}
