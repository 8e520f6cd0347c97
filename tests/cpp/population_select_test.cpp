// population_select_test.cpp -- rdis_amd/csrc/population_select.hpp without a device: the draw of population_sample and the
// order of population_sort.  Prints "draw seed stream member var slo shi lo hi value" (doubles as their 64 bits in hex) over a
// grid of arguments -- tests/test_population_select_cpu.py compares every value with oracle.levels.splitmix_restart_value, bit
// for bit --, checks that better() is a strict total order over a set with NaNs, zeros of both signs, infinities, equal values
// and distinct indices (exit code 1 and a line on stderr at the first property that fails), and prints, per set of values,
// "set n", "f <bits> ..." and "order ..." -- the rank by counting restated with rank_of(), which the Python side compares with
// sorted() under the rule restated.  Then "ok".
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "../../rdis_amd/csrc/population_select.hpp"

using rdis_hip::better;
using rdis_hip::rank_of;
using rdis_hip::sample_member_key;
using rdis_hip::sample_value;

static unsigned long long bits(double d) { unsigned long long b; std::memcpy(&b, &d, 8); return b; }
static double from_bits(unsigned long long b) { double d; std::memcpy(&d, &b, 8); return d; }
static void die(const char* what, long long a, long long b, long long c) {
    std::fprintf(stderr, "%s: %lld %lld %lld\n", what, a, b, c);
    std::exit(1);
}

static void order_of(const std::vector<double>& f) {
    const long long n = (long long)f.size();
    std::vector<long long> order((size_t)n, -1);
    for (long long s = 0; s < n; ++s) {
        const long long r = rank_of(n, f.data(), s);
        if (r < 0 || r >= n) die("rank out of range", s, r, n);
        if (order[(size_t)r] != -1) die("two members of one rank", s, order[(size_t)r], r);
        order[(size_t)r] = s;
    }
    std::printf("set %lld\nf", n);
    for (double v : f) std::printf(" %016llx", bits(v));
    std::printf("\norder");
    for (long long s : order) std::printf(" %lld", s);
    std::printf("\n");
}

int main() {
    const double pi = 3.14159265358979323846, inf = std::numeric_limits<double>::infinity();
    // ---- the draw ----
    const unsigned long long seeds[] = {0ull, 0x5D15ull, 0x9E3779B97F4A7C15ull, ~0ull};
    const long long streams[] = {0, 3, 2147483646ll};
    const long long members[] = {0, 1, 7, 999, 2147483646ll};
    const long long vars[] = {0, 5, 134, 23768, 2147483646ll};
    const struct { double slo, shi, lo, hi; } iv[] = {
        {-pi, pi, -1e30, 1e30},                      // rotations
        {-1.3862e2 - 100.0, -1.3862e2 + 100.0, -inf, inf},   // init +- 100, an unbounded domain
        {4.2e-8 - 1e-6, 4.2e-8 + 1e-6, -1.0, 1.0},   // init +- 1e-6
        {2.5, 2.5, -10.0, 10.0},                     // zero width
        {-7.0, -7.0, -1.0, 1.0},                     // zero width outside the domain: the bound
        {-100.0, 100.0, -1.0, 1.0},                  // wider than the domain on both sides
        {-100.0, 0.5, -1.0, 1.0},                    // ... below
        {-0.5, 100.0, -1.0, 1.0},                    // ... above
        {0.0, 1.0, 0.0, 1.0},
    };
    long long below = 0, above = 0, inside = 0;
    for (unsigned long long seed : seeds)
        for (long long stream : streams)
            for (long long m : members) {
                const unsigned long long key = sample_member_key(seed, stream, m);
                for (long long v : vars)
                    for (const auto& d : iv) {
                        const double val = sample_value(key, v, d.slo, d.shi, d.lo, d.hi);
                        if (!(d.lo <= val && val <= d.hi)) die("a draw outside the domain", stream, m, v);
                        if (d.slo == d.shi && d.lo <= d.slo && d.slo <= d.hi && bits(val) != bits(d.slo)) die("a zero-width interval off its bound", stream, m, v);
                        if (d.slo < d.lo || d.shi > d.hi) { below += val == d.lo; above += val == d.hi; inside += val != d.lo && val != d.hi; }
                        std::printf("draw %llu %lld %lld %lld %016llx %016llx %016llx %016llx %016llx\n", seed, stream, m, v, bits(d.slo), bits(d.shi),
                                    bits(d.lo), bits(d.hi), bits(val));
                    }
            }
    if (below == 0 || above == 0 || inside == 0) die("the intervals wider than the domain never clamp on one side", below, above, inside);

    // ---- better(): a strict total order on (value, index), indices distinct ----
    const double nan1 = std::nan(""), nan2 = from_bits(0xfff8000000000001ull);
    const std::vector<double> vals = {nan1, 1.0, -0.0, 0.0, inf, -inf, 1.0, nan2, -1.0, 5e-324, -5e-324, 0.0, -0.0, 1.7976931348623157e308, 1.0, nan1, -inf, inf};
    const long long n = (long long)vals.size();
    for (long long a = 0; a < n; ++a) {
        if (better(vals[(size_t)a], a, vals[(size_t)a], a)) die("not irreflexive", a, a, 0);
        for (long long b = 0; b < n; ++b) {
            if (a == b) continue;
            const bool ab = better(vals[(size_t)a], a, vals[(size_t)b], b), ba = better(vals[(size_t)b], b, vals[(size_t)a], a);
            if (ab == ba) die("not total / not asymmetric", a, b, ab);
            for (long long c = 0; c < n; ++c) {
                if (c == a || c == b) continue;
                if (ab && better(vals[(size_t)b], b, vals[(size_t)c], c) && !better(vals[(size_t)a], a, vals[(size_t)c], c)) die("not transitive", a, b, c);
            }
        }
    }
    // the rule in words: a number before a NaN; the lower number; a tie (the zeros of both signs are one) and two NaNs by index
    if (!better(1.0, 9, nan1, 0) || better(nan1, 0, 1.0, 9)) die("a NaN before a number", 0, 0, 0);
    if (!better(-0.0, 2, 0.0, 3) || !better(0.0, 2, -0.0, 3) || better(-0.0, 3, 0.0, 2)) die("the zeros are not a tie by index", 0, 0, 0);
    if (!better(nan2, 1, nan1, 2) || better(nan1, 2, nan2, 1)) die("two NaNs not by index", 0, 0, 0);
    if (!better(-inf, 5, -1.0, 0) || !better(1.0, 5, inf, 0)) die("the infinities", 0, 0, 0);

    // ---- rank by counting is a permutation (order_of checks that); the Python side compares it with sorted() ----
    order_of(vals);
    order_of({nan1, nan1, nan2});
    order_of({0.0, 0.0, 0.0, 0.0});
    order_of({3.0});
    std::vector<double> many;   // more than two tiles of 256, many equal values, NaNs at both ends
    unsigned long long z = 0x5D15;
    for (int i = 0; i < 700; ++i) {
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        many.push_back(i == 0 || i == 699 ? nan1 : (double)((z >> 33) % 97) - 48.0);
    }
    order_of(many);
    std::printf("ok\n");
    return 0;
}
