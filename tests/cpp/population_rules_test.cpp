// population_rules_test.cpp -- rdis_amd/csrc/population_rules.hpp without a device; tests/test_population_rules_cpu.py feeds it
// and holds every message as a literal.  Integers are read with INT64_MAX / INT64_MIN spelled "max" / "min".
//   range      stdin: cases "who first count n has_vid nmembers N";  prints "code message" per case ("0 -": in range)
//   many       stdin: cases "rows per_row";  prints "too_many_values too_many_rows" per case
//   permute    stdin: cases "n order[n]";  prints the refusal per case ("-": a permutation)
//   sampling   stdin: cases "N which lo[N] hi[N]" (doubles; which: 0 both arrays, 1 lo NULL, 2 hi NULL, 3 both NULL);  prints the refusal or "-"
//   novalues   prints "reader message" for the three readers
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>
#include "../../rdis_amd/csrc/population_rules.hpp"

using namespace rdis_hip;

static bool read_i64(int64_t& v) {
    char w[64];
    if (std::scanf("%63s", w) != 1) return false;
    if (!std::strcmp(w, "max")) v = std::numeric_limits<int64_t>::max();
    else if (!std::strcmp(w, "min")) v = std::numeric_limits<int64_t>::min();
    else v = std::strtoll(w, nullptr, 10);
    return true;
}
static double read_double() {
    char w[64];
    if (std::scanf("%63s", w) != 1) { std::fprintf(stderr, "a double is missing\n"); std::exit(1); }
    return std::strtod(w, nullptr);   // ("inf", "nan" too)
}
static void print_refusal(const std::string& why) { std::printf("%s\n", why.empty() ? "-" : why.c_str()); }

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "range")) {
        char who[64];
        while (std::scanf("%63s", who) == 1) {
            int64_t first, count, n, has_vid, nmembers, N;
            if (!(read_i64(first) && read_i64(count) && read_i64(n) && read_i64(has_vid) && read_i64(nmembers) && read_i64(N))) return 1;
            const PopulationRefusal r = population_range_refusal(who, first, count, n, has_vid != 0, nmembers, N);
            if ((r.code == 0) != r.message.empty()) return 2;
            std::printf("%d %s\n", r.code, r.code ? r.message.c_str() : "-");
        }
        return 0;
    }
    if (!std::strcmp(mode, "many")) {
        int64_t rows, per;
        while (read_i64(rows) && read_i64(per)) std::printf("%d %d\n", (int)too_many_values(rows, per), (int)too_many_rows(rows, per));
        return 0;
    }
    if (!std::strcmp(mode, "permute")) {
        int64_t n;
        while (read_i64(n)) {
            std::vector<int64_t> order((size_t)n);
            for (auto& s : order) if (!read_i64(s)) return 1;
            print_refusal(population_permutation_refusal(order.data(), n));
        }
        return 0;
    }
    if (!std::strcmp(mode, "sampling")) {
        int64_t N, which;
        while (read_i64(N) && read_i64(which)) {
            std::vector<double> lo((size_t)N), hi((size_t)N);
            for (auto& v : lo) v = read_double();
            for (auto& v : hi) v = read_double();
            print_refusal(population_sampling_refusal(which & 1 ? nullptr : lo.data(), which & 2 ? nullptr : hi.data(), N));
        }
        return 0;
    }
    if (!std::strcmp(mode, "novalues")) {
        for (int reader = 0; reader < POPULATION_READERS; ++reader) std::printf("%d %s\n", reader, population_no_values_refusal(reader).c_str());
        return 0;
    }
    std::fprintf(stderr, "usage: population_rules_test range | many | permute | sampling | novalues\n");
    return 1;
}
