// lm_rules_test.cpp -- rdis_amd/csrc/lm_rules.hpp without a device; tests/test_lm_rules_cpu.py feeds it and restates every rule.
//   layout     stdin: cases "N F cam[F] pt[F]";  prints "ncams factors_fit whole_points" per case
//   rows       stdin: cases "rows hist_cap mask  res[rows][12] hist[rows][hist_cap][4]" (doubles as hex floats).  mask names the
//              output pointers that are handed over: 1 fret, 2 delta, 4 info8, 8 nhist, 16 hist4.  Every destination is filled
//              with a sentinel first (-7.5; nhist -7); prints the five destinations whole, a line each ("-" for one not handed over)
//   refusals   prints "reader last_kind message" for the 6 readers x kinds 0..3 ("-": the reader may read)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>
#include "../../rdis_amd/csrc/lm_rules.hpp"

using namespace rdis_hip;

static bool read_ll(long long& v) { return std::scanf("%lld", &v) == 1; }
static double read_double() {
    char w[64];
    if (std::scanf("%63s", w) != 1) { std::fprintf(stderr, "a double is missing\n"); std::exit(1); }
    return std::strtod(w, nullptr);
}

int main(int argc, char** argv) {
    const char* mode = argc > 1 ? argv[1] : "";
    if (!std::strcmp(mode, "layout")) {
        long long N, F;
        while (read_ll(N) && read_ll(F)) {
            std::vector<int> cam((size_t)F), pt((size_t)F);
            long long v;
            for (auto& c : cam) { read_ll(v); c = (int)v; }
            for (auto& p : pt) { read_ll(v); p = (int)v; }
            const LmBlockLayout B = lm_block_layout(N, F, cam.data(), pt.data());
            std::printf("%d %d %d\n", B.ncams, (int)B.factors_fit, (int)B.whole_points);
        }
        return 0;
    }
    if (!std::strcmp(mode, "rows")) {
        long long rows, cap, mask;
        while (read_ll(rows) && read_ll(cap) && read_ll(mask)) {
            std::vector<double> res((size_t)rows * LM_BATCH_RES), hist((size_t)(rows * cap * 4));
            for (auto& v : res) v = read_double();
            for (auto& v : hist) v = read_double();
            std::vector<double> fret((size_t)rows, -7.5), delta((size_t)rows, -7.5), info8((size_t)rows * 8, -7.5), hist4((size_t)(rows * cap * 4), -7.5);
            std::vector<int64_t> nhist((size_t)rows, -7);
            lm_result_rows(rows, res.data(), hist.data(), cap, mask & 1 ? fret.data() : nullptr, mask & 2 ? delta.data() : nullptr,
                           mask & 4 ? info8.data() : nullptr, mask & 8 ? nhist.data() : nullptr, mask & 16 ? hist4.data() : nullptr);
            auto line = [](bool on, const std::vector<double>& v) {
                if (!on) { std::printf("-\n"); return; }
                for (double d : v) std::printf("%a ", d);
                std::printf("\n");
            };
            line(mask & 1, fret); line(mask & 2, delta); line(mask & 4, info8);
            if (mask & 8) { for (int64_t n : nhist) std::printf("%lld ", (long long)n); std::printf("\n"); } else std::printf("-\n");
            line(mask & 16, hist4);
            // what was not handed over was not written
            for (double d : fret) if (!(mask & 1) && d != -7.5) return 2;
            for (double d : delta) if (!(mask & 2) && d != -7.5) return 2;
            for (double d : info8) if (!(mask & 4) && d != -7.5) return 2;
            for (int64_t n : nhist) if (!(mask & 8) && n != -7) return 2;
            for (double d : hist4) if (!(mask & 16) && d != -7.5) return 2;
        }
        return 0;
    }
    if (!std::strcmp(mode, "refusals")) {
        for (int reader = 0; reader < LM_READERS; ++reader)
            for (int kind = 0; kind < 4; ++kind) {
                const char* why = lm_read_refusal(reader, kind);
                std::printf("%d %d %s\n", reader, kind, why ? why : "-");
            }
        return 0;
    }
    std::fprintf(stderr, "usage: lm_rules_test layout | rows | refusals\n");
    return 1;
}
