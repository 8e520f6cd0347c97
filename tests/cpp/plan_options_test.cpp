// plan_options_test.cpp -- rdis_amd/csrc/plan_options.hpp without a device (tests/test_plan_options_cpu.py).  Reads commands
// from standard input and answers each with one line of JSON:
//   names                 the table's option names, in order
//   defaults              every field of a default PlanOptions (by this program's own list of the fields, not the table's)
//   set NAME VALUE        what plan_option_set does to a default PlanOptions: unknown / refused with the message, or the
//                         effects and every field that differs from its default afterwards
// Its own checks: the table names no option twice, every row has exactly one member, and the row handed back is the option's.
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <set>
#include <sstream>
#include <string>

#include "../../rdis_amd/csrc/plan_options.hpp"

using namespace rdis_hip;

#define PLAN_OPTION_FIELDS(X)                                                                                                       \
    X(block_threads) X(coop_min_factors) X(quad_min_components) X(coop_group_min_factors) X(tiny_max_blocks) X(overlap_batch)        \
    X(row_min_components) X(camera_records) X(quad_max_vars) X(coop_max_components) X(coop_workgroups) X(coop_threads)               \
    X(coop_speculate) X(coop_pipeline) X(lds_resident) X(ptm_stream) X(ptm_group) X(ptm_round_slots) X(ptm_threads)                  \
    X(ptm_local_cameras) X(emulate_stale) X(factor_rounding) X(lds_camera_sums) X(lds_matrix) X(lds_rot) X(lds_threads)              \
    X(force_stream) X(coop_poll_delay) X(coop_poll_inflight) X(coop_poll_stagger) X(starts_workspace_bytes)                          \
    X(population_point_major) X(population_plain) X(population_tiny) X(tiny_population_fill) X(trace_records) X(dump_iters)

// {"field": value, ...} of the fields where `o` differs from `base` (base null: every field)
static std::string fields_json(const PlanOptions& o, const PlanOptions* base) {
    std::ostringstream s;
    const char* sep = "";
    s << "{";
#define X(f) if (!base || o.f != base->f) { s << sep << "\"" #f "\": " << (long long)o.f; sep = ", "; }
    PLAN_OPTION_FIELDS(X)
#undef X
    s << "}";
    return s.str();
}

int main() {
    size_t nrows = 0;
    const PlanOptionRow* rows = plan_option_table(&nrows);
    std::set<std::string> seen;
    for (size_t i = 0; i < nrows; ++i) {
        if ((rows[i].i32 != nullptr) == (rows[i].i64 != nullptr)) { std::printf("row %s: one member, not two or none\n", rows[i].name); return 1; }
        if (!seen.insert(rows[i].name).second) { std::printf("row %s twice\n", rows[i].name); return 1; }
    }
    const PlanOptions defaults;
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd, name;
        long long value = 0;
        in >> cmd >> name >> value;
        if (cmd == "names") {
            std::printf("[");
            for (size_t i = 0; i < nrows; ++i) std::printf("%s\"%s\"", i ? ", " : "", rows[i].name);
            std::printf("]\n");
        } else if (cmd == "defaults") {
            std::printf("%s\n", fields_json(defaults, nullptr).c_str());
        } else if (cmd == "set") {
            PlanOptions o;
            std::string message = "(none)";
            const PlanOptionRow* row = rows;
            const int e = plan_option_set(o, name.c_str(), value, &message, &row);
            if ((row == nullptr) != (e == PLAN_OPTION_UNKNOWN) || (row && name != row->name)) { std::printf("set %s: the row handed back is not the option's\n", name.c_str()); return 1; }
            if (e == PLAN_OPTION_UNKNOWN || e == PLAN_OPTION_REFUSED)
                std::printf("{\"result\": \"%s\", \"message\": \"%s\", \"changed\": %s}\n", e == PLAN_OPTION_UNKNOWN ? "unknown" : "refused", message.c_str(),
                            fields_json(o, &defaults).c_str());
            else {
                std::string effects;
                auto add = [&](int bit, const char* what) { if (e & bit) effects += std::string(effects.empty() ? "" : ", ") + "\"" + what + "\""; };
                add(PLAN_OPTION_ROUNDS, "rounds"); add(PLAN_OPTION_LOCAL, "local"); add(PLAN_OPTION_WORKSPACE, "workspace");
                add(PLAN_OPTION_TRACE, "trace"); add(PLAN_OPTION_DUMP, "dump");
                const int known = PLAN_OPTION_DIRTY | PLAN_OPTION_ROUNDS | PLAN_OPTION_LOCAL | PLAN_OPTION_WORKSPACE | PLAN_OPTION_TRACE | PLAN_OPTION_DUMP;
                if (e < 0 || (e & ~known)) { std::printf("set %s: effect %d\n", name.c_str(), e); return 1; }
                std::printf("{\"result\": \"stored\", \"message\": \"%s\", \"dirty\": %s, \"effects\": [%s], \"changed\": %s}\n", message.c_str(),
                            (e & PLAN_OPTION_DIRTY) ? "true" : "false", effects.c_str(), fields_json(o, &defaults).c_str());
            }
        } else {
            std::printf("unknown command %s\n", cmd.c_str());
            return 1;
        }
    }
    std::printf("\"ok\"\n");
    return 0;
}
