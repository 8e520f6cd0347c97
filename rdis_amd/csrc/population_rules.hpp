// population_rules.hpp -- the rules the population entries of the C ABI (population_entries.hip) share, each written once as a
// pure host function: a member and value range, "too many", a permutation, the sampling intervals, and what a reader of the
// values is told while the population has none.  No HIP call and nothing of HIP in this header
// (tests/cpp/population_rules_test.cpp runs every rule without a device).
#pragma once
#include <cmath>
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/rdis_hip.h"   // RDIS_HIP_EINVAL, RDIS_HIP_ERANGE

namespace rdis_hip {

// code 0: nothing to refuse; otherwise the entry's return code and the context's message
struct PopulationRefusal {
    int code;
    std::string message;
};

// ---- "too many": rows x per_row values are indexed in doubles' exact integers, rows by 32-bit grids and counters
inline bool too_many_values(int64_t rows, int64_t per_row) { return (double)rows * (double)per_row >= 9.0e15; }
inline bool too_many_rows(int64_t rows, int64_t per_row) { return rows >= (1ll << 31) || too_many_values(rows, per_row); }

// ---- members first .. first + count - 1 of nmembers, n values each (has_vid: at listed variables; otherwise variables
// 0 .. n - 1 of N), for the entry `who`.  first == nmembers with count == 0 is in range; nothing here overflows.
inline PopulationRefusal population_range_refusal(const char* who, int64_t first, int64_t count, int64_t n, bool has_vid, int64_t nmembers, int64_t N) {
    const std::string w(who);
    if (first < 0 || count < 0 || first > nmembers || count > nmembers - first) return {RDIS_HIP_EINVAL, w + ": members out of range"};
    if (!has_vid && n > N) return {RDIS_HIP_EINVAL, w + ": n > nvars"};
    if (too_many_values(count, n)) return {RDIS_HIP_ERANGE, w + ": too many values"};
    return {0, std::string()};
}

// ---- order[0 .. n) is a permutation of 0 .. n - 1, nothing less (order[r]: the row that becomes row r).  Empty: it is;
// otherwise the first entry that is out of range or names a member a second time
inline std::string population_permutation_refusal(const int64_t* order, int64_t n) {
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int64_t r = 0; r < n; ++r) {
        const int64_t s = order[r];
        if (s < 0 || s >= n)
            return "population_permute: order[" + std::to_string(r) + "] = " + std::to_string(s) + " is out of range (the population has " +
                   std::to_string(n) + " members)";
        if (seen[(size_t)s])
            return "population_permute: member " + std::to_string(s) + " is named twice (order[" + std::to_string(r) + "]): not a permutation";
        seen[(size_t)s] = 1;
    }
    return std::string();
}

// ---- the sampling intervals lo[N], hi[N] (both null: the problem's domains again, nothing to refuse)
inline std::string population_sampling_refusal(const double* lo, const double* hi, int64_t N) {
    if (!lo && !hi) return std::string();
    if (!lo || !hi) return "population_set_sampling: lo and hi are given together (both NULL: the problem's domains)";
    for (int64_t v = 0; v < N; ++v)
        if (!std::isfinite(lo[v]) || !std::isfinite(hi[v]) || lo[v] > hi[v])
            return "population_set_sampling: variable " + std::to_string(v) + ": the sampling interval must be finite with lo <= hi";
    return std::string();
}

// ---- what a reader of f is told while f does not hold the values of X as it is.  population_sort names population_sample
// among the writers, the two readers of the best member (which are older than it) do not.
enum PopulationReader { POPULATION_READ_BEST = 0, POPULATION_READ_ASSIGN_BEST, POPULATION_READ_SORT, POPULATION_READERS };
inline std::string population_no_values_refusal(int reader) {
    static const char* const who[POPULATION_READERS] = {"population_best", "population_assign_best", "population_sort"};
    return std::string(who[reader]) + ": the population has no current values (evaluate first: rdis_hip_population_eval or _eval_device after the last " +
           (reader == POPULATION_READ_SORT ? "population_set_x / population_sample / plan_solve_population)" : "population_set_x / plan_solve_population)");
}

// ---- rdis_hip_plan_solve_population_cooperative (`who`), before any row is written: what it refuses beyond the refusals it
// shares with rdis_hip_plan_solve_population.  The pipelined layout's lane tables are built for another lane layout than the
// population kernel's (solver_coop_population.hpp runs the plain one); the grid solver has no population entry.
inline std::string population_coop_pipelined_refusal(const char* who) {
    return std::string(who) + ": cooperative components are solved on a population in the plain cooperative layout, and this plan's ordinary solve "
                              "runs them in the pipelined layout (other lane tables; the same bits): set the plan option coop_pipeline = 0";
}
inline std::string population_coop_grid_refusal(const char* who, int64_t components) {
    return std::string(who) + ": " + std::to_string(components) + " component(s) of the plan run on the grid solver, which has no population entry "
                              "(too large for a cooperative group of resident workgroups)";
}
// a cooperative launch of the plan (packed under the ordinary kernel's residency) has more workgroups a member than the
// population kernel can have resident at all: not one member fits a launch
inline std::string population_coop_residency_refusal(const char* who, int64_t launch_workgroups, int64_t cap_workgroups) {
    return std::string(who) + ": a cooperative launch of the plan has " + std::to_string(launch_workgroups) + " workgroups a member, and the population "
                              "kernel can have " + std::to_string(cap_workgroups) + " resident: not one member fits a launch (set the plan option "
                              "coop_workgroups to at most that)";
}
// ... and what rdis_hip_plan_solve_population and _range add to their refusal of a plan with cooperative components
inline std::string population_coop_hint() {
    return " (cooperative components are solved on a population by rdis_hip_plan_solve_population_cooperative, a group per member: "
           "solver_coop_population.hpp)";
}

}  // namespace rdis_hip
