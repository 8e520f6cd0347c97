// lm_rules.hpp -- the rules the Levenberg-Marquardt entries of the C ABI (lm_api.hip) share, each written once as a pure host
// function: the block layout rdis_hip_lm_optimize requires, a result row as the caller's fields, which reader the last solve
// allows, a population's member range, levmar's constants.  No HIP call, nothing of HIP in what a host compiler sees of this
// header (tests/cpp/lm_rules_test.cpp runs the first three without a device).
#pragma once
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>

#include "lm_batch.hpp"   // LM_BATCH_RES, LM_BATCH_RES_NHIST; LmBatchOptions where the HIP compiler reads this

namespace rdis_hip {

// ---- block layout: cameras occupy the ids below the first point block (BundleAdjustmentFunction.h:88-96), blocks of 9 then
// blocks of 3.  factors_fit: every factor's camera block starts on the 9-grid below 9 ncams and its point block on the 3-grid
// from there (no factor: nothing to refuse) -- what rdis_hip_lm_optimize requires.  whole_points: the ids from 9 ncams to N are
// whole blocks of 3 -- what lm_batch_prepare needs besides, to give a variable no factor reads the layout's block.
struct LmBlockLayout {
    int ncams;
    bool factors_fit, whole_points;
};
inline LmBlockLayout lm_block_layout(int64_t N, int64_t F, const int* h_cam, const int* h_pt) {
    int minpt = INT32_MAX;
    for (int64_t f = 0; f < F; ++f) minpt = std::min(minpt, h_pt[(size_t)f]);
    const int ncams = F > 0 ? minpt / 9 : 0;
    bool fit = true;
    for (int64_t f = 0; f < F && fit; ++f)
        fit = h_cam[(size_t)f] % 9 == 0 && h_cam[(size_t)f] < 9 * ncams && (h_pt[(size_t)f] - 9 * ncams) % 3 == 0;
    return LmBlockLayout{ncams, fit, (N - 9ll * ncams) % 3 == 0};
}

// ---- result rows: `rows` rows of LM_BATCH_RES doubles (lm_batch.hpp: fret, finit, then info8's eight, then the history's
// record count) and their history block [rows][hist_cap][4] as the caller's fields, each optional.  Entry cc of a field is row
// cc's.  Of a row's history the first min(records, hist_cap) are copied; what lies beyond them in hist4 is left as it was.
inline void lm_result_rows(int64_t rows, const double* res, const double* hist, int64_t hist_cap, double* fret, double* delta, double* info8,
                           int64_t* nhist, double* hist4) {
    for (size_t cc = 0; cc < (size_t)rows; ++cc) {
        const double* r = res + cc * LM_BATCH_RES;
        if (fret) fret[cc] = r[0];
        if (delta) delta[cc] = r[0] - r[1];
        if (info8) std::memcpy(info8 + 8 * cc, r + 2, 8 * sizeof(double));
        if (nhist) nhist[cc] = (int64_t)r[LM_BATCH_RES_NHIST];
        if (hist4 && hist_cap > 0) {
            const int64_t n = std::min<int64_t>((int64_t)r[LM_BATCH_RES_NHIST], hist_cap);
            std::memcpy(hist4 + cc * (size_t)hist_cap * 4, hist + cc * (size_t)hist_cap * 4, (size_t)n * 32);
        }
    }
}

// ---- last-solve refusals: a plan's last solve is of kind 0 (none yet), 1 (rdis_hip_lm_plan_solve), 2 (a population solve) or
// 3 (a multi-start solve); each of the six entries that read its outputs takes some kinds and refuses the others with a
// message for "nothing yet" and one for the wrong kind.
enum LmReader { LM_READ_FETCH = 0, LM_READ_FETCH_POPULATION, LM_READ_FETCH_STARTS, LM_READ_OBJECTIVE_DEVICE, LM_READ_SUMMARY_DEVICE,
                LM_READ_SUMMARY_POPULATION_DEVICE, LM_READERS };
// nullptr: the reader may read; otherwise its refusal
inline const char* lm_read_refusal(int reader, int last_kind) {
    static const struct { unsigned kinds; const char *nothing, *wrong; } rule[LM_READERS] = {
        {1u << 1 | 1u << 3, "lm_plan_fetch: nothing was solved yet",
         "lm_plan_fetch: the last solve was a population solve (rdis_hip_lm_plan_fetch_population)"},
        {1u << 2, "lm_plan_fetch_population: nothing was solved yet",
         "lm_plan_fetch_population: the last solve was not a population solve (rdis_hip_lm_plan_fetch)"},
        {1u << 3, "lm_plan_fetch_starts: nothing was solved yet",
         "lm_plan_fetch_starts: the last solve was not a multi-start solve (rdis_hip_lm_plan_fetch, rdis_hip_lm_plan_fetch_population)"},
        {1u << 1 | 1u << 3, "lm_plan_objective_device: nothing was solved yet",
         "lm_plan_objective_device: the last solve was a population solve (its members have no common objective)"},
        {1u << 1 | 1u << 3, "lm_plan_summary: nothing was solved yet",
         "lm_plan_summary: the last solve was a population solve (its members have no common summary)"},
        {1u << 2, "lm_plan_summary_population: nothing was solved yet",
         "lm_plan_summary_population: the last solve was not a population solve (rdis_hip_lm_plan_summary)"},
    };
    if (rule[reader].kinds >> last_kind & 1u) return nullptr;
    return last_kind == 0 ? rule[reader].nothing : rule[reader].wrong;
}

// ---- a population's member range for the plan's entry `who`: the population is the plan's problem's, and members
// first .. first + count - 1 exist.  Empty: in range; otherwise the refusal.
inline std::string lm_member_range_refusal(const char* who, bool same_problem, int64_t first, int64_t count, int64_t nmembers) {
    if (!same_problem) return std::string(who) + ": the population belongs to another problem than the plan's";
    if (count < 1 || first < 0 || first > nmembers || count > nmembers - first)
        return std::string(who) + ": members out of range (count >= 1, first + count <= nmembers)";
    return std::string();
}

// ---- levmar's opts[0..2] as the reference sets them (tau, eps1, eps2; opts[3] is the caller's ftol)
constexpr double LM_TAU = 1e-3, LM_EPS1 = 1e-15, LM_EPS2 = 1e-15;
#if defined(__HIPCC__)
inline LmBatchOptions lm_batch_options(int maxiters, int R, double ftol) { return LmBatchOptions{maxiters, R, LM_TAU, LM_EPS1, LM_EPS2, ftol}; }
#endif

}  // namespace rdis_hip
