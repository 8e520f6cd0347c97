// population_state.hpp -- struct rdis_hip_population, for the translation units of the C ABI that use it: population_entries.hip,
// which holds the population's entries, and rdis_hip.hip and lm_api.hip, whose plans solve on a population's rows.
#pragma once
#include "abi_state.hpp"

struct rdis_hip_population {
    rdis_hip_problem* prob = nullptr;
    int64_t nmembers = 0;
    DevBuf X;                  // [nmembers][N]
    DevBuf f;                  // [nmembers] values of the last population_eval
    DevBuf tmp_val, tmp_out;   // staging of set_x / get_x
    // the batched evaluation (population_eval_enqueue): scratch of the population's own, per member of a launch
    DevBuf eval_partial;       // [R][chunks or blocks] the members' partial sums
    DevBuf eval_xr;            // [R][N] the members' rotation records (the records branch only)
    DevBuf best;               // one MemberValue: the argmin of f (population_argmin_kernel)
    int64_t eval_workspace_bytes = (int64_t)1 << 30;   // option "eval_workspace_bytes": bounds eval_partial + eval_xr
    int eval_batched = 1;      // option "eval_batched": 0 = member by member through the problem's scratch (enqueue_eval)
    int64_t eval_per_launch = 0, eval_launches = 0;    // of the last evaluation: members of a launch, kernels launched
    bool eval_valid = false;   // f holds the values of X as it is (set_x and plan_solve_population write X: stale)
    bool best_current = false; // best holds the argmin of f
    DevBuf slo, shi;           // [N] each: the sampling intervals of population_sample (population_set_sampling) ...
    bool sampling_set = false; // ... false: the problem's domains
    DevBuf X2, f2, order;      // population_sort: the other buffer of X's size (X and X2 swap roles), the permuted values, order[nmembers] (int64)
    // value + gradient of a member range (population_grad_enqueue): results and scratch of the population's own
    DevBuf grad_f, grad_g;     // [rows], [rows][N]: what the last gradient call handed out
    DevBuf grad_gmax;          // [rows]: population_grad_max of those rows
    DevBuf grad_ws;            // the replicas of a launch's members (population_grid.hpp: grad_member_bytes each)
    DevBuf grad_v2s_ptr, grad_v2s_idx;   // the gather lists of the call's explicit list (short and two-pass branch)
    int64_t grad_workspace_bytes = (int64_t)1 << 30;   // option "grad_workspace_bytes": bounds grad_ws
    int64_t grad_rows = -1;    // rows of the last gradient call; -1: none yet
    int64_t grad_per_launch = 0, grad_launches = 0;    // of the last gradient call: members of a launch, kernels launched
    int grad_branch = 0;       // ... and its form (GradBranch)
    double* row(int64_t s) const { return X.as<double>() + (size_t)s * (size_t)prob->N; }
    void x_written() { eval_valid = false; best_current = false; }   // X is written: the values of the last evaluation are stale
};

namespace rdis_hip {
// `bytes` of device memory into the caller's array, waited for: what every entry that hands values to the host ends in
inline int read_back(rdis_hip_ctx* c, void* dst, const void* src, size_t bytes) {
    HIPCHK(c, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return 0;
}
}  // namespace rdis_hip
