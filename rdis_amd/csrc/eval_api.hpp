// eval_api.hpp -- what population_entries.hip needs of rdis_hip.hip's problem and evaluation block, declared once.  All nine are
// defined in rdis_hip.hip, beside the single-x entries they serve (rdis_hip_set_x, rdis_hip_eval, rdis_hip_eval_grad), so a
// population's evaluation takes the branch, the chunk size and the tables of the single-x one.
#pragma once
#include "abi_state.hpp"

namespace rdis_hip {

// The two on rdis_hip.hip's own timed paths stay in its anonymous namespace (stage_ids, enqueue_eval) and are reached through
// one-line forwarders, as ensure_problem_scratch is through problem_scratch:
// an int64 id list staged as int32 on the device, in the problem's tmp_idx (nullptr stays nullptr); ids outside [0, limit) are refused
int problem_stage_ids(rdis_hip_problem* p, int64_t n, const int64_t* ids, int64_t limit, const int** dev);
// the value of the listed factors (dfac on the device, null: all) at x, enqueued; one double at out_dev
int problem_enqueue_eval(rdis_hip_problem* p, double* x, int64_t nf, const int* dfac, double* out_dev);

// nf and fac name a factor list (fac null: all factors)
int check_list(rdis_hip_problem* p, int64_t nf, const int64_t* fac);
// a gradient over a list that holds an exponential factor is refused (`who` names the entry)
int refuse_exponential(rdis_hip_problem* p, int64_t nf, const int64_t* fac, const char* who);
// bundle adjustment with camera blocks: the chunked evaluation and the fused gradient
bool fused_path(const rdis_hip_problem* p);
// the form a list's value + gradient takes (population_grid.hpp: GradBranch)
int grad_branch_of(const rdis_hip_problem* p, int64_t nf, const int64_t* fac);
// the fused pass's tables of a list: found among the problem's or built
int grad_plan_for(rdis_hip_problem* p, int64_t nf, const int64_t* fac, GradPlan** out);
// for every variable the gradient slots that feed it, in factor-list order: of all factors (on the device, kept by the problem), of a list
int all_factors_v2s(rdis_hip_problem* p, const int** dptr, const int** didx);
void build_v2s(const rdis_hip_problem* p, int64_t nf, const int64_t* fac, ivec& ptr, ivec& idx);

}  // namespace rdis_hip
