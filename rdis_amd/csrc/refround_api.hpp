// refround_api.hpp -- the solvers that BASELINE's configs 3 - 5 reach (the cooperative ones for ladybug as one component,
// the LDS-resident batch solver for ladybug 5 / 30 and the synthetic 3 x 40 components) a second time, with the factor
// arithmetic rounded like the reference's build: every product rounded before it is added, no fused multiply-add (g++ -O2 on
// x86-64 emits none; BundleAdjustmentFactor.cpp:160-185, 266-335, 351-554).  Plan option "factor_rounding" = 1 selects them.
// Why it exists: 25 unconverged CG iterations are a chaotic map of the start, and the DISTRIBUTION of end values over
// one-ulp starts depends on the evaluator's rounding -- the oracle compiled with contraction parts from itself with KS 0.21
// (DESIGN.md section 6); with this option the device's population is compared with the reference-faithful oracle's on equal terms.
// The kernels are the same headers compiled in a namespace of their own with -DRDIS_FACTORS_NO_CONTRACT (refround_kernels.hip).
// Both instantiations take the same views and groups (namespace rdis_views, device_views.hpp), so a solver's launch has one
// signature whatever its rounding: SolverSet names the launches of one rounding, and the host picks a set, not a function.
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "device_views.hpp"
#include "starts_api.hpp"   // StartsView, CoopReplicas

namespace rdis_views {

struct SolverSet {
    // solver_pipe.hpp / solver_coop.hpp: launch_pipe, launch_coop and the resident workgroups a launch of theirs may have
    int (*launch_pipe)(hipStream_t stream, int kind, const ProblemView& P, const PlanView& V, const CoopGroup& first, const CoopGroup* groups,
                       const int* wg_group, int ngroups, int total_wg, int maxiters, double ftol);
    int (*launch_coop)(hipStream_t stream, int kind, const ProblemView& P, const PlanView& V, const CoopGroup& first, const CoopGroup* groups,
                       const int* wg_group, int ngroups, int total_wg, int threads, int maxiters, double ftol);
    int (*pipe_max_workgroups)(int num_cus);
    int (*coop_max_workgroups)(int threads, int num_cus);
    // solver_lds.hpp: launch_lds
    hipError_t (*launch_lds)(int rot, int stale, int threads, int grid, size_t dyn, hipStream_t stream, const ProblemView& P, const PlanView& V,
                             int maxiters, double ftol, int ns_cap, int ncb_cap, int chunk_cap);
    // solver_coop_population.hpp: launch_coop_population and the resident workgroups a launch of it may have, over all its members
    int (*launch_coop_population)(hipStream_t stream, int kind, const ProblemView& P, const PlanView& V, const StartsView& S, const CoopReplicas& RC,
                                  double* X, const CoopGroup* groups, const int* wg_group, int ngroups, int total_wg, int members_of_launch,
                                  int threads, int maxiters, double ftol);
    int (*coop_population_max_workgroups)(int threads, int num_cus);
};

}  // namespace rdis_views

namespace rdis_hip {

const rdis_views::SolverSet& refround_solvers();   // (the default rounding's set is rdis_hip.hip's own)
// per-factor values / twelve partials of bundle-adjustment factors in this rounding (rdis_hip_set_factor_rounding(problem, 1))
hipError_t refround_eval_each(int grid, hipStream_t stream, const rdis_views::ProblemView& P, int nf, const int* fac, double* out);
hipError_t refround_grad_each(int grid, hipStream_t stream, const rdis_views::ProblemView& P, int nf, const int* fac, double* out12);

}  // namespace rdis_hip
