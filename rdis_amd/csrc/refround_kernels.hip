// refround_kernels.hip -- see refround_api.hpp: solver_pipe.hpp / solver_coop.hpp / solver_lds.hpp compiled once more, in
// namespace rdis_hip_refround, with the factor arithmetic's contraction off.  The rename leaves namespace rdis_views alone
// (device_views.hpp), so the headers' own launches take the host's views and groups and stand in refround_solvers() unwrapped.
#define RDIS_FACTORS_NO_CONTRACT 1
#define RDIS_REFERENCE_SLOPE 1      // solver_lds.hpp: a trial's slope as gradient times direction, like Df1dim::df
#define rdis_hip rdis_hip_refround
#include "solver_lds.hpp"
#include "solver_pipe.hpp"
#include "solver_coop_population.hpp"
#undef rdis_hip
#include "refround_api.hpp"

namespace rdis_hip {
namespace rr = ::rdis_hip_refround;

// (the views and groups are namespace rdis_views' own in either instantiation: the launches go into the set as they are)
const rdis_views::SolverSet& refround_solvers() {
    static const rdis_views::SolverSet set = {rr::launch_pipe, rr::launch_coop, rr::pipe_max_workgroups, rr::coop_max_workgroups, rr::launch_lds,
                                              rr::launch_coop_population, rr::coop_population_max_workgroups};
    return set;
}

// per-factor values / twelve partials in this rounding (rdis_hip_eval_each / rdis_hip_grad_each_ba after
// rdis_hip_set_factor_rounding(problem, 1): what the parity tests compare with the oracle's device arithmetic, ==)
namespace {
__global__ void __launch_bounds__(256)
rr_eval_each_kernel(rr::ProblemView P, int nf, const int* __restrict__ fac, double* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
        double f, s;
        rr::factor_value<rr::KIND_BA, false>(P, nullptr, fac ? fac[i] : i, f, s);
        out[i] = f;
    }
}
__global__ void __launch_bounds__(256)
rr_grad_each_kernel(rr::ProblemView P, int nf, const int* __restrict__ fac, double* __restrict__ out12) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
        const int fid = fac ? fac[i] : i;
        const int c = P.cam[fid], q = P.pt[fid];
        const double2 o = P.obs[fid];
        double v[12], g[12];
#pragma unroll
        for (int k = 0; k < 9; ++k) v[k] = P.x[c + k];
#pragma unroll
        for (int k = 0; k < 3; ++k) v[9 + k] = P.x[q + k];
        rr::ba_eval_grad(v, o.x, o.y, g);
#pragma unroll
        for (int k = 0; k < 12; ++k) out12[12ll * i + k] = g[k];
    }
}
}  // namespace
hipError_t refround_eval_each(int grid, hipStream_t stream, const rdis_views::ProblemView& P, int nf, const int* fac, double* out) {
    rr_eval_each_kernel<<<grid, 256, 0, stream>>>(P, nf, fac, out);
    return hipGetLastError();
}
hipError_t refround_grad_each(int grid, hipStream_t stream, const rdis_views::ProblemView& P, int nf, const int* fac, double* out12) {
    rr_grad_each_kernel<<<grid, 256, 0, stream>>>(P, nf, fac, out12);
    return hipGetLastError();
}

}  // namespace rdis_hip
