// ptm_population_kernels.hip -- the population kernels of the point-major streaming solver (solver_ptm_population.hpp) and their
// launch, a translation unit of their own (with cgd_ptm_kernel's they are the library's largest kernels; rdis_hip.hip sees them
// through population_api.hpp).  The instantiation list is ptm_kernels.hip's: 256, 512, and 768 lanes for everything else, rotation
// records that follow the trial point or cameras that are constants.
// (solver_ptm.hpp also defines ptm_gather_kernel, a plain kernel of the plan's set-up that belongs to ptm_kernels.hip: in this unit
// it takes a name of the unit's own, so that the library has one ptm_gather_kernel, and is never launched)
#define ptm_gather_kernel ptm_gather_kernel_of_the_population_unit
#include "solver_ptm.hpp"
#undef ptm_gather_kernel
#include "solver_ptm_population.hpp"
#include "launch_dispatch.hpp"

namespace rdis_hip {

template <int ROT>
static hipError_t population_launch_ptm_rot(int threads, int ncomp_listed, int members_of_launch, size_t dyn, hipStream_t stream, const ProblemView& P,
                                            const PlanView& V, const StartsView& S, const PtmReplicas& RP, double* X, int maxiters, double ftol, int ncb_cap) {
    return with_threads<256, 512, 768>(threads, [&](auto T) {
        return launch_dyn(cgd_ptm_population_kernel<T.value, ROT>, dim3((unsigned)ncomp_listed, (unsigned)members_of_launch), T.value, dyn, stream, P, V, S, RP,
                          X, maxiters, ftol, ncb_cap);
    });
}

hipError_t population_launch_ptm(int rot, int threads, int ncomp_listed, int members_of_launch, size_t dyn, hipStream_t stream, const ProblemView& P,
                                 const PlanView& V, const StartsView& S, const PtmReplicas& RP, double* X, int maxiters, double ftol, int ncb_cap) {
    switch (rot) {
        case ROT_CAMFIX: return population_launch_ptm_rot<ROT_CAMFIX>(threads, ncomp_listed, members_of_launch, dyn, stream, P, V, S, RP, X, maxiters, ftol, ncb_cap);
        default: return population_launch_ptm_rot<ROT_RECORDS>(threads, ncomp_listed, members_of_launch, dyn, stream, P, V, S, RP, X, maxiters, ftol, ncb_cap);
    }
}

}  // namespace rdis_hip
