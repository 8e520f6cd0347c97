// starts_kernels.hip -- the multi-start kernels of the LDS-resident solver (solver_lds_starts.hpp) and of the plain
// one-workgroup solver (solver_wg_starts.hpp) and their launches, a translation unit of their own (rdis_hip.hip sees them through starts_api.hpp).  A workgroup size becomes a template
// argument through launch_dispatch.hpp, as in solver_lds.hpp's launch_lds: 64 ... 768, 1024 for everything else.
#define RDIS_LDS_NO_LAUNCHER   // (cgd_lds_kernel is instantiated where it is launched: rdis_hip.hip, refround_kernels.hip)
#include <algorithm>
#include "solver_lds_starts.hpp"
#include "solver_wg_starts.hpp"

namespace rdis_hip {

hipError_t starts_launch(int rot, int threads, int ncomp_listed, int nstarts_of_launch, size_t dyn, hipStream_t stream, const ProblemView& P,
                         const PlanView& V, const StartsView& S, int maxiters, double ftol, int ns_cap, int ncb_cap, int chunk_cap) {
    return with_threads<64, 128, 256, 512, 768, 1024>(threads, [&](auto T) {
        auto* kernel = rot == ROT_CAMFIX ? cgd_lds_starts_kernel<T.value, ROT_CAMFIX>
                     : rot == ROT_RECORDS ? cgd_lds_starts_kernel<T.value, ROT_RECORDS>
                                          : cgd_lds_starts_kernel<T.value, ROT_PER_FACTOR>;
        return launch_dyn(kernel, dim3((unsigned)ncomp_listed, (unsigned)nstarts_of_launch), T.value, dyn, stream, P, V, S, maxiters, ftol, ns_cap, ncb_cap, chunk_cap);
    });
}

// (the list of cgd_wg_kernel's launch, rdis_hip.hip launch_wg: a sum's tree depends on the workgroup size)
hipError_t starts_launch_wg(int threads, int ncomp_listed, int nstarts_of_launch, hipStream_t stream, const ProblemView& P, const PlanView& V,
                            const StartsView& S, int maxiters, double ftol) {
    return with_threads<64, 128, 256, 512, 768, 1024>(threads, [&](auto T) {
        cgd_wg_starts_kernel<KIND_NLP, T.value><<<dim3((unsigned)ncomp_listed, (unsigned)nstarts_of_launch), T.value, 0, stream>>>(P, V, S, maxiters, ftol);
        return hipGetLastError();
    });
}

hipError_t starts_fill_x_launch(hipStream_t stream, const ProblemView& P, const StartsView& S, long long replicas) {
    const long long total = replicas * S.N;
    if (total <= 0) return hipSuccess;
    const int grid = (int)std::min<long long>((total + 255) / 256, 4096);
    starts_fill_x_kernel<<<grid, 256, 0, stream>>>(P.x, S.x, S.N, total);
    return hipGetLastError();
}

hipError_t starts_select_launch(hipStream_t stream, const ProblemView& P, const PlanView& V, const StartsView& S, long long nstarts, int* best) {
    const int grid = V.ncomp < 1 ? 1 : V.ncomp > 4096 ? 4096 : V.ncomp;
    select_best_start_kernel<<<grid, 256, 0, stream>>>(P, V, S, nstarts, best);
    return hipGetLastError();
}

}  // namespace rdis_hip
