// ptm_kernels.hip -- the point-major streaming solver's kernels (solver_ptm.hpp) and their launches, a translation
// unit of their own (they are the library's largest kernels; rdis_hip.hip sees them through ptm_api.hpp).  A workgroup size
// becomes a template argument through launch_dispatch.hpp: 256, 512, and 768 for everything else.
#include "solver_ptm.hpp"
#include "launch_dispatch.hpp"

namespace rdis_hip {

template <int ROT>
static hipError_t ptm_launch_rot(int threads, int grid, size_t dyn, hipStream_t stream, const ProblemView& P, const PlanView& V,
                                 int maxiters, double ftol, int ncb_cap) {
    return with_threads<256, 512, 768>(threads, [&](auto T) {
        return launch_dyn(cgd_ptm_kernel<T.value, ROT>, grid, T.value, dyn, stream, P, V, maxiters, ftol, ncb_cap);
    });
}

hipError_t ptm_launch(int rot, int threads, int grid, size_t dyn, hipStream_t stream, const ProblemView& P, const PlanView& V,
                      int maxiters, double ftol, int ncb_cap) {
    switch (rot) {
        case ROT_CAMFIX: return ptm_launch_rot<ROT_CAMFIX>(threads, grid, dyn, stream, P, V, maxiters, ftol, ncb_cap);
        default: return ptm_launch_rot<ROT_RECORDS>(threads, grid, dyn, stream, P, V, maxiters, ftol, ncb_cap);
    }
}

template <int ROT>
static const void* ptmg_kernel_ptr(int threads, bool wide, bool local) {
    if (wide && local) return (const void*)cgd_ptmg_kernel<PTM_WIDE_THREADS, ROT, true, true>;
    if (wide) return (const void*)cgd_ptmg_kernel<PTM_WIDE_THREADS, ROT, true>;
    return with_threads<256, 512, 768>(threads, [](auto T) { return (const void*)cgd_ptmg_kernel<T.value, ROT>; });
}
const void* ptmg_kernel_fn(int rot, int threads, bool wide, bool local) {
    switch (rot) {
        case ROT_CAMFIX: return ptmg_kernel_ptr<ROT_CAMFIX>(threads, wide, local);
        default: return ptmg_kernel_ptr<ROT_RECORDS>(threads, wide, local);
    }
}

hipError_t ptm_gather_launch(int grid, hipStream_t stream, int n, const int* jg, const unsigned* fidx, const double2* fobs,
                             short* pcam, double2* pobs) {
    ptm_gather_kernel<<<grid, 256, 0, stream>>>(n, jg, fidx, fobs, pcam, pobs);
    return hipGetLastError();
}

}  // namespace rdis_hip
