// population_kernels.hip -- the population kernels of the LDS-resident solver (solver_lds_population.hpp) and of the plain
// one-workgroup solver (solver_wg_population.hpp) and their launches, a
// translation unit of their own (rdis_hip.hip sees them through population_api.hpp), and the kernels that draw, rank and reorder
// the members (population_select.hpp) and evaluate them (population_eval_kernels.hpp).  A workgroup size becomes a template
// argument through launch_dispatch.hpp, with the list of starts_kernels.hip: 64 ... 768, 1024 for everything else.
#define RDIS_POPULATION_SELECT_KERNELS   // (population_select.hpp: its three kernels are defined here and nowhere else)
#define RDIS_LDS_NO_LAUNCHER   // (cgd_lds_kernel is instantiated where it is launched: rdis_hip.hip, refround_kernels.hip)
#include <algorithm>
#include "solver_lds_population.hpp"
#include "solver_wg_population.hpp"
#include "solver_quad_population.hpp"   // (the tiny-component solver's entry: plan option population_tiny)
#include "population_select.hpp"        // (draw, rank, permute: what a restart loop does between two solves)
#include "population_eval_kernels.hpp"  // (evaluation, argmin, gradient: the population forms of eval_kernels.hpp)
#include "population_api.hpp"

namespace rdis_hip {

hipError_t population_launch(int rot, int threads, int ncomp_listed, int members_of_launch, size_t dyn, hipStream_t stream, const ProblemView& P,
                             const PlanView& V, const StartsView& S, double* X, int maxiters, double ftol, int ns_cap, int ncb_cap, int chunk_cap) {
    return with_threads<64, 128, 256, 512, 768, 1024>(threads, [&](auto T) {
        auto* kernel = rot == ROT_CAMFIX ? cgd_lds_population_kernel<T.value, ROT_CAMFIX>
                     : rot == ROT_RECORDS ? cgd_lds_population_kernel<T.value, ROT_RECORDS>
                                          : cgd_lds_population_kernel<T.value, ROT_PER_FACTOR>;
        return launch_dyn(kernel, dim3((unsigned)ncomp_listed, (unsigned)members_of_launch), T.value, dyn, stream, P, V, S, X, maxiters, ftol, ns_cap, ncb_cap, chunk_cap);
    });
}

// (the list of cgd_wg_kernel's launch, rdis_hip.hip launch_wg: a sum's tree depends on the workgroup size)
hipError_t population_launch_wg(int threads, int ncomp_listed, int members_of_launch, hipStream_t stream, const ProblemView& P, const PlanView& V,
                                const StartsView& S, double* X, int maxiters, double ftol) {
    return with_threads<64, 128, 256, 512, 768, 1024>(threads, [&](auto T) {
        cgd_wg_population_kernel<KIND_NLP, T.value><<<dim3((unsigned)ncomp_listed, (unsigned)members_of_launch), T.value, 0, stream>>>(P, V, S, X, maxiters, ftol);
        return hipGetLastError();
    });
}

// (the two instantiations of cgd_group_kernel, rdis_hip.hip: the bits depend on the group size)
hipError_t population_launch_tiny(int group, int blocks_per_member, int members_of_launch, hipStream_t stream, const ProblemView& P, const PlanView& V,
                                  const StartsView& S, double* X, double* XR, const int* list, int ntiny, int* queues, int maxiters, double ftol) {
    const dim3 grid((unsigned)blocks_per_member, (unsigned)members_of_launch);
    if (group == 4) cgd_group_population_kernel<4, QUAD_THREADS><<<grid, QUAD_THREADS, 0, stream>>>(P, V, S, X, XR, list, ntiny, queues, maxiters, ftol);
    else cgd_group_population_kernel<16, 64><<<grid, 64, 0, stream>>>(P, V, S, X, XR, list, ntiny, queues, maxiters, ftol);
    return hipGetLastError();
}

hipError_t population_rotations_launch(hipStream_t stream, const double* X, long long N, long long first, int members_of_launch, const int* cam_blocks,
                                       int nblocks, double* XR) {
    if (nblocks <= 0 || members_of_launch <= 0) return hipSuccess;
    population_rotations_kernel<<<dim3((unsigned)((nblocks + 255) / 256), (unsigned)members_of_launch), 256, 0, stream>>>(X, N, first, cam_blocks, nblocks, XR);
    return hipGetLastError();
}

namespace {
int helper_grid(long long total) { return (int)std::min<long long>((total + 255) / 256, 4096); }
}  // namespace

hipError_t population_gather_launch(hipStream_t stream, const double* X, long long N, const int* free_vid, long long nfree, long long members, double* xstart) {
    const long long total = members * nfree;
    if (total <= 0) return hipSuccess;
    population_gather_kernel<<<helper_grid(total), 256, 0, stream>>>(X, N, free_vid, nfree, total, xstart);
    return hipGetLastError();
}

hipError_t population_scatter_launch(hipStream_t stream, double* X, long long N, long long first, long long count, const int* vid, long long n, const double* val) {
    const long long total = count * n;
    if (total <= 0) return hipSuccess;
    population_scatter_kernel<<<helper_grid(total), 256, 0, stream>>>(X, N, first, vid, n, total, val);
    return hipGetLastError();
}

hipError_t population_pick_launch(hipStream_t stream, const double* X, long long N, long long first, long long count, const int* vid, long long n, double* out) {
    const long long total = count * n;
    if (total <= 0) return hipSuccess;
    population_pick_kernel<<<helper_grid(total), 256, 0, stream>>>(X, N, first, vid, n, total, out);
    return hipGetLastError();
}

hipError_t population_copy_rows_launch(hipStream_t stream, const double* src, double* dst, long long N, long long rows) {
    const long long total = rows * N;
    if (total <= 0) return hipSuccess;
    population_copy_rows_kernel<<<helper_grid(total), 256, 0, stream>>>(src, dst, N, total);
    return hipGetLastError();
}

// grid (blocks over the row, members): the second dimension holds at most 65535, the kernels stride over the rest
hipError_t population_sample_launch(hipStream_t stream, double* X, long long N, long long first, long long count, const int* vid, long long n,
                                    unsigned long long seed, long long stream_id, const double* slo, const double* shi, const double* lo, const double* hi) {
    if (count <= 0 || n <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::min<long long>((n + 255) / 256, 4096), (unsigned)std::min<long long>(count, 65535));
    population_sample_kernel<<<grid, 256, 0, stream>>>(X, N, first, count, vid, n, seed, stream_id, slo, shi, lo, hi);
    return hipGetLastError();
}

hipError_t population_rank_launch(hipStream_t stream, long long members, const double* f, long long* order) {
    if (members <= 0) return hipSuccess;
    population_rank_kernel<<<(unsigned)((members + 255) / 256), 256, 0, stream>>>(members, f, order);
    return hipGetLastError();
}

hipError_t population_permute_rows_launch(hipStream_t stream, long long members, long long N, const long long* order, const double* X, const double* f,
                                          double* X2, double* f2) {
    if (members <= 0) return hipSuccess;
    const dim3 grid((unsigned)std::max<long long>(1, std::min<long long>((N + 255) / 256, 4096)), (unsigned)std::min<long long>(members, 65535));
    population_permute_rows_kernel<<<grid, 256, 0, stream>>>(members, N, order, X, f, X2, f2);
    return hipGetLastError();
}

// ---- evaluation, argmin, gradient: the grids are the callers' (population_entries.hip), which take them from the single-x entries ----

hipError_t population_eval_sum_launch(hipStream_t stream, int kind, int nb, int members_of_launch, const ProblemView& P, double* X, long long first, int nf,
                                      const int* fac, double* partial) {
    const dim3 grid((unsigned)nb, (unsigned)members_of_launch);
    if (kind == KIND_BA) population_eval_sum_kernel<KIND_BA><<<grid, 256, 0, stream>>>(P, X, first, nf, fac, partial);
    else population_eval_sum_kernel<KIND_NLP><<<grid, 256, 0, stream>>>(P, X, first, nf, fac, partial);
    return hipGetLastError();
}

hipError_t population_final_sum_launch(hipStream_t stream, int members_of_launch, int n, const double* partial, long long first, double* f) {
    population_final_sum_kernel<<<members_of_launch, 256, 0, stream>>>(n, partial, first, f);
    return hipGetLastError();
}

hipError_t population_argmin_launch(hipStream_t stream, long long members, const double* f, MemberValue* best) {
    population_argmin_kernel<<<1, 256, 0, stream>>>(members, f, best);
    return hipGetLastError();
}

hipError_t population_copy_best_launch(hipStream_t stream, int grid, const double* X, long long N, const MemberValue* best, double* x) {
    population_copy_best_kernel<<<grid, 256, 0, stream>>>(X, N, best, x);
    return hipGetLastError();
}

// (population_partials_launch, population_eval_sum_grad_launch: rdis_hip.hip, where their kernels compile to the text they had)

hipError_t population_gather_grad_launch(hipStream_t stream, int grid, int members_of_launch, int nvars, const int* v2s_ptr, const int* v2s_idx,
                                         const double* gfac, long long nslots, double* G, long long row0) {
    population_gather_grad_kernel<<<dim3((unsigned)grid, (unsigned)members_of_launch), 256, 0, stream>>>(nvars, v2s_ptr, v2s_idx, gfac, nslots, G, row0);
    return hipGetLastError();
}

hipError_t population_grad_max_launch(hipStream_t stream, long long rows, long long N, const double* G, double* gmax) {
    population_grad_max_kernel<<<(unsigned)rows, 256, 0, stream>>>(N, G, gmax);
    return hipGetLastError();
}

}  // namespace rdis_hip
