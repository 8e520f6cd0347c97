// population_api.hpp -- what rdis_hip.hip sees of the population entries of the LDS-resident solver (solver_lds_population.hpp)
// and of the plain one-workgroup solver (solver_wg_population.hpp), whose kernels are a translation unit of their own (population_kernels.hip),
// and of the point-major streaming solver (solver_ptm_population.hpp; ptm_population_kernels.hip).  The per-solve arrays are the multi-start
// entry's (starts_api.hpp: StartsView); the population itself is X[members][N], row-major.
#pragma once
#include "starts_api.hpp"

namespace rdis_hip {

// cgd_lds_population_kernel<threads, rot>: grid (ncomp_listed, members_of_launch); V.order lists the components; member
// S.first + blockIdx.y reads its constants from X[S.first + blockIdx.y] and is assigned there
hipError_t population_launch(int rot, int threads, int ncomp_listed, int members_of_launch, size_t dyn, hipStream_t stream, const ProblemView& P,
                             const PlanView& V, const StartsView& S, double* X, int maxiters, double ftol, int ns_cap, int ncb_cap, int chunk_cap);
// cgd_wg_population_kernel<KIND_NLP, threads>: the plain solver's, same grid; the member's row of X carries its trial points too,
// S.dir holds the launch's replicas of dir (S.x is not used: no replica of x)
hipError_t population_launch_wg(int threads, int ncomp_listed, int members_of_launch, hipStream_t stream, const ProblemView& P, const PlanView& V,
                                const StartsView& S, double* X, int maxiters, double ftol);
// cgd_group_population_kernel<group, threads> (solver_quad_population.hpp; group 4: <4, QUAD_THREADS>, else <16, 64>): grid
// (blocks_per_member, members_of_launch) on the tiny components list[0 .. ntiny); queues[members_of_launch] zero at the start;
// XR null, or the launch's rotation records [members_of_launch][N] (P.rot_mode == ROT_CAMFIX)
hipError_t population_launch_tiny(int group, int blocks_per_member, int members_of_launch, hipStream_t stream, const ProblemView& P, const PlanView& V,
                                  const StartsView& S, double* X, double* XR, const int* list, int ntiny, int* queues, int maxiters, double ftol);
// The replicas of the point-major streaming solver's per-solve arrays (solver_ptm_population.hpp): replica r of the launch has
// PlanView::pm_rec at rec + 6 blocks r, pm_gh at gh + 6 blocks r, pm_bex at bex + 6 blocks r and pm_cbox at cbox + 8 chunks r,
// each laid out like the plan's own array (blocks: point blocks of the plan's point-major components, chunks: entries of pm_cptr)
struct PtmReplicas {
    double* rec;
    double* gh;
    double* bex;
    float* cbox;
    long long blocks, chunks;
};
// cgd_ptm_population_kernel<threads, rot> (threads 256 / 512 / 768 as cgd_ptm_kernel's): grid (ncomp_listed, members_of_launch) on
// the components V.order lists -- point-major ones and components without factors; dyn = ptm_bytes_for(ncb_cap, threads, V.pm_round_slots)
hipError_t population_launch_ptm(int rot, int threads, int ncomp_listed, int members_of_launch, size_t dyn, hipStream_t stream, const ProblemView& P,
                                 const PlanView& V, const StartsView& S, const PtmReplicas& RP, double* X, int maxiters, double ftol, int ncb_cap);
// population_rotations_kernel: XR[r] = the rotation records of member S.first + r's cameras, r < members_of_launch
hipError_t population_rotations_launch(hipStream_t stream, const double* X, long long N, long long first, int members_of_launch, const int* cam_blocks,
                                       int nblocks, double* XR);
// population_gather_kernel: xstart[s][nfree] = X[s][free_vid] for s < members
hipError_t population_gather_launch(hipStream_t stream, const double* X, long long N, const int* free_vid, long long nfree, long long members, double* xstart);
// population_scatter_kernel / population_pick_kernel: members first .. first + count - 1, n values each (vid null: variables 0 .. n-1)
hipError_t population_scatter_launch(hipStream_t stream, double* X, long long N, long long first, long long count, const int* vid, long long n, const double* val);
hipError_t population_pick_launch(hipStream_t stream, const double* X, long long N, long long first, long long count, const int* vid, long long n, double* out);
// population_copy_rows_kernel: `rows` rows of dst, each a copy of src[N]
hipError_t population_copy_rows_launch(hipStream_t stream, const double* src, double* dst, long long N, long long rows);
// population_sample_kernel (population_select.hpp): members first .. first + count - 1 at the variables vid[0 .. n) (null: 0 .. n-1)
// drawn from (seed, stream, member, variable); slo / shi the sampling intervals, lo / hi the domains, [N] each
hipError_t population_sample_launch(hipStream_t stream, double* X, long long N, long long first, long long count, const int* vid, long long n,
                                    unsigned long long seed, long long stream_id, const double* slo, const double* shi, const double* lo, const double* hi);
// population_rank_kernel: order[rank of s] = s under better() on (f[s], s)
hipError_t population_rank_launch(hipStream_t stream, long long members, const double* f, long long* order);
// population_permute_rows_kernel: X2[r] = X[order[r]], f2[r] = f[order[r]]
hipError_t population_permute_rows_launch(hipStream_t stream, long long members, long long N, const long long* order, const double* X, const double* f,
                                          double* X2, double* f2);

}  // namespace rdis_hip
