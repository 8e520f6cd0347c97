// population_api.hpp -- what rdis_hip.hip and population_entries.hip see of the population entries of the LDS-resident solver (solver_lds_population.hpp)
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

// ---- a population's evaluation, argmin and gradient (population_eval_kernels.hpp); the shapes are the callers' ----
// The member a population keeps: the minimum of f[members] by better() (population_select.hpp)
struct MemberValue { double f; long long s; };
// population_eval_sum_kernel<kind>: grid (nb, members_of_launch); partial[members_of_launch][nb]
hipError_t population_eval_sum_launch(hipStream_t stream, int kind, int nb, int members_of_launch, const ProblemView& P, double* X, long long first, int nf,
                                      const int* fac, double* partial);
// population_final_sum_kernel: f[first + r] = the sum of partial[r][0 .. n), r < members_of_launch
hipError_t population_final_sum_launch(hipStream_t stream, int members_of_launch, int n, const double* partial, long long first, double* f);
// population_argmin_kernel (one workgroup) and population_copy_best_kernel (grid blocks): x = X[best->s]
hipError_t population_argmin_launch(hipStream_t stream, long long members, const double* f, MemberValue* best);
hipError_t population_copy_best_launch(hipStream_t stream, int grid, const double* X, long long N, const MemberValue* best, double* x);
// population_partials_kernel, population_eval_sum_grad_kernel<kind>, population_gather_grad_kernel: grid (grid, members_of_launch);
// gfac[members_of_launch][nslots], member first + r's gradient is row row0 + r of G.  The first two kernels are eval_kernels.hpp's and
// their launches rdis_hip.hip's (elsewhere they compile to other text), the third is population_kernels.hip's like the rest
hipError_t population_partials_launch(hipStream_t stream, int grid, int members_of_launch, const ProblemView& P, double* X, long long first, int nf,
                                      const int* fac, double* gfac, long long nslots);
hipError_t population_eval_sum_grad_launch(hipStream_t stream, int kind, int grid, int members_of_launch, const ProblemView& P, double* X, long long first,
                                           int nf, const int* fac, double* gfac, long long nslots, double* partial);
hipError_t population_gather_grad_launch(hipStream_t stream, int grid, int members_of_launch, int nvars, const int* v2s_ptr, const int* v2s_idx,
                                         const double* gfac, long long nslots, double* G, long long row0);
// population_grad_max_kernel: gmax[k] = max |G[k][.]| for k < rows, a workgroup a row
hipError_t population_grad_max_launch(hipStream_t stream, long long rows, long long N, const double* G, double* gmax);

}  // namespace rdis_hip
