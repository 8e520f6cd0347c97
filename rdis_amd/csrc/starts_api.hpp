// starts_api.hpp -- what the C ABI's translation units (through abi_state.hpp: StartsView; rdis_hip.hip: the launches) see of the multi-start entries of the LDS-resident solver (solver_lds_starts.hpp) and of
// the plain one-workgroup solver (solver_wg_starts.hpp), whose kernels are a translation unit of their own (starts_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include "device_views.hpp"

namespace rdis_views {

// The per-solve arrays of a multi-start solve.  Inputs and outputs hold every start of the call, row-major [start][...],
// and are kept until fetched; the workspace holds the replicas of one launch, which solves the starts first .. first + gridDim.y - 1.
struct StartsView {
    const double* xstart;   // [nstarts][nfree]
    double* xout;           // [nstarts][nfree]
    double* fret;           // [nstarts][ncomp] ...
    double* delta;
    int* iters;
    int* status;
    long long* nfeval;
    long long* ngeval;
    double* ws;             // [replicas][5 nfree]   PlanView::ws of a replica
    double* gfac;           // [replicas][ngfac]     PlanView::gfac of a replica
    double* x;              // [replicas][N]         plain solver only: ProblemView::x of a replica (the trial point lives there) ...
    double* dir;            // [replicas][N]         ... and PlanView::dir of a replica; zero between launches
    long long nfree, ngfac, N; // row lengths
    long long first;        // the launch's first start
};

// The replicas of the cooperative solver's per-solve arrays on a population (solver_coop_population.hpp; the replica of gfac is
// StartsView::gfac): replica r of the launch publishes the direction of a group whose CoopArgs::xi_glob is xi_plan + off at
// xi + r xi_doubles + off, and group g of the launch exchanges through st[r groups + g].  Both instantiations of the kernel
// (refround_api.hpp) take this very struct.
struct CoopReplicas {
    double* xi;              // [replicas][xi_doubles]
    const double* xi_plan;   // the plan's own xi_glob: the base the groups' offsets are taken from
    long long xi_doubles;
    CoopState* st;           // [replicas][groups]
    int groups;              // states per replica: the most groups a launch of the plan has
    long long* timing;       // CoopArgs::timing of every group: null (no member's group writes the problem's debug counters)
};

}  // namespace rdis_views

namespace rdis_hip {

// the view of start (S.first + r), replica r of the launch
__device__ __forceinline__ PlanView starts_shift(PlanView L, const StartsView& S, int r) {
    const long long s = S.first + r;
    L.xstart = S.xstart + s * S.nfree;
    L.xout = S.xout + s * S.nfree;
    L.fret = S.fret + s * L.ncomp; L.delta = S.delta + s * L.ncomp;
    L.iters = S.iters + s * L.ncomp; L.status = S.status + s * L.ncomp;
    L.nfeval = S.nfeval + s * L.ncomp; L.ngeval = S.ngeval + s * L.ncomp;
    L.ws = S.ws + (long long)r * 5 * S.nfree;
    L.gfac = S.gfac + (long long)r * S.ngfac;
    L.trace = nullptr; L.trace_n = nullptr; L.trace_cap = 0;
    L.vdump = nullptr; L.dump_iters = 0;
    return L;
}

// cgd_lds_starts_kernel<threads, rot>: grid (ncomp_listed, nstarts_of_launch); V.order lists the components
hipError_t starts_launch(int rot, int threads, int ncomp_listed, int nstarts_of_launch, size_t dyn, hipStream_t stream, const ProblemView& P,
                         const PlanView& V, const StartsView& S, int maxiters, double ftol, int ns_cap, int ncb_cap, int chunk_cap);
// cgd_wg_starts_kernel<KIND_NLP, threads>: the plain solver's, same grid; S.x and S.dir hold the launch's replicas
hipError_t starts_launch_wg(int threads, int ncomp_listed, int nstarts_of_launch, hipStream_t stream, const ProblemView& P, const PlanView& V,
                            const StartsView& S, int maxiters, double ftol);
// starts_fill_x_kernel: every one of the `replicas` rows of S.x = P.x
hipError_t starts_fill_x_launch(hipStream_t stream, const ProblemView& P, const StartsView& S, long long replicas);
// select_best_start_kernel over the S.fret of all nstarts starts: best[ncomp], the plan's ordinary outputs, P.x
hipError_t starts_select_launch(hipStream_t stream, const ProblemView& P, const PlanView& V, const StartsView& S, long long nstarts, int* best);

}  // namespace rdis_hip
