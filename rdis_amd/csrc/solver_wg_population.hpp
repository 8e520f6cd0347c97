// solver_wg_population.hpp -- the population entry of the plain one-workgroup solver (solver_wg.hpp), the counterpart of
// solver_lds_population.hpp for nonlinear-product components: one plan solved on S complete states resident on the device,
// one workgroup per (component, member).
//
// Nonlinear-product functions are where RDIS lives on restarts (optSinusoid and the polynomial tests: sampleRandomState,
// reference src/RDISOptimizer.cpp:1196-1216): a whole state is drawn and the decomposition run on it, so from the second
// half-round on the constants of restart s are restart s's own earlier results.  The multi-start entry
// (solver_wg_starts.hpp), whose constants are the problem's x for every start, cannot serve that.  Here every member has its
// own x, X[s][N]:
//
//   per member, the population's     X[s][N]            start AND constants of member s; trial points and the result go into it
//   per member, kept until fetched   xstart[s][nfree]  xout[s][nfree]  fret / delta / iters / status / nfeval / ngeval [s][ncomp]
//   per member of a launch (replica) ws[r][5 nfree]  gfac[r][ngfac]  dir[r][N]
//
// population_gather_kernel (solver_lds_population.hpp) fills xstart[s] = X[s][free_vid] for all members before the first
// launch (what plan_set_start(plan, NULL) does on a problem whose x is X[s]).  blockIdx.x is the component (heaviest first, as
// in cgd_wg_kernel), blockIdx.y the member within the launch: the workgroup runs WgEnv / CgdMachine / run_machine unchanged on
// a ProblemView whose x is X[first + r] and a PlanView shifted by starts_shift whose dir is replica r's -- the arithmetic, the
// order of every sum (the workgroup size is the one plan_solve picks) and so the bits of (s, c) are those of cgd_wg_kernel on a
// problem whose assigned x is X[s].
//
// The plain solver keeps its trial point in global memory (assign_line / assign_vec write P.x, the factors gather from it), so
// during the launch the member's row carries trial points; at the end it holds what cgd_wg_kernel leaves in P.x: assign_vec(p),
// or clamp(x_init) after a roll-back.  Unlike cgd_wg_starts_kernel this needs NO replica of x.  INVARIANT:
//   - the components of a plan are independent (plan_create checks it: RDIS_HIP_EOVERLAP) -- no free variable is shared, and no
//     factor of one component reads a free variable of another.  So a variable that workgroup (c, s) writes into X[s], trial
//     points included, is read by no other workgroup of member s, in this launch or in another launch of the same call;
//   - a constant of the plan is never written: every workgroup of member s reads the value the member came with;
//   - workgroups of other members read and write other rows.
// That is the argument that lets cgd_wg_kernel run its components side by side on one P.x.  (A component's stores are plain
// vector stores of whole doubles: a neighbour's variable on the same cache line is not disturbed, and a stale copy of it in
// this compute unit's cache is never read.)  The gather kernel has finished before the first solver launch starts (one stream).
//   dir  lives in the plan's ms_dir, zero when allocated; the kernel leaves the free entries it wrote zero on exit, as
//        cgd_wg_starts_kernel does, so the replica serves the next launch and the multi-start entry as it is.
// The problem's own x and dir are not touched.  No trace and no vector dump are written (starts_shift clears them).
#pragma once
#include "solver_wg.hpp"
#include "starts_api.hpp"

namespace rdis_hip {

// (instantiation list and launch bounds: cgd_wg_kernel's -- a sum's tree depends on the workgroup size)
template <int KIND, int THREADS>
__global__ void __launch_bounds__(THREADS, (THREADS <= 256 ? 2 : 1))
cgd_wg_population_kernel(ProblemView P0, PlanView L0, StartsView S, double* X, int maxiters, double ftol) {
    __shared__ double red[2][3][MAX_WAVES];
    __shared__ int long_q[WG_LONG_QUEUE];
    __shared__ int long_n;
    ProblemView P = P0;
    P.x = X + (S.first + (long long)blockIdx.y) * S.N;   // member first + r: its constants, its trial points, its result
    PlanView L = starts_shift(L0, S, (int)blockIdx.y);
    L.dir = S.dir + (long long)blockIdx.y * S.N;
    const int comp = L.order[blockIdx.x];
    const int f0 = L.free_ptr[comp], f1 = L.free_ptr[comp + 1];
    const int c0 = L.fac_ptr[comp], c1 = L.fac_ptr[comp + 1];
    const int n = f1 - f0, m = c1 - c0;

    if (m == 0) {  // nothing to optimise: return 0, the member's x untouched (.cpp:26-29)
        for (int i = threadIdx.x; i < n; i += blockDim.x) L.xout[f0 + i] = L.xstart[f0 + i];
        if (threadIdx.x == 0) {
            L.fret[comp] = 0.0; L.delta[comp] = 0.0; L.iters[comp] = 0;
            L.status[comp] = EXIT_EMPTY; L.nfeval[comp] = 0; L.ngeval[comp] = 0;
        }
        return;
    }

    double* ws = L.ws + 5ll * f0;
    WgEnv<KIND> E{P, L, comp, n, m, c0, (int)threadIdx.x, (int)blockDim.x, (int)(blockDim.x >> 6),
                  L.free_vid + f0, L.fac_id + c0, L.v2s_ptr + f0,
                  ws, ws + n, ws + 2ll * n, ws + 3ll * n, ws + 4ll * n,
                  red, 0, long_q, &long_n, nullptr, 0, 0};

    __shared__ CgdMachine M;
    __shared__ Request Q[2];
    E.init_vectors();
    run_machine(E, M, Q, maxiters, ftol);
    // gdmin.p with sanitisation (.cpp:61) into the member's x (the invariant above); after a rollback it already holds clamp(x_init)
    if (!M.rolled_back) E.assign_vec(E.p);
    for (int i = E.tid; i < n; i += E.nt) {
        L.xout[f0 + i] = P.x[E.fv[i]];
        L.dir[E.fv[i]] = 0.0;  // the replica's dir is zero between launches
    }
    if (E.tid == 0) {
        L.fret[comp] = M.fret; L.delta[comp] = delta_fval(M.fret, M.finit, M.rolled_back); L.iters[comp] = M.iter;
        L.status[comp] = M.status(); L.nfeval[comp] = M.nfeval; L.ngeval[comp] = M.ngeval;
    }
}

}  // namespace rdis_hip
