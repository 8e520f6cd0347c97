// solver_wg_starts.hpp -- the multi-start entry of the plain one-workgroup solver (solver_wg.hpp), the counterpart of
// solver_lds_starts.hpp for nonlinear-product components: the same decomposition solved from many starting points in one
// launch, one workgroup per (component, start).
//
// Nonlinear-product functions are where RDIS lives on restarts (optSinusoid and the polynomial tests: sampleRandomState,
// reference src/RDISOptimizer.cpp:1196-1216, a node's restarts :1087-1094), and where one solve uses the device worst: a
// component is one workgroup walking a chain of dependent evaluations.  The starts are the parallelism such a problem has.
//
// Unlike the LDS-resident solver, cgd_wg_kernel keeps its trial point in global memory: assign_line / assign_vec write P.x,
// line_begin writes L.dir, and the factors gather from both.  So a replica of this solver carries two arrays more:
//
//   per start, kept until fetched    xstart[s][nfree]  xout[s][nfree]  fret / delta / iters / status / nfeval / ngeval [s][ncomp]
//   per start of a launch (replica)  ws[r][5 nfree]  gfac[r][ngfac]  x[r][N]  dir[r][N]
//
// blockIdx.x is the component (heaviest first, as in cgd_wg_kernel), blockIdx.y the start within the launch: the workgroup
// runs WgEnv / CgdMachine / run_machine unchanged on a ProblemView whose x is replica r's and a PlanView whose dir, ws, gfac
// and per-solve outputs are shifted to its replica and start -- the arithmetic, the order of every sum (the workgroup size is
// the one plan_solve picks) and so the bits of a row are those of cgd_wg_kernel from that row.
//
// No start sees another's values, and the solver never writes the problem's own x or dir:
//   x    starts_fill_x_kernel copies P.x into every replica before the first launch of a call: that is how a component's
//        constants arrive.  A replica reused by a later launch of the same call needs no refill: the solver assigns every
//        free variable of a component (init_vectors, then assign_vec / assign_line before any evaluation) before a factor
//        reads it, and a constant of one component is never free in another of the same plan -- so what an earlier start
//        left in the free entries is never read, and the constants are never written.
//   dir  zero when allocated; the kernel leaves the free entries it wrote zero on exit, as cgd_wg_kernel does.
// select_best_start_kernel (solver_lds_starts.hpp), after the last launch, assigns per component the start with the lowest
// value and copies its row into the plan's ordinary outputs and the problem's x.
#pragma once
#include "solver_wg.hpp"
#include "solver_lds_starts.hpp"   // starts_shift, select_best_start_kernel

namespace rdis_hip {

// every replica's copy of the problem's variables: xr[r][N] = x[N]; plain vector stores
__global__ void __launch_bounds__(256)
starts_fill_x_kernel(const double* __restrict__ x, double* __restrict__ xr, long long N, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        xr[i] = x[i % N];
}

// (launch bounds: cgd_wg_kernel's)
template <int KIND, int THREADS>
__global__ void __launch_bounds__(THREADS, (THREADS <= 256 ? 2 : 1))
cgd_wg_starts_kernel(ProblemView P0, PlanView L0, StartsView S, int maxiters, double ftol) {
    __shared__ double red[2][3][MAX_WAVES];
    __shared__ int long_q[WG_LONG_QUEUE];
    __shared__ int long_n;
    ProblemView P = P0;
    P.x = S.x + (long long)blockIdx.y * S.N;
    PlanView L = starts_shift(L0, S, (int)blockIdx.y);
    L.dir = S.dir + (long long)blockIdx.y * S.N;
    const int comp = L.order[blockIdx.x];
    const int f0 = L.free_ptr[comp], f1 = L.free_ptr[comp + 1];
    const int c0 = L.fac_ptr[comp], c1 = L.fac_ptr[comp + 1];
    const int n = f1 - f0, m = c1 - c0;

    if (m == 0) {  // nothing to optimise: return 0, this start's x as it came (.cpp:26-29)
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
    // gdmin.p with sanitisation (.cpp:61) into the replica's x; after a rollback it already holds clamp(x_init)
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
