// solver_lds_starts.hpp -- the multi-start entry of the LDS-resident solver (solver_lds.hpp): the same decomposition
// solved from many starting points in one launch, one workgroup per (start, component).
//
// RDIS is a multi-start method: optBA's sample loop (reference src/bundleadjust/optBA.cpp:198-224), a node's random
// restarts (src/RDISOptimizer.cpp:1087-1094) and sampleRandomState (:1196-1216) all solve one decomposition again from
// other values.  A component's iterate lives in LDS, its index tables are read-only and its constants come from the
// problem's x, so a start needs a copy of the per-solve arrays only:
//
//   per start, kept until fetched    xstart[s][nfree]  xout[s][nfree]  fret / delta / iters / status / nfeval / ngeval [s][ncomp]
//   per start of a launch (replica)  ws[r][5 nfree]  gfac[r][ngfac]     -- g, h of the recurrence and the point partials
//
// blockIdx.x is the component (heaviest first, as in cgd_lds_kernel), blockIdx.y the start within the launch: the workgroup
// runs LdsEnv / CgdMachine / run_machine unchanged on a PlanView whose per-solve pointers are shifted to its start and
// replica -- the arithmetic, the order of every sum and so the bits of a row are those of cgd_lds_kernel from that row.
// It does NOT write P.x at its end: no start may see another's result (a constant of one component is never free in
// another of the same plan, but P.x is also what a start's init_vectors reads).  select_best_start_kernel, after the last
// launch, assigns per component the start with the lowest value and copies its row into the plan's ordinary outputs.
#pragma once
#include "solver_lds.hpp"
#include "starts_api.hpp"

namespace rdis_hip {

// (starts_shift, the view of start S.first + r on replica r of the launch: starts_api.hpp -- solver_lds_population.hpp shifts alike)

template <int THREADS, int ROT>
__global__ void __launch_bounds__(THREADS, (THREADS <= 256 ? 2 : 1))
cgd_lds_starts_kernel(ProblemView P, PlanView L0, StartsView S, int maxiters, double ftol, int ns_cap, int ncb_cap, int chunk_cap) {
    extern __shared__ double lds_dyn[];
    __shared__ double red[2][3][MAX_WAVES];
    const PlanView L = starts_shift(L0, S, (int)blockIdx.y);
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
    const int s0 = L.ls_ptr[comp], ns = L.ls_ptr[comp + 1] - s0, ncb = L.ls_ncb[comp];
    double* base = lds_dyn;
    double* CG = base + LDS_DOUBLES_PER_SLOT * ns_cap + 7 * ncb_cap;
    int* CGC = (int*)(CG + 9 * chunk_cap);
    int* SF = CGC + chunk_cap;
    int* CHE = SF + ns_cap;
    double* CTR = reinterpret_cast<double*>(reinterpret_cast<char*>(lds_dyn) + lds_matrix_offset(lds_bytes_for(ns_cap, ncb_cap, chunk_cap)));
    double* CDR = CTR + LDS_TS * ncb_cap;   // (allocated only when ls_matrix is set)
    for (int s = threadIdx.x; s < ns; s += blockDim.x) SF[s] = L.ls_free[s0 + s];
    __syncthreads();
    double* ws = L.ws + 5ll * f0;
    LdsEnv<ROT, (THREADS <= 512)> E{P, L, comp, n, m, f0, c0, (int)threadIdx.x, (int)blockDim.x, (int)(blockDim.x >> 6),
                  ns, ncb, L.ls_obs + c0, L.ls_fidx + c0, L.ls_gperm + 64ll * L.ls_gptr[comp], L.ls_gptr[comp + 1] - L.ls_gptr[comp], CG, CGC, L.v2s_ptr + f0, L.ls_vid + s0,
                  base, base + ns_cap, base + 2 * ns_cap, base + 3 * ns_cap, base + 4 * ns_cap, base + LDS_DOUBLES_PER_SLOT * ns_cap,
                  CTR, CDR, SF, CHE, nullptr, nullptr, 0, ws + 2ll * n, ws + 3ll * n,
                  red, 0, nullptr, 0, 0
#ifdef RDIS_COOP_TIMING
                  , {}
#endif
    };

    __shared__ CgdMachine M;
    __shared__ Request Q[2];
    E.init_vectors();
    run_machine(E, M, Q, maxiters, ftol);
    // gdmin.p with sanitisation (.cpp:61); after a rollback X already holds clamp(x_init).  To this start's row only.
    if (!M.rolled_back) E.assign_p();
    for (int s = E.tid; s < ns; s += E.nt) {
        const int fi = SF[s];
        if (fi >= 0) L.xout[f0 + fi] = E.X[s];
    }
    if (E.tid == 0) {
        L.fret[comp] = M.fret; L.delta[comp] = delta_fval(M.fret, M.finit, M.rolled_back); L.iters[comp] = M.iter;
        L.status[comp] = M.status(); L.nfeval[comp] = M.nfeval; L.ngeval[comp] = M.ngeval;
    }
}

// What an RDIS node keeps of its restarts, the minimum: per component the start with the lowest value (the lowest index on a
// tie; a NaN never, unless every start's is one: then start 0).  Its row becomes the plan's ordinary outputs (what plan_fetch
// returns and objective_sum_kernel adds) and the assignment of the component's free variables -- but for an empty component,
// whose solve touches no variable (cgd_lds_kernel).  One workgroup per component; plain stores.
__global__ void __launch_bounds__(256)
select_best_start_kernel(ProblemView P, PlanView L, StartsView S, long long nstarts, int* best) {
    __shared__ int bsel;
    for (int comp = blockIdx.x; comp < L.ncomp; comp += gridDim.x) {
        if (threadIdx.x == 0) {
            int b = 0;
            double fb = S.fret[comp];
            for (long long s = 1; s < nstarts; ++s) {
                const double f = S.fret[s * L.ncomp + comp];
                if (f < fb || (fb != fb && f == f)) { fb = f; b = (int)s; }
            }
            bsel = b;
            const long long o = (long long)b * L.ncomp + comp;
            best[comp] = b;
            L.fret[comp] = S.fret[o]; L.delta[comp] = S.delta[o]; L.iters[comp] = S.iters[o];
            L.status[comp] = S.status[o]; L.nfeval[comp] = S.nfeval[o]; L.ngeval[comp] = S.ngeval[o];
            L.trace_n[comp] = 0;
        }
        __syncthreads();
        const int f0 = L.free_ptr[comp], n = L.free_ptr[comp + 1] - f0;
        const bool assign = L.fac_ptr[comp + 1] > L.fac_ptr[comp];
        const double* row = S.xout + (long long)bsel * S.nfree + f0;
        for (int i = threadIdx.x; i < n; i += blockDim.x) {
            const double xv = row[i];
            L.xout[f0 + i] = xv;
            if (assign) P.x[L.free_vid[f0 + i]] = xv;
        }
        __syncthreads();
    }
}

}  // namespace rdis_hip
