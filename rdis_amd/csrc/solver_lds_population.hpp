// solver_lds_population.hpp -- the population entry of the LDS-resident solver (solver_lds.hpp): one plan solved on S
// complete states resident on the device, one workgroup per (component, member).
//
// RDIS's restarts draw a whole state and then run the decomposition on it -- fix a separator, solve the children, swap,
// repeat (optBA's sample loop, reference src/bundleadjust/optBA.cpp:198-224; sampleRandomState, src/RDISOptimizer.cpp:
// 1196-1216).  From the second half-round on, the constants of sample s are sample s's own results: the multi-start entry
// (solver_lds_starts.hpp), whose constants are the problem's x for every start, cannot serve that.  Here every member has
// its own x, X[s][N]:
//
//   per member, the population's     X[s][N]            start AND constants of member s; the result is assigned into it
//   per member, kept until fetched   xstart[s][nfree]  xout[s][nfree]  fret / delta / iters / status / nfeval / ngeval [s][ncomp]
//   per member of a launch (replica) ws[r][5 nfree]  gfac[r][ngfac]     -- as in the multi-start entry
//
// population_gather_kernel fills xstart[s] = X[s][free_vid] for all members before the first launch (what plan_set_start(plan,
// NULL) does on a problem whose x is X[s]).  blockIdx.x is the component (heaviest first), blockIdx.y the member within the
// launch: the workgroup runs LdsEnv / CgdMachine / run_machine unchanged on a ProblemView whose x is X[first + r] and a
// PlanView shifted by starts_shift -- the arithmetic, the order of every sum and so the bits of (s, c) are those of
// cgd_lds_kernel on a problem whose assigned x is X[s].  The solver touches that x in two places only: init_vectors reads
// the constants' slots from it once, and the final assignment below writes the free slots.
//
// The write-back needs no replica of x.  INVARIANT: the components of a plan are independent (plan_create checks it:
// RDIS_HIP_EOVERLAP) -- no free variable is shared, and no factor of one component reads a free variable of another.  So a
// variable that workgroup (c, s) writes into X[s] is read by no other workgroup of member s, in this launch or in another
// launch of the same call; workgroups of other members read and write other rows.  That is the argument that lets
// cgd_lds_kernel write P.x.  The gather kernel has finished before the first solver launch starts (one stream).
// No trace and no vector dump are written (starts_shift clears them).
#pragma once
#include "solver_lds.hpp"
#include "starts_api.hpp"

namespace rdis_hip {

// (instantiation list, launch bounds and dynamic LDS: cgd_lds_starts_kernel's -- a sum's tree depends on the workgroup size)
template <int THREADS, int ROT>
__global__ void __launch_bounds__(THREADS, (THREADS <= 256 ? 2 : 1))
cgd_lds_population_kernel(ProblemView P0, PlanView L0, StartsView S, double* X, int maxiters, double ftol, int ns_cap, int ncb_cap,
                          int chunk_cap) {
    extern __shared__ double lds_dyn[];
    __shared__ double red[2][3][MAX_WAVES];
    ProblemView P = P0;
    P.x = X + (S.first + (long long)blockIdx.y) * S.N;   // member first + r: its constants, and where its result goes
    const PlanView L = starts_shift(L0, S, (int)blockIdx.y);
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
    // gdmin.p with sanitisation (.cpp:61); after a rollback X already holds clamp(x_init).  Into the member's row of the
    // outputs and into the member's x (the invariant above), as cgd_lds_kernel assigns P.x
    if (!M.rolled_back) E.assign_p();
    for (int s = E.tid; s < ns; s += E.nt) {
        const int fi = SF[s];
        if (fi >= 0) { const double xv = E.X[s]; P.x[E.svid[s]] = xv; L.xout[f0 + fi] = xv; }
    }
    if (E.tid == 0) {
        L.fret[comp] = M.fret; L.delta[comp] = delta_fval(M.fret, M.finit, M.rolled_back); L.iters[comp] = M.iter;
        L.status[comp] = M.status(); L.nfeval[comp] = M.nfeval; L.ngeval[comp] = M.ngeval;
    }
}

// ---- the population's helpers: plain vector stores, grid-stride over 64-bit indices ----

// xstart[s][i] = X[s][free_vid[i]] for every member: the start rows of a population solve
__global__ void __launch_bounds__(256)
population_gather_kernel(const double* __restrict__ X, long long N, const int* __restrict__ free_vid, long long nfree, long long total,
                         double* __restrict__ xstart) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long s = i / nfree, k = i - s * nfree;
        xstart[i] = X[s * N + free_vid[k]];
    }
}

// X[first + r][vid[k]] = val[r][k], r < count, k < n (vid null: k); total = count * n
__global__ void __launch_bounds__(256)
population_scatter_kernel(double* __restrict__ X, long long N, long long first, const int* __restrict__ vid, long long n, long long total,
                          const double* __restrict__ val) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / n, k = i - r * n;
        X[(first + r) * N + (vid ? vid[k] : k)] = val[i];
    }
}

// out[r][k] = X[first + r][vid[k]]
__global__ void __launch_bounds__(256)
population_pick_kernel(const double* __restrict__ X, long long N, long long first, const int* __restrict__ vid, long long n, long long total,
                       double* __restrict__ out) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x) {
        const long long r = i / n, k = i - r * n;
        out[i] = X[(first + r) * N + (vid ? vid[k] : k)];
    }
}

// dst[r][i] = src[i] for `rows` rows of N: every member a copy of the problem's x (rows = members), or the problem's x a copy
// of one member (rows = 1, src = that member's row)
__global__ void __launch_bounds__(256)
population_copy_rows_kernel(const double* __restrict__ src, double* __restrict__ dst, long long N, long long total) {
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (long long)gridDim.x * blockDim.x)
        dst[i] = src[i % N];
}

}  // namespace rdis_hip
