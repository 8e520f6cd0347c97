// solver_ptm_population.hpp -- the population entry of the point-major streaming solver (solver_ptm.hpp): the components of one
// plan that are too large for a compute unit's LDS, solved on S complete states resident on the device, ONE workgroup per
// (component, member) -- cgd_ptm_kernel's regime (K = 1: no cooperative launch, no residency), which a population fills: 256
// members of one large component are a workgroup per compute unit.
//
//   grid               (entries of the batch list handed over, members of the launch); blockIdx.y = r is member S.first + r
//   per member         X[s][N]: start AND constants of member s; write_back assigns the result into it (P.x[v])
//   per member, kept   xstart / xout [s][nfree], fret / delta / iters / status / nfeval / ngeval [s][ncomp]  (starts_shift)
//   per member of a launch (replica r; PtmReplicas)
//                      rec[r][6 blocks]  gh[r][6 blocks]  bex[r][6 blocks]  cbox[r][8 chunks]   PlanView::pm_rec / pm_gh / pm_bex /
//                      pm_cbox of the replica, laid out like the plan's own (a component's blocks at pm_pt0, its chunks at pm_ch0)
//
// The workgroup builds a ProblemView whose x is the member's row and a PlanView of the member (starts_shift) whose four arrays
// are the replica's, and runs ptm_env / init_vectors / run_machine / write_back unchanged: the arithmetic, the order of every sum
// and so the bits of (s, c) are those of cgd_ptm_kernel<THREADS, ROT> on a problem whose assigned x is X[s].
//
// What the solver writes to global memory with one workgroup a component (GROUP = LOCAL = false), read off solver_ptm.hpp:
//   PT = pm_rec    init_vectors, gradient_fused (finish_block), point_pass (cg_start, cg_update, line_end)
//   PG = pm_gh     init_vectors, point_pass
//   PE = pm_bex    init_vectors
//   CBX = pm_cbox  init_vectors
//   P.x, L.xout    write_back;  fret ... ngeval: the kernel's last statement
// and nothing else: trace and vdump are null (starts_shift), the exchange buffers and GridSync state belong to GROUP, the timing
// counters to -DRDIS_COOP_TIMING builds of cgd_ptm_kernel (not written here).  It reads P.x in init_vectors only (the constants)
// and no global xrot: the cameras' records are formed in LDS in every rotation mode.
//
// INVARIANT of the replicas: a replica serves another member in the next launch of the call, and is never cleared.  That is
// sound because init_vectors writes, before anything reads them, every entry of the four arrays the solve reads: for every point
// block ps < npb of the component (my_points covers every chunk c < npc, every lane with 64 c + lane < npb) all six planes of PT
// and of PG and the six bounds of PE; for every chunk c < npc entries 0..2 and 4..6 of its box.  The readers stay inside that:
// load_recs reads block min(64 c + lane, npb - 1) -- in the last, ragged chunk the lanes beyond npb read the component's last
// block -- and box entries k, 4 + k (k < 3) of a chunk c < npc (a row of nothing names chunk 0); clamp_exact, point_start,
// point_pass and finish_block take blocks < npb only.  Entries 3 and 7 of a box are neither written nor read.
//
// The write-back needs no replica of x: the components of a plan are independent (RDIS_HIP_EOVERLAP, the invariant of
// solver_lds_population.hpp), so what workgroup (c, s) writes into X[s] no other workgroup of member s reads, in this kernel, in
// the tiny-component launch before it or in the LDS-resident one behind it.  The problem's own x, the plan's start, its ordinary
// outputs and its own pm_* arrays are not touched.
#pragma once
#include "solver_ptm.hpp"
#include "population_api.hpp"

namespace rdis_hip {

// (instantiation list, launch bounds, dynamic LDS and the PAIR rule: cgd_ptm_kernel's -- a sum's tree depends on the workgroup
// size, the gradient's rounds on PAIR)
template <int THREADS, int ROT>
__global__ void __launch_bounds__(THREADS, (THREADS <= 256 ? 2 : 1))
cgd_ptm_population_kernel(ProblemView P0, PlanView L0, StartsView S, PtmReplicas RP, double* X, int maxiters, double ftol, int ncb_cap) {
    extern __shared__ __attribute__((aligned(16))) double lds_dyn[];
    __shared__ double red[2][3][MAX_WAVES];
    const int r = (int)blockIdx.y;
    ProblemView P = P0;
    P.x = X + (S.first + (long long)r) * S.N;   // member first + r: its constants, and where its result goes
    PlanView L = starts_shift(L0, S, r);
    L.pm_rec = RP.rec + (long long)r * PT_REC * RP.blocks;
    L.pm_gh = RP.gh + (long long)r * PT_REC * RP.blocks;
    L.pm_bex = RP.bex + (long long)r * PT_BND * RP.blocks;
    L.pm_cbox = RP.cbox + (long long)r * 8 * RP.chunks;
    const int comp = L.order[blockIdx.x];
    const int f0 = L.free_ptr[comp], n = L.free_ptr[comp + 1] - f0;
    if (L.fac_ptr[comp + 1] == L.fac_ptr[comp]) {  // nothing to optimise (no slot table): return 0, the member's x untouched -- as cgd_lds_population_kernel does
        for (int i = threadIdx.x; i < n; i += blockDim.x) L.xout[f0 + i] = L.xstart[f0 + i];
        if (threadIdx.x == 0) {
            L.fret[comp] = 0.0; L.delta[comp] = 0.0; L.iters[comp] = 0;
            L.status[comp] = EXIT_EMPTY; L.nfeval[comp] = 0; L.ngeval[comp] = 0;
        }
        return;
    }
    constexpr bool PAIR = THREADS <= PTM_PAIR_MAX_THREADS;
    PtmEnv<ROT, false, SmallCoopState, false, PAIR> E = ptm_env<ROT, false, SmallCoopState, false, PAIR>(P, L, comp, lds_dyn, red, ncb_cap, 0, 1, (SmallCoopState*)nullptr, nullptr, 0, nullptr);
    __shared__ CgdMachine M;
    __shared__ Request Q[2];
    E.init_vectors();
    run_machine(E, M, Q, maxiters, ftol);
    E.write_back(M.rolled_back);
    if (E.tid == 0) {
        L.fret[comp] = M.fret; L.delta[comp] = delta_fval(M.fret, M.finit, M.rolled_back); L.iters[comp] = M.iter;
        L.status[comp] = M.status(); L.nfeval[comp] = M.nfeval; L.ngeval[comp] = M.ngeval;
    }
}

}  // namespace rdis_hip
