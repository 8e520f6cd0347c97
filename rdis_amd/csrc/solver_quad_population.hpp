// solver_quad_population.hpp -- the population entry of the tiny-component solver (solver_quad.hpp): the tiny components of
// one plan solved on S complete states resident on the device, a few lanes per (component, member), persistent groups.
//
// With the cameras assigned every point is a component of its own, and a population has S x ntiny of them.  The LDS-resident
// entry (solver_lds_population.hpp) gives each a workgroup of 64 lanes, 60 of them idle; here a block belongs to ONE member
// and its groups of G lanes walk that member's components as cgd_group_kernel's walk the problem's:
//
//   grid               (blocks per member, members of the launch); blockIdx.y = r is member S.first + r
//   per member         X[s][N]: start AND constants of member s; GroupEnv::next_problem assigns the result into it (P.x[fv])
//   per member, kept   xstart / xout [s][nfree], fret / delta / iters / status / nfeval / ngeval [s][ncomp]  (starts_shift)
//   per member of a launch (replica r)
//                      queues[r]   the member's own queue counter: a block takes its first components by position within
//                                  the member's blocks and every later one with atomicAdd, so no residency is needed
//                      XR[r][N]    rotation records of the member's cameras, indexed like the problem's xrot (xrot + c);
//                                  only when the launch reads records (rest_rot_mode == ROT_CAMFIX), else null
//
// The block builds a ProblemView (x, xrot) and a PlanView (starts_shift) of its member and runs GroupEnv<G>, CgdMachine and
// run_machine unchanged: every group of a block belongs to one member, so the shifted pointers are wave-uniform, and the
// arithmetic, the order of every sum and so the bits of (s, c) are those of cgd_group_kernel<G, THREADS> on a problem whose
// assigned x is X[s].  G must be the plan's tiny_group: the bits depend on it.
//
// The write-back needs no replica of x: the components of a plan are independent (RDIS_HIP_EOVERLAP, the invariant of
// solver_lds_population.hpp), so what a group writes into X[s] no other group of member s reads, in this kernel or in the
// LDS-resident one that follows it in a mixed plan.
//
// INVARIANT of the records: XR[r] must hold the records of member S.first + r when the launch starts.  A replica is reused by
// the next launch of the call for another member, so population_rotations_kernel runs before EVERY launch, not once per call.
// The problem's own xrot is neither read nor written.  No trace and no vector dump are written (starts_shift clears them).
#pragma once
#include "solver_quad.hpp"
#include "starts_api.hpp"

namespace rdis_hip {

// (instantiations and launch bounds: cgd_group_kernel's -- <4, QUAD_THREADS> and <16, 64>)
template <int G, int THREADS>
__global__ void __launch_bounds__(THREADS, G == 4 ? 1 : 2)
cgd_group_population_kernel(ProblemView P0, PlanView L0, StartsView S, double* X, double* XR, const int* __restrict__ list, int ncomp,
                            int* __restrict__ queues, int maxiters, double ftol) {
    __shared__ CgdMachine Ms[THREADS / G];
    __shared__ Request Qs[THREADS / G][2];
    const int r = (int)blockIdx.y;
    ProblemView P = P0;
    P.x = X + (S.first + (long long)r) * S.N;      // member first + r: its constants, and where its results go
    if (XR != nullptr) P.xrot = XR + (long long)r * S.N;
    const PlanView L = starts_shift(L0, S, r);
    const int grp = threadIdx.x / G;
    GroupEnv<G> E{P, L, 0, 0, 0, 0, 0, (int)(threadIdx.x % G), false,
                  {}, {}, {}, {}, {}, {}, {}, {}, {},
                  nullptr, 0, 0, list, ncomp, queues + r, (int)(gridDim.x * (THREADS / G))};
    E.active = E.load_next((int)blockIdx.x * (THREADS / G) + grp);   // the first component: by position among the member's blocks
    if (E.active) run_machine(E, Ms[grp], Qs[grp], maxiters, ftol);
}

// XR[r][c ..] = the rotation record of camera block c at X[first + r], for every member of the launch: camera_rotations_kernel's
// statement on the member's row (the same bits).  Grid (ceil(nblocks / 256), members of the launch).
__global__ void __launch_bounds__(256)
population_rotations_kernel(const double* __restrict__ X, long long N, long long first, const int* __restrict__ cam_blocks, int nblocks,
                            double* __restrict__ XR) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    const double* x = X + (first + (long long)blockIdx.y) * N;
    double* xrot = XR + (long long)blockIdx.y * N;
    const int c = cam_blocks[i];
    store_rotation(x[c], x[c + 1], x[c + 2], xrot + c);
}

}  // namespace rdis_hip
