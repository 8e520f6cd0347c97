// solver_coop_population.hpp -- the population entry of the cooperative solver (solver_coop.hpp, the plain layout): the
// components of one plan that run as cooperative groups, solved on S complete states resident on the device, a group per
// (component, member), side by side in ONE cooperative launch.
//
//   grid               (total_wg of the launch's groups, members of the launch); blockIdx.y = r is member S.first + r;
//                      workgroup blockIdx.x belongs to group groups[wg_group[blockIdx.x]], as in cgd_coop_kernel
//   per member         X[s][N]: start AND constants of member s; write_back assigns the result into it (P.x[v])
//   per member, kept   xstart / xout [s][nfree], fret / delta / iters / status / nfeval / ngeval [s][ncomp]  (starts_shift)
//   per member of a launch (replica r; CoopReplicas, replica_layout.hpp: population_coop_layout)
//                      gfac[r][ngfac]    PlanView::gfac of the replica (S.gfac: starts_shift)
//                      xi[r][xi_doubles] the groups' published directions, each at its offset in the plan's xi_glob
//                      st[r][groups]     one CoopState per (member, group of the launch)
//
// The workgroup builds a ProblemView whose x is the member's row, a PlanView of the member (starts_shift) and the group's
// CoopArgs with xi_glob and st replaced by the replica's, and calls coop_solve<THREADS> unchanged: CoopEnv, GridSync and the
// minimizer are those of cgd_coop_kernel, so the arithmetic, the order of every sum and the bits of (s, c) are those of
// cgd_coop_kernel<THREADS> on a problem whose assigned x is X[s].  Nothing in coop_solve looks at gridDim or blockIdx: a
// group knows its size and a workgroup its rank from the arguments, and groups never talk to each other -- the groups of two
// members no more than two groups of one launch of cgd_coop_kernel.
//
// What coop_solve writes to global memory, read off solver_coop.hpp:
//   L.gfac          gradient_to_xi (scatter_partials belongs to factor_rounding = 1, refused on a population)
//   A.xi_glob       publish_xi (cg_start, cg_update)
//   A.st            the granules and the abort word, through GridSync
//   P.x, L.xout     write_back;  fret ... ngeval: the kernel's last statements
// and nothing else here: A.timing and A.objective are null, trace and vdump are null (starts_shift; both options are refused),
// seq_val and seq_ab belong to factor_rounding = 1.  It reads P.x in load_base only (the constants of a factor lane).
//
// INVARIANT of the replicas: a replica serves another member in the next launch of the call, and is never cleared.  That is
// sound because
//   * the granules and the abort word are armed before EVERY launch (coop_population_arm_kernel, for every (member, group) of it);
//   * gfac: gradient_to_xi stores, before the barrier behind which anything reads, the partial of every factor slot of the
//     component that feeds a free variable (slot_pos >= 0), and the owners read the runs [v2s_ptr[i], v2s_ptr[i + 1]) of the
//     component's free variables, which consist of exactly those slots;
//   * xi: every free variable of a component has one owner, a lane or a wave (coop_owner_tables), and publish_xi stores the
//     entry of every owned variable before its barrier; line_begin, the only reader, runs behind a cg_start or a cg_update of
//     the same request (minimizer.hpp: start_line), so it reads what this solve published -- entry 0, which a constant slot
//     loads and throws away, included (a component has a free variable).
// A member that ends in NaN leaves NaN in its replica; the next member overwrites every entry before it reads one.
//
// The write-back needs no replica of x: the components of a plan are independent (RDIS_HIP_EOVERLAP, the invariant of
// solver_lds_population.hpp), so what the group (c, s) writes into X[s] no other group of member s reads, in this launch or in
// the launches of the other solvers around it.  The problem's own x and exchange state, the plan's start, its ordinary
// outputs, its gfac and its xi_glob are not touched.
#pragma once
#include "solver_coop.hpp"
#include "starts_api.hpp"   // StartsView, CoopReplicas, starts_shift

namespace rdis_hip {

template <int THREADS>
__global__ void __launch_bounds__(THREADS)
cgd_coop_population_kernel(ProblemView P0, PlanView L0, StartsView S, CoopReplicas RC, double* X, const CoopGroup* __restrict__ groups,
                           const int* __restrict__ wg_group, int maxiters, double ftol) {
    const int r = (int)blockIdx.y;
    const int gi = wg_group[blockIdx.x];
    const CoopGroup G = groups[gi];
    ProblemView P = P0;
    P.x = X + (S.first + (long long)r) * S.N;   // member first + r: its constants, and where its result goes
    const PlanView L = starts_shift(L0, S, r);
    CoopArgs A = G.a;
    // (null, and an argument rather than the constant: with `nullptr` written here hipcc's gfx950 backend stops on the
    // reference-rounding instantiation with "Illegal instruction detected: Operand has incorrect register class")
    A.timing = RC.timing;
    A.objective = nullptr;
    A.xi_glob = RC.xi + (long long)r * RC.xi_doubles + (G.a.xi_glob - RC.xi_plan);   // the group's offset in the plan's xi_glob
    A.st = RC.st + ((long long)r * RC.groups + gi);
    coop_solve<THREADS>(P, L, A, G.nwg, (int)blockIdx.x - G.wg0, maxiters, ftol);
}

// arms the granules of every (member, group) of a launch: grid (groups, members)
__global__ void __launch_bounds__(256) coop_population_arm_kernel(const CoopGroup* __restrict__ groups, int waves_per_wg, CoopReplicas RC) {
    const CoopGroup G = groups[blockIdx.x];
    CoopState* st = RC.st + ((long long)blockIdx.y * RC.groups + blockIdx.x);
    const int entries = G.nwg * waves_per_wg;
    for (int t = threadIdx.x; t < COOP_NBUF * COOP_KP * entries; t += blockDim.x) {
        const int k = t % COOP_KP, e = (t / COOP_KP) % entries, b = t / (COOP_KP * entries);
        st->granule[b][e][k] = ~0ull;
    }
    if (threadIdx.x == 0) st->abort_flag = 0u;
}

inline const void* coop_population_kernel_fn(int threads) {
    return with_threads<512, 128, 256>(threads, [](auto T) { return (const void*)cgd_coop_population_kernel<T.value>; });
}

// returns hipSuccess (0) or a hipError_t.  groups / wg_group: the device arrays of the plan's CoopLaunch; RC.groups >= ngroups
inline int launch_coop_population(hipStream_t stream, int kind, const ProblemView& P, const PlanView& V, const StartsView& S, const CoopReplicas& RC,
                                  double* X, const CoopGroup* groups, const int* wg_group, int ngroups, int total_wg, int members_of_launch,
                                  int threads, int maxiters, double ftol) {
    if (kind != KIND_BA) return (int)hipErrorNotSupported;
    coop_population_arm_kernel<<<dim3((unsigned)ngroups, (unsigned)members_of_launch), 256, 0, stream>>>(groups, threads / 64, RC);
    hipError_t e0 = hipGetLastError();
    if (e0 != hipSuccess) return (int)e0;
    ProblemView p = P;
    PlanView v = V;
    StartsView s = S;
    CoopReplicas rc = RC;
    double* x = X;
    const CoopGroup* gp = groups;
    const int* wp = wg_group;
    int mi = maxiters;
    double ft = ftol;
    void* args[] = {&p, &v, &s, &rc, &x, &gp, &wp, &mi, &ft};
    return (int)hipLaunchCooperativeKernel(coop_population_kernel_fn(threads), dim3((unsigned)total_wg, (unsigned)members_of_launch), dim3(threads),
                                           args, 0, stream);
}

// resident workgroups of a launch of THIS kernel, over all its members: coop_max_workgroups' rule on its own occupancy (the
// wrapper holds a member's views in registers of its own: the old kernel's number says nothing about this one)
inline int coop_population_max_workgroups(int threads, int num_cus) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, coop_population_kernel_fn(threads), threads, 0) != hipSuccess) return 0;
    // stay one block per CU below what the API reports when it reports more than one (coop_max_workgroups)
    if (per_cu > 1) per_cu -= 1;
    const long long cap = (long long)per_cu * num_cus;
    return (int)(cap > COOP_MAX_WG ? COOP_MAX_WG : cap);
}

}  // namespace rdis_hip
