// eval_kernels.hpp -- batched factor evaluation over a factor list at the
// currently assigned x (K1 / K2 of SURVEY.md 2.1): the device side of
// OptimizableFunction::evalFactors and computeGradient(facs, pg)
// (reference src/OptimizableFunction.cpp:95-135, 234-262).
//
// HBM-bound streaming kernels: one lane per factor, grid-stride, 16-byte obs load
// + two int32 indices per factor, variable blocks gathered through L1/L2.
// Reductions are fixed-order (wave butterfly -> LDS -> per-block partial ->
// single-block final pass), so results are bit-reproducible.
#pragma once
#include "eval_sums.hpp"   // block_sum, eval_sum_of, final_sum_of: shared with the population forms (population_eval_kernels.hpp)

namespace rdis_hip {

template <int KIND>
__global__ void __launch_bounds__(256)
eval_each_kernel(ProblemView P, int nf, const int* __restrict__ fac, double* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x) {
        double f, s;
        factor_value<KIND, false>(P, nullptr, fac ? fac[i] : i, f, s);
        out[i] = f;
    }
}

// per-factor partials; BA only for the public grad_each entry point
template <int KIND>
__global__ void __launch_bounds__(256)
partials_kernel(ProblemView P, int nf, const int* __restrict__ fac, double* __restrict__ gfac) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x)
        factor_partials<KIND>(P, gfac, nullptr, fac ? fac[i] : i);
}

// rotation record of every camera block at the assigned x (one lane per camera): what the factors of
// a launch without free camera variables read instead of redoing ba_rotation per trial point
__global__ void __launch_bounds__(256)
camera_rotations_kernel(const double* __restrict__ x, const int* __restrict__ cam_blocks, int nblocks,
                        double* __restrict__ xrot) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nblocks) return;
    const int c = cam_blocks[i];
    store_rotation(x[c], x[c + 1], x[c + 2], xrot + c);
}

// a plan's copy of its listed factors' observations, in listed order (solver_lds.hpp)
__global__ void __launch_bounds__(256)
gather_obs_kernel(int n, const int* __restrict__ fac, const double2* __restrict__ obs, double2* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) out[i] = obs[fac[i]];
}

__global__ void __launch_bounds__(256)
gather_rows12_kernel(int nf, const int* __restrict__ fac, const double* __restrict__ gfac,
                     double* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf * 12; i += gridDim.x * blockDim.x) {
        const int r = i / 12, k = i - 12 * r;
        out[i] = gfac[12ll * (fac ? fac[r] : r) + k];
    }
}

// f partial per block (+ optionally the per-factor partials for the gradient)
template <int KIND, bool GRAD>
__global__ void __launch_bounds__(256)
eval_sum_kernel(ProblemView P, int nf, const int* __restrict__ fac, double* __restrict__ gfac,
                double* __restrict__ block_partial) {
    __shared__ double red[MAX_WAVES];
    const double acc = eval_sum_of<KIND, GRAD>(P, nf, fac, gfac, (int)blockIdx.x, (int)gridDim.x, red);
    if (threadIdx.x == 0) block_partial[blockIdx.x] = acc;
}

__global__ void __launch_bounds__(256)
final_sum_kernel(int n, const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double red[MAX_WAVES];
    const double acc = final_sum_of(n, partial, red);
    if (threadIdx.x == 0) out[0] = acc;
}

// g[v] = sum of the slots that feed v, in factor-list order (src/State.h:157-210).  population_gather_grad_kernel
// (population_eval_kernels.hpp) restates this loop line by line: a change to either is a change to both
__global__ void __launch_bounds__(256)
gather_grad_kernel(int nvars, const int* __restrict__ v2s_ptr, const int* __restrict__ v2s_idx,
                   const double* __restrict__ gfac, double* __restrict__ g) {
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvars; v += gridDim.x * blockDim.x) {
        const int b = v2s_ptr[v], e = v2s_ptr[v + 1];
        // sixteen slots in flight (their positions first, then the values), the additions strictly in
        // order: the bits of the plain loop without its one memory round trip per slot -- a camera's
        // run is hundreds of slots long
        double s = 0.0;
        for (int k0 = b; k0 < e; k0 += 16) {
            int id[16];
            double t[16];
#pragma unroll
            for (int j = 0; j < 16; ++j) id[j] = (k0 + j < e) ? v2s_idx[k0 + j] : 0;
#pragma unroll
            for (int j = 0; j < 16; ++j) t[j] = (k0 + j < e) ? gfac[id[j]] : 0.0;
#pragma unroll
            for (int j = 0; j < 16; ++j)
                if (k0 + j < e) s = (k0 + j == b) ? t[j] : s + t[j];
        }
        g[v] = s;
    }
}

// ---- value and gradient of a population on the short and the two-pass branch (population_entries.hip: population_grad_enqueue) ----
// These two stay in this header and are launched from rdis_hip.hip (population_partials_launch, population_eval_sum_grad_launch):
// compiled in population_kernels.hip, where the other population forms live (population_eval_kernels.hpp), their instructions come
// out in another order.
// Block (., r) is member first + r of X[members][N]: the view's x becomes the member's row, gfac replica r of the launch's
// [members of the launch][nslots] (wave-uniform: scalar registers); the statements, and so the bits, are the single-x kernels'.

// partials_kernel<KIND_BA> per member: grid (blocks, members of the launch)
__global__ void __launch_bounds__(256)
population_partials_kernel(ProblemView P, double* __restrict__ X, long long first, int nf, const int* __restrict__ fac, double* __restrict__ gfac,
                           long long nslots) {
    const long long r = blockIdx.y;
    P.x = X + (first + r) * (long long)P.N;
    gfac += r * nslots;
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += gridDim.x * blockDim.x)
        factor_partials<KIND_BA>(P, gfac, nullptr, fac ? fac[i] : i);
}

// eval_sum_kernel<KIND, true> per member: grid (nb, members of the launch), nb the block count rdis_hip_eval_grad takes for nf;
// partial: [members of the launch][nb]
template <int KIND>
__global__ void __launch_bounds__(256)
population_eval_sum_grad_kernel(ProblemView P, double* __restrict__ X, long long first, int nf, const int* __restrict__ fac, double* __restrict__ gfac,
                                long long nslots, double* __restrict__ partial) {
    __shared__ double red[MAX_WAVES];
    const long long r = blockIdx.y;
    P.x = X + (first + r) * (long long)P.N;
    const double acc = eval_sum_of<KIND, true>(P, nf, fac, gfac + r * nslots, (int)blockIdx.x, (int)gridDim.x, red);
    if (threadIdx.x == 0) partial[r * gridDim.x + blockIdx.x] = acc;
}

__global__ void scatter_x_kernel(int n, const int* __restrict__ vid, const double* __restrict__ val,
                                 double* __restrict__ x) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        x[vid ? vid[i] : i] = val[i];
}
__global__ void gather_x_kernel(int n, const int* __restrict__ vid, const double* __restrict__ x,
                                double* __restrict__ out) {
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x)
        out[i] = x[vid ? vid[i] : i];
}

__global__ void __launch_bounds__(256)
objective_sum_kernel(int ncomp, const double* __restrict__ fret, double* __restrict__ out) {
    // top-level objective = sum over components (reference src/RDISOptimizer.cpp:1491-1494)
    __shared__ double red[MAX_WAVES];
    double acc = 0.0;
    for (int i = threadIdx.x; i < ncomp; i += blockDim.x) acc += fret[i];
    acc = block_sum(acc, red);
    if (threadIdx.x == 0) out[0] = acc;
}

}  // namespace rdis_hip
