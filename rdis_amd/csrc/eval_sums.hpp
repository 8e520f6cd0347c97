// eval_sums.hpp -- the fixed-order sums of the batched evaluation as device functions, no kernel: what eval_kernels.hpp's
// single-x kernels (rdis_hip.hip) and their population forms (population_eval_kernels.hpp: population_kernels.hip) both call,
// so a value has the same bits on either side.
#pragma once
#include "solver_wg.hpp"

namespace rdis_hip {

__device__ __forceinline__ double block_sum(double v, double* red /* [MAX_WAVES] */) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double r = 0.0;
    for (int i = 0; i < (int)(blockDim.x >> 6); ++i) r += red[i];
    __syncthreads();
    return r;
}

// a block's share of the listed factors (block bx of nb, grid-stride), added per lane in list order and then over the block:
// the one definition of eval_sum_kernel's sum and of its population form's
template <int KIND, bool GRAD>
__device__ __forceinline__ double eval_sum_of(const ProblemView& P, int nf, const int* __restrict__ fac, double* __restrict__ gfac, int bx, int nb,
                                              double* red /* [MAX_WAVES] */) {
    double acc = 0.0;
    for (int i = bx * blockDim.x + threadIdx.x; i < nf; i += nb * blockDim.x) {
        const int fid = fac ? fac[i] : i;
        double f, s;
        factor_value<KIND, false>(P, nullptr, fid, f, s);
        acc += f;
        if constexpr (GRAD) factor_partials<KIND>(P, gfac, nullptr, fid);
    }
    return block_sum(acc, red);
}

// partial[0 .. n) added by one workgroup: the one definition of final_sum_kernel's sum and of its population form's
__device__ __forceinline__ double final_sum_of(int n, const double* __restrict__ partial, double* red /* [MAX_WAVES] */) {
    double acc = 0.0;
    // (eight loads in flight, added in index order: the bits of the plain loop without its round trip per element)
    for (int i0 = threadIdx.x; i0 < n; i0 += 8 * blockDim.x) {
        double t[8];
#pragma unroll
        for (int j = 0; j < 8; ++j) t[j] = (i0 + j * (int)blockDim.x < n) ? partial[i0 + j * (int)blockDim.x] : 0.0;
#pragma unroll
        for (int j = 0; j < 8; ++j)
            if (i0 + j * (int)blockDim.x < n) acc += t[j];
    }
    return block_sum(acc, red);
}

}  // namespace rdis_hip
