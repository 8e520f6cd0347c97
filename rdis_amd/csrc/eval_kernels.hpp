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
#include "solver_wg.hpp"
#include "population_select.hpp"

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

// f partial per block (+ optionally the per-factor partials for the gradient)
template <int KIND, bool GRAD>
__global__ void __launch_bounds__(256)
eval_sum_kernel(ProblemView P, int nf, const int* __restrict__ fac, double* __restrict__ gfac,
                double* __restrict__ block_partial) {
    __shared__ double red[MAX_WAVES];
    const double acc = eval_sum_of<KIND, GRAD>(P, nf, fac, gfac, (int)blockIdx.x, (int)gridDim.x, red);
    if (threadIdx.x == 0) block_partial[blockIdx.x] = acc;
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

__global__ void __launch_bounds__(256)
final_sum_kernel(int n, const double* __restrict__ partial, double* __restrict__ out) {
    __shared__ double red[MAX_WAVES];
    const double acc = final_sum_of(n, partial, red);
    if (threadIdx.x == 0) out[0] = acc;
}

// ---- the evaluation of a population, the member a grid dimension (rdis_hip.hip: population_eval_enqueue) ----
// Block (., r) is member first + r of X[members][N]: the view's x becomes the member's row (wave-uniform: scalar registers), the
// statement and so the bits are those of the single-x kernel above.  partial: [members of the launch][nb], the population's own.

// eval_sum_kernel<KIND, false> per member: grid (nb, members of the launch), nb the block count rdis_hip_eval takes for nf
template <int KIND>
__global__ void __launch_bounds__(256)
population_eval_sum_kernel(ProblemView P, double* __restrict__ X, long long first, int nf, const int* __restrict__ fac,
                           double* __restrict__ partial) {
    __shared__ double red[MAX_WAVES];
    const long long r = blockIdx.y;
    P.x = X + (first + r) * (long long)P.N;
    const double acc = eval_sum_of<KIND, false>(P, nf, fac, nullptr, (int)blockIdx.x, (int)gridDim.x, red);
    if (threadIdx.x == 0) partial[r * gridDim.x + blockIdx.x] = acc;
}

// final_sum_kernel per member: grid (members of the launch), f[first + r] = the sum of partial[r][0 .. n)
__global__ void __launch_bounds__(256)
population_final_sum_kernel(int n, const double* __restrict__ partial, long long first, double* __restrict__ f) {
    __shared__ double red[MAX_WAVES];
    const long long r = blockIdx.x;
    const double acc = final_sum_of(n, partial + r * n, red);
    if (threadIdx.x == 0) f[first + r] = acc;
}

// The member a population keeps, the minimum of f[members], by better() (population_select.hpp: the argmin rule as a strict total
// order on (value, index) pairs, shared with the population's ranking -- one definition)
struct MemberValue { double f; long long s; };
// one workgroup of 256 lanes; lanes stride over the members, then wave shuffles, then the waves' winners through LDS
__global__ void __launch_bounds__(256)
population_argmin_kernel(long long members, const double* __restrict__ f, MemberValue* __restrict__ best) {
    __shared__ double wf[MAX_WAVES];
    __shared__ long long ws[MAX_WAVES];
    double bf = __builtin_nan("");
    long long bs = INT64_MAX;             // (no member yet: loses against every member, NaN or not)
    for (long long s = threadIdx.x; s < members; s += blockDim.x) {
        const double v = f[s];
        if (better(v, s, bf, bs)) { bf = v; bs = s; }
    }
    for (int m = 1; m < 64; m <<= 1) {
        const double of = __shfl_xor(bf, m, 64);
        const long long os = __shfl_xor(bs, m, 64);
        if (better(of, os, bf, bs)) { bf = of; bs = os; }
    }
    if ((threadIdx.x & 63) == 0) { wf[threadIdx.x >> 6] = bf; ws[threadIdx.x >> 6] = bs; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w)
            if (better(wf[w], ws[w], bf, bs)) { bf = wf[w]; bs = ws[w]; }
        best->f = bf; best->s = bs;
    }
}

// x[0 .. N) = X[best->s][0 .. N): the member's index read on the device (grid-stride, plain stores)
__global__ void __launch_bounds__(256)
population_copy_best_kernel(const double* __restrict__ X, long long N, const MemberValue* __restrict__ best, double* __restrict__ x) {
    const double* row = X + best->s * N;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) x[i] = row[i];
}

// g[v] = sum of the slots that feed v, in factor-list order (src/State.h:157-210)
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

// ---- value and gradient of a population on the short and the two-pass branch (rdis_hip.hip: population_grad_enqueue) ----
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

// gather_grad_kernel per member: grid (blocks, members of the launch); the gather lists are the members' common ones, member
// first + r's row of the result is G[row0 + r].  The loop is gather_grad_kernel's, RESTATED line by line (moving it into a
// function the two kernels share changes that kernel's registers: 58 scalar / 44 vector become 57 / 45): the slots' positions,
// their values, the additions strictly in order -- a change to either loop is a change to both.
__global__ void __launch_bounds__(256)
population_gather_grad_kernel(int nvars, const int* __restrict__ v2s_ptr, const int* __restrict__ v2s_idx, const double* __restrict__ gfac, long long nslots,
                              double* __restrict__ G, long long row0) {
    const long long r = blockIdx.y;
    gfac += r * nslots;
    double* __restrict__ g = G + (row0 + r) * (long long)nvars;
    for (int v = blockIdx.x * blockDim.x + threadIdx.x; v < nvars; v += gridDim.x * blockDim.x) {
        const int b = v2s_ptr[v], e = v2s_ptr[v + 1];
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

// gmax[k] = max_i |G[k][i]|, NaN if any entry of the row is one: one workgroup per row, lanes stride over the row.  A maximum
// is exact, so no bit depends on the shape of the reduction.
__global__ void __launch_bounds__(256)
population_grad_max_kernel(long long N, const double* __restrict__ G, double* __restrict__ gmax) {
    __shared__ double wm[MAX_WAVES];
    __shared__ int wn[MAX_WAVES];
    const double* row = G + (long long)blockIdx.x * N;
    double m = 0.0;
    int isnan_ = 0;
    for (long long i = threadIdx.x; i < N; i += blockDim.x) {
        const double a = __builtin_fabs(row[i]);
        if (a != a) isnan_ = 1; else m = a > m ? a : m;
    }
    for (int k = 1; k < 64; k <<= 1) {
        const double om = __shfl_xor(m, k, 64);
        isnan_ |= __shfl_xor(isnan_, k, 64);
        m = om > m ? om : m;
    }
    if ((threadIdx.x & 63) == 0) { wm[threadIdx.x >> 6] = m; wn[threadIdx.x >> 6] = isnan_; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < (int)(blockDim.x >> 6); ++w) { m = wm[w] > m ? wm[w] : m; isnan_ |= wn[w]; }
        gmax[blockIdx.x] = isnan_ ? __builtin_nan("") : m;
    }
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
