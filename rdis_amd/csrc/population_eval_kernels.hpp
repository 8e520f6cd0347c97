// population_eval_kernels.hpp -- the kernels of a population's evaluation, argmin, gradient and gradient maximum, the member a
// grid dimension.  They are the population forms of eval_kernels.hpp's single-x kernels and share their sums (eval_sums.hpp).
// Non-template __global__ functions: seen by population_kernels.hip alone, launched through population_api.hpp's *_launch
// functions (population_entries.hip: population_eval_enqueue, population_select, population_grad_enqueue).
#pragma once
#include "eval_sums.hpp"
#include "population_api.hpp"      // MemberValue
#include "population_select.hpp"   // better()

namespace rdis_hip {

// ---- the evaluation of a population, the member a grid dimension (population_entries.hip: population_eval_enqueue) ----
// Block (., r) is member first + r of X[members][N]: the view's x becomes the member's row (wave-uniform: scalar registers), the
// statement and so the bits are those of the single-x kernel (eval_kernels.hpp).  partial: [members of the launch][nb], the population's own.

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
// order on (value, index) pairs, shared with the population's ranking -- one definition; MemberValue: population_api.hpp)
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

// ---- value and gradient of a population on the short and the two-pass branch (population_entries.hip: population_grad_enqueue) ----
// gfac is replica r of the launch's [members of the launch][nslots].  population_partials_kernel and population_eval_sum_grad_kernel
// are eval_kernels.hpp's: compiled in this unit their instructions come out in another order than in rdis_hip.hip.

// gather_grad_kernel (eval_kernels.hpp) per member: grid (blocks, members of the launch); the gather lists are the members' common
// ones, member first + r's row of the result is G[row0 + r].  The loop is gather_grad_kernel's, RESTATED line by line (moving it into a
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

}  // namespace rdis_hip
