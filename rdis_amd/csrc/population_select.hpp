// population_select.hpp -- what a restart loop does to a population between two solves, on the device: draw members
// (population_sample_kernel), put the members into the order of their last evaluation (population_rank_kernel,
// population_permute_rows_kernel).  The two rules -- the draw and the order -- are plain functions for the host and the device
// (tests/cpp/population_select_test.cpp runs them without a device); the kernels are seen by the HIP compiler only.
//
//   draw   HipRDISLevelOptimizer::restartValue (rdis_amd/host/rdis_levels.cpp; oracle/levels.py: splitmix_restart_value) with
//          node = stream and restart = the member's absolute row, bit for bit: splitmix64 of (seed, stream, member, variable),
//          uniform over the sampling interval, VariableDomain::closestVal into the domain.  A value depends on those four only.
//   order  better(): numbers ascending, a tie (-0.0 against +0.0 is one) by lower index, NaNs last by index -- the argmin rule of
//          eval_kernels.hpp as a strict total order, so "how many members are better than s" is a permutation of 0 .. S-1.
#pragma once
#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define RDIS_SELECT_FN __host__ __device__ __forceinline__
#else
#define RDIS_SELECT_FN inline
#endif

namespace rdis_hip {

// The member a population keeps, the minimum of f[members]: select_best_start_kernel's rule (solver_lds_starts.hpp), which as a
// sequential scan reads  b = 0; for s >= 1: if (f[s] < f[b] || (f[b] != f[b] && f[s] == f[s])) b = s  -- the lowest value, on a
// tie (-0.0 against +0.0 is one) the lowest index, a NaN never unless every value is one: then member 0.  better() is that rule as
// a strict total order on (value, index) pairs with distinct indices, so the winner is the same whatever the reduction's shape.
RDIS_SELECT_FN bool better(double fa, long long sa, double fb, long long sb) {
    const bool na = fa != fa, nb = fb != fb;
    if (na != nb) return nb;              // a number beats a NaN
    if (!na && fa != fb) return fa < fb;  // two different numbers: the lower
    return sa < sb;                       // a tie, or two NaNs: the lower index
}

// the part of the draw's key that a row shares: seed, stream (restartValue's node) and the member's absolute row (its restart)
RDIS_SELECT_FN unsigned long long sample_member_key(unsigned long long seed, long long stream, long long member) {
    return seed + 0x9E3779B97F4A7C15ull * (unsigned long long)(stream + 1) + 0xBF58476D1CE4E5B9ull * (unsigned long long)(member + 1);
}

// restartValue for variable v of that row: sampling interval [slo, shi], domain [lo, hi]
RDIS_SELECT_FN double sample_value(unsigned long long member_key, long long v, double slo, double shi, double lo, double hi) {
    unsigned long long z = member_key + 0x94D049BB133111EBull * (unsigned long long)(v + 1);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    const double u = (double)(z >> 11) * (1.0 / 9007199254740992.0);
    // the host adds a ROUNDED product (x86-64 without contraction); the device compiler would fuse the two into one FMA -- also
    // through __dadd_rn(slo, __dmul_rn(u, w)), which are a plain + and * to it -- and that is another double in about half of all
    // draws: contraction is switched off for this statement
    const double w = shi - slo;
    double val;
    {
#if defined(__clang__)
#pragma clang fp contract(off)
        const double prod = u * w;
#else
        volatile double prod = u * w;   // (a store between the two: no compiler fuses them)
#endif
        val = slo + prod;
    }
    if (lo <= val && val <= hi) return val;   // VariableDomain::closestVal
    return val < lo ? lo : hi;
}

// rank by counting, as the kernel does it and as the host test restates it: the members better than s
RDIS_SELECT_FN long long rank_of(long long members, const double* f, long long s) {
    long long r = 0;
    const double fs = f[s];
    for (long long t = 0; t < members; ++t) r += better(f[t], t, fs, s) ? 1 : 0;
    return r;
}

// (the kernels are defined once: in the translation unit that launches them, population_kernels.hip -- eval_kernels.hpp
// includes this header for better() alone)
#if defined(__HIPCC__) && defined(RDIS_POPULATION_SELECT_KERNELS)

// X[first + r][vid[k]] = the draw of (seed, stream, first + r, vid[k]), r < count, k < n (vid null: k).  Grid (blocks over n,
// members): one lane per (member, variable), the member's key formed once per row (blockIdx.y is wave-uniform); with vid null a
// wave stores 64 consecutive doubles.  slo / shi: the population's sampling intervals, lo / hi: the problem's domains, all [N].
__global__ void __launch_bounds__(256)
population_sample_kernel(double* __restrict__ X, long long N, long long first, long long count, const int* __restrict__ vid, long long n,
                         unsigned long long seed, long long stream, const double* __restrict__ slo, const double* __restrict__ shi,
                         const double* __restrict__ lo, const double* __restrict__ hi) {
    for (long long r = blockIdx.y; r < count; r += gridDim.y) {
        const long long s = first + r;
        const unsigned long long key = sample_member_key(seed, stream, s);
        double* __restrict__ row = X + s * N;
        for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += (long long)gridDim.x * blockDim.x) {
            const long long v = vid ? vid[k] : k;
            row[v] = sample_value(key, v, slo[v], shi[v], lo[v], hi[v]);
        }
    }
}

// order[rank] = s for every member s, rank = the number of members better than s.  256 lanes, a member each; f passes through
// LDS in tiles of 256 values, and in the inner loop every lane reads the same LDS address (a broadcast: no bank conflict).
// better() is a strict total order, so the ranks are a permutation of 0 .. members-1 and no two lanes store to one place.
__global__ void __launch_bounds__(256)
population_rank_kernel(long long members, const double* __restrict__ f, long long* __restrict__ order) {
    __shared__ double tile[256];
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    const bool live = s < members;
    const double fs = live ? f[s] : 0.0;
    long long rank = 0;
    for (long long t0 = 0; t0 < members; t0 += 256) {
        const long long t = t0 + threadIdx.x;
        tile[threadIdx.x] = t < members ? f[t] : 0.0;
        __syncthreads();
        const int nt = (int)(members - t0 < 256 ? members - t0 : 256);
        for (int j = 0; j < nt; ++j) rank += better(tile[j], t0 + j, fs, s) ? 1 : 0;
        __syncthreads();
    }
    if (live) order[rank] = s;
}

// X2[r][i] = X[order[r]][i] and f2[r] = f[order[r]]: grid (blocks over N, members), order[r] read once per workgroup, 8-byte
// copies (a row starts 16-byte aligned only when N is even).  HBM-bound: 16 N bytes a member.
__global__ void __launch_bounds__(256)
population_permute_rows_kernel(long long members, long long N, const long long* __restrict__ order, const double* __restrict__ X,
                               const double* __restrict__ f, double* __restrict__ X2, double* __restrict__ f2) {
    for (long long r = blockIdx.y; r < members; r += gridDim.y) {
        const long long src = order[r];
        const double* __restrict__ from = X + src * N;
        double* __restrict__ to = X2 + r * N;
        for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < N; i += (long long)gridDim.x * blockDim.x) to[i] = from[i];
        if (blockIdx.x == 0 && threadIdx.x == 0) f2[r] = f[src];
    }
}

#endif  // RDIS_POPULATION_SELECT_KERNELS

}  // namespace rdis_hip
