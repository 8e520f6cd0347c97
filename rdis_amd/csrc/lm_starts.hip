// lm_starts.hip -- the kernels a Levenberg-Marquardt plan's multi-start solve runs around lm_batch.hip's (lm_starts.hpp): the
// scratch rows of x the starts of a launch are solved in, the selection of every component's best start, the gather of the
// winners' x into the problem's, the sum of the plan's objective and the 16 doubles of a step's summary.  Plain vector stores only; no atomics.
#include <hip/hip_runtime.h>

#include "lm_starts.hpp"

namespace rdis_hip {
namespace {

// Grid (blocks over N, starts of the launch), as population_sample_kernel: one lane per (start, variable), a wave stores 64
// consecutive doubles of a row.  pos and x are read once per row; the start's values by pos (scattered over the row's free
// entries: 8 N bytes read, 8 N written per start at most).
__global__ void __launch_bounds__(256)
k_lm_starts_fill(double* __restrict__ rows, long long N, const double* __restrict__ x, const int* __restrict__ pos, const double* __restrict__ src,
                 long long src_stride, int by_pos, long long first, long long count) {
    for (long long r = blockIdx.y; r < count; r += gridDim.y) {
        const double* __restrict__ from = src + (first + r) * src_stride;
        double* __restrict__ row = rows + r * N;
        for (long long v = (long long)blockIdx.x * blockDim.x + threadIdx.x; v < N; v += (long long)gridDim.x * blockDim.x) {
            const int k = pos[v];
            row[v] = k >= 0 ? from[by_pos ? (long long)k : v] : x[v];
        }
    }
}

// One lane per component: the scan over the starts' fret (lm_starts_best), then the winner's result row and the history
// records it wrote (at most hist_cap) into the winners' row.
__global__ void __launch_bounds__(256)
k_lm_starts_select(LmStartsOut O, long long nstarts, long long ncomp) {
    for (long long c = (long long)blockIdx.x * blockDim.x + threadIdx.x; c < ncomp; c += (long long)gridDim.x * blockDim.x) {
        const long long b = lm_starts_best(nstarts, O.res + c * O.res_doubles, O.res_ms);
        O.best[c] = (int)b;
        const double* __restrict__ from = O.res + b * O.res_ms + c * O.res_doubles;
        double* __restrict__ to = O.res + nstarts * O.res_ms + c * O.res_doubles;
        for (int i = 0; i < O.res_doubles; ++i) to[i] = from[i];
        if (O.hist_cap > 0) {
            const long long written = (long long)from[O.nhist_at];
            const long long n = 4 * (written < O.hist_cap ? written : O.hist_cap);
            const double* __restrict__ hf = O.hist + b * O.hist_ms + c * O.hist_cap * 4;
            double* __restrict__ ht = O.hist + nstarts * O.hist_ms + c * O.hist_cap * 4;
            for (long long i = 0; i < n; ++i) ht[i] = hf[i];
        }
    }
}

// One lane per entry of the free list
__global__ void __launch_bounds__(256)
k_lm_starts_gather(LmStartsOut O, long long nstarts, long long nfree, const int* __restrict__ free32, const int* __restrict__ comp_of,
                   double* __restrict__ x) {
    for (long long k = (long long)blockIdx.x * blockDim.x + threadIdx.x; k < nfree; k += (long long)gridDim.x * blockDim.x) {
        const double v = O.xout[(long long)O.best[comp_of[k]] * O.xout_ms + k];
        x[free32[k]] = v;
        O.xout[nstarts * O.xout_ms + k] = v;
    }
}

__global__ void __launch_bounds__(256)
k_lm_plan_objective(long long ncomp, const double* __restrict__ res, long long stride, double* __restrict__ out) {
    __shared__ double red[4];
    double acc = 0.0;
    for (long long c = threadIdx.x; c < ncomp; c += 256) acc += res[c * stride];
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) {
        double s = 0.0;
        for (int w = 0; w < 4; ++w) s += red[w];
        out[0] = s;
    }
}

// The plan's ordinary outputs in 16 doubles (lm_starts.hpp: LmPlanSummary): every field added in k_lm_plan_objective's order -- a
// lane's stride over the components in component order, a butterfly over the wave, the waves in wave order -- so field 0 is bit for
// bit that kernel's sum and the counts (whole numbers far below 2^53) are exact.  Lane 0 stores the block; nothing else is written.
__global__ void __launch_bounds__(256)
k_lm_plan_summary(long long ncomp, const double* __restrict__ res, long long stride, double* __restrict__ out) {
    __shared__ double red[4][LM_SUMMARY_FIELDS];
    double acc[LM_SUMMARY_FIELDS];
    for (int k = 0; k < LM_SUMMARY_FIELDS; ++k) acc[k] = 0.0;
    for (long long c = threadIdx.x; c < ncomp; c += 256) {
        const double* __restrict__ r = res + c * stride;
        const double fret = r[LM_ROW_FRET];
        acc[LM_SUMMARY_FRET] += fret;
        acc[LM_SUMMARY_DELTA] += fret - r[LM_ROW_F0];   // (delta as a fetch forms it)
        acc[LM_SUMMARY_ITERS] += r[LM_ROW_INFO + 0];
        acc[LM_SUMMARY_NFEV] += r[LM_ROW_INFO + 2];
        acc[LM_SUMMARY_NJEV] += r[LM_ROW_INFO + 3];
        acc[LM_SUMMARY_NSOLVE] += r[LM_ROW_INFO + 4];
        const int stop = (int)r[LM_ROW_INFO + 1];
        for (int k = 1; k <= 7; ++k) acc[LM_SUMMARY_STOP1 + k - 1] += stop == k ? 1.0 : 0.0;
        acc[LM_SUMMARY_NONFINITE] += (fret - fret == 0.0) ? 0.0 : 1.0;
    }
    for (int k = 0; k < LM_SUMMARY_FIELDS; ++k) {
        double a = acc[k];
        for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
        if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = a;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 0; k < LM_SUMMARY_FIELDS; ++k) {
            double s = 0.0;
            for (int w = 0; w < 4; ++w) s += red[w][k];
            out[k] = s;
        }
        for (int k = LM_SUMMARY_FIELDS; k < LM_SUMMARY_DOUBLES; ++k) out[k] = 0.0;
    }
}

// k_lm_plan_summary for every member of a population solve at once: workgroup blockIdx.x (striding beyond the grid) sums member
// m's result rows res + m * member_stride + c * stride into out + m * LM_SUMMARY_DOUBLES.  Per member the very sequence of
// additions of k_lm_plan_summary -- the lane's stride, the butterfly, the waves in wave order -- so a member's block is bit for
// bit that kernel's over the same rows.  Lane 0 stores the member's block; nothing else is written.
__global__ void __launch_bounds__(256)
k_lm_plan_summary_members(long long nmembers, long long ncomp, const double* __restrict__ res, long long member_stride, long long stride,
                          double* __restrict__ out) {
    __shared__ double red[4][LM_SUMMARY_FIELDS];
    for (long long m = blockIdx.x; m < nmembers; m += gridDim.x) {
        const double* __restrict__ rows = res + m * member_stride;
        double acc[LM_SUMMARY_FIELDS];
        for (int k = 0; k < LM_SUMMARY_FIELDS; ++k) acc[k] = 0.0;
        for (long long c = threadIdx.x; c < ncomp; c += 256) {
            const double* __restrict__ r = rows + c * stride;
            const double fret = r[LM_ROW_FRET];
            acc[LM_SUMMARY_FRET] += fret;
            acc[LM_SUMMARY_DELTA] += fret - r[LM_ROW_F0];
            acc[LM_SUMMARY_ITERS] += r[LM_ROW_INFO + 0];
            acc[LM_SUMMARY_NFEV] += r[LM_ROW_INFO + 2];
            acc[LM_SUMMARY_NJEV] += r[LM_ROW_INFO + 3];
            acc[LM_SUMMARY_NSOLVE] += r[LM_ROW_INFO + 4];
            const int stop = (int)r[LM_ROW_INFO + 1];
            for (int k = 1; k <= 7; ++k) acc[LM_SUMMARY_STOP1 + k - 1] += stop == k ? 1.0 : 0.0;
            acc[LM_SUMMARY_NONFINITE] += (fret - fret == 0.0) ? 0.0 : 1.0;
        }
        for (int k = 0; k < LM_SUMMARY_FIELDS; ++k) {
            double a = acc[k];
            for (int o = 32; o > 0; o >>= 1) a += __shfl_xor(a, o);
            if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6][k] = a;
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            double* __restrict__ to = out + m * LM_SUMMARY_DOUBLES;
            for (int k = 0; k < LM_SUMMARY_FIELDS; ++k) {
                double s = 0.0;
                for (int w = 0; w < 4; ++w) s += red[w][k];
                to[k] = s;
            }
            for (int k = LM_SUMMARY_FIELDS; k < LM_SUMMARY_DOUBLES; ++k) to[k] = 0.0;
        }
        __syncthreads();   // (red is free again before the next member of this workgroup)
    }
}

// blocks of 256 lanes over `work` items, at most `cap` (the kernels stride beyond)
unsigned blocks_for(long long work, long long cap) {
    const long long b = (work + 255) / 256;
    return (unsigned)(b < 1 ? 1 : b > cap ? cap : b);
}

}  // namespace

hipError_t lm_starts_fill_launch(hipStream_t stream, int blocks, double* rows, long long N, const double* x, const int* pos, const double* src,
                                 long long src_stride, bool by_pos, long long first, int count) {
    if (count <= 0 || N <= 0) return hipSuccess;
    if (count > 65535) return hipErrorInvalidValue;
    k_lm_starts_fill<<<dim3(blocks_for(N, blocks), (unsigned)count), 256, 0, stream>>>(rows, N, x, pos, src, src_stride, by_pos ? 1 : 0, first, count);
    return hipGetLastError();
}

hipError_t lm_starts_select_launch(hipStream_t stream, const LmStartsOut& O, long long nstarts, long long ncomp) {
    if (ncomp <= 0) return hipSuccess;
    k_lm_starts_select<<<blocks_for(ncomp, 4096), 256, 0, stream>>>(O, nstarts, ncomp);
    return hipGetLastError();
}

hipError_t lm_starts_gather_launch(hipStream_t stream, const LmStartsOut& O, long long nstarts, long long nfree, const int* free32, const int* comp_of,
                                   double* x) {
    if (nfree <= 0) return hipSuccess;
    k_lm_starts_gather<<<blocks_for(nfree, 4096), 256, 0, stream>>>(O, nstarts, nfree, free32, comp_of, x);
    return hipGetLastError();
}

hipError_t lm_plan_objective_launch(hipStream_t stream, long long ncomp, const double* res, long long stride, double* out) {
    k_lm_plan_objective<<<1, 256, 0, stream>>>(ncomp, res, stride, out);
    return hipGetLastError();
}

hipError_t lm_plan_summary_launch(hipStream_t stream, long long ncomp, const double* res, long long stride, double* out) {
    k_lm_plan_summary<<<1, 256, 0, stream>>>(ncomp, res, stride, out);
    return hipGetLastError();
}

hipError_t lm_plan_summary_members_launch(hipStream_t stream, long long nmembers, long long ncomp, const double* res, long long member_stride,
                                          long long stride, double* out) {
    if (nmembers <= 0) return hipSuccess;
    k_lm_plan_summary_members<<<(unsigned)(nmembers < 65535 ? nmembers : 65535), 256, 0, stream>>>(nmembers, ncomp, res, member_stride, stride, out);
    return hipGetLastError();
}

}  // namespace rdis_hip
