// lm_starts.hpp -- interface of lm_starts.hip: what a Levenberg-Marquardt plan's multi-start solve
// (rdis_hip_lm_plan_solve_starts, rdis_hip_lm_plan_solve_starts_population) runs around lm_batch.hip's kernel, which it does not
// touch.  Every start of a launch gets a scratch row of x (the plan's free variables from the start, every other variable the
// problem's x); the kernel's members are those rows; after the last round the best start of every component is selected, its
// results become the plan's ordinary outputs and its clamped x is gathered into the problem's x.
//
// The host part is pure (no HIP call, nothing of HIP in what a host compiler sees of this header): the two int32 tables the
// kernels follow (lm_starts_tables) and the select rule as a sequential scan (lm_starts_best), which the select kernel calls and
// tests/cpp/lm_starts_layout_test.cpp runs without a device.
#pragma once
#include <cstdint>
#include <vector>

#include "population_select.hpp"   // better(): the one order of "which start is kept"

namespace rdis_hip {

// pos[N]: where variable v stands in the plan's free list (free_vid[pos[v]] == v), -1: v is not free in the plan -- a constant
// every start shares.  comp_of[nfree]: the component entry k of the free list belongs to (free_ptr[comp_of[k]] <= k <
// free_ptr[comp_of[k] + 1]).  The lists have passed plan_index_build: ids in range, no variable free twice.
inline void lm_starts_tables(int64_t N, int64_t ncomp, const int64_t* free_ptr, const int64_t* free_vid, std::vector<int32_t>& pos,
                             std::vector<int32_t>& comp_of) {
    const int64_t nfree = ncomp > 0 ? free_ptr[ncomp] : 0;
    pos.assign((size_t)(N > 0 ? N : 0), -1);
    comp_of.assign((size_t)nfree, 0);
    for (int64_t c = 0; c < ncomp; ++c)
        for (int64_t k = free_ptr[c]; k < free_ptr[c + 1]; ++k) {
            pos[(size_t)free_vid[k]] = (int32_t)k;
            comp_of[(size_t)k] = (int32_t)c;
        }
}

// The start a component keeps: the minimum of f[s * stride], s < nstarts, by better() -- the lowest value, on a tie (-0.0 against
// +0.0 is one) the lowest index, a NaN never unless every value is one: then start 0.  A sequential scan in start order.
RDIS_SELECT_FN long long lm_starts_best(long long nstarts, const double* f, long long stride) {
    long long b = 0;
    double fb = f[0];
    for (long long s = 1; s < nstarts; ++s) {
        const double fs = f[s * stride];
        if (better(fs, s, fb, b)) { fb = fs; b = s; }
    }
    return b;
}

// A step's summary (rdis_hip_lm_plan_summary): 16 doubles over the plan's ordinary outputs.  Where a result row keeps what is
// summed (lm_batch.hip writes the row: fret, the value at the start, then info8) and where each sum stands in the block; the
// counts of stop codes 1..7 follow LM_SUMMARY_STOP1, the last two doubles are zero.
constexpr int LM_ROW_FRET = 0, LM_ROW_F0 = 1, LM_ROW_INFO = 2;
constexpr int LM_SUMMARY_DOUBLES = 16;   // RDIS_HIP_LM_SUMMARY_DOUBLES (lm_api.hip asserts both equal)
constexpr int LM_SUMMARY_FRET = 0, LM_SUMMARY_DELTA = 1, LM_SUMMARY_ITERS = 2, LM_SUMMARY_NFEV = 3, LM_SUMMARY_NJEV = 4, LM_SUMMARY_NSOLVE = 5,
              LM_SUMMARY_STOP1 = 6, LM_SUMMARY_NONFINITE = 13, LM_SUMMARY_FIELDS = 14;

#if defined(__HIPCC__)
// What the launches below share: the plan's outputs for R = nstarts + 1 rows (replica_layout.hpp: lm_starts_layout; strides in
// doubles) and its tables.
struct LmStartsOut {
    double *res, *hist, *xout;               // row 0 of each field
    long long res_ms, hist_ms, xout_ms;      // a row's stride: [ncomp][res_doubles], [ncomp][hist_cap][4], [nfree]
    long long hist_cap;
    int res_doubles, nhist_at;               // doubles of a result row; where in it the history's record count stands
    int* best;                               // [ncomp]
};
// rows[r][v] = pos[v] >= 0 ? src[(first + r) * src_stride + (by_pos ? pos[v] : v)] : x[v],  r < count (at most 65535), v < N.
// by_pos: src is an uploaded [nstarts][nfree] block in free-list order; otherwise rows of N values indexed by variable id.
hipError_t lm_starts_fill_launch(hipStream_t stream, int blocks, double* rows, long long N, const double* x, const int* pos, const double* src,
                                 long long src_stride, bool by_pos, long long first, int count);
// best[c] = lm_starts_best over res[s][c][0]; the winner's result row and history records copied to row nstarts
hipError_t lm_starts_select_launch(hipStream_t stream, const LmStartsOut& O, long long nstarts, long long ncomp);
// x[free32[k]] = xout[nstarts][k] = xout[best[comp_of[k]]][k],  k < nfree
hipError_t lm_starts_gather_launch(hipStream_t stream, const LmStartsOut& O, long long nstarts, long long nfree, const int* free32, const int* comp_of,
                                   double* x);
// out[0] = the sum of res[c * stride], c < ncomp, in a fixed order: one workgroup of 256, a lane's stride in component order, a
// butterfly over the wave, then the waves in wave order
hipError_t lm_plan_objective_launch(hipStream_t stream, long long ncomp, const double* res, long long stride, double* out);
// out[0 .. LM_SUMMARY_DOUBLES): the fields above over the rows res + c * stride, c < ncomp, every field in that same order; one
// workgroup of 256, lane 0 stores the block with plain stores
hipError_t lm_plan_summary_launch(hipStream_t stream, long long ncomp, const double* res, long long stride, double* out);
// the same per member of a population solve, in one launch: out[m][0 .. LM_SUMMARY_DOUBLES) over the rows res + m * member_stride +
// c * stride, c < ncomp, m < nmembers; one workgroup of 256 per member (the member in the grid's x dimension, striding beyond 65535
// workgroups), every field in lm_plan_summary_launch's order -- member m's block is bit for bit that launch's over the same rows
hipError_t lm_plan_summary_members_launch(hipStream_t stream, long long nmembers, long long ncomp, const double* res, long long member_stride,
                                          long long stride, double* out);
#endif

}  // namespace rdis_hip
