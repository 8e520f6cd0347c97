// lm_batch.hip -- Levenberg-Marquardt for a batch of small bundle-adjustment components: one workgroup per component,
// the whole solve of a component inside one launch (rdis_hip_lm_batch).
//
// Each component is a run of oracle/lm_oracle.py's lm_optimize: the iteration of lm_solver.hip (Nielsen's damping update,
// levmar's stop codes, model 2's projected trial points and Marquardt scaling) with its control loop moved from the host
// into the workgroup.  Every thread of the workgroup carries the loop's scalars (mu, nu, the objective, the counters) and
// takes the same decisions from sums that were broadcast through LDS: no host round trip, no second launch.
//
// The linear algebra is lm_solver.hip's, sized for one workgroup:
//     [ U + D_c    W       ] [dc]   [bc]       U_c = sum_j Jc_j Jc_j^T   (9 x 9 per camera),  V_p likewise (3 x 3 per point)
//     [ W^T        V + D_p ] [dp] = [bp]
// reduced to the cameras, (U + D_c - Z Z^T) dc = bc - Z y with L_p L_p^T = V_p + D_p, Z's block (c, p) = Jc_j (L_p^-1 Jp_j)^T,
// y_p = L_p^-1 bp_p;  dp_p = L_p^-T (y_p - Z_p^T dc).  Z Z^T is block-sparse over the camera pairs that share a point
// (lm_batch_prepare lists them).  The reduced system (at most 144 unknowns) lives in LDS as a packed lower triangle with
// the right-hand side as one more row, so that the factorisation leaves L^-1 rhs behind and only L^T dc = z remains.
// Per-factor rows (Jc, Jp, e, T, Z blocks) and per-point blocks are in the component's workspace slice in HBM.
//
// A component of 17 to 64 cameras (class 3, the wide class, by option) runs the same iteration; its reduced system (up to
// 576 unknowns) does not fit the LDS, lies in the workspace slice as 16 x 16 tiles (lm_batch.hpp: LmWideTiles) and is
// factorised in panels of 16 columns that pass through the LDS, the trailing update on the matrix cores.
//
// Every sum runs in an order fixed by the component's own lists and its class (lm_batch.hpp: the class, and with it the
// workgroup size, is a function of the component's camera count alone): a component's bits depend neither on what else
// is in the batch nor on where it stands in it.
//
// The kernel is instantiated twice per class from the one body.  In the plans' instantiation the grid's second dimension is the
// member (rdis_hip_lm_plan_solve_population: a population's rows of x; rdis_hip_lm_plan_solve: one member): a member has its own
// x, its own replica of the workspace and its own rows of the outputs, and shares everything else.  The member enters pointer
// sums only, so its bits are those of rdis_hip_lm_batch's instantiation, which has no member terms at all, on its x.
#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "factors.hpp"
#include "launch_dispatch.hpp"
#include "lm_batch.hpp"

namespace rdis_hip {
namespace {

struct BatchDev {   // everything the kernel needs, by value
    double* x;                 // member 0's
    const double *lo, *hi;
    const int *cam, *pt;
    const double2* obs;
    const int *ints, *free32, *order;
    const unsigned char* freem;
    const LmBatchComp* comps;
    double *res, *hist, *ws;   // per member: [ncomp][LM_BATCH_RES], [ncomp][hist_cap][4] (or null), the workspace slices
    int R, maxiters;
    long long hist_cap;
    double tau, eps1, eps2, eps3;
    // the members' instantiation only: member m = blockIdx.y reads and writes x + m x_ms, and so for ws, res and hist (strides
    // in doubles; everything else is shared by the members); xout + m xout_ms: [nfree] the member's clamped results, kept for the fetch
    long long x_ms, ws_ms, res_ms, hist_ms, xout_ms;
    double* xout;
};

__device__ __forceinline__ double wave_sum(double v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ double wave_max(double v) {
    for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o));
    return v;
}
// sums (s) and maxima (m) over the workgroup, every thread receiving the same values: waves in wave order
template <int NT, int KS, int KM>
__device__ __forceinline__ void block_reduce(double* s, double* m, double* red) {
#pragma unroll
    for (int k = 0; k < KS; ++k) s[k] = wave_sum(s[k]);
#pragma unroll
    for (int k = 0; k < KM; ++k) m[k] = wave_max(m[k]);
    if (NT == 64) return;
    constexpr int K = KS + KM;
    static_assert(K * (NT / 64) <= 64, "reduction scratch");
    __syncthreads();   // (the scratch's last readers)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < KS; ++k) red[K * (threadIdx.x >> 6) + k] = s[k];
#pragma unroll
        for (int k = 0; k < KM; ++k) red[K * (threadIdx.x >> 6) + KS + k] = m[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < KS; ++k) s[k] = 0.0;
#pragma unroll
    for (int k = 0; k < KM; ++k) m[k] = red[KS + k];
    for (int w = 0; w < NT / 64; ++w) {
#pragma unroll
        for (int k = 0; k < KS; ++k) s[k] += red[K * w + k];
#pragma unroll
        for (int k = 0; k < KM; ++k) m[k] = fmax(m[k], red[K * w + KS + k]);
    }
}

typedef double d4 __attribute__((ext_vector_type(4)));   // the accumulator of v_mfma_f64_16x16x4_f64

__device__ __forceinline__ int tri(int i) { return i * (i + 1) / 2; }   // start of row i of a packed lower triangle
__device__ __forceinline__ int vdiag(int k) { return k == 0 ? 0 : k == 1 ? 2 : 5; }   // V's packing: v00 v10 v11 v20 v21 v22

// MEMBERS false: a launch of one member whose pointers are B's own (rdis_hip_lm_batch) -- the member's terms are compiled out;
// true: the grid's second dimension is the member (the plans' launches).  One body: the arithmetic is the same text.
template <int CLS, bool MEMBERS>
__global__ void __launch_bounds__(lm_batch_class_threads(CLS)) k_lm_batch(BatchDev B, int first) {
    constexpr int NT = lm_batch_class_threads(CLS), MAXC = lm_batch_class_cameras(CLS);
    extern __shared__ __attribute__((aligned(16))) double lm_batch_lds[];
    double* const red = lm_batch_lds;
    double* const U = lm_batch_lds + LM_BATCH_LDS_HEAD;
    double* const bc = U + 81 * MAXC;
    double* const dc = bc + 9 * MAXC;
    double* const S = dc + 9 * MAXC;
    const int tid = threadIdx.x;
    const LmBatchComp C = B.comps[B.order[first + blockIdx.x]];
    // the member: its x, its replica of the workspace, its rows of the outputs.  Nothing else depends on it: no count, no
    // stride of a loop, no order of a sum
    const long long mem = MEMBERS ? (long long)blockIdx.y : 0;
    double* const x = MEMBERS ? B.x + mem * B.x_ms : B.x;
    const int nf = C.nf, nca = MAXC > 0 ? C.nca : 0, npa = C.npa, nfree = C.nfree, R = B.R, M = 9 * nca;
    const int* const it = B.ints + C.ints0;
    const int *lf = it + C.o_lf, *fci = it + C.o_fci, *fpi = it + C.o_fpi, *cptr = it + C.o_cptr, *clist = it + C.o_clist;
    const int *pptr = it + C.o_pptr, *plist = it + C.o_plist, *fslot = it + C.o_fslot;
    const int *pab = it + C.o_pab, *pairptr = it + C.o_pairptr, *pja = it + C.o_pja, *pjb = it + C.o_pjb;
    const int* const fv = B.free32 + C.free0;
    const LmBatchSlice W = lm_batch_slice(nf, C.nca, npa, nfree, R);
    double* const ws = (MEMBERS ? B.ws + mem * B.ws_ms : B.ws) + C.ws0;
    double *Jc = ws + W.Jc, *Jp = ws + W.Jp, *E = ws + W.e, *T = ws + W.T, *Zc = ws + W.Zc, *V = ws + W.V, *bp = ws + W.bp;
    double *Lp = ws + W.Lp, *yp = ws + W.yp, *dp = ws + W.dp, *psave = ws + W.psave;

    auto load12 = [&](int f, double (&v)[12]) {
        const int c = B.cam[f], q = B.pt[f];
#pragma unroll
        for (int k = 0; k < 12; ++k) v[k] = x[k < 9 ? c + k : q + (k - 9)];
    };
    // objective of the listed factors at the current x
    auto objective = [&]() -> double {
        __syncthreads();   // (x as the workgroup last wrote it)
        double acc[1] = {0.0};
        for (int j = tid; j < nf; j += NT) {
            const int f = lf[j];
            double v[12];
            load12(f, v);
            const double2 o = B.obs[f];
            acc[0] += ba_eval(v, o.x, o.y);
        }
        block_reduce<NT, 1, 0>(acc, nullptr, red);
        return acc[0];
    };
    // residuals and Jacobian rows, U_c, V_p, the gradient; max diag(J^T J), |J^T e|_inf, |p|^2
    auto linearise = [&](double& maxdiag, double& jte_inf, double& p_L2) {
        for (int j = tid; j < nf; j += NT) {
            const int f = lf[j], c = B.cam[f], q = B.pt[f], ci = fci[j], pi = fpi[j];
            double v[12], g[12];
            load12(f, v);
            const double2 o = B.obs[f];
            if (R == 1) {   // the reference's formulation: one residual sqrt(2 E), row grad E / e
                const double Ev = ba_eval_grad(v, o.x, o.y, g);
                const double e = sqrt(2.0 * Ev);
                const double inv = e > 0.0 ? 1.0 / e : 0.0;
                E[j] = e;
                if (ci >= 0)
#pragma unroll
                    for (int k = 0; k < 9; ++k) Jc[9ll * j + k] = B.freem[c + k] ? g[k] * inv : 0.0;
                if (pi >= 0)
#pragma unroll
                    for (int k = 0; k < 3; ++k) Jp[3ll * j + k] = B.freem[q + k] ? g[9 + k] * inv : 0.0;
            } else {        // the two pixel residuals and their Jacobian rows
                double res[2], g2[12];
                ba_residual_jacobian(v, o.x, o.y, res, g, g2);
                E[2ll * j] = res[0]; E[2ll * j + 1] = res[1];
                if (ci >= 0)
#pragma unroll
                    for (int k = 0; k < 9; ++k) {
                        const bool fr = B.freem[c + k];
                        Jc[18ll * j + k] = fr ? g[k] : 0.0; Jc[18ll * j + 9 + k] = fr ? g2[k] : 0.0;
                    }
                if (pi >= 0)
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        const bool fr = B.freem[q + k];
                        Jp[6ll * j + k] = fr ? g[9 + k] : 0.0; Jp[6ll * j + 3 + k] = fr ? g2[9 + k] : 0.0;
                    }
            }
        }
        __syncthreads();
        if (MAXC > 0)   // a thread per entry of U_c and of bc, over the camera's rows in listed order
            for (int t = tid; t < 90 * nca; t += NT) {
                const int c = t / 90, k = t - 90 * c;
                const int b0 = cptr[c], b1 = cptr[c + 1];
                const int row = k < 81 ? k / 9 : k - 81, col = k < 81 ? k - 9 * (k / 9) : 0;
                double acc = 0.0;
                int u = b0;
                if constexpr (CLS == 3) {
                    // (a wide component's cameras have hundreds of rows and the workgroup has the unit to itself: the operands
                    // of four factors are fetched before they are added, in the same order)
                    for (; u + 4 <= b1; u += 4) {
                        double p[4][2], q[4][2];
#pragma unroll
                        for (int v = 0; v < 4; ++v) {
                            const long long j = clist[u + v];
#pragma unroll
                            for (int r = 0; r < 2; ++r) {
                                const long long jr = j * R + (r < R ? r : 0);
                                p[v][r] = Jc[9 * jr + row];
                                q[v][r] = k < 81 ? Jc[9 * jr + col] : E[jr];
                            }
                        }
#pragma unroll
                        for (int v = 0; v < 4; ++v)
#pragma unroll
                            for (int r = 0; r < 2; ++r)
                                if (r < R) acc += p[v][r] * q[v][r];
                    }
                }
                for (; u < b1; ++u)
                    for (int r = 0; r < R; ++r) {
                        const long long jr = (long long)clist[u] * R + r;
                        acc += Jc[9 * jr + row] * (k < 81 ? Jc[9 * jr + col] : E[jr]);
                    }
                if (k < 81) U[81 * c + k] = acc;
                else bc[9 * c + row] = -acc;
            }
        for (int t = tid; t < 9 * npa; t += NT) {   // V_p: v00 v10 v11 v20 v21 v22, then bp
            const int p = t / 9, k = t - 9 * p;
            const int i = k < 6 ? (k == 0 ? 0 : k < 3 ? 1 : 2) : k - 6, jj = k == 0 || k == 1 || k == 3 ? 0 : k == 2 || k == 4 ? 1 : 2;
            double acc = 0.0;
            for (int u = pptr[p]; u < pptr[p + 1]; ++u)
                for (int r = 0; r < R; ++r) {
                    const long long jr = (long long)plist[u] * R + r;
                    acc += Jp[3 * jr + i] * (k < 6 ? Jp[3 * jr + jj] : E[jr]);
                }
            if (k < 6) V[6ll * p + k] = acc;
            else bp[3ll * p + i] = -acc;
        }
        __syncthreads();
        double s[1] = {0.0}, m[2] = {0.0, 0.0};
        if (MAXC > 0)
            for (int t = tid; t < M; t += NT) {
                m[0] = fmax(m[0], U[81 * (t / 9) + 10 * (t % 9)]);
                m[1] = fmax(m[1], fabs(bc[t]));
            }
        for (int t = tid; t < 3 * npa; t += NT) {
            m[0] = fmax(m[0], V[6ll * (t / 3) + vdiag(t % 3)]);
            m[1] = fmax(m[1], fabs(bp[t]));
        }
        for (int i = tid; i < nfree; i += NT) { const double xv = x[fv[i]]; s[0] += xv * xv; }
        block_reduce<NT, 1, 2>(s, m, red);
        maxdiag = m[0]; jte_inf = m[1]; p_L2 = s[0];
    };
    // damping added to a diagonal entry d of J^T J: mu (model 1) or mu * max(d, floor) (Marquardt's scaling, model 2)
    auto damp = [&](double mu, double floor_, double d) { return R == 2 ? mu * fmax(d, floor_) : mu; };
    // one damped solve and its trial point (x = accepted point + step): false on a pivot <= 0 of the reduced system
    auto attempt = [&](double mu, double floor_, double& Dp_L2, double& dL) -> bool {
        for (int p = tid; p < npa; p += NT) {   // point Cholesky, y_p
            const double* Vp = V + 6ll * p;
            const double l00 = sqrt(Vp[0] + damp(mu, floor_, Vp[0]));
            const double l10 = Vp[1] / l00, l20 = Vp[3] / l00;
            const double l11 = sqrt(Vp[2] + damp(mu, floor_, Vp[2]) - l10 * l10);
            const double l21 = (Vp[4] - l20 * l10) / l11;
            const double l22 = sqrt(Vp[5] + damp(mu, floor_, Vp[5]) - l20 * l20 - l21 * l21);
            double* L = Lp + 6ll * p;
            L[0] = l00; L[1] = l10; L[2] = l11; L[3] = l20; L[4] = l21; L[5] = l22;
            const double y0 = bp[3ll * p] / l00;
            const double y1 = (bp[3ll * p + 1] - l10 * y0) / l11;
            const double y2 = (bp[3ll * p + 2] - l20 * y0 - l21 * y1) / l22;
            yp[3ll * p] = y0; yp[3ll * p + 1] = y1; yp[3ll * p + 2] = y2;
        }
        __syncthreads();
        for (int j = tid; j < nf; j += NT) {    // T_j = L_p^-1 Jp_j and the factor's Z block
            const int ci = fci[j], pi = fpi[j];
            if (pi < 0) continue;
            const double* L = Lp + 6ll * pi;
            double t0[2] = {0, 0}, t1[2] = {0, 0}, t2[2] = {0, 0};
            for (int r = 0; r < R; ++r) {
                const long long jr = (long long)j * R + r;
                t0[r] = Jp[3 * jr] / L[0];
                t1[r] = (Jp[3 * jr + 1] - L[1] * t0[r]) / L[2];
                t2[r] = (Jp[3 * jr + 2] - L[3] * t0[r] - L[4] * t1[r]) / L[5];
                T[3 * jr] = t0[r]; T[3 * jr + 1] = t1[r]; T[3 * jr + 2] = t2[r];
            }
            if (MAXC == 0 || ci < 0) continue;
            double* z = Zc + 27ll * j;
#pragma unroll
            for (int a = 0; a < 9; ++a) {
                const double jc0 = Jc[9ll * j * R + a], jc1 = R == 2 ? Jc[9ll * (2 * j + 1) + a] : 0.0;
                z[a] = jc0 * t0[0] + jc1 * t0[1]; z[9 + a] = jc0 * t1[0] + jc1 * t1[1]; z[18 + a] = jc0 * t2[0] + jc1 * t2[1];
            }
        }
        __syncthreads();
        bool solved = true;
        if constexpr (CLS == 3) {
            // The wide class: the reduced system lies in the slice's 16 x 16 tiles (LmWideTiles: rows 0 .. M, the right-hand
            // side as row M) and is factorised right-looking in panels of 16 columns that pass through the LDS.
            constexpr int TS = LM_WIDE_TILE, PS = LM_WIDE_PANEL_STRIDE;
            const LmWideTiles G(nca);
            double* const Sg = ws + W.S;
            double* const P = S;                 // the panel: row r of its tile rows at P + PS r
            double* const flag = red + LM_BATCH_LDS_HEAD - 1;   // 0: a pivot <= 0 (block_reduce uses the scratch's first 24 at most)
            const int tx = tid & 15, ty = tid >> 4, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
            // S = U + damping on the block diagonal, zero elsewhere, the tiles' padding and row M included
            for (int row = ty; row < TS * G.nt; row += NT / 16)
                for (int col = tx; col < TS * (row / TS + 1); col += 16) {
                    double v = 0.0;
                    if (row < M && col <= row) {
                        if (row / 9 == col / 9) v = U[81 * (row / 9) + 9 * (row % 9) + (col % 9)];
                        if (row == col) v += damp(mu, floor_, v);
                    }
                    Sg[G.at(row, col)] = v;
                }
            __syncthreads();
            for (int t = tid; t < M; t += NT) {   // row M: rhs = bc - Z y
                const int c = t / 9, a = t - 9 * c;
                double acc = 0.0;
#pragma unroll 4
                for (int u = cptr[c]; u < cptr[c + 1]; ++u) {
                    const int j = clist[u], pi = fpi[j];
                    if (pi < 0) continue;
                    for (int r = 0; r < R; ++r) {
                        const long long jr = (long long)j * R + r;
                        const double wv_ = T[3 * jr] * yp[3ll * pi] + T[3 * jr + 1] * yp[3ll * pi + 1] + T[3 * jr + 2] * yp[3ll * pi + 2];
                        acc += Jc[9 * jr + a] * wv_;
                    }
                }
                Sg[G.at(M, t)] = bc[t] - acc;
            }
            // S -= Z Z^T: a thread per entry of a pair's 9 x 9 block, over the points both cameras see, in point order
            for (int t = tid; t < 81 * C.npair; t += NT) {
                const int q = t / 81, k = t - 81 * q, row = k / 9, col = k - 9 * row;
                const int a = pab[2 * q], b = pab[2 * q + 1];
                if (a == b && col > row) continue;
                double acc = 0.0;
                int e = pairptr[q];
                const int e1 = pairptr[q + 1];
                // (a wide component's pairs share many points and the workgroup has the unit to itself: the operands of four
                // entries are fetched before they are added, in the same order)
                for (; e + 4 <= e1; e += 4) {
                    double za[4][3], zb[4][3];
#pragma unroll
                    for (int u = 0; u < 4; ++u) {
                        const double *pa = Zc + 27ll * pja[e + u] + row, *pb = Zc + 27ll * pjb[e + u] + col;
                        za[u][0] = pa[0]; za[u][1] = pa[9]; za[u][2] = pa[18];
                        zb[u][0] = pb[0]; zb[u][1] = pb[9]; zb[u][2] = pb[18];
                    }
#pragma unroll
                    for (int u = 0; u < 4; ++u) acc += za[u][0] * zb[u][0] + za[u][1] * zb[u][1] + za[u][2] * zb[u][2];
                }
                for (; e < e1; ++e) {
                    const double *za = Zc + 27ll * pja[e], *zb = Zc + 27ll * pjb[e];
                    acc += za[row] * zb[col] + za[9 + row] * zb[9 + col] + za[18 + row] * zb[18 + col];
                }
                Sg[G.at(9 * a + row, 9 * b + col)] -= acc;
            }
            // Cholesky by panels; row M (the right-hand side) rides along as the last row of every panel
            for (int kp = 0; kp < G.np; ++kp) {
                __syncthreads();   // (the stores of S above / of the last trailing update; the panel's last readers)
                const int nr = TS * (G.nt - kp), w = min(TS, M - TS * kp);   // the panel's rows; its columns that exist
                for (int e = tid; e < nr * TS; e += NT) {
                    const int r = e >> 4, c = e & 15;
                    P[PS * r + c] = Sg[G.tile(kp + (r >> 4), kp) + ((r & 15) << 4) + c];
                }
                if (tid == 0) *flag = 1.0;
                __syncthreads();
                if (tid < 64) {   // the diagonal tile in wave 0's registers: lane r (and r + 16, ...) holds row r; by columns
                    const int r = lane & 15;
                    double a[TS];
#pragma unroll
                    for (int c = 0; c < TS; ++c) a[c] = P[PS * r + c];
                    bool okp = true;
#pragma unroll
                    for (int c = 0; c < TS; ++c) {
                        if (c < w && okp) {   // (the same for every lane)
                            const double d = __shfl(a[c], c);
                            if (!(d > 0.0)) {
                                okp = false;
                            } else {
                                const double l = sqrt(d);
                                a[c] = r == c ? l : a[c] / l;
#pragma unroll
                                for (int j = c + 1; j < TS; ++j)
                                    if (j < w) a[j] -= a[c] * __shfl(a[c], j);   // (entries right of the diagonal: computed, never stored)
                            }
                        }
                    }
                    if (lane < TS)
#pragma unroll
                        for (int c = 0; c < TS; ++c)
                            if (c <= r && c < w) P[PS * r + c] = a[c];
                    if (lane == 0 && !okp) *flag = 0.0;
                }
                __syncthreads();
                if (*flag == 0.0) { solved = false; break; }   // (every thread reads the same value)
                for (int r = TS + tid; r < nr; r += NT) {   // the rows below: row L_kk^T = row, a lane per row
                    double a[TS];
#pragma unroll
                    for (int c = 0; c < TS; ++c) a[c] = P[PS * r + c];
#pragma unroll
                    for (int c = 0; c < TS; ++c)
                        if (c < w) {
                            double v = a[c];
#pragma unroll
                            for (int j = 0; j < c; ++j) v -= a[j] * P[PS * c + j];
                            a[c] = v / P[PS * c + c];
                        }
#pragma unroll
                    for (int c = 0; c < TS; ++c) P[PS * r + c] = a[c];
                }
                __syncthreads();
                for (int e = tid; e < nr * TS; e += NT) {
                    const int r = e >> 4, c = e & 15;
                    Sg[G.tile(kp + (r >> 4), kp) + ((r & 15) << 4) + c] = P[PS * r + c];
                }
                // trailing update on the matrix cores: tile (ti, tj) -= P_ti P_tj^T, the waves striding over the tile pairs.
                // v_mfma_f64_16x16x4_f64 (lm_solver.hip's k_cam): lane l supplies A[l & 15][l >> 4] and B[l >> 4][l & 15], its
                // result register r is D[(l >> 4) + 4 r][l & 15]; four of them cover the panel's sixteen columns.
                {
                    const int i16 = lane & 15, kq = lane >> 4;
                    // a wave's unit of work: up to four neighbouring tiles of one tile row (they share P_ti and lie one behind the
                    // other), all loaded before the first is updated
                    int cnt = 0;
                    for (int ti = kp + 1; ti < G.nt; ++ti) {
                        const int tjend = min(ti, G.np - 1);
                        for (int tj0 = kp + 1; tj0 <= tjend; tj0 += 4, cnt = (cnt + 1) & (NT / 64 - 1)) {
                            if (cnt != wv) continue;
                            double* const tl = Sg + G.tile(ti, tj0) + TS * kq + i16;
                            const double* const pa = P + PS * (TS * (ti - kp) + i16) + kq;
                            const double* const pb = P + PS * (TS * (tj0 - kp) + i16) + kq;
                            const int n = min(4, tjend - tj0 + 1);
                            const double a0 = -pa[0], a1 = -pa[4], a2 = -pa[8], a3 = -pa[12];
                            d4 acc[4];
#pragma unroll
                            for (int u = 0; u < 4; ++u) {   // (beyond the row's end: its last tile once more, computed and not stored)
                                const double* const t = tl + TS * TS * min(u, n - 1);
                                acc[u] = d4{t[0], t[4 * TS], t[8 * TS], t[12 * TS]};
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u) {
                                const double* const b = pb + PS * TS * min(u, n - 1);
                                acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, b[0], acc[u], 0, 0, 0);
                                acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, b[4], acc[u], 0, 0, 0);
                                acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a2, b[8], acc[u], 0, 0, 0);
                                acc[u] = __builtin_amdgcn_mfma_f64_16x16x4f64(a3, b[12], acc[u], 0, 0, 0);
                            }
#pragma unroll
                            for (int u = 0; u < 4; ++u)
                                if (u < n) {
                                    tl[TS * TS * u] = acc[u][0]; tl[TS * TS * u + 4 * TS] = acc[u][1];
                                    tl[TS * TS * u + 8 * TS] = acc[u][2]; tl[TS * TS * u + 12 * TS] = acc[u][3];
                                }
                        }
                    }
                }
            }
            __syncthreads();
            if (solved) {   // L^T dc = z (row M), tile row by tile row from the bottom
                for (int t = tid; t < M; t += NT) dc[t] = Sg[G.at(M, t)];
                for (int kt = G.np - 1; kt >= 0; --kt) {
                    const int w = min(TS, M - TS * kt);
                    if (tid < TS * TS) P[tid] = Sg[G.tile(kt, kt) + tid];
                    __syncthreads();
                    if (tid < 64) {   // the tile's own unknowns in wave 0: lane r holds z_r
                        const int r = lane & 15;
                        double z = r < w ? dc[TS * kt + r] : 0.0;
#pragma unroll
                        for (int k = TS - 1; k >= 0; --k)
                            if (k < w) {
                                const double xk = __shfl(z, k) / P[TS * k + k];
                                if (r == k) z = xk;
                                else if (r < k) z -= P[TS * k + r] * xk;
                            }
                        if (lane < w) dc[TS * kt + lane] = z;
                    }
                    __syncthreads();
                    for (int i = tid; i < TS * kt; i += NT) {   // ... taken out of the unknowns above, a lane per unknown
                        const double* const col = Sg + G.tile(kt, i / TS) + i % TS;
                        double l[TS];   // (all sixteen rows of the tile exist; those beyond w are loaded and not used)
#pragma unroll
                        for (int k = 0; k < TS; ++k) l[k] = col[TS * k];
                        double acc = dc[i];
#pragma unroll
                        for (int k = TS - 1; k >= 0; --k)
                            if (k < w) acc -= l[k] * dc[TS * kt + k];
                        dc[i] = acc;
                    }
                }
            }
            __syncthreads();
            if (!solved) return false;
        } else
        if (MAXC > 0 && nca > 0) {
            const int tx = tid & 15, ty = tid >> 4;
            // S = U + damping on the block diagonal, zero elsewhere; row M: rhs = bc - Z y
            for (int row = ty; row < M; row += NT / 16)
                for (int col = tx; col <= row; col += 16) {
                    double v = 0.0;
                    if (row / 9 == col / 9) v = U[81 * (row / 9) + 9 * (row % 9) + (col % 9)];
                    if (row == col) v += damp(mu, floor_, v);
                    S[tri(row) + col] = v;
                }
            for (int t = tid; t < M; t += NT) {
                const int c = t / 9, a = t - 9 * c;
                double acc = 0.0;
                for (int u = cptr[c]; u < cptr[c + 1]; ++u) {
                    const int j = clist[u], pi = fpi[j];
                    if (pi < 0) continue;
                    for (int r = 0; r < R; ++r) {
                        const long long jr = (long long)j * R + r;
                        const double wv = T[3 * jr] * yp[3ll * pi] + T[3 * jr + 1] * yp[3ll * pi + 1] + T[3 * jr + 2] * yp[3ll * pi + 2];
                        acc += Jc[9 * jr + a] * wv;
                    }
                }
                S[tri(M) + t] = bc[t] - acc;
            }
            __syncthreads();
            // S -= Z Z^T: a thread per entry of a pair's 9 x 9 block, over the points both cameras see, in point order
            for (int t = tid; t < 81 * C.npair; t += NT) {
                const int q = t / 81, k = t - 81 * q, row = k / 9, col = k - 9 * row;
                const int a = pab[2 * q], b = pab[2 * q + 1];
                if (a == b && col > row) continue;
                double acc = 0.0;
                for (int e = pairptr[q]; e < pairptr[q + 1]; ++e) {
                    const double *za = Zc + 27ll * pja[e], *zb = Zc + 27ll * pjb[e];
                    acc += za[row] * zb[col] + za[9 + row] * zb[9 + col] + za[18 + row] * zb[18 + col];
                }
                S[tri(9 * a + row) + 9 * b + col] -= acc;
            }
            // Cholesky, right-looking by columns; row M (the right-hand side) rides along
            for (int k = 0; k < M; ++k) {
                __syncthreads();
                const double d = S[tri(k) + k];
                if (!(d > 0.0)) { solved = false; break; }   // (every thread reads the same value)
                const double l = sqrt(d);
                __syncthreads();
                for (int i = k + tid; i <= M; i += NT) S[tri(i) + k] = i == k ? l : S[tri(i) + k] / l;
                __syncthreads();
                for (int i = k + 1 + ty; i <= M; i += NT / 16) {
                    const double lik = S[tri(i) + k];
                    const int jend = i < M ? i : M - 1;
                    for (int j = k + 1 + tx; j <= jend; j += 16) S[tri(i) + j] -= lik * S[tri(j) + k];
                }
            }
            if (solved) {   // L^T dc = z, from the bottom
                for (int k = M - 1; k >= 0; --k) {
                    __syncthreads();
                    const double xk = S[tri(M) + k] / S[tri(k) + k];
                    for (int i = tid; i < k; i += NT) S[tri(M) + i] -= S[tri(k) + i] * xk;
                    if (tid == 0) dc[k] = xk;
                }
            }
            __syncthreads();
            if (!solved) return false;
        }
        for (int p = tid; p < npa; p += NT) {   // back-substitution for the points
            double s0 = 0, s1 = 0, s2 = 0;
            if (MAXC > 0)
                for (int u = pptr[p]; u < pptr[p + 1]; ++u) {
                    const int j = plist[u], ci = fci[j];
                    if (ci < 0) continue;
                    for (int r = 0; r < R; ++r) {
                        const long long jr = (long long)j * R + r;
                        double w = 0.0;
#pragma unroll
                        for (int a = 0; a < 9; ++a) w += Jc[9 * jr + a] * dc[9 * ci + a];
                        s0 += T[3 * jr] * w; s1 += T[3 * jr + 1] * w; s2 += T[3 * jr + 2] * w;
                    }
                }
            const double* L = Lp + 6ll * p;
            const double r0 = yp[3ll * p] - s0, r1 = yp[3ll * p + 1] - s1, r2 = yp[3ll * p + 2] - s2;
            const double d2 = r2 / L[5];
            const double d1 = (r1 - L[4] * d2) / L[2];
            const double d0 = (r0 - L[1] * d1 - L[3] * d2) / L[0];
            dp[3ll * p] = d0; dp[3ll * p + 1] = d1; dp[3ll * p + 2] = d2;
        }
        __syncthreads();
        double s[2] = {0.0, 0.0};   // |Dp|^2, dL = Dp . (damping Dp + J^T e)
        for (int i = tid; i < nfree; i += NT) {
            const int v = fv[i], sl = fslot[i];
            double dpv = 0.0, b = 0.0, dg = 0.0;
            if (sl >= 0) {
                if (MAXC > 0) { dpv = dc[sl]; b = bc[sl]; dg = U[81 * (sl / 9) + 10 * (sl % 9)]; }
            } else if (sl <= -2) {
                const int u = -(sl + 2);
                dpv = dp[u]; b = bp[u]; dg = V[6ll * (u / 3) + vdiag(u % 3)];
            }
            double xn = psave[i] + dpv;
            if (R == 2) {   // the pixel-residual model keeps every trial point inside the domains
                const double lo = B.lo[v], hi = B.hi[v];
                xn = (lo <= xn && xn <= hi) ? xn : (xn < lo ? lo : hi);
            }
            x[v] = xn;
            s[0] += dpv * dpv;
            s[1] += dpv * (damp(mu, floor_, dg) * dpv + b);
        }
        block_reduce<NT, 2, 0>(s, nullptr, red);
        Dp_L2 = s[0]; dL = s[1];
        return true;
    };

    // ---- the iteration of lm_oracle.lm_optimize / device_lm_ba -----------------------------------------------------------
    for (int i = tid; i < nfree; i += NT) psave[i] = x[fv[i]];
    const double finit = objective();
    double p_eL2 = 2.0 * finit, mu = 0.0;
    long long nu = 2;
    int stop = 0, k = 0, nfev = 1, njev = 0, nsolve = 0;
    long long nh = 0;
    const double EPSILON = 1e-12, ONE_THIRD = 0.3333333334;
    while (k < B.maxiters && !stop) {
        if (!isfinite(p_eL2)) { stop = 7; break; }   // a start whose objective is not finite: nothing is linearised (every thread holds the same sum)
        if (p_eL2 <= B.eps3) { stop = 6; break; }
        double maxdiag, jte_inf, p_L2;
        linearise(maxdiag, jte_inf, p_L2);
        ++njev;
        if (jte_inf <= B.eps1) { stop = 1; break; }
        const double floor_ = 1e-9 * maxdiag;
        if (k == 0) mu = R == 2 ? B.tau : B.tau * maxdiag;
        for (;;) {
            double Dp_L2 = 0.0, dL = 0.0;
            const bool solved = attempt(mu, floor_, Dp_L2, dL);
            ++nsolve;
            if (solved) {
                if (Dp_L2 <= B.eps2 * B.eps2 * p_L2) { stop = 2; break; }
                if (Dp_L2 >= (p_L2 + B.eps2) / (EPSILON * EPSILON)) { stop = 4; break; }
                const double ftrial = objective();
                ++nfev;
                const double pDp_eL2 = 2.0 * ftrial;
                if (!isfinite(pDp_eL2)) { stop = 7; break; }
                const double dF = p_eL2 - pDp_eL2;
                const bool ok = dL > 0.0 && dF > 0.0;
                if (tid == 0 && B.hist && nh < B.hist_cap) {
                    double* h = (MEMBERS ? B.hist + mem * B.hist_ms : B.hist) + ((long long)C.comp * B.hist_cap + nh) * 4;
                    h[0] = mu; h[1] = Dp_L2; h[2] = ftrial; h[3] = ok ? 1.0 : 0.0;
                }
                ++nh;
                if (ok) {
                    double tmp = 2.0 * dF / dL - 1.0;
                    tmp = 1.0 - tmp * tmp * tmp;
                    mu = mu * (tmp >= ONE_THIRD ? tmp : ONE_THIRD);
                    nu = 2;
                    p_eL2 = pDp_eL2;
                    for (int i = tid; i < nfree; i += NT) psave[i] = x[fv[i]];   // (each thread its own entries: written and read by it alone)
                    break;
                }
            }
            mu *= (double)nu;
            const long long nu2 = nu << 1;
            if (nu2 >= (1ll << 31)) { stop = 5; break; }
            nu = nu2;
        }
        ++k;
    }
    if (!stop) stop = 3;
    __syncthreads();
    for (int i = tid; i < nfree; i += NT) {   // x = clamp(accepted point)
        const int v = fv[i];
        const double xv = psave[i], lo = B.lo[v], hi = B.hi[v];
        const double xc = xv < lo ? lo : (xv > hi ? hi : xv);   // (a NaN stays a NaN)
        x[v] = xc;
        if (MEMBERS) B.xout[mem * B.xout_ms + C.free0 + i] = xc;
    }
    const double fret = objective();
    if (tid == 0) {
        double* r = (MEMBERS ? B.res + mem * B.res_ms : B.res) + (long long)C.comp * LM_BATCH_RES;
        r[0] = fret; r[1] = finit; r[2] = k; r[3] = stop; r[4] = nfev; r[5] = njev; r[6] = nsolve; r[7] = mu;
        r[8] = C.nca; r[9] = npa; r[10] = (double)nh; r[11] = 0.0;
    }
}

template <int CLS>
hipError_t launch_class(hipStream_t stream, const BatchDev& B, int first, int count, int members) {
    if (count <= 0) return hipSuccess;
    const size_t lds = lm_batch_class_lds_doubles(CLS) * sizeof(double);
    if (B.xout) return launch_dyn(k_lm_batch<CLS, true>, dim3((unsigned)count, (unsigned)members), lm_batch_class_threads(CLS), lds, stream, B, first);
    return launch_dyn(k_lm_batch<CLS, false>, dim3((unsigned)count), lm_batch_class_threads(CLS), lds, stream, B, first);
}

#define LMB_CHK(expr)                                  \
    do {                                               \
        const hipError_t e_ = (expr);                  \
        if (e_ != hipSuccess) return (int)e_;          \
    } while (0)

}  // namespace

LmBatchWorkspace::~LmBatchWorkspace() {
    if (dev) (void)hipFree(dev);
}

int lm_batch_launch(hipStream_t stream, const LmBatchProblem& P, const void* tables, const LmBatchTableLayout& lay, const int (&n)[LM_BATCH_CLASSES],
                    const LmBatchOptions& opt, int64_t hist_cap, const LmBatchMembers& M) {
    const char* const base = static_cast<const char*>(tables);
    BatchDev B{};
    B.x = P.x; B.lo = P.lo; B.hi = P.hi; B.cam = P.cam; B.pt = P.pt; B.obs = P.obs;
    if (!M.xout && M.count != 1) return (int)hipErrorInvalidValue;   // (one member without strides, or members with all of them)
    B.x_ms = M.x_stride; B.ws_ms = M.ws_stride; B.res_ms = M.res_stride; B.hist_ms = M.hist_stride;
    B.xout = M.xout; B.xout_ms = M.xout_stride;
    B.comps = reinterpret_cast<const LmBatchComp*>(base + lay.comps);
    B.ints = reinterpret_cast<const int*>(base + lay.ints);
    B.free32 = reinterpret_cast<const int*>(base + lay.free32);
    B.order = reinterpret_cast<const int*>(base + lay.order);
    B.freem = reinterpret_cast<const unsigned char*>(base + lay.freem);
    B.res = M.res;
    B.hist = hist_cap > 0 ? M.hist : nullptr;
    B.ws = M.ws;
    B.R = opt.model; B.maxiters = opt.maxiters; B.hist_cap = hist_cap;
    B.tau = opt.tau; B.eps1 = opt.eps1; B.eps2 = opt.eps2; B.eps3 = opt.eps3;
    // one launch per class that occurs, its components heaviest first
    LMB_CHK(launch_class<3>(stream, B, n[0] + n[1] + n[2], n[3], M.count));
    LMB_CHK(launch_class<2>(stream, B, n[0] + n[1], n[2], M.count));
    LMB_CHK(launch_class<1>(stream, B, n[0], n[1], M.count));
    LMB_CHK(launch_class<0>(stream, B, 0, n[0], M.count));
    return 0;
}

int device_lm_batch(hipStream_t stream, const LmBatchProblem& P, const LmBatchTables& T, const LmBatchOptions& opt,
                    int64_t hist_cap, LmBatchWorkspace* ws, std::vector<double>* res, std::vector<double>* hist) {
    const size_t ncomp = T.comps.size();
    res->assign(ncomp * LM_BATCH_RES, 0.0);
    hist->clear();
    if (ncomp == 0) return 0;
    // One device block, kept by the caller between calls and grown on demand: the tables (one upload), the results
    // (one download), the history, the components' workspace slices.
    struct Part { size_t bytes, off; };
    const LmBatchTableLayout lay = lm_batch_table_layout(T);
    Part p_res{ncomp * LM_BATCH_RES * 8, 0}, p_hist{hist_cap > 0 ? ncomp * (size_t)hist_cap * 32 : 0, 0}, p_ws{(size_t)T.ws_doubles * 8, 0};
    size_t total = lay.bytes;
    for (Part* q : {&p_res, &p_hist, &p_ws}) {
        q->off = total;
        total += (std::max<size_t>(q->bytes, 8) + 255) / 256 * 256;
    }
    if (ws->dev_bytes < total) {
        LMB_CHK(hipStreamSynchronize(stream));
        if (ws->dev) { LMB_CHK(hipFree(ws->dev)); ws->dev = nullptr; ws->dev_bytes = 0; }
        LMB_CHK(hipMalloc(&ws->dev, total + total / 4));
        ws->dev_bytes = total + total / 4;
    }
    std::vector<char> stage(lay.bytes, 0);
    lm_batch_stage_tables(T, lay, stage.data());
    char* const base = static_cast<char*>(ws->dev);
    LMB_CHK(hipMemcpyAsync(base, stage.data(), lay.bytes, hipMemcpyHostToDevice, stream));

    // a launch of one member
    const LmBatchMembers M{0, reinterpret_cast<double*>(base + p_res.off), 0, reinterpret_cast<double*>(base + p_hist.off), 0,
                           reinterpret_cast<double*>(base + p_ws.off), 0, nullptr, 0, 1};
    const int n[LM_BATCH_CLASSES] = {(int)T.order[0].size(), (int)T.order[1].size(), (int)T.order[2].size(), (int)T.order[3].size()};
    if (int e = lm_batch_launch(stream, P, base, lay, n, opt, hist_cap, M)) return e;
    LMB_CHK(hipMemcpyAsync(res->data(), M.res, p_res.bytes, hipMemcpyDeviceToHost, stream));
    if (hist_cap > 0) {
        hist->resize(ncomp * (size_t)hist_cap * 4);
        LMB_CHK(hipMemcpyAsync(hist->data(), M.hist, p_hist.bytes, hipMemcpyDeviceToHost, stream));
    }
    LMB_CHK(hipStreamSynchronize(stream));
    return 0;
}

}  // namespace rdis_hip
