/*
 * rdis_hip.h -- C ABI of the MI355X (gfx950) subspace-solver path for RDIS.
 *
 * The reference has no FFI: its boundary for this path is C++ virtual dispatch,
 *     Numeric SubspaceOptimizer::optimize(const VariablePtrVec& vars,
 *         const FactorPtrVec& factors, NumericVec& xval, Numeric& deltaFval,
 *         const bool printdbg)                       (src/SubspaceOptimizer.h:37-39)
 * called from RDISOptimizer::getValueFromDomain (src/RDISOptimizer.cpp:1067) and
 * BCDOptimizer::optimize (src/optimizers/BCDOptimizer.cpp:149).  The drop-in
 * `rdis::HipCGDSubspaceOptimizer` (rdis_amd/host/) implements that virtual and
 * reaches the GPU only through the entry points below (plain pointers and sizes,
 * no C++ or torch types).  INTEGRATION.md shows the reference-side binding.
 *
 * Conventions
 *  - every function returns 0 or a negative RDIS_HIP_E* code; nothing throws
 *    across the ABI; rdis_hip_last_error() gives the text for the last failure
 *    on a context.
 *  - variable / factor ids are int64 like the reference's VariableID / FactorID
 *    (src/common.h:30-32): variable ids dense 0..N-1 in creation order, factor id
 *    = index in the function's factor list.  (Narrowed to int32 on the device;
 *    N, F and nnz must be < 2^31.)
 *  - the caller owns all host buffers; device memory belongs to the handles.
 *  - one context per GPU; calls on a context are serialised by the caller (the
 *    reference path is single-threaded and not re-entrant either).
 *  - fp64 throughout ("Numeric = double", src/common.h:25).
 *  - several contexts may be driven from one thread (one per GPU: rdis::OptimizableFunction::setDevices): every entry point
 *    makes its context's device current first.  Environment RDIS_HIP_VIRTUAL_DEVICES=n (a test aid for boxes with one GPU):
 *    rdis_hip_device_count() reports n devices that all stand on GPU 0, and every HIP call the library issues for a context
 *    while another context's device is the current one fails with RDIS_HIP_EDEVICE -- what a forgotten "make current" would
 *    do on a real node.
 */
#ifndef RDIS_HIP_H_
#define RDIS_HIP_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RDIS_HIP_ABI_VERSION 1

enum {
    RDIS_HIP_OK = 0,
    RDIS_HIP_EINVAL = -1,   /* bad argument (NULL, negative size, id out of range) */
    RDIS_HIP_ENOMEM = -2,   /* host or device allocation failed */
    RDIS_HIP_EDEVICE = -3,  /* HIP runtime error (no device, launch failure, ...) */
    RDIS_HIP_EOVERLAP = -4, /* components of a plan are not independent */
    RDIS_HIP_ERANGE = -5    /* size exceeds the int32 device index range */
};

/* exit reason of one component solve = status & 0xff; these replace the
 * exceptions / asserts the reference uses inside optimize()
 * (src/optimizers/CGDSubspaceOptimizer.cpp:42-58, :175;
 *  external/include/minimize_nrc.h:649,663,675,690,403) */
enum {
    RDIS_HIP_EXIT_FTOL = 0,         /* 2|df| <= ftol(|f|+|fp|+1e-18) */
    RDIS_HIP_EXIT_GTOL = 1,         /* scaled gradient below 1e-8 */
    RDIS_HIP_EXIT_GGZERO = 2,       /* gradient exactly zero */
    RDIS_HIP_EXIT_ITMAX = 3,        /* "Too many iterations in frprmn" (normal for BA) */
    RDIS_HIP_EXIT_DBRENT_ITMAX = 4, /* "Too many iterations in routine dbrent" */
    RDIS_HIP_EXIT_NAN = 5,          /* a NaN objective (the reference asserts) */
    RDIS_HIP_EXIT_EMPTY = 6,        /* empty factor list: returns 0, touches nothing */
    RDIS_HIP_EXIT_SYNC_TIMEOUT = 7  /* device-side barrier gave up (never expected) */
};
#define RDIS_HIP_STATUS_ROLLED_BACK 0x100 /* negative progress: initial x restored
                                             (CGDSubspaceOptimizer.cpp:66-80) */

typedef struct rdis_hip_ctx rdis_hip_ctx;
typedef struct rdis_hip_problem rdis_hip_problem;
typedef struct rdis_hip_plan rdis_hip_plan;

/* ---- context ------------------------------------------------------------------ */
int rdis_hip_abi_version(void);
int rdis_hip_device_count(void);
int rdis_hip_create(int device, rdis_hip_ctx **out);
void rdis_hip_destroy(rdis_hip_ctx *ctx);
const char *rdis_hip_last_error(const rdis_hip_ctx *ctx);
/* run on a caller-provided hipStream_t (NULL: the context's own stream) */
int rdis_hip_set_stream(rdis_hip_ctx *ctx, void *hip_stream);
int rdis_hip_synchronize(rdis_hip_ctx *ctx);
/* copy bytes from a device pointer handed out by this library to host memory
 * (for FFI callers without HIP bindings); ordered after prior work on the stream */
int rdis_hip_copy_to_host(rdis_hip_ctx *ctx, void *dst, const void *dev_src, int64_t bytes);

/* ---- an OptimizableFunction in packed form --------------------------------------
 * x0/lo/hi: assigned value and single-interval domain of every variable
 * (VariableDomain::interval(), src/VariableDomain.h:53; CGD asserts one
 * sub-interval, CGDSubspaceOptimizer.cpp:119).
 *
 * upload_ba replaces F BundleAdjustmentFactor objects
 * (src/bundleadjust/BundleAdjustmentFactor.h:18-31): factor i reads variables
 * cam_vid0[i]..+8 = [rx ry rz tx ty tz f k1 k2] and pt_vid0[i]..+2 = [X Y Z]
 * (BundleAdjustmentFunction.h:88-96) and the observation obs[2i], obs[2i+1]. */
int rdis_hip_upload_ba(rdis_hip_ctx *ctx, int64_t nvars, const double *x0, const double *lo,
                       const double *hi, int64_t nfac, const int64_t *cam_vid0,
                       const int64_t *pt_vid0, const double *obs, rdis_hip_problem **out);
/* upload_nlp replaces F NonlinearProductFactor objects
 * (src/NonlinearProductFactor.h:21-113): factor i = coeff[i] * prod over
 * k in [rowptr[i], rowptr[i+1]) of g((x[vid[k]] - cons[k])^expo[k]), g = sin iff sine[k].
 * Arithmetic: exponents 0, 1, 2 as the reference special-cases them (src/util/numeric.cpp:12-23), 3 and 4 by multiplication,
 * others through pow; sine and cosine by the library's own routine of the rotation angle (below 1 ulp) -- last-place differences
 * from std::pow / std::sin / std::cos, chosen so that a host can compute the same bits. */
int rdis_hip_upload_nlp(rdis_hip_ctx *ctx, int64_t nvars, const double *x0, const double *lo,
                        const double *hi, int64_t nfac, const double *coeff,
                        const int64_t *rowptr, const int64_t *vid, const double *expo,
                        const double *cons, const uint8_t *sine, rdis_hip_problem **out);
/* NonlinearProductFactor's useExponential (src/NonlinearProductFactor.h:62, 113): factor i with use_exp[i] != 0
 * evaluates to coeff[i] * exp(-product) (src/NonlinearProductFactor.cpp:140, 204).  Values only: the reference's
 * computeGradient asserts the flag off (.cpp:110), so eval_grad, plan_create and cgd_batch over a list that holds
 * such a factor return RDIS_HIP_EINVAL.  use_exp == NULL or all zero: cleared (the state after upload_nlp). */
int rdis_hip_nlp_set_exponential(rdis_hip_problem *p, const uint8_t *use_exp);
void rdis_hip_free_problem(rdis_hip_problem *p);

/* Variable::assign for already-assigned variables (src/Variable.cpp:66-88): the
 * constants an outer optimiser fixes before a solve.  vid == NULL: vid = 0..n-1. */
int rdis_hip_set_x(rdis_hip_problem *p, int64_t n, const int64_t *vid, const double *val);
int rdis_hip_get_x(rdis_hip_problem *p, int64_t n, const int64_t *vid, double *out);

/* ---- batched factor evaluation at the currently assigned x ----------------------
 * fac == NULL: all factors 0..nf-1 (nf must then equal the factor count).
 * eval      : OptimizableFunction::evalFactors (src/OptimizableFunction.cpp:95-135)
 * eval_grad : ... + computeGradient(facs, pg) (src/OptimizableFunction.cpp:234-262, the merge of src/State.h:157-210);
 *             g is dense over all N variables (0 where no listed factor touches it).  Bundle adjustment: one
 *             pass over the factors, no per-factor partial leaves the compute unit (rdis_amd/csrc/grad_fused.hpp);
 *             a point variable's contributions are added in factor-list order like the reference's merge, a camera
 *             variable's in factor-list order within a tile of the list and then tile by tile -- a fixed order, the
 *             same bits run to run; the value is bit for bit what eval returns for the same list.  The tables of
 *             a list are built at its first use and kept (up to 64 lists within 1 GiB of device memory, least recently used
 *             first to go; all factors: fac == NULL; an explicit list of at most 512 entries needs no tables and builds none).
 *             Nonlinear-product functions: per-factor partials, then each g[v] in factor-list order.
 * eval_grad_device : the same, results left on the device: *f_dev points to one double, *g_dev to N doubles,
 *             valid until the next evaluation call on this problem; asynchronous on the context's stream
 *             (rdis_hip_synchronize / rdis_hip_copy_to_host order after it).
 * eval_each / grad_each_ba: per-factor values / 12 partials, for kernel parity tests
 *             (Factor::eval, BundleAdjustmentFactor::computeGradient). */
int rdis_hip_eval(rdis_hip_problem *p, int64_t nf, const int64_t *fac, double *f);
int rdis_hip_eval_grad(rdis_hip_problem *p, int64_t nf, const int64_t *fac, double *f, double *g);
int rdis_hip_eval_grad_device(rdis_hip_problem *p, int64_t nf, const int64_t *fac, void **f_dev, void **g_dev);
int rdis_hip_eval_each(rdis_hip_problem *p, int64_t nf, const int64_t *fac, double *fvals);
/* how eval_each / grad_each_ba round a bundle-adjustment factor's arithmetic: 0 (default) = one fused multiply-add where the
 * model has a * b + c, 1 = every product rounded before it is added, like the reference's x86-64 build -- the arithmetic of the
 * solvers' parity option (plan option "factor_rounding" = 1), so that tests can compare it factor by factor, bit for bit,
 * with a CPU restatement (BundleAdjustmentFactor.cpp:160-185, 266-335) */
int rdis_hip_set_factor_rounding(rdis_hip_problem *p, int32_t mode);
int rdis_hip_grad_each_ba(rdis_hip_problem *p, int64_t nf, const int64_t *fac, double *g12);

/* ---- a second subspace solver: Levenberg-Marquardt (bundle adjustment) ---------------
 * The least-squares problem LMSubspaceOptimizer::optimize hands to levmar
 * (src/optimizers/LMSubspaceOptimizer.cpp:28-147, 176-278: residual sqrt(2 E_j) per factor,
 * Jacobian row grad E_j / e_j, damping scale 1e-3, eps1 = eps2 = 1e-15, eps3 = ftol, itmax =
 * maxiters, result clamped into the domains), solved on the device: normal equations in
 * camera / point blocks, Schur complement onto the cameras, both contractions on the matrix
 * cores (rdis_amd/csrc/lm_solver.hip).  levmar is not vendored by the reference: parity is
 * unpinned, the iteration is checked step by step against oracle/lm_oracle.py.
 * residual_model 1 is that formulation; 2 replaces it by the two pixel residuals of every
 * observation (the usual bundle-adjustment Gauss-Newton model: J^T J of rank 2 per factor instead
 * of 1, same machinery) -- not something the reference offers, far faster convergence.
 * Bits 4-5 of residual_model choose how the Schur product Z Z^T is formed: 0 = by fill (block-sparse over the
 * camera pairs that share a point where cameras see few of the points -- every BAL problem --, dense on the
 * matrix cores otherwise), 1 = dense, 2 = block-sparse.
 * Same calling convention as one component of rdis_hip_cgd_batch; x_inout may be NULL (start at
 * the currently assigned x; the result is left assigned either way).
 * info[8] = {iterations, stop code (levmar's: 1 small gradient, 2 small step, 3 itmax,
 * 4 singular, 5 no further reduction, 6 small error, 7 invalid values), residual evaluations,
 * Jacobian evaluations, linear solves, final damping mu, camera blocks, point blocks};
 * hist (may be NULL): up to hist_cap records {mu, |Dp|^2, f(trial), accepted} per linear solve.
 * A start at which the listed factors' value is not finite (a NaN coordinate; a point in a camera's plane) ends with
 * code 7 before anything is linearised: 0 iterations, 1 residual evaluation, no Jacobian evaluation, no linear solve, no
 * history record, fret not finite; a NaN coordinate is left NaN, every other free variable clamped into its domain as
 * always.  The same holds for every component of rdis_hip_lm_batch and of the plans below, whatever its class; the other
 * components of the call, and the other members or starts, are not affected.  (maxiters < 1 is RDIS_HIP_EINVAL in every
 * entry, so no call skips that test and returns code 3 for such a start.)
 * Listed factors that read no free variable of the call (or of a component) are not refused: the gradient is zero, the
 * solve ends with code 1 at iteration 0 (1 Jacobian evaluation, no linear solve), x = clamp(start), fret = the value at
 * the start.  A free camera or point block that no listed factor reads is damped like the others and gets the step 0. */
int rdis_hip_lm_optimize(rdis_hip_problem *p, int64_t nfree, const int64_t *free_vid, int64_t nf,
                         const int64_t *fac_id, double *x_inout, int32_t maxiters, double ftol,
                         int32_t residual_model, double *fret, double *delta, double *info8, double *hist4, int64_t hist_cap,
                         int64_t *nhist);

/* ---- the same solver for a batch of small independent components, in one launch per class -----
 * Component c is free_vid[free_ptr[c] .. free_ptr[c+1]) over fac_id[fac_ptr[c] .. fac_ptr[c+1]): the calling convention
 * of rdis_hip_cgd_batch (components must be independent, otherwise RDIS_HIP_EOVERLAP; x_inout concatenated in
 * free-variable order, NULL = start at the assigned x; the variables are left assigned to every component's clamped
 * result).  Each component is solved as rdis_hip_lm_optimize would solve it -- one run of oracle/lm_oracle.py's
 * lm_optimize -- by one workgroup that runs the whole iteration on the device (rdis_amd/csrc/lm_batch.hip): the number of
 * launches and stream waits of a call depends neither on ncomp nor on the iterations or rejected steps.
 * residual_model is 1 or 2 (bits 4-5 are ignored).  Bundle adjustment only.
 * Per component: fret[c], delta[c] (fret minus the listed factors' value at the start), info8[c][8], hist4[c][hist_cap][4]
 * and nhist[c] with the meaning they have for rdis_hip_lm_optimize; any output pointer may be NULL.  A component's results
 * do not depend, bit for bit, on the other components of the call or on its position among them.
 * Unlike rdis_hip_lm_optimize a component may have an empty factor list (rdis_hip_components produces them): it ends
 * with stop code 6, 0 iterations, fret 0 and x = clamp(start).
 * A component with more than RDIS_HIP_LM_BATCH_MAX_CAMERAS camera blocks that hold a free variable makes the whole call
 * fail with RDIS_HIP_ERANGE before anything is solved (the message names it): such a component belongs on
 * rdis_hip_lm_optimize.  Points and factors per component are not limited.  Two listed factors of a component that join the
 * same camera and point: RDIS_HIP_EINVAL.  Returns 0 also when components stop with codes 4, 5 or 7.
 *
 * RDIS_HIP_LM_WIDE, a bit of residual_model read by rdis_hip_lm_batch and rdis_hip_lm_plan_create (rdis_hip_lm_optimize
 * ignores it): components of 17 to RDIS_HIP_LM_WIDE_MAX_CAMERAS active camera blocks are solved too, as a fourth, wide class
 * -- the same iteration by one workgroup of 512 lanes, the reduced system (up to 576 unknowns) in the component's workspace
 * slice instead of the LDS, factorised in panels of 16 columns on the matrix cores.  Nothing changes for components of at
 * most 16 camera blocks: same class, same bits.  More than RDIS_HIP_LM_WIDE_MAX_CAMERAS: RDIS_HIP_ERANGE as above, the
 * message naming that limit.  A wide component needs up to 1.5 MB of workspace per member.
 * Which entry for which size: up to 64 cameras, many components or many population members at once -- this entry and its
 * plans with the bit set (one launch, no host traffic); one large component alone (full ladybug, 7776 points) --
 * rdis_hip_lm_optimize, whose launches use the whole device where a wide component has one workgroup. */
#define RDIS_HIP_LM_BATCH_MAX_CAMERAS 16
#define RDIS_HIP_LM_WIDE 0x100
#define RDIS_HIP_LM_WIDE_MAX_CAMERAS 64
int rdis_hip_lm_batch(rdis_hip_problem *p, int64_t ncomp, const int64_t *free_ptr, const int64_t *free_vid,
                      const int64_t *fac_ptr, const int64_t *fac_id, double *x_inout, int32_t maxiters, double ftol,
                      int32_t residual_model, double *fret, double *delta, double *info8, double *hist4,
                      int64_t hist_cap, int64_t *nhist);

/* ---- the step before the path: which independent sub-problems are there? -----
 * Connected components of the factor graph once the variables with assigned[v] != 0 are fixed:
 * what Component::createChildren (src/Component.cpp:508-549) obtains from the reference's dynamic
 * connectivity structure (ConnectivityGraph.h:255-261), computed on the device by a lock-free
 * union-find (rdis_amd/csrc/components.hip).  A component = unassigned variables connected
 * through factors.  Lists come out the way Component::init leaves them (Component.cpp:60-79):
 * variable ids ascending, factor ids ascending; components ordered by number of variables
 * ascending (ComponentComparator, Component.cpp:603-608), equal sizes by smallest variable id.
 * Factors all of whose variables are assigned are in no component; an unassigned variable that
 * no factor reads is a component with an empty factor list.  The four arrays are exactly the
 * arguments of rdis_hip_plan_create / rdis_hip_cgd_batch.
 *   rdis_hip_components        computes; returns the sizes
 *   rdis_hip_components_fetch  copies the lists of the last call (free_ptr, fac_ptr: ncomp + 1) */
int rdis_hip_components(rdis_hip_problem *p, const uint8_t *assigned, int64_t *ncomp, int64_t *nfree,
                        int64_t *nfac);
int rdis_hip_components_fetch(rdis_hip_problem *p, int64_t *free_ptr, int64_t *free_vid, int64_t *fac_ptr,
                              int64_t *fac_id);

/* ---- the solver: CGDSubspaceOptimizer::optimize for a batch of independent
 * components --------------------------------------------------------------------
 * Component c optimises the free variables free_vid[free_ptr[c] .. free_ptr[c+1])
 * over the factors fac_id[fac_ptr[c] .. fac_ptr[c+1]) (each list in the order the
 * reference would pass vars / factors).  Components must be independent: no
 * shared free variable and no factor of one reading a free variable of another
 * (they are connected components of the residual factor graph,
 * src/Component.cpp:508-549); otherwise RDIS_HIP_EOVERLAP.
 *
 * x_inout (free-variable order, concatenated over components): start values in,
 * final clamped values out; the problem's variables are left assigned to them
 * (post-condition of optimize(), CGDSubspaceOptimizer.cpp:84-86).  maxiters / ftol
 * are SubspaceOptimizer's SSmaxit / SSftol (src/SubspaceOptimizer.cpp:15-32).
 * Per component: fret (returned value), delta (deltaFval), iters (Frprmn::iter),
 * status (RDIS_HIP_EXIT_* | RDIS_HIP_STATUS_ROLLED_BACK), nfeval / ngeval (calls
 * of SubfunctionFD::operator() / ::df the reference would have made).  Any output
 * pointer may be NULL. */
int rdis_hip_cgd_batch(rdis_hip_problem *p, int64_t ncomp, const int64_t *free_ptr,
                       const int64_t *free_vid, const int64_t *fac_ptr, const int64_t *fac_id,
                       double *x_inout, int32_t maxiters, double ftol, double *fret,
                       double *delta, int32_t *iters, int32_t *status, int64_t *nfeval,
                       int64_t *ngeval);

/* The same in three steps, so that a decomposition is analysed and uploaded once
 * and solved many times with everything resident in HBM:
 *   plan_create : validate + upload the decomposition, build the per-variable
 *                 gather lists, allocate workspace
 *   plan_set_start : (optional) new start values, free-variable order; NULL = take
 *                 the problem's currently assigned x
 *   plan_solve  : reset the free variables to the start and run the solver
 *                 (asynchronous on the context's stream)
 *   plan_fetch  : wait and copy results out (any pointer may be NULL) */
int rdis_hip_plan_create(rdis_hip_problem *p, int64_t ncomp, const int64_t *free_ptr,
                         const int64_t *free_vid, const int64_t *fac_ptr, const int64_t *fac_id,
                         rdis_hip_plan **out);
void rdis_hip_plan_destroy(rdis_hip_plan *plan);
int rdis_hip_plan_set_start(rdis_hip_plan *plan, const double *x_start);
int rdis_hip_plan_solve(rdis_hip_plan *plan, int32_t maxiters, double ftol);
int rdis_hip_plan_fetch(rdis_hip_plan *plan, double *x_out, double *fret, double *delta,
                        int32_t *iters, int32_t *status, int64_t *nfeval, int64_t *ngeval);

/* ---- multi-start solves: one plan, many starting points, one launch -------------------
 * RDIS solves a decomposition again and again from other starting values (optBA's sample loop,
 * src/bundleadjust/optBA.cpp:198-224; a node's random restarts, src/RDISOptimizer.cpp:1087-1094; sampleRandomState,
 * :1196-1216).  plan_solve_starts solves every component of the plan from each of nstarts rows of start values
 * exactly as plan_solve would from that row -- the same bits --, one workgroup per (start, component) in one launch
 * (rdis_amd/csrc/solver_lds_starts.hpp; nonlinear-product plans: solver_wg_starts.hpp).  Variables that are not free in the plan are constants shared by all
 * starts, read from the problem's currently assigned x.
 *   x_starts[s][nfree_total]  row-major; a row is what plan_set_start takes (free-variable order, concatenated
 *                             over components); copied before the call returns
 *   x_out[s][nfree_total]; fret, delta, iters, status, nfeval, ngeval [s][ncomp]; best[ncomp]
 * plan_solve_starts is asynchronous on the context's stream; plan_fetch_starts waits and copies out (any pointer
 * may be NULL); the outputs of all starts are kept until the next plan_solve_starts or plan_solve_population.
 * State afterwards -- what an RDIS node keeps of its restarts, the minimum: best[c] is the start with the lowest
 * fret[s][c] (the lowest index on a tie; a NaN is never best unless every start of the component is one: then 0);
 * the free variables of component c are left assigned to that start's result (a following
 * plan_set_start(plan, NULL) continues from it; an empty component's variables are not touched, as in plan_solve),
 * and the plan's ordinary outputs -- plan_fetch, plan_objective_device and so the objective's all-reduce -- hold
 * the best start's row per component.  plan_last_kernel_ms covers the solver launches.
 * Memory: inputs and outputs for all nstarts starts, and replicas of the per-solve workspace (5 doubles per free
 * variable and one per partial, per start of a launch; on the plain batch solver also a copy of the problem's x and
 * of its search direction, 2 N doubles: that solver keeps its trial point in global memory), allocated at first use, kept with the plan and reported by
 * plan_device_bytes.  The plan option "starts_workspace_bytes" (default 1 GiB) bounds the replicas: when nstarts do
 * not fit, the call runs in several launches of R starts each, R the largest count that fits (at least 1, at most
 * 65535), the last one possibly with fewer; plan_get_info "starts_per_launch" and "starts_launches" tell R and the
 * number of launches of the last call.
 * Scope: every component of the plan goes to the LDS-resident solver (bundle adjustment; plan_get_info
 * "components_lds"), or the problem is a nonlinear-product one and every component goes to the plain batch solver
 * ("components_plain": BASELINE configs 1 and 2, every decomposition of the sinusoid); components without factors
 * count as either.  Not yet: the cooperative, grid, tiny-component and point-major solvers, bundle-adjustment
 * components on the plain batch solver (their rotation records would need replicas too), transient plans.  With the
 * default factor_rounding and emulate_stale_cache, trace_records and dump_iters off; nstarts >= 1; plan_fetch_starts needs a plan_solve_starts before it.  Anything
 * else: RDIS_HIP_EINVAL and a message that names the cause; the plan stays usable. */
int rdis_hip_plan_solve_starts(rdis_hip_plan *plan, int64_t nstarts, const double *x_starts,
                               int32_t maxiters, double ftol);
int rdis_hip_plan_fetch_starts(rdis_hip_plan *plan, double *x_out, double *fret, double *delta,
                               int32_t *iters, int32_t *status, int64_t *nfeval, int64_t *ngeval,
                               int32_t *best);
/* ---- populations: S complete states on the device, a plan solved on all of them at once ----
 * RDIS's restarts draw a whole state and then run the decomposition on it: fix a separator, solve the children, swap,
 * repeat (optBA's sample loop, src/bundleadjust/optBA.cpp:198-224; sampleRandomState, src/RDISOptimizer.cpp:1196-1216).
 * From the second half-round on the constants of sample s are sample s's own results, which plan_solve_starts -- constants
 * shared by all starts -- cannot express.  A population holds X[nmembers][N] on the device, every member a complete
 * assignment of the problem's variables; plan_solve_population runs a plan on all members in one launch, member s taking
 * both its start and its constants from X[s] and leaving its result there, so that the next plan (the other variables
 * free) follows with no host traffic (rdis_amd/csrc/solver_lds_population.hpp; nonlinear-product plans, with the plan
 * option "population_plain": solver_wg_population.hpp; bundle-adjustment plans with tiny components, with the plan option
 * "population_tiny": solver_quad_population.hpp; components too large for the LDS, on the point-major streaming solver, with
 * the plan option "population_point_major": solver_ptm_population.hpp).
 *   population_create   allocates X; x[nmembers][N] row-major, or NULL: every member a copy of the problem's currently
 *                       assigned x.  nmembers >= 1 (RDIS_HIP_EINVAL), below 2^31 and nmembers * N below 9e15
 *                       (RDIS_HIP_ERANGE).  Both problem kinds.  A population belongs to one problem and is destroyed
 *                       before it.  Its device memory is its own (not in any plan_device_bytes).
 *   population_set_x / _get_x   members first .. first + count - 1, n values each: val / out [count][n] row-major;
 *                       vid == NULL: variables 0..n-1 (n <= N); ids and ranges checked like rdis_hip_set_x.
 *   population_assign   the problem's assigned x := that member's x (asynchronous on the context's stream).
 *   population_eval     f[s], s < nmembers: bit for bit what rdis_hip_eval(p, nf, fac, .) returns when member s's x is the
 *                       assigned x -- the same statements with x replaced, the rotation records of a long bundle-adjustment
 *                       list rebuilt from the member's x --, all members enqueued without a wait, one copy back.  The
 *                       problem's assigned x and what eval_grad_device handed out are left as they were.  The members are a
 *                       dimension of the grid: per launch of R members one kernel for the chunk (or block) sums and one
 *                       final-sum workgroup per member, preceded on the rotation-records branch by the records of THAT
 *                       launch's members -- two or three kernels for the whole population, not per member.  The scratch
 *                       (R x partial sums, R x N records) is the population's own, bounded by the population option
 *                       "eval_workspace_bytes": R = min(nmembers, 65535, max(1, bytes / bytes per member)), ceil(nmembers / R)
 *                       launches, the same bits however it is split.  The problem's scalar, partial sums and rotation
 *                       records are not written.
 *   population_eval_device   the same evaluation left on the device: *f_dev points at f[nmembers], valid until the next
 *                       evaluation of the population.  With fac == NULL nothing is waited for; an explicit list is staged
 *                       like every id list (one synchronisation).
 *   population_best     the argmin of the last evaluation: member and its value.  The rule is plan_solve_starts' selection:
 *                       the lowest value; on a tie (-0.0 against +0.0 is one) the lowest index; a NaN never, unless every
 *                       value is one: then member 0.  Selected on the device; one copy of 16 bytes and one synchronisation.
 *   population_assign_best   the same selection, then the problem's assigned x := X[best], the index read on the device:
 *                       enqueued, no wait, no host round trip.  Afterwards the problem is as population_assign(best) leaves it.
 *                       So rounds x (plan_solve_population ..., population_eval_device, population_assign_best) run without
 *                       a synchronisation until the caller asks for a result.
 *                       best / assign_best refer to the last evaluation of this population (whatever list it took).
 *                       population_set_x and plan_solve_population write X and mark its values stale; before any evaluation
 *                       or with stale values both return RDIS_HIP_EINVAL ("evaluate first") and change nothing.
 *                       population_assign, _get_x and evaluations do not invalidate.
 *   population_set_option   "eval_workspace_bytes" (default 2^30, the default of "starts_workspace_bytes"; >= 0; lowering it
 *                       releases scratch beyond it), "eval_batched" (default 1; 0 = the evaluation member by member through
 *                       the problem's scratch, two or three launches a member: the yardstick of the batched path),
 *                       "grad_workspace_bytes" (population_eval_grad below; default 2^30; >= 0; lowering it releases scratch).
 *   population_get_info     "eval_members_per_launch" (R of the last evaluation), "eval_launches" (kernels it launched),
 *                       "eval_valid" (1: best / assign_best are served); "grad_members_per_launch", "grad_launches" and
 *                       "grad_branch" of the last gradient call (population_eval_grad below); "nmembers" and "problem_handle"
 *                       (the population's rdis_hip_problem* as an integer: what a caller that is handed a population compares
 *                       with its own problem before it writes a row).  Unknown names: RDIS_HIP_EINVAL.
 *   plan_solve_population   asynchronous on the context's stream.  For every member s and component c exactly what
 *                       plan_set_start(plan, NULL) + plan_solve would do on a problem whose assigned x is X[s] -- the same
 *                       bits in fret, delta, x, iters, status, nfeval, ngeval: the start is X[s][free_vid], clamped at
 *                       entry; the constants are X[s][v] for the other variables the component's factors read; the result
 *                       (clamped; after a rollback clamp(x_init)) is assigned into X[s][free_vid]; an empty component's
 *                       variables are untouched, its status RDIS_HIP_EXIT_EMPTY.  Writing into X[s] needs no replica of
 *                       it: the components of a plan are independent (plan_create: RDIS_HIP_EOVERLAP), so a variable one
 *                       workgroup of member s writes is read by no other workgroup of member s.  The problem's own x, the
 *                       plan's ordinary outputs (plan_fetch, plan_objective_device) and start are not touched.
 *   plan_fetch_population   waits and copies out (any pointer may be NULL): x_out[s][nfree_total]; fret, delta, iters,
 *                       status, nfeval, ngeval [s][ncomp].  The outputs are kept until the next plan_solve_population or
 *                       plan_solve_starts on the plan, whose buffers they share: plan_fetch_starts after a population
 *                       solve, and plan_fetch_population after a multi-start solve or before any, return RDIS_HIP_EINVAL.
 * Workspace: the replicas of the multi-start entry on the LDS-resident solver (5 doubles per free variable and one per
 * partial, per member of a launch; on the plain batch solver also a search direction of the problem's size, N doubles,
 * but no copy of x: that solver's trial points go into the member's own row X[s], which the independence of the
 * components allows just as it allows the result), bounded by the plan option "starts_workspace_bytes" with the same
 * splitting into launches of R members (plan_get_info "starts_per_launch" / "starts_launches"), counted by
 * plan_device_bytes; plan_last_kernel_ms covers the solver launches.  With "population_tiny" a replica holds only what
 * the launch's kernels read: the rotation records of the member's cameras (N doubles) where the tiny-component solver reads
 * records (cameras constant in the whole plan, "camera_records" not 0), the LDS-resident solver's part only where that solver
 * has components in the plan -- a plan of points alone with "camera_records" = 0 needs no replica and is never split below
 * 65535 members; every member of a launch also has a 4-byte queue counter.  A launch of R members is then one launch of the
 * tiny-component solver (its grid: blocks per member x R, plan_get_info "population_tiny_blocks") followed, where the plan has
 * other components, by one of the LDS-resident solver; "starts_launches" and plan_last_kernel_ms count both.  With
 * "population_point_major" a member of a launch also has a replica of the point-major solver's four per-solve arrays -- p and
 * xi, g and h, the exact bounds (six doubles a point block each) and the wave-chunks' float boxes: 144 bytes per point block of
 * the plan's point-major components and 32 per entry of their chunk tables, 1.1 MB a member for full ladybug as one component
 * -- under the same bound and splitting; a launch of R members is then the tiny-component launch (where the plan has tiny
 * components), the point-major kernel on a grid of (its components, R), and the LDS-resident kernel (where that solver has
 * components), in this order, every one counted.
 * Scope: a bundle-adjustment problem, every non-empty component of the plan on the LDS-resident solver (plan_get_info
 * "components_lds"); or, with the plan option "population_plain" = 1 (default 0: refused, as before the option existed), a
 * nonlinear-product problem with every non-empty component on the plain batch solver ("components_plain": BASELINE
 * configs 1 and 2, every decomposition of the sinusoid) -- the option has no effect on bundle-adjustment plans; or, with
 * the plan option "population_tiny" = 1 (default 0: refused, as before the option existed), a bundle-adjustment problem whose
 * non-empty components run on the tiny-component solver ("components_tiny": a point against constant cameras and the like) or
 * on the LDS-resident solver, in any mix; the lanes per tiny component are plan_solve's ("quad_min_components",
 * "row_min_components": the bits depend on them); and, with the plan option "population_point_major" = 1 (default 0: refused,
 * as before the option existed), also components on the point-major streaming solver ("components_point_major": too large for
 * a compute unit's LDS -- full ladybug as one component, each component of BASELINE config 5-L) as ONE workgroup per component
 * and member, beside the others in any mix.  The contract is plan_solve's bits, and a group of workgroups per component adds
 * every sum in another order: the plan is taken only where plan_solve would run one workgroup per component (the plan option
 * "ptm_group" = 1; the lanes are "ptm_threads", else 768: plan_get_info "population_point_major_threads"), otherwise
 * RDIS_HIP_EINVAL with a message that names "ptm_group" and the group size plan_solve would pick.  A
 * persistent plan; default factor_rounding; emulate_stale_cache, trace_records and dump_iters off; the population must be
 * the plan's problem's.  Not yet: the grid solver and point-major components shared by several workgroups (the cooperative
 * solver: plan_solve_population_cooperative, below);
 * bundle-adjustment components on the plain batch solver; tiny and point-major components in plan_solve_starts.  Anything
 * else: RDIS_HIP_EINVAL and a message that names the cause; the plan and the population stay usable.
 *
 * A restart loop on one stream: draw -> solve -> evaluate -> rank -> keep -> redraw -> solve, nothing crossing to the host until
 * the caller asks for a result (rdis_amd/csrc/population_select.hpp; examples/ba_population_halving.py).
 *   population_set_sampling   lo[N], hi[N]: the intervals random states are drawn from (VariableDomain::getSamplingInterval),
 *                       copied once and kept on the device with the population (2 N doubles).  Both NULL: the problem's
 *                       domains, the state before the first call.  One of them NULL, a non-finite bound or lo[v] > hi[v]:
 *                       RDIS_HIP_EINVAL, the message names the first such variable, nothing changes.
 *   population_sample   members first .. first + count - 1 at the variables vid[0 .. n) (vid == NULL: variables 0 .. n-1,
 *                       n <= N; ranges checked like population_set_x) are drawn on the device:
 *                       X[s][v] = closestVal_v(slo[v] + u (shi[v] - slo[v])), u = (double)(z >> 11) 2^-53, z = splitmix64 of
 *                       seed + 0x9E3779B97F4A7C15 (stream + 1) + 0xBF58476D1CE4E5B9 (s + 1) + 0x94D049BB133111EB (v + 1) --
 *                       HipRDISLevelOptimizer::restartValue(seed, node = stream, restart = s, vid = v, dom) bit for bit (the
 *                       product is rounded before it is added, as the host's is), s the member's absolute row, closestVal
 *                       clamping into the problem's lo / hi.  A value depends on (seed, stream, s, v) only -- not on how a
 *                       range is cut into calls.  stream in [0, 2^31 - 2] (RDIS_HIP_EINVAL otherwise) is what a caller
 *                       varies from round to round.  Asynchronous on the context's stream: with vid == NULL nothing is
 *                       waited for; an explicit list is staged like every id list (one synchronisation).  Marks the
 *                       evaluation stale, as population_set_x does.
 *   population_sort     puts the members into the order of their last evaluation -- best's rule as a total order: numbers
 *                       ascending, a tie (-0.0 against +0.0 is one) by lower index, NaNs last by index.  With order[r] the
 *                       member of rank r, afterwards X_new[r] = X_old[order[r]] and f_new[r] = f_old[order[r]]: a pure
 *                       permutation, the evaluation stays valid ("eval_valid" stays 1, the address population_eval_device
 *                       handed out holds the permuted values), population_best returns member 0 and population_assign_best
 *                       assigns row 0.  Before any evaluation or with stale values: RDIS_HIP_EINVAL ("evaluate first").
 *                       order_out == NULL: enqueued, no wait; otherwise order_out[nmembers] is copied out (one
 *                       synchronisation).  What a plan kept of an earlier solve (plan_fetch_population) refers to the members
 *                       as they were numbered when that solve ran.  Memory: the permuted rows go into a second buffer of X's
 *                       size, allocated at the first sort -- the population's device memory doubles from then on -- and the
 *                       two buffers swap roles; RDIS_HIP_ENOMEM at that allocation leaves the population as it was.  Rank by
 *                       counting is quadratic in the members: nmembers > 2^18 returns RDIS_HIP_ERANGE before anything is
 *                       launched.
 *   population_permute  the members put into an order the caller chose: order[nmembers] a permutation of 0 .. nmembers - 1,
 *                       afterwards X_new[r] = X_old[order[r]] (what a driver does whose members stop at different times: the
 *                       active ones to the front, so that the solves' contiguous member range covers exactly them).  With a
 *                       valid last evaluation f_new[r] = f_old[order[r]] and it stays valid, as after population_sort; stale
 *                       values stay stale.  The kernel, the second buffer, its memory note and RDIS_HIP_ENOMEM are
 *                       population_sort's.  order is copied before the call returns (staged like every id list: one
 *                       synchronisation); the permutation itself is enqueued.  order NULL, an entry out of range or a member
 *                       named twice -- all checked on the host before anything is launched: RDIS_HIP_EINVAL with a message,
 *                       nothing changed.
 *   plan_solve_population_range   plan_solve_population restricted to members first .. first + count - 1: every (member,
 *                       component) of the range gets the bits a whole-population solve leaves for that member, the rows
 *                       outside the range are untouched.  count >= 1 and the range inside the population, else
 *                       RDIS_HIP_EINVAL.  plan_fetch_population afterwards returns [count][...] arrays, row i belonging to
 *                       member first + i.  The splitting by "starts_workspace_bytes" ("starts_per_launch" /
 *                       "starts_launches" of count members), plan_last_kernel_ms and every refusal are the whole-population
 *                       entry's.
 *   plan_solve_population_cooperative   plan_solve_population_range for plans with components on the cooperative solver,
 *                       single large components and group mode alike (plan_get_info "components_cooperative"; ladybug's
 *                       separator, its camera level), which the two entries above refuse: a cooperative group per (member,
 *                       component), the groups of all members of a launch side by side in one cooperative launch per launch of
 *                       the plan's ordinary solve (rdis_amd/csrc/solver_coop_population.hpp).  Every (member, component) gets the
 *                       bits rdis_hip_plan_solve leaves on a problem whose x is that member's -- in the plain cooperative
 *                       layout and, since the pipelined layout returns the same bits, in that one too.  The plan's other
 *                       components (tiny, point-major, LDS-resident) follow as in plan_solve_population, under the options that
 *                       admit them there; everything runs on the context's stream.  A member of a launch has replicas of the
 *                       solver's gfac and published directions and an exchange state a group (0.5 MiB each), the plan's own,
 *                       within "starts_workspace_bytes"; the problem's exchange state is not used.  Every workgroup of a
 *                       cooperative launch must be resident, so the members of a launch are bounded a second time:
 *                       R workgroups-a-member <= the resident workgroups of the kernel (plan_get_info
 *                       "population_cooperative_workgroups", "population_cooperative_cap"; "starts_per_launch" is R,
 *                       "starts_launches" the kernel launches).  No bit depends on R.  Refused, RDIS_HIP_EINVAL with a
 *                       message, before any row is written: a plan whose ordinary solve uses the pipelined layout (set the plan
 *                       option "coop_pipeline" = 0), components on the grid solver, and what plan_solve_population refuses
 *                       ("factor_rounding" = 1, "emulate_stale_cache", "trace_records", "dump_iters", a transient plan, another
 *                       problem's population).  rdis_hip_plan_solve_starts has no such form.
 *
 * The members' gradients, the member a grid dimension (computeGradient(facs, pg) on every member at once):
 *   population_eval_grad   f[count] and g[count][N], row-major, for members first .. first + count - 1; nf / fac as in
 *                       rdis_hip_eval_grad (fac == NULL: all factors).  Row k holds, bit for bit, what rdis_hip_eval_grad(p, nf,
 *                       fac, ...) returns on a problem whose assigned x is X[first + k], exact zeros where no listed factor
 *                       reads included.  The range is checked like population_set_x's; count == 0 succeeds and does nothing;
 *                       count N beyond what population_create accepts: RDIS_HIP_ERANGE.  nf == 0: zeros in both, no kernel.
 *                       Refusals are rdis_hip_eval_grad's (the list's form; an exponential factor; a tile's cameras that do
 *                       not fit the LDS), each with a message.  The form is rdis_hip_eval_grad's for the list
 *                       (population_get_info "grad_branch": 0 none, 1 the fused pass, 2 a list of one chunk, 3 two passes);
 *                       the list's tables are shared by the members (and cached with the problem, as rdis_hip_eval_grad's
 *                       are), every member of a launch has scratch of its own, the population's -- camera records, staging
 *                       arrays and chunk sums (fused), the per-factor partials and value partials (the others): rdis_amd/csrc/
 *                       population_grid.hpp, grad_member_bytes -- within the option "grad_workspace_bytes" (default 2^30;
 *                       negative: RDIS_HIP_EINVAL; lowering it releases scratch beyond it): R = min(count, 65535, max(1,
 *                       bound / bytes per member)) members a round ("grad_members_per_launch"), ceil(count / R) rounds of
 *                       three or four kernels ("grad_launches" counts them).  No bit depends on R.  Not written: X, the
 *                       values, "eval_valid" and the best member of the last population_eval; the problem's x and the
 *                       scratch and results of its own evaluation entries (the pointers rdis_hip_eval_grad_device handed
 *                       out keep their contents).
 *   population_eval_grad_device   the same, left on the device: *f_dev -> f[count], *g_dev -> g[count][N], buffers of the
 *                       population, grown on demand, valid until the next gradient call on this population or its
 *                       destruction.  Enqueued on the context's stream; nothing is waited for but what a list's first use
 *                       waits for (its tables; the staging of an explicit list).  population_eval_grad is this entry, two
 *                       copies and one synchronisation.
 *   population_grad_max   gmax[k] = max_i |g[k][i]| for every row k of the last gradient call (NaN if an entry of the row is
 *                       one), exact: its bits do not depend on the reduction.  gmax (host, [rows]) and gmax_dev (the address
 *                       of the population's buffer; enqueued, no wait) may each be NULL.  It describes the rows as that call
 *                       left them -- a later population_set_x, _sort, _sample or solve does not change it.  Before any
 *                       gradient call: RDIS_HIP_EINVAL ("evaluate the gradient first"). */
typedef struct rdis_hip_population rdis_hip_population;
int rdis_hip_population_create(rdis_hip_problem *p, int64_t nmembers, const double *x, rdis_hip_population **out);
void rdis_hip_population_destroy(rdis_hip_population *pop);
int rdis_hip_population_set_x(rdis_hip_population *pop, int64_t first, int64_t count, int64_t n, const int64_t *vid,
                              const double *val);
int rdis_hip_population_get_x(rdis_hip_population *pop, int64_t first, int64_t count, int64_t n, const int64_t *vid,
                              double *out);
int rdis_hip_population_assign(rdis_hip_population *pop, int64_t member);
int rdis_hip_population_eval(rdis_hip_population *pop, int64_t nf, const int64_t *fac, double *f);
int rdis_hip_population_eval_device(rdis_hip_population *pop, int64_t nf, const int64_t *fac, void **f_dev);
int rdis_hip_population_best(rdis_hip_population *pop, int64_t *member, double *f);
int rdis_hip_population_assign_best(rdis_hip_population *pop);
int rdis_hip_population_set_option(rdis_hip_population *pop, const char *name, int64_t value);
int rdis_hip_population_get_info(rdis_hip_population *pop, const char *name, int64_t *value);
int rdis_hip_population_set_sampling(rdis_hip_population *pop, const double *lo, const double *hi);
int rdis_hip_population_sample(rdis_hip_population *pop, int64_t first, int64_t count, int64_t n, const int64_t *vid,
                               uint64_t seed, int64_t stream);
int rdis_hip_population_sort(rdis_hip_population *pop, int64_t *order_out);
int rdis_hip_population_permute(rdis_hip_population *pop, const int64_t *order);
int rdis_hip_population_eval_grad(rdis_hip_population *pop, int64_t first, int64_t count, int64_t nf, const int64_t *fac,
                                  double *f, double *g);
int rdis_hip_population_eval_grad_device(rdis_hip_population *pop, int64_t first, int64_t count, int64_t nf,
                                         const int64_t *fac, void **f_dev, void **g_dev);
int rdis_hip_population_grad_max(rdis_hip_population *pop, double *gmax, void **gmax_dev);
int rdis_hip_plan_solve_population(rdis_hip_plan *plan, rdis_hip_population *pop, int32_t maxiters, double ftol);
int rdis_hip_plan_solve_population_range(rdis_hip_plan *plan, rdis_hip_population *pop, int64_t first, int64_t count,
                                         int32_t maxiters, double ftol);
int rdis_hip_plan_solve_population_cooperative(rdis_hip_plan *plan, rdis_hip_population *pop, int64_t first, int64_t count,
                                               int32_t maxiters, double ftol);
int rdis_hip_plan_fetch_population(rdis_hip_plan *plan, double *x_out, double *fret, double *delta, int32_t *iters,
                                   int32_t *status, int64_t *nfeval, int64_t *ngeval);
/* sum of fret over the plan's components, left on the device (for the RCCL
 * all-reduce of the top-level objective, src/RDISOptimizer.cpp:1491-1494);
 * returns a device pointer to one double valid until the next plan_solve. */
int rdis_hip_plan_objective_device(rdis_hip_plan *plan, void **dev_ptr);

/* ---- Levenberg-Marquardt plans: rdis_hip_lm_batch's tables built once, solves that stay on the stream -----
 * rdis_hip_lm_batch does a plan's work in every call: it checks the lists, builds and uploads the components' tables,
 * downloads the results and waits.  A rdis_hip_lm_plan does the first two once (the tables do not depend on x) and leaves
 * the last two to a fetch: between create and fetch nothing is copied, allocated (after the first solve) or waited for, so
 * an alternation of camera and point plans runs on the stream from end to end.
 *   rdis_hip_lm_plan_create   everything rdis_hip_lm_batch checks before it assigns x, with its codes (messages are
 *                             labelled lm_plan_create): bundle adjustment only, residual_model 1 or 2, RDIS_HIP_EOVERLAP,
 *                             ids in range, more than RDIS_HIP_LM_BATCH_MAX_CAMERAS active camera blocks RDIS_HIP_ERANGE
 *                             (with RDIS_HIP_LM_WIDE in residual_model: more than RDIS_HIP_LM_WIDE_MAX_CAMERAS),
 *                             two listed factors joining one camera and point RDIS_HIP_EINVAL.  hist_cap: history records
 *                             kept per component (0: none)
 *   rdis_hip_lm_plan_solve    every component from the problem's currently assigned x, the clamped results left assigned:
 *                             at most four launches (one per class that occurs); bit for bit rdis_hip_lm_batch with
 *                             x_inout = NULL
 *   rdis_hip_lm_plan_fetch    waits, then the last solve's outputs with the shapes and meaning of rdis_hip_lm_batch's
 *                             (hist4[c][hist_cap][4] with the plan's hist_cap); x_out: the solve's clamped results,
 *                             concatenated in free-variable order, kept by the plan beside the other outputs -- what the
 *                             solve left assigned, whatever was assigned since.  Any pointer may be NULL
 *   rdis_hip_lm_plan_solve_population   members first .. first + count - 1 of a population of the same problem, the member
 *                             the grid's second dimension: member s starts from X[s], reads its constants there and is
 *                             left at its clamped result -- what rdis_hip_lm_batch leaves on a problem whose x is X[s], bit
 *                             for bit.  Other rows and the problem's x are untouched; the population's values become stale
 *                             (rdis_hip_population_best: evaluate first).  RDIS_HIP_EINVAL: another problem's population,
 *                             count < 1, a range out of bounds.  No wait
 *   rdis_hip_lm_plan_fetch_population   the same outputs, [count][ncomp]...; row i is member first + i; x_out [count][nfree]
 *                             comes from the plan's own outputs too: the population may have been written or destroyed since
 *   A fetch that does not match the kind of the last solve, or before any solve: RDIS_HIP_EINVAL, nothing changed.
 *   rdis_hip_lm_plan_set_option   "workspace_bytes" (default 2^30, >= 0): bounds the workspace replicas of one population
 *                             launch; a solve of more members than fit is split into launches (at least one member
 *                             each), the same bits whatever the split
 *   rdis_hip_lm_plan_get_info "members_per_launch", "launches" (of the last solve), "device_bytes", "workspace_bytes",
 *                             "member_workspace_bytes" (one member's workspace replica)
 *
 * Multi-start solves: what an RDIS node keeps of its random restarts (RDISOptimizer.cpp:1087-1094), with Levenberg-Marquardt.
 *   rdis_hip_lm_plan_solve_starts   x_starts[nstarts][nfree], a host array in the plan's free-variable order, copied before
 *                             the call returns.  Start s solves every component from the problem's currently assigned x
 *                             with the plan's free variables replaced by row s; variables that are not free in the plan
 *                             are constants all starts share.  Every (start, component) is bit for bit what
 *                             rdis_hip_lm_batch with x_inout = NULL returns and leaves on a problem whose x is that vector.
 *                             Afterwards best[c] is the start with the lowest fret[s][c] (the lowest index on a tie; a NaN
 *                             never, unless every value is one: then 0), the free variables of component c are assigned
 *                             that start's clamped result, and the plan's ordinary outputs hold the winner's row per
 *                             component: rdis_hip_lm_plan_fetch returns them, its x_out is what was left assigned.  The
 *                             solves run on scratch rows: no other variable of the problem is written at any time.  The
 *                             starts of one launch are bounded by "workspace_bytes", a start charged
 *                             "member_workspace_bytes" + 8 nvars bytes; more starts run in rounds, the same bits whatever
 *                             the split ("members_per_launch", "launches": the solver's launches, classes x rounds; beside
 *                             them one small kernel a round and two at the end).  Nothing else is copied, nothing is waited
 *                             for, and after the first call of a size nothing is allocated.  RDIS_HIP_EINVAL: nstarts < 1,
 *                             x_starts NULL, maxiters < 1; RDIS_HIP_ERANGE: a start count that cannot be sized -- all before
 *                             anything is launched, copied or marked.  A plan of no component: 0, and nothing is done
 *   rdis_hip_lm_plan_solve_starts_population   the same solve, start s taken from row first + s of a population of the
 *                             plan's problem: only the plan's free variables are read from the row, the constants are still
 *                             the problem's x.  The population is only read -- its rows, its values and what
 *                             rdis_hip_population_best answers stay -- and no host memory is touched, so starts drawn with
 *                             rdis_hip_population_sample never leave the device.  RDIS_HIP_EINVAL: another problem's
 *                             population, count < 1, a range out of bounds
 *   rdis_hip_lm_plan_fetch_starts   waits, then all starts' outputs, [nstarts][ncomp]... like
 *                             rdis_hip_lm_plan_fetch_population's, x_out[nstarts][nfree] and best[ncomp].  Any pointer may
 *                             be NULL.  RDIS_HIP_EINVAL after any other solve or before one; rdis_hip_lm_plan_fetch_population
 *                             after a multi-start solve likewise.  Nothing is changed by a refused fetch
 *   rdis_hip_lm_plan_objective_device   enqueues one kernel that sums fret over the plan's ordinary outputs -- after
 *                             rdis_hip_lm_plan_solve the solve's rows, after a multi-start solve the winners' -- in a fixed
 *                             order (one workgroup: a lane's stride in component order, a butterfly over the wave, the waves
 *                             in wave order); a device pointer to one double, valid until the plan's next solve.
 *                             RDIS_HIP_EINVAL before any solve and after a population solve
 *   rdis_hip_lm_plan_summary_device   enqueues one kernel (one workgroup) over the same rows and returns a device pointer to
 *                             RDIS_HIP_LM_SUMMARY_DOUBLES doubles, valid until the plan's next summary: what a caller that
 *                             alternates plans needs of a step without fetching every component's arrays --
 *                               [0] sum of fret   [1] sum of delta   [2] sum of iterations   [3] sum of residual evaluations
 *                               [4] sum of Jacobian evaluations   [5] sum of linear solves
 *                               [6..12] the number of components that ended with stop code 1..7
 *                               [13] the number of components whose fret is not finite   [14], [15] zero.
 *                             Every field is added in rdis_hip_lm_plan_objective_device's order, so [0] is that entry's double
 *                             bit for bit and the counts are exact.  Nothing a fetch returns is written.  No wait.
 *                             RDIS_HIP_EINVAL before any solve and after a population solve
 *   rdis_hip_lm_plan_summary  the same, then waits and copies the 128 bytes to out16 (through a pinned host image)
 *   rdis_hip_lm_plan_summary_population_device   the summary per member of the last rdis_hip_lm_plan_solve_population: enqueues
 *                             one kernel -- one workgroup per member, the member in the grid's x dimension, one launch for the
 *                             whole range however "workspace_bytes" split the solve -- and returns a device pointer to
 *                             [count][RDIS_HIP_LM_SUMMARY_DOUBLES] doubles, valid until the plan's next member summary.  Row i
 *                             belongs to member first + i of that solve's range and holds the 16 doubles above over that
 *                             member's result rows, every field added in rdis_hip_lm_plan_objective_device's order: bit for bit
 *                             what rdis_hip_lm_plan_summary returns after rdis_hip_lm_plan_solve on a problem whose x is that
 *                             member's.  Nothing a fetch returns is written.  No wait.  Valid after a population solve only:
 *                             before any solve and after rdis_hip_lm_plan_solve or a multi-start solve RDIS_HIP_EINVAL, nothing
 *                             changed (rdis_hip_lm_plan_summary and _objective_device keep refusing after a population solve)
 *   rdis_hip_lm_plan_summary_population   the same, then waits and copies the count x 128 bytes to out (through a pinned host
 *                             image of that size) */
#define RDIS_HIP_LM_SUMMARY_DOUBLES 16
typedef struct rdis_hip_lm_plan rdis_hip_lm_plan;
int rdis_hip_lm_plan_create(rdis_hip_problem *p, int64_t ncomp, const int64_t *free_ptr, const int64_t *free_vid,
                            const int64_t *fac_ptr, const int64_t *fac_id, int32_t residual_model, int64_t hist_cap,
                            rdis_hip_lm_plan **out);
void rdis_hip_lm_plan_destroy(rdis_hip_lm_plan *plan);
int rdis_hip_lm_plan_solve(rdis_hip_lm_plan *plan, int32_t maxiters, double ftol);
int rdis_hip_lm_plan_fetch(rdis_hip_lm_plan *plan, double *x_out, double *fret, double *delta, double *info8,
                           double *hist4, int64_t *nhist);
int rdis_hip_lm_plan_solve_population(rdis_hip_lm_plan *plan, rdis_hip_population *pop, int64_t first, int64_t count,
                                      int32_t maxiters, double ftol);
int rdis_hip_lm_plan_fetch_population(rdis_hip_lm_plan *plan, double *x_out, double *fret, double *delta, double *info8,
                                      double *hist4, int64_t *nhist);
int rdis_hip_lm_plan_solve_starts(rdis_hip_lm_plan *plan, int64_t nstarts, const double *x_starts, int32_t maxiters,
                                  double ftol);
int rdis_hip_lm_plan_solve_starts_population(rdis_hip_lm_plan *plan, rdis_hip_population *pop, int64_t first,
                                             int64_t count, int32_t maxiters, double ftol);
int rdis_hip_lm_plan_fetch_starts(rdis_hip_lm_plan *plan, double *x_out, double *fret, double *delta, double *info8,
                                  double *hist4, int64_t *nhist, int32_t *best);
int rdis_hip_lm_plan_objective_device(rdis_hip_lm_plan *plan, void **dev_ptr);
int rdis_hip_lm_plan_summary_device(rdis_hip_lm_plan *plan, void **dev_ptr);
int rdis_hip_lm_plan_summary(rdis_hip_lm_plan *plan, double *out16);
int rdis_hip_lm_plan_summary_population_device(rdis_hip_lm_plan *plan, void **dev_ptr);
int rdis_hip_lm_plan_summary_population(rdis_hip_lm_plan *plan, double *out /*[count][16]*/);
int rdis_hip_lm_plan_set_option(rdis_hip_lm_plan *plan, const char *name, int64_t value);
int rdis_hip_lm_plan_get_info(rdis_hip_lm_plan *plan, const char *name, int64_t *value);

/* ---- the path's one collective --------------------------------------------------------
 * Independent components of a recursion level are sharded over the GPUs of a node (rdis_amd/dist.py, DESIGN.md section 5:
 * no data-path collective); what the ranks exchange is the top-level objective -- the sum the reference forms on one host
 * (src/RDISOptimizer.cpp:1491-1494) -- one fp64 all-reduce over RCCL / xGMI, on the stream the solve ran on.
 *   comm_unique_id   rank 0 makes the 128-byte id the ranks of a communicator share (ncclGetUniqueId); the caller
 *                    distributes it (a file, a socket, MPI: its business)
 *   comm_create      one rank per process and GPU (ncclCommInitRank on the context's device); collective over the ranks
 *   comm_create_all  one process that drives several contexts (rdis::OptimizableFunction::setDevices): one communicator
 *                    per context, each on a different GPU (ncclCommInitAll)
 *   allreduce_objective      sum over the ranks of rdis_hip_plan_objective_device's double, in place, asynchronous on the
 *                    context's stream; sum_out != NULL: copied out (waits).  comm == NULL: a world of one.
 *   allreduce_objective_all  the same for the plans of one process's contexts (grouped: one thread drives every rank);
 *                    comms == NULL: the partial sums meet on the host in plan order (no RCCL, or one GPU listed twice)
 *   comm_allreduce_f64       a few doubles of host memory summed (op 0) or maximised (op 1) over the ranks: counters, and the
 *                    barrier + maximum of a timed region
 * RCCL is loaded when the first communicator is made (dlopen): a single-GPU user never maps it. */
#define RDIS_HIP_COMM_ID_BYTES 128
typedef struct rdis_hip_comm rdis_hip_comm;
int rdis_hip_comm_unique_id(void *id128);
int rdis_hip_comm_create(rdis_hip_ctx *ctx, int32_t world, int32_t rank, const void *id128, rdis_hip_comm **out);
int rdis_hip_comm_create_all(int32_t n, rdis_hip_ctx *const *ctxs, rdis_hip_comm **comms);
void rdis_hip_comm_destroy(rdis_hip_comm *comm);
int rdis_hip_allreduce_objective(rdis_hip_plan *plan, rdis_hip_comm *comm, double *sum_out);
int rdis_hip_allreduce_objective_all(int32_t n, rdis_hip_plan *const *plans, rdis_hip_comm *const *comms, double *sum_out);
int rdis_hip_comm_allreduce_f64(rdis_hip_comm *comm, double *inout, int32_t n, int32_t op);

/* tuning / introspection ---------------------------------------------------------- */
/* option names: "block_threads" (workgroup size of the per-component solver: 64, 128, 256, 512,
 * 768 or 1024; 0 = auto), "coop_min_factors" (bundle-adjustment components with at least this
 * many factors are solved by the multi-workgroup cooperative kernel, one launch each; 0 = never;
 * default 4096), "coop_max_components" (only when the plan has at most this many such
 * components, default 48 -- their groups are packed into launches of what is resident at once; a
 * plan with more of them is one batched launch, one workgroup per component), "coop_group_min_factors" (default 256: when the cooperative groups of ALL
 * components with at least this many factors fit the device together, each of them gets one and
 * they run side by side in one launch; 0 = off), "coop_workgroups" (cap, 0 = what fits),
 * "coop_threads" (128, 256 or 512), "coop_poll_delay" (x64 cycles between publishing and the
 * first granule sweep), "coop_poll_inflight" (pipelined groups, 0 or 1: 1 = a collector that had to wait
 * for its own lanes keeps several polls of the value+slope slot it sweeps in flight, one issued every
 * "coop_poll_stagger" x64 cycles (0 ... 64), and looks at each as it returns -- solver_pipe.hpp:
 * sweep_ring; 0 = one poll at a time; results do not depend on either), "coop_pipeline" (default 1: cooperative groups run with the control logic,
 * the exchange and the factor arithmetic on waves of their own, solver_pipe.hpp, whenever every
 * group of the plan fits that layout of 128 factor lanes per workgroup; 0 = the plain cooperative
 * kernel; same bits either way as long as every variable fed by more than 48 partials has a wave;
 * the environment variable RDIS_HIP_COOP_PIPELINE=0 / 1 sets the default for plans the caller does
 * not see, e.g. the transient one of rdis_hip_cgd_batch),
 * "coop_speculate" (default 1: the pipelined groups evaluate guesses at the following trial steps
 * of a line search ahead of the control logic; results do not depend on it), "force_stream" (send large components to the streaming grid solver even
 * when they fit the register-resident one; large components that do not fit, and large
 * nonlinear-product components, always go there),
 * "quad_max_vars" / "quad_min_components" / "row_min_components" (bundle-adjustment components
 * with at most quad_max_vars free variables, default and maximum 4, are solved by groups of four
 * lanes, sixteen per wave, when the plan has at least quad_min_components of them, default 16384;
 * by groups of sixteen lanes from row_min_components, default 4096; below that by a workgroup
 * each; 0 variables = never),
 * "camera_records" (bundle adjustment, batched launches: 1 = default -- when no camera variable is
 * free in the launch its factors read per-camera rotation records (angle, axis, sine, cosine,
 * computed once per camera) and form only the point partials; with free cameras and more than 2048
 * factors in a component the component rewrites the records of its cameras at every trial point;
 * 2 = records wherever possible; 0 = every factor forms its camera's rotation itself.  Results
 * are bit-identical in all three settings),
 * "tiny_max_blocks" (cap on the grid of the persistent tiny-component kernels, 0 = what is
 * resident; for tests),
 * "overlap_batch" (default 1: the batched launch of a plan runs on a second stream, concurrently
 * with its cooperative launches when those take at most half of the compute units),
 * "lds_resident" (bundle adjustment, default 1: a component of the batched launch whose variables --
 * free ones and the constants its factors read -- fit a compute unit's LDS keeps them there as slots,
 * solver_lds.hpp; 0 = never: such components run on the plain batch solver, bit-identical where the
 * slots are the free variables), "lds_threads" / "lds_rot" / "lds_camera_sums" (its workgroup size,
 * 0 = auto; rotation records in it, -1 = auto; 0 = camera partials through memory like the plain
 * solver, for bit-for-bit comparisons),
 * "lds_matrix" (default 0; 1 = the LDS-resident solver's line-search trials in matrix form, a camera's rotation matrix and its
 * derivative along the direction formed once per camera and trial point -- what the point-major streaming solver does; measured
 * slower here, where a component has a few hundred factors per camera: the records are one lane's chain in front of every trial),
 * "ptm_stream" (default 1: components too large for the LDS whose CAMERA blocks fit it stream their
 * point blocks from HBM once per trial point, solver_ptm.hpp; 0 = never, 2 = every component whose
 * tables fit), "ptm_threads" (its workgroup size: 0 = auto, 256, 512 or 768), "ptm_group" (workgroups
 * that share one such component when the launch has fewer components than compute units: 0 = auto,
 * 1 = never, k <= 16 = k; for the WIDE groups of at most eight large components -- a component too large for a
 * cooperative group whose cameras fit the LDS streams through this solver on as many workgroups of 512 lanes as are resident,
 * instead of the grid solver -- up to 512),
 * "ptm_round_slots" (the slots of factors a round of that solver's gradient pass evaluates and stages: 0 = two where the workgroup
 * has at most 512 lanes and the LDS holds their staging rows, else one; 1; 2 -- the same bits on chunks of even slot counts),
 * "ptm_local_cameras" (a wide group whose component has more cameras than a compute unit's LDS holds, about 125: every
 * workgroup keeps only the cameras its own contiguous share of the camera-sorted chunk order meets, under local numbers;
 * -1 = default: where the cameras do not fit; 0 = never: such a component takes the grid solver; 1 = every wide group, for
 * tests.  One such component a plan; falls back to the grid solver when a workgroup's cameras would not fit either),
 * "factor_rounding" (how the factor arithmetic rounds a * b + c: 0 = one fused multiply-add; 1 = the PARITY option: the product
 * is rounded before it is added, like the reference's x86-64 build (g++ emits no fused multiply-add), and EVERY sum of a solve is
 * added in the reference's order by one lane (or one wave feeding one lane): the objective over the listed factors
 * (OptimizableFunction.cpp:95-135), every variable's partials in factor-list order (State.h:157-210), a trial's slope as gradient
 * times direction over the variables in list order (Df1dim::df, minimize_nrc.h:439-447), gg and dgg of the Polak-Ribiere step
 * (minimize_nrc.h:665-672).  With it -- and "emulate_stale_cache" -- a solve returns, bit for bit (==: fret, x, iterations, call
 * counts), what the CPU oracle returns when its three named switches for the device's factor arithmetic are on (its own sine /
 * cosine of the rotation angle, two reciprocals in place of five quotients, the adjoint sweep in place of the reference's forward
 * chain: oracle/rdis_oracle.h RO_ARITH_*, RO_BA_DERIV_ADJOINT_DEVICE), on BASELINE configs 3 and 4, from x0, 25 iterations, no
 * re-synchronisation (tests/test_gpu_parity.py); and the end values over one-ulp starts pass the plain two-sample test against the
 * reference-faithful oracle.  A parity option, not a fast path: the LDS-resident batch solver pays a full gradient and four
 * sequential sums per trial, a cooperative group runs in the plain layout with two sequential sums per trial (full ladybug: 0.4 s a
 * solve instead of 2.5 ms); refused where other solvers would run; -1 = default: the cooperative solvers round like the reference
 * (4 % slower) and keep their parallel sums, the batch solvers fuse.  After 25 unconverged CG iterations the DISTRIBUTION of end
 * values over one-ulp starts depends on all of that: DESIGN.md section 6),
 * "emulate_stale_cache" (default 0; 1 = the reference's factor cache, Variable.cpp:66-76 and
 * Factor.h:228-234 -- a factor keeps its value while its variables have moved by less than 1e-12 since
 * it was computed -- emulated in the LDS-resident batch solver and, with factor_rounding = 1, in the cooperative solver's plain
 * layout; refused where other solvers would run),
 * "starts_workspace_bytes" (default 1 GiB: device memory the workspace replicas of a multi-start launch may take,
 * rdis_hip_plan_solve_starts, and of a population launch, rdis_hip_plan_solve_population),
 * "population_plain" (default 0; 1 = rdis_hip_plan_solve_population accepts a nonlinear-product plan whose components all
 * run on the plain batch solver, one workgroup per (component, member) working in the member's own x; 0 = such a plan is
 * refused with RDIS_HIP_EINVAL; no effect on bundle-adjustment plans or on any other entry),
 * "population_tiny" (default 0; 1 = rdis_hip_plan_solve_population accepts a bundle-adjustment plan with components on the
 * tiny-component solver, alone or beside components on the LDS-resident solver: a few lanes per (component, member), every
 * member's blocks walking that member's components, rotation records per member; 0 = such a plan is refused with
 * RDIS_HIP_EINVAL; no effect on any other entry -- rdis_hip_plan_solve_starts keeps refusing tiny components),
 * "population_point_major" (default 0; 1 = rdis_hip_plan_solve_population accepts a bundle-adjustment plan with components on
 * the point-major streaming solver, alone or beside components of the two solvers above: one workgroup per (component, member)
 * -- the plan must run one workgroup per component in plan_solve too, "ptm_group" = 1 --, every member of a launch a replica of
 * that solver's point records; 0 = such a plan is refused with RDIS_HIP_EINVAL; no effect on any other entry --
 * rdis_hip_plan_solve_starts keeps refusing point-major components),
 * "tiny_population_fill" (default 1, 1 ... 64: that launch takes this many times the blocks the device holds at once; a
 * measurement aid, no bit depends on it),
 * "trace_records" (per-component trace capacity, 0 = off), "dump_iters" (record p and
 * the search direction at the start of the first k line minimisations, 0 = off). */
int rdis_hip_plan_set_option(rdis_hip_plan *plan, const char *name, int64_t value);
/* which solver the plan's components go to (a test and tuning aid; the partition is computed on demand):
 * "components_cooperative", "components_grid_stream", "components_tiny", "components_lds",
 * "components_point_major", "components_plain" (counts), "pipelined" (0/1: cooperative groups use the
 * pipelined layout), "coop_poll_delay" / "coop_poll_inflight" / "coop_poll_stagger" (the options' values), "point_major_group" (workgroups per component in the last solve's point-major launch), "point_major_threads" (their lanes), "point_major_round_slots" (slots a gradient round staged), "grid_stream_workgroups" (workgroups of the first component on the grid solver),
 * "point_major_wide" (0/1: that launch was a wide group), "point_major_local_cameras" (0, or the most cameras a workgroup of
 * a wide group with local camera numbering holds), "starts_per_launch" / "starts_launches" (starts a launch of the last multi-start
 * solve held; its number of launches), "population_tiny_blocks" (blocks per member of the tiny-component solver's launch in the
 * last population solve, 0 = it had none), "population_point_major_threads" (lanes of the point-major kernel's workgroups in
 * the last population solve, 0 = it had none), "population_cooperative_workgroups" / "population_cooperative_cap" (of the last
 * population solve: the most workgroups a member of a cooperative launch; the resident workgroups such a launch may have over all
 * its members -- 0, 0: it had no cooperative launch) */
int rdis_hip_plan_get_info(rdis_hip_plan *plan, const char *name, int64_t *value);
/* device memory the plan holds beyond the problem's (index tables, workspace, per-factor
 * partials, results): what a host-side cache of plans budgets with
 * (rdis::HipCGDSubspaceOptimizer::setPlanCacheBytes).  The solvers' tables are built on demand: the call builds
 * them if they do not exist yet (it may return RDIS_HIP_ENOMEM); what the first solve adds for the launch shape
 * it picks shows in a query after that solve. */
int rdis_hip_plan_device_bytes(rdis_hip_plan *plan, int64_t *bytes);
/* device time of the solver kernel(s) of the last plan_solve, measured with HIP
 * events on the launch stream; launches = number of kernel launches it covers */
int rdis_hip_plan_last_kernel_ms(rdis_hip_plan *plan, double *ms, int32_t *launches);
/* solver trace of component c of the last solve (trace_records > 0): up to cap
 * records of 4 doubles {tag, a, b, c}; *nrec = records written by the device */
int rdis_hip_plan_get_trace(rdis_hip_plan *plan, int64_t comp, double *rec4, int64_t cap,
                            int64_t *nrec);

/* 48 shader-cycle accumulators of the last cooperative solve, as seen by lane 0 of
 * workgroup 0: {factor arithmetic, workgroup reduce, publish, granule sweep, tail,
 * #exchanges, #sweeps, whole kernel, control step, request hand-over, combine, release,
 * [12..20] cycles per request kind, [22..30] requests per kind; the pipelined solver's
 * collector, by kind of sweep (one that waited for its own lanes / one that did not):
 * [32, 35] polls, [33, 36] polling cycles, [34, 37] completed sweeps; [38..41] sweeps that
 * took 1, 2, 3, 4 or more polls; [42] cycles from a poll's issue to its return, [43] polls
 * so timed}.  THE BUFFER SIZE CHANGED: the call writes 48 values (it wrote 32 before the collector's
 * counters were added), so a caller built against the earlier header must enlarge its buffer.  All zero unless the
 * library was built with -DRDIS_COOP_TIMING (profiling aid) */
int rdis_hip_plan_debug_counters(rdis_hip_plan *plan, int64_t *out48);
/* p and search direction at the start of each of the first dump_iters line
 * minimisations of component c: out[dump_iters][2][nfree_c] (dump_iters > 0) */
int rdis_hip_plan_get_vectors(rdis_hip_plan *plan, int64_t comp, double *out, int64_t cap_doubles);

#ifdef __cplusplus
}
#endif
#endif /* RDIS_HIP_H_ */
